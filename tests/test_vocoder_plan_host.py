"""The schedule of the vocoder's stages (vits.cpp_amd/csrc/vocoder_plan.cpp: which kernel every resblock runs on, and whether a stage's resblocks chain, run side
by side or go out grouped) against its frozen table, on the CPU.

tests/vocoder_plan_dump.cpp links vocoder_plan.o, conv_plan.o and launch_plan.o ALONE (that the link succeeds is the proof that the schedule needs no device),
walks a fixed sweep of stages x batches x lengths x arithmetic modes x knob sets and prints one line per case; the output must equal
tests/golden/vocoder_plan_table.txt byte for byte. The table was recorded from the code BEFORE the planner existed: the decision blocks of run_vocoder_window16,
run_vocoder_window32 and Engine::rb32_kind, copied verbatim into a throwaway host shim (not committed) that printed instead of launching, the `aligned` axis as
the real pointer test on a buffer four bytes off and the 16-bit lat3 answer by the dry run of the launch builders that the planner now answers from shape. So
the table pins which schedule a shape gets, and its last column that Engine::plan_tile_maps plans lists for the kernels rb32_kind named. The dump program also
checks every fused kernel a plan names against that kernel's own *_supported predicate and fails on a miss. The second test checks the table itself: it cannot
pass by being thin. The third runs the same sources as a stand-alone AddressSanitizer + UBSan program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vits.cpp_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "vocoder_plan_table.txt")
F32, F16, BF16, SPLIT = 0, 1, 2, 3


def build(target):
    subprocess.check_call(["make", "-s", "-C", CSRC, target])
    return os.path.join(CSRC, target)


def test_table_is_the_recorded_one():
    out = subprocess.run([build("vocoder_plan_dump")], check=True, capture_output=True).stdout
    want = open(GOLDEN, "rb").read()
    if out != want:
        a, b = out.decode().splitlines(), want.decode().splitlines()
        diff = [(i + 1, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y][:10]
        raise AssertionError("vocoder_plan_dump differs from the golden table (%d lines against %d); first differing lines (got, want):\n%s"
                             % (len(a), len(b), "\n".join("%d: %s\n   %s" % d for d in diff)))


def table():
    """{knob set: {(stage, (arith, planes, prof, aligned)): {(B, frames): [fields ...]}}}, as printed"""
    sets, cur, ctx = {}, None, None
    for line in open(GOLDEN).read().splitlines():
        if line.startswith("## "):
            cur = sets.setdefault(line[3:], {})
        elif line.startswith("@ "):
            f = line.split()
            ctx = cur.setdefault((f[1], tuple(int(x) for x in f[2:])), {})
        elif not line.startswith("#"):
            key, fields = line.split(" : ")
            ctx[tuple(int(x) for x in key.split())] = fields.split()
    return sets


def parent(ctx):
    """the context whose lines stand for this one's where they are equal (vocoder_plan_dump.cpp's parent())"""
    arith, planes, prof, aligned = ctx
    if arith == BF16:
        return (F16, planes, prof, aligned)
    if arith == SPLIT:
        return (F32, 1, prof, aligned)
    if not planes:
        return (arith, 1, prof, aligned)
    if not aligned:
        return (arith, planes, prof, 1)
    if prof:
        return (arith, planes, 0, aligned)
    return None


def lookup(T, knobs, stage, ctx, case):
    """the fields of a case, printed or not (the tile lists' column only where printed)"""
    got = T[knobs].get((stage, ctx), {}).get(case)
    if got is not None:
        return got
    if knobs != "default":
        return lookup(T, "default", stage, ctx, case)
    assert parent(ctx) is not None, (stage, ctx, case)
    return lookup(T, knobs, stage, parent(ctx), case)[:2]


def test_the_table_covers_the_schedule():
    T = table()
    assert os.path.getsize(GOLDEN) < 150 * 1024
    names = list(T)
    assert len(names) == 38 and names[0] == "default"
    # every knob set moves at least one case, and each of the sets the GPU tests run is there
    for s in names:
        assert any(T[s][k] for k in T[s]), "knob set %s changes no case" % s
    for s in ("rb_streams=1", "rb_group_always", "no_rbblock16", "no_fuse16", "no_fuse32", "no_rbblock32", "no_rb_sum3", "no_rb_sum3_f32", "rb16_serial_min_frames=1000000",
              "lrelu_copy_minc=1000", "no_lat16h", "no_rbb_group3"):
        assert s in names, s
    # every boolean field and every per-resblock kernel both ways, per layout (a 16-bit line has six flags, an fp32 line five, conv_pre's one)
    flags, kernels = {6: [set() for _ in range(6)], 5: [set() for _ in range(5)]}, {6: set(), 5: set()}
    pre = set()
    for s in names:
        for (stage, ctx), cases in T[s].items():
            for f in cases.values():
                if stage == "pre":
                    pre.add(f[0])
                    continue
                kernels[len(f[1])] |= set(f[0])
                for i, ch in enumerate(f[1]):
                    flags[len(f[1])][i].add(ch)
    assert pre == {"0", "1"} and all(v == {"0", "1"} for n in flags for v in flags[n]), (pre, flags)
    assert kernels[6] == {"0", "2", "3"} and kernels[5] == {"0", "1", "2", "3"}, kernels  # (the split convs exist in the fp32 layout only)
    d16, d32 = (F16, 1, 0, 1), (F32, 1, 0, 1)
    every = [f for s in names for k, cases in T[s].items() if k[0] != "pre" for f in cases.values()]
    assert any(len(f[1]) == 6 and f[1][4] == "1" for f in every), "group3"
    assert any(len(f[1]) == 6 and f[1][5] == "1" for f in every), "lat3"
    assert any(len(f[1]) == 5 and f[1][1] == "1" for f in every), "grouped"

    # the thresholds from both sides: a case and its neighbour (one more frame, or one more utterance) that plan differently
    def flips(stage, ctx, a, b, knobs="default", field=None):
        x, y = lookup(T, knobs, stage, ctx, a), lookup(T, knobs, stage, ctx, b)
        return x[:2] != y[:2] if field is None else field(x) != field(y)
    for stage in ("c256", "c128", "c64", "c32"):
        assert flips(stage, d16, (1, 599), (1, 600)) and flips(stage, d16, (2, 299), (2, 300)), "rb16_serial_min_frames at " + stage
        assert flips(stage, d16, (1, 1300), (1, 1301)), "rb16_serial_max_frames at " + stage
        assert flips(stage, d32, (1, 1999), (1, 2000)) and flips(stage, d32, (3, 666), (3, 667)), "rb32_sum3_max_frames at " + stage
    kern = lambda f: f[0]
    assert flips("c256", d16, (1, 1024), (1, 1025), field=kern) and flips("c256", d16, (4, 256), (5, 256), field=kern), "conv16_lat's 2048 tiles at C = 256"
    assert not flips("c128", d16, (1, 512), (1, 513)) and flips("c128", d16, (1, 512), (1, 513), "lat16h_max_tiles_c128=4096", kern), "conv16_lat's tiles at C = 128"
    assert flips("pre", d16, (1, 4096), (1, 4097)) and flips("pre", d16, (4, 1024), (5, 1024)), "conv_pre's 2048 tiles"
    group3 = lambda f: f[1][4]
    wide = "rb16_serial_min_frames=1000000"
    assert flips("c32", d16, (1, 2208), (1, 2209), wide, group3) and flips("c64", d16, (64, 69), (64, 70), wide, group3), "the grouped launch's 3072 blocks"
    assert lookup(T, wide, "c32", d16, (1, 2208))[1][4] == "1"
    grouped = lambda f: f[1][1]
    prof32 = (F32, 1, 1, 1)  # (small grids step down from the 128 x 128 tile and are not grouped: one more utterance brings the C = 128 stage onto it)
    assert flips("c128", prof32, (3, 290), (4, 290), field=grouped) and grouped(lookup(T, "default", "c128", prof32, (4, 290))) == "1", "grouped: the 128 x 128 tile"
    assert grouped(lookup(T, "default", "c256", prof32, (64, 290))) == "1" and grouped(lookup(T, "default", "c256", prof32, (1, 290))) == "0"

    # Every exact-fp32 case: the kernels Engine::plan_tile_maps plans lists for are the ones the stage plan names. plan_tile_maps runs before the call's buffers
    # are laid out and plans for aligned ones, which is what the arena gives; the lines of the unaligned guard (aligned 0) show the fused kernels it rules out.
    n = guard = 0
    for s in names:
        for (stage, ctx), cases in T[s].items():
            for f in cases.values():
                if ctx[0] == F32 and len(f) == 3 and len(f[1]) == 5:  # (under no_group16 the 16-bit modes take this layout too: no lists there)
                    if ctx[3]:
                        assert f[2] == f[0], (s, stage, ctx, f)
                        n += 1
                    else:
                        guard += f[2] != f[0]
    assert n > 500 and guard > 50, (n, guard)
    # what the fused kernels refuse: a stage of one and of two resblocks, another dilation list, k = 5, a conv without bias / 16-bit weights / fp32 weights / split planes
    D = T["default"]
    assert {k[0] for k in D} >= {"c64.nk1", "c64.nk2", "c256.nk2", "c32.nk4", "c64.dil132", "c256.dil13", "c64.k5", "c128.k5", "c32.nobias", "c128.nobias", "c32.nowp16",
                                 "c256.nowp16", "c64.nowp", "c128.nowps", "c256.nowps"}
    assert lookup(T, "default", "c32", d16, (1, 290))[0] == "333" and lookup(T, "default", "c32.nobias", d16, (1, 290))[0] == "033"
    assert lookup(T, "default", "c32.nowp16", d16, (1, 290))[0] == "323" and lookup(T, "default", "c64.dil132", d16, (64, 290))[0][1] != "3"
    assert lookup(T, "default", "c64", d32, (1, 290))[0] == "322" and lookup(T, "default", "c64.nowp", d32, (1, 290))[0] == "222"
    assert lookup(T, "default", "c128", (SPLIT, 1, 0, 1), (1, 290))[0] == "111" and lookup(T, "default", "c128.nowps", (SPLIT, 1, 0, 1), (1, 290))[0] == "101"
    assert lookup(T, "default", "c128", (SPLIT, 0, 0, 1), (1, 290))[0] == lookup(T, "default", "c128", d32, (1, 290))[0] == "200"


def test_planner_under_the_sanitizers():
    """the same sweep through the AddressSanitizer + UBSan build of the same sources (a stand-alone program): the same table, clean exit"""
    asan = build("_asan/vocoder_plan_dump")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")
    got = subprocess.run([asan], capture_output=True, env=env)
    assert got.returncode == 0, got.stderr[-2000:]
    assert got.stdout == open(GOLDEN, "rb").read()
