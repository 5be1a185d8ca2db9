"""The delivery planner (vits.cpp_amd/csrc/delivery_plan.cpp: which stage behind the vocoder reads and writes which buffer, what is delivered, which arena
buffers a call needs, which combinations are refused) against its frozen table, on the CPU.

tests/delivery_plan_dump.cpp links delivery_plan.o ALONE (that the link succeeds is the proof that the planner needs no device), walks every combination
of the ask and prints one line per case; the output must equal tests/golden/delivery_plan_table.txt byte for byte. The table was recorded from the code
BEFORE the planner existed, not from the planner: a throwaway stand-alone shim evaluated the engine's own expressions of that time for every case — the
nested conditionals of run_stage_two that chose the destination and stride of the vocoder, the edges stage, levelling and the resampler and the resampler's
source, the allocation conditions of layout_stage_two, what run_edges and run_level read, and the refusal conditions of check_level and check_edges — with
every pointer replaced by the name of its buffer, and printed them in the dump's format (E_stride named S_stride where the edges stage is off: the two were
the same number there). The second test checks the table itself: it cannot pass by being thin. The dump also runs as a stand-alone program under
AddressSanitizer + UBSan."""
import itertools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vits.cpp_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "delivery_plan_table.txt")
STAGES = ("vocoder", "edges", "level", "resample")
LEVELS = ("none", "measure", "gain", "whole")
ARENA = {"EDGE": "wave_edge", "LVL": "wave_lvl", "OUT": "wave_out"}
STRIDE_OF = {"NONE": {"-"}, "WAVE": {"S_stride"}, "EDGE": {"E_stride"}, "LVL": {"S_stride", "E_stride"}, "OUT": {"out_ws"}, "CALLER": {"caller"}}


def build(target):
    subprocess.check_call(["make", "-s", "-C", CSRC, target])
    return os.path.join(CSRC, target)


def test_plan_table_is_the_recorded_one():
    out = subprocess.run([build("delivery_plan_dump"), "base"], check=True, capture_output=True).stdout
    want = open(GOLDEN, "rb").read()
    if out != want:
        a, b = out.decode().splitlines(), want.decode().splitlines()
        diff = [(i + 1, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y][:10]
        raise AssertionError("delivery_plan_dump differs from the golden table (%d lines against %d); first differing lines (got, want):\n%s"
                             % (len(a), len(b), "\n".join("%d: %s\n   %s" % d for d in diff)))
    # the same program under the sanitizers: same output, clean exit
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")
    got = subprocess.run([build("_asan/delivery_plan_dump"), "base"], capture_output=True, env=env)
    assert got.returncode == 0, got.stderr[-2000:]
    assert got.stdout == want


def rows():
    """(ask dict, refusal or None, {stage: (src, dst) or None}, delivered, needs) per line of the golden table; a route is (buffer, stride kind)"""
    for line in open(GOLDEN).read().splitlines():
        key, fields = line.split(" : ", 1)
        ask = dict(kv.split("=") for kv in key.split())
        if fields.startswith("refuse "):
            yield ask, fields.split()[1], None, None, None
            continue
        parts = fields.split(" | ")
        assert len(parts) == 6 and [p.split()[0] for p in parts] == list(STAGES) + ["deliver", "needs"], line
        route = lambda r: tuple(r.split("/"))
        stages = {}
        for name, p in zip(STAGES, parts):
            what = p.split()[1]
            stages[name] = None if what == "off" else tuple(route(r) for r in what.split(">"))
        needs = parts[5].split()[1]
        yield ask, None, stages, route(parts[4].split()[1]), set() if needs == "-" else set(needs.split(","))


def test_the_table_covers_the_policy():
    R = list(rows())
    assert os.path.getsize(GOLDEN) < 64 * 1024
    # every combination of the ask, exactly once
    keys = [tuple(a[k] for k in ("edges", "level", "limiter", "rate", "out_device", "on_chunk", "async")) for a, *_ in R]
    want = [(e, lv) + rest for e in "01" for lv in LEVELS for rest in itertools.product("01", repeat=5)]
    assert keys == want and len(set(keys)) == len(keys) == 256
    # every refusal kind; a call that neither streams nor returns early is never refused
    assert {r for _, r, *_ in R if r} == {"limit_stream", "level_stream", "edges_stream", "edges_async"}
    assert all(r is None for a, r, *_ in R if a["on_chunk"] == "0" and a["async"] == "0")
    bufs, strides, needs_seen = set(), set(), set()
    for ask, refusal, stages, delivered, needs in R:
        if refusal:
            continue
        od = ask["out_device"] == "1"
        # who runs
        assert stages["vocoder"] is not None
        assert (stages["edges"] is not None) == (ask["edges"] == "1") and (stages["level"] is not None) == (ask["level"] != "none")
        assert (stages["resample"] is not None) == (ask["rate"] == "1")
        # a chain: the vocoder reads nothing; every other running stage reads what the last stage that wrote left; a level that only measures writes nothing
        cur = ("NONE", "-")
        writers = []
        for name in STAGES:
            if stages[name] is None:
                continue
            src, dst = stages[name]
            assert src == cur, (ask, name)
            if name == "level" and ask["level"] == "measure":
                assert dst == ("NONE", "-"), ask
                continue
            assert dst[0] not in ("NONE", "WAVE") or name == "vocoder", (ask, name)
            writers.append((name, dst))
            cur = dst
        assert delivered == cur, ask
        # the caller's buffer: written by the last stage that writes, exactly when the call gives one; read only by a level that measures it there
        for name, dst in writers:
            assert (dst[0] == "CALLER") == (od and name == writers[-1][0]), (ask, name)
        # every buffer has its one stride kind (the levelled rows follow their input's: E_stride exactly when the edges stage is on)
        named = [r for st in stages.values() if st for r in st]
        for buf, stride in named:
            assert stride in STRIDE_OF[buf], (ask, buf, stride)
            if buf == "LVL":
                assert stride == ("E_stride" if ask["edges"] == "1" else "S_stride"), ask
        bufs |= {b for b, _ in named}
        strides |= {s for _, s in named}
        # an arena buffer is needed if and only if a stage names it; the scratch and the range tables by what runs
        for buf, need in ARENA.items():
            assert (need in needs) == any(b == buf for b, _ in named), (ask, buf)
        multiplies = ask["level"] in ("gain", "whole")
        assert ("ed_scratch" in needs) == (ask["edges"] == "1") and ("lvl_scratch" in needs) == (ask["level"] != "none")
        assert ("lim_scratch" in needs) == (multiplies and ask["limiter"] == "1")
        assert ("out_ranges" in needs) == (ask["rate"] == "1" and ask["on_chunk"] == "1") and ("lvl_ranges" in needs) == (multiplies and ask["on_chunk"] == "1")
        needs_seen |= needs
    assert bufs == {"NONE", "WAVE", "EDGE", "LVL", "OUT", "CALLER"} and strides == {"-", "S_stride", "E_stride", "out_ws", "caller"}
    assert needs_seen == {"wave_edge", "wave_lvl", "wave_out", "ed_scratch", "lvl_scratch", "lim_scratch", "out_ranges", "lvl_ranges"}
