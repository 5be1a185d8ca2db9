"""The joined half of the delivery planner (vits.cpp_amd/csrc/delivery_plan.cpp with DeliveryAsk::joined: where the join of vits_model_process_joined sits in
the chain, what it reads and writes, what the level and the resampler behind it then work on) against its frozen table, on the CPU.

tests/delivery_plan_dump.cpp (its slice `joined`) links delivery_plan.o ALONE, walks every combination of the ask with joined = true and prints one line per case; the output must
equal tests/golden/joined_plan_table.txt byte for byte. The table was recorded once and read line by line against the rules the second test states; the
test never regenerates it. The unjoined half is tests/test_delivery_plan_host.py's, whose table this change leaves as it was. The dump also runs as a
stand-alone program under AddressSanitizer + UBSan."""
import itertools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vits.cpp_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "joined_plan_table.txt")
STAGES = ("vocoder", "edges", "join", "level", "resample")
LEVELS = ("none", "measure", "gain", "whole")
ARENA = {"EDGE": "wave_edge", "LVL": "wave_lvl", "OUT": "wave_out", "JOIN": "wave_join"}
STRIDE_OF = {"NONE": "-", "WAVE": "S_stride", "EDGE": "E_stride", "JOIN": "J_stride", "LVL": "J_stride", "OUT": "out_ws", "CALLER": "caller"}


def build(target):
    subprocess.check_call(["make", "-s", "-C", CSRC, target])
    return os.path.join(CSRC, target)


def test_joined_plan_table_is_the_recorded_one():
    out = subprocess.run([build("delivery_plan_dump"), "joined"], check=True, capture_output=True).stdout
    want = open(GOLDEN, "rb").read()
    if out != want:
        a, b = out.decode().splitlines(), want.decode().splitlines()
        diff = [(i + 1, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y][:10]
        raise AssertionError("joined_plan_dump differs from the golden table (%d lines against %d); first differing lines (got, want):\n%s"
                             % (len(a), len(b), "\n".join("%d: %s\n   %s" % d for d in diff)))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")
    got = subprocess.run([build("_asan/delivery_plan_dump"), "joined"], capture_output=True, env=env)
    assert got.returncode == 0, got.stderr[-2000:]
    assert got.stdout == want


def rows():
    for line in open(GOLDEN).read().splitlines():
        key, fields = line.split(" : ", 1)
        ask = dict(kv.split("=") for kv in key.split())
        if fields.startswith("refuse "):
            yield ask, fields.split()[1], None, None, None
            continue
        parts = fields.split(" | ")
        assert len(parts) == 7 and [p.split()[0] for p in parts] == list(STAGES) + ["deliver", "needs"], line
        route = lambda r: tuple(r.split("/"))
        stages = {}
        for name, p in zip(STAGES, parts):
            what = p.split()[1]
            stages[name] = None if what == "off" else tuple(route(r) for r in what.split(">"))
        needs = parts[6].split()[1]
        yield ask, None, stages, route(parts[5].split()[1]), set() if needs == "-" else set(needs.split(","))


def test_the_joined_table_covers_the_policy():
    R = list(rows())
    assert os.path.getsize(GOLDEN) < 64 * 1024
    keys = [tuple(a[k] for k in ("edges", "level", "limiter", "rate", "out_device", "on_chunk", "async")) for a, *_ in R]
    want = [(e, lv) + rest for e in "01" for lv in LEVELS for rest in itertools.product("01", repeat=5)]
    assert keys == want and len(set(keys)) == len(keys) == 256
    # a joined call neither streams nor returns early, whatever else is asked; everything else runs
    for ask, refusal, *_ in R:
        assert refusal == ("join_stream" if ask["on_chunk"] == "1" else "join_async" if ask["async"] == "1" else None), ask
    bufs, needs_seen = set(), set()
    for ask, refusal, stages, delivered, needs in R:
        if refusal:
            continue
        od = ask["out_device"] == "1"
        # who runs: the vocoder and the join always
        assert stages["vocoder"] is not None and stages["join"] is not None
        assert (stages["edges"] is not None) == (ask["edges"] == "1") and (stages["level"] is not None) == (ask["level"] != "none")
        assert (stages["resample"] is not None) == (ask["rate"] == "1")
        # a chain in the order vocoder, edges, join, level, resample
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
            writers.append((name, dst))
            cur = dst
        assert delivered == cur, ask
        # the join reads the per-utterance rows (the edges stage's, else the vocoder's): neither of those ever writes to the caller's buffer
        assert stages["vocoder"][1] == ("WAVE", "S_stride")
        assert stages["edges"] is None or stages["edges"][1] == ("EDGE", "E_stride")
        assert stages["join"][0] == (("EDGE", "E_stride") if ask["edges"] == "1" else ("WAVE", "S_stride"))
        for name, dst in writers:
            assert (dst[0] == "CALLER") == (od and name == writers[-1][0]), (ask, name)
        # everything behind the join is track rows: J_stride (the levelled buffer follows its input), the output rate's, or the caller's
        named = [r for st in stages.values() if st for r in st]
        for buf, stride in named:
            assert stride == STRIDE_OF[buf], (ask, buf, stride)
        for name in ("level", "resample"):
            if stages[name]:
                assert stages[name][0][1] in ("J_stride", "caller"), (ask, name)
        bufs |= {b for b, _ in named}
        for buf, need in ARENA.items():
            assert (need in needs) == any(b == buf for b, _ in named), (ask, buf)
        multiplies = ask["level"] in ("gain", "whole")
        assert "join_table" in needs
        assert ("ed_scratch" in needs) == (ask["edges"] == "1") and ("lvl_scratch" in needs) == (ask["level"] != "none")
        assert ("lim_scratch" in needs) == (multiplies and ask["limiter"] == "1")
        assert "out_ranges" not in needs and "lvl_ranges" not in needs
        needs_seen |= needs
    assert bufs == {"NONE", "WAVE", "EDGE", "JOIN", "LVL", "OUT", "CALLER"}
    assert needs_seen == {"wave_edge", "wave_lvl", "wave_out", "wave_join", "join_table", "ed_scratch", "lvl_scratch", "lim_scratch"}
