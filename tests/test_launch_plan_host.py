"""The fused kernels' launch policy (vocoder resblocks and upsamplers, flow, attention / LayerNorm / DDS) (vits.cpp_amd/csrc/launch_plan.cpp) against its frozen table, on the CPU.

tests/launch_plan_dump.cpp links launch_plan.o ALONE (that the link succeeds is the proof that the policy needs no device), walks a fixed sweep of
shapes x grids x knob sets and prints one line per case; the output must equal tests/golden/launch_plan_table.txt byte for byte. The table was
recorded from the code BEFORE the planner covered these families (a throwaway shim beside the old launch functions that printed, instead of
launching, the kernel instantiation, grid, block and LDS bytes of every launch), so it pins which instantiation runs on which grid. The dump
program also checks every launchable plan against the launchers' own existence predicates and fails on a miss. The second test checks the table
itself: it cannot pass by being thin."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vits.cpp_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_plan_table.txt")


def test_plan_table_is_the_recorded_one():
    subprocess.check_call(["make", "-s", "-C", CSRC, "launch_plan_dump"])
    out = subprocess.run([os.path.join(CSRC, "launch_plan_dump")], check=True, capture_output=True).stdout
    want = open(GOLDEN, "rb").read()
    if out != want:
        a, b = out.decode().splitlines(), want.decode().splitlines()
        diff = [(i + 1, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y][:10]
        raise AssertionError("launch_plan_dump differs from the golden table (%d lines against %d); first differing lines (got, want):\n%s"
                             % (len(a), len(b), "\n".join("%d: %s\n   %s" % d for d in diff)))


def rows():
    """(knob set, family, case ints, fields) per case line of the golden table"""
    knobs = None
    for line in open(GOLDEN).read().splitlines():
        if line.startswith("## "):
            knobs = line[3:]
        elif not line.startswith("#"):
            key, fields = line.split(" : ", 1)
            yield knobs, key.split()[0], [int(x) for x in key.split()[1:]], fields


def test_the_table_covers_the_policy():
    R = list(rows())
    assert os.path.getsize(GOLDEN) < 150 * 1024
    # every knob set moves at least one case
    sets = [line[3:] for line in open(GOLDEN).read().splitlines() if line.startswith("## ")]
    assert len(sets) == 29 and sets[0] == "default"
    for s in sets:
        assert any(kn == s for kn, *_ in R), "knob set %s changes no case" % s
    # every instantiation arm of every dispatcher (operand type apart: the table is recorded for f16)
    kernels = set(re.findall(r"\w+_kernel<[^>]*>", "\n".join(f for *_, f in R)))
    want = {"rbblock16_group3_kernel<32, false>", "rbblock16_group3_kernel<64, false>", "rbblock32_kernel<32, 2>", "rbblock32_kernel<64, 4>", "wavenet32_kernel<192, 5>",
            "wavenet16_kernel<192, 5, false, 1>", "wavenet16_kernel<192, 5, false, 2>", "convt16_lines_kernel<64, false>", "convt16_lines_kernel<128, false>"}
    want |= {"flow_couple16_kernel<false, %d, %d>" % a for a in ((1, 1), (1, 2), (2, 2))}
    want |= {"rel_attention_mfma_kernel<%s>" % a for a in ("8, 24, false, true", "4, 24, true, false", "4, 32, false, false", "8, 32, false, false")}
    want |= {"rel_attention_kernel<1024>", "rel_attention_kernel<256>", "add_layer_norm_kernel<32>", "add_layer_norm_kernel<64>", "dds_layer_lat_kernel<0, 0, 6>", "dds_layer_lat_kernel<0, 0, 8>"}
    want |= {"dds_layer_kernel<0, %d>" % m for m in (2, 4, 6, 8)}
    want |= {"convt16_kernel<%d, %d, %d, false>" % (nr, cs, rs) for nr, cs in ((4, 2), (2, 1), (4, 1)) for rs in (8, 16)}
    for k in (3, 7, 11):
        for d in (1, 3, 5):
            want |= {"rbpair16_kernel<%d, %d, %d, 2, false, false>" % (k, d, C) for C in (32, 64)}
            want |= {"rbpair16_kernel<%d, %d, %d, %d, false, true>" % (k, d, C, nr) for C in (128, 256) for nr in (2, 4)}
            want |= {"rbpair32_kernel<%d, %d, %d>" % (k, d, C) for C in (32, 64, 128) if C < 128 or k == 3}
        for stream in ("false", "true"):
            want |= {"rbblock16_kernel<%d, 32, 4, 3, 1, 1, 3, 5, false, %s>" % (k, stream), "rbblock16_kernel<%d, 64, %s, 1, 1, 3, 5, false, %s>" % (k, "4, 3" if k == 11 else "2, 4", stream)}
            if k == 3:
                want.add("rbblock16_kernel<3, 128, 4, 2, 2, 1, 3, 5, false, %s>" % stream)
    assert kernels == want, (sorted(want - kernels), sorted(kernels - want))
    # segments of 2 ... cap tiles for the three shapes that take them by default (6, 3, 4), one tile everywhere else
    nt = {}
    for kn, fam, case, f in R:
        if fam == "B16" and kn == "default" and " nt " in f:
            nt.setdefault((case[0], case[1]), set()).add(int(f.split(" nt ")[1].split()[0]))
    assert nt[(32, 11)] == set(range(1, 7)) and nt[(64, 7)] == {1, 2, 3} and nt[(64, 11)] == {2, 3, 4} and nt[(32, 3)] == {1} and nt[(128, 3)] == {1}, nt
    # every *_supported answers both ways (the leading digits of a line; WN / FC: the shape part, which is the plan's ok)
    bits = {}
    for kn, fam, case, f in R:
        for i, ch in enumerate(f.split()[0]):
            bits.setdefault((fam, i), set()).add(ch)
    for fam, n in (("P16", 1), ("B16", 3), ("G3", 2), ("P32", 1), ("B32", 2), ("CT", 2), ("WN", 1), ("FC", 1), ("AT", 1), ("LN", 1), ("DW", 1), ("DL", 1), ("DT", 1)):
        for i in range(n):
            if (fam, i) in (("B16", 1), ("B16", 2), ("G3", 1), ("B32", 1), ("CT", 1)):  # (other dilations / kernel sizes, no 16-bit weights: never supported)
                assert bits[(fam, i)] == {"0"}, (fam, i)
            else:
                assert bits[(fam, i)] == {"0", "1"}, (fam, i)
    # the thresholds from both sides: a case and its neighbour (one more column) that plan differently
    by_key = {(fam, tuple(case)): f for kn, fam, case, f in R if kn == "default"}

    def flips(fam, case, field):
        a, b = by_key[(fam, tuple(case))], by_key[(fam, tuple(case[:-2]) + (case[-2] + 1, case[-1]))]
        return field(a) != field(b)
    kernel = lambda f: re.search(r"\w+_kernel<[^>]*>", f).group(0)
    assert flips("P16", [256, 11, 3, 128 * 118, 1], kernel) and flips("P16", [128, 3, 3, 16 * 126, 8], kernel), "rb16_narrow_max"
    assert flips("G3", [32, 3072 * 184, 1], lambda f: f.split()[1]) and flips("G3", [64, 48 * 184, 64], lambda f: f.split()[1]), "the grouped launch's 3072 blocks"
    assert flips("FC", [192, 96, 5, 1, 4, 96 * 48, 1], kernel) and flips("FC", [192, 96, 5, 1, 4, 24 * 48, 4], kernel), "flow_narrow_max"
    gz = lambda f: f.split(" | ")[1].split()[2]
    assert by_key[("CT", (256, 128, 8, 64 * 128 - 1, 1))] != by_key[("CT", (256, 128, 8, 64 * 128, 1))] and gz(by_key[("CT", (256, 128, 8, 64 * 128 - 1, 1))]) == "4", "convt16_split_max"
    assert gz(by_key[("CT", (512, 256, 8, 64 * 64 - 1, 1))]) == "4" and gz(by_key[("CT", (512, 256, 8, 64 * 64, 1))]) == "1", "convt16_split_max at c_in = 512"
    assert flips("AT", [2, 96, 4, 512, 8], kernel) and flips("AT", [2, 64, 4, 512, 8], kernel), "attention's short variant up to 512 tokens"
    assert flips("AT", [1, 64, 4, 2048, 1], kernel) and flips("AT", [2, 96, 4, 256, 4], kernel), "attention's latency variant up to 128 blocks"
    assert flips("AT", [2, 24, 4, 256, 16], kernel), "the VALU attention kernel's block size at 512 blocks"
    assert {f.split("vshift ")[1] for kn, fam, _, f in R if fam == "AT" and "vshift" in f} >= {"6", "5"}, "the vshift search"
    assert any(fam == "AT" and case[1] == 144 and f == "0 -" for _, fam, case, f in R), "the attention launch that is refused"
    lds = lambda f: int(f.split(" | ")[1].split()[4])
    at = {tuple(case): f for kn, fam, case, f in R if kn == "default" and fam == "AT" and "mfma" in f}
    assert any(2 * lds(f) <= 160 * 1024 for f in at.values()) and any(2 * lds(f) > 160 * 1024 for f in at.values()), "four and eight waves by LDS footprint"
    ln = {kn: {case[0] for k2, fam, case, f in R if fam == "LN" and k2 == kn and f != "0 -"} for kn in ("default", "ln_tw=64")}
    assert 1168 in ln["default"] and 1169 not in ln["default"] and 568 in ln["ln_tw=64"] and 569 not in ln["ln_tw=64"], "LayerNorm's 150 KB refusal, both tile widths"
    assert flips("DT", [192, 3, 1, 1536, 1], lambda f: f.split()[1]) and flips("DT", [192, 3, 9, 256, 6], lambda f: f.split()[1]), "dds_lat_max_blocks"
    # a refused launch where the predicate says yes: the developer override that names no instantiation
    assert any(kn == "convt16_r128=311" and f.startswith("10 0 S3.1.") for kn, fam, _, f in R if fam == "CT")
