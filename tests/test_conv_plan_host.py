"""The convolutions' launch policy (vits.cpp_amd/csrc/conv_plan.cpp) against its frozen table, on the CPU.

tests/conv_plan_dump.cpp links conv_plan.o ALONE (that the link succeeds is the proof that the policy needs no device), walks a fixed sweep of
layers x lengths x batches x knob sets and prints one line per case; the output must equal tests/golden/conv_plan_table.txt byte for byte. The table
was recorded from the code BEFORE the planner existed (a throwaway shim printing the same fields next to the old launch functions), so it pins which
instantiation runs with which grid, LDS size, ring depth and one-shot fill. The dump program also checks every launchable plan against the launchers' own
existence predicates and fails on a miss. The second test checks the table itself: it cannot pass by being thin."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vits.cpp_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_plan_table.txt")


def test_plan_table_is_the_recorded_one():
    subprocess.check_call(["make", "-s", "-C", CSRC, "conv_plan_dump"])
    out = subprocess.run([os.path.join(CSRC, "conv_plan_dump")], check=True, capture_output=True).stdout
    want = open(GOLDEN, "rb").read()
    if out != want:
        a, b = out.decode().splitlines(), want.decode().splitlines()
        diff = [(i + 1, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y][:10]
        raise AssertionError("conv_plan_dump differs from the golden table (%d lines against %d); first differing lines (got, want):\n%s"
                             % (len(a), len(b), "\n".join("%d: %s\n   %s" % d for d in diff)))


def rows():
    """(knob set, layer = (epi, k, cin, cout, stride, dil), kind, key ints, field ints / strings) per case line of the golden table"""
    knobs, layer = None, None
    for line in open(GOLDEN).read().splitlines():
        if line.startswith("## "):
            knobs = line[3:]
        elif line.startswith("@ "):
            layer = tuple(int(x) for x in line.split()[1:])
        elif not line.startswith("#"):
            key, fields = line.split(" : ")
            yield knobs, layer, key[0], [int(x) for x in key.split()[1:]], fields.replace("|", " ").split()


def test_the_table_covers_the_policy():
    R = list(rows())
    assert os.path.getsize(GOLDEN) < 150 * 1024
    F = [(kn, l, k, [int(x) for x in f[:16]], f[16]) for kn, l, kind, k, f in R if kind == "F"]
    G = [(kn, l, k, [int(x) for x in f[:15]], f[15], f[16:]) for kn, l, kind, k, f in R if kind == "G"]
    # F: ok tile dil dil_ct db gx gy gz block lds xw lds_off nbuf oneshot pitch ln_ok {bits}
    assert {f[1] for _, _, _, f, _ in F} == set(range(7)), "every ConvTile"
    lat16 = [l for _, l, _, f, _ in F if f[1] == 6]
    assert any(l[0] == 1 or l[1] == 1 for l in lat16), "TILE_LAT16 by the tiny-grid rule (gated / 1x1 convs cannot take the unfilled-SIMD rule)"
    assert any(l[0] == 0 and (l[1] >= 5 or l[5] > 1) for l in lat16), "TILE_LAT16 by the unfilled-SIMD rule (no narrow tile for these taps)"
    assert {2, 3} <= {f[12] for _, _, _, f, _ in F}, "ring depths 2 and 3"
    assert any(f[13] == 1 and f[12] == (l[2] + 31) // 32 and f[12] > 3 for _, l, _, f, _ in F), "one-shot fill: one buffer per chunk"
    assert {f[4] for _, _, _, f, _ in F} == {0, 1}, "producer-wave variant and register-staged variant"
    assert {f[3] != 0 for _, _, _, f, _ in F} == {False, True}, "compile-time and run-time dilation"
    assert any(f[15] for _, _, _, f, _ in F) and not all(f[15] for _, _, _, f, _ in F), "LayerNorm on load"
    for bit, what in enumerate(["conv_group_supported", "conv_split_supported", "conv_split_candidate", "conv_lat16_candidate"]):
        assert {b[bit] for _, _, _, _, b in F} == {"0", "1"}, what
    # G: ok lat epi16 chosen tile part dil dil_ct gx gy gz lds xwp lds_off nbuf {bits} | wm nr pitch gx gy gz block lds
    assert {g[4] for _, _, _, g, _, _ in G} == set(range(8)), "conv16 tiles 0 to 6 and the conv16_lat route"
    assert any(g[3] in (0, 5, 6) and g[4] == 1 for _, _, _, g, _, _ in G), "first fallback step: no 128-row tile for this epilogue / dilation"
    assert any(g[3] == 2 and g[4] == 4 for _, _, _, g, _, _ in G), "second fallback step: 32 x 256 only in the group layout"
    assert {g[2] for _, _, _, g, _, _ in G} == set(range(5)), "every conv16 epilogue"
    assert {g[5] for _, _, _, g, _, _ in G} == set(range(4)), "every dispatcher"
    for bit, what in enumerate(["conv16_lat_shape_ok", "conv16_lat_wanted"]):
        assert {b[bit] for _, _, _, _, b, _ in G} == {"0", "1"}, what
    assert {(int(l[0]), int(l[1])) for _, _, _, g, _, l in G if g[1]} == {(2, 1), (2, 2), (4, 2)}, "conv16_lat block shapes"
    L = [f for _, _, kind, _, f in R if kind == "L"]
    P = [f for _, _, kind, _, f in R if kind == "P"]
    assert {(int(f[1]), int(f[2])) for f in L if f[0] == "1"} == {(2, 1), (4, 1), (2, 2), (4, 2)}, "grouped conv16_lat block shapes"
    assert {f[0] for f in L} == {"0", "1"} and {f[0] for f in P} == {"0", "1"}, "conv16_lat_group_wanted / conv16_lat_pre_wanted both ways"
    # every knob set moves at least one case
    sets = [line[3:] for line in open(GOLDEN).read().splitlines() if line.startswith("## ")]
    assert len(sets) == 22 and sets[0] == "default"
    for s in sets:
        assert any(kn == s for kn, *_ in R), "knob set %s changes no case" % s
    # The planner never asks for an instantiation the launcher lacks. conv_plan_dump evaluates conv_tile_exists / conv_lat16_exists / conv16_tile_exists /
    # conv16_lat_shape_exists itself on every plan marked launchable and exits non-zero on a miss (test_plan_table_is_the_recorded_one runs it). The plans marked
    # refused are the two known kinds, refused before the planner existed too: VITS_DB_MIN=2 has no narrow tile (producer-wave only) for the single-chunk inputs it
    # moves to the register-staged kernels, and a standard conv with 2 taps has no tile kernel at all (conv_lat16_kernel runs it on tiny grids: those rows are launchable)
    # (On a refused row only ok, tile and the fields up to the refusal are behaviour: the old launch code returned before it computed a grid, a block size or
    # LDS bytes, so those columns of a refused row are the dump's formula, not something a launch ever used.)
    for kn, l, k, f, _ in F:
        assert f[0] == 1 or (kn == "db_min=2" and f[1] == 5 and f[4] == 0 and l[2] <= 32) or (l[:2] == (0, 2) and f[3] == -99 and f[1] != 6), (kn, l, k, f)
    assert any(l[:2] == (0, 2) and f[0] == 1 and f[1] == 6 for _, l, _, f, _ in F), "the 2-tap standard conv on conv_lat16_kernel"
    assert all(g[0] == 1 for _, _, _, g, _, _ in G)
