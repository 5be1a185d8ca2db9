"""The join kernels at operator level (vits_op_join, join.hip) against the numpy restatement (tests/join_ref.py), bit for bit: the half rule's clamps,
zero-length rows wherever they can stand, utterance boundaries, overlaps and pauses on the edges of the kernel's tile, tracks of very different bounds in
one grid, and the independence of a track from the rows around it. x carries NaN behind every n_b and y is NaN before the call: [0, T) matches, [T, bound)
is +0, everything behind the bound is still NaN."""
import numpy as np
import pytest

import join_ref as JR

pytestmark = pytest.mark.gpu

FS = 16000
MS = 1000.0 / FS  # one sample


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def make_rows(lens, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(n).astype(np.float32) for n in lens]


def run(pkg, rows, track=None, gap_ms=None, spare=37):
    """vits_op_join on rows staged with NaN behind each; returns (tracks as delivered [T_g], track_lens, device rows, y whole)"""
    B = len(rows)
    lens = np.array([len(r) for r in rows], np.int32)
    x = np.full((B, max(int(lens.max(initial=0)), 1) + 5), np.nan, np.float32)
    for b, r in enumerate(rows):
        x[b, : len(r)] = r
    G, bounds, tile = pkg.join_plan(FS, lens, track, gap_ms)
    y = np.full((G, max(int(bounds.max()), 1) + spare), np.nan, np.float32)
    y, tl, dev_rows = pkg.join(x, FS, lens=lens, track=track, gap_ms=gap_ms, out=y)
    return y, tl, dev_rows, bounds


def check(pkg, rows, track=None, gap_ms=None):
    want, o, T, bounds = JR.join(rows, FS, track, gap_ms)
    y, tl, dev_rows, got_bounds = run(pkg, rows, track, gap_ms)
    assert np.array_equal(got_bounds, bounds)
    assert np.array_equal(tl, T) and np.array_equal(dev_rows[:, 0], o) and np.array_equal(dev_rows[:, 1], [len(r) for r in rows])
    for g in range(len(want)):
        assert same(y[g, : T[g]], want[g]) and np.isfinite(y[g, : T[g]]).all()
        tail = y[g, T[g]:bounds[g]]
        assert not tail.any() and not np.signbit(tail).any()  # [T, bound) is +0, the sign bit included
        assert np.isnan(y[g, bounds[g]:]).all()  # nothing is written behind the bound
    return [y[g, : T[g]].copy() for g in range(len(want))], o, T


@pytest.fixture(scope="module")
def tile(pkg):
    t = pkg.join_plan(FS, [1])[2]
    assert t == 1024
    return t


GAPS = {"none": 0.0, "plus3": 3 * MS, "minus1": -1 * MS, "minus2000ms": -2000.0}


@pytest.mark.parametrize("gap", sorted(GAPS))
@pytest.mark.parametrize("track", [None, (0, 0, 1, 1, 1)], ids=["one_track", "two_and_three"])
def test_lengths_and_clamps(pkg, gap, track):
    # under -2000 ms the half rule binds everywhere: n = 1 gives nothing (v = 0), n = 3 one sample, 7 against 300 three: the shorter neighbour's half
    for lens in ((0, 1, 3, 7, 300), (300, 7, 3, 1, 0), (3, 300, 1, 7, 7)):
        _, o, T = check(pkg, make_rows(lens, 11), track, GAPS[gap])
        if gap == "minus2000ms" and track is None and lens == (0, 1, 3, 7, 300):
            assert o.tolist() == [0, 0, 1, 3, 7] and T.tolist() == [307]  # steps 0, 0, -1, -3


@pytest.mark.parametrize("gap", sorted(GAPS))
def test_zero_length_rows(pkg, gap):
    g = GAPS[gap]
    for lens in ((0, 40, 9), (40, 0, 9), (40, 9, 0), (40, 0, 0, 9), (0, 0, 40), (0,)):
        check(pkg, make_rows(lens, 12), None, g)
    # a track that is empty altogether between two that are not; T = 0 unless a pause lies in it
    _, o, T = check(pkg, make_rows((40, 0, 0, 9), 13), (0, 1, 1, 2), g)
    assert T.tolist() == [40, max(JR.gap_samples(g, FS), 0), 9]


def test_tile_edges(pkg, tile):
    t = tile
    for first in (t - 1, t, t + 1):  # an utterance boundary at t - 1, t and t + 1
        check(pkg, make_rows((first, 50), 14), None, 0.0)
    # an overlap that straddles the tile edge: 40 samples, 20 on each side
    out, o, T = check(pkg, make_rows((t + 20, 300), 15), None, -40 * MS)
    assert o.tolist() == [0, t - 20]
    # a pause that straddles it
    out, o, T = check(pkg, make_rows((t - 10, 300), 16), None, 25 * MS)
    assert o.tolist() == [0, t + 15] and not out[0][t - 10: t + 15].any()
    # a single row of 2 t + 1 samples: a pure copy through three tiles, the last of one sample
    rows = make_rows((2 * t + 1,), 17)
    out, o, T = check(pkg, rows)
    assert same(out[0], rows[0])
    # many short utterances inside one tile, and overlaps on every tile edge of a longer track
    check(pkg, make_rows((5,) * 40 + (t,) * 3 + (1, 0, 2), 18), None, -3 * MS)


def test_three_tracks_of_very_different_bounds(pkg, tile):
    # the grid is sized by the largest bound: the blocks of the short tracks behind their bound write nothing
    lens = (3, 5 * tile + 7, 100, 2, 1, 900)
    out, o, T = check(pkg, make_rows(lens, 19), (0, 1, 1, 2, 2, 2), [0.0, 0.0, -10 * MS, 0.0, 2 * MS, -2000.0])
    assert T.tolist() == [3, 5 * tile + 7 + 100 - 10, 2 + 2 + 1 + 900 - 0]


def test_row_placement_enters_no_bit(pkg, tile):
    lens = (700, tile + 3, 0, 250, 31)
    gaps = [0.0, -20 * MS, 5 * MS, -7 * MS, 0.0]
    rows = make_rows(lens, 20)
    alone, o, T = check(pkg, rows[:4], None, gaps[:4])
    # the same utterances as rows 0 .. 3 of a larger batch whose other rows form tracks of their own
    more = rows[:4] + make_rows((tile * 2, 5, 77), 21)
    big, o2, T2 = check(pkg, more, (0, 0, 0, 0, 1, 1, 2), gaps[:4] + [0.0, -1 * MS, 0.0])
    assert same(big[0], alone[0]) and np.array_equal(o2[:4], o)
    # ... behind other tracks instead of in front of them
    behind, o3, T3 = check(pkg, more[4:] + rows[:4], (0, 0, 1, 2, 2, 2, 2), [0.0, -1 * MS, 0.0] + gaps[:4])
    assert same(behind[2], alone[0]) and same(behind[0], big[1])
    # two tracks in one call equal two calls
    a, _, _ = check(pkg, rows[:2], None, gaps[:2])
    b, _, _ = check(pkg, rows[2:], None, [0.0] + gaps[3:])
    both, _, _ = check(pkg, rows, (0, 0, 1, 1, 1), gaps)
    assert same(both[0], a[0]) and same(both[1], b[0])


def test_refusals(pkg):
    x = np.zeros((2, 8), np.float32)
    with pytest.raises(pkg.VitsError, match=r"vits_op_join: lens\[1\] = 9 is outside \[0, x_stride = 8\]"):
        pkg.join(x, FS, lens=[8, 9])
    with pytest.raises(pkg.VitsError, match=r"vits_op_join: y_stride = 17 is below the largest track bound \(18 samples\)"):
        pkg.join(x, FS, gap_ms=[0.0, 2 * MS], out=np.zeros((1, 17), np.float32))
    with pytest.raises(pkg.VitsError, match=r"vits_op_join: gap_ms\[1\] = 60000.5 \(utterance 1\)"):
        pkg.join(x, FS, gap_ms=[0.0, 60000.5], out=np.zeros((1, 17), np.float32))
    with pytest.raises(pkg.VitsError, match=r"vits_op_join: track\[1\] = 2 after track\[0\] = 0"):
        pkg.join(x, FS, track=[0, 2], out=np.zeros((1, 17), np.float32))
