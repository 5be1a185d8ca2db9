"""The edges kernels (edges.hip) at the operator level, vits_op_edges, against the float64 restatement of the definition (tests/edges_ref.py): the rows
{a, b, N', n_active} and lens_out exact, y bit for bit, [N', bound) zero and nothing behind the bound written (a sentinel-filled y), NaNs behind every
row changing nothing, every length and burst position at which a window or a tile of the window kernel ends, and bits that depend on nothing but the
row's own samples. Every comparison of bounds first asserts the reference's margin (edges_ref.margin): a condition on the inputs, not a tolerance."""
import numpy as np
import pytest

import edges_ref as ER

pytestmark = pytest.mark.gpu

FS = ER.FS
MARGIN = 1e-6
CANARY = np.float32(7.25)
DESC = dict(keep_head_ms=12.5, keep_tail_ms=7.3, fade_in_ms=5.0, fade_out_ms=9.0, lead_ms=20.0, tail_ms=150.0)
MODES = ((ER.PAD, 0.0),) + ER.THRESHOLDS


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def ragged(rows, gap=5):
    """the rows side by side, NaN behind each: a read past a row's samples shows in the result"""
    lens = np.array([r.size for r in rows], np.int32)
    x = np.full((len(rows), int(lens.max()) + gap), np.nan, np.float32)
    for b, r in enumerate(rows):
        x[b, :r.size] = r
    return x, lens


def run(pkg, fs, rows, mode, threshold_db, desc, gap=5):
    """vits_op_edges on the ragged batch, every row held against the restatement; returns (y, lens_out, rows)"""
    x, lens = ragged(rows, gap)
    p = ER.plan(fs, **desc)
    pads = p["Pl"] + p["Pt"]
    out = np.full((len(rows), int(lens.max()) + pads + 3), CANARY, np.float32)
    y, lens_out, got = pkg.edges(x, fs, mode, lens=lens, out=out, threshold_db=threshold_db, **desc)
    for b, r in enumerate(rows):
        assert ER.margin(r, fs, mode, threshold_db, **desc) >= MARGIN, b
        want_y, want_row = ER.edges(r, fs, mode, threshold_db, **desc)
        assert np.array_equal(got[b], want_row), (b, r.size, got[b], want_row)
        n1, bound = int(want_row[2]), r.size + pads
        assert lens_out[b] == n1
        assert same(y[b, :n1], want_y), (b, r.size, int(np.flatnonzero(bits(y[b, :n1]) != bits(want_y))[0]))
        assert not bits(y[b, n1:bound]).any(), b  # [N', bound) is +0
        assert (y[b, bound:] == CANARY).all(), b  # nothing behind the bound was written
    return y, lens_out, got


def tail_burst(n, width=50, seed=3):
    """a floor with a burst over its last `width` samples: the row's last window decides the bounds"""
    return ER.burst(ER.floor(n, seed), max(0, n - width), n, seed + 1)


@pytest.mark.parametrize("mode,threshold_db", MODES)
def test_every_signal_in_one_ragged_batch(pkg, mode, threshold_db):
    sig = ER.signals()
    rows = [sig[k] for k in sorted(sig)]
    _, _, got = run(pkg, FS, rows, mode, threshold_db, DESC)
    if mode != ER.PAD:
        assert got[:, 3].tolist() == [26, 20, 4, 6, 4, 1, 26 if mode == ER.TRIM_RELATIVE else 0, 0, 1]  # (alphabetical: all_active .. single)


def test_every_length_at_which_a_window_or_a_tile_ends(pkg):
    W, t = pkg.edges_plan(FS)[0], pkg.edges_plan(FS)[7]
    assert (W, t) == (160, 4000)
    ns = [0, 1, W - 1, W, W + 1, t - 1, t, t + 1, 2 * t + W + 1]
    rows = [tail_burst(n, seed=20 + i) for i, n in enumerate(ns)]
    for mode, th in MODES:
        _, _, got = run(pkg, FS, rows, mode, th, DESC, gap=1)
        if mode != ER.PAD:
            # the burst of 50 samples ends at N: it lies in the last window, or in the last two
            assert [int(v) for v in got[:, 1]] == ns and all(got[i, 3] == (0 if n == 0 else 2 if 0 < n % W < 50 and n > W else 1) for i, n in enumerate(ns))
    # the same lengths with nothing to cut and no fades or pads: the row itself, bit for bit
    y, lens_out, _ = run(pkg, FS, rows, ER.TRIM_RELATIVE, -120.0, {}, gap=1)
    for b, r in enumerate(rows):
        assert lens_out[b] == r.size and same(y[b, :r.size], r)


@pytest.mark.parametrize("d_on,d_end", [(-1, -1), (0, 0), (1, 1), (-1, 1), (1, -1)])
def test_the_onset_and_the_end_on_a_tile_edge_and_one_sample_either_side(pkg, d_on, d_end):
    W, t = pkg.edges_plan(FS)[0], pkg.edges_plan(FS)[7]
    n = 2 * t + W + 1
    x = ER.sig_onset(n, t + d_on, 2 * t + d_end, seed=40 + 3 * d_on + d_end)
    for mode, th in ER.THRESHOLDS:
        _, _, got = run(pkg, FS, [x, x[:2 * t + 1], x[:t + 2]], mode, th, DESC)
        first, last = (t + d_on) // W, (2 * t + d_end - 1) // W
        assert got[0].tolist()[:2] == [first * W - 200, min(n, (last + 1) * W + 117)] and got[0, 3] == last - first + 1


@pytest.mark.parametrize("fs", (8000, 22050))
def test_another_rate(pkg, fs):
    W, t = pkg.edges_plan(fs)[0], pkg.edges_plan(fs)[7]
    assert W == (fs + 50) // 100 and t % W == 0
    sig = ER.signals(W=W, n=25 * W)
    rows = [sig[k] for k in sorted(sig)] + [tail_burst(n, seed=60 + i) for i, n in enumerate((t - 1, t + 1, 2 * t + W + 1))]
    for mode, th in MODES:
        run(pkg, fs, rows, mode, th, DESC)


def test_a_row_alone_first_and_last_in_a_batch(pkg):
    t = pkg.edges_plan(FS)[7]
    row = ER.sig_onset(t + 700, 900, t + 300, seed=70)
    others = [tail_burst(t + 1, seed=71), ER.floor(3 * t, 72), np.zeros(0, np.float32)]
    for mode, th in MODES:
        alone = run(pkg, FS, [row], mode, th, DESC)
        first = run(pkg, FS, [row] + others, mode, th, DESC, gap=2)
        last = run(pkg, FS, others + [row], mode, th, DESC, gap=9)
        n1 = int(alone[1][0])
        for name, (y, lo, rw), b in (("first", first, 0), ("last", last, 3)):
            assert lo[b] == n1 and np.array_equal(rw[b], alone[2][0]) and same(y[b, :n1], alone[0][0, :n1]), (mode, name)


def test_fades_longer_than_the_kept_range_and_pads_longer_than_the_row(pkg):
    desc = dict(fade_in_ms=25.0, fade_out_ms=40.0, lead_ms=375.0, tail_ms=380.0)
    rows = [ER.signals()["single"], tail_burst(161, seed=80), tail_burst(7, width=7, seed=81)]
    for mode, th in MODES:
        run(pkg, FS, rows, mode, th, desc)


def test_refusals(pkg):
    x = np.zeros((1, 8000), np.float32)
    with pytest.raises(pkg.VitsError, match="y_stride"):
        pkg.edges(x, FS, pkg.EDGES_PAD, out=np.zeros((1, 8000 + 320 + 2400 - 1), np.float32), **DESC)
    pkg.edges(x, FS, pkg.EDGES_PAD, out=np.zeros((1, 8000 + 320 + 2400), np.float32), **DESC)
    with pytest.raises(pkg.VitsError, match=r"lens\[0\]"):
        pkg.edges(x, FS, pkg.EDGES_PAD, lens=[8001])
    with pytest.raises(pkg.VitsError, match="VITS_EDGES_OFF"):
        pkg.edges(x, FS, pkg.EDGES_OFF)
    with pytest.raises(pkg.VitsError, match="unknown mode"):
        pkg.edges(x, FS, 7)
    with pytest.raises(pkg.VitsError, match="threshold_db"):
        pkg.edges(x, FS, pkg.EDGES_TRIM_ABSOLUTE, threshold_db=1.0)
    with pytest.raises(pkg.VitsError, match="192001"):
        pkg.edges(x, 192001, pkg.EDGES_PAD)
    # a NULL y (the other pointers are never dereferenced before the check)
    d = pkg.edges_desc(pkg.EDGES_PAD)
    one = np.zeros(4, np.int64)
    p = one.ctypes.data
    assert pkg.lib().vits_op_edges(FS, pkg.C.byref(d), 1, p, 8, p, None, 8, p, p) == -1 and "null" in pkg.last_error()
