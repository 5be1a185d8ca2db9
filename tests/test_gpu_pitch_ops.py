"""The varispeed kernel at operator level (vits_op_pitch, pitch.hip): every output sample inside the derived rounding bound around the float64 restatement
(tests/pitch_ref.py) evaluated from the product's own tables, the counts of the plan and nothing written behind them, rows of a mixed-ratio batch that never
see their neighbours, the gap behind their own end, their batch position, the stride or the base alignment, and exact copies at ratio 1.

The bound. Index, fr and a are exact integers or exact fp32 values on both sides; the reference interpolates the same fp32 tables. The device rounds a tap's
weight twice, h32 = fl(a fl(fr D[i] + G[i])) (one fmaf, one multiply): |h32 - h| <= (2 u + u^2) |h|, u = 2^-24. The chain acc = fmaf(h32, x, acc) rounds once
per tap: after K taps |acc - sum h32 x| <= ((1 + u)^K - 1) sum |h32| |x| (the standard bound of recursive summation with fused products). Together, to first
order, |y - y_f64| <= (K + 2) u sum |h| |x|; the second-order terms are below K^2 u^2 < 2e-11 of the same sum, and one more u covers them and the float64
reference's own rounding: (K + 3) 2^-24 sum_k |h_k| |x_k|."""
import numpy as np
import pytest

import pitch_ref as PR

pytestmark = pytest.mark.gpu

TILE = 1024  # output samples per block of pitch_kernel (kernels.h kPitchTile)
RATIOS = (0.5, PR.ratio(-2), 1.0 - 2.0 ** -24, 1.0, 1.0 + 2.0 ** -23, PR.ratio(2), 1.5, 2.0)
NAN_FILL = 0xFF


def row_lengths(p):
    """1 (both edges at once), 2, around the filter's half width and its whole width, around a wave and 256 threads, 1000, and rows whose output ends before, at
    and after the end of the first tile (N' = ceil(N / p): the nearest counts that exist at this ratio)"""
    P, _, R = PR.plan(p, 0)[:3]
    return [1, 2, R, R + 1, 2 * R + 1, 255, 256, 257, 1000] + [-((-t * P) >> 24) for t in (TILE - 1, TILE, TILE + 1)]


def ragged(lens, seed, fill=np.nan, extra=5):
    lens = np.asarray(lens, np.int64)
    rng = np.random.default_rng(seed)
    x = np.full((lens.size, int(lens.max()) + extra), fill, np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = rng.standard_normal(n).astype(np.float32)
    return x, lens


@pytest.fixture(scope="module")
def tables(pkg):
    G, D = pkg.pitch_table()
    return G, D


@pytest.fixture(autouse=True)
def nan_behind_the_rows(pkg):
    """the device copy of y holds 0xFF bytes (NaN) wherever the kernel does not write"""
    pkg.op_set_output_fill(NAN_FILL)
    yield
    pkg.op_set_output_fill(0)


@pytest.mark.parametrize("p", RATIOS)
def test_every_sample_is_inside_the_chain_bound(pkg, tables, p):
    """accuracy (the bound of the module docstring), counts (N' of the plan, NaN — the fill — behind it) and tiles (rows of one block and of more than one);
    at ratio 1 the rows are exact copies"""
    x, lens = ragged(row_lengths(p), 31)
    y, n_out = pkg.pitch(x, p, lens)
    P, _, _, K, _ = PR.plan(p, 0)
    tiles = set()
    for b, n in enumerate(lens):
        want, mag = PR.pitch(x[b, :n], p, tables=tables, with_bound=True)
        assert n_out[b] == want.size == PR.plan(p, int(n))[4] == pkg.pitch_plan(p, int(n))[3]
        got = y[b, :want.size]
        if P == PR.ONE:
            assert np.array_equal(got.view(np.uint32), x[b, :n].view(np.uint32)), (b, int(n))
        else:
            err = np.abs(got.astype(np.float64) - want)
            bound = (K + 3) * 2.0 ** -24 * mag
            print(f"p = {p}, n = {int(n)}: worst error / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
            assert (err <= bound).all(), (p, b, int(n), float((err / np.maximum(bound, 1e-300)).max()))
        assert np.isnan(y[b, want.size:]).all(), (b, int(n))
        tiles.add((want.size + TILE - 1) // TILE)
    assert min(tiles) == 1 and max(tiles) >= 2


def mixed_batch(seed):
    """every ratio on a row of more than one tile and on short rows: 24 rows, the ratios interleaved so that neighbours differ"""
    lens, ratios = [], []
    for i, n in enumerate((1, 71, 2 * TILE + 77)):
        for j, p in enumerate(RATIOS):
            lens.append(max(1, int(n * min(p, 1.0)) if n > TILE else n + i + j))
            ratios.append(p)
    order = np.random.default_rng(seed).permutation(len(lens))
    return np.asarray(lens, np.int64)[order], np.asarray(ratios, np.float32)[order]


def test_rows_of_a_mixed_batch_are_the_rows_alone(pkg):
    """NaN behind every length; one launch, eight ratios: every row finite and bit for bit the row run alone (batch 1, x_stride = the row), every row at
    every batch position (all 24 rotations of the batch), over five layouts in turn: two with a 16-byte-aligned base and a stride that is a multiple of 4 (the
    kernel's 16-byte loads), a stride that is no multiple of 4, and two unaligned bases (its scalar loads). The base is placed, not hoped for."""
    lens, ratios = mixed_batch(32)
    B = lens.size
    x0, _ = ragged(lens, 33, extra=0)
    alone = []
    for b in range(B):
        y, n_out = pkg.pitch(x0[b, :lens[b]].copy(), ratios[b])
        alone.append(y[0, :n_out[0]].copy())
        assert np.isfinite(alone[-1]).all()
    assert max(a.size for a in alone) > 2 * TILE and any(r == 0.5 and a.size > TILE for r, a in zip(ratios, alone)) and any(r == 2.0 and a.size > TILE for r, a in zip(ratios, alone))
    w4 = (x0.shape[1] + 3) // 4 * 4
    layouts = ((w4, 0), (w4 + 3, 0), (w4 + 8, 0), (w4 + 4, 1), (w4 + 1, 3))
    vec = 0
    for shift in range(B):
        stride, offset = layouts[shift % len(layouts)]
        order = np.roll(np.arange(B), shift)
        flat = np.full(B * stride + 8, np.nan, np.float32)
        offset += (-(flat.ctypes.data // 4)) % 4  # (floats up to the next 16-byte boundary, then the layout's own)
        x = flat[offset:offset + B * stride].reshape(B, stride)  # (a C-contiguous view: stride and alignment reach the device as they are)
        assert (x.ctypes.data % 16 == 0) == (layouts[shift % len(layouts)][1] == 0)
        vec += int(x.ctypes.data % 16 == 0 and stride % 4 == 0)
        for i, b in enumerate(order):
            x[i, :lens[b]] = x0[b, :lens[b]]
        y, n_out = pkg.pitch(x, ratios[order], lens[order])
        for i, b in enumerate(order):
            assert n_out[i] == alone[b].size
            assert np.array_equal(y[i, :n_out[i]].view(np.uint32), alone[b].view(np.uint32)), (stride, offset, i, int(b), float(ratios[b]))
            assert np.isnan(y[i, n_out[i]:]).all()
    assert 0 < vec < B  # (both instances of the kernel ran)


def test_ratio_one_copies_and_the_refusals(pkg):
    x, lens = ragged(row_lengths(1.0), 34)
    y = np.zeros((lens.size, x.shape[1] + 9), np.float32)
    _, n_out = pkg.pitch(x, 1.0, lens, out=y)
    for b, n in enumerate(lens):
        assert n_out[b] == n and np.array_equal(y[b, :n].view(np.uint32), x[b, :n].view(np.uint32)) and np.isnan(y[b, n:]).all()
    need = max(PR.plan(0.5, int(n))[4] for n in lens)
    with pytest.raises(pkg.VitsError, match="y_stride = %d is shorter than the longest output row" % (need - 1)):
        pkg.pitch(x, 0.5, lens, out=np.zeros((lens.size, need - 1), np.float32))
    with pytest.raises(pkg.VitsError, match=r"lens\[0\]"):
        pkg.pitch(x, 1.5, np.full(lens.size, x.shape[1] + 1, np.int64))
    with pytest.raises(pkg.VitsError, match=r"row 1: pitch ratio .* outside \[0.5, 2\]"):
        pkg.pitch(x[:2], np.array([1.0, 2.5], np.float32), lens[:2], out=np.zeros((2, 4096), np.float32))
