"""The resampling kernel at operator level (vits_op_resample, resample.hip): every output sample inside the derived rounding bound of a K-term fp32
chain around the float64 restatement (tests/resample_ref.py), rows that never see their neighbours or the gap behind their own end, the same bits at
every batch size and stride, and the two refusals."""
import numpy as np
import pytest

import resample_ref as R

pytestmark = pytest.mark.gpu

TILE = 1024  # output samples per block of resample_kernel (kernels.h kResampleTile)
PAIRS = ((16000, 8000), (16000, 24000), (16000, 44100), (44100, 16000), (48000, 16000))


def row_lengths(fi, fo):
    """1 (both edges at once), 2, around the filter's half width and its whole width, around a wave and 256 threads, 1000, and rows whose output ends one
    sample before, at and after the end of the first tile"""
    L, M, Rr = R.plan(fi, fo)[:3]
    return [1, 2, Rr, Rr + 1, 2 * Rr + 1, 255, 256, 257, 1000] + [-((-t * M) // L) for t in (TILE - 1, TILE, TILE + 1)]


def ragged(fi, fo, seed, fill=0.0):
    lens = np.array(row_lengths(fi, fo), np.int64)
    rng = np.random.default_rng(seed)
    x = np.full((lens.size, int(lens.max()) + 5), fill, np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = rng.standard_normal(n).astype(np.float32)
    return x, lens


@pytest.mark.parametrize("fi,fo", PAIRS)
def test_every_sample_is_inside_the_chain_bound(pkg, fi, fo):
    """|y_gpu - y_f64| <= (K + 3) 2^-24 sum_k |h_k| |x_k|: K roundings of the fp32 chain, the table's own rounding to fp32, and slack for the last bits of
    the restatement's I0 — derived, not measured. h in the magnitude sum is the product's table."""
    x, lens = ragged(fi, fo, 11)
    y, n_out = pkg.resample(x, fi, fo, lens)
    K = R.plan(fi, fo)[3]
    h32 = pkg.resample_taps(fi, fo)
    tiles = set()
    for b, n in enumerate(lens):
        want, _ = R.resample(x[b, :n], fi, fo, with_bound=True)
        _, mag = R.resample(x[b, :n], fi, fo, h=h32, with_bound=True)
        assert n_out[b] == want.size == R.out_len(fi, fo, int(n))
        err = np.abs(y[b, :want.size].astype(np.float64) - want)
        bound = (K + 3) * 2.0 ** -24 * mag
        assert (err <= bound).all(), (fi, fo, b, int(n), float((err / np.maximum(bound, 1e-300)).max()))
        assert (y[b, want.size:] == 0).all()
        tiles.add((want.size + TILE - 1) // TILE)
    assert min(tiles) == 1 and max(tiles) >= 2  # (rows of one block and of more than one)


@pytest.mark.parametrize("fi,fo", PAIRS)
def test_rows_are_independent(pkg, fi, fo):
    """NaN between every row's end and x_stride: every output finite and equal, bit for bit, to the row resampled alone; nothing behind N_out is written"""
    x, lens = ragged(fi, fo, 12, fill=np.nan)
    n_max = max(R.out_len(fi, fo, int(n)) for n in lens)
    y = np.full((lens.size, n_max + 7), -123.0, np.float32)
    _, n_out = pkg.resample(x, fi, fo, lens, out=y)
    for b, n in enumerate(lens):
        alone, _ = pkg.resample(x[b, :n].copy(), fi, fo)
        got = y[b, :n_out[b]]
        assert np.isfinite(got).all(), (b, int(n))
        assert np.array_equal(got.view(np.uint32), alone[0, :n_out[b]].view(np.uint32)), (b, int(n))
        assert (y[b, n_out[b]:] == -123.0).all(), (b, int(n))


@pytest.mark.parametrize("fi,fo,tile", ((192000, 12000, 512), (192000, 4000, 256)))
def test_steep_downsampling_takes_the_smaller_tiles(pkg, fi, fo, tile):
    """16 : 1 and 48 : 1: the input span of 1,024 outputs would not fit the block's LDS, so the launch halves the tile (two outputs per thread, one). Same
    bound, same independence, on rows of one tile, around its end and of more than three tiles."""
    L, M, Rr, K = R.plan(fi, fo)[:4]
    t = TILE  # (the launcher's rule, restated: halve while the staged span of t outputs exceeds 64 KB)
    while t > 256 and 4 * (t * M // L + K + 8) > 65536:
        t //= 2
    assert t == tile
    lens = np.array([1, 2 * Rr + 1, (tile - 1) * M // L, -((-(tile + 1) * M) // L), 3 * tile * M // L + 5], np.int64)
    rng = np.random.default_rng(15)
    x = np.full((lens.size, int(lens.max()) + 3), np.nan, np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = rng.standard_normal(n).astype(np.float32)
    y, n_out = pkg.resample(x, fi, fo, lens)
    h32 = pkg.resample_taps(fi, fo)
    for b, n in enumerate(lens):
        want, _ = R.resample(x[b, :n], fi, fo, with_bound=True)
        _, mag = R.resample(x[b, :n], fi, fo, h=h32, with_bound=True)
        got = y[b, :n_out[b]]
        assert n_out[b] == want.size
        assert (np.abs(got.astype(np.float64) - want) <= (K + 3) * 2.0 ** -24 * mag).all(), (b, int(n))
        alone, _ = pkg.resample(x[b, :n].copy(), fi, fo)
        assert np.array_equal(got.view(np.uint32), alone[0, :n_out[b]].view(np.uint32)) and (y[b, n_out[b]:] == 0).all(), (b, int(n))
    assert n_out.max() > 3 * tile and n_out[2] <= tile < n_out[3]


def test_the_chain_is_deterministic_across_batch_sizes_and_strides(pkg):
    fi, fo = 16000, 44100
    rng = np.random.default_rng(13)
    rows = [rng.standard_normal(n).astype(np.float32) for n in (700, 377, 1)]
    want = [pkg.resample(r, fi, fo)[0][0] for r in rows]  # batch 1, x_stride = the row
    for B, stride in ((3, 700), (3, 701), (64, 704), (64, 1023)):
        x = np.full((B, stride), np.nan, np.float32)
        lens = np.zeros(B, np.int64)
        for b in range(B):
            r = rows[b % 3]
            x[b, :r.size] = r
            lens[b] = r.size
        y, n_out = pkg.resample(x, fi, fo, lens)
        for b in range(B):
            w = want[b % 3]
            assert n_out[b] == w.size and np.array_equal(y[b, :w.size].view(np.uint32), w.view(np.uint32)), (B, stride, b)


def test_equal_rates_copy_and_a_short_stride_is_refused(pkg):
    x, lens = ragged(16000, 8000, 14, fill=np.nan)
    y = np.full(x.shape, -5.0, np.float32)
    _, n_out = pkg.resample(x, 22050, 22050, lens, out=y)
    for b, n in enumerate(lens):
        assert n_out[b] == n and np.array_equal(y[b, :n], x[b, :n]) and (y[b, n:] == -5.0).all()
    need = max(R.out_len(16000, 8000, int(n)) for n in lens)
    short = np.zeros((lens.size, need - 1), np.float32)
    with pytest.raises(pkg.VitsError, match="y_stride = %d is shorter than the longest output row" % (need - 1)):
        pkg.resample(x, 16000, 8000, lens, out=short)
    with pytest.raises(pkg.VitsError, match=r"lens\[0\]"):
        pkg.resample(x, 16000, 8000, np.full(lens.size, x.shape[1] + 1, np.int64))
