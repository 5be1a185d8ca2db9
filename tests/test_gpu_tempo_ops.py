"""The time-stretch kernels at operator level (vits_op_tempo, tempo.hip): offsets and samples bit for bit what the numpy restatement (tests/tempo_ref.py) gives,
on the signals, lengths, rates and tempos of tests/test_tempo_host.py and on rows whose output ends around an edge of the overlap-add's tile; the counts of the
plan and nothing written behind them; rows of a mixed-tempo batch that never see their neighbours, their batch position, the strides or the base alignment;
exact copies at tempo 1; the refusals.

Bit for bit includes rows that hold NaN and +Inf: a NaN sample is 0 to the search and goes through the two products and the add as IEEE 754 says (the quiet NaN
numpy writes keeps its bits through a multiply and an add on either side); the rows hold no -Inf, so no sum makes a NaN of its own, whose sign a processor is
free to choose."""
import numpy as np
import pytest

import tempo_ref as TR

pytestmark = pytest.mark.gpu

TILE = 1024  # output samples per block of tempo_ola_kernel (kernels.h kTempoTile)
NAN_FILL = 0xFF


@pytest.fixture(autouse=True)
def nan_behind_the_rows(pkg):
    """the device copies of y and of the offsets hold 0xFF bytes (NaN; -1 as an int32) wherever no kernel writes"""
    pkg.op_set_output_fill(NAN_FILL)
    yield
    pkg.op_set_output_fill(0)


_REF = {}


def ref(kind, n, rate, q):
    """the restatement of one row, computed once per session and never written to"""
    key = (kind, n, rate, q)
    if key not in _REF:
        y, off = TR.tempo(TR.signal(kind, n), rate, q)
        y.setflags(write=False)
        off.setflags(write=False)
        _REF[key] = (y, off)
    return _REF[key]


def tile_edge_lengths(q):
    """rows whose output ends just before, at and just after the end of the first tile (N' = ceil(N / q): the nearest counts that exist at this tempo)"""
    Q = TR.plan(16000, q, 0)[2]
    return [-((-t * Q) >> 24) for t in (TILE - 1, TILE, TILE + 1)]


def check_rows(pkg, rate, q, kinds_lens):
    lens = np.asarray([n for _, n in kinds_lens], np.int64)
    x = np.full((lens.size, int(lens.max()) + 5), np.nan, np.float32)
    for b, (kind, n) in enumerate(kinds_lens):
        x[b, :n] = TR.signal(kind, n)
    y, n_out, off = pkg.tempo(x, rate, q, lens)
    for b, (kind, n) in enumerate(kinds_lens):
        want, want_off = ref(kind, n, rate, q)
        H, D, Q, F, N1 = TR.plan(rate, q, n)
        assert n_out[b] == want.size == N1 == pkg.tempo_plan(rate, q, n)[4], (kind, n)
        assert np.array_equal(off[b, :F], want_off), (rate, q, kind, n, off[b, :F], want_off)
        assert (off[b, F:] == -1).all(), (kind, n)  # (the fill: nothing written behind a row's F offsets)
        assert np.array_equal(y[b, :N1].view(np.uint32), want.view(np.uint32)), (rate, q, kind, n)
        assert np.isnan(y[b, N1:]).all(), (kind, n)
        if Q == TR.ONE:
            assert np.array_equal(y[b, :n].view(np.uint32), x[b, :n].view(np.uint32))
        if kind == "silence":
            assert not want_off.any()


@pytest.mark.parametrize("q", TR.TEMPOS)
@pytest.mark.parametrize("rate", TR.RATES)
def test_offsets_and_samples_are_the_restatement(pkg, rate, q):
    """every signal at every length in one launch per signal; at 16 kHz the rows around the tile's edge as well (white noise)"""
    for kind in TR.KINDS:
        check_rows(pkg, rate, q, [(kind, n) for n in TR.lengths(rate)])
    if rate == 16000:
        edge = tile_edge_lengths(q)
        check_rows(pkg, rate, q, [("noise", n) for n in edge])
        assert {(TR.plan(rate, q, n)[4] + TILE - 1) // TILE for n in edge} == {1, 2}


def mixed_batch():
    """every tempo on a short row and on a row of more than two tiles: 16 rows, short and long in turn, the long rows' tempos three places on, so that
    neighbours differ"""
    lens, tempos = [], []
    for j, q in enumerate(TR.TEMPOS):
        ql = TR.TEMPOS[(j + 3) % len(TR.TEMPOS)]
        lens += [97 + j, int((2 * TILE + 77) * max(ql, 1.0)) + 1 + j]
        tempos += [q, ql]
    return np.asarray(lens, np.int64), np.asarray(tempos, np.float32)


def test_rows_of_a_mixed_batch_are_the_rows_alone(pkg):
    """NaN behind every length; one launch, eight tempos: every row, offsets and samples, bit for bit the row run alone (batch 1, x_stride = the row), every row
    at every batch position (all 16 rotations), over five layouts of x and of y in turn: 16-byte-aligned bases with strides that are multiples of 4 (the 16-byte
    path), a stride that is no multiple of 4, and unaligned bases (the scalar path). The bases are placed, not hoped for."""
    rate = 16000
    lens, tempos = mixed_batch()
    B = lens.size
    rows = [TR.signal("noise", int(n), seed=7) for n in lens]
    alone = []
    for b in range(B):
        y, n_out, off = pkg.tempo(rows[b], rate, tempos[b])
        F = TR.plan(rate, float(tempos[b]), int(lens[b]))[3]
        alone.append((y[0, :n_out[0]].copy(), off[0, :F].copy()))
        assert np.isfinite(alone[-1][0]).all()
    assert sum(a.size > 2 * TILE for a, _ in alone) == len(TR.TEMPOS)
    assert all(tempos[b] != tempos[(b + 1) % B] for b in range(B))
    longest_out = max(a.size for a, _ in alone)
    w4, o4 = (int(lens.max()) + 3) // 4 * 4, (longest_out + 3) // 4 * 4
    layouts = ((0, 0, 0, 0), (3, 0, 0, 0), (8, 0, 4, 0), (4, 1, 0, 0), (0, 0, 1, 0), (4, 0, 4, 3), (1, 3, 2, 2))  # (x stride +, x offset, y stride +, y offset)
    vec = 0

    def place(rows_, stride, offset):
        flat = np.full(rows_ * stride + 8, np.nan, np.float32)
        offset += (-(flat.ctypes.data // 4)) % 4  # (floats up to the next 16-byte boundary, then the layout's own)
        return flat[offset:offset + rows_ * stride].reshape(rows_, stride)  # (a C-contiguous view: stride and alignment reach the device as they are)

    for shift in range(B):
        xs, xo, ys, yo = layouts[shift % len(layouts)]
        order = np.roll(np.arange(B), shift)
        x, out = place(B, w4 + xs, xo), place(B, o4 + ys, yo)
        assert (x.ctypes.data % 16 == 0) == (xo == 0) and (out.ctypes.data % 16 == 0) == (yo == 0)
        vec += int(xo == 0 and yo == 0 and xs % 4 == 0 and ys % 4 == 0)
        for i, b in enumerate(order):
            x[i, :lens[b]] = rows[b]
        y, n_out, off = pkg.tempo(x, rate, tempos[order], lens[order], out=out)
        assert y is out
        for i, b in enumerate(order):
            want, want_off = alone[b]
            assert n_out[i] == want.size
            assert np.array_equal(off[i, :want_off.size], want_off), (layouts[shift % len(layouts)], i, int(b), float(tempos[b]))
            assert (off[i, want_off.size:] == -1).all()
            assert np.array_equal(y[i, :n_out[i]].view(np.uint32), want.view(np.uint32)), (layouts[shift % len(layouts)], i, int(b), float(tempos[b]))
            assert np.isnan(y[i, n_out[i]:]).all()
    assert 0 < vec < B  # (both instances of the overlap-add ran)


def test_tempo_one_copies_and_the_refusals(pkg):
    rate = 16000
    lens = np.asarray(TR.lengths(rate) + [2 * TILE + 3], np.int64)
    x = np.full((lens.size, int(lens.max()) + 5), np.nan, np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = TR.signal("nonfinite" if b % 2 else "noise", int(n))
    y = np.zeros((lens.size, x.shape[1] + 9), np.float32)
    _, n_out, off = pkg.tempo(x, rate, 1.0, lens, out=y)
    for b, n in enumerate(lens):
        F = TR.plan(rate, 1.0, int(n))[3]
        assert n_out[b] == n and np.array_equal(y[b, :n].view(np.uint32), x[b, :n].view(np.uint32)) and np.isnan(y[b, n:]).all()
        assert not off[b, :F].any() and (off[b, F:] == -1).all()
    need = max(TR.plan(rate, 0.5, int(n))[4] for n in lens)
    with pytest.raises(pkg.VitsError, match="y_stride = %d is shorter than the longest output row" % (need - 1)):
        pkg.tempo(x, rate, 0.5, lens, out=np.zeros((lens.size, need - 1), np.float32))
    with pytest.raises(pkg.VitsError, match=r"lens\[0\]"):
        pkg.tempo(x, rate, 1.5, np.full(lens.size, x.shape[1] + 1, np.int64))
    with pytest.raises(pkg.VitsError, match=r"row 1: tempo .* outside \[0.5, 2\]"):
        pkg.tempo(x[:2], rate, np.array([1.0, 2.5], np.float32), lens[:2], out=np.zeros((2, 4096), np.float32))
    with pytest.raises(pkg.VitsError, match=r"row 0: tempo .* not finite"):
        pkg.tempo(x[:1], rate, float("nan"), lens[:1], out=np.zeros((1, 4096), np.float32))
    for bad in (7999, 48001):
        with pytest.raises(pkg.VitsError, match=r"rate %d is outside \[8000, 48000\]" % bad):
            pkg.tempo(x[:1], bad, 1.5, lens[:1], out=np.zeros((1, 4096), np.float32))
