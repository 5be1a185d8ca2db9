"""The levelling kernels (loudness.hip) at the operator level, vits_op_level, against the float64 restatement of the definition (tests/loudness_ref.py):
integrated loudness within 0.01 LU, the sample peak and the block counts exactly, the gain of every kind from the reported L and P, the multiply bit for
bit, nothing read or written behind an utterance, and bits that depend on nothing but the utterance's own samples."""
import ctypes as C

import numpy as np
import pytest

import loudness_ref as R

pytestmark = pytest.mark.gpu

Q = 64            # samples per sub-segment of the kernels (kernels.h kLevelQ)
L_TOL = 0.01      # LU: the largest fp32-against-float64 difference of a sequential evaluation is 3e-4, the smallest defect effect of the signals 0.55
G_TOL = 1e-4      # dB: a few fp32 ulps of exp10 / log10
_REF = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def ref(fs, name, x):
    """the restatement of one signal, computed once and shared"""
    if (fs, name) not in _REF:
        _REF[(fs, name)] = R.loudness(x, fs)
    return _REF[(fs, name)]


def batch_of(fs):
    sig = R.signals(fs) if fs in (16000, 22050) else {"levels": R.sig_levels(fs)}
    return list(sig), [sig[k] for k in sig]


def check_levels(fs, names, rows, levels):
    worst = 0.0
    for b, (name, x) in enumerate(zip(names, rows)):
        L, P, nb = ref(fs, name, x)
        got_L, got_P, _, got_nb = (float(v) for v in levels[b])
        assert got_P == np.float32(P), (fs, name)
        assert got_nb == nb, (fs, name)
        if np.isfinite(L):
            worst = max(worst, abs(got_L - L))
            assert abs(got_L - L) <= L_TOL, (fs, name, got_L, L)
        else:
            assert got_L == -np.inf, (fs, name)
    return worst


@pytest.mark.parametrize("fs", [16000, 22050, 8000, 48000])
def test_loudness_peak_and_blocks_of_a_ragged_batch(pkg, fs):
    names, rows = batch_of(fs)
    x, lens = R.ragged(rows)
    y, levels = pkg.level(x, fs, pkg.LEVEL_MEASURE, lens=lens)
    worst = check_levels(fs, names, rows, levels)
    print(f"{fs} Hz: worst |L - float64| = {worst:.2e} LU")
    for b, r in enumerate(rows):
        assert levels[b, 2] == 1.0
        assert same(y[b, :r.size], r)  # MEASURE leaves the samples as they are
        assert not y[b, r.size:].any()  # nothing written behind lens[b]


def test_lengths_around_every_boundary(pkg):
    fs, S = 16000, 1600
    rng = np.random.default_rng(11)
    base = (0.1 * rng.standard_normal(5 * S + 8)).astype(np.float32)
    ns = [0, 1, 4 * S - 1, 4 * S, 4 * S + 1, 5 * S - 1, 5 * S, Q - 1, Q, Q + 1]
    rows = [base[:n] for n in ns]
    x, lens = R.ragged(rows)
    y, levels = pkg.level(x, fs, pkg.LEVEL_PEAK, -6.0, lens=lens)
    for b, n in enumerate(ns):
        L, P, nb = R.loudness(rows[b], fs)
        assert levels[b, 3] == nb == (0 if n < 4 * S else (n - 3 * S) // S), n
        assert levels[b, 1] == np.float32(P), n
        if nb:
            assert abs(float(levels[b, 0]) - L) <= L_TOL, n
        else:
            assert levels[b, 0] == -np.inf, n
        g = R.gain(R.LEVEL_PEAK, -6.0, 0.0, levels[b, 0], levels[b, 1])
        assert abs(20 * np.log10(float(levels[b, 2])) - 20 * np.log10(g)) <= G_TOL, n
        assert same(y[b, :n], rows[b] * levels[b, 2]) and not y[b, n:].any(), n
    assert levels[0, 2] == 1.0  # (an empty utterance: P == 0)


KINDS = (("LEVEL_MEASURE", 0.0, 0.0), ("LEVEL_GAIN", -3.0, 0.0), ("LEVEL_GAIN", 12.5, 0.0), ("LEVEL_PEAK", -1.0, 0.0), ("LEVEL_LOUDNESS", -23.0, -1.0),
         ("LEVEL_LOUDNESS", -16.0, -20.0), ("LEVEL_LOUDNESS", -16.0, -1.0))


@pytest.mark.parametrize("kind,value,ceiling", KINDS)
def test_every_kind_gain_multiply_and_identities(pkg, kind, value, ceiling):
    fs = 16000
    k = getattr(pkg, kind)
    names, rows = batch_of(fs)
    x, lens = R.ragged(rows, gap=7)
    canary = np.float32(7.25)
    out = np.full((len(rows), x.shape[1] + 2), canary, np.float32)
    y, levels = pkg.level(x, fs, k, value, ceiling, lens=lens, out=out)
    check_levels(fs, names, rows, levels)
    for b, (name, r) in enumerate(zip(names, rows)):
        L, P, g = (float(v) for v in levels[b, :3])
        want = R.gain(k, value, ceiling, L, P)
        assert abs(20 * np.log10(g) - 20 * np.log10(want)) <= G_TOL, (kind, name, g, want)
        assert same(y[b, :r.size], r * np.float32(g)), (kind, name)  # one fp32 multiply by the reported g
        assert (y[b, r.size:] == canary).all(), (kind, name)  # nothing written behind lens[b]
    if k == pkg.LEVEL_LOUDNESS:
        i = names.index("levels")
        L, P, g = (float(v) for v in levels[i, :3])
        by_loudness, by_ceiling = 10.0 ** ((value - L) / 20.0), 10.0 ** (ceiling / 20.0) / P
        binds = by_ceiling < by_loudness
        assert binds == (ceiling == -20.0)  # (L = -16.29, P = 0.25: -16 LUFS needs + 0.29 dB, a ceiling of -20 dB allows - 7.96 dB)
        assert abs(g / min(by_loudness, by_ceiling) - 1) < 1e-5
        assert levels[names.index("silence"), 2] == 1.0  # unmeasurable
    # a row of the batch = the same row alone = the batch in reversed order = a second run
    y2, levels2 = pkg.level(x, fs, k, value, ceiling, lens=lens)
    xr, lr = R.ragged(rows[::-1], gap=1)
    y3, levels3 = pkg.level(xr, fs, k, value, ceiling, lens=lr)
    for b, r in enumerate(rows):
        y1, levels1 = pkg.level(r, fs, k, value, ceiling)
        rb = len(rows) - 1 - b
        assert same(levels1[0], levels[b]) and same(levels2[b], levels[b]) and same(levels3[rb], levels[b]), (kind, b)
        assert same(y1[0, :r.size], y[b, :r.size]) and same(y2[b, :r.size], y[b, :r.size]) and same(y3[rb, :r.size], y[b, :r.size]), (kind, b)


def test_measure_only_and_a_long_utterance(pkg):
    """more than one group chain of the state scan (65536 samples), more than one tile per row, an odd stride"""
    fs = 16000
    t = np.arange(70001, dtype=np.float64) / fs
    x = (0.5 + 0.01 * np.sin(2 * np.pi * 300 * t)).astype(np.float32)
    y, levels = pkg.level(x, fs, pkg.LEVEL_MEASURE, apply=False)
    L, P, nb = R.loudness(x, fs)
    print(f"long carry: {float(levels[0, 0])!r} against {L!r}")
    assert y is None and abs(float(levels[0, 0]) - L) <= L_TOL and levels[0, 1] == np.float32(P) and levels[0, 3] == nb


def test_refusals(pkg):
    x = np.zeros((1, 8000), np.float32)
    for kind, value, ceiling, word in ((pkg.LEVEL_NONE, 0, 0, "VITS_LEVEL_NONE"), (9, 0, 0, "unknown kind"), (pkg.LEVEL_GAIN, 41, 0, "value_db"),
                                       (pkg.LEVEL_GAIN, -61, 0, "value_db"), (pkg.LEVEL_GAIN, float("nan"), 0, "value_db"), (pkg.LEVEL_PEAK, 0.5, 0, "value_db"),
                                       (pkg.LEVEL_PEAK, -60.5, 0, "value_db"), (pkg.LEVEL_LOUDNESS, -71, -1, "value_db"), (pkg.LEVEL_LOUDNESS, 1, -1, "value_db"),
                                       (pkg.LEVEL_LOUDNESS, -23, 0.5, "ceiling_db"), (pkg.LEVEL_LOUDNESS, -23, float("inf"), "ceiling_db")):
        with pytest.raises(pkg.VitsError, match=word):
            pkg.level(x, 16000, kind, value, ceiling)
    for fs in (3999, 192001):
        with pytest.raises(pkg.VitsError, match=str(fs)):
            pkg.level(x, fs, pkg.LEVEL_MEASURE)
    with pytest.raises(pkg.VitsError, match=r"lens\[0\]"):
        pkg.level(x, 16000, pkg.LEVEL_MEASURE, lens=[8001])
    with pytest.raises(pkg.VitsError, match="y_stride"):
        pkg.level(x, 16000, pkg.LEVEL_GAIN, -3.0, out=np.zeros((1, 7999), np.float32))
    # the ceiling is ignored by the kinds that have none
    pkg.level(x, 16000, pkg.LEVEL_PEAK, -3.0, 55.0)
