"""The limiter kernels (limiter.hip) at the operator level, vits_op_limit, against the float64 restatement of the definition (tests/limiter_ref.py) fed
the device's own oversampled row: the true peak bit for bit, every sample of y within the five fp32 roundings that separate the two, the ceiling, the
identity under the ceiling, every length and peak position at which a tile or a window ends, nothing read or written behind a row, and bits that
depend on nothing but the row's own samples."""
import numpy as np
import pytest

import limiter_ref as LR

pytestmark = pytest.mark.gpu

RATES = (16000, 22050, 8000, 48000)
# five fp32 roundings separate the definitions (g0 e, the division, s to fp32, g0 s, x times that), 2^-24 relative each; six allows for their
# second-order terms. Derived, not measured. A lost halo or hold is an error of order 0.1 (tests/test_limiter_host.py).
Y_TOL = 6 * 2.0 ** -24
C_TOL = 2.0 ** -22   # |y| <= c (1 + 2^-22)
S_TOL = 2.0 ** -23   # min s
G_TOL = 1e-4         # dB on g0: a few fp32 ulps of exp10 / log10 (tests/test_gpu_level_ops.py)
CANARY = np.float32(7.25)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def ragged(rows, gap=5):
    lens = np.array([r.size for r in rows], np.int64)
    x = np.full((len(rows), int(lens.max()) + gap), np.nan, np.float32)
    for b, r in enumerate(rows):
        x[b, :r.size] = r
    return x, lens


def c32(ceiling_db):
    return float(np.float32(10.0 ** (float(np.float32(ceiling_db)) / 20.0)))


def oversampled(pkg, rows, fs):
    """the device's own 4x rows (vits_op_resample), one call for the batch"""
    x, lens = ragged(rows)
    u, n = pkg.resample(x, fs, 4 * fs, lens=lens)
    assert [int(v) for v in n] == [4 * r.size for r in rows]
    return [u[b, :4 * r.size] for b, r in enumerate(rows)]


def run(pkg, fs, rows, kind, value_db, ceiling_db, gap=5):
    x, lens = ragged(rows, gap)
    out = np.full((len(rows), x.shape[1] + 3), CANARY, np.float32)
    y, levels, limits = pkg.limit(x, fs, kind, value_db, ceiling_db, lens=lens, out=out)
    assert not np.isnan(y).any() and not np.isnan(levels).any() and not np.isnan(limits).any()  # nothing behind a row was read
    for b, r in enumerate(rows):
        assert (y[b, r.size:] == CANARY).all(), b  # nothing behind a row was written
    return y, levels, limits


def check(pkg, fs, rows, y, levels, limits, ceiling_db, tag=""):
    """every row of a limited batch against the restatement fed the device's own u; returns the worst relative error of y"""
    c = c32(ceiling_db)
    us = oversampled(pkg, rows, fs)
    uys = oversampled(pkg, [y[b, :r.size] for b, r in enumerate(rows)], fs)
    worst = worst_tp = worst_s = 0.0
    for b, (r, u, uy) in enumerate(zip(rows, us, uys)):
        n, g0, got = r.size, float(levels[b, 2]), y[b, :r.size].astype(np.float64)
        P = np.abs(r).max() if n else np.float32(0)
        tp = np.float32(max(float(P), float(np.abs(u).max()) if n else 0.0))
        assert levels[b, 1] == P and limits[b, 0] == tp, (tag, b, limits[b], tp)  # bit for bit: a maximum does not round
        want = LR.limiter(r, fs, g0, c, u=u)
        err = np.abs(got - want["y"])
        nz = want["y"] != 0
        assert (got[~nz] == 0).all(), (tag, b)
        if nz.any():
            worst = max(worst, float((err[nz] / np.abs(want["y"][nz])).max()))
        assert (err <= Y_TOL * np.abs(want["y"])).all(), (tag, b, n, float((err[nz] / np.abs(want["y"][nz])).max()), int(np.argmax(err)))
        assert (np.abs(got) <= c * (1 + C_TOL)).all(), (tag, b, float(np.abs(got).max()), c)
        # the rows of limits: TP(y) from the restatement's y and the device's 4x row of what was delivered; min s; the share
        s32 = want["s"].astype(np.float32)
        want_tpy = max(float(np.abs(want["y"]).max()) if n else 0.0, float(np.abs(uy).max()) if n else 0.0)
        worst_tp = max(worst_tp, abs(float(limits[b, 1]) - want_tpy) / want_tpy if want_tpy else 0.0)
        assert abs(float(limits[b, 1]) - want_tpy) <= Y_TOL * want_tpy, (tag, b, limits[b, 1], want_tpy)
        want_min = float(want["s"].min()) if n else 1.0
        worst_s = max(worst_s, abs(float(limits[b, 2]) - want_min))
        assert abs(float(limits[b, 2]) - want_min) <= S_TOL, (tag, b, limits[b, 2], want_min)
        want_share = np.float32(float((s32 < 1).sum()) / n) if n else np.float32(0)
        assert limits[b, 3] == want_share, (tag, b, limits[b, 3], want_share)
    print(f"{tag}: worst |y - ref| / |ref| = {worst / 2.0 ** -24:.2f} x 2^-24 (bound 6), TP(y) {worst_tp / 2.0 ** -24:.2f} x 2^-24, min s {worst_s / 2.0 ** -23:.2f} x 2^-23")
    return worst


def batch_of(pkg, fs):
    tile = pkg.limiter_plan(fs)[2]
    return [LR.sig_voiced(fs), LR.sig_noise(2 * tile + 3), (0.1 * LR.sig_voiced(fs, 0.25, 140.0)).astype(np.float32), LR.sig_quarter_sine(fs, 3000, 0.5, 256),
            LR.sig_peaks(tile + 7, tile), np.zeros(100, np.float32)]


@pytest.mark.parametrize("fs", RATES)
def test_a_ragged_batch_under_a_gain(pkg, fs):
    rows = batch_of(pkg, fs)
    y, levels, limits = run(pkg, fs, rows, pkg.LEVEL_GAIN, 6.0, -6.0)
    assert (levels[:, 2] == np.float32(10.0 ** (6.0 / 20.0))).all()
    check(pkg, fs, rows, y, levels, limits, -6.0, f"{fs} Hz gain")
    assert limits[0, 2] < 0.5 and limits[0, 3] > 0.3  # the voiced row is limited in earnest
    assert limits[2, 2] == 1.0 and limits[2, 3] == 0.0  # the quiet one not at all
    assert abs(float(limits[3, 0]) / 0.5 - 1) <= 1e-4 and abs(float(levels[3, 1]) * np.sqrt(2) / 0.5 - 1) <= 1e-6  # the sine: TP = amplitude, P = amplitude / sqrt(2)
    assert list(limits[5]) == [0.0, 0.0, 1.0, 0.0]  # silence: e == 0, r = 1


def test_loudness_without_the_ceiling_rule_and_true_peak_normalisation(pkg):
    fs = 16000
    t = np.arange(fs, dtype=np.float64) / fs
    rows = [np.tile(LR.sig_voiced(fs, 0.5), 2), (1e-5 * np.random.default_rng(3).standard_normal(fs)).astype(np.float32), LR.sig_quarter_sine(fs, 8000, 0.5, 256),
            (0.25 * np.sin(2 * np.pi * 500 * t)).astype(np.float32)]
    y, levels, limits = run(pkg, fs, rows, pkg.LEVEL_LOUDNESS, -12.0, -3.0)
    for b in range(len(rows)):
        L, P, g, blocks = (float(v) for v in levels[b])
        want = 10.0 ** ((-12.0 - L) / 20.0) if blocks > 0 else 1.0  # the ceiling no longer reduces it
        assert abs(20 * np.log10(g) - 20 * np.log10(want)) <= G_TOL, (b, g, want)
    assert levels[1, 2] == 1.0 and levels[1, 3] == 0  # unmeasurable
    assert levels[0, 2] * limits[0, 0] > c32(-3.0) and limits[0, 2] < 1.0  # the ceiling binds on the voiced row: the rule would have cut the gain of all of it
    check(pkg, fs, rows, y, levels, limits, -3.0, "loudness")
    # PEAK: g = 10^(value / 20) / TP, the plain multiply, and the second meter pass reads the stated peak
    y, levels, limits = run(pkg, fs, rows, pkg.LEVEL_PEAK, -2.0, 0.0)
    uys = oversampled(pkg, [y[b, :r.size] for b, r in enumerate(rows)], fs)
    for b, r in enumerate(rows):
        g, tp = float(levels[b, 2]), float(limits[b, 0])
        assert abs(20 * np.log10(g) - (-2.0 - 20 * np.log10(tp))) <= G_TOL, b
        assert same(y[b, :r.size], r * levels[b, 2])
        assert limits[b, 1] == np.float32(max(np.abs(y[b, :r.size]).max(), np.abs(uys[b]).max())) and limits[b, 2] == 1.0 and limits[b, 3] == 0.0
        assert abs(20 * np.log10(float(limits[b, 1])) - (-2.0)) <= 1e-3, (b, limits[b])
    assert limits[2, 0] > 1.4 * levels[2, 1]  # (the sine: sample-peak normalisation would have left it 3 dB over)


@pytest.mark.parametrize("fs", (16000, 48000))
def test_rows_under_the_ceiling_equal_the_plain_gain_bit_for_bit(pkg, fs):
    rows = [(0.1 * r).astype(np.float32) for r in batch_of(pkg, fs)]
    y, levels, limits = run(pkg, fs, rows, pkg.LEVEL_GAIN, 6.0, -6.0)
    x, lens = ragged(rows)
    yl, ll = pkg.level(x, fs, pkg.LEVEL_GAIN, 6.0, lens=lens)
    for b, r in enumerate(rows):
        assert same(y[b, :r.size], yl[b, :r.size]), b
        assert same(levels[b], ll[b]) and limits[b, 2] == 1.0 and limits[b, 3] == 0.0, b


@pytest.mark.parametrize("fs", (16000, 48000))
def test_every_length_and_a_peak_at_every_edge(pkg, fs):
    """at 48 kHz the window of the sliding minimum (2641) is longer than a tile: a block's halo spans two tiles"""
    A, H, tile = pkg.limiter_plan(fs)
    ns = [0, 1, 2, A, A + 1, H, H + A + 1, tile - 1, tile, tile + 1, 2 * tile + 3]
    rows = [LR.sig_peaks(n, tile, seed=20 + i) for i, n in enumerate(ns)]
    y, levels, limits = run(pkg, fs, rows, pkg.LEVEL_GAIN, 6.0, -6.0, gap=1)
    check(pkg, fs, rows, y, levels, limits, -6.0, f"{fs} Hz edges")
    for b, n in enumerate(ns):
        if n:
            assert limits[b, 2] < 0.5, n  # every row has a peak of 0.9 g0 = 1.8 over c = 0.5
            assert np.abs(y[b, :n]).max() > 0.45, n  # and it leaves at the ceiling, not under a gain cut for the whole row


def test_a_row_alone_first_and_last_in_a_batch(pkg):
    fs = 22050
    tile = pkg.limiter_plan(fs)[2]
    row = LR.sig_voiced(fs, 0.3)
    others = [LR.sig_noise(tile + 1, seed=9), LR.sig_peaks(3 * tile, tile)]
    alone = run(pkg, fs, [row], pkg.LEVEL_GAIN, 6.0, -6.0)
    first = run(pkg, fs, [row] + others, pkg.LEVEL_GAIN, 6.0, -6.0, gap=2)
    last = run(pkg, fs, others + [row], pkg.LEVEL_GAIN, 6.0, -6.0, gap=9)
    again = run(pkg, fs, [row], pkg.LEVEL_GAIN, 6.0, -6.0)
    for name, (y, lv, lm), b in (("first", first, 0), ("last", last, 2), ("again", again, 0)):
        assert same(y[b, :row.size], alone[0][0, :row.size]), name
        assert same(lv[b], alone[1][0]) and same(lm[b], alone[2][0]), name


def test_refusals(pkg):
    x = np.zeros((1, 8000), np.float32)
    for kind, value, ceiling, word in ((pkg.LEVEL_NONE, 0, 0, "VITS_LEVEL_NONE"), (pkg.LEVEL_MEASURE, 0, 0, "VITS_LEVEL_MEASURE"), (9, 0, 0, "unknown kind"),
                                       (pkg.LEVEL_GAIN, 41, 0, "value_db"), (pkg.LEVEL_GAIN, 0, 0.5, "ceiling_db"), (pkg.LEVEL_GAIN, 0, -61, "ceiling_db"),
                                       (pkg.LEVEL_GAIN, 0, float("nan"), "ceiling_db"), (pkg.LEVEL_PEAK, 0.5, 0, "value_db"), (pkg.LEVEL_LOUDNESS, -71, -1, "value_db"),
                                       (pkg.LEVEL_LOUDNESS, -23, 0.5, "ceiling_db")):
        with pytest.raises(pkg.VitsError, match=word):
            pkg.limit(x, 16000, kind, value, ceiling)
    for fs in (3999, 48001, 96000):
        with pytest.raises(pkg.VitsError, match=str(fs)):
            pkg.limit(x, fs, pkg.LEVEL_GAIN)
    with pytest.raises(pkg.VitsError, match="VITS_LIMIT_OFF"):
        pkg.limit(x, 16000, pkg.LEVEL_GAIN, mode=pkg.LIMIT_OFF)
    with pytest.raises(pkg.VitsError, match="unknown mode"):
        pkg.limit(x, 16000, pkg.LEVEL_GAIN, mode=7)
    with pytest.raises(pkg.VitsError, match=r"lens\[0\]"):
        pkg.limit(x, 16000, pkg.LEVEL_GAIN, lens=[8001])
    with pytest.raises(pkg.VitsError, match="y_stride"):
        pkg.limit(x, 16000, pkg.LEVEL_GAIN, -3.0, out=np.zeros((1, 7999), np.float32))
    d = pkg.LimitDesc(pkg.LevelDesc(16000, 1, 8000, 8000, pkg.LEVEL_GAIN, 0.0, 0.0), pkg.LIMIT_TRUE_PEAK)
    lv = np.zeros(4, np.float32)
    assert pkg.lib().vits_op_limit(pkg.C.byref(d), x.ctypes.data, None, None, lv.ctypes.data, lv.ctypes.data) == -1 and "null" in pkg.last_error()
    pkg.limit(x, 16000, pkg.LEVEL_PEAK, -3.0, 55.0)  # the ceiling is ignored by the kind that has none
