"""The true-peak limiter, host side (include/vits.h vits_model_set_limiter): the constants, vits_limiter_host against the float64 restatement
(tests/limiter_ref.py) on rows that each expose one stage, the guarantee s <= r, the identity under the ceiling, the shortest rows, the hold, the
meter on a sine whose samples miss its crests, the two mutations the GPU tests' bounds must catch, and the refusals. No device."""
import ctypes as C

import numpy as np
import pytest

import limiter_ref as LR

RATES = (8000, 16000, 22050, 48000)
TOL = 1e-9                 # both sides are double: only the order of the sums (the oversampled row, the mean) differs
Y_BOUND = 6 * 2.0 ** -24   # the bound of tests/test_gpu_limit_ops.py on every sample of y
_REF = {}


def db(v):
    return 20.0 * np.log10(v)


def ref(pkg, fs, name, x, g0, c):
    """the restatement of one row on the product's own fp32 table, computed once and shared"""
    key = (fs, name, g0, c)
    if key not in _REF:
        _REF[key] = LR.limiter(x, fs, g0, c, u=LR.oversample(x, fs, pkg.resample_taps(fs, 4 * fs)))
    return _REF[key]


def s_of(y, x, g0):
    """s where the row is not zero (y = x g0 s)"""
    nz = x != 0
    return y[nz] / (g0 * x[nz].astype(np.float64)), nz


@pytest.mark.parametrize("fs,A,H", [(8000, 40, 400), (16000, 80, 800), (22050, 110, 1103), (48000, 240, 2400)])
def test_plan_constants(pkg, fs, A, H):
    got = pkg.limiter_plan(fs)
    assert got[:2] == (A, H) == LR.constants(fs)
    assert got[2] >= 256 and got[2] % 4 == 0  # the device kernels' time tile
    assert H + A + 1 == {8000: 441, 16000: 881, 22050: 1214, 48000: 2641}[fs]  # the sliding minimum's window


@pytest.mark.parametrize("fs", RATES)
def test_host_equals_the_restatement(pkg, fs):
    x = LR.sig_voiced(fs)
    g0, c = 2.0, 0.5
    want = ref(pkg, fs, "voiced", x, g0, c)
    y, lim = pkg.limiter_host(x, fs, g0, db(c))
    scale = np.abs(want["y"]).max()
    s, nz = s_of(y, x, g0)
    print(f"{fs}: worst |y - ref| / peak = {np.abs(y - want['y']).max() / scale:.2e}, worst |s - ref| = {np.abs(s - want['s'][nz]).max():.2e}, limits {lim}")
    assert np.abs(y - want["y"]).max() <= TOL * scale
    assert np.abs(s - want["s"][nz]).max() <= TOL
    uy = LR.oversample(want["y"], fs, pkg.resample_taps(fs, 4 * fs))
    wl = LR.limits(x, LR.oversample(x, fs, pkg.resample_taps(fs, 4 * fs)), want["y"], uy, want["s"])
    assert np.abs(lim - wl).max() <= TOL
    assert 0.2 < lim[2] < 0.5 and 0.3 < lim[3] < 1.0  # (the row is limited in earnest)
    # the guarantee: every window of the mean contains the sample itself
    assert (want["s"] <= want["r"] * (1 + 1e-15)).all()
    assert (s <= want["r"][nz] * (1 + 1e-12)).all()
    assert np.abs(y).max() <= c * (1 + 1e-12)


@pytest.mark.parametrize("fs", RATES)
def test_identity_under_the_ceiling(pkg, fs):
    x = LR.sig_voiced(fs)
    g0 = 0.5
    tp = pkg.limiter_host(x, fs, 1.0, 0.0)[1][0]
    y, lim = pkg.limiter_host(x, fs, g0, db(g0 * tp * 1.000001))
    assert np.array_equal(y, x.astype(np.float64) * g0)  # s == 1 exactly: the mean of ones is 1 in any order
    assert lim[2] == 1.0 and lim[3] == 0.0 and abs(lim[1] / (g0 * tp) - 1) <= TOL


@pytest.mark.parametrize("fs", (16000, 48000))
def test_the_shortest_rows_and_an_impulse_at_either_end(pkg, fs):
    A, H, _ = pkg.limiter_plan(fs)
    y, lim = pkg.limiter_host(np.zeros(0, np.float32), fs, 2.0, db(0.5))
    assert y.size == 0 and list(lim) == [0.0, 0.0, 1.0, 0.0]
    for N in (1, 2, A, A + 1, H + A + 2):
        for pos in (0, N - 1):
            x = np.zeros(N, np.float32)
            x[pos] = 1.0
            y, lim = pkg.limiter_host(x, fs, 2.0, db(0.5))
            want = ref(pkg, fs, ("impulse", N, pos), x, 2.0, 0.5)
            # g0 = 2 on a unit impulse under c = 0.5: r = 0.25 there, so the peak leaves at exactly the ceiling
            assert np.abs(y).max() == 0.5 and lim[2] == 0.25 and lim[0] == 1.0, (N, pos)
            assert np.abs(y - want["y"]).max() <= TOL, (N, pos)
            # the gain is down from A samples before the impulse (attack) to H + A behind it (hold, release), inside the row; the oversampled impulse
            # passes the ceiling beside its two neighbours too (|u| = 0.64 half a sample away), which is the tolerance
            want_share = (min(N - 1, pos + H + A) - max(0, pos - A) + 1) / N
            assert abs(lim[3] - want_share) <= 2.0 / N, (N, pos, lim[3], want_share)


@pytest.mark.parametrize("gap", (-1, 0, 1, 83, 84, 85))
def test_the_hold_merges_two_impulses_or_does_not(pkg, gap):
    """two impulses H + gap apart. m[j] covers r[j - H .. j + A]: behind the first impulse it is held for H samples, and A samples before the second one the
    look-ahead has it already. H - 1, H and H + 1 apart the two are one gain reduction. They come apart only beyond H + A + 1, and since the oversampled
    impulse passes the ceiling beside its two neighbours too (|u| = 0.64 half a sample away), beyond H + A + 3 = H + 83: one sample of m returns to 1 for
    every sample of distance from there on"""
    fs = 16000
    A, H, _ = pkg.limiter_plan(fs)
    assert A + 3 == 83
    d = H + gap
    x = np.zeros(2 * A + d + H + 3 * A, np.float32)
    p0 = 2 * A
    x[p0] = x[p0 + d] = 1.0
    y, lim = pkg.limiter_host(x, fs, 2.0, db(0.5))
    want = ref(pkg, fs, ("pair", gap), x, 2.0, 0.5)
    assert np.abs(y - want["y"]).max() <= TOL
    assert list(np.flatnonzero(want["r"] < 1.0)) == [p0 - 1, p0, p0 + 1, p0 + d - 1, p0 + d, p0 + d + 1]
    between = want["m"][A + p0:A + p0 + d]  # m[j], j in [p0, p0 + d)
    released = int((between == 1.0).sum())
    print(f"impulses {d} apart: {released} samples of m back at 1, largest s between them {want['s'][p0:p0 + d].max():.4f}")
    assert released == max(0, d - A - H - 3)
    assert (want["s"][p0:p0 + d] < 1.0).all()  # (the mean over A + 1 needs A + 1 released samples to return to 1)
    assert (want["s"][p0 + A + 1:p0 + H + 1] == 0.25).all()  # held at the floor for H samples
    # (the restatement without the hold lets go at once: the stage is visible in the result)
    no_hold = LR.limiter(x, fs, 2.0, 0.5, u=LR.oversample(x, fs, pkg.resample_taps(fs, 4 * fs)), hold=False)
    assert (no_hold["s"][p0 + 3 * A:p0 + d - 3 * A] == 1.0).all()


@pytest.mark.parametrize("fs", RATES)
def test_true_peak_of_a_sine_whose_samples_miss_its_crests(pkg, fs):
    """fs / 4 with phase pi / 4: |x[n]| = amp / sqrt(2) at every sample, the waveform reaches amp. The meter's filter is a Kaiser window with beta 9, whose
    ripple is below 10^(-90 / 20) = 3.2e-5 of the amplitude; the bound is 1e-4. An abrupt start rings to 0.5067 (printed), hence the fade."""
    amp, n = 0.5, 4096
    x = LR.sig_quarter_sine(fs, n, amp, fade=256)
    _, lim = pkg.limiter_host(x, fs, 1.0, 0.0)
    u = LR.oversample(x, fs)
    raw = LR.sig_quarter_sine(fs, n, amp)
    print(f"{fs}: P = {np.abs(x).max():.7f}, TP host = {lim[0]:.7f}, TP float64 table = {LR.true_peak(x, u):.7f}, "
          f"unfaded interior = {np.abs(LR.oversample(raw, fs)[4 * 1000:4 * 3000]).max():.7f}, unfaded = {pkg.limiter_host(raw, fs, 1.0, 0.0)[1][0]:.7f}")
    assert abs(np.abs(x).max() - amp / np.sqrt(2)) <= 1e-7
    assert abs(lim[0] / amp - 1) <= 1e-4
    assert abs(LR.true_peak(x, u) / amp - 1) <= 1e-4
    # limiting to the sample peak's level: the sample-peak rule would do nothing, the true-peak limiter turns the row down by sqrt(2)
    c = amp / np.sqrt(2) * 1.001
    y, lim = pkg.limiter_host(x, fs, 1.0, db(c))
    assert abs(lim[2] - c / amp) <= 1e-3 * lim[2] and lim[1] <= c * (1 + 1e-3)


@pytest.mark.parametrize("fs", RATES)
@pytest.mark.parametrize("stage", ("hold", "smooth"))
def test_the_gpu_bound_catches_a_lost_stage(pkg, fs, stage):
    """the restatement with the hold taken out (H = 0), or with the look-back mean taken out (s = m): every GPU test compares y against the restatement
    within 6 * 2^-24 relative per sample; either loss moves samples by more than a tenth"""
    x = LR.sig_voiced(fs)
    want = ref(pkg, fs, "voiced", x, 2.0, 0.5)
    u = LR.oversample(x, fs, pkg.resample_taps(fs, 4 * fs))
    broken = LR.limiter(x, fs, 2.0, 0.5, u=u, hold=stage != "hold", smooth=stage != "smooth")
    nz = want["y"] != 0
    rel = np.abs(broken["y"][nz] - want["y"][nz]) / np.abs(want["y"][nz])
    print(f"{fs} without {stage}: worst relative error {rel.max():.3f}, {100 * (rel > Y_BOUND).mean():.1f} % of the samples over the bound, peak {np.abs(broken['y']).max():.4f}")
    assert rel.max() > 0.1 and (rel > Y_BOUND).mean() > 0.25
    # (the ceiling alone would NOT show it: both broken variants still hold |y| <= c)
    assert np.abs(broken["y"]).max() <= 0.5 * (1 + 1e-12)


def test_refusals_and_prototypes(pkg):
    for fs in (3999, 48001, 96000):
        with pytest.raises(pkg.VitsError, match=str(fs)):
            pkg.limiter_plan(fs)
        with pytest.raises(pkg.VitsError, match=str(fs)):
            pkg.limiter_host(np.zeros(8, np.float32), fs, 1.0, -1.0)
    for g0, cdb in ((0.0, -1.0), (-1.0, -1.0), (float("nan"), -1.0), (1.0, 0.5), (1.0, -61.0), (1.0, float("nan"))):
        with pytest.raises(pkg.VitsError, match="vits_limiter_host"):
            pkg.limiter_host(np.zeros(8, np.float32), 16000, g0, cdb)
    L = pkg.lib()
    assert L.vits_limiter_host(None, 4, 16000, 1.0, -1.0, None, None) == -1 and "null" in pkg.last_error()
    assert L.vits_limiter_host(None, 0, 16000, 1.0, -1.0, None, None) == 0  # (an empty row, nothing asked for)
    assert L.vits_limiter_plan(16000, None, None, None) == 0
    assert (pkg.LIMIT_OFF, pkg.LIMIT_TRUE_PEAK) == (0, 1)
    for name in ("vits_model_set_limiter", "vits_model_get_limiter", "vits_model_last_limits", "vits_limiter_plan", "vits_limiter_host", "vits_op_limit"):
        assert hasattr(L, name) and name in pkg.EXPORTED_SYMBOLS
    assert C.sizeof(pkg.LimitDesc) == C.sizeof(pkg.LevelDesc) + 8  # vits_level_desc + mode, padded to its 8-byte alignment
