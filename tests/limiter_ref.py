"""The true-peak limiter of include/vits.h (vits_model_set_limiter), restated in float64 numpy: the 4x oversampled row by tests/resample_ref.py (or handed
in: the GPU tests feed the device's own), the envelope, r, the sliding minimum as a plain window minimum, the mean, the multiply. Nothing is rounded to
fp32. `hold` and `smooth` switch the two stages off that a broken kernel would lose, for the tests that show the bounds catch it."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import resample_ref as RR


def constants(fs):
    """(A, H): 5 ms of look-ahead and attack, 50 ms of hold, in samples (truncating divisions)"""
    return (fs + 100) // 200, (fs + 10) // 20


def oversample(x, fs, h=None):
    """u [4 N]: x at four times its rate by the project's filter; h: another table [4, K] (the product's fp32 one) instead of the float64 one"""
    x = np.asarray(x, np.float64)
    return RR.resample(x, fs, 4 * fs, h) if x.size else np.zeros(0)


def true_peak(x, u):
    x, u = np.asarray(x, np.float64), np.asarray(u, np.float64)
    return max(np.abs(x).max() if x.size else 0.0, np.abs(u).max() if u.size else 0.0)


def envelope(x, u):
    """e[n] = max(|x[n]|, |u[j]| for j in [4n - 2, 4n + 2] inside [0, 4N))"""
    x, u = np.asarray(x, np.float64), np.asarray(u, np.float64)
    N = x.size
    assert u.size == 4 * N
    au = np.concatenate([np.zeros(2), np.abs(u), np.zeros(2)])  # au[j + 2] = |u[j]|
    e = np.abs(x)
    for d in range(-2, 3):
        e = np.maximum(e, au[4 * np.arange(N) + d + 2])
    return e


def limiter(x, fs, g0, c, u=None, hold=True, smooth=True):
    """dict(y, s, r, m, e) of one row, all float64. m[j + A] is the minimum of r over [j - H, j + A], j in [-A, N). hold=False: H = 0. smooth=False: s = m
    at the sample itself (the mean over one value)."""
    x = np.asarray(x, np.float64)
    N = x.size
    A, H = constants(fs)
    if not hold:
        H = 0
    u = oversample(x, fs) if u is None else np.asarray(u, np.float64)
    e = envelope(x, u)
    with np.errstate(divide="ignore", over="ignore"):
        r = np.where(e == 0.0, 1.0, np.minimum(1.0, c / (float(g0) * np.where(e == 0.0, 1.0, e))))
    rp = np.concatenate([np.ones(A + H), r, np.ones(A)])  # rp[k + A + H] = r[k]
    m = sliding_window_view(rp, H + A + 1).min(axis=1) if N else np.ones(A)
    assert m.size == N + A
    if smooth:
        s = sliding_window_view(m, A + 1).mean(axis=1) if N else np.zeros(0)  # m[n - A .. n]
    else:
        s = m[A:].copy()
    assert s.size == N
    return {"y": x * (float(g0) * s), "s": s, "r": r, "m": m, "e": e}


def limits(x, u, y, uy, s):
    """the row [TP(x), TP(y), min s, share of s < 1]"""
    return np.array([true_peak(x, u), true_peak(y, uy), s.min() if s.size else 1.0, float((s < 1.0).mean()) if s.size else 0.0])


# ---- the test signals -----------------------------------------------------------------------------------------------------------------
def sig_voiced(fs, seconds=0.4, f0=110.0, seed=5):
    """a pulse train through harmonics with aligned phases (crest about 12 dB) under a slow swell, and a little noise"""
    t = np.arange(int(round(fs * seconds)), dtype=np.float64) / fs
    k = np.arange(1, int(0.45 * fs / f0))
    v = (np.cos(2 * np.pi * f0 * t[:, None] * k[None, :]) / k[None, :] ** 0.7).sum(axis=1)
    v *= 0.5 * (1.0 - np.cos(2 * np.pi * t / seconds)) / np.abs(v).max()
    return (0.9 * v + 0.002 * np.random.default_rng(seed).standard_normal(t.size)).astype(np.float32)


def sig_noise(n, amp=0.2, seed=6):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def sig_peaks(n, tile, amp=0.9, floor=0.02, seed=7):
    """a quiet floor with one peak at sample 0, at n - 1 and on both sides of every tile edge inside the row"""
    x = (floor * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)
    at = [0, n - 1] + [e + d for e in range(tile, n + 1, tile) for d in (-1, 0)]
    for i, p in enumerate(at):
        if 0 <= p < n:
            x[p] = amp * (-1.0) ** i
    return x


def sig_quarter_sine(fs, n, amp=0.5, fade=None):
    """a sine at fs / 4 with phase pi / 4: every sample is amp / sqrt(2) in magnitude, the waveform between them reaches amp. Faded in and out over
    `fade` samples (raised cosine): an abrupt start rings."""
    i = np.arange(n, dtype=np.float64)
    x = amp * np.sin(np.pi / 2 * i + np.pi / 4)
    if fade:
        w = 0.5 * (1.0 - np.cos(np.pi * np.minimum(np.minimum(i, n - 1 - i) / fade, 1.0)))
        x *= w
    return x.astype(np.float32)
