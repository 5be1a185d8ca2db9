"""The edges stage of include/vits.h (vits_model_set_edges), restated in float64 numpy: the sample counts, the 10 ms windows and their mean squares, the
threshold, the bounds, the two fade tables, and the delivered row as fp32 with the two stated multiplies, so that y is comparable bit for bit. A desc is
the keyword arguments of pkg.set_edges / pkg.edges: mode, threshold_db, keep_head_ms, keep_tail_ms, fade_in_ms, fade_out_ms, lead_ms, tail_ms.
`defect` switches in one of the mistakes a broken implementation would make, for the tests that show the signals expose it.

The signals at 16 kHz (W = 160) are built from exact zeros, a floor of seeded noise at -70 dB and bursts at -20 dB whose samples all have the magnitude
0.1 (random signs): a window that holds ONE burst sample among floor samples has q = 0.01 / 160 = -42 dB, a full one -20 dB, a floor one -70 dB. The
tests' thresholds (RELATIVE -35 dB: T = -55 dB; ABSOLUTE -55 dB) lie 13 dB or more from every one of them."""
import math

import numpy as np

OFF, PAD, TRIM_RELATIVE, TRIM_ABSOLUTE = 0, 1, 2, 3
FS = 16000
FIELDS = ("keep_head_ms", "keep_tail_ms", "fade_in_ms", "fade_out_ms", "lead_ms", "tail_ms")


def samples(ms, fs):
    """(int64) floor((double) ms * fs / 1000 + 0.5), ms an fp32 field"""
    return int(math.floor(float(np.float32(ms)) * fs / 1000 + 0.5))


def plan(fs, **desc):
    """dict(W, Kh, Kt, Fi, Fo, Pl, Pt)"""
    p = {"W": (fs + 50) // 100}
    for short, name in zip(("Kh", "Kt", "Fi", "Fo", "Pl", "Pt"), FIELDS):
        p[short] = samples(desc.get(name, 0.0), fs)
    return p


def fade(F):
    """0.5 - 0.5 cos(pi (k + 0.5) / F) in double (libm's cos), rounded once to fp32"""
    return np.array([0.5 - 0.5 * math.cos(math.pi * (k + 0.5) / F) for k in range(F)], np.float64).astype(np.float32)


def window_q(x, W, partial=True):
    """q_i: the mean of x^2 over window i in float64; the partial last window counts, over its own samples"""
    x = np.asarray(x, np.float32).astype(np.float64)
    n_win = -(-x.size // W) if partial else x.size // W
    return np.array([np.mean(x[i * W:min((i + 1) * W, x.size)] ** 2) for i in range(n_win)], np.float64)


def threshold(q, mode, threshold_db):
    f = 10.0 ** (float(np.float32(threshold_db)) / 10.0)
    if mode == TRIM_ABSOLUTE:
        return f
    with np.errstate(invalid="ignore"):
        q_max = float(np.fmax.reduce(q, initial=0.0)) if q.size else 0.0  # (a NaN is dropped)
    return q_max * f


def edges(x, fs, mode=PAD, threshold_db=0.0, defect=None, **desc):
    """(y float32 [N'], row int64 [4] = a, b, N', n_active). defect: None | "keep" (the keep margins dropped) | "partial" (the partial last window
    dropped) | "strict" (> in place of >=) | "fade_end" (the fade-out indexed from the row's start)"""
    x = np.asarray(x, np.float32)
    N, p = x.size, plan(fs, **desc)
    W = p["W"]
    a = b = n_active = 0
    if mode == PAD:
        b = N
    else:
        q = window_q(x, W, partial=defect != "partial")
        T = threshold(q, mode, threshold_db)
        with np.errstate(invalid="ignore"):
            active = ((q > T) if defect == "strict" else (q >= T)) & (q > 0)
        idx = np.flatnonzero(active)
        n_active = int(idx.size)
        if n_active:
            Kh, Kt = (0, 0) if defect == "keep" else (p["Kh"], p["Kt"])
            a, b = max(0, int(idx[0]) * W - Kh), min(N, (int(idx[-1]) + 1) * W + Kt)
    M = b - a
    k = np.arange(M)
    wi, wo = np.ones(M, np.float32), np.ones(M, np.float32)
    win, wout = fade(p["Fi"]), fade(p["Fo"])
    wi[:min(M, p["Fi"])] = win[:min(M, p["Fi"])]
    r = k if defect == "fade_end" else M - 1 - k
    sel = r < p["Fo"]
    wo[sel] = wout[r[sel]]
    mid = (x[a:b] * wi) * wo  # two fp32 multiplies
    y = np.concatenate([np.zeros(p["Pl"], np.float32), mid.astype(np.float32), np.zeros(p["Pt"], np.float32)])
    return y, np.array([a, b, p["Pl"] + M + p["Pt"], n_active], np.int64)


def margin(x, fs, mode=PAD, threshold_db=0.0, **desc):
    """the smallest |q_i / T - 1| over the windows: how far every decision of the stage is from flipping. The fp64 sum of at most 1920 exact squares moves
    q by less than 1e-12 relative whatever its association, so with margin >= 1e-6 every implementation of the definition finds the same active windows.
    inf under PAD (nothing is measured) and when T == 0 (only q_i > 0 decides, and a sum of squares is 0 iff every sample is). At threshold_db == 0 under
    TRIM_RELATIVE T is q_max itself: the loudest window compares equal to its own value in any implementation, and is left out."""
    if mode == PAD:
        return math.inf
    q = window_q(x, (fs + 50) // 100)
    T = threshold(q, mode, threshold_db)
    if T == 0.0 or q.size == 0:
        return math.inf
    if mode == TRIM_RELATIVE and float(np.float32(threshold_db)) == 0.0:
        q = np.delete(q, int(np.argmax(q)))
    return float(np.abs(q / T - 1.0).min()) if q.size else math.inf


# ---- the test signals ---------------------------------------------------------------------------------------------------------------------
FLOOR, BURST = 10.0 ** (-70.0 / 20.0), 0.1
THRESHOLDS = ((TRIM_RELATIVE, -35.0), (TRIM_ABSOLUTE, -55.0))


def floor(n, seed=11):
    return (FLOOR * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def burst(x, lo, hi, seed=12):
    """samples [lo, hi) of x become +-0.1"""
    x[lo:hi] = np.float32(BURST) * np.random.default_rng(seed).choice(np.array([-1.0, 1.0], np.float32), hi - lo)
    return x


def sig_onset(n, onset, end, zeros_head=0, seed=11):
    """floor, a burst over [onset, end), and `zeros_head` exact zeros at the start"""
    x = burst(floor(n, seed), onset, end, seed + 1)
    x[:zeros_head] = 0.0
    return x


def signals(W=160, n=4000):
    """name -> row at 16 kHz. onset_*: an onset exactly on a window edge and one sample either side of it; partial_last: a burst in the partial last window
    only; silent_zeros / silent_floor / all_active; single: one active window; ends_at_n: a burst that ends at N"""
    assert n % W == 0 and n >= 12 * W
    out = {
        "onset_edge": sig_onset(n, 5 * W, 9 * W, zeros_head=W),
        "onset_before": sig_onset(n, 5 * W - 1, 9 * W + 1, seed=21),
        "onset_after": sig_onset(n, 5 * W + 1, 9 * W - 1, seed=31),
        "partial_last": sig_onset(n + 7, n, n + 7, seed=41),
        "silent_zeros": np.zeros(n, np.float32),
        "silent_floor": floor(n + 3, 51),
        "all_active": burst(np.zeros(n + W // 2, np.float32), 0, n + W // 2, 61),
        "single": sig_onset(n, 7 * W, 8 * W, seed=71),
        "ends_at_n": sig_onset(n + 33, 6 * W, n + 33, seed=81),
    }
    return out
