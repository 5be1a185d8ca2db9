"""The resampling filter of include/vits.h (vits_model_set_rates), restated in float64 numpy: np.i0, np.sinc and the index rule, nothing else.
Shared by tests/test_resample_host.py (the product's table against this one; what the filter does to sinusoids) and the GPU tests (the
float64 value of every output sample and the magnitude sum of its error bound)."""
import math

import numpy as np

ZEROS, ROLLOFF, BETA = 32.0, 0.92, 9.0


def plan(fi, fo):
    """(L, M, R, K, s, W) of fi -> fo"""
    d = math.gcd(fi, fo)
    L, M = fo // d, fi // d
    s = ROLLOFF * min(1.0, L / M)
    W = ZEROS / s
    R = int(math.ceil(W))
    return L, M, R, 2 * R + 1, s, W


def taps(fi, fo):
    """h [L, K] in float64: h[p][k] = g(R - k + p / L), g(t) = s sinc(s t) I0(beta sqrt(1 - (t / W)^2)) / I0(beta) inside |t| < W"""
    L, M, R, K, s, W = plan(fi, fo)
    t = (R - np.arange(K, dtype=np.float64))[None, :] + (np.arange(L, dtype=np.float64) / L)[:, None]
    inside = np.abs(t) < W
    u = np.where(inside, t / W, 0.0)
    g = s * np.sinc(s * t) * np.i0(BETA * np.sqrt(1.0 - u * u)) / np.i0(BETA)
    return np.where(inside, g, 0.0)


def out_len(fi, fo, n):
    L, M = plan(fi, fo)[:2]
    return (n * L + M - 1) // M


def resample(x, fi, fo, h=None, with_bound=False):
    """y[j] = sum_k h[p][k] x[n_c - R + k] in float64, x = 0 outside [0, N); q = j M, n_c = q // L, p = q % L. h: another table (e.g. the product's
    fp32 one) instead of taps(fi, fo). with_bound: also sum_k |h[p][k]| |x[.]|, the magnitude sum of the rounding-error bound."""
    L, M, R, K = plan(fi, fo)[:4]
    h = taps(fi, fo) if h is None else np.asarray(h, np.float64)
    x = np.asarray(x, np.float64)
    N = x.size
    n_out = out_len(fi, fo, N)
    xp = np.concatenate([np.zeros(R), x, np.zeros(R + 1)])  # xp[i] = x[i - R]
    q = np.arange(n_out, dtype=np.int64) * M
    nc, p = q // L, q % L
    y = np.zeros(n_out)
    mag = np.zeros(n_out)
    for k in range(K):
        xv = xp[nc + k]  # x[n_c - R + k]
        hv = h[p, k]
        y += hv * xv
        if with_bound:
            mag += np.abs(hv) * np.abs(xv)
    return (y, mag) if with_bound else y
