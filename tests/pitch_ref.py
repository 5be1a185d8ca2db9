"""The varispeed of include/vits.h ("a stated pitch"), restated in float64 numpy: the integers of a row, the prototype and its two tables, the tap rule and
the sum, nothing else. Shared by tests/test_pitch_host.py (the product's plan, tables and host evaluation against this one; what the filter does to
sinusoids and how far the table lies from the exact sinc) and the GPU tests (the float64 value of every output sample and the magnitude sum of its error
bound)."""
import numpy as np

Z, Q, BETA = 32, 256, 9.0
ZQ = Z * Q
ONE = 1 << 24
S0 = 15435038  # floor(0.92 2^24)


def ratio(semitones):
    """(float)exp2((double)semitones / 12)"""
    return float(np.float32(2.0 ** (float(semitones) / 12.0)))


def plan(p, n):
    """(P, S, R, K, N') of a row of n samples at ratio p (a float32 value in [0.5, 2])"""
    P = int(float(np.float32(p)) * ONE)
    assert P == float(np.float32(p)) * ONE and (ONE >> 1) <= P <= (ONE << 1)
    S = S0 if P <= ONE else (S0 << 24) // P
    R = -((-(1 << 29)) // S)
    return P, S, R, 2 * R + 1, -((-n * ONE) // P)


def g0(u):
    """the prototype in float64: sinc(u) I0(beta sqrt(1 - (u / Z)^2)) / I0(beta) inside |u| < Z, else 0"""
    u = np.asarray(u, np.float64)
    inside = np.abs(u) < Z
    w = np.where(inside, u / Z, 0.0)
    return np.where(inside, np.sinc(u) * np.i0(BETA * np.sqrt(1.0 - w * w)) / np.i0(BETA), 0.0)


def table():
    """(G, D) float32 [Z Q + 2] each: G[i] = fp32(g0(i / Q)), G[Z Q] = G[Z Q + 1] = 0; D[i] = G[i + 1] - G[i] in fp32, D[Z Q + 1] = 0"""
    G = np.zeros(ZQ + 2, np.float32)
    G[:ZQ] = g0(np.arange(ZQ) / Q).astype(np.float32)
    D = np.zeros(ZQ + 2, np.float32)
    D[:ZQ + 1] = G[1:] - G[:-1]
    return G, D


def weights(p, n, tables=None, exact=False):
    """(h float64 [N', K], idx int64 [N', K]): the weight of every tap of every output sample of a row of n samples, and the input sample it meets.
    tables: (G, D) to interpolate in (default: table()); exact: g0 itself at the tap's exact position instead of the table."""
    P, S, R, K, n_out = plan(p, n)
    t = np.arange(n_out, dtype=np.int64) * P
    n0, f = t >> 24, t & (ONE - 1)
    k = np.arange(K, dtype=np.int64)
    tau = np.abs((k[None, :] - R) * ONE - f[:, None])
    a = S / ONE
    if exact:
        h = a * g0(tau.astype(np.float64) * S / 2.0 ** 48)
    else:
        G, D = table() if tables is None else tables
        u = (tau * S) >> 24
        i = u >> 16
        fr = (u & 65535).astype(np.float64) / 65536.0
        ic = np.minimum(i, ZQ)
        h = np.where(i >= ZQ, 0.0, a * (fr * D[ic].astype(np.float64) + G[ic].astype(np.float64)))
    return h, n0[:, None] - R + k[None, :]


def pitch(x, p, tables=None, exact=False, with_bound=False):
    """y[m] = sum_k h x[n0 - R + k] in float64, x = 0 outside [0, N); a row at ratio 1 is copied. with_bound: also sum_k |h| |x|, the magnitude sum of
    the rounding-error bound."""
    x = np.asarray(x, np.float64)
    if plan(p, x.size)[0] == ONE:
        return (x.copy(), np.abs(x)) if with_bound else x.copy()
    h, idx = weights(p, x.size, tables, exact)
    inside = (idx >= 0) & (idx < x.size)
    xv = np.where(inside, x[np.clip(idx, 0, max(x.size - 1, 0))] if x.size else 0.0, 0.0)
    y = (h * xv).sum(axis=1)
    return (y, (np.abs(h) * np.abs(xv)).sum(axis=1)) if with_bound else y
