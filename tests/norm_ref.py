"""numpy side of the operator tests of the LayerNorm kernels (add_layer_norm_kernel and LayerNorm on load in conv_lat16_kernel: tests/test_gpu_norm_ops.py,
tests/test_encoder_op_host.py): the float64 reference, its restatement in sequential fp32 ("the chain" of tests/split_ref.py), ggml's fp16 GELU table, and the
data makers. No GPU.

Per column (b, t < lens[b]), over the channels c:  v = x [+ residual];  y = (v - mean(v)) / sqrt(var(v) + eps) * gamma + beta  (biased variance);
post_gelu: y = 0.5 y (1 + erf(y / sqrt 2)), or with a table y = tab[fp16(y)] (ggml's tanh-GELU table: fp16 bits in, fp16 value out).
The chain: the sum, then the sum of squared deviations, each a sequential fp32 sum over the channels in ascending order; one fp32 rounding per operation after that."""
import math

import numpy as np

import split_ref as R

FACTOR = R.FACTOR
MIN_OUTPUTS = 2000  # below this a case's rms ratio is noise: printed, not asserted

_erf = np.vectorize(math.erf, otypes=[np.float64])


def gelu_table():
    """ggml's table: entry i = fp16(tanh-GELU(the fp16 value with bits i)), as raw uint16"""
    x = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        y = 0.5 * x * (1.0 + np.tanh(0.79788456080286535587989211986876 * x * (1.0 + 0.044715 * x * x)))
        return y.astype(np.float16).view(np.uint16)


def table_lookup(tab, x):
    with np.errstate(over="ignore"):
        idx = np.asarray(x).astype(np.float16).view(np.uint16)
    return np.asarray(tab, np.uint16).view(np.float16)[idx].astype(np.float32)


def case_seed(C, T, offset):
    return (C * 4099 + T) * 2 + int(offset) + 1234


def make_case(C, T, B, offset=False):
    """x, residual ~ N(0, 1) [B, C, T] (offset: x ~ N(50, 1), where a one-pass variance E[v^2] - E[v]^2 would lose every digit in fp32), y0 ~ N(0, 1) (what add_to
    adds to), gamma ~ 1 + 0.1 N, beta ~ 0.5 N"""
    rng = np.random.default_rng(case_seed(C, T, offset))
    x = rng.standard_normal((B, C, T)).astype(np.float32)
    if offset:
        x = (x + np.float32(50)).astype(np.float32)
    res = rng.standard_normal((B, C, T)).astype(np.float32)
    y0 = rng.standard_normal((B, C, T)).astype(np.float32)
    gamma = (1 + 0.1 * rng.standard_normal(C)).astype(np.float32)
    beta = (0.5 * rng.standard_normal(C)).astype(np.float32)
    return x, res, y0, gamma, beta


def reference64(x, res, gamma, beta, eps, lens, gelu=False, gelu_tab=None):
    """float64 on the valid columns, [C, sum(lens)] (tests/split_ref.py gather_cols)"""
    v = R.gather_cols(x, lens).astype(np.float64)
    if res is not None:
        v = v + R.gather_cols(res, lens).astype(np.float64)
    mean = v.mean(axis=0, keepdims=True)
    var = ((v - mean) ** 2).mean(axis=0, keepdims=True)
    y = (v - mean) / np.sqrt(var + np.float64(np.float32(eps))) * gamma.astype(np.float64)[:, None] + beta.astype(np.float64)[:, None]
    if gelu_tab is not None:
        return table_lookup(gelu_tab, y).astype(np.float64)
    if gelu:
        y = 0.5 * y * (1.0 + _erf(y / math.sqrt(2.0)))
    return y


def chain32(x, res, gamma, beta, eps, lens, gelu=False, gelu_tab=None):
    """the fp32 restatement on the valid columns, fp32 [C, sum(lens)]"""
    f = np.float32
    v = R.gather_cols(x, lens).astype(f)
    if res is not None:
        v = (v + R.gather_cols(res, lens).astype(f)).astype(f)
    C = v.shape[0]
    s = np.zeros(v.shape[1], f)
    for c in range(C):
        s = (s + v[c]).astype(f)
    mean = (s / f(C)).astype(f)
    vs = np.zeros(v.shape[1], f)
    for c in range(C):
        d = (v[c] - mean).astype(f)
        vs = (vs + (d * d).astype(f)).astype(f)
    var = (vs / f(C)).astype(f)
    inv = (f(1) / np.sqrt((var + f(eps)).astype(f)).astype(f)).astype(f)
    y = ((((v - mean[None]).astype(f) * inv[None]).astype(f) * gamma.astype(f)[:, None]).astype(f) + beta.astype(f)[:, None]).astype(f)
    if gelu_tab is not None:
        return table_lookup(gelu_tab, y)
    if gelu:
        e = _erf((y * f(0.70710678118654752440)).astype(f).astype(np.float64)).astype(f)
        y = ((f(0.5) * y).astype(f) * (f(1) + e).astype(f)).astype(f)
    return y


def edge_columns(lens, tw):
    """mask over the gathered columns: the last column of every utterance and one column on each side of every tile boundary m tw inside it"""
    parts = []
    for n in lens:
        n = int(n)
        t = np.arange(n)
        m = t == n - 1
        for edge in range(tw, n, tw):
            m |= (t == edge - 1) | (t == edge)
        parts.append(m)
    return np.concatenate(parts) if parts else np.zeros(0, bool)
