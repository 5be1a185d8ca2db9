"""numpy side of the operator tests of the stochastic duration predictor's kernels (tests/test_gpu_dds_ops.py, tests/test_gpu_spline_ops.py,
tests/test_dp_op_host.py): a DDS block, the inverse rational-quadratic spline of a conv flow, and the durations, each restated from the project's own kernels
(vits.cpp_amd/csrc/dds.hip, spline.hip, stage1_lat.hip), their comments and the published definition of the model (transformers modeling_vits.py).

Every function takes a `dtype`: float64 is the reference, float32 the "restatement" — the same statements with every tensor and every operation in fp32, whose
error against float64 is the yardstick of the GPU tests (the 2x rule of tests/split_ref.py). Nothing here knows how a kernel tiles its work."""
import math

import numpy as np

import split_ref as R

F32, BF16, F16 = 0, 1, 2  # pkg.ARITH_*
MODE_REFERENCE, MODE_HF = 0, 1
_erf = np.frompyfunc(math.erf, 1, 1)


def round_arith(v, arith):
    """round_arith of kernel_common.h: a conv operand in the 16-bit arithmetics is rounded (nearest even) to fp16 / bf16"""
    if arith == F16:
        return np.asarray(v).astype(np.float16).astype(np.float32)
    if arith == BF16:
        return R.bf16_rne(np.asarray(v, np.float32))
    return v


def gelu(v, dtype):
    """exact-erf GELU: 0.5 v (1 + erf(v / sqrt 2)); erf itself is taken in float64 and rounded to dtype (a correctly rounded erf)"""
    v = np.asarray(v, dtype)
    e = _erf((v * dtype(0.70710678118654752440)).astype(np.float64)).astype(np.float64).astype(dtype)
    return dtype(0.5) * v * (dtype(1) + e)


def mm(w, h):
    """a 1x1 conv, w [rows, channels] on h [channels, columns], every product and sum in the operands' type (einsum: no BLAS call, whose thread pool
    costs more than the product at these sizes)"""
    return np.einsum("oc,ct->ot", w, h)


def layer_norm(h, g, b, eps, dtype):
    """LayerNorm over the channels (axis 0) of every column: biased variance, eps inside the square root"""
    H = dtype(h.shape[0])
    mean = h.sum(axis=0, dtype=dtype) / H
    d = h - mean
    var = (d * d).sum(axis=0, dtype=dtype) / H
    inv = dtype(1) / np.sqrt(var + dtype(eps))
    return d * inv * g[:, None] + b[:, None]


def make_params(H, k, layers, seed, tail_rows=0, bias_rows=3):
    """One DDS block's parameters and both heads' and the tail's: fp16-valued 1x1 weights scaled by 1 / sqrt(fan_in), depthwise taps ~ N(0, 1 / k), LayerNorm
    weights around 1, biases 0.1 sigma; head_conv_b is a `bias_rows`-row table."""
    rng = np.random.default_rng(seed)
    f16 = lambda a: a.astype(np.float16).astype(np.float32)
    n = lambda *s: rng.standard_normal(s)
    P = dict(dw_w=(n(layers, H, k) / np.sqrt(k)).astype(np.float32), dw_b=(0.1 * n(layers, H)).astype(np.float32),
             g1=(1 + 0.1 * n(layers, H)).astype(np.float32), b1=(0.1 * n(layers, H)).astype(np.float32),
             pw_w=f16(n(layers, H, H) / np.sqrt(H)), pw_b=(0.1 * n(layers, H)).astype(np.float32),
             g2=(1 + 0.1 * n(layers, H)).astype(np.float32), b2=(0.1 * n(layers, H)).astype(np.float32),
             from1_w=n(H).astype(np.float32), from1_b=(0.1 * n(H)).astype(np.float32),
             conv_w=f16(n(H, H) / np.sqrt(H)), conv_b=(0.1 * n(bias_rows, H)).astype(np.float32))
    if tail_rows:
        P["tail_w"] = f16(n(tail_rows, H) / np.sqrt(H))
        P["tail_b"] = (0.1 * n(tail_rows)).astype(np.float32)
    return P


def dds_block(P, lens, dtype, x=None, z=None, cond=None, zc=0, head=0, bias_rows=None, tail=False, eps=1e-5, arith=F32):
    """The block on a ragged batch: x [B, H, T] (head 0 and 2), or z [B, 2, T] and cond [B, H, T] (head 1); columns t < lens[b] are the utterance, everything
    else is zero padding. Layer i: depthwise conv with dilation k^i and (k - 1) k^i / 2 zeros on both sides (bias first, then the taps in ascending order),
    LayerNorm, GELU, 1x1 conv, LayerNorm, GELU, residual. In a 16-bit arithmetic the operands of every conv (depthwise, 1x1, head, tail) are rounded as
    round_arith does; everything else stays in dtype. Returns (y [H, columns], y2 [R, columns] or None), the valid columns of the batch side by side."""
    layers, H, k = P["dw_w"].shape
    c = lambda a: np.asarray(a, dtype)
    q = lambda a: c(round_arith(np.asarray(a, np.float32), arith)) if arith != F32 else c(a)
    # (an fp32 value between layers is what a 16-bit conv rounds: in float64 the rounding is applied to the fp32 rounding of the value)
    ys, y2s = [], []
    for b, n in enumerate(lens):
        if n == 0:
            continue
        if head == 1:
            cur = q(P["from1_w"])[:, None] * q(z[b, zc, :n])[None, :] + c(P["from1_b"])[:, None]
            cur = cur + c(cond[b, :, :n])
        elif head == 2:
            row = 0 if bias_rows is None else int(bias_rows[b])
            cur = mm(q(P["conv_w"]), q(x[b, :, :n])) + c(P["conv_b"][row])[:, None]
        else:
            cur = c(x[b, :, :n])
        for i in range(layers):
            dil = k ** i
            pad = (k * dil - dil) // 2
            xp = np.zeros((H, n + (k - 1) * dil), dtype)
            xp[:, pad:pad + n] = q(cur)
            w = q(P["dw_w"][i])
            h = np.repeat(c(P["dw_b"][i])[:, None], n, axis=1)
            for j in range(k):
                h = h + w[:, j:j + 1] * xp[:, j * dil:j * dil + n]
            h = gelu(layer_norm(h, c(P["g1"][i]), c(P["b1"][i]), eps, dtype), dtype)
            h = mm(q(P["pw_w"][i]), q(h)) + c(P["pw_b"][i])[:, None]
            h = gelu(layer_norm(h, c(P["g2"][i]), c(P["b2"][i]), eps, dtype), dtype)
            cur = cur + h
        ys.append(cur)
        if tail:
            y2s.append(mm(q(P["tail_w"]), q(cur)) + c(P["tail_b"])[:, None])
    return np.concatenate(ys, axis=1), (np.concatenate(y2s, axis=1) if tail else None)


# ---- the spline ------------------------------------------------------------------------------------------------------------------------------
def _softplus(x, dtype):
    """softplus_f of spline.hip: x beyond 20, else log(1 + exp(x)) taken in double and rounded to dtype"""
    x = np.asarray(x, dtype)
    return np.where(x > dtype(20), x, np.log(1.0 + np.exp(np.minimum(x, dtype(30)).astype(np.float64))).astype(dtype))


def _spline_rows(x, u, nb, B, inv_sqrt, mode, q4, masked, dtype):
    """spline_row of spline.hip on every token at once: x [T], u [3 nb - 1, T]; q4, masked: bool [T]"""
    T = x.size
    one, B = dtype(1), dtype(B)
    min_w = min_h = min_d = dtype(1e-3)
    u = np.asarray(u, dtype)
    x = np.asarray(x, dtype)

    def knots(rows, widths):
        v = np.where(masked[None, :], dtype(0), rows * dtype(inv_sqrt))
        v = np.exp(v - v.max(axis=0))
        v = v / v.sum(axis=0, dtype=dtype)
        if widths and mode == MODE_REFERENCE:
            v = v * (min_w + (one - min_w * dtype(nb)))  # (Q3: the reference scales the widths and never adds the minimum)
        else:
            v = min_w + (one - min_w * dtype(nb)) * v
        cum = np.zeros((nb + 1, T), dtype)
        run = np.zeros(T, dtype)
        for i in range(nb):
            run = run + v[i]
            cum[i + 1] = run
        cum = (B - (-B)) * cum + (-B)
        cum[0] = -B
        cum[nb] = np.where(q4, cum[nb], B)  # (Q4: the last token's row keeps the computed end knot)
        return cum, cum[1:] - cum[:-1]

    cw, W = knots(u[:nb], True)
    ch, Hh = knots(u[nb:2 * nb], False)
    loc = ch.copy()
    loc[nb] = np.where(q4, loc[nb], loc[nb] + dtype(1e-6))
    bins = np.clip((x[None, :] >= loc).sum(axis=0) - 1, 0, nb - 1)
    constant = dtype(math.log(math.exp(1.0 - 1e-3) - 1.0))
    ud = np.zeros((nb + 1, T), dtype)
    ud[0] = constant
    ud[nb] = np.where(q4, dtype(0), constant)
    ud[1:nb] = u[2 * nb:3 * nb - 1]
    ud = np.where(masked[None, :], dtype(0), ud)
    D = min_d + _softplus(ud, dtype)
    take = lambda a, idx: np.take_along_axis(a, idx[None, :], axis=0)[0]
    in_cw, in_w, in_ch, in_h = take(cw, bins), take(W, bins), take(ch, bins), take(Hh, bins)
    d0, d1 = take(D, bins), take(D, bins + 1)
    delta = in_h / in_w
    i1 = d0 + d1 - dtype(2) * delta
    i2 = x - in_ch
    i3 = i2 * i1
    a = in_h * (delta - d0) + i3
    bq = in_h * d0 - i3
    cc = -delta * i2
    disc = bq * bq - dtype(4) * a * cc
    root = (dtype(2) * cc) / (-bq - np.sqrt(disc))
    return root * in_w + in_cw


def spline_sources(z_row, tail):
    """Reference mode's masked get / set pair (Q6) as an index map: (inside [T] bool, src [T] int). The k-th inside token receives the spline result of token
    src = k; the j-th outside token receives element src = j of the masked input [x_t if inside_t else 0]."""
    x = np.asarray(z_row, np.float32)
    inside = (x >= -np.float32(tail)) & (x <= np.float32(tail))
    src = np.where(inside, np.cumsum(inside) - 1, np.cumsum(~inside) - 1)
    return inside, src.astype(np.int64)


def spline(z_row, u, bins, tail, inv_sqrt, mode, dtype):
    """The inverse rational-quadratic spline on one utterance: z_row [T] (fp32 values), u [3 bins - 1, T]. MODE_HF: identity outside [-tail, tail], bounds
    inclusive. MODE_REFERENCE: the reference's width scaling (Q3), the last token's row without its end knot and end derivative (Q4), and the masked get / set
    pair (Q6): every token goes through the spline, an outside one as input 0 with zeroed parameters; see spline_sources. Returns [T] in dtype."""
    x32 = np.asarray(z_row, np.float32)
    T = x32.size
    inside = (x32 >= -np.float32(tail)) & (x32 <= np.float32(tail))
    x = x32.astype(dtype)
    if mode == MODE_HF:
        no = np.zeros(T, bool)
        r = _spline_rows(np.where(inside, x, dtype(0)), u, bins, tail, inv_sqrt, mode, no, no, dtype)
        return np.where(inside, r, x)
    q4 = np.arange(T) == T - 1
    vals = np.where(inside, x, dtype(0))
    res = _spline_rows(vals, u, bins, tail, inv_sqrt, mode, q4, ~inside, dtype)
    _, src = spline_sources(x32, tail)
    return np.where(inside, res[src], vals[src])


def make_spline_case(T, bins, seed, scale=1.0, outside=()):
    """u [3 bins - 1, T] ~ N(0, 1) x scale (x 8: sharp bins), z_row uniform in (-0.98 tail, 0.98 tail) with the tokens of `outside` moved beyond the interval
    (alternating sides, distinct values), tail = 5"""
    rng = np.random.default_rng(seed)
    tail = 5.0
    u = (scale * rng.standard_normal((3 * bins - 1, T))).astype(np.float32)
    zr = rng.uniform(-0.98 * tail, 0.98 * tail, T).astype(np.float32)
    for j, t in enumerate(outside):
        zr[t] = np.float32((tail + 0.25 + 0.001 * j) * (1 if j % 2 == 0 else -1))
    return u, zr, tail


# ---- durations ---------------------------------------------------------------------------------------------------------------------------------
INT_MAX = 0x7FFFFFFF


def durations(logw_row, lens, length_scale=1.0, length_scales=None, overrides=None, fixed=0, stage_mul=(), stage_add=()):
    """d = ceil(exp(logw) * scale) in float64 on the fp32 inputs, overrides >= 0 and `fixed` > 0 replace it; inclusive per-utterance sums; frames =
    max(1, sum); stage_lens[s][b] = frames[b] * stage_mul[s] + stage_add[s]; behind lens[b]: dur 0, cum INT_MAX. Exact integers. Also returns the float64
    products (before ceil) of the tokens whose duration is the prediction, for the distance-from-integer check."""
    logw_row = np.asarray(logw_row, np.float32)
    B, ts = logw_row.shape
    dur = np.zeros((B, ts), np.int64)
    cum = np.full((B, ts), INT_MAX, np.int64)
    frames = np.zeros(B, np.int64)
    products = []
    for b in range(B):
        n = int(lens[b])
        ls = np.float64(np.float32(length_scale if length_scales is None else length_scales[b]))
        prod = np.exp(logw_row[b, :n].astype(np.float64)) * ls
        d = np.ceil(prod).astype(np.int64)
        predicted = np.ones(n, bool)
        if overrides is not None:
            o = np.asarray(overrides[b, :n], np.int64)
            d = np.where(o >= 0, o, d)
            predicted &= o < 0
        if fixed > 0:
            d[:] = fixed
            predicted[:] = False
        products.append(prod[predicted])
        dur[b, :n] = d
        cum[b, :n] = np.cumsum(d)
        frames[b] = max(1, int(d.sum()))
    sl = np.array([[int(frames[b]) * int(m) + int(a) for b in range(B)] for m, a in zip(stage_mul, stage_add)], np.int64).reshape(len(stage_mul), B)
    return dur, cum, frames, sl, np.concatenate(products) if products else np.zeros(0)


def make_logw(lens, ts, scales, seed, rows=2, row=1):
    """logw [B, rows, ts]: row `row` = log((n + f) / scale_b), n in 0..11, f uniform in [0.05, 0.95] — the product exp(logw) * scale then keeps a distance of 0.05
    from every integer, far beyond any fp32 error of expf and the product; the other rows and everything behind lens[b] are NaN"""
    rng = np.random.default_rng(seed)
    B = len(lens)
    logw = np.full((B, rows, ts), np.nan, np.float32)
    for b in range(B):
        n = rng.integers(0, 12, lens[b])
        f = rng.uniform(0.05, 0.95, lens[b])
        logw[b, row, :lens[b]] = np.log((n + f) / np.float64(np.float32(scales[b]))).astype(np.float32)
    return logw
