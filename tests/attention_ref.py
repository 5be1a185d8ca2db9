"""numpy side of the operator tests of the text encoder's attention kernels (tests/test_gpu_attention_ops.py, tests/test_encoder_op_host.py): the float64
reference of the relative-position attention core, its restatement in sequential fp32 ("the chain" of tests/split_ref.py), ggml's fp16
exponential table, and the data makers. No GPU.

Per utterance b on [0, n), n = lens[b], per head, with q' = fp32(q * q_scale) (one deterministic rounding, the same on every side), w = window:
    s_ij = q'_i . k_j + [|j - i| <= w] q'_i . Ek[j - i + w];   p_i = softmax_j(s_i);   o_i = sum_j p_ij v_j + sum_{|j - i| <= w} p_ij Ev[j - i + w]
With a table: e_ij = tab[fp16(s_ij - max_j s_ij)] (fp16 bits in, fp16 value out), p_ij = e_ij / sum_j e_ij.

The chain: every dot product a sequential fmaf chain (over head_dim for the scores and the relative logits, over the keys in ascending order for the outputs, over
the relative positions for the relative-value term), the relative logit added to the score in fp32, the soft-max in fp32 (max, exp rounded to fp32, a sequential
sum, one reciprocal, one product per entry), the two output sums added in fp32. It is the yardstick of the 2x rule, not a model of any kernel's order.

Tensors are [B, heads * head_dim, T] as the kernels take them; results likewise, zero behind lens[b]."""
import numpy as np

import split_ref as R

FACTOR = R.FACTOR
MIN_OUTPUTS = 2000  # below this a case's rms ratio is noise: printed, not asserted


def exp_table():
    """ggml's table: entry i = fp16(exp(the fp16 value with bits i)), as raw uint16"""
    x = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.exp(x.astype(np.float64)).astype(np.float16).view(np.uint16)


def table_lookup(tab, x):
    """tab[fp16 bits of x] as fp32 (x: fp32 or float64, rounded to fp16 to nearest even, as GGML_FP32_TO_FP16 does)"""
    with np.errstate(over="ignore"):
        idx = np.asarray(x).astype(np.float16).view(np.uint16)
    return np.asarray(tab, np.uint16).view(np.float16)[idx].astype(np.float32)


def case_seed(hd, window, T, peaked):
    return ((hd * 131 + window) * 4099 + T) * 2 + int(peaked) + 77


def make_case(heads, hd, window, T, B, peaked=False):
    """q, k, v ~ N(0, 1) [B, heads * hd, T]; rel_k, rel_v ~ N(0, 1) [2 window + 1, hd]. peaked: q and k x 4, so that one key dominates a row."""
    rng = np.random.default_rng(case_seed(hd, window, T, peaked))
    q, k, v = (rng.standard_normal((B, heads * hd, T)).astype(np.float32) for _ in range(3))
    rel_k, rel_v = (rng.standard_normal((2 * window + 1, hd)).astype(np.float32) for _ in range(2))
    if peaked:
        q, k = q * np.float32(4), k * np.float32(4)
    return q, k, v, rel_k, rel_v


def _heads(x, heads):
    B, C, T = x.shape
    return x.reshape(B, heads, C // heads, T)


def _rel_index(T, window):
    """r[i, j] = j - i + window and the mask |j - i| <= window"""
    i = np.arange(T)
    r = i[None, :] - i[:, None] + window
    return r, (r >= 0) & (r <= 2 * window)


def _valid(lens, T):
    return np.arange(T)[None, :] < np.asarray(lens)[:, None]  # [B, T]


def reference64(q, k, v, rel_k, rel_v, heads, window, lens, q_scale=1.0, exp_tab=None):
    """float64, [B, C, T], zero behind lens[b]"""
    B, C, T = q.shape
    qs = _heads((q * np.float32(q_scale)).astype(np.float32), heads).astype(np.float64)
    kk, vv = _heads(k, heads).astype(np.float64), _heads(v, heads).astype(np.float64)
    ek, ev = rel_k.astype(np.float64), rel_v.astype(np.float64)
    r, win = _rel_index(T, window)
    rc = np.clip(r, 0, 2 * window)
    out = np.zeros((B, heads, C // heads, T))
    for b in range(B):
        n = int(lens[b])
        if n == 0:
            continue
        s = np.einsum("hdi,hdj->hij", qs[b, :, :, :n], kk[b, :, :, :n])
        qe = np.einsum("hdi,rd->hir", qs[b, :, :, :n], ek)  # [h, i, r]
        rr, ww = rc[:n, :n], win[:n, :n]
        s = s + np.where(ww[None], np.take_along_axis(qe, np.broadcast_to(rr[None], s.shape), axis=2), 0.0)
        x = s - s.max(axis=2, keepdims=True)
        e = table_lookup(exp_tab, x).astype(np.float64) if exp_tab is not None else np.exp(x)
        p = e / e.sum(axis=2, keepdims=True)
        o = np.einsum("hij,hdj->hdi", p, vv[b, :, :, :n])
        pw = np.zeros((heads, n, 2 * window + 1))  # pw[h, i, r] = p[h, i, i + r - w]
        for rel in range(2 * window + 1):
            j = np.arange(n) + rel - window
            ok = (j >= 0) & (j < n)
            pw[:, ok, rel] = p[:, np.arange(n)[ok], j[ok]]
        out[b, :, :, :n] = o + np.einsum("hir,rd->hdi", pw, ev)
    return out.reshape(B, C, T)


def _chain(steps, term):
    """sequential fmaf chain: acc = fp32(acc + a_s * b_s), the product exact in float64; term(s) -> the two float64 operands of step s, broadcastable"""
    acc = None
    for s in range(steps):
        x, y = term(s)
        prod = x * y
        acc = prod.astype(np.float32) if acc is None else (acc.astype(np.float64) + prod).astype(np.float32)
    return acc


def chain32(q, k, v, rel_k, rel_v, heads, window, lens, q_scale=1.0, exp_tab=None):
    """the fp32 restatement, [B, C, T] fp32, zero behind lens[b]; every utterance and head at once (padded entries are masked out of every sum)"""
    B, C, T = q.shape
    hd = C // heads
    qs = _heads((q * np.float32(q_scale)).astype(np.float32), heads).astype(np.float64)  # [B, h, d, T]
    kk, vv = _heads(k, heads).astype(np.float64), _heads(v, heads).astype(np.float64)
    ek, ev = rel_k.astype(np.float64), rel_v.astype(np.float64)
    nrel = 2 * window + 1
    valid = _valid(lens, T)  # [B, T]
    r, win = _rel_index(T, window)
    rc = np.clip(r, 0, 2 * window)
    # scores [B, h, i, j] and relative logits [B, h, i, r]: chains over d
    s = _chain(hd, lambda d: (qs[:, :, d, :, None], kk[:, :, d, None, :]))
    qe = _chain(hd, lambda d: (qs[:, :, d, :, None], ek[None, None, None, :, d]))
    s = np.where(win[None, None], s + np.take_along_axis(qe, np.broadcast_to(rc[None, None], s.shape), axis=3), s).astype(np.float32)
    keymask = valid[:, None, None, :]
    s = np.where(keymask, s, -np.inf).astype(np.float32)
    with np.errstate(invalid="ignore"):
        x = (s - s.max(axis=3, keepdims=True)).astype(np.float32)
    x = np.where(keymask, x, -np.inf)
    if exp_tab is not None:
        e = np.where(keymask, table_lookup(exp_tab, np.where(keymask, x, 0.0)), 0.0).astype(np.float32)
        tot = e.astype(np.float64).sum(axis=3, keepdims=True)  # (the kernel sums fp16 values in double: exact)
        inv = (1.0 / np.where(tot > 0, tot, 1.0)).astype(np.float32)
    else:
        e = np.exp(x.astype(np.float64)).astype(np.float32)
        tot = np.zeros(e.shape[:3], np.float32)
        for j in range(T):
            tot = tot + e[..., j]
        inv = (np.float32(1) / np.where(tot > 0, tot, np.float32(1)))[..., None].astype(np.float32)
    p = (e * inv).astype(np.float32)  # [B, h, i, j], zero on padded keys
    p64 = p.astype(np.float64)
    o = _chain(T, lambda j: (p64[:, :, None, :, j], vv[:, :, :, None, j]))  # [B, h, d, i]
    pw = np.zeros((B, heads, T, nrel))
    i = np.arange(T)
    for rel in range(nrel):
        j = i + rel - window
        ok = (j >= 0) & (j < T)
        pw[:, :, i[ok], rel] = p64[:, :, i[ok], j[ok]]
    rs = _chain(nrel, lambda rel: (pw[:, :, None, :, rel], ev[None, None, rel, :, None]))
    out = (o + rs).astype(np.float32)
    out = np.where(valid[:, None, None, :], out, np.float32(0))
    return out.reshape(B, C, T)


def edge_queries(lens, window):
    """mask over the gathered columns (tests/split_ref.py gather_cols): queries within `window` of either end of their utterance, and the last query tile"""
    parts = []
    for n in lens:
        n = int(n)
        t = np.arange(n)
        parts.append((t < window) | (t >= n - window) | (t >= (n - 1) // 16 * 16) if n else np.zeros(0, bool))
    return np.concatenate(parts) if parts else np.zeros(0, bool)


def partial_group_queries(lens):
    """mask over the gathered columns: every query of an utterance whose last group of 16 keys is partial (its P V product runs over padded keys)"""
    return np.concatenate([np.full(int(n), int(n) % 16 != 0) for n in lens]) if len(lens) else np.zeros(0, bool)
