"""numpy side of the operator tests of the flow's coupling layer (vits_op_flow_coupling: tests/test_gpu_flow_ops.py, tests/test_flow_op_host.py): the data, the
float64 reference of one coupling layer and the sequential fp32 chain through all ten convs, both built from tests/split_ref.py (im2col, conv64, chain32, the
epilogues) and both returned on the valid columns (split_ref.gather_cols order).

    h = W_pre x0 + b_pre;  out = 0
    l < layers:  g = Conv_k(h) + b_in[row_b][l];  a = tanh(g[0:H]) * sigmoid(g[H:2H]);  rs = W_rs[l] a + b_rs[l]
                 l + 1 < layers: h += rs[0:H], out += rs[H:2H];  the last layer: out += rs
    m = W_post out + b_post;  x1' = x1 + m

Reference: float64 product sums; every intermediate (h, g, a, out) exists only as an fp32 value and is rounded to fp32; the tanh and the sigmoid are fp32
functions of the fp32 g on both sides. Chain: the same with every product sum a sequential fp32 fmaf chain (split_ref.chain32) and every epilogue step one fp32
rounding (split_ref.epilogue32).

The rule is split_ref's: rms error of the result under test <= FACTOR (2.0) x the chain's, both against float64 — applied to the UPDATE m = x1' - x1, not to
x1': the passed-through x1 roughly halves the relative error and would hide a fault. Measured on the CPU for the whole layer (lens 70, 69, 33, 5; six draws
including weights x 3, inputs x 3 and x 4): a chain in the kernels' own order (32-channel chunk, tap, channel) sits at 0.99-1.01 of the row-order chain, a
BLAS-order fp32 product at 0.87-0.93; the chain's own error ran from 3e-7 to 2.9e-6 of RMS."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import split_ref as R

H, HALF, K, LAYERS = 192, 96, 5, 4  # the one shape with fused instantiations
B = 4
BIAS_ROWS = [2, 0, 1, 2]  # per-utterance rows of the three-row b_in table
FACTOR = R.FACTOR


def _w(rng, cout, cin, k):
    """fp16-valued, as stored models' (export_vits.py), scaled by 1 / sqrt(fan_in)"""
    return (rng.standard_normal((cout, cin, k)) / np.sqrt(cin * k)).astype(np.float16).astype(np.float32)


def make_weights(seed=0x0F10):
    rng = np.random.default_rng(seed)
    b = lambda *shape: (0.1 * rng.standard_normal(shape)).astype(np.float32)
    W = dict(w_pre=_w(rng, H, HALF, 1), b_pre=b(H), w_in=np.stack([_w(rng, 2 * H, H, K) for _ in range(LAYERS)]), b_in=b(3, LAYERS, 2 * H))
    W["w_rs"] = [_w(rng, 2 * H if l + 1 < LAYERS else H, H, 1) for l in range(LAYERS)]
    W["b_rs"] = [b(2 * H if l + 1 < LAYERS else H) for l in range(LAYERS)]
    W["w_post"], W["b_post"] = _w(rng, HALF, H, 1), b(HALF)
    return W


def make_inputs(T, hot, seed=0):
    """(x0, x1), each [B, HALF, T]: unit variance; hot: x0 x 4, so that gate inputs saturate"""
    rng = np.random.default_rng(R.case_seed(H, HALF, K, 1 + int(hot), T) + seed)
    x0 = rng.standard_normal((B, HALF, T)).astype(np.float32)
    x1 = rng.standard_normal((B, HALF, T)).astype(np.float32)
    return (x0 * np.float32(4) if hot else x0), x1


def place(x0, x1, flipped):
    """z [B, 2 HALF, T]: flipped 0 = x0 first, 1 = x1 first (the engine's two placements)"""
    return np.concatenate([x1, x0] if flipped else [x0, x1], axis=1)


def halves(z, flipped):
    return (z[:, HALF:], z[:, :HALF]) if flipped else (z[:, :HALF], z[:, HALF:])


def gate32(g):
    """tanh(g[0:H]) * sigmoid(g[H:2H]) in fp32, the sigmoid as the kernels write it: 1 / (1 + exp(-s))"""
    g = np.asarray(g, np.float32)
    one = np.float32(1)
    return (np.tanh(g[:H]) * (one / (one + np.exp(-g[H:])))).astype(np.float32)


def chain32(W, A, threads=8):
    """split_ref.chain32 on slices of the columns in parallel (columns never interact: the same values)"""
    n = A.shape[1]
    if n < 64:
        return R.chain32(W, A)
    cuts = np.linspace(0, n, threads + 1).astype(int)
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(lambda i: R.chain32(W, A[:, cuts[i]:cuts[i + 1]]), range(threads)))
    return np.concatenate(parts, axis=1)


def bias_columns(b_in, l, lens, bias_rows):
    """[2H, columns]: the gated conv's bias of every valid column (its utterance's table row)"""
    rows = [0] * len(lens) if bias_rows is None else bias_rows
    return np.concatenate([np.repeat(b_in[rows[b], l][:, None], int(n), axis=1) for b, n in enumerate(lens)], axis=1)


def layer_reference(x0, x1, W, lens, bias_rows=None, chain=True):
    """(m64 [HALF, columns] float64, m32 fp32 or None, x1c [HALF, columns]): the update W_post out + b_post in float64, and the fp32 chain's x1' - x1"""
    T = x0.shape[2]
    x1c = R.gather_cols(x1, lens)
    A0 = R.im2col(x0, lens, 1, 1)

    def run(prod, epi, final):
        h = epi(prod(W["w_pre"], A0), W["b_pre"]).astype(np.float32)
        out = np.zeros_like(h)
        for l in range(LAYERS):
            A = R.im2col(R.scatter_cols(h, lens, T), lens, K, 1)
            g = (epi(prod(W["w_in"][l], A)) + bias_columns(W["b_in"], l, lens, bias_rows)).astype(np.float32)
            a = gate32(g)
            rs = prod(W["w_rs"][l], a)
            if l + 1 < LAYERS:
                h = epi(rs[:H], W["b_rs"][l][:H], h).astype(np.float32)
                out = epi(rs[H:], W["b_rs"][l][H:], out).astype(np.float32)
            else:
                out = epi(rs, W["b_rs"][l], out).astype(np.float32)
        return final(prod(W["w_post"], out))

    m64 = run(R.conv64, R.epilogue64, lambda acc: R.epilogue64(acc, W["b_post"]))
    m32 = None
    if chain:
        x1n = run(lambda w, A: chain32(w.reshape(w.shape[0], -1), A), R.epilogue32, lambda acc: R.epilogue32(acc, W["b_post"], x1c))
        m32 = x1n.astype(np.float64) - x1c.astype(np.float64)
    return m64, m32, x1c


def update_of(got_x1, x1c, lens):
    """the update a result carries: x1' - x1 on the valid columns, float64 [HALF, columns]"""
    return R.gather_cols(got_x1, lens).astype(np.float64) - x1c.astype(np.float64)


def ratios(m_got, m64, m32, mask=None):
    """(rms error of m_got, of the chain) against float64, relative to its RMS — overall or on the masked columns"""
    if mask is not None:
        m_got, m64, m32 = m_got[:, mask], m64[:, mask], m32[:, mask]
    return R.rms_err(m_got, m64)[0], R.rms_err(m32, m64)[0]
