"""numpy side of the operator tests of the fp32-accurate kernels (VITS_ARITH_F32_SPLIT: tests/test_gpu_split_ops.py, tests/test_split_emulation.py; the fused
fp32 ResBlock kernels: tests/test_gpu_resblock_ops.py, tests/test_resblock_op_host.py): the float64 reference of a
conv / a ResBlock pair, the sequential fp32 fmaf chain the bound is derived from, and a restatement of the split arithmetic itself
(vits.cpp_amd/csrc/conv_split.hip: weights = two bf16 pieces, activations = three, five of the six cross products, fp32 accumulation).

Everything works on COLUMNS: the valid outputs (b, t < lens[b]) of a batch side by side, [channels, sum(lens)], and on the im2col matrix A [c_in * k, columns] of
the activated, zero-padded input, row index ci * k + j — the order of w.reshape(c_out, c_in * k). An input past lens[b] is zero padding, as in the kernels.

The bound (the "2x rule"): rms error of the result under test <= 2 x rms error of the sequential fp32 chain on the same data, both against the float64 result and
relative to its RMS. The matrix core adds its sixteen products in its own order; blocked orders are no worse than a sequential chain; the split's own sequential
order sits at 1.6-1.7 x the chain, a lost cross product at 3.7-8.6 x (tests/test_split_emulation.py pins both)."""
import numpy as np

FACTOR = 2.0
MIN_ELEMS = 8192  # outputs the chain is computed on, at least (or every output there is, when a case has fewer)


def case_seed(cin, cout, k, dil, T):
    return ((cin * 1009 + cout) * 131 + k * 7 + dil) * 4099 + T


def make_case(cin, cout, k, dil, T, B, bf16_weights=False):
    """x ~ N(0, 1), weights ~ N(0, 1 / (c_in k)) rounded through float16 (or, bf16_weights, to bf16: an all-zero second plane), bias, residual, accum."""
    rng = np.random.default_rng(case_seed(cin, cout, k, dil, T))
    x = rng.standard_normal((B, cin, T)).astype(np.float32)
    w = (rng.standard_normal((cout, cin, k)) / np.sqrt(cin * k)).astype(np.float16).astype(np.float32)
    if bf16_weights:
        w = bf16_rne(w)
    bias = rng.standard_normal(cout).astype(np.float32)
    res = rng.standard_normal((B, cout, T)).astype(np.float32)
    acc = rng.standard_normal((B, cout, T)).astype(np.float32)
    return x, w, bias, res, acc


def lrelu32(v, slope):
    """leaky ReLU as the kernels compute it: max(v, v * slope) in fp32 — one deterministic rounding, the same on both sides"""
    v = np.asarray(v, np.float32)
    return np.maximum(v, v * np.float32(slope))


def bf16_rne(x):
    """fp32 -> the nearest bf16 value (ties to even), as fp32, by bit operations"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return r.view(np.float32)


def split_pieces(x, n):
    """x as n bf16 pieces, piece p = RNE of what the pieces before it left (exact fp32 subtractions); returns (pieces, remainder)"""
    r = np.array(x, np.float32)
    out = []
    for _ in range(n):
        p = bf16_rne(r)
        out.append(p)
        r = (r - p).astype(np.float32)
    return out, r


def gather_cols(y, lens):
    """[B, C, T] -> [C, sum(lens)]: the valid columns of every utterance"""
    return np.concatenate([y[b, :, : lens[b]] for b in range(len(lens))], axis=1)


def scatter_cols(cols, lens, T):
    """inverse of gather_cols, zero past lens[b]"""
    out = np.zeros((len(lens), cols.shape[0], T), cols.dtype)
    o = 0
    for b, n in enumerate(lens):
        out[b, :, :n] = cols[:, o:o + n]
        o += n
    return out


def im2col(a, lens, k, dil, pad_left=None):
    """a [B, c_in, T] fp32 (already activated) -> A [c_in * k, sum(lens)] fp32; taps that fall outside [0, lens[b]) are zero"""
    B, cin, _ = a.shape
    pad = (k - 1) * dil // 2 if pad_left is None else pad_left
    blocks = []
    for b in range(B):
        n = int(lens[b])
        A = np.zeros((cin, k, n), np.float32)
        for j in range(k):
            s = j * dil - pad  # source time of output t is t + s
            lo, hi = max(0, -s), min(n, n - s)
            if hi > lo:
                A[:, j, lo:hi] = a[b, :, lo + s:hi + s]
        blocks.append(A.reshape(cin * k, n))
    return np.concatenate(blocks, axis=1)


def conv64(w, A):
    """the float64 product sums, [c_out, columns]"""
    return w.reshape(w.shape[0], -1).astype(np.float64) @ A.astype(np.float64)


def chain_rows(cout, ncols):
    """the fixed subset of output channels the chain is computed on: evenly spread, as few as give MIN_ELEMS outputs (all of them if that is not enough)"""
    m = min(cout, max(1, -(-MIN_ELEMS // max(1, ncols))))
    return (np.arange(m) * cout) // m


def chain32(W, A):
    """sequential fp32 fmaf chain: acc = fp32(acc + w a), one exact float64 product per step, in row order of A. W [m, n], A [n, L] -> fp32 [m, L]"""
    W64, A64 = W.astype(np.float64), A.astype(np.float64)
    acc = np.zeros((W.shape[0], A.shape[1]), np.float32)
    for i in range(A.shape[0]):
        acc = (acc.astype(np.float64) + np.multiply.outer(W64[:, i], A64[i])).astype(np.float32)
    return acc


SPLIT_TERMS = ((2, 0), (1, 1), (0, 1), (1, 0), (0, 0))  # (activation piece, weight piece) in the kernel's order: a3 w1, a2 w2, a1 w2, a2 w1, a1 w1


def emulate_split(W, A, drops=(None,)):
    """The split arithmetic with SEQUENTIAL fp32 accumulation (the worst order): per product the five kept cross terms, each exact, added one at a time.
    One result per entry of `drops`: None = all five terms, (p, q) = without the product of activation piece p and weight piece q."""
    wp, rw = split_pieces(W, 2)
    ap, ra = split_pieces(A, 3)
    assert not rw.any(), "a weight is not the exact sum of two bf16 values"
    assert not ra.any(), "an activation is not the exact sum of three bf16 values"
    wp = [p.astype(np.float64) for p in wp]
    ap = [p.astype(np.float64) for p in ap]
    accs = [np.zeros((W.shape[0], A.shape[1]), np.float32) for _ in drops]
    for i in range(A.shape[0]):
        for term in SPLIT_TERMS:
            prod = np.multiply.outer(wp[term[1]][:, i], ap[term[0]][i])
            for v, drop in enumerate(drops):
                if drop != term:
                    accs[v] = (accs[v].astype(np.float64) + prod).astype(np.float32)
    return accs


def epilogue32(acc, bias=None, res=None, accum=None, scale=1.0):
    """the kernels' epilogue in their order, every step one fp32 rounding: + bias, residual +, (accum + v) * scale. All operands [rows, columns] / [rows]."""
    v = np.asarray(acc, np.float32)
    if bias is not None:
        v = v + np.asarray(bias, np.float32)[:, None]
    if res is not None:
        v = np.asarray(res, np.float32) + v
    if accum is not None:
        v = (np.asarray(accum, np.float32) + v) * np.float32(scale)
    return v.astype(np.float32)


def epilogue64(acc, bias=None, res=None, accum=None, scale=1.0):
    v = np.asarray(acc, np.float64)
    if bias is not None:
        v = v + np.asarray(bias, np.float64)[:, None]
    if res is not None:
        v = v + np.asarray(res, np.float64)
    if accum is not None:
        v = (v + np.asarray(accum, np.float64)) * np.float64(np.float32(scale))
    return v


def rms_err(got, ref):
    """(rms, max) of got - ref relative to the RMS of ref (float64)"""
    ref = np.asarray(ref, np.float64)
    e = np.asarray(got, np.float64) - ref
    rms = np.sqrt((ref ** 2).mean()) + 1e-300
    return float(np.sqrt((e ** 2).mean()) / rms), float(np.abs(e).max() / rms)


# ---- a ResBlock conv pair against float64, and the rule applied to a result (shared by the split-operand and the fused fp32 pair tests) --------------------
def make_pair(C, k, dil, T, B):
    rng = np.random.default_rng(case_seed(C, C, k, dil, T) + 1)
    x = rng.standard_normal((B, C, T)).astype(np.float32)
    w1, w2 = ((rng.standard_normal((C, C, k)) / np.sqrt(C * k)).astype(np.float16).astype(np.float32) for _ in range(2))
    b1, b2 = (rng.standard_normal(C).astype(np.float32) for _ in range(2))
    return x, w1, b1, w2, b2


def pair_reference(x, w1, b1, w2, b2, lens, dil, slope):
    """y = x + b2 + conv2(lrelu(b1 + conv1(lrelu(x)))) on the valid columns: (ref float64 [C, columns], chain fp32 [len(rows), columns], rows)"""
    C, _, k = w1.shape
    T = x.shape[2]
    xc = gather_cols(x, lens)
    A1 = im2col(lrelu32(x, slope), lens, k, dil)
    # reference: float64 sums; the intermediate is rounded to fp32 before its leaky ReLU (it exists only as an fp32 value)
    t32 = epilogue64(conv64(w1, A1), b1).astype(np.float32)
    A2 = im2col(scatter_cols(lrelu32(t32, slope), lens, T), lens, k, 1)
    ref = epilogue64(conv64(w2, A2), b2, xc)
    # the chain through both convs: conv 1 on every channel (conv 2 reads them all), conv 2 on the subset
    tc = epilogue32(chain32(w1.reshape(C, -1), A1), b1)
    A2c = im2col(scatter_cols(lrelu32(tc, slope), lens, T), lens, k, 1)
    rows = chain_rows(C, A1.shape[1])
    chain = epilogue32(chain32(w2.reshape(C, -1)[rows], A2c), b2[rows], xc[rows])
    return ref, chain, rows


def hold_to_the_chain(label, got, lens, ref, chain, rows):
    """got [B, C, T] from the GPU; ref [C, columns] float64; chain fp32 [len(rows), columns]. Prints, then asserts the 2x rule (overall and per 32-row tile)."""
    for b, n in enumerate(lens):
        assert not got[b, :, n:].any(), (label, b, "a column past lens[b] was written")
    cols = gather_cols(got, lens)
    assert np.isfinite(cols).all(), (label, "a slot past an utterance's length (NaN) was read")
    c_rms, c_max = rms_err(chain, ref[rows])
    g_rms, g_max = rms_err(cols, ref)
    print("%s: %d outputs (chain on %d): gpu rms %.2e max %.2e of RMS; chain rms %.2e max %.2e; ratio %.2f"
          % (label, cols.size, chain.size, g_rms, g_max, c_rms, c_max, g_rms / c_rms))
    assert g_rms <= FACTOR * c_rms, (label, g_rms, c_rms)
    if 32 * cols.shape[1] >= MIN_ELEMS:
        for mt in range(cols.shape[0] // 32):
            t_rms, _ = rms_err(cols[32 * mt:32 * mt + 32], ref[32 * mt:32 * mt + 32])
            assert t_rms <= FACTOR * c_rms, (label, "row tile", mt, t_rms, c_rms)
    return g_rms / c_rms


def edge_columns(lens, k, bo):
    """mask over the gathered columns: the last k - 1 columns of every row and the k - 1 columns on each side of every tile boundary m bo inside the row — where
    a fused kernel masks its intermediate and where one block's outputs depend on its halo"""
    parts = []
    for n in lens:
        t = np.arange(int(n))
        m = t >= n - (k - 1)
        for edge in range(bo, int(n), bo):
            m |= (t >= edge - (k - 1)) & (t < edge + (k - 1))
        parts.append(m)
    return np.concatenate(parts) if parts else np.zeros(0, bool)


class EdgePool:
    """Squared errors on the edge windows of a case's calls, pooled: the 2x rule on them alone, so that a fault at an edge is not diluted by the columns around it."""

    def __init__(self):
        self.g = self.c = self.rg = self.rc = 0.0
        self.n = 0

    def add(self, cols, ref, chain, rows, mask):
        if not mask.any():
            return
        r = np.asarray(ref, np.float64)[:, mask]
        self.g += float(((np.asarray(cols, np.float64)[:, mask] - r) ** 2).sum())
        self.rg += float((r ** 2).sum())
        self.c += float(((np.asarray(chain, np.float64)[:, mask] - r[rows]) ** 2).sum())
        self.rc += float((r[rows] ** 2).sum())
        self.n += int(mask.sum()) * r.shape[0]

    def ratio(self):
        """rms error of the result over rms error of the chain, each relative to the reference's RMS on its own outputs"""
        return np.sqrt(self.g / self.rg) / (np.sqrt(self.c / self.rc) + 1e-300)
