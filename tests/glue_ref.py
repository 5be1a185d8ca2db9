"""numpy side of the operator tests of the kernels between the conv families (tests/test_gpu_glue_ops.py, tests/test_glue_op_host.py): prior and posterior sampling
(zp_kernel, posterior_sample_kernel), conv_post (conv_post_kernel, conv_post16_kernel) and the sum over a stage's resblocks (rb_sum3_std_kernel).

Every operation has a float64 reference and an fp32 restatement of the kernel's own expression, each step rounded to fp32; the restatement's error against float64 is
what the 2x rule of tests/split_ref.py (FACTOR, MIN_ELEMS) doubles. The sum has no error to bound: numpy's float32 arithmetic is the kernel's, bit for bit.
  * counter_normal: include/vits_synth_noise.h's vits_counter_normal in integer arithmetic and one rounded multiply, bit-identical to the header on the host.
  * sampling: a(j) = the first token with cum > j (-1: none, mean 0 and logvar 0); z = mean[a] + (eps * exp(logvar[a])) * scale; the posterior draw is
    mean + (eps * eps_scale) * exp(logstd). fp32: numpy's float32 exp.
  * conv_post: leaky_relu in fp32 on both sides (one deterministic rounding, tests/split_ref.py lrelu32), in a 16-bit arithmetic rounded to that type afterwards as
    the kernels round it, the weights rounded likewise; float64 sums over those operands, and the sequential fp32 fmaf chain over them, channel-major and tap-minor.
    tanh: the device library's tanhf is held to the 5 ulp of the OpenCL full profile (TANH_ULP), which its tanh documents."""
import numpy as np

import split_ref as R

FACTOR, MIN_ELEMS = R.FACTOR, R.MIN_ELEMS
STREAM_NOISE_PRIOR = 2
SENTINEL = 0x7FFFFFFF
TANH_ULP = 5

# ---- case tables (checked on the CPU by tests/test_glue_op_host.py) ----------------------------------------------------------------------------------------------
SAMPLE_FRAMES = (1, 255, 256, 257, 513)   # zp_kernel and posterior_sample_kernel: one block per 256 frames
SAMPLE_CHANNELS = (1, 15, 16, 17, 192)    # split over gridDim.z = 16
POST_CIN = (1, 7, 8, 9, 32, 40)           # conv_post_kernel's fast path takes eight channels per step
POST_K = (3, 5, 7)                        # the fast path is k = 7
POST_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 11, 12, 13, 1023, 1024, 1025, 2051)  # one block = 1024 samples, one fast-path thread = 4
POST_RAGGED = (2051, 1025, 1023, 7)
POST_EMIT_LO = (0, 4, 6, 1020, 1024)
POST16_CIN = (8, 32, 40)
POST16_CIN_FP32_LAYOUT = (7, 9)
SUM_CASES = [(C, T) for C in (1, 5, 32) for T in (1, 255, 256, 257, 600)]  # rb_sum3_std_kernel: one block per 256 columns of one channel


def emit_his(n, lo):
    """the emit_hi values of a row of n samples: the row's end, one and five before it, and emit_lo itself (an empty window)"""
    return sorted({n, max(0, n - 1), max(0, n - 5), lo})


def odd_pitch(T):
    """a device pitch >= T that is no multiple of 4"""
    p = T + 1
    return p if p % 4 else p + 1


def aligned_pitch(T):
    return (T + 3) // 4 * 4


# ---- the counter stream ------------------------------------------------------------------------------------------------------------------------------------------
def _mix64(z):
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _hash3(seed, stream, index):
    with np.errstate(over="ignore"):
        h = _mix64(np.uint64(seed) ^ np.uint64(0xD1B54A32D192ED03))
        h = _mix64(h ^ (np.uint64(stream) * np.uint64(0x9E3779B97F4A7C15)))
        return _mix64(h ^ index.astype(np.uint64))


def counter_normal(seed, stream, index):
    """vits_counter_normal(seed, stream, index) for an array of indices"""
    index = np.asarray(index, np.uint64)
    a, b = _hash3(seed, stream, np.uint64(2) * index), _hash3(seed, stream, np.uint64(2) * index + np.uint64(1))
    s = np.zeros(index.shape, np.int64)
    for h in (a, b):
        for sh in (0, 16, 32, 48):
            s += ((h >> np.uint64(sh)) & np.uint64(0xFFFF)).astype(np.int64)
    centred = s.astype(np.float32) - np.float32(262140.0)
    return (centred * np.float32(1.8688258e-05)).astype(np.float32)


def counter_noise(seed, seed_offsets, channels, frames, t_stride):
    """[B, channels, t_stride]: row b's draw, index c * frames[b] + j, on [0, frames[b]); NaN behind it"""
    out = np.full((len(frames), channels, t_stride), np.nan, np.float32)
    for b, L in enumerate(frames):
        off = b if seed_offsets is None else int(seed_offsets[b])
        out[b, :, :L] = counter_normal(seed + off, STREAM_NOISE_PRIOR, np.arange(channels * L)).reshape(channels, L)
    return out


# ---- sampling ----------------------------------------------------------------------------------------------------------------------------------------------------
def durations_case(name, T, frames):
    """int durations [T] summing to `frames` (all zero: `none`), with runs of zero-duration tokens where the name says"""
    rng = np.random.default_rng(T * 7919 + frames)
    d = np.zeros(T, np.int64)
    if name == "none":
        return d
    live = np.ones(T, bool)
    run = max(1, T // 4)
    if name in ("zeros_start", "zeros_everywhere") and T > 1:
        live[:run] = False
    if name in ("zeros_middle", "zeros_everywhere") and T > 3:
        live[T // 2 - run // 2:T // 2 - run // 2 + run] = False
    if name in ("zeros_end", "zeros_everywhere") and T > 2:
        live[T - run:] = False
    idx = np.flatnonzero(live)
    assert idx.size, (name, T)
    cuts = np.sort(rng.integers(0, frames + 1, idx.size - 1))
    d[idx] = np.diff(np.concatenate([[0], cuts, [frames]]))
    assert d.sum() == frames
    return d


DURATION_KINDS = ("plain", "zeros_start", "zeros_middle", "zeros_end", "zeros_everywhere", "none")


def cum_rows(durs, t_tok):
    """cum int32 [B, t_tok] as the durations kernel leaves it: inclusive sums, SENTINEL behind every row's tokens; tok_lens; frames = max(1, sum)"""
    B = len(durs)
    cum = np.full((B, t_tok), SENTINEL, np.int32)
    for b, d in enumerate(durs):
        cum[b, :len(d)] = np.cumsum(d)
    return cum, np.array([len(d) for d in durs], np.int32), np.array([max(1, int(np.sum(d))) for d in durs], np.int32)


def token_of_frame(cum_row, T, L):
    """a(j) for j < L: the first token i < T with cum[i] > j, -1 where there is none"""
    a = np.searchsorted(np.asarray(cum_row[:T], np.int64), np.arange(L), side="right")
    return np.where(a < T, a, -1)


def gathered(mean, cum, tok_lens, frames, t_stride):
    """mean [B, C, t_tok] -> [B, C, t_stride]: mean[b, :, a(j)] on [0, frames[b]) (0 where a(j) = -1), NaN behind"""
    B, C, _ = mean.shape
    out = np.full((B, C, t_stride), np.nan, mean.dtype)
    for b in range(B):
        a = token_of_frame(cum[b], tok_lens[b], frames[b])
        out[b, :, :frames[b]] = np.where(a[None, :] >= 0, mean[b][:, np.maximum(a, 0)], 0)
    return out


def sample64(mu, lv, eps, scale):
    """mu + eps * exp(lv) * scale in float64; scale a scalar or [B]"""
    s = np.asarray(scale, np.float64).reshape(-1, 1, 1) if np.ndim(scale) else np.float64(np.float32(scale))
    return mu.astype(np.float64) + eps.astype(np.float64) * np.exp(lv.astype(np.float64)) * s


def prior32(mu, lv, eps, scale):
    """zp_kernel's expression: n = eps * expf(lv); n = n * scale; mu + n, each rounded to fp32"""
    s = np.asarray(scale, np.float32).reshape(-1, 1, 1) if np.ndim(scale) else np.float32(scale)
    with np.errstate(invalid="ignore"):
        n = (eps.astype(np.float32) * np.exp(lv.astype(np.float32))).astype(np.float32)
        return (mu.astype(np.float32) + (n * s).astype(np.float32)).astype(np.float32)


def posterior32(mu, ls, eps, eps_scale):
    """posterior_sample_kernel's expression: mu + (eps * eps_scale) * expf(ls), each rounded to fp32"""
    with np.errstate(invalid="ignore"):
        e = (eps.astype(np.float32) * np.float32(eps_scale)).astype(np.float32)
        return (mu.astype(np.float32) + (e * np.exp(ls.astype(np.float32))).astype(np.float32)).astype(np.float32)


def valid(x, frames):
    """[B, C, t] -> the valid elements of every row, one flat array"""
    return np.concatenate([x[b, :, :L].ravel() for b, L in enumerate(frames)])


# ---- conv_post ---------------------------------------------------------------------------------------------------------------------------------------------------
def round16(v, arith_name):
    """fp32 -> the nearest value of the arithmetic's type (ties to even), as fp32; "f32": unchanged"""
    v = np.asarray(v, np.float32)
    if arith_name == "f16":
        return v.astype(np.float16).astype(np.float32)
    if arith_name == "bf16":
        return R.bf16_rne(v)
    assert arith_name == "f32"
    return v


def post_case(cin, k, T, B):
    rng = np.random.default_rng(((cin * 131 + k) * 4099 + T) * 8 + B)
    x = rng.standard_normal((B, cin, T)).astype(np.float32)
    w = (rng.standard_normal((cin, k)) / np.sqrt(cin * k)).astype(np.float32)
    return x, w


def post_reference(x, w, slope, lens, arith_name="f32"):
    """(float64 sums [columns], the fp32 chain [columns]) of the valid columns side by side, over the operands as the kernel holds them"""
    cin, k = w.shape
    a = round16(np.where(x > 0, x, (x * np.float32(slope)).astype(np.float32)), arith_name)
    A = R.im2col(a, lens, k, 1)  # row ci * k + j: channel-major, tap-minor
    W = round16(w, arith_name).reshape(1, cin * k)
    return R.conv64(W, A)[0], R.chain32(W, A)[0]


def tanh_within(wave, pre):
    """|wave - tanh(pre)| in units of the fp32 spacing at tanh(pre): the largest over the array"""
    t = np.tanh(pre.astype(np.float64))
    ulp = np.spacing(np.maximum(np.abs(t), np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)
    return float((np.abs(wave.astype(np.float64) - t) / ulp).max()) if t.size else 0.0


# ---- the sum -----------------------------------------------------------------------------------------------------------------------------------------------------
def sum32(y0, y1, y2, scale, scale_div, act, slope):
    """rb_sum3_std_kernel in numpy float32: (y0 + y1) [+ y2], * scale or / scale, [max(x, x * slope)]"""
    x = y0.astype(np.float32) + y1.astype(np.float32)
    if y2 is not None:
        x = x + y2.astype(np.float32)
    x = x / np.float32(scale) if scale_div else x * np.float32(scale)
    if act:
        x = np.maximum(x, x * np.float32(slope))
    assert x.dtype == np.float32
    return x
