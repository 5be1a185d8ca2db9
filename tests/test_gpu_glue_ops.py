"""The kernels between the conv families at operator level: zp_kernel (vits_op_prior_sample), posterior_sample_kernel (vits_op_posterior_sample), conv_post_kernel
and conv_post16_kernel (vits_op_conv_post) and rb_sum3_std_kernel (vits_op_resblock_sum), on inputs no whole model produces: a model samples 192 channels (or the
tiny files' 16), has conv_post at 32 channels with k = 7 behind tensors whose pitch is a multiple of 4, and windows it only at multiples of 256.

Outputs are staged as 0xFF bytes, inputs with NaN behind every length (tests/glue_ref.py holds the references and the case tables, tests/test_glue_op_host.py
checks them on the CPU). The 2x rule is tests/split_ref.py's: rms error against float64 <= 2 x the fp32 restatement's, asserted where a case has MIN_ELEMS
outputs (pooled over its lengths), printed below that.

vits_op_prior_sample, channels in {1, 15, 16, 17, 192} (fewer than the sixteen channel blocks, one short, one each, one over, twelve each) x frames in {1, 255, 256,
257, 513}, ragged batches of 4 whose rows have plain durations, runs of zero-duration tokens (start, middle, end, all three in turn), no duration at all (one frame,
a(j) = -1) and a single token; cum carries INT32_MAX behind every row's tokens:
  * noise scale 0 == mean[a(j)] bit for bit (the gather alone); mean 0, logvar 0, scale 1 with the counter stream == vits_counter_normal bit for bit, with the
    row's own seed offset; the counter call == the explicit-noise call fed those values; per-row scales == the scalar call row by row; nothing behind frames[b]
    is written; the 2x rule.
vits_op_posterior_sample, the same channels and frames x flip: eps_scale 0 == the mean bit for bit with a NaN noise tensor; counter == explicit; the 2x rule.
vits_op_conv_post, cin in {1, 7, 8, 9, 32, 40} x k in {3, 5, 7} x lengths {1, 2, 3, 4, 5, 7, 8, 11, 12, 13, 1023, 1024, 1025, 2051} and the ragged batch
(2051, 1025, 1023, 7):
  * the float4 path (k = 7, x pitch a multiple of 4) == the scalar path (an odd x pitch; emit_lo = 6) bit for bit; an odd pre pitch and pre = NULL change nothing;
  * a window [emit_lo, emit_hi) for emit_lo in {0, 4, 6, 1020, 1024} and emit_hi in {len, len - 1, len - 5, emit_lo} == the same samples of the whole call, and
    nothing outside it is written; wave is tanh(pre) within the device library's 5 ulp; the 2x rule on pre;
  * 16-bit arithmetic, f16 and bf16: the streaming form at cin in {8, 32, 40}, refused for cin in {7, 9} with the cause named, which run on the fp32-layout form.
vits_op_resblock_sum == numpy float32 bit for bit: two and three addends, scale and divide, leaky_relu on and off, ragged lengths, distinct pitches.
Observed on an MI355X (the tests print every figure), GPU / restatement pooled per case, with the restatement's own rms error of RMS: prior sampling 0.63 to 0.75
(4.7e-8 to 5.7e-8; 1 channel has 7678 outputs: printed only), the posterior draw 0.66 to 0.67 (4.7e-8): the device contracts the last product and sum into one
rounding; conv_post fp32 1.00 in all eighteen cases (3.7e-8 to 2.8e-7: the kernel's sum IS the sequential fmaf chain), the fp32-layout form in f16 and bf16 1.00
(5.7e-8 to 2.8e-7), the streaming form 0.71 to 0.84 in f16 and 0.83 to 0.98 in bf16 (7.3e-8 to 2.8e-7; exact 16-bit products, added in pairs), 9295 outputs each.
Every bit identity held on the first run. The float4 store to pre, which checked the alignment of x alone, takes element stores at a pre pitch that is no
multiple of 4 since this file exists; the cases with an odd pre pitch run that branch."""
import numpy as np
import pytest

import glue_ref as G
import split_ref as R

pytestmark = pytest.mark.gpu
NAN_BITS = 0xFFFFFFFF
T_TOK = 12
SLOPE = 0.01  # HiFi-GAN's conv_post takes the default leaky_relu


@pytest.fixture
def nan_outputs(pkg):
    pkg.op_set_output_fill(0xFF)
    yield
    pkg.op_set_output_fill(0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_valid(label, got, want, frames):
    """[B, C, t]: the valid columns hold want's bits, everything behind frames[b] the staged 0xFF bytes"""
    for b, L in enumerate(frames):
        assert np.array_equal(bits(got[b, :, :L]), bits(want[b, :, :L])), (label, "row", b, "frames", L, int((bits(got[b, :, :L]) != bits(want[b, :, :L])).sum()), "values differ")
        assert (bits(got[b, :, L:]) == NAN_BITS).all(), (label, "row", b, "a column behind frames[b] was written")


class Pool:
    """squared errors of a case's calls against float64, pooled: the 2x rule over all of them"""

    def __init__(self):
        self.g = self.c = self.r = 0.0
        self.n = 0

    def add(self, got, chain, ref):
        ref = np.asarray(ref, np.float64).ravel()
        self.g += float(((np.asarray(got, np.float64).ravel() - ref) ** 2).sum())
        self.c += float(((np.asarray(chain, np.float64).ravel() - ref) ** 2).sum())
        self.r += float((ref ** 2).sum())
        self.n += ref.size

    def hold(self, label):
        c_rms = np.sqrt(self.c / self.r)
        ratio = np.sqrt(self.g / self.c) if self.c else np.inf
        print("%s: %d outputs: gpu / restatement %.2f (restatement rms %.2e of RMS)" % (label, self.n, ratio, c_rms))
        assert self.c > 0 and np.isfinite(c_rms), (label, "the restatement has no error: the rule would be vacuous")
        if self.n >= G.MIN_ELEMS:
            assert ratio <= G.FACTOR, (label, ratio)
        return ratio


# ---- prior sampling -------------------------------------------------------------------------------------------------------------------------------------------
def prior_batch(C, L, turn):
    """the ragged batch of 4 for (channels, frames): (mean, logvar, cum, tok_lens, frames)"""
    kinds = ("zeros_start", "zeros_middle", "zeros_end", "zeros_everywhere")
    durs = [G.durations_case("plain", T_TOK, L), G.durations_case(kinds[turn % 4], 9, max(1, L - 1)), G.durations_case("none", 5, 0), G.durations_case("plain", 1, max(1, L - 2))]
    cum, tok_lens, frames = G.cum_rows(durs, T_TOK)
    rng = np.random.default_rng(C * 1009 + L)
    mean = rng.standard_normal((4, C, T_TOK)).astype(np.float32)
    logvar = (0.5 * rng.standard_normal((4, C, T_TOK))).astype(np.float32)
    return mean, logvar, cum, tok_lens, frames


@pytest.mark.parametrize("C", G.SAMPLE_CHANNELS)
def test_prior_sample_gather_counter_scales_and_float64(pkg, nan_outputs, C):
    pool = Pool()
    for turn, L in enumerate(G.SAMPLE_FRAMES):
        mean, logvar, cum, tok_lens, frames = prior_batch(C, L, turn)
        assert frames[2] == 1 and (G.token_of_frame(cum[2], tok_lens[2], 1) == -1).all()
        ts = int(frames.max()) + 3
        label = "channels %d frames %d" % (C, L)
        kw = dict(t_stride=ts, tok_lens=tok_lens)
        rng = np.random.default_rng(C * 7 + L)
        eps = rng.standard_normal((4, C, ts)).astype(np.float32)
        mu, lv = G.gathered(mean, cum, tok_lens, frames, ts), G.gathered(logvar, cum, tok_lens, frames, ts)
        # the gather alone
        same_valid(label + ": scale 0", pkg.op_prior_sample(mean, logvar, cum, frames, noise=eps, noise_scale=0.0, **kw), mu, frames)
        # the counter stream, each row with its own seed offset
        offs = np.array([5, 0, 9, 2], np.int32)
        draw = G.counter_noise(77, offs, C, frames, ts)
        zero = np.zeros_like(mean)
        same_valid(label + ": counter draw", pkg.op_prior_sample(zero, zero, cum, frames, seed=77, seed_offsets=offs, noise_scale=1.0, **kw), draw, frames)
        same_valid(label + ": counter draw, offsets b", pkg.op_prior_sample(zero, zero, cum, frames, seed=77, noise_scale=1.0, **kw), G.counter_noise(77, None, C, frames, ts), frames)
        got = pkg.op_prior_sample(mean, logvar, cum, frames, seed=77, seed_offsets=offs, noise_scale=0.667, **kw)
        same_valid(label + ": counter vs explicit", pkg.op_prior_sample(mean, logvar, cum, frames, noise=draw, noise_scale=0.667, **kw), got, frames)
        # per-row scales
        scales = np.array([0.667, 0.0, 1.0, 1.25], np.float32)
        rows = pkg.op_prior_sample(mean, logvar, cum, frames, noise=eps, noise_scales=scales, noise_scale=3.0, **kw)
        same_valid(label + ": per-row scales, layout", rows, rows, frames)
        for b in range(4):
            one = pkg.op_prior_sample(mean, logvar, cum, frames, noise=eps, noise_scale=float(scales[b]), **kw)
            assert np.array_equal(bits(one[b, :, :frames[b]]), bits(rows[b, :, :frames[b]])), (label, "per-row scale", b)
        assert np.isfinite(G.valid(rows, frames)).all(), (label, "a value from behind a length (NaN) was read")
        pool.add(G.valid(rows, frames), G.valid(G.prior32(mu, lv, eps, scales), frames), G.valid(G.sample64(mu, lv, eps, scales), frames))
        pool.add(G.valid(got, frames), G.valid(G.prior32(mu, lv, draw, 0.667), frames), G.valid(G.sample64(mu, lv, draw, 0.667), frames))
    pool.hold("prior sample, channels %d, pooled over the frame counts" % C)


@pytest.mark.parametrize("flip", (False, True), ids=("plain", "flip"))
@pytest.mark.parametrize("C", G.SAMPLE_CHANNELS)
def test_posterior_sample_mean_counter_flip_and_float64(pkg, nan_outputs, C, flip):
    pool = Pool()
    for L in G.SAMPLE_FRAMES:
        frames = np.array([L, max(1, L - 1), 1, max(1, L - 2)], np.int32)
        ts = L + 3
        label = "channels %d frames %d flip %d" % (C, L, flip)
        rng = np.random.default_rng(C * 1013 + L)
        mean = rng.standard_normal((4, C, ts)).astype(np.float32)
        logstd = (0.5 * rng.standard_normal((4, C, ts))).astype(np.float32)
        eps = rng.standard_normal((4, C, ts)).astype(np.float32)
        rows = (lambda a: a[:, ::-1]) if flip else (lambda a: a)  # logical channel c -> row C - 1 - c
        nan = np.full((4, C, ts), np.nan, np.float32)
        same_valid(label + ": eps_scale 0", pkg.op_posterior_sample(mean, logstd, frames, noise=nan, flip=flip, eps_scale=0.0), rows(mean), frames)
        same_valid(label + ": eps_scale 0, counter", pkg.op_posterior_sample(mean, logstd, frames, seed=3, flip=flip, eps_scale=0.0), rows(mean), frames)
        offs = np.array([1, 8, 0, 4], np.int32)
        draw = G.counter_noise(91, offs, C, frames, ts)
        zero = np.zeros_like(mean)
        same_valid(label + ": counter draw", pkg.op_posterior_sample(zero, zero, frames, seed=91, seed_offsets=offs, flip=flip), rows(draw), frames)
        got = pkg.op_posterior_sample(mean, logstd, frames, seed=91, seed_offsets=offs, flip=flip)
        same_valid(label + ": counter vs explicit", pkg.op_posterior_sample(mean, logstd, frames, noise=draw, flip=flip), got, frames)
        half = pkg.op_posterior_sample(mean, logstd, frames, noise=eps, flip=flip, eps_scale=0.5)
        same_valid(label + ": layout", half, half, frames)
        assert np.isfinite(G.valid(half, frames)).all() and np.isfinite(G.valid(got, frames)).all(), (label, "a value from behind a length (NaN) was read")
        pool.add(G.valid(half, frames), G.valid(rows(G.posterior32(mean, logstd, eps, 0.5)), frames), G.valid(rows(G.sample64(mean, logstd, eps, 0.5)), frames))
        pool.add(G.valid(got, frames), G.valid(rows(G.posterior32(mean, logstd, draw, 1.0)), frames), G.valid(rows(G.sample64(mean, logstd, draw, 1.0)), frames))
    pool.hold("posterior sample, channels %d flip %d, pooled over the frame counts" % (C, flip))


# ---- conv_post ------------------------------------------------------------------------------------------------------------------------------------------------
def window_equals_whole(label, got, whole, lens, lo, his):
    """[B, T]: samples [lo, min(hi, len)) hold the whole call's bits, every other the staged 0xFF bytes"""
    for b, n in enumerate(lens):
        hi = min(n if his is None else int(his[b]), n)
        w = np.zeros(got.shape[1], bool)
        w[lo:max(lo, hi)] = True
        assert np.array_equal(bits(got[b][w]), bits(whole[b][w])), (label, "row", b, "window", lo, hi, "differs from the whole call")
        assert (bits(got[b][~w]) == NAN_BITS).all(), (label, "row", b, "window", lo, hi, "a sample outside the window was written")


def conv_post_checks(pkg, label, x, w, lens, pool, layout=0, arith_name="f32"):
    """every check of one (cin, k, lengths) on the current arithmetic; returns the whole call's (wave, pre)"""
    B, cin, T = x.shape
    kw = dict(lens=lens, layout=layout)
    wave, pre = pkg.op_conv_post(x, w, SLOPE, **kw)
    window_equals_whole(label + ": whole call, layout", wave, wave, lens, 0, None)
    window_equals_whole(label + ": whole call, pre layout", pre, pre, lens, 0, None)
    for b, n in enumerate(lens):
        assert np.isfinite(pre[b, :n]).all() and np.isfinite(wave[b, :n]).all(), (label, b, "a value from behind lens[b] (NaN) was read")
    cols = np.concatenate([pre[b, :n] for b, n in enumerate(lens)])
    ulps = G.tanh_within(np.concatenate([wave[b, :n] for b, n in enumerate(lens)]), cols)
    assert ulps <= G.TANH_ULP, (label, "wave is not tanh(pre)", ulps)
    ref, chain = G.post_reference(x, w, SLOPE, lens, arith_name)
    pool.add(cols, chain, ref)
    # the other forms of the same call: an odd x pitch (the scalar path), an odd pre pitch (no float4 store), no pre
    for name, over in (("odd x pitch", dict(x_pitch=G.odd_pitch(T))), ("odd pre pitch", dict(pre_pitch=G.odd_pitch(T))), ("both odd", dict(x_pitch=G.odd_pitch(T), pre_pitch=G.odd_pitch(T) + 2))):
        w2, p2 = pkg.op_conv_post(x, w, SLOPE, **kw, **over)
        window_equals_whole(label + ": " + name + ", wave", w2, wave, lens, 0, None)
        window_equals_whole(label + ": " + name + ", pre", p2, pre, lens, 0, None)
    w3, p3 = pkg.op_conv_post(x, w, SLOPE, want_pre=False, **kw)
    assert p3 is None
    window_equals_whole(label + ": no pre", w3, wave, lens, 0, None)
    # windows
    for lo in G.POST_EMIT_LO:
        if lo > T:
            continue
        for pick in range(4):  # (a row with fewer distinct values takes its last one again)
            his = np.array([G.emit_his(int(n), lo)[min(pick, len(G.emit_his(int(n), lo)) - 1)] for n in lens], np.int32)
            w4, p4 = pkg.op_conv_post(x, w, SLOPE, emit_lo=lo, emit_hi=his, **kw)
            window_equals_whole(label + ": window, wave", w4, wave, lens, lo, his)
            window_equals_whole(label + ": window, pre", p4, pre, lens, lo, his)
        w5, p5 = pkg.op_conv_post(x, w, SLOPE, emit_lo=lo, pre_pitch=G.odd_pitch(T), **kw)
        window_equals_whole(label + ": emit_lo alone, wave", w5, wave, lens, lo, None)
        window_equals_whole(label + ": emit_lo alone, odd pre pitch", p5, pre, lens, lo, None)
    return wave, pre


def post_lengths():
    return [[T] for T in G.POST_LENGTHS] + [list(G.POST_RAGGED)]


@pytest.mark.parametrize("c", [(cin, k) for cin in G.POST_CIN for k in G.POST_K], ids=lambda c: "cin%d-k%d" % c)
def test_conv_post_paths_windows_and_float64(pkg, nan_outputs, c):
    cin, k = c
    pkg.op_set_arith(pkg.ARITH_F32)
    pool = Pool()
    for lens in post_lengths():
        x, w = G.post_case(cin, k, max(lens), len(lens))
        conv_post_checks(pkg, "cin %d k %d lens %s" % (cin, k, lens), x, w, lens, pool)
    pool.hold("conv_post cin %d k %d, pooled over the lengths" % c)


@pytest.mark.parametrize("arith_name", ("f16", "bf16"))
@pytest.mark.parametrize("c", [(cin, k) for cin in G.POST16_CIN + G.POST16_CIN_FP32_LAYOUT for k in (3, 7)], ids=lambda c: "cin%d-k%d" % c)
def test_conv_post_16bit_forms(pkg, nan_outputs, c, arith_name):
    cin, k = c
    pkg.op_set_arith(pkg.ARITH_F16 if arith_name == "f16" else pkg.ARITH_BF16)
    try:
        for layout in (pkg.CONV_POST_STREAM, pkg.CONV_POST_FP32_LAYOUT):
            form = "stream" if layout == pkg.CONV_POST_STREAM else "fp32 layout"
            if layout == pkg.CONV_POST_STREAM and cin % 8:
                x, w = G.post_case(cin, k, 13, 1)
                with pytest.raises(pkg.VitsError) as e:
                    pkg.op_conv_post(x, w, SLOPE, layout=layout)
                assert "vits_op_conv_post" in str(e.value) and "cin = %d is no multiple of 8" % cin in str(e.value), str(e.value)
                continue
            pool = Pool()
            for lens in post_lengths():
                x, w = G.post_case(cin, k, max(lens), len(lens))
                conv_post_checks(pkg, "%s %s cin %d k %d lens %s" % (arith_name, form, cin, k, lens), x, w, lens, pool, layout, arith_name)
            pool.hold("conv_post %s %s cin %d k %d, pooled over the lengths" % (arith_name, form, cin, k))
    finally:
        pkg.op_set_arith(pkg.ARITH_F32)


# ---- the sum over a stage's resblocks -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", G.SUM_CASES, ids=lambda c: "c%d-t%d" % c)
def test_resblock_sum_is_numpy_float32(pkg, nan_outputs, c):
    C, T = c
    B = 4
    lens = [T, max(0, T - 1), max(1, T - 255), 0]
    rng = np.random.default_rng(C * 1009 + T)
    y0, y1, y2 = (rng.standard_normal((B, C, T)).astype(np.float32) for _ in range(3))
    for three in (False, True):
        for scale, div in ((1.0 / 3.0, False), (3.0, True), (0.5, False), (1.0, False)):
            for act in (False, True):
                for in_pitch, out_pitch in ((T, T), (T + 3, T + 6), (G.aligned_pitch(T) + 4, T + 1)):
                    label = "c %d t %d three %d scale %g div %d act %d pitches %d %d" % (C, T, three, scale, div, act, in_pitch, out_pitch)
                    got = pkg.op_resblock_sum(y0, y1, y2 if three else None, scale=scale, scale_div=div, act=act, slope=0.1, lens=lens, in_pitch=in_pitch, out_pitch=out_pitch)
                    want = G.sum32(y0, y1, y2 if three else None, scale, div, act, 0.1)
                    same_valid(label, got, want, lens)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause(pkg):
    z = np.zeros((1, 4, 8), np.float32)
    cum = np.arange(1, 9, dtype=np.int32)[None]

    def refused(cause, call):
        with pytest.raises(pkg.VitsError) as e:
            call()
        assert cause in str(e.value), str(e.value)

    refused("frames = 9, outside [0, t_stride = 8]", lambda: pkg.op_prior_sample(z, z, cum, [9], t_stride=8))
    refused("tok_lens", lambda: pkg.op_prior_sample(z, z, cum, [8], tok_lens=[9]))
    refused("every utterance has 0 frames", lambda: pkg.op_prior_sample(z, z, cum, [0], t_stride=8))
    refused("frames = -1", lambda: pkg.op_posterior_sample(z, z, [-1]))
    refused("every utterance has 0 frames", lambda: pkg.op_posterior_sample(z, z, [0]))
    x, w = G.post_case(8, 7, 16, 1)
    refused("an odd tap count", lambda: pkg.op_conv_post(x, w[:, :6], SLOPE))
    refused("must reach t = 16", lambda: pkg.op_conv_post(x, w, SLOPE, x_pitch=15))
    refused("must reach t = 16", lambda: pkg.op_conv_post(x, w, SLOPE, pre_pitch=12))
    refused("emit_lo = 17", lambda: pkg.op_conv_post(x, w, SLOPE, emit_lo=17))
    refused("emit_hi[0] = -2", lambda: pkg.op_conv_post(x, w, SLOPE, emit_hi=[-2]))
    refused("lens", lambda: pkg.op_conv_post(x, w, SLOPE, lens=[17]))
    refused("layout 2", lambda: pkg.op_conv_post(x, w, SLOPE, layout=2))
    refused("exists only in a 16-bit arithmetic", lambda: pkg.op_conv_post(x, w, SLOPE, layout=pkg.CONV_POST_STREAM))
    refused("must reach t = 8", lambda: pkg.op_resblock_sum(z, z, in_pitch=7))
    refused("must reach t = 8", lambda: pkg.op_resblock_sum(z, z, out_pitch=7))
    refused("lens", lambda: pkg.op_resblock_sum(z, z, lens=[9]))
    pkg.op_set_arith(pkg.ARITH_F16)
    try:
        refused("VITS_ARITH_F32 only", lambda: pkg.op_resblock_sum(z, z))
    finally:
        pkg.op_set_arith(pkg.ARITH_F32)
    pkg.op_set_arith(pkg.ARITH_F32_SPLIT)
    try:
        refused("VITS_ARITH_F32_SPLIT", lambda: pkg.op_conv_post(x, w, SLOPE))
    finally:
        pkg.op_set_arith(pkg.ARITH_F32)
