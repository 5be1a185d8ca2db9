// abi_ops_glue.cpp — operator-level entry points of the kernels between the conv families: vits_op_spectrogram (spectrogram.hip), vits_op_prior_sample and
// vits_op_posterior_sample (zp_kernel, posterior_sample_kernel), vits_op_conv_post (conv_post_kernel, and in a 16-bit arithmetic the converter +
// conv_post16_kernel as engine_vocoder.cpp runs them) and vits_op_resblock_sum (rb_sum3_std_kernel). Host arrays in, host arrays out; staging: abi_ops_common.h.
// Every operator calls the engine's own launcher; what a launcher cannot take is refused with the cause named, before the first device call.
#include "abi_ops_common.h"

using namespace vits;

namespace {
std::string at(const char* op, int b) { return std::string(op) + ": utterance " + std::to_string(b) + " "; }
// frames[b] in [0, t_stride]; the longest in lmax
bool frames_ok(const char* op, const int32_t* frames, int batch, int t_stride, int& lmax) {
    lmax = 0;
    for (int b = 0; b < batch; ++b) {
        if (frames[b] < 0 || frames[b] > t_stride) return refuse(at(op, b) + "has frames = " + std::to_string(frames[b]) + ", outside [0, t_stride = " + std::to_string(t_stride) + "]");
        lmax = std::max(lmax, (int)frames[b]);
    }
    return true;
}
}  // namespace

VITS_API int vits_op_spectrogram(int32_t n_fft, int32_t hop, int32_t bins, int32_t batch, const float* pcm, int64_t pcm_stride, const int32_t* n_samples,
                                 int32_t t_stride, float* out) {
    VITS_TRY
    const char* op = "vits_op_spectrogram";
    if (!pcm || !n_samples || !out || batch < 1 || pcm_stride < 1) return fail("vits_op_spectrogram: null argument, empty batch or pcm_stride < 1");
    if (const std::string why = stft_geometry(n_fft, hop); !why.empty()) return fail("vits_op_spectrogram: " + why);
    if (bins < 1 || bins > n_fft / 2 + 1) return fail("vits_op_spectrogram: bins = " + std::to_string(bins) + " is outside [1, n_fft / 2 + 1 = " + std::to_string(n_fft / 2 + 1) + "]");
    const int pad = stft_pad(n_fft, hop), min_n = stft_min_samples(n_fft, hop);
    std::vector<int32_t> frames(batch);
    int nmax = 0, tmax = 0;
    for (int b = 0; b < batch; ++b) {
        const int64_t n = n_samples[b];
        if (n > pcm_stride) return fail(at(op, b) + "has n_samples = " + std::to_string(n) + ", beyond pcm_stride " + std::to_string(pcm_stride));
        if (n > ((int64_t)1 << 30)) return fail(at(op, b) + "is longer than 2^30 samples");
        if (n < min_n)
            return fail(at(op, b) + "has " + std::to_string(n) + " samples: at least " + std::to_string(min_n) + " are needed (one hop, and more than the reflection pad of " +
                        std::to_string(pad) + ")");
        frames[b] = (int32_t)(n / hop);  // spectrogram_torch: floor(N / hop) frames
        nmax = std::max(nmax, (int)n), tmax = std::max(tmax, (int)frames[b]);
    }
    if (t_stride < tmax) return fail("vits_op_spectrogram: t_stride = " + std::to_string(t_stride) + " is shorter than the longest row (" + std::to_string(tmax) + " frames)");
    std::vector<float> tw, win;
    stft_tables(n_fft, tw, win);
    const int64_t pitch = round_up(nmax, 64) + 64;  // the engine's PCM stride and 64 samples to spare: NaN behind every utterance, the longest included
    const size_t ny = (size_t)batch * bins * t_stride * 4;
    DevMem dx, dy, dn, df, dtw, dwin;
    if (!stage_rows(dx, pcm, batch, 1, pcm_stride, pitch, n_samples, 0) || !dy.fill(ny, g_op_out_fill) || !dn.put(n_samples, (size_t)batch * 4) ||
        !df.put(frames.data(), (size_t)batch * 4) || !dtw.put(tw.data(), tw.size() * 4) || !dwin.put(win.data(), win.size() * 4))
        return -1;
    SpectrogramCall sc;
    sc.pcm = dx.f();
    sc.pcm_stride = pitch;
    sc.n_samples = dn.i();
    sc.frames = df.i();
    sc.tw = static_cast<const float2*>(dtw.p);
    sc.win = dwin.f();
    sc.n_fft = n_fft, sc.hop = hop, sc.pad = pad, sc.bins = bins, sc.batch = batch, sc.tmax = tmax;
    sc.out = tref(dy.f(), bins, t_stride);
    return finish(launch_spectrogram(sc, nullptr), op) && dy.get(out, ny) ? 0 : -1;
    VITS_CATCH(-1)
}

VITS_API int vits_op_prior_sample(int32_t batch, int32_t channels, int32_t t_tok, int32_t t_stride, const float* mean, const float* logvar, const int32_t* cum,
                                  const int32_t* tok_lens, const int32_t* frames, const float* noise, uint64_t seed, const int32_t* seed_offsets, float noise_scale,
                                  const float* noise_scales, float* zp) {
    VITS_TRY
    const char* op = "vits_op_prior_sample";
    if (!mean || !logvar || !cum || !frames || !zp) return fail("vits_op_prior_sample: null argument (mean, logvar, cum, frames and zp are required)");
    if (batch < 1 || channels < 1 || t_tok < 1 || t_stride < 1) return fail("vits_op_prior_sample: batch, channels, t_tok and t_stride are at least 1");
    if (!lens_ok(tok_lens, batch, t_tok)) return fail("vits_op_prior_sample: 0 <= tok_lens[b] <= t_tok is required");
    int lmax = 0;
    if (!frames_ok(op, frames, batch, t_stride, lmax)) return -1;
    if (lmax < 1) return fail("vits_op_prior_sample: every utterance has 0 frames: nothing to launch");
    const size_t nz = (size_t)batch * channels * t_stride * 4;
    DevMem dm, dv, dc, dt, df, dnz, dso, dns, dz;
    if (!stage_rows(dm, mean, batch, channels, t_tok, t_tok, tok_lens, t_tok) || !stage_rows(dv, logvar, batch, channels, t_tok, t_tok, tok_lens, t_tok) ||
        !dc.put(cum, (size_t)batch * t_tok * 4) || !dt.put_opt(tok_lens, (size_t)batch * 4) || !df.put(frames, (size_t)batch * 4) ||
        (noise && !stage_rows(dnz, noise, batch, channels, t_stride, t_stride, frames, 0)) || !dso.put_opt(seed_offsets, (size_t)batch * 4) ||
        !dns.put_opt(noise_scales, (size_t)batch * 4) || !dz.fill(nz, g_op_out_fill))
        return -1;
    const hipError_t e = launch_zp(tref(dm.f(), channels, t_tok), tref(dv.f(), channels, t_tok), dc.i(), t_tok, dt.i(), df.i(), tref(dnz.f(), channels, t_stride),
                                   noise ? VITS_NOISE_EXPLICIT : VITS_NOISE_COUNTER, seed, dso.i(), noise_scale, dns.f(), tref(dz.f(), channels, t_stride), batch, channels, lmax,
                                   nullptr);
    return finish(e, op) && dz.get(zp, nz) ? 0 : -1;
    VITS_CATCH(-1)
}

VITS_API int vits_op_posterior_sample(int32_t batch, int32_t channels, int32_t t_stride, const float* mean, const float* logstd, const int32_t* frames,
                                      const float* noise, uint64_t seed, const int32_t* seed_offsets, int32_t flip, float eps_scale, float* zq) {
    VITS_TRY
    const char* op = "vits_op_posterior_sample";
    if (!mean || !logstd || !frames || !zq) return fail("vits_op_posterior_sample: null argument (mean, logstd, frames and zq are required)");
    if (batch < 1 || channels < 1 || t_stride < 1) return fail("vits_op_posterior_sample: batch, channels and t_stride are at least 1");
    if (flip != 0 && flip != 1) return fail("vits_op_posterior_sample: flip is 0 or 1");
    int lmax = 0;
    if (!frames_ok(op, frames, batch, t_stride, lmax)) return -1;
    if (lmax < 1) return fail("vits_op_posterior_sample: every utterance has 0 frames: nothing to launch");
    const size_t nz = (size_t)batch * channels * t_stride * 4;
    DevMem dm, dv, df, dnz, dso, dz;
    if (!stage_rows(dm, mean, batch, channels, t_stride, t_stride, frames, 0) || !stage_rows(dv, logstd, batch, channels, t_stride, t_stride, frames, 0) ||
        !df.put(frames, (size_t)batch * 4) || (noise && !stage_rows(dnz, noise, batch, channels, t_stride, t_stride, frames, 0)) ||
        !dso.put_opt(seed_offsets, (size_t)batch * 4) || !dz.fill(nz, g_op_out_fill))
        return -1;
    const hipError_t e = launch_posterior_sample(tref(dm.f(), channels, t_stride), tref(dv.f(), channels, t_stride), df.i(), tref(dnz.f(), channels, t_stride),
                                                 noise ? VITS_NOISE_EXPLICIT : VITS_NOISE_COUNTER, seed, dso.i(), tref(dz.f(), channels, t_stride), batch, channels, lmax,
                                                 flip, nullptr, eps_scale);
    return finish(e, op) && dz.get(zq, nz) ? 0 : -1;
    VITS_CATCH(-1)
}

VITS_API int vits_op_conv_post(const vits_conv_post_desc* d, const float* x, const float* w, const int32_t* lens, const int32_t* emit_hi, float* pre, float* wave) {
    VITS_TRY
    const char* op = "vits_op_conv_post";
    if (!d || !x || !w || !wave) return fail("vits_op_conv_post: null argument (the descriptor, x, w and wave are required)");
    const int B = d->batch, cin = d->cin, k = d->k, T = d->t, arith = g_op_arith;
    if (B < 1 || cin < 1 || T < 1) return fail("vits_op_conv_post: batch, cin and t are at least 1");
    if (k < 1 || !(k & 1)) return fail("vits_op_conv_post: k = " + std::to_string(k) + ": an odd tap count is required");
    if (d->x_pitch < T || d->pre_pitch < T)
        return fail("vits_op_conv_post: x_pitch = " + std::to_string(d->x_pitch) + " and pre_pitch = " + std::to_string(d->pre_pitch) + " must reach t = " + std::to_string(T));
    if (!lens_ok(lens, B, T)) return fail("vits_op_conv_post: 0 <= lens[b] <= t is required");
    if (d->emit_lo < 0 || d->emit_lo > T) return fail("vits_op_conv_post: emit_lo = " + std::to_string(d->emit_lo) + " is outside [0, t = " + std::to_string(T) + "]");
    for (int b = 0; emit_hi && b < B; ++b)
        if (emit_hi[b] < 0) return fail("vits_op_conv_post: emit_hi[" + std::to_string(b) + "] = " + std::to_string(emit_hi[b]) + " is negative");
    if (arith == VITS_ARITH_F32_SPLIT) return fail("vits_op_conv_post: VITS_ARITH_F32_SPLIT has no conv_post of its own (the engine runs the fp32 kernel)");
    if (d->layout != VITS_CONV_POST_FP32_LAYOUT && d->layout != VITS_CONV_POST_STREAM) return fail("vits_op_conv_post: layout " + std::to_string(d->layout) + " is not a layout");
    const bool stream = d->layout == VITS_CONV_POST_STREAM;
    if (stream && arith == VITS_ARITH_F32) return fail("vits_op_conv_post: the streaming form (conv_post16_kernel) exists only in a 16-bit arithmetic (vits_op_set_arith)");
    if (stream && (cin & 7))
        return fail("vits_op_conv_post: cin = " + std::to_string(cin) + " is no multiple of 8: conv_post16_kernel reads whole groups of eight channels (the fp32-layout form takes any cin)");
    const size_t nw = (size_t)B * T * 4, npre = (size_t)B * d->pre_pitch * 4;
    DevMem dx, dw, dl, dh, dp, dv, dx16;
    if (!stage_rows(dx, x, B, cin, T, d->x_pitch, lens, T) || !dw.put(w, (size_t)cin * k * 4) || !dl.put_opt(lens, (size_t)B * 4) || !dh.put_opt(emit_hi, (size_t)B * 4) ||
        (pre && !dp.fill(npre, g_op_out_fill)) || !dv.fill(nw, g_op_out_fill))
        return -1;
    const TensorRef rx = tref(dx.f(), cin, d->x_pitch), rpre = tref(dp.f(), 1, d->pre_pitch), rwave = tref(dv.f(), 1, T);
    hipError_t e;
    if (!stream) {
        e = launch_conv_post(rx, dw.f(), cin, k, d->slope, rpre, rwave, dl.i(), B, T, nullptr, d->emit_lo, dh.i(), arith);
    } else {
        // engine_vocoder.cpp's streaming path: the last stage's 16-bit copy carries conv_post's leaky_relu; the kernel reads that copy alone
        if (!dx16.fill(group16_bytes(B, cin, T), 0xFF)) return -1;
        Ref16 r;
        r.p = dx16.h(), r.ts = round_up(T, 8), r.bs = (int64_t)(cin / 8) * r.ts * 8;
        e = launch_to_group16(rx, dl.i(), B, cin, T, d->slope, r, arith, nullptr);
        if (e == hipSuccess) e = launch_conv_post16(r, dw.f(), cin, k, rpre, rwave, dl.i(), B, T, arith, nullptr, d->emit_lo, dh.i());
    }
    if (!finish(e, op)) return -1;
    if (pre && !unstage_rows(dp, pre, B, 1, d->pre_pitch, T, T)) return -1;
    return dv.get(wave, nw) ? 0 : -1;
    VITS_CATCH(-1)
}

VITS_API int vits_op_resblock_sum(int32_t batch, int32_t channels, int32_t t, int32_t in_pitch, int32_t out_pitch, float scale, int32_t scale_div, int32_t act,
                                  float slope, const float* y0, const float* y1, const float* y2, const int32_t* lens, float* out) {
    VITS_TRY
    const char* op = "vits_op_resblock_sum";
    if (!y0 || !y1 || !out) return fail("vits_op_resblock_sum: null argument (y0, y1 and out are required: two or three addends)");
    if (batch < 1 || channels < 1 || t < 1) return fail("vits_op_resblock_sum: batch, channels and t are at least 1");
    if (in_pitch < t || out_pitch < t)
        return fail("vits_op_resblock_sum: in_pitch = " + std::to_string(in_pitch) + " and out_pitch = " + std::to_string(out_pitch) + " must reach t = " + std::to_string(t));
    if (!lens_ok(lens, batch, t)) return fail("vits_op_resblock_sum: 0 <= lens[b] <= t is required");
    if ((scale_div != 0 && scale_div != 1) || (act != 0 && act != 1)) return fail("vits_op_resblock_sum: scale_div and act are 0 or 1");
    if (g_op_arith != VITS_ARITH_F32) return fail("vits_op_resblock_sum: VITS_ARITH_F32 only (the 16-bit vocoder adds its resblocks in their epilogues)");
    DevMem d0, d1, d2, dl, dy;
    if (!stage_rows(d0, y0, batch, channels, t, in_pitch, lens, t) || !stage_rows(d1, y1, batch, channels, t, in_pitch, lens, t) ||
        (y2 && !stage_rows(d2, y2, batch, channels, t, in_pitch, lens, t)) || !dl.put_opt(lens, (size_t)batch * 4) ||
        !dy.fill((size_t)batch * channels * out_pitch * 4, g_op_out_fill))
        return -1;
    const hipError_t e = launch_rb_sum3_std(tref(d0.f(), channels, in_pitch), tref(d1.f(), channels, in_pitch), y2 ? tref(d2.f(), channels, in_pitch) : TensorRef(),
                                            tref(dy.f(), channels, out_pitch), channels, dl.i(), batch, t, scale, scale_div, act ? 2 : 0, slope, nullptr);
    return finish(e, op) && unstage_rows(dy, out, batch, channels, out_pitch, t, t) ? 0 : -1;
    VITS_CATCH(-1)
}
