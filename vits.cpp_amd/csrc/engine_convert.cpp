// engine_convert.cpp — voice conversion (VITS SynthesizerTrn.voice_conversion; include/vits.h vits_model_convert_batch): PCM of a source
// speaker -> linear spectrogram (spectrogram.hip) -> posterior encoder with the source speaker (transformers VitsPosteriorEncoder: conv_pre,
// WaveNet, conv_proj, sample) -> coupling flow forward with the source speaker = z_p; from there the text-to-speech tail: the flow in reverse
// and the vocoder, both with the target speaker (engine.cpp run_stage_two).
#include "engine_internal.h"

namespace vits {

// ---- weights: built on first use, from the host copies load() kept -------------------------------------------------------------
int Engine::prepare_conversion(std::string& err) {
    if (vc_ready_) return 0;
    const int H = hp.hidden, F = hp.flow_size, nl = hp.post_wn_layers, bins = hp.spec_bins;
    ModelFile f;
    f.tensors = vc_src_;
    if (!f.find("posterior_encoder.conv_pre.weight")) {
        err = "model file has no posterior encoder (posterior_encoder.* tensors): voice conversion needs them";
        return -1;
    }
    // the STFT of spectrogram_torch: n_fft = 2 (bins - 1), hop = the vocoder's samples per frame, reflection pad (n_fft - hop) / 2
    int hop = 1;
    for (int r : hp.up_rates) hop *= r;
    const int n_fft = 2 * (bins - 1);
    if (const std::string why = stft_geometry(n_fft, hop); !why.empty()) {
        err = "spectrogram_bins = " + std::to_string(bins) + " and the upsample rates' product " + std::to_string(hop) + " give " + why;
        return -1;
    }
    if (nl < 1) {
        err = "posterior_encoder_num_wavenet_layers must be at least 1";
        return -1;
    }
    HIP_OK(hipStreamSynchronize(stream));
    const size_t first_pack = packs_.size();
    // (vectors sized before anything is packed: packs_ keeps pointers to their entries)
    post_.in_layers.assign(nl, PackedConv());
    post_.res_skip.assign(nl, PackedConv());
    flow_fwd_post_.assign(hp.n_flows, PackedConv());
    const std::string b = "posterior_encoder.";
    if (!pack(f, b + "conv_pre.weight", b + "conv_pre.bias", EPI_STD, {H, bins, 1}, post_.pre, err)) return -1;
    for (int l = 0; l < nl; ++l) {
        const std::string sl = std::to_string(l);
        if (!pack(f, b + "wavenet.in_layers." + sl + ".weight", b + "wavenet.in_layers." + sl + ".bias", EPI_GATE, {2 * H, H, hp.wn_k}, post_.in_layers[l], err)) return -1;
        if (!pack(f, b + "wavenet.res_skip_layers." + sl + ".weight", b + "wavenet.res_skip_layers." + sl + ".bias", EPI_STD, {l + 1 < nl ? 2 * H : H, H, 1},
                  post_.res_skip[l], err))
            return -1;
    }
    if (!pack(f, b + "conv_proj.weight", b + "conv_proj.bias", EPI_STD, {2 * F, H, 1}, post_.proj, err)) return -1;
    // the forward flow's conv_post: x1 += mean — the reverse flow's packs without the negation, same output-channel reversal
    for (int i = 0; i < hp.n_flows; ++i) {
        const std::string fb = "flow.flows." + std::to_string(i) + ".";
        const bool flipped = ((hp.n_flows - i) % 2) == 1;
        if (!pack(f, fb + "conv_post.weight", fb + "conv_post.bias", EPI_STD, {F / 2, H, 1}, flow_fwd_post_[i], err, 0, flipped ? 4 : 0)) return -1;
    }
    // speaker terms of the posterior's WaveNet: its own effective-bias table (row 0 = speaker -1 = the plain biases), built like load_speakers' table
    if (hp.num_speakers > 1) {
        const int E = hp.speaker_embedding_size, N = hp.num_speakers;
        const TensorEntry *te = f.find("embed_speaker.weight"), *tw = f.find(b + "wavenet.cond_layer.weight"), *tb = f.find(b + "wavenet.cond_layer.bias");
        if (!te || !tw || !tb) {
            err = std::string("[ERROR] tensor not found: ") + (!te ? "embed_speaker.weight" : !tw ? "posterior_encoder.wavenet.cond_layer.weight" : "posterior_encoder.wavenet.cond_layer.bias");
            return -1;
        }
        if (te->count() != (int64_t)E * N || tw->count() != (int64_t)2 * H * nl * E || tb->count() != (int64_t)2 * H * nl || te->dtype > DT_BF16 || tw->dtype > DT_BF16 ||
            tb->dtype > DT_BF16) {
            err = "tensor 'posterior_encoder.wavenet.cond_layer' must be a [" + std::to_string(2 * H * nl) + ", " + std::to_string(E) + ", 1] conv with a bias";
            return -1;
        }
        // custom voices (engine_voices.cpp): this table takes the same rows as load_speakers' — the voices registered so far now (the same kernel and
        // vectors as a registration after this call: the same rows either way), later ones as they come
        VoiceTable vt;  // (becomes vt_post_ only once it holds the registered voices' rows: a failure below leaves the registry serving the main table alone)
        vt.rs = (int64_t)nl * 2 * H;  // segments of 2H floats: multiples of four (float4 bias loads)
        for (int l = 0; l < nl; ++l) vt.segs.push_back({&post_.in_layers[l], 2 * H, (int64_t)2 * H * l});
        vt.cond_w = tw->to_f32();
        vt.cond_b = tb->to_f32();
        if (!build_speaker_table(vt, te->to_f32())) {
            err = "could not build the posterior encoder's speaker bias table on the device";
            return -1;
        }
        if (num_voices() > 0 && voice_rows({&vt}, voices_.data(), num_voices(), 1 + N, err)) return -1;
        vt_post_ = std::move(vt);
    }
    // STFT tables, in double, rounded once to fp32: twiddles exp(-2 pi i m / n) and the periodic Hann window (torch.hann_window(n))
    {
        std::vector<float> tw, win;
        stft_tables(n_fft, tw, win);
        if (!(stft_tw_ = upload(tw)) || !(stft_win_ = upload(win))) {
            err = "hipMalloc failed for the STFT tables";
            return -1;
        }
    }
    n_fft_ = n_fft;
    hop_ = hop;
    stft_pad_ = stft_pad(n_fft, hop);
    // a handle already in a 16-bit arithmetic: the new convs get their fragments now (set_arith packs only on a change of mode)
    if (arith == VITS_ARITH_F16 || arith == VITS_ARITH_BF16) {
        for (size_t i = first_pack; i < packs_.size(); ++i) {
            PackSrc& ps = packs_[i];
            HIP_OK(pack16_device(ps, arith, &ps.pc->wp16, &ps.pc->bytes16));  // (a buffer whose upload failed is the conv's all the same: freed with the handle)
        }
    }
    lat16_ready_ = false;  // (the latency kernels' copy of the new layers is made by ensure_lat16 at the next small call)
    HIP_OK(hipDeviceSynchronize());
    vc_ready_ = true;
    return 0;
}

// the PCM side of a call (conversion and alignment): every utterance inside its row, at least one hop and more than the reflection pad; nmax = the longest
// as given, n_model = every utterance's samples at the model's rate (the given count, or with an input rate set ceil(N L / M): what the length rule applies to)
int Engine::check_conversion_pcm(const int64_t* pcm_lens, int B, int64_t pcm_stride, int64_t& nmax, std::vector<int64_t>& n_model, std::string& err) const {
    const int pad = stft_pad_, min_n = stft_min_samples(n_fft_, hop_);
    ResamplePlan plan;
    if (input_rate_ && !resample_plan(input_rate_, hp.sampling_rate, plan, err)) return -1;
    nmax = 0;
    n_model.resize(B);
    for (int b = 0; b < B; ++b) {
        const int64_t n = pcm_lens[b];
        if (n > pcm_stride) {
            err = "pcm_lengths[" + std::to_string(b) + "] = " + std::to_string(n) + " exceeds pcm_stride " + std::to_string(pcm_stride);
            return -1;
        }
        if (n > ((int64_t)1 << 30)) {
            err = "utterance " + std::to_string(b) + " is longer than 2^30 samples";
            return -1;
        }
        const int64_t nm = n_model[b] = n < 0 ? n : plan.out_len(n);
        if (nm < min_n) {
            err = "utterance " + std::to_string(b) + " has " + std::to_string(n) + " samples" +
                  (input_rate_ ? " at " + std::to_string(input_rate_) + " Hz = " + std::to_string(nm) + " at the model's " + std::to_string(hp.sampling_rate) + " Hz" : std::string()) +
                  ": at least " + std::to_string(min_n) + " are needed (one hop, and more than the reflection pad of " + std::to_string(pad) + ")";
            return -1;
        }
        if (nm > ((int64_t)1 << 30)) {
            err = "utterance " + std::to_string(b) + " is longer than 2^30 samples at the model's rate (" + std::to_string(n) + " given, " + std::to_string(nm) + " resampled)";
            return -1;
        }
        nmax = std::max(nmax, n);
    }
    return 0;
}

// frame counts, vocoder stage lengths and the call's own arena (the current stage-one slot): header ints | PCM | spectrogram | posterior statistics;
// uploads the header and the PCM. Leaves c.s1.lens / frames / stage_lens / seed_off pointing into that header.
int Engine::layout_conversion(Call& c, const float* pcm, const int64_t* pcm_lens, int64_t pcm_stride, const int32_t* src, const int32_t* tgt, int64_t nmax,
                              const std::vector<int64_t>& n_model) {
    std::string& err = c.err;
    const vits_process_opts& o = c.o;
    Call::Vc& vc = *c.vc;
    const int B = c.B, hop = hop_, n_up = c.n_up;
    // frame counts and vocoder stage lengths, all on the host (spectrogram_torch: floor(N / hop) frames)
    c.frames.resize(B);
    for (int b = 0; b < B; ++b) c.frames[b] = (int)(n_model[b] / hop);
    // an input rate (vits_model_set_rates): the caller's PCM goes to scratch of this arena and resample.hip writes vc.pcm at the model's rate
    const RateTable* rate_in = nullptr;
    if (input_rate_ && !(rate_in = rate_table(input_rate_, hp.sampling_rate, err))) return -1;
    const int64_t nmax_model = *std::max_element(n_model.begin(), n_model.end());
    set_stage_affine(c);
    c.frames_known();
    if (!lat16_ready_ && knobs.lat16_lazy_tokens > 0 && (int64_t)B * c.Lmax <= knobs.lat16_lazy_tokens && ensure_lat16(err)) return -1;
    // ---- the call's own arena (the current stage-one slot): header ints | PCM | spectrogram | posterior statistics ----------------------
    const int ls = round_up(c.Lmax, 32), bins = hp.spec_bins, F = hp.flow_size;
    const int64_t pstride = round_up((int)nmax_model, 64), raw_stride = round_up((int)nmax, 64);
    const size_t hdr_ints = (size_t)(n_up + 1) * B + (rate_in ? 5 : 4) * (size_t)B;
    float* raw = nullptr;
    auto layout = [&](Arena& a) {
        c.s1.stage_lens = a.alloc<int>(hdr_ints);  // stage_lens [n_up + 1][B] | n_samples | seed_off | src rows | tgt rows [| samples as given]
        raw = rate_in ? a.alloc<float>((size_t)B * raw_stride) : nullptr;
        vc.nsamp = c.s1.stage_lens + (size_t)(n_up + 1) * B;
        c.s1.seed_off = vc.nsamp + B;
        vc.pcm = a.alloc<float>((size_t)B * pstride);
        vc.spec = a.alloc<float>((size_t)B * bins * ls);
        vc.stats = a.alloc<float>((size_t)B * 2 * F * ls);
    };
    if (arena_layout(a1(), stream, err, layout)) return -1;
    vc.pcm_stride = pstride;
    {
        std::vector<int> hdr(hdr_ints, 0);
        bool any_src = false, any_tgt = false;
        for (int i = 0; i <= n_up; ++i)
            for (int b = 0; b < B; ++b) hdr[(size_t)i * B + b] = c.slen[i][b];
        for (int b = 0; b < B; ++b) {
            int* h = hdr.data() + (size_t)(n_up + 1) * B;
            h[b] = (int)n_model[b];
            if (rate_in) h[4 * B + b] = (int)pcm_lens[b];
            h[B + b] = o.noise_seed_offsets ? o.noise_seed_offsets[b] : b;
            const int s = src ? src[b] : -1, t = tgt ? tgt[b] : -1;
            h[2 * B + b] = s + 1;
            h[3 * B + b] = t + 1;
            any_src = any_src || s >= 0;
            any_tgt = any_tgt || t >= 0;
        }
        // (pageable sources: both copies are complete when hipMemcpy* returns to the host, so the caller's PCM and hdr may go)
        HIP_OK(hipMemcpyAsync(c.s1.stage_lens, hdr.data(), sizeof(int) * hdr_ints, hipMemcpyHostToDevice, stream));
        HIP_OK(hipMemcpy2DAsync(rate_in ? raw : vc.pcm, (size_t)(rate_in ? raw_stride : pstride) * 4, pcm, (size_t)pcm_stride * 4, (size_t)nmax * 4, (size_t)B,
                                hipMemcpyHostToDevice, stream));
        HIP_OK(hipStreamSynchronize(stream));
        prof.fence();
        if (rate_in) {
            ResampleCall rc;
            rc.x = raw;
            rc.x_stride = raw_stride;
            rc.lens = vc.nsamp + 4 * B;
            rc.y = vc.pcm;
            rc.y_stride = pstride;
            rc.taps = rate_in->taps;
            rc.plan = rate_in->plan;
            rc.batch = B;
            rc.max_range = nmax_model;
            int64_t in_s = 0, out_s = 0;
            for (int b = 0; b < B; ++b) in_s += pcm_lens[b], out_s += n_model[b];
            HIP_OK(resample("resample_in", rc, in_s, out_s));
            if (o.collect_taps) {
                TensorRef t;
                t.p = vc.pcm;
                t.bs = pstride;
                t.cs = (int)pstride;
                snapshot("pcm_model", t, 1, (int)nmax_model, B, std::vector<int>(n_model.begin(), n_model.end()));
            }
        }
        vc.spk_src = any_src ? vc.nsamp + 2 * B : nullptr;
        vc.spk_tgt = any_tgt ? vc.nsamp + 3 * B : nullptr;
    }
    c.s1.lens = c.s1.stage_lens;  // (frames per utterance = stage-0 lengths)
    c.s1.frames = c.s1.stage_lens;
    return 0;
}

// ---- one conversion call -------------------------------------------------------------------------------------------------------
int Engine::convert_batch(const float* pcm, const int64_t* pcm_lens, int B, int64_t pcm_stride, const int32_t* src, const int32_t* tgt, const vits_process_opts& o,
                          vits_batch_result* out, std::string& err) {
    ResolvedConversion rc(*this);  // (first of all: the pairs given for this conversion are taken, whatever becomes of it)
    std::vector<float> given;
    FitGiven fit_given;
    const bool fit_was_given = take_fit(fit_given);  // (taken with the ratios: whatever becomes of this call, both are gone)
    if (take_pitch_ratios(given)) {
        err = "voice conversion does not take the ratios of vits_model_set_pitch_ratios (a pitch is paid for by the duration predictor's stretch, and a conversion "
              "predicts no durations)";
        return -1;
    }
    if (fit_was_given) {
        err = "voice conversion does not take the fit of vits_model_set_fit (a conversion predicts no durations to fit; its time stretch is "
              "vits_model_set_conversion_prosody)";
        return -1;
    }
    if (refuse_pending(err)) return -1;
    if (B <= 0 || !pcm || !pcm_lens || pcm_stride <= 0) {
        err = B <= 0 ? "empty batch" : "null PCM, null lengths or pcm_stride <= 0";
        return -1;
    }
    if (const char* what = first_set({{"fixed_duration", o.fixed_duration > 0}, {"frames_only", o.frames_only != 0}, {"async", o.async != 0}})) {
        err = std::string("voice conversion does not take ") + what + " (the frame counts come from the input PCM; the call is synchronous)";
        return -1;
    }
    if (o.speaker_ids) {
        err = "voice conversion takes its speakers from src_speakers and tgt_speakers, not from opts.speaker_ids";
        return -1;
    }
    if (const char* what = prosody_opt_set(o)) {
        err = std::string("voice conversion does not take opts.") + what + " (it has no duration prediction, and the posterior draw has no noise scale)";
        return -1;
    }
    if (o.on_chunk && o.skip_host_copy) {
        err = "on_chunk needs a host copy (skip_host_copy = 0)";
        return -1;
    }
    for (int b = 0; b < B; ++b)
        for (int side = 0; side < 2; ++side) {
            const int32_t* arr = side ? tgt : src;
            const int s = arr ? arr[b] : -1;
            if (s == -1) continue;
            const std::string who = std::string(side ? "tgt_speakers[" : "src_speakers[") + std::to_string(b) + "] = " + std::to_string(s) + " (" +
                                    (side ? "target" : "source") + " speaker of utterance " + std::to_string(b) + ")";
            if (check_speaker(s, who, err)) return -1;
        }
    // a rate and a pitch (include/vits.h "a stated tempo"): with every value 1 both stay null and the call is what it always was
    if (resolve_conversion_prosody(B, o, rc, err)) return -1;
    ScopedSet<const float*> tempo_scope(call_tempo_, rc.tempo), pitch_scope(call_pitch_, rc.pitch);
    DeliveryPlan refusable;  // (the refusals of the delivery chain, before anything is queued)
    if (plan_delivery(o, refusable, err)) return -1;
    clear_reports();
    if (prepare_conversion(err)) return -1;
    int64_t nmax = 0;
    std::vector<int64_t> n_model;
    if (check_conversion_pcm(pcm_lens, B, pcm_stride, nmax, n_model, err)) return -1;
    a1_slot_ = 0;
    Call c(o, err, nullptr, B, 0);
    Call::Vc vc;
    c.vc = &vc;
    c.tempo = call_tempo_, c.pitch = call_pitch_;
    c.md = o.mode == VITS_MODE_DEFAULT ? mode : o.mode;
    c.refmode = c.md == VITS_MODE_REFERENCE;
    c.n_up = (int)ups_.size();
    clear_taps();
    tap_batch_ = B;
    arith_now_ = arith_kernels();
    if (layout_conversion(c, pcm, pcm_lens, pcm_stride, src, tgt, nmax, n_model)) return -1;
    return run_stage_two(c, out, nullptr, false);
}

// ---- spectrogram -> posterior encoder -> forward flow: z_p in s2.zp ------------------------------------------------------------------------------
int Engine::run_conversion_front(Call& c) {
    std::string& err = c.err;
    const vits_process_opts& o = c.o;
    Call::Vc& vc = *c.vc;
    Call::S2& s2 = c.s2;
    const int B = c.B, Lmax = c.Lmax, ls = c.ls, H = hp.hidden, F = hp.flow_size, bins = hp.spec_bins;
    const std::vector<int>& frames = c.frames;
    const int64_t sum_frames = c.sum_frames;
    const int* ll = c.d_len_full[0];
    auto TR = make_ref;
    auto sub = sub_rows;
    // spectrogram
    c.rx.phase("vits.spectrogram");
    TensorRef spec = TR(vc.spec, bins, ls);
    {
        SpectrogramCall sc;
        sc.pcm = vc.pcm;
        sc.pcm_stride = vc.pcm_stride;
        sc.n_samples = vc.nsamp;
        sc.frames = ll;
        sc.tw = reinterpret_cast<const float2*>(stft_tw_);
        sc.win = stft_win_;
        sc.n_fft = n_fft_;
        sc.hop = hop_;
        sc.pad = stft_pad_;
        sc.bins = bins;
        sc.batch = B;
        sc.tmax = Lmax;
        sc.out = spec;
        // algorithmic bytes: every sample once, every bin once
        int64_t samples = 0;
        for (int b = 0; b < B; ++b) samples += (int64_t)frames[b] * hop_ + 2 * stft_pad_;
        int log2n = 0;
        while ((1 << log2n) < n_fft_) ++log2n;
        prof.begin("spectrogram", 5.0 * n_fft_ * log2n * (double)sum_frames, 4.0 * (double)samples + 4.0 * (double)bins * sum_frames, stream, true);
        HIP_OK(launch_spectrogram(sc, stream));
        prof.end(stream);
    }
    if (o.collect_taps) snapshot("spec", spec, bins, Lmax, B, frames);
    // posterior encoder, conditioned on the source speaker
    c.rx.phase("vits.posterior");
    TensorRef hout = TR(s2.hout, 2 * H, ls), stats = TR(vc.stats, 2 * F, ls);
    const int* spk = c.spk = vc.spk_src;  // (the posterior encoder and the forward flow: the source speaker)
    auto mk = [&](TensorRef xin, TensorRef yout) {
        ConvCall k;
        k.x = xin;
        k.y = yout;
        k.len_in = ll;
        k.len_out = ll;
        k.spk = spk;
        k.batch = B;
        k.t_in = k.t_out = Lmax;
        k.sum_in = k.sum_out = sum_frames;
        return k;
    };
    // conv_pre and conv_proj stay fp32 in every arithmetic mode (bins -> H from a spectrogram in the hundreds; the statistics feed exp())
    {
        ScopedSet<int> f32(arith_now_, VITS_ARITH_F32);
        HIP_OK(conv("post_conv_pre", post_.pre, mk(spec, hout)));
    }
    static const WaveNetLabels labels{"post_wavenet_layer", "post_wavenet_gated_conv", "post_conv1x1"};
    if (run_wavenet(c, post_.in_layers, post_.res_skip, hp.post_wn_layers, labels)) return -1;
    {
        ScopedSet<int> f32(arith_now_, VITS_ARITH_F32);
        HIP_OK(conv("post_conv_proj", post_.proj, mk(sub(hout, H), stats)));
    }
    if (o.collect_taps) {
        snapshot("post_mean", stats, F, Lmax, B, frames);
        snapshot("post_logstd", sub(stats, F), F, Lmax, B, frames);
    }
    // eps: the [F][L] draw prior sampling would make (engine_flow.cpp run_prior_sampling), then z_q — in the forward flow's physical input layout
    TensorRef zp = TR(s2.zp, F, ls), noise = TR(s2.noise, F, ls);
    // (scale 0 = the posterior mean: no noise drawn, uploaded or read)
    if (o.noise_kind != VITS_NOISE_COUNTER && vc.eps_scale != 0.f && upload_host_noise(c)) return -1;
    const int nk = o.noise_kind == VITS_NOISE_COUNTER ? VITS_NOISE_COUNTER : VITS_NOISE_EXPLICIT;
    prof.begin("posterior_sample", 0, 0, stream, true);
    HIP_OK(launch_posterior_sample(stats, sub(stats, F), ll, noise, nk, o.noise_seed, c.s1.seed_off, zp, B, F, Lmax, hp.n_flows % 2, stream, vc.eps_scale));
    prof.end(stream);
    if (o.collect_taps) {
        // (the logical z_q: with an odd layer count zp holds it reversed)
        if (hp.n_flows % 2) snapshot_flipped("z_q", zp, F, Lmax, B, frames);
        else snapshot("z_q", zp, F, Lmax, B, frames);
    }
    // forward flow, source speaker
    return run_coupling(c, true);
}

}  // namespace vits
