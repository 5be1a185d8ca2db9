// engine_align.cpp — forced alignment (include/vits.h vits_model_align_batch): which frames of a recording belong to which token of its transcript, by
// VITS's own monotonic alignment search (SynthesizerTrn.forward: neg_cent, then maximum_path) between the text encoder's prior statistics per token and
// z_p of the recording. The two halves already exist: run_text_encoder (stage-one slot 0) and the conversion front end run_conversion_front (its arena in
// stage-one slot 1: the prior statistics must survive it); align.hip adds the likelihood matrix and the search. No duration predictor, no reverse flow, no
// vocoder; one D2H copy (durations, scores) and one host wait.
#include "engine_internal.h"

namespace vits {

int Engine::align_batch(const float* pcm, const int64_t* pcm_lens, int B, int64_t pcm_stride, const int32_t* ids, const int32_t* id_lens, int id_stride,
                        const int32_t* speakers, float noise_scale, const vits_process_opts& o, int32_t* durations, int64_t* frames_out, float* scores,
                        std::string& err) {
    std::vector<float> given;
    FitGiven fit_given;
    const bool fit_was_given = take_fit(fit_given);  // (taken with the ratios: whatever becomes of this call, both are gone)
    if (take_pitch_ratios(given)) {
        err = "alignment does not take the ratios of vits_model_set_pitch_ratios (it produces no audio)";
        return -1;
    }
    if (fit_was_given) {
        err = "alignment does not take the fit of vits_model_set_fit (its durations are the recording's, not the predictor's)";
        return -1;
    }
    if (refuse_pending(err)) return -1;
    if (B <= 0 || id_stride <= 0) {
        err = "empty batch";
        return -1;
    }
    if (!pcm || !pcm_lens || pcm_stride <= 0 || !ids || !durations) {
        err = "null PCM, lengths, ids or durations, or pcm_stride <= 0";
        return -1;
    }
    if (const char* what = first_set({{"fixed_duration", o.fixed_duration > 0},
                                      {"frames_only", o.frames_only != 0},
                                      {"async", o.async != 0},
                                      {"out_device", o.out_device != nullptr},
                                      {"skip_host_copy", o.skip_host_copy != 0},
                                      {"vocoder_chunk_frames", o.vocoder_chunk_frames > 0},
                                      {"on_chunk", o.on_chunk != nullptr}})) {
        err = std::string("alignment does not take opts.") + what + " (it produces no audio: the frame counts come from the input PCM and the call is synchronous)";
        return -1;
    }
    if (o.speaker_ids) {
        err = "alignment takes the speaker of the recording from its speakers argument, not from opts.speaker_ids";
        return -1;
    }
    if (const char* what = prosody_opt_set(o)) {
        err = std::string("alignment does not take opts.") + what + " (it has no duration prediction; the scale of the posterior draw is the call's noise_scale)";
        return -1;
    }
    if (!std::isfinite(noise_scale) || noise_scale < 0.f || noise_scale > 10.f) {
        char buf[48];
        std::snprintf(buf, sizeof(buf), "%.9g", (double)noise_scale);
        err = std::string("noise_scale = ") + buf + ": must be finite and in [0, 10]";
        return -1;
    }
    for (int b = 0; b < B; ++b) {
        const int s = speakers ? speakers[b] : -1;
        if (s == -1) continue;
        const std::string who = "speakers[" + std::to_string(b) + "] = " + std::to_string(s) + " (speaker of recording " + std::to_string(b) + ")";
        if (check_speaker(s, who, err)) return -1;
    }
    Call c(o, err, ids, B, id_stride);
    Call::Vc vc;
    c.vc = &vc;
    vc.eps_scale = noise_scale;
    c.md = o.mode == VITS_MODE_DEFAULT ? mode : o.mode;
    c.refmode = c.md == VITS_MODE_REFERENCE;
    c.tlen.resize(B);
    for (int b = 0; b < B; ++b) {
        c.tlen[b] = id_lens ? id_lens[b] : id_stride;
        if (c.tlen[b] <= 0 || c.tlen[b] > id_stride) {
            err = "utterance " + std::to_string(b) + " has " + std::to_string(c.tlen[b]) + " tokens: an alignment needs between 1 and id_stride = " + std::to_string(id_stride);
            return -1;
        }
        c.Tmax = std::max(c.Tmax, c.tlen[b]);
        c.sum_t += c.tlen[b];
        for (int t = 0; t < c.tlen[b]; ++t) {
            const int id = ids[(size_t)b * id_stride + t];
            if (id < 0 || id >= hp.vocab_size) {
                err = "token id out of range";
                return -1;
            }
        }
    }
    if (c.Tmax > 2048) {
        err = "more than 2048 ids per utterance is not supported";
        return -1;
    }
    if (prepare_conversion(err)) return -1;
    int64_t nmax = 0;
    std::vector<int64_t> n_model;  // samples at the model's rate (an input rate resamples the recording: vits_model_set_rates)
    if (check_conversion_pcm(pcm_lens, B, pcm_stride, nmax, n_model, err)) return -1;
    for (int b = 0; b < B; ++b) {
        const int64_t L = n_model[b] / hop_;
        if (c.tlen[b] > L) {  // (L >= 1: at least one hop of samples was checked above)
            err = "utterance " + std::to_string(b) + " has " + std::to_string(c.tlen[b]) + " tokens but only " + std::to_string(L) + " frames (" +
                  std::to_string(n_model[b]) + " samples / hop " + std::to_string(hop_) + "): every token needs at least one frame, no monotonic path exists";
            return -1;
        }
    }
    if (!lat16_ready_ && knobs.lat16_lazy_tokens > 0 && (int64_t)B * c.Tmax <= knobs.lat16_lazy_tokens && ensure_lat16(err)) return -1;
    c.ts = round_up(c.Tmax, 32);
    c.n_up = (int)ups_.size();
    clear_taps();
    tap_batch_ = B;
    const int F = hp.flow_size, H = hp.hidden, Tmax = c.Tmax, ts = c.ts;

    // ---- the text side: the text encoder alone, in stage-one slot 0 (arithmetic as in process_batch) ----------------------------
    arith_now_ = arith_scope == VITS_ARITH_SCOPE_ALL_CONVS ? arith_kernels() : VITS_ARITH_F32;
    a1_slot_ = 0;
    if (layout_stage_one(c)) return -1;
    if (run_text_encoder(c)) return -1;
    const int* d_tlens = c.s1.lens;
    TensorRef prior = make_ref(c.s1.stats, 2 * F, ts);
    arith_now_ = arith_kernels();

    // ---- the audio side: the conversion front end; its own arena goes to stage-one slot 1 (no batch is in flight: the slot is free) -------------------
    ScopedSet<int> slot(a1_slot_, 1);
    if (layout_conversion(c, pcm, pcm_lens, pcm_stride, speakers, nullptr, nmax, n_model)) return -1;
    const int Lmax = c.Lmax, ls = c.ls = round_up(Lmax, 32);
    const int* d_frames = c.s1.frames;
    c.d_len_full[0] = c.s1.stage_lens;
    // stage-two arena: what the posterior encoder and the forward flow use of it, then the alignment's own buffers
    const bool need_noise_buf = o.noise_kind != VITS_NOISE_COUNTER && noise_scale != 0.f;
    const bool bits_in_lds = align_mas_bits_in_lds(Tmax, Lmax);
    const size_t bit_words = bits_in_lds ? 0 : align_mas_bits_words(Tmax, Lmax);
    const size_t x16_elems = arith_now_ != VITS_ARITH_F32 ? (size_t)B * round_up(std::max(H, F), 8) * round_up(ls, 8) + 64 : 0;
    Call::S2& s2 = c.s2;
    AlignCall ac;
    int* d_dur = nullptr;
    auto layout = [&](Arena& a) {
        s2.zp = a.alloc<float>((size_t)B * F * ls);
        s2.noise = need_noise_buf ? a.alloc<float>((size_t)B * F * ls) : nullptr;
        s2.hout = a.alloc<float>((size_t)B * 2 * H * ls);
        s2.gate = a.alloc<float>((size_t)B * H * ls);
        s2.x16[0] = x16_elems ? a.alloc<uint16_t>(x16_elems) : nullptr;
        ac.plane_a = a.alloc<float>((size_t)B * 2 * F * ts);
        ac.plane_z = a.alloc<float>((size_t)B * 2 * F * ls);
        ac.ct = a.alloc<float>((size_t)B * ts);
        ac.logp = a.alloc<float>((size_t)B * ts * ls);
        ac.bits = bit_words ? a.alloc<unsigned long long>((size_t)B * bit_words) : nullptr;
        ac.path = a.alloc<float>((size_t)B * ls);
        // results, one block = one D2H copy: durations [B][id_stride] ints | scores [B] floats
        d_dur = a.alloc<int>((size_t)B * id_stride + B);
    };
    if (arena_layout(a2_, stream, err, layout)) return -1;
    set_x16_scratch(s2.x16[0], nullptr, nullptr, x16_elems);
    if (run_conversion_front(c)) return -1;  // z_p in s2.zp, logical channel order

    // ---- likelihood matrix and search (align.hip), fp32 in every arithmetic mode ----------------------------------------------------------------
    c.rx.phase("vits.align");
    ac.mean = prior;
    ac.logs = sub_rows(prior, F);
    ac.z = make_ref(s2.zp, F, ls);
    ac.tlens = d_tlens;
    ac.frames = d_frames;
    ac.channels = F;
    ac.batch = B;
    ac.tmax = Tmax;
    ac.lmax = Lmax;
    ac.t_stride = ts;
    ac.l_stride = ls;
    ac.dur = d_dur;
    ac.dur_stride = id_stride;
    ac.score = reinterpret_cast<float*>(d_dur + (size_t)B * id_stride);
    double cells = 0;
    for (int b = 0; b < B; ++b) cells += (double)c.tlen[b] * c.frames[b];
    // algorithmic work: the [T x 2F] . [2F x L] product; bytes: statistics and z_p read once, logp written once
    prof.begin("align_logp", 2.0 * 2.0 * F * cells, 4.0 * (2.0 * F * ((double)c.sum_t + (double)c.sum_frames) + cells), stream, true);
    HIP_OK(launch_align_logp(ac, stream));
    prof.end(stream);
    // the search: one add and one max per cell; logp read once, one bit per cell written and (along the path) read, the results
    prof.begin("align_mas", 2.0 * cells, 4.0 * cells + cells / 8.0 + 4.0 * ((double)B * id_stride + (double)c.sum_frames), stream, true);
    HIP_OK(launch_align_mas(ac, stream));
    prof.end(stream);
    if (o.collect_taps) {
        snapshot("align_logp", make_ref(ac.logp, ts, ls), Tmax, Lmax, B, c.frames);
        if (auto it = taps_.find("align_logp"); it != taps_.end()) it->second.chans = c.tlen;
        TensorRef p;
        p.p = ac.path;
        p.cs = ls;
        p.bs = ls;
        snapshot("align_path", p, 1, Lmax, B, c.frames);
    }
    // ---- results: one copy, one wait -------------------------------------------------------------------------------------------------------------
    const size_t n_res = (size_t)B * id_stride + B;
    HIP_OK(align_host_.ensure(n_res, n_res + n_res / 4 + 64));
    HIP_OK(hipMemcpyAsync(align_host_.p, d_dur, sizeof(int) * n_res, hipMemcpyDeviceToHost, stream));
    prof.fence();
    HIP_OK(hipStreamSynchronize(stream));
    prof.fence();
    std::memcpy(durations, align_host_.p, sizeof(int32_t) * (size_t)B * id_stride);
    if (scores) std::memcpy(scores, align_host_.p + (size_t)B * id_stride, sizeof(float) * B);
    if (frames_out)
        for (int b = 0; b < B; ++b) frames_out[b] = c.frames[b];
    return 0;
}

}  // namespace vits
