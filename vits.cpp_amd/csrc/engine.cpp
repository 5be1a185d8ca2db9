// engine.cpp — one call from ids to PCM (see engine.h): input checks, the two arenas, the single host read of the frame counts,
// vocoder windows (window_plan.h) / streaming, results. The phases themselves live in engine_stage1.cpp, engine_flow.cpp and engine_vocoder.cpp, the delivery
// chain behind the vocoder in engine_delivery.cpp.
// Compiled with hipcc as host C++.
#include <cmath>
#include <numeric>

#include "engine_internal.h"

namespace vits {

// ---- convolution wrappers (profiled launches) -------------------------------------------------------------------------------
// One 16-bit-operand convolution launch (conv16.hip), profiled like conv(): tile names carry a capital T
hipError_t Engine::conv16(const char* name, const PackedConv& w, const Conv16Call& c, hipStream_t stream, double bytes) {
    if (prof.on) {
        const Conv16Plan pl = plan_conv16(w, c);  // (the tile that runs; 7: conv16_lat_kernel)
        const bool group = c.yg || c.y16.p;
        char full[160];
        std::snprintf(full, sizeof(full), "%s|k%d|d%d|T%d|e%d%s|c%dx%d", name, w.kt, pl.dil, pl.tile, w.epi, group ? "g" : "", w.cin,
                      w.cout);
        const int64_t tot_in = c.sum_in >= 0 ? c.sum_in : (int64_t)c.batch * c.t_in;
        const int64_t tot_out = c.sum_out >= 0 ? c.sum_out : (int64_t)c.batch * c.t_out;
        const int64_t cols = w.epi == EPI_CONVT ? tot_in : tot_out;
        prof.begin(full, 2.0 * (double)w.rows * (double)w.cin * (double)w.kt * (double)cols, bytes, stream, /*chain=*/true);
    }
    hipError_t e = launch_conv16(w, c, arith_now_, stream);
    prof.end(stream);
    return e;
}

// A conv of the fp32-layout orchestration in a 16-bit arithmetic mode: (1) the input is rounded into the 16-bit group layout,
// with the conv's input leaky_relu fused (the reference's leaky_relu node + fp16 im2col, vits.cpp:554 + custom-ops.h:684-690),
// (2) the 16-bit-operand kernel writes the same fp32 outputs the fp32 kernel would. Used for stage one, the flow, and any
// vocoder whose channel counts rule out the group-layout fast path.
hipError_t Engine::conv16_transparent(const char* name, const PackedConv& w, const ConvCall& c, hipStream_t stream) {
    int si = 0;
    if (stream == side_[0]) si = 1;
    else if (stream == side_[1]) si = 2;
    Ref16 x16 = x16_[si];
    const int groups = (w.cin + 7) / 8;
    x16.ts = round_up(std::max(c.t_in, 1), 8);
    x16.bs = (int64_t)groups * x16.ts * 8;
    if (!x16.p || (size_t)c.batch * (size_t)x16.bs > x16_cap_[si]) return hipErrorOutOfMemory;
    const int64_t tot_in = c.sum_in >= 0 ? c.sum_in : (int64_t)c.batch * c.t_in;
    const int64_t tot_out = c.sum_out >= 0 ? c.sum_out : (int64_t)c.batch * c.t_out;
    prof.begin("to_group16", 0, 6.0 * (double)w.cin * (double)tot_in, stream, true);
    hipError_t e = launch_to_group16(c.x, c.len_in, c.batch, w.cin, c.t_in, c.pre_act ? c.slope : 1.0f, x16, arith_now_, stream);
    prof.end(stream);
    if (e != hipSuccess) return e;
    Conv16Call k;
    k.x = x16;
    k.len_in = c.len_in;
    k.spk = c.spk;
    k.len_out = c.len_out;
    k.batch = c.batch;
    k.t_in = c.t_in;
    k.t_out = c.t_out;
    k.dil = c.dil;
    k.pad_l = c.pad_l;
    k.post_act = c.post_act;
    k.post_slope = c.post_slope;
    k.scale = c.scale;
    k.scale_div = c.scale_div;
    k.ct_crop = c.ct_crop;
    k.y = c.y;
    k.res = c.res;
    k.acc = c.acc;
    k.y2 = c.y2;
    k.sum_in = c.sum_in;
    k.sum_out = c.sum_out;
    const int cout_stored = w.epi == EPI_GATE ? w.cout / 2 : w.cout;
    const double bytes = 2.0 * (double)w.cin * tot_in + 4.0 * (double)cout_stored * tot_out * (1 + (c.res.p ? 1 : 0) + (c.acc.p ? 1 : 0) + (c.y2 ? 1 : 0)) + (double)w.bytes16;
    return conv16(name, w, k, stream, bytes);
}

hipError_t Engine::conv(const char* name, const PackedConv& w, ConvCall c, hipStream_t on) {
    hipStream_t stream = on ? on : this->stream;
    if (c.xs3.p) {
        // VITS_ARITH_F32_SPLIT: a conv whose input exists as split planes (the wide stages' resblocks, engine_vocoder.cpp) runs on conv_split.hip
        if (prof.on) {
            char full[160];
            std::snprintf(full, sizeof(full), "%s|k%d|d%d|S128|e0|c%dx%d", name, w.kt, c.dil, w.cin, w.cout);
            const int64_t tot = c.sum_out >= 0 ? c.sum_out : (int64_t)c.batch * c.t_out;
            const double bytes = (double)tot * (6.0 * w.cin + (double)w.cout * (4.0 * ((c.y.p ? 1 : 0) + (c.res.p ? 1 : 0) + (c.acc.p ? 1 : 0)) + (c.ys3.p ? 6.0 : 0.0))) + (double)w.bytes_s;
            prof.begin(full, conv_flops(w, c, tot), bytes, stream, /*chain=*/true);
        }
        hipError_t e = launch_conv_split(w, c, stream);
        prof.end(stream);
        return e;
    }
    if (arith_now_ != VITS_ARITH_F32 && w.wp16) return conv16_transparent(name, w, c, stream);
    if (prof.on) {
        // name = label|k<taps>|d<dilation>|t<tile>|e<epilogue>|c<cin>x<cout>: one entry per kernel instantiation and shape, so the
        // bench can line entries up with rocprofv3's per-kernel-name statistics
        const ConvPlan pl = plan_conv(w, c);
        char full[160];
        std::snprintf(full, sizeof(full), "%s|k%d|d%d|t%d|e%d|c%dx%d", name, w.kt, pl.dil, pl.tile, w.epi, w.cin,
                      w.cout);
        // algorithmic work over the REAL lengths (sum over utterances), not the padded grid extent
        const int64_t tot_in = c.sum_in >= 0 ? c.sum_in : (int64_t)c.batch * c.t_in;
        const int64_t tot_out = c.sum_out >= 0 ? c.sum_out : (int64_t)c.batch * c.t_out;
        const int64_t cols = w.epi == EPI_CONVT ? tot_in : tot_out;
        // algorithmic bytes: input read once, output (and its activated copy, if any) written once, residual/accumulator read once, weights once
        const int cout_stored = w.epi == EPI_GATE ? w.cout / 2 : w.cout;
        double bytes = 4.0 * ((double)w.cin * tot_in + (double)cout_stored * tot_out * (1 + (c.res.p ? 1 : 0) + (c.acc.p ? 1 : 0) + (c.y2 ? 1 : 0))) + (double)w.bytes;
        prof.begin(full, conv_flops(w, c, cols), bytes, stream, /*chain=*/true);
    }
    hipError_t e = launch_conv(w, c, stream);
    prof.end(stream);
    return e;
}

int Engine::sync(std::string& err) {
    if (front_) HIP_OK(hipStreamSynchronize(front_));
    HIP_OK(hipStreamSynchronize(stream));
    // (the rows of an async call have landed now)
    lv_.settle(), lm_.settle(), ed_.settle();
    async_tail_ = false;
    return 0;
}

int Engine::check_speaker(int s, const std::string& who, std::string& err, const char* outside) const {
    if (s == -1) return 0;
    if (hp.num_speakers <= 1) {
        err = who + ": this model has a single speaker and no speaker conditioning (use -1)";
        return -1;
    }
    if (!speaker_in_range(s)) {
        err = who + outside + std::to_string(speaker_limit()) + ")";
        return -1;
    }
    return 0;
}

int Engine::check_speakers(const vits_process_opts& o, int B, std::string& err) const {
    for (int b = 0; b < B; ++b) {
        const int s = speaker_of(o, b);
        if (s == -1) continue;
        const std::string who = (o.speaker_ids ? "speaker_ids[" + std::to_string(b) + "] = " : "the model's default speaker (utterance " + std::to_string(b) + ") = ") +
                                std::to_string(s);
        if (check_speaker(s, who, err)) return -1;
        if (ggml_tables == 1) {
            err = who + ": vits_model_set_ggml_tables(model, 1) runs stage one in the CPU oracle's exact order, which has no speaker conditioning (use -1, or tables mode 0 / 2)";
            return -1;
        }
    }
    return 0;
}

int Engine::set_prosody(float rate, float ns, float nsd, std::string& err) {
    if (!rate_ok(rate) || !noise_scale_ok(ns) || !noise_scale_ok(nsd)) {
        err = "vits_model_set_prosody(" + fmt_float(rate) + ", " + fmt_float(ns) + ", " + fmt_float(nsd) + "): " +
              (!rate_ok(rate) ? "speaking_rate must be finite and in [0.1, 10]" : "noise scales must be finite and in [0, 10]");
        return -1;
    }
    speaking_rate = rate, noise_scale = ns, noise_scale_dur = nsd;
    return 0;
}

// ---- a stated duration (include/vits.h): what is given for the next call, and what a call makes of it ---------------------------------------------
int Engine::set_fit(const int64_t* targets, const int32_t* groups, int n, float min_rate, float max_rate, std::string& err) {
    if (n < 0 || (!targets && n > 0)) {
        err = "vits_model_set_fit: " + std::string(n < 0 ? "n < 0" : "null argument (target_frames is NULL with n > 0)");
        return -1;
    }
    FitGiven g;
    if (targets && n > 0) {
        g.set = true;
        g.targets.assign(targets, targets + n);
        g.has_groups = groups != nullptr;
        if (groups) g.groups.assign(groups, groups + n);
        g.min_rate = min_rate, g.max_rate = max_rate;
    }
    fit_given_.give(std::move(g));
    return 0;
}

int Engine::set_fit_total(int64_t total, float min_rate, float max_rate, std::string& err) {
    (void)err;
    FitGiven g;
    g.set = g.total = true;
    g.targets.assign(1, total);
    g.min_rate = min_rate, g.max_rate = max_rate;
    fit_given_.give(std::move(g));
    return 0;
}

int Engine::resolve_fit(int B, const vits_process_opts& o, const float* pitch, ResolvedFit& rf, std::string& err) const {
    if (!rf.have) return 0;
    const FitGiven& g = rf.given;
    const std::string who = g.total ? "vits_model_set_fit_total: " : "vits_model_set_fit: ";
    if (B <= 0) return 0;  // (the call's own refusal follows)
    if (!g.total && (int)g.targets.size() != B) {
        err = who + "n = " + std::to_string(g.targets.size()) + " was given, and this call has " + std::to_string(B) + " utterances";
        return -1;
    }
    rf.group.assign((size_t)B, 0);
    rf.target.assign((size_t)B, 0);
    if (g.total) {
        rf.target[0] = g.targets[0];
        if (g.targets[0] < 1 || g.targets[0] > kFitMaxTarget) {
            err = who + "total_frames = " + std::to_string(g.targets[0]) + ": a target is 1 to 2^22 frames";
            return -1;
        }
    } else {
        for (int b = 0; b < B; ++b) rf.group[(size_t)b] = g.has_groups ? g.groups[(size_t)b] : b;
        rf.target = g.targets;
    }
    std::string why;
    if (!fit_check(B, rf.group.data(), rf.target.data(), why) || !fit_limits(g.min_rate, g.max_rate, rf.s_lo, rf.s_hi, why)) {
        err = who + why;
        return -1;
    }
    int fitted = -1;  // (the first utterance of a fitted group)
    for (int b = B - 1; b >= 0; --b)
        if (rf.target[(size_t)rf.group[(size_t)b]] != 0) fitted = b;
    if (fitted < 0) return 0;  // (every target 0: the call runs as always)
    const std::string what = who + "group " + std::to_string(rf.group[(size_t)fitted]) + " is fitted to " + std::to_string(rf.target[(size_t)rf.group[(size_t)fitted]]) + " frames: ";
    if (o.fixed_duration > 0) {
        err = what + "fixed_duration > 0 leaves the duration predictor nothing to scale";
        return -1;
    }
    if (ggml_tables == 1) {
        err = what + "vits_model_set_ggml_tables(model, 1) runs stage one in the CPU oracle's exact order, whose duration is not expf(logw) x scale (use tables mode 0 or 2)";
        return -1;
    }
    if (o.async) {
        err = what + "async returns before the device has finished, and the fit's rows are read from the device behind stage one: call without async, or pipeline "
                     "with vits_model_submit_batch / vits_model_wait";
        return -1;
    }
    for (int b = 0; pitch && b < B; ++b)
        if (pitch[b] != 1.f && rf.target[(size_t)rf.group[(size_t)b]] != 0) {
            err = who + "utterance " + std::to_string(b) + " of the fitted group " + std::to_string(rf.group[(size_t)b]) + " has the pitch ratio " + fmt_float(pitch[b]) +
                  ": the varispeed's stretch and the fit both own the length scale (the combination is not built)";
            return -1;
        }
    rf.on = true;
    return 0;
}

int64_t Engine::fit_frames(double seconds) const {
    if (!std::isfinite(seconds)) return -1;
    int64_t hop = 1, sadd = 0;
    const bool refmode = mode == VITS_MODE_REFERENCE;
    for (const auto& u : ups_) {  // (set_stage_affine's recurrence)
        const int s = u.stride, K = u.k;
        const int crop = refmode ? 0 : (K - s) / 2;
        hop *= s;
        sadd = sadd * s + (K - s - 2 * crop);
    }
    const double samples = std::floor(seconds * (double)hp.sampling_rate);
    if (!(samples < 9.0e15)) return (int64_t)kFitMaxTarget;
    const int64_t L = ((int64_t)samples - sadd) / hop;
    return std::min<int64_t>(std::max<int64_t>(samples < (double)sadd ? 1 : L, 1), kFitMaxTarget);
}

// the group rows [B][kFitRowInts] of a call that fits, queued for the host beside the frame counts; fit_report turns the landed copy into the rows of
// vits_model_last_fit, one per utterance
hipError_t Engine::copy_fit_rows(const Call& c, PinnedBuf<int64_t>& pinned) {
    const size_t n = (size_t)c.B * kFitRowInts;
    if (hipError_t e = pinned.ensure(n, n + 64)) return e;
    return hipMemcpyAsync(pinned.p, c.s1.fit_rows, sizeof(int64_t) * n, hipMemcpyDeviceToHost, stream);
}
std::vector<double> Engine::fit_report(const Call& c, const int64_t* pinned) const {
    std::vector<double> by_group((size_t)c.B * kFitRowInts), rows((size_t)c.B * 6);
    fit_rows_double(c.B, pinned, by_group.data());
    for (int b = 0; b < c.B; ++b) {
        const int g = c.fit->group[(size_t)b];
        rows[(size_t)6 * b] = g;
        std::copy_n(by_group.begin() + (size_t)kFitRowInts * g, kFitRowInts, rows.begin() + (size_t)6 * b + 1);
    }
    return rows;
}

void Engine::batch_landed(Pending& p, int slot, bool append) {
    lv_.landed(slot, p.lv_rows, append);
    lm_.landed(slot, p.lm_rows, append);
    if (p.ed_rows) edges_lengths(ed_.slot_rows(slot), p.ed_rows, p.lengths.data());
    ed_.landed(slot, p.ed_rows, append);
    pt_.store(p.pt_rows, append);
    if (!append) fit_rows_.clear();
    fit_rows_.insert(fit_rows_.end(), p.fit_rows.begin(), p.fit_rows.end());
}

// the one place that allocates what a call hands out: lengths[] and frames[] of B utterances, no PCM yet
template <class LenIt, class FrameIt>
static void fill_result(vits_batch_result* out, int B, size_t stride, LenIt lengths, FrameIt frames) {
    out->batch = (size_t)B;
    out->stride = stride;
    out->lengths = new int64_t[B];
    out->frames = new int64_t[B];
    out->data = nullptr;
    std::copy_n(lengths, B, out->lengths);
    std::copy_n(frames, B, out->frames);
}

int Engine::check_prosody(const vits_process_opts& o, int B, int id_stride, const int32_t* id_lens, std::string& err) const {
    if (o.fixed_duration > 0 && (o.speaking_rates || o.duration_override)) {
        err = std::string(o.speaking_rates ? "speaking_rates" : "duration_override") + " cannot be combined with fixed_duration > 0 (every token already lasts fixed_duration frames)";
        return -1;
    }
    for (int b = 0; b < B; ++b) {
        if (o.speaking_rates && !rate_ok(o.speaking_rates[b])) {
            err = "speaking_rates[" + std::to_string(b) + "] = " + fmt_float(o.speaking_rates[b]) + ": must be finite and in [0.1, 10]";
            return -1;
        }
        for (const auto& [arr, name] : {std::make_pair(o.noise_scales, "noise_scales"), std::make_pair(o.noise_scale_durations, "noise_scale_durations")})
            if (arr && !noise_scale_ok(arr[b])) {
                err = std::string(name) + "[" + std::to_string(b) + "] = " + fmt_float(arr[b]) + ": must be finite and in [0, 10]";
                return -1;
            }
        if (o.duration_override) {
            const int len = std::min(id_stride, std::max(0, id_lens ? id_lens[b] : id_stride));  // (entries past the utterance are never read)
            for (int t = 0; t < len; ++t) {
                const int32_t v = o.duration_override[(size_t)b * id_stride + t];
                if (v < -1 || v > 10000) {
                    err = "duration_override[" + std::to_string(b) + "][" + std::to_string(t) + "] = " + std::to_string(v) +
                          " (utterance " + std::to_string(b) + ", token " + std::to_string(t) + "): must be -1 (the prediction) or in [0, 10000]";
                    return -1;
                }
            }
        }
    }
    return 0;
}

int Engine::process_batch(const int32_t* ids, const int32_t* id_lens, int B, int id_stride, const vits_process_opts& o, vits_batch_result* out,
                          std::string& err) {
    ResolvedPitch rp(*this, o);
    ResolvedFit rf(*this);
    if (refuse_pending(err)) return -1;
    if (check_speakers(o, B, err)) return -1;
    if (check_prosody(o, B, id_stride, id_lens, err)) return -1;
    if (resolve_pitch(B, id_stride, id_lens, rp, err)) return -1;
    if (resolve_fit(B, o, rp.pitch, rf, err)) return -1;
    ScopedSet<const float*> pitch_scope(call_pitch_, rp.pitch);
    ScopedSet<const ResolvedFit*> fit_scope(call_fit_, rf.on ? &rf : nullptr);
    DeliveryPlan refusable;  // (the refusals of the delivery chain, before stage one is queued; the call's own plan is made where its stage two begins)
    if (plan_delivery(rp.o, refusable, err)) return -1;
    clear_reports();
    // The drop-in callers' share of the pipeline: a large batch is split in two inside the call — stage one of the
    // second part runs on the front-end stream under the flow / vocoder of the first, exactly as two vits_model_submit_batch calls would.
    // Every kernel is batch-invariant, so PCM, lengths and frames are those of the unsplit call bit for bit (GPU test, fuzz_identity.py).
    const int smin = knobs.split_min_batch;
    // (a call that shifts stays whole: a part whose ratios are all 1 would run without the stage and leave the report without its rows; so does a call that
    // fits: a group stays in one launch)
    if (smin > 0 && B >= smin && B >= 2 && front_ && !prof.on && !knobs.no_pipeline && o.noise_kind == VITS_NOISE_COUNTER && !o.collect_taps && !o.on_chunk &&
        !o.frames_only && !o.async && o.vocoder_chunk_frames <= 0 && !rp.pitch && !rf.on)
        return process_split(ids, id_lens, B, id_stride, o, out, err);
    a1_slot_ = 0;
    const int rc = process_impl(ids, id_lens, B, id_stride, rp.o, out, err, nullptr);
    if (rc) drain_streams();
    return rc;
}

void Engine::drain_streams() {
    // A call that fails behind its first launch returns with work queued (with fixed_duration > 0 there is no frame-count synchronise in front of stage two's
    // refusals). Nothing orders the front-end stream of a later vits_model_submit_batch behind the main stream but the event of an async call, which a failed
    // call does not record: left queued, that stage one and the next submit's would write stage-one arena 0 side by side.
    if (front_) hipStreamSynchronize(front_);
    hipStreamSynchronize(stream);
}

int Engine::process_joined(const int32_t* ids, const int32_t* id_lens, int B, int id_stride, const vits_process_opts& o, const int32_t* track, const float* gap_ms,
                           const int32_t* index, vits_batch_result* out, std::string& err) {
    const std::string who = "vits_model_process_joined: ";
    ResolvedPitch rp(*this, o);
    ResolvedFit rf(*this);
    if (refuse_pending(err)) return -1;
    // (on_chunk and async are the plan's refusals, below)
    if (o.collect_taps) {
        err = who + "opts.collect_taps is not taken: the taps of the stages in front of the join are per utterance and those behind it per track (run "
                    "vits_model_process_batch for the former, the vits_op_* entry points for the latter)";
        return -1;
    }
    if (o.noise_kind != VITS_NOISE_COUNTER && o.noise_kind != VITS_NOISE_EXPLICIT) {
        err = who + "noise_kind " + std::to_string(o.noise_kind) + " is not taken: VITS_NOISE_COUNTER or VITS_NOISE_EXPLICIT (the reference's own stream is that of "
                    "vits_model_process, one utterance at a time)";
        return -1;
    }
    if (B <= 0 || id_stride <= 0) {
        err = who + "empty batch";
        return -1;
    }
    if (rp.have || pitch_ratio != 1.f) {
        // (the ratios are validated here, in front of the plan's refusals, which ask whether the stage runs; the rates they divide, below, where they always were)
        if (check_prosody(o, B, id_stride, id_lens, err)) return -1;
        if (resolve_pitch(B, id_stride, id_lens, rp, err)) {
            err = who + err;
            return -1;
        }
    }
    if (resolve_fit(B, o, rp.pitch, rf, err)) {
        err = who + err;
        return -1;
    }
    ScopedSet<const float*> pitch_scope(call_pitch_, rp.pitch);
    ScopedSet<const ResolvedFit*> fit_scope(call_fit_, rf.on ? &rf : nullptr);
    DeliveryPlan refusable;
    if (plan_delivery(rp.o, refusable, err, /*joined=*/true)) return -1;
    JoinPlan plan;
    std::string why;
    if (!join_plan(hp.sampling_rate, B, track, gap_ms, plan, why)) {
        err = who + why;
        return -1;
    }
    if (check_speakers(o, B, err)) return -1;
    if (check_prosody(o, B, id_stride, id_lens, err)) return -1;
    clear_reports();
    a1_slot_ = 0;
    join_index_.assign(B, 0);
    for (int b = 0; b < B; ++b) join_index_[b] = index ? index[b] : b;
    const int rc = process_impl(ids, id_lens, B, id_stride, rp.o, out, err, nullptr, &plan);
    if (rc) drain_streams();
    return rc;
}

int Engine::process_split(const int32_t* ids, const int32_t* id_lens, int B, int id_stride, const vits_process_opts& o, vits_batch_result* out,
                          std::string& err) {
    // first part: knobs.split_first_pct per cent of the utterances (its stage one is the only exposed one)
    const int B1 = std::min(B - 1, std::max(1, (int)(((int64_t)B * knobs.split_first_pct + 50) / 100)));
    const int nb[2] = {B1, B - B1}, b0[2] = {0, B1};
    std::vector<int32_t> offs(B);
    for (int b = 0; b < B; ++b) offs[b] = o.noise_seed_offsets ? o.noise_seed_offsets[b] : b;  // (a part keeps its utterances' global noise streams)
    int queued = 0;
    for (int h = 0; h < 2; ++h) {
        vits_process_opts oh = o;
        oh.noise_seed_offsets = offs.data() + b0[h];
        if (o.speaker_ids) oh.speaker_ids = o.speaker_ids + b0[h];
        if (o.speaking_rates) oh.speaking_rates = o.speaking_rates + b0[h];
        if (o.noise_scales) oh.noise_scales = o.noise_scales + b0[h];
        if (o.noise_scale_durations) oh.noise_scale_durations = o.noise_scale_durations + b0[h];
        if (o.duration_override) oh.duration_override = o.duration_override + (size_t)b0[h] * id_stride;
        if (o.durations_out) oh.durations_out = o.durations_out + (size_t)b0[h] * id_stride;
        if (o.out_device) oh.out_device = (float*)o.out_device + (int64_t)b0[h] * o.out_device_stride;
        if (submit_batch(ids + (size_t)b0[h] * id_stride, id_lens ? id_lens + b0[h] : nullptr, nb[h], id_stride, oh, err, /*part=*/true)) break;
        ++queued;
    }
    if (queued < 2) {
        std::string ignored;
        while (pending()) wait_batch(nullptr, ignored);
        return -1;
    }
    // hand over: the parts' results side by side, rows at the stride of the longer part
    Pending* part[2] = {&pend_[wait_seq_ & 1], &pend_[(wait_seq_ + 1) & 1]};
    int rc = 0;
    for (int h = 0; h < 2 && !rc; ++h)
        if (hipEventSynchronize(part[h]->done) != hipSuccess) {
            err = "hipEventSynchronize failed";
            rc = -1;
        }
    // (the two slots are released whatever happens below: an allocation failure must not leave the handle with batches in flight)
    struct Release {
        Engine& e;
        Pending** part;
        ~Release() {
            for (int h = 0; h < 2; ++h) {
                part[h]->active = false;
                ++e.wait_seq_;
            }
        }
    } release{*this, part};
    // the parts' rows side by side (part h lives in pipeline slot (wait_seq_ + h) & 1); the trimmed lengths of a part are known now that its rows have landed
    for (int h = 0; h < 2 && !rc; ++h) batch_landed(*part[h], (int)((wait_seq_ + h) & 1), /*append=*/h > 0);
    if (!rc && out) {
        const size_t stride = std::max(part[0]->stride, part[1]->stride);
        std::vector<int64_t> lengths(part[0]->lengths), frames(part[0]->frames);
        lengths.insert(lengths.end(), part[1]->lengths.begin(), part[1]->lengths.end());
        frames.insert(frames.end(), part[1]->frames.begin(), part[1]->frames.end());
        fill_result(out, B, stride, lengths.begin(), frames.begin());
        if (!o.skip_host_copy) out->data = new float[(size_t)B * stride];
        for (int h = 0; h < 2; ++h) {
            const Pending& p = *part[h];
            if (out->data)
                for (int b = 0; b < nb[h]; ++b) {
                    float* dst = out->data + (size_t)(b0[h] + b) * stride;
                    std::memcpy(dst, (const float*)p.host.p + (size_t)b * p.stride, sizeof(float) * p.stride);
                    // (columns past a row's own length are unspecified in the unsplit result too; keep them defined)
                    if (p.stride < stride) std::memset(dst + p.stride, 0, sizeof(float) * (stride - p.stride));
                }
        }
    }
    return rc;
}

// ---- pipelined batches (vits.h: vits_model_submit_batch / vits_model_wait) --------------------------------------------------
// submit(n): stage one of batch n on the front-end stream into stage-one arena n & 1 — beside the flow / vocoder of batch n - 1,
// which is running on the main stream —, the frame counts through pinned memory behind an event (the host waits for THAT event,
// not for the device), stage two behind batch n - 1 on the main stream. Batch n - 2, the previous user of the arena, was waited
// for before this submit was accepted, so nothing on the device still reads it.
int Engine::submit_batch(const int32_t* ids, const int32_t* id_lens, int B, int id_stride, const vits_process_opts& o, std::string& err, bool part) {
    ResolvedPitch rp(*this, o);  // (its arrays live until process_impl has returned: the ratios have gone to the slot's pinned memory by then, the rates into the header)
    ResolvedFit rf(*this);       // (likewise: its groups and targets have gone into the header)
    if (pending() >= 2) {
        err = "two batches in flight already: call vits_model_wait first";
        return -1;
    }
    if (o.noise_kind != VITS_NOISE_COUNTER || o.collect_taps || o.on_chunk || o.frames_only || o.async) {
        err = "vits_model_submit_batch: VITS_NOISE_COUNTER only, and no collect_taps / on_chunk / frames_only / async";
        return -1;
    }
    if (check_speakers(o, B, err)) return -1;  // (the speakers are copied into the call's header below: the caller's array may go at once)
    if (check_prosody(o, B, id_stride, id_lens, err)) return -1;  // (so are the prosody arrays; durations_out is written when the frame counts are read)
    if (!part && resolve_pitch(B, id_stride, id_lens, rp, err)) return -1;
    if (!part && resolve_fit(B, o, rp.pitch, rf, err)) return -1;
    ScopedSet<const float*> pitch_scope(call_pitch_, rp.pitch);
    ScopedSet<const ResolvedFit*> fit_scope(call_fit_, rf.on ? &rf : nullptr);
    Pending& p = pend_[submit_seq_ & 1];
    if (!p.done) {
        HIP_OK(hipEventCreateWithFlags(&p.s1_done, hipEventDisableTiming));
        HIP_OK(hipEventCreateWithFlags(&p.done, hipEventDisableTiming));
    }
    a1_slot_ = (int)(submit_seq_ & 1);
    const int rc = process_impl(ids, id_lens, B, id_stride, rp.o, nullptr, err, &p);
    a1_slot_ = 0;
    if (rc) {
        // (whatever was queued is harmless: it only touches this slot's arenas; leave the device idle before the slot is reused)
        if (front_) hipStreamSynchronize(front_);
        hipStreamSynchronize(stream);
        return rc;
    }
    p.active = true;
    ++submit_seq_;
    return 0;
}

int Engine::wait_batch(vits_batch_result* out, std::string& err) {
    if (!pending()) {
        err = "vits_model_wait: nothing was submitted";
        return -1;
    }
    Pending& p = pend_[wait_seq_ & 1];
    HIP_OK(hipEventSynchronize(p.done));
    // the reports of the batch that has just completed, on the host now that `done` has passed (copied: the slot's pinned rows are the next submit's); stated
    // edges: the batch's lengths are its trimmed ones
    batch_landed(p, (int)(wait_seq_ & 1));
    if (out) {
        // (the slot is released only once the result has been handed over: an allocation failure below leaves the batch waitable)
        fill_result(out, p.B, p.stride, p.lengths.begin(), p.frames.begin());
        if (p.host_copy) {
            out->data = new float[(size_t)p.B * p.stride];
            std::memcpy(out->data, p.host.p, sizeof(float) * (size_t)p.B * p.stride);
        }
    }
    p.active = false;
    ++wait_seq_;
    return 0;
}

// opts.durations_out: the durations of stage one (dur [B][id_stride], integer-valued floats, 0 past each utterance) queued for the host beside the
// frame counts, into grow-only pinned memory; store_durations converts them once that copy has landed
hipError_t Engine::copy_durations(const Call& c, PinnedBuf<float>& pinned) {
    const size_t n = (size_t)c.B * c.id_stride;
    if (hipError_t e = pinned.ensure(n, n + n / 4 + 64)) return e;
    return hipMemcpyAsync(pinned.p, c.s1.dur, sizeof(float) * n, hipMemcpyDeviceToHost, stream);
}
void Engine::store_durations(const Call& c, const float* pinned) const {
    const size_t n = (size_t)c.B * c.id_stride;
    for (size_t i = 0; i < n; ++i) c.o.durations_out[i] = (int32_t)pinned[i];
}

// the dispatcher query (opts.frames_only): predicted frames / samples per utterance — or, a joined call, per track — and no audio (buffer sizing, shard balancing by frames)
int Engine::frames_only_result(Call& c, vits_batch_result* out) {
    std::string& err = c.err;
    const int B = c.B;
    const JoinPlan* join = c.join;
    const std::vector<int>& frames = c.frames;
    if (out && join) {
        // per track: the bound a full call stays within, at the rate it would deliver at, and the frames of the track's utterances
        if (plan_rows(c)) return -1;
        const Call::RowSet& pcm = c.behind[STAGE_RESAMPLE];
        fill_result(out, join->tracks, (size_t)pcm.max, pcm.len.begin(), c.track_frames().begin());
    } else if (out) {
        // (samples at the rate the full call would deliver them at; no table is needed for that, and none is uploaded)
        ResamplePlan plan;
        if (output_rate_ && !resample_plan(hp.sampling_rate, output_rate_, plan, err)) return -1;
        // (stated edges: the bound N + Pl + Pt of every utterance, the size to allocate: exact under VITS_EDGES_PAD, an upper bound when the stage trims)
        const int64_t pads = edges_on() ? edges_plan_.Pl + edges_plan_.Pt : 0;
        std::vector<int64_t> lengths(B);
        // (a stated pitch: N' of every utterance in place of the vocoder's sample count)
        if (c.pitched() && plan_rows(c)) return -1;
        const std::vector<int>& len = c.pitched() ? c.behind[STAGE_PITCH].len : c.slen[c.n_up];
        const int longest = c.pitched() ? c.behind[STAGE_PITCH].max : c.smax[c.n_up];
        for (int b = 0; b < B; ++b) lengths[b] = plan.out_len(len[(size_t)b] + pads);
        fill_result(out, B, (size_t)plan.out_len(longest + pads), lengths.begin(), frames.begin());
    }
    HIP_OK(hipStreamSynchronize(stream));
    prof.fence();
    fit_rows_ = c.fit_report;
    return 0;
}

int Engine::process_impl(const int32_t* ids, const int32_t* id_lens, int B, int id_stride, const vits_process_opts& o, vits_batch_result* out,
                         std::string& err, Pending* pend, JoinPlan* join) {
    if (B <= 0 || id_stride <= 0) {
        err = "empty batch";
        return -1;
    }
    if (o.on_chunk && o.skip_host_copy) {  // (the only misuse of the sink; checked before any work is queued)
        err = "on_chunk needs a host copy (skip_host_copy = 0)";
        return -1;
    }
    Call c(o, err, ids, B, id_stride);
    c.join = join;
    c.pitch = call_pitch_;
    c.fit = call_fit_;
    // An error path between the speculative draw and its commit must not leave the reference stream locked — nor at a timing-dependent
    // position: finish(0) rewinds to the state behind the [T, 2] tensor, where the sequential path this replaces leaves the stream when a call
    // fails before prior sampling (finish(drawn()) committed however many values the helper happened to have drawn).
    struct AheadGuard {
        RefNoiseAhead& a;
        ~AheadGuard() {
            if (a.active()) a.finish(0);
        }
    } ahead_guard{ref_ahead_};
    c.md = o.mode == VITS_MODE_DEFAULT ? mode : o.mode;
    c.refmode = c.md == VITS_MODE_REFERENCE;
    c.tlen.resize(B);
    for (int b = 0; b < B; ++b) {
        c.tlen[b] = id_lens ? id_lens[b] : id_stride;
        if (c.tlen[b] <= 0 || c.tlen[b] > id_stride) {
            err = "bad id length";
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
    if (!lat16_ready_ && knobs.lat16_lazy_tokens > 0 && (int64_t)B * c.Tmax <= knobs.lat16_lazy_tokens && ensure_lat16(err)) return -1;
    if (c.Tmax > 2048) {
        err = "more than 2048 ids per utterance is not supported";
        return -1;
    }
    const bool want_async = o.async && o.skip_host_copy && o.fixed_duration > 0 && !o.collect_taps;
    c.ts = round_up(c.Tmax, 32);
    c.n_up = (int)ups_.size();
    clear_taps();
    tap_batch_ = B;

    // ---- stage one: text encoder + duration predictor -------------------------------------------------------
    // Under VITS_ARITH_SCOPE_FLOW_VOCODER (default) stage one is exact fp32 in every arithmetic mode: the durations — the path's
    // only integer output, ceil() of a float (vits.cpp:996-1001) — are then bit-identical to the fp32 path's.
    arith_now_ = arith_scope == VITS_ARITH_SCOPE_ALL_CONVS ? arith_kernels() : VITS_ARITH_F32;
    // pipelined batch: stage one goes to the front-end stream (the per-kernel profiler needs kernels that do not overlap: then,
    // and under VITS_NO_PIPELINE, everything stays on the main stream and a pipelined batch is merely a deferred result)
    const bool overlap = pend && front_ && !prof.on;
    // (the stream member of the engine is "the stream being queued on": stage one of a pipelined batch swaps the front-end stream in)
    ScopedSet<hipStream_t> s1_stream(stream, overlap ? front_ : stream);
    hipStream_t const main_stream = s1_stream.saved;
    if (overlap && async_tail_) {
        // an earlier opts.async call returned without synchronising: its flow / vocoder may still be reading stage-one arena 0 on the
        // main stream, and nothing else orders the front-end stream behind it: stage one of this batch waits for that tail
        if (!ev_async_) HIP_OK(hipEventCreateWithFlags(&ev_async_, hipEventDisableTiming));
        HIP_OK(hipEventRecord(ev_async_, main_stream));
        HIP_OK(hipStreamWaitEvent(front_, ev_async_, 0));
    }
    // (before the reference stream is touched: a refused call leaves it alone)
    if (ggml_tables == 1 && !hp.stochastic_duration) {
        err = "vits_model_set_ggml_tables(model, 1) runs stage one in the CPU oracle's exact order, and this model has a deterministic duration predictor, which the oracle "
              "(like the reference) does not have (use tables mode 0 or 2)";
        return -1;
    }
    if (B == 1 && o.noise_kind == VITS_NOISE_REFERENCE && !o.frames_only && knobs.ref_ahead_frames_per_id > 0) {
        // The reference's own call (vits_model_process: one utterance, libstdc++ noise). Its two noise tensors are drawn on the host: [T, 2] at
        // vits.cpp:948 and [L, 192] at :1059 — ~1.25 ms for 128 ids, and L is known only behind stage one. A helper thread draws the stream from NOW on,
        // while this thread queues stage one and the device runs it (RefNoiseAhead, engine_support.cpp); run_prior_sampling names the size.
        // (sized by the utterance's length scale: a slowed-down utterance needs proportionally more frames per id)
        const double ls = o.speaking_rates ? 1.0 / (double)o.speaking_rates[0] : 1.0 / (double)speaking_rate;
        const size_t per_id = (size_t)std::ceil(knobs.ref_ahead_frames_per_id * std::max(1.0, ls));
        const size_t want = (size_t)hp.flow_size * (per_id * c.Tmax + 64);
        HIP_OK(ref_noise_pinned_.ensure(want, want));
        // (the deterministic duration predictor draws nothing: the stream goes straight to the prior tensor)
        ref_ahead_.start(hp.stochastic_duration ? (size_t)2 * c.tlen[0] : 0, ref_noise_pinned_.p, ref_noise_pinned_.cap);
        c.ref_ahead = &ref_ahead_;
    }
    std::vector<int>& frames = c.frames;
    if (o.fixed_duration > 0) {
        // every frame count is host arithmetic: so is every bound behind it, and what they refuse is refused here, before anything is queued
        set_stage_affine(c);
        frames.resize(B);
        for (int b = 0; b < B; ++b) frames[b] = std::max(1, o.fixed_duration * c.tlen[b]);
        c.frames_known();
        if (plan_rows(c)) return -1;
    }
    if (layout_stage_one(c)) return -1;
    if (ggml_tables == 1) {
        // emulated-ggml mode: stage one in the exact order shared with the oracle (engine_stage1_exact.cpp)
        if (run_stage_one_exact(c)) return -1;
    } else {
        if (run_text_encoder(c)) return -1;
        if (run_duration_predictor(c)) return -1;
    }
    arith_now_ = arith_kernels();

    // ---- the one data-dependent shape (vits.cpp:1133): frames per utterance ---------------------------------
    c.rx.phase("vits.frame_count_sync");
    if (o.fixed_duration > 0) {
        // (known since before stage one)
    } else if (pend) {
        frames.resize(B);
        // through pinned memory behind an event on the stage-one stream: the host waits for this batch's stage one only, while the
        // previous batch's vocoder keeps the device busy
        HIP_OK(pend->frames_pinned.ensure((size_t)B, (size_t)B + 64));
        HIP_OK(hipMemcpyAsync(pend->frames_pinned.p, c.s1.frames, sizeof(int) * B, hipMemcpyDeviceToHost, stream));
        if (o.durations_out) HIP_OK(copy_durations(c, pend->dur_pinned));
        if (c.fit) HIP_OK(copy_fit_rows(c, pend->fit_pinned));
        HIP_OK(hipEventRecord(pend->s1_done, stream));
        prof.fence();
        HIP_OK(hipEventSynchronize(pend->s1_done));
        std::copy(pend->frames_pinned.p, pend->frames_pinned.p + B, frames.begin());
        if (o.durations_out) store_durations(c, pend->dur_pinned.p);
        if (c.fit) c.fit_report = fit_report(c, pend->fit_pinned.p);
    } else {
        frames.resize(B);
        // (pinned destination, owned by the engine: into the caller-side std::vector the copy went through the runtime's staging buffer, + 15 us per batch-1 call)
        HIP_OK(frames_host_.ensure((size_t)B, (size_t)B + 64));
        HIP_OK(hipMemcpyAsync(frames_host_.p, c.s1.frames, sizeof(int) * B, hipMemcpyDeviceToHost, stream));
        if (o.durations_out) HIP_OK(copy_durations(c, dur_host_));
        if (c.fit) HIP_OK(copy_fit_rows(c, fit_host_));
        prof.fence();
        HIP_OK(hipStreamSynchronize(stream));
        prof.fence();
        std::copy(frames_host_.p, frames_host_.p + B, frames.begin());
        if (o.durations_out) store_durations(c, dur_host_.p);
        if (c.fit) c.fit_report = fit_report(c, fit_host_.p);
    }
    if (o.durations_out && o.fixed_duration > 0)  // (no device read: every token lasts fixed_duration frames)
        for (int b = 0; b < B; ++b)
            for (int t = 0; t < id_stride; ++t) o.durations_out[(size_t)b * id_stride + t] = t < c.tlen[b] ? o.fixed_duration : 0;
    if (overlap) {
        // stage two runs on the main stream, behind this batch's stage one (pinned durations: no host read ordered them yet)
        if (o.fixed_duration > 0) HIP_OK(hipEventRecord(pend->s1_done, stream));
        HIP_OK(hipStreamWaitEvent(main_stream, pend->s1_done, 0));
    }
    s1_stream.restore();
    if (o.fixed_duration <= 0) c.frames_known();
    if (o.collect_taps) {
        TensorRef d;
        d.p = c.s1.dur;
        d.cs = id_stride;
        d.bs = id_stride;
        snapshot("durations", d, 1, c.Tmax, B, c.tlen);
    }
    if (o.frames_only) return frames_only_result(c, out);
    return run_stage_two(c, out, pend, want_async);
}

// ---- ragged batches: the lists of existing tiles of the fp32 vocoder's launches (tile_map.h) -------------------------------------------------------------
// Which launches take one is asked of the planners with the shapes and the policy run_vocoder_window32 will pass. A list is planned where the launch is large (kSmallGridBlocks, as tile_map_for) and its dense grid would hold blocks past an
// utterance's end; VITS_TILE_MAP plans it for every converted launch. Host arithmetic only.
void Engine::plan_tile_maps(Call& c) {
    c.tm_jobs.clear();
    c.tm_total = 0;
    const KernelKnobs& kn = knobs.kernel;
    if (arith_now_ != VITS_ARITH_F32 || split_on() || kn.no_tile_map || (c.B < 2 && !kn.tile_map)) return;
    const int B = c.B, n_up = c.n_up;
    const size_t nk = hp.rb_k.size();
    const VocPolicy pol = voc_policy(c);
    std::vector<int> la(B), lb(B);
    const WindowPlan& win = c.win;
    for (size_t wi = 0; wi < win.size(); ++wi) {
        const int64_t frames = win.stage_sum(wi, 0);
        auto smax = [&](int i) { return win.stage_max(wi, i); };
        auto want = [&](int vec, int width, bool convt, int64_t dense_blocks) {
            for (const Call::TileMapJob& j : c.tm_jobs)
                if (j.win == (int)wi && j.vec == vec && j.width == width && j.convt == convt) return;
            if (!kn.tile_map && dense_blocks < kSmallGridBlocks) return;
            const int vo = convt ? vec + 1 : vec;
            for (int b = 0; b < B; ++b) la[b] = win.len(wi, vec, b), lb[b] = win.len(wi, vo, b);
            if (!kn.tile_map && !tile_map_needed(la.data(), lb.data(), B, smax(vec), smax(vo), width, convt)) return;
            const int64_t n = tile_map_count(la.data(), lb.data(), B, width, convt);
            c.tm_jobs.push_back({(int)wi, vec, width, convt, c.tm_total, n});
            c.tm_total += n;
        };
        // a convolution over the lengths of stage `vec` (the transposed conv: upsampler `vec`), on the tile plan_conv gives it
        auto conv_width = [&](const PackedConv& w, int vec, int dil) {
            const bool convt = w.epi == EPI_CONVT;
            ConvCall shape;
            shape.batch = B;
            shape.t_in = smax(vec);
            shape.t_out = smax(convt ? vec + 1 : vec);
            shape.dil = dil;
            const ConvPlan pl = plan_conv(w, shape);
            if (!pl.ok || !conv_tile_mapped(pl.tile)) return;  // (the small tiles and the latency kernels keep their dense grids)
            want(vec, tile_shape(pl.tile).bn(), convt, (int64_t)pl.gx * pl.gy * pl.gz);
        };
        conv_width(dec_pre_, 0, 1);
        for (int i = 0; i < n_up; ++i) {
            const UpStageW& U = ups_[i];
            const int C = U.channels, vec = i + 1;
            conv_width(U.up, i, 1);
            const VocStage32Plan stage = plan_voc_stage32(U, B, smax(vec), frames, pol);
            for (size_t j = 0; j < nk; ++j) {
                const ResBlockW& R = U.rbs[j];
                const RbKernel kernel = stage.kernel_of(j);
                if (kernel == RbKernel::Block) {
                    const RbBlock32Plan pl = plan_rbblock32(C, R.k, B, smax(vec));
                    want(vec, rbblock32_geom(C, pl.nr).bo, false, (int64_t)pl.gx * pl.gy);
                } else if (kernel == RbKernel::Pairs) {
                    for (size_t d = 0; d < R.dil.size(); ++d) {
                        const LaunchGrid pl = plan_rbpair32(C, R.k, R.dil[d], B, smax(vec));
                        want(vec, rbpair32_geom(R.k, R.dil[d], C).bo, false, (int64_t)pl.gx * pl.gy);
                    }
                } else {
                    for (size_t d = 0; d < R.dil.size(); ++d) {
                        conv_width(R.c1[d], vec, R.dil[d]);
                        conv_width(R.c2[d], vec, 1);
                    }
                }
            }
        }
    }
}

// the lists into `pinned` (which outlives the copy: the engine's own for a synchronous call, the slot's for a pipelined batch), then one copy on the stream
hipError_t Engine::upload_tile_maps(Call& c, PinnedBuf<TileEntry>& pinned) {
    if (!c.tm_total) return hipSuccess;
    const size_t total = (size_t)c.tm_total;
    if (hipError_t e = pinned.ensure(total, total + total / 4 + 64)) return e;
    std::vector<int> la(c.B), lb(c.B);
    for (const Call::TileMapJob& j : c.tm_jobs) {
        for (int b = 0; b < c.B; ++b) la[b] = c.win.len(j.win, j.vec, b), lb[b] = c.win.len(j.win, j.convt ? j.vec + 1 : j.vec, b);
        if (tile_map_fill(la.data(), lb.data(), c.B, j.width, j.convt, pinned.p + j.off) != j.n) return hipErrorUnknown;
    }
    prof.fence();
    return hipMemcpyAsync(c.s2.tile_maps, pinned.p, sizeof(TileEntry) * total, hipMemcpyHostToDevice, stream);
}

void Engine::window_tile_maps(const Call& c, WinCtx& w) const {
    for (const Call::TileMapJob& j : c.tm_jobs)
        if (j.win == (int)w.wi && c.s2.tile_maps) (j.convt ? w.maps_up[j.vec] : w.maps[j.vec]).add(TileMapRef{c.s2.tile_maps + j.off, (int)j.n, j.width, j.convt});
}

// ---- the streaming state of a call with a sink (opts.on_chunk): window w's finished samples are multiplied (VITS_LEVEL_GAIN), resampled (an output rate) and
// shipped to pinned staging behind its kernels, and the PREVIOUS window's callbacks are served while the device works on this one
struct Engine::ChunkStream {
    Engine& e;
    Call& c;
    const bool rs, la;           // the output resampler runs; a level that multiplies
    Call::Rows pcm;              // what the call delivers
    size_t out_stride = 0;       // the longest delivered row: the row stride of the staging
    float* host_pcm = nullptr;   // pinned [B][out_stride] staging of the streamed PCM
    std::vector<hipEvent_t> ev;  // one per window: its PCM is on the host
    // streaming at another rate: after window w the model-rate samples [0, E_w) of an utterance are final, and with them the output samples whose taps all lie
    // in there (ResamplePlan::final_prefix; everything once the utterance has ended: the zeros behind its end are final). Window w resamples and delivers
    // [o_(w-1), o_w): rg [window][2][B], on the device as s2.out_ranges.
    // streaming under VITS_LEVEL_GAIN: window w multiplies the model-rate samples it makes final, [E_(w-1), E_w) of every utterance, once: lrg [window][2][B]
    std::vector<int> rg, lrg;
    ResampleCall rsc;
    LevelScale lsc;
    ChunkStream(Engine& e_, Call& c_) : e(e_), c(c_), rs(c_.dp[STAGE_RESAMPLE].runs), la(c_.dp.multiplies) {}
    ~ChunkStream() {
        for (hipEvent_t x : ev) hipEventDestroy(x);
    }

    int setup() {
        std::string& err = c.err;
        const int B = c.B;
        pcm = c.rows_of(c.dp.delivered);
        out_stride = (size_t)c.behind[STAGE_RESAMPLE].max;
        const size_t need = (size_t)B * out_stride * sizeof(float);
        HIP_OK(e.pinned_.ensure(need, need));
        host_pcm = (float*)e.pinned_.p;
        if (rs) {
            rsc = e.resample_out_call(c);
            if (e.upload_ranges(c, rg, c.s2.out_ranges, [&](int b, int64_t x) { return (int)c.rate_out->plan.final_prefix(x, c.behind[STAGE_RESAMPLE - 1].len[(size_t)b]); })) return -1;
        }
        if (la) {
            if (e.upload_ranges(c, lrg, c.s2.lvl_ranges, [](int, int64_t x) { return (int)x; })) return -1;
            const Call::Rows x = c.rows_of(c.dp[STAGE_LEVEL].src), y = c.rows_of(c.dp[STAGE_LEVEL].dst);
            lsc.x = x.p;  // (the call's own buffer: a level that multiplies keeps the vocoder there)
            lsc.x_stride = x.stride;
            lsc.y = y.p;
            lsc.y_stride = y.stride;
            lsc.lens = c.behind[STAGE_LEVEL - 1].dev;
            lsc.gain = e.level_gain();
            lsc.batch = B;
        }
        return 0;
    }

    // behind the kernels of window wi: ship its samples to the host, then serve the previous window's callbacks
    int after_window(size_t wi) {
        std::string& err = c.err;
        Profiler& prof = e.prof;
        hipStream_t const stream = e.stream;
        const int B = c.B;
        // (+ the no-crop tail of utterances that end inside this window, Q1; the same columns of longer utterances are not
        // final yet and travel again with the next window)
        size_t g0 = 0, g1 = 0;
        c.win.copy_span(wi, out_stride, g0, g1);
        if (la) {
            // the gain on what this window made final, before anything reads it (the resampler below, the copy to the host)
            int64_t n = 0;
            for (int b = 0; b < B; ++b) {
                const int64_t r = lrg[(wi * 2 + 1) * B + b] - lrg[(wi * 2) * B + b];
                lsc.max_range = std::max(lsc.max_range, r);
                n += r;
            }
            lsc.j0 = c.s2.lvl_ranges + (wi * 2) * B;
            lsc.j1 = lsc.j0 + B;
            PROF_LAUNCH("level_scale", (double)n, 8.0 * (double)n, launch_level_scale(lsc, stream));
            lsc.max_range = 0;
        }
        if (rs) {
            // the output samples this window made final, one launch for every utterance, then the columns they span
            g0 = out_stride, g1 = 0;
            int64_t in_s = 0, out_s = 0;
            for (int b = 0; b < B; ++b) {
                const int j0 = rg[(wi * 2) * B + b], j1 = rg[(wi * 2 + 1) * B + b];
                if (j1 <= j0) continue;
                g0 = std::min(g0, (size_t)j0), g1 = std::max(g1, (size_t)j1);
                rsc.max_range = std::max(rsc.max_range, (int64_t)(j1 - j0));
                out_s += j1 - j0;
                in_s += (int64_t)(j1 - j0) * rsc.plan.M / rsc.plan.L;
            }
            if (g1 > g0) {
                rsc.j0 = c.s2.out_ranges + (wi * 2) * B;
                rsc.j1 = rsc.j0 + B;
                HIP_OK(e.resample("resample_out", rsc, in_s, out_s));
            }
            rsc.max_range = 0;
        }
        if (g1 > g0)
            HIP_OK(hipMemcpy2DAsync(host_pcm + g0, out_stride * 4, pcm.p + g0, (size_t)pcm.stride * 4, (g1 - g0) * 4, (size_t)B, hipMemcpyDeviceToHost, stream));
        prof.fence();
        hipEvent_t done;
        HIP_OK(hipEventCreateWithFlags(&done, hipEventDisableTiming));
        ev.push_back(done);
        HIP_OK(hipEventRecord(done, stream));
        return wi > 0 ? flush(wi - 1) : 0;
    }

    int last_chunks() { return flush(c.win.size() - 1); }

   private:
    // hands the finished window `w` to the caller's sink (blocks until its PCM is on the host): 0, 1 the sink aborted, -1 the wait failed
    int deliver(size_t w) {
        const vits_process_opts& o = c.o;
        const int B = c.B;
        if (hipEventSynchronize(ev[w]) != hipSuccess) return -1;
        for (int b = 0; b < B; ++b) {
            if (rs) {
                // (a window that finalises nothing for an utterance makes no call for it)
                const size_t j0 = (size_t)rg[(w * 2) * B + b], j1 = (size_t)rg[(w * 2 + 1) * B + b];
                if (j1 > j0 && o.on_chunk(o.on_chunk_user, b, j0, host_pcm + (size_t)b * out_stride + j0, j1 - j0)) return 1;
                continue;
            }
            if (!c.win.owns(w, b)) continue;
            const size_t off = (size_t)c.win.chunk_begin(w), end = (size_t)c.win.final_end(w, b);
            if (o.on_chunk(o.on_chunk_user, b, off, host_pcm + (size_t)b * out_stride + off, end - off)) return 1;
        }
        return 0;
    }
    // ... and the one exit of a call whose sink aborted, or whose wait failed: the device idle, the message set
    int flush(size_t w) {
        const int rc = deliver(w);
        if (!rc) return 0;
        hipStreamSynchronize(e.stream);
        c.err = rc > 0 ? "aborted by the on_chunk callback" : "hipEventSynchronize failed";
        return -1;
    }
};

// the device table of a windowed call (WindowPlan::device_table) into s2.win_lens
int Engine::upload_window_table(Call& c, Pending* pend) {
    std::string& err = c.err;
    const std::vector<int> wl = c.win.device_table();
    if (pend) {
        // a pipelined batch: the table travels through pinned memory owned by the slot (it outlives this call), so that the submit does not
        // drain the main stream — the previous batch's vocoder is running there (the synchronise below serialised windowed submits)
        HIP_OK(pend->win_pinned.ensure(wl.size(), wl.size() + wl.size() / 4 + 64));
        std::memcpy(pend->win_pinned.p, wl.data(), sizeof(int) * wl.size());
        HIP_OK(hipMemcpyAsync(c.s2.win_lens, pend->win_pinned.p, sizeof(int) * wl.size(), hipMemcpyHostToDevice, stream));
        prof.fence();
    } else {
        HIP_OK(hipMemcpyAsync(c.s2.win_lens, wl.data(), sizeof(int) * wl.size(), hipMemcpyHostToDevice, stream));
        prof.fence();
        HIP_OK(hipStreamSynchronize(stream));  // wl goes out of scope
    }
    return 0;
}

// what the window functions see of window wi (engine_vocoder.cpp): everything in there is window-local
void Engine::window_ctx(const Call& c, size_t wi, WinCtx& w) const {
    const WindowPlan& win = c.win;
    const int B = c.B, n_up = c.n_up;
    const Call::Rows wave = c.rows_of(c.dp[STAGE_VOCODER].dst);  // (Call::rows_of: straight to out_device when nothing follows)
    w.wi = wi;
    w.wn = win[wi];
    w.Lw = w.wn.hi - w.wn.lo;
    w.smax.resize(n_up + 1);
    w.ssum.resize(n_up + 1);
    for (int i = 0; i <= n_up; ++i) w.smax[i] = win.stage_max(wi, i), w.ssum[i] = win.stage_sum(wi, i);
    const int* table = win.windowed ? c.s2.win_lens + wi * win.table_rows() * B : nullptr;
    for (int i = 0; i <= n_up && i < 8; ++i) w.d_len[i] = table ? table + (size_t)i * B : c.d_len_full[i];
    w.emit_hi = table ? table + (size_t)(n_up + 1) * B : nullptr;
    w.emit_lo = win.emit_lo(wi);
    w.zwin = make_ref(c.s2.zp, hp.flow_size, c.ls);
    w.zwin.p += w.wn.lo;
    w.pre.p = c.s2.pre;
    w.pre.bs = w.pre.cs = c.behind[STAGE_VOCODER].stride;
    w.wv.p = wave.p + (int64_t)w.wn.lo * win.M;  // window-local sample 0 is global sample lo * M
    w.wv.bs = wave.stride;
    w.wv.cs = (int)wave.stride;
    w.final_slope = c.refmode ? hp.lrelu : 0.01f;  // Q2 (vits.cpp:638)
    window_tile_maps(c, w);
}

// ---- stage two from the known frame counts on: vocoder windows, arena, latent (prior sampling, or the conversion front end), flow, vocoder,
// results. Shared by process_impl and convert_batch.
int Engine::run_stage_two(Call& c, vits_batch_result* out, Pending* pend, bool want_async) {
    std::string& err = c.err;
    const vits_process_opts& o = c.o;
    const int B = c.B, n_up = c.n_up;
    // the delivery chain behind the vocoder, planned once (its refusals were the entry points', before stage one was queued: nothing is refused here that was not
    // there), and what the host knows of the rows the call delivers: refused here, with nothing of stage two queued, if it was not before stage one
    if (plan_rows(c)) return -1;
    const DeliveryPlan& dp = c.dp;
    // the vocoder windows (long-form / streaming, vits.h vocoder_chunk_frames; window_plan.h): one window unless the call asked for chunks
    c.win.plan(c.frames.data(), B, c.smul.data(), c.sadd.data(), n_up, halo_frames_, o.vocoder_chunk_frames, o.collect_taps != 0);
    // the call delivers its PCM at another rate (vits_model_set_rates): the vocoder writes the model-rate waveform to the call's own buffer and resample.hip
    // writes what the caller gets; lengths, strides and stream offsets below are output-rate quantities (plan_rows)
    if (output_rate_ && !(c.rate_out = rate_table(hp.sampling_rate, output_rate_, err))) return -1;
    // a level that multiplies (every kind but VITS_LEVEL_MEASURE): the vocoder writes to the call's own buffer, loudness.hip measures it there and
    // multiplies it into what is delivered, or into the resampler's input. VITS_LEVEL_MEASURE measures the waveform where the vocoder wrote it
    c.lev = level_kind_;

    // (a call that returns with device work queued owns no pinned memory that outlives the copy of its lists: it keeps the dense grids)
    if (pend || !want_async) plan_tile_maps(c);
    if (layout_stage_two(c)) return -1;
    if (c.vc) {
        // voice conversion (engine_convert.cpp): spectrogram, posterior encoder and forward flow with the source speaker give z_p; the reverse
        // flow and the vocoder below then run with the target speaker
        if (run_conversion_front(c)) return -1;
        c.spk = c.vc->spk_tgt;
    } else if (run_prior_sampling(c)) return -1;
    if (run_flow(c)) return -1;
    // (filled here, behind the flow's launches: the device has work while the host writes the lists)
    HIP_OK(upload_tile_maps(c, pend ? pend->map_pinned : tile_map_host_));

    // ---- HiFiGAN (vits.cpp:583-644), window by window ---------------------------------------------------------------
    c.rx.phase("vits.hifigan");
    c.pitch_pin = pend ? &pend->pitch_pinned : &pitch_host_;
    // the device lengths of the rows behind every stage (Call::behind): what the stage writes, else what lies in front of it. The vocoder's sample counts, N' of
    // the tempo and the pitch stage in the arena, the trimmed lengths behind the edges' rows, the track lengths T_g behind the {o_b, n_b} rows of the joins' report
    if (dp[STAGE_EDGES].runs) HIP_OK(ed_.grow(B, owned_, weight_bytes));
    if (dp[STAGE_JOIN].runs) HIP_OK(jn_.grow(B, owned_, weight_bytes));
    const int* const own_lens[STAGE_COUNT] = {c.s1.stage_lens + (size_t)n_up * B, c.s2.tempo_lens, c.s2.pitch_lens, dp[STAGE_EDGES].runs ? edges_lens() : nullptr,
                                              dp[STAGE_JOIN].runs ? track_lens(B) : nullptr, nullptr, nullptr};
    const int* lens = nullptr;
    for (int s = 0; s < STAGE_RESAMPLE; ++s) {
        if (own_lens[s]) lens = own_lens[s];
        c.behind[s].dev = lens;
    }
    ChunkStream chunks(*this, c);
    if (o.on_chunk && chunks.setup()) return -1;
    if (c.win.windowed && upload_window_table(c, pend)) return -1;
    for (size_t wi = 0; wi < c.win.size(); ++wi) {
        WinCtx w;
        window_ctx(c, wi, w);
        if (c.fast16 ? run_vocoder_window16(c, w) : run_vocoder_window32(c, w)) return -1;
        if (o.on_chunk && chunks.after_window(wi)) return -1;
        if (o.collect_taps) {
            snapshot("pre_tanh", w.pre, 1, w.smax[n_up], B, c.slen[n_up]);
            snapshot("waveform", w.wv, 1, w.smax[n_up], B, c.slen[n_up]);
        }
    }
    std::function<int()> last_chunks;
    if (o.on_chunk) last_chunks = [&] { return chunks.last_chunks(); };
    if (run_delivery_tail(c, last_chunks)) return -1;
    return hand_over(c, out, pend, want_async, chunks.host_pcm);
}

// ---- results: the pipelined slot, the synchronous result (streamed: the pinned staging a sink's call has filled already), or the async tail; the report rows
// and the trimmed / track lengths once they have landed
int Engine::hand_over(Call& c, vits_batch_result* out, Pending* pend, bool want_async, const float* streamed) {
    std::string& err = c.err;
    const vits_process_opts& o = c.o;
    const DeliveryPlan& dp = c.dp;
    c.rx.phase("vits.results");
    const bool rs = dp[STAGE_RESAMPLE].runs;
    // what the call delivers: the vocoder's waveform, or (output rate set) the resampler's
    // (stated edges: the bounds; the lengths proper are read from the stage's rows below)
    const std::vector<int>& pcm_len = c.behind[STAGE_RESAMPLE].len;
    const int pcm_max = c.behind[STAGE_RESAMPLE].max;
    const Call::Rows pcm = c.rows_of(dp.delivered);
    const int B = c.B, R = c.behind[STAGE_RESAMPLE].n;  // what the call hands out: one row per utterance, or per track
    const int lv_n = c.lev ? R : 0, lm_n = dp.limits ? R : 0, ed_n = dp[STAGE_EDGES].runs ? B : 0, jn_n = c.join ? B : 0;  // the rows of the reports this call fills
    if (pend) {
        // a pipelined batch: everything the host will hand out is known now; the PCM (if a host copy was asked for) goes to the
        // slot's pinned staging behind the kernels, and `done` marks the end of the batch on the device
        pend->B = B;
        pend->stride = (size_t)pcm_max;
        pend->lengths.assign(pcm_len.begin(), pcm_len.end());
        pend->frames.assign(c.frames.begin(), c.frames.end());
        pend->lv_rows = lv_n;
        pend->lm_rows = lm_n;
        pend->ed_rows = ed_n;  // (lengths: the bounds until vits_model_wait reads the rows)
        pend->pt_rows = c.pit_rows;
        pend->fit_rows = c.fit_report;
        pend->host_copy = !o.skip_host_copy;
        if (pend->host_copy) {
            const size_t need = sizeof(float) * (size_t)B * pend->stride;
            HIP_OK(pend->host.ensure(need, need + need / 8));
            HIP_OK(hipMemcpy2DAsync(pend->host.p, pend->stride * 4, pcm.p, (size_t)pcm.stride * 4, pend->stride * 4, (size_t)B, hipMemcpyDeviceToHost, stream));
        }
        HIP_OK(hipEventRecord(pend->done, stream));
        prof.fence();
        return 0;
    }
    if (out) {
        // (a joined call: the lengths are the bounds until the track lengths have landed below; frames: the sums over each track's utterances)
        if (c.join) fill_result(out, R, (size_t)pcm_max, pcm_len.begin(), c.track_frames().begin());
        else fill_result(out, B, (size_t)pcm_max, pcm_len.begin(), c.frames.begin());
        if (!o.skip_host_copy) {
            out->data = new float[(size_t)R * out->stride];
            if (o.on_chunk) std::memcpy(out->data, streamed, sizeof(float) * (size_t)B * out->stride);  // already streamed to the host
            else
                HIP_OK(hipMemcpy2DAsync(out->data, out->stride * 4, pcm.p, (size_t)pcm.stride * 4, out->stride * 4, (size_t)R, hipMemcpyDeviceToHost, stream));
            prof.fence();
        }
    }
    async_tail_ = want_async;
    if (want_async) {
        // (the rows are on their way to the slot's pinned copy: the reports are valid after sync())
        lv_.expect(a1_slot_, lv_n), lm_.expect(a1_slot_, lm_n), ed_.expect(a1_slot_, ed_n);
        return 0;
    }
    HIP_OK(hipStreamSynchronize(stream));
    prof.fence();
    // the rows have landed: kept apart from the pinned copies, which a later submit into this slot overwrites; the trimmed lengths are what the call reports
    if (jn_n) {
        // the joins' rows and the track lengths have landed: the report names each utterance and its track; the call reports T_g (at the output rate)
        const int64_t* on = jn_.slot_rows(a1_slot_);
        const int* tl = track_lens(on, B);
        std::vector<int64_t> rows((size_t)4 * B);
        for (int g = 0; g < R; ++g)
            for (int b = c.join->first[(size_t)g]; b < c.join->first[(size_t)g + 1]; ++b) {
                rows[(size_t)4 * b] = join_index_[(size_t)b], rows[(size_t)4 * b + 1] = g;
                rows[(size_t)4 * b + 2] = on[(size_t)2 * b], rows[(size_t)4 * b + 3] = on[(size_t)2 * b + 1];
            }
        jn_.store(std::move(rows));
        if (out)
            for (int g = 0; g < R; ++g) out->lengths[g] = rs ? c.rate_out->plan.out_len(tl[g]) : tl[g];
    } else if (ed_n && out) edges_lengths(ed_.slot_rows(a1_slot_), B, out->lengths);
    lv_.landed(a1_slot_, lv_n), lm_.landed(a1_slot_, lm_n), ed_.landed(a1_slot_, ed_n);
    pt_.store(c.pit_rows);
    tm_.store(c.tem_rows);
    fit_rows_ = c.fit_report;
    // (event timings are read back lazily — vits_prof_report / vits_prof_reset — not here: ~1 ms of host work per call
    // with the device idle would otherwise sit inside the caller's timed region; cap the backlog for long runs)
    if (prof.on && prof.recs.size() > 50000) prof.collect();
    return 0;
}

}  // namespace vits
