// engine_delivery.cpp — the delivery chain behind the vocoder (delivery_plan.h): the handle's settings (rates, level, limiter, edges, pitch, a conversion's rate
// and pitch) and their plans, the call's routing plan (dp[STAGE_X], one array in chain order) and what the host knows of the rows behind every stage of it
// (Call::behind, filled by plan_rows: a stage reads behind[X - 1]), and the stages themselves: tempo, pitch, edges, join, level / limiter, the output resampler.
// engine.cpp's run_stage_two calls run_delivery_tail behind the last vocoder window. Compiled with hipcc as host C++.
#include <numeric>

#include "engine_internal.h"

namespace vits {


int Engine::set_pitch(float ratio, std::string& err) {
    PitchPlan p;
    std::string why;
    if (!pitch_plan(ratio, 0, p, why)) {
        err = "vits_model_set_pitch: " + why;
        return -1;
    }
    pitch_ratio = ratio;
    return 0;
}

int Engine::set_pitch_ratios(const float* ratios, int n, std::string& err) {
    if (n < 0 || (!ratios && n > 0)) {
        err = "vits_model_set_pitch_ratios: " + std::string(n < 0 ? "n < 0" : "null argument (ratios is NULL with n > 0)");
        return -1;
    }
    pitch_given_.give(ratios, n);
    return 0;
}

int Engine::resolve_pitch(int B, int id_stride, const int32_t* id_lens, ResolvedPitch& rp, std::string& err) const {
    const vits_process_opts& o = rp.o;
    const bool have = rp.have;
    if (have && (int)rp.given.size() != B) {
        err = "vits_model_set_pitch_ratios gave " + std::to_string(rp.given.size()) + " ratios, and this call has " + std::to_string(B) + " utterances";
        return -1;
    }
    const float* given = have ? rp.given.data() : nullptr;
    bool any = false;
    for (int b = 0; b < B; ++b) {
        const float p = given ? given[b] : pitch_ratio;
        if (!std::isfinite(p) || p < kPitchMinRatio || p > kPitchMaxRatio) {
            err = "pitch_ratios[" + std::to_string(b) + "] = " + fmt_float(p) + ": must be finite and in [0.5, 2]";
            return -1;
        }
        any = any || p != 1.f;
    }
    if (!any) return 0;
    rp.ratios.resize((size_t)B);
    rp.rates.resize((size_t)B);
    for (int b = 0; b < B; ++b) {
        const float p = rp.ratios[(size_t)b] = given ? given[b] : pitch_ratio;
        const float rate = o.speaking_rates ? o.speaking_rates[b] : speaking_rate;
        rp.rates[(size_t)b] = rate;  // (o.speaking_rates is the caller's until the last line)
        if (p == 1.f) continue;
        const std::string who = "utterance " + std::to_string(b) + " has the pitch ratio " + fmt_float(p) + ", which it pays for by being spoken slower by that ratio: ";
        if (o.fixed_duration > 0) {
            err = who + "fixed_duration > 0 leaves the duration predictor nothing to stretch";
            return -1;
        }
        if (o.duration_override) {
            const int len = std::min(id_stride, std::max(0, id_lens ? id_lens[b] : id_stride));
            for (int t = 0; t < len; ++t)
                if (o.duration_override[(size_t)b * id_stride + t] >= 0) {
                    err = who + "duration_override states token " + std::to_string(t) + "'s frames, which the stretch would have to change";
                    return -1;
                }
        }
        const float r = rp.rates[(size_t)b] = (float)((double)rate / (double)p);
        if (!rate_ok(r)) {
            err = who + "its speaking rate " + fmt_float(rate) + " becomes " + fmt_float(r) + ", outside [0.1, 10]";
            return -1;
        }
    }
    rp.pitch = rp.ratios.data();
    rp.o.speaking_rates = rp.rates.data();
    return 0;
}

int Engine::set_conversion_prosody(float rate, float pitch, std::string& err) {
    for (int side = 0; side < 2; ++side) {
        const float v = side ? pitch : rate;
        if (!std::isfinite(v) || v < kTempoMin || v > kTempoMax) {
            err = std::string("vits_model_set_conversion_prosody: ") + (side ? "pitch " : "rate ") + fmt_float(v) + " is not finite or outside [0.5, 2]";
            return -1;
        }
    }
    vc_rate = rate, vc_pitch = pitch;
    return 0;
}

int Engine::set_conversion_ratios(const float* rates, const float* pitches, int n, std::string& err) {
    if (n < 0) {
        err = "vits_model_set_conversion_ratios: n < 0";
        return -1;
    }
    vc_rates_given_.give(rates, n);
    vc_pitches_given_.give(pitches, n);
    return 0;
}

int Engine::resolve_conversion_prosody(int B, const vits_process_opts& o, ResolvedConversion& rc, std::string& err) const {
    if (rc.have && rc.n != B) {
        err = "vits_model_set_conversion_ratios gave " + std::to_string(rc.n) + " pairs, and this call has " + std::to_string(B) + " utterances";
        return -1;
    }
    const float* rates = rc.have && !rc.rates.empty() ? rc.rates.data() : nullptr;
    const float* pitches = rc.have && !rc.pitches.empty() ? rc.pitches.data() : nullptr;
    rc.tempos.assign((size_t)B, 1.f);
    rc.ratios.assign((size_t)B, 1.f);
    bool any_q = false, any_p = false;
    for (int b = 0; b < B; ++b) {
        const float r = rates ? rates[b] : vc_rate, p = pitches ? pitches[b] : vc_pitch;
        const std::string who = "utterance " + std::to_string(b) + ": ";
        for (int side = 0; side < 2; ++side) {
            const float v = side ? p : r;
            if (!std::isfinite(v) || v < kTempoMin || v > kTempoMax) {
                err = who + (side ? "conversion pitch " : "conversion rate ") + fmt_float(v) + " is not finite or outside [0.5, 2]";
                return -1;
            }
        }
        if (r == 1.f && p == 1.f) continue;
        if (o.on_chunk) {
            err = who + "on_chunk streams an utterance while it is being made, and this one has the conversion rate " + fmt_float(r) + " and pitch " + fmt_float(p) +
                  " (vits_model_set_conversion_ratios, vits_model_set_conversion_prosody): where a segment of the time stretch starts is decided by samples a "
                  "window's end does not have yet: call without on_chunk, or with every rate and pitch 1";
            return -1;
        }
        const float q = (float)((double)r / (double)p);
        if (!std::isfinite(q) || q < kTempoMin || q > kTempoMax) {
            err = who + "conversion rate " + fmt_float(r) + " over pitch " + fmt_float(p) + " is the tempo " + fmt_float(q) + ", outside [0.5, 2]";
            return -1;
        }
        if (hp.sampling_rate < kTempoMinRate || hp.sampling_rate > kTempoMaxRate) {
            err = who + "a conversion rate or pitch other than 1 needs a model rate in [8000, 48000] Hz (this model: " + std::to_string(hp.sampling_rate) + " Hz)";
            return -1;
        }
        rc.tempos[(size_t)b] = q, rc.ratios[(size_t)b] = p;
        any_q = any_q || q != 1.f, any_p = any_p || p != 1.f;
    }
    if (any_q) rc.tempo = rc.tempos.data();
    if (any_p) rc.pitch = rc.ratios.data();
    return 0;
}

int Engine::set_rates(int in_rate, int out_rate, std::string& err) {
    int stored[2] = {in_rate, out_rate};
    for (int side = 0; side < 2; ++side) {
        int& r = stored[side];
        if (r == 0 || r == hp.sampling_rate) {
            r = 0;
            continue;
        }
        ResamplePlan p;
        std::string why;
        if (!(side == 0 ? resample_plan(r, hp.sampling_rate, p, why) : resample_plan(hp.sampling_rate, r, p, why))) {
            err = std::string("vits_model_set_rates: ") + (side == 0 ? "input_rate: " : "output_rate: ") + why + " (the model's rate is " + std::to_string(hp.sampling_rate) + " Hz; 0 = that rate)";
            return -1;
        }
    }
    input_rate_ = stored[0], output_rate_ = stored[1];
    return 0;
}

const RateTable* Engine::rate_table(int fi, int fo, std::string& err) {
    const auto it = rate_tabs_.find({fi, fo});
    if (it != rate_tabs_.end()) return &it->second;
    RateTable t;
    if (!resample_plan(fi, fo, t.plan, err)) return nullptr;
    // the kernel reads [K][L]: at one tap the threads of a wave differ in their phase only (resample.hip)
    const std::vector<float> h = resample_taps(t.plan);
    std::vector<float> ht(h.size());
    for (int p = 0; p < t.plan.L; ++p)
        for (int k = 0; k < t.plan.K; ++k) ht[(size_t)k * t.plan.L + p] = h[(size_t)p * t.plan.K + k];
    if (!(t.taps = upload(ht))) {  // (owned by the handle and counted in weight_bytes from here on)
        err = "resampling table: device allocation failed";
        return nullptr;
    }
    return &rate_tabs_.emplace(std::make_pair(fi, fo), t).first->second;
}

hipError_t Engine::resample(const char* name, const ResampleCall& rc, int64_t in_samples, int64_t out_samples) {
    prof.begin(name, 2.0 * rc.plan.K * (double)out_samples, 4.0 * ((double)in_samples + (double)out_samples), stream, /*chain=*/true);
    const hipError_t e = launch_resample(rc, stream);
    prof.end(stream);
    return e;
}

int Engine::set_level(int kind, float value_db, float ceiling_db, std::string& err) {
    const char* who = "vits_model_set_level: ";
    std::string why;
    if (!level_values_ok(kind, value_db, ceiling_db, why)) {
        err = who + why;
        return -1;
    }
    if (kind != VITS_LEVEL_NONE) {
        LoudnessPlan p;
        if (!loudness_plan(hp.sampling_rate, p, why)) {
            err = who + ("the model's " + why);
            return -1;
        }
        level_plan_ = p;
    }
    // (with the limiter on a gain is delivered under the ceiling too: the value is checked and kept)
    const bool gain_ceiling = kind == VITS_LEVEL_GAIN && limit_mode_ != VITS_LIMIT_OFF;
    if (gain_ceiling && !level_values_ok(VITS_LEVEL_LOUDNESS, 0.f, ceiling_db, why)) {
        err = who + why;
        return -1;
    }
    level_kind_ = kind;
    level_value_ = kind >= VITS_LEVEL_GAIN ? value_db : 0.f;
    level_ceiling_ = kind == VITS_LEVEL_LOUDNESS || gain_ceiling ? ceiling_db : 0.f;
    return 0;
}

int Engine::set_limiter(int mode, std::string& err) {
    const char* who = "vits_model_set_limiter: ";
    if (mode != VITS_LIMIT_OFF && mode != VITS_LIMIT_TRUE_PEAK) {
        err = who + ("unknown mode " + std::to_string(mode));
        return -1;
    }
    if (mode != VITS_LIMIT_OFF) {
        LimiterPlan p;
        std::string why;
        if (!limiter_plan(hp.sampling_rate, p, why)) {
            err = who + ("the model's " + why);
            return -1;
        }
        limit_plan_ = p;
    }
    limit_mode_ = mode;
    return 0;
}

int Engine::plan_delivery(const vits_process_opts& o, DeliveryPlan& plan, std::string& err, bool joined) const {
    DeliveryAsk ask;
    ask.edges = edges_on();
    switch (level_kind_) {
        case VITS_LEVEL_NONE: ask.level = DLEVEL_NONE; break;
        case VITS_LEVEL_MEASURE: ask.level = DLEVEL_MEASURE; break;
        case VITS_LEVEL_GAIN: ask.level = DLEVEL_GAIN; break;
        default: ask.level = DLEVEL_WHOLE; break;  // (peak, loudness)
    }
    ask.limiter = limit_mode_ != VITS_LIMIT_OFF;
    ask.rate = output_rate_ != 0;
    ask.out_device = o.out_device != nullptr;
    ask.on_chunk = o.on_chunk != nullptr;
    ask.async = o.async != 0;
    ask.joined = joined;
    ask.pitch = call_pitch_ != nullptr;  // (resolved: Engine::resolve_pitch, or a conversion's Engine::resolve_conversion_prosody)
    ask.tempo = call_tempo_ != nullptr;  // (resolved: Engine::resolve_conversion_prosody)
    plan = delivery_plan(ask);
    switch (plan.refusal) {
        case DELIVER_OK: return 0;
        case REFUSE_LIMIT_STREAM:
            err = "on_chunk streams an utterance while it is being made, and this handle's limiter (vits_model_set_limiter) is on: the gain of a sample looks " +
                  std::to_string(limit_plan_.A) + " samples ahead and " + std::to_string(limit_plan_.H + limit_plan_.A) +
                  " back, so a window's last samples are not final when it ends, and the halo of finished samples that streaming would need is not built: "
                  "stream with VITS_LIMIT_OFF, or limit without on_chunk";
            break;
        case REFUSE_LEVEL_STREAM:
            err = "on_chunk streams an utterance while it is being made, and this handle's level (vits_model_set_level: measure, peak or loudness) needs the whole "
                  "utterance before its first sample can leave: only VITS_LEVEL_GAIN streams";
            break;
        case REFUSE_EDGES_STREAM:
            err = "on_chunk streams an utterance while it is being made, and this handle's edges stage (vits_model_set_edges) is on: the end of the utterance decides "
                  "what leaves (the last active window, the fade-out and the silence behind it count from there), so no sample can leave before the last one is made: "
                  "stream with VITS_EDGES_OFF, or set edges without on_chunk";
            break;
        case REFUSE_EDGES_ASYNC:
            err = "async returns before the device has finished, and this handle's edges stage (vits_model_set_edges) is on: lengths[] of the result is read from the "
                  "device (the trimmed length depends on the audio), which needs a host read behind the call's work: call without async, or pipeline with "
                  "vits_model_submit_batch / vits_model_wait";
            break;
        case REFUSE_JOIN_STREAM:
            err = "vits_model_process_joined: on_chunk streams an utterance while it is being made, and a track is laid out once every utterance of it has its length "
                  "(an overlap reaches back into the utterance in front): call without on_chunk";
            break;
        case REFUSE_JOIN_ASYNC:
            err = "vits_model_process_joined: async returns before the device has finished, and the lengths of the tracks are read from the device behind the call's "
                  "work: call without async";
            break;
        case REFUSE_PITCH_STREAM:
            err = "on_chunk streams an utterance while it is being made, and an utterance of this call has a pitch ratio other than 1 (vits_model_set_pitch_ratios, "
                  "vits_model_set_pitch): streaming pitch is not built (the varispeed of a window's last samples reads the next window's first): call without "
                  "on_chunk, or with every ratio 1";
            break;
        case REFUSE_PITCH_ASYNC:
            err = "async returns before the device has finished, and an utterance of this call has a pitch ratio other than 1 (vits_model_set_pitch_ratios, "
                  "vits_model_set_pitch): streaming pitch is not built, and the ratios travel to the device through memory the next call reuses: call without async, "
                  "or pipeline with vits_model_submit_batch / vits_model_wait";
            break;
        case REFUSE_TEMPO_STREAM:
            err = "on_chunk streams an utterance while it is being made, and an utterance of this conversion has a rate or pitch other than 1 "
                  "(vits_model_set_conversion_ratios, vits_model_set_conversion_prosody): where a segment of the time stretch starts is decided by samples a window's "
                  "end does not have yet: call without on_chunk, or with every rate and pitch 1";
            break;
        default: err = "this combination of delivery stages is not supported"; break;
    }
    return -1;
}

// the tail of a levelling call: loudness, peak and gain of every utterance of the stage's source (the plan's: what the vocoder or the edges stage wrote; under
// VITS_LEVEL_MEASURE that may be out_device, and no PCM path changes) -> the levels rows, the multiply into the stage's destination (every kind but MEASURE; a
// streaming call has multiplied window by window already), and the rows on their way to the slot's pinned copy
int Engine::run_level(Call& c) {
    std::string& err = c.err;
    const Call::RowSet& in = c.behind[STAGE_LEVEL - 1];  // (the rows the stage reads: the utterances, or a joined call's tracks)
    const int B = in.n;
    const Call::Rows src = c.rows_of(c.dp[STAGE_LEVEL].src), dst = c.rows_of(c.dp[STAGE_LEVEL].dst);
    HIP_OK(lv_.grow(B, owned_, weight_bytes));
    const int64_t samples = c.wave_samples();
    LevelCall lc;
    lc.x = src.p;
    lc.x_stride = src.stride;
    lc.lens = in.dev;
    lc.batch = B;
    lc.max_len = in.max;
    lc.plan = level_plan_;
    lc.scratch = c.s2.lvl_scratch;
    lc.kind = c.lev;
    lc.value_db = level_value_;
    lc.ceiling_db = level_ceiling_;
    lc.gain = level_gain();
    lc.levels = lv_.dev();
    // two walks of the cascade (9 fp64 fma a sample each) and the squares; the samples read twice
    PROF_LAUNCH("level_measure", 2.0 * (2 * 9 + 1) * (double)samples, 8.0 * (double)samples, launch_level_measure(lc, stream));
    if (c.dp.limits) {
        // the limiter in place of the plain multiply: meter, g0 (which replaces the measured row's gain), limiter, meter of what is delivered
        HIP_OK(lm_.grow(B, owned_, weight_bytes));
        const RateTable* up = rate_table(hp.sampling_rate, 4 * hp.sampling_rate, err);
        if (!up) return -1;
        LimitCall mc;
        mc.x = src.p;
        mc.x_stride = src.stride;
        mc.y = dst.p;
        mc.y_stride = dst.stride;
        mc.lens = lc.lens;
        mc.batch = B;
        mc.max_len = in.max;
        mc.plan = limit_plan_;
        mc.taps = up->taps;
        mc.scratch = c.s2.lim_scratch;
        mc.kind = c.lev;
        mc.value_db = level_value_;
        mc.gain = lc.gain;
        mc.ceiling = (float)std::pow(10.0, (double)level_ceiling_ / 20.0);
        mc.levels = lv_.dev();
        mc.limits = lm_.dev();
        // two meter passes (4 K fma a sample each); the doubling steps and the mean; x, e and y read, e and y written
        PROF_LAUNCH("limit", (2.0 * 2 * 4 * limit_plan_.up.K + limit_plan_.A + 16) * (double)samples, 20.0 * (double)samples, launch_limit(mc, stream));
        HIP_OK(lm_.queue_copy(a1_slot_, B, stream));
    } else if (c.dp.multiplies && !c.o.on_chunk) {
        LevelScale sc;
        sc.x = src.p;
        sc.x_stride = src.stride;
        sc.y = dst.p;
        sc.y_stride = dst.stride;
        sc.lens = lc.lens;
        sc.levels = lv_.dev();
        sc.batch = B;
        sc.max_range = in.max;
        PROF_LAUNCH("level_scale", (double)samples, 8.0 * (double)samples, launch_level_scale(sc, stream));
    }
    HIP_OK(lv_.queue_copy(a1_slot_, B, stream));
    prof.fence();
    return 0;
}

int Engine::set_edges(const vits_edges_desc* d, std::string& err) {
    const vits_edges_desc off{(uint32_t)sizeof(vits_edges_desc), VITS_EDGES_OFF, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (!d || (d->struct_size == sizeof(vits_edges_desc) && d->mode == VITS_EDGES_OFF)) {
        edges_desc_ = off;
        return 0;
    }
    EdgesPlan p;
    std::string why;
    if (!edges_plan(hp.sampling_rate, *d, p, why)) {
        err = "vits_model_set_edges: " + why;
        return -1;
    }
    ed_fades_stale_ = ed_fades_stale_ || p.Fi != edges_plan_.Fi || p.Fo != edges_plan_.Fo;  // (the tables depend on the two counts alone)
    edges_plan_ = p;
    edges_desc_ = *d;
    if (p.mode == VITS_EDGES_PAD) edges_desc_.threshold_db = 0.f;  // (ignored, and not kept)
    return 0;
}

// the edges stage of a call: the vocoder's waveform -> the stage's destination (the plan's: the call's own buffer, or out_device when nothing follows), the
// trimmed lengths (behind[STAGE_EDGES].dev: what every stage behind this one reads its rows' lengths from) and the rows on the device, and the rows on their way to the
// slot's pinned copy
int Engine::run_edges(Call& c) {
    std::string& err = c.err;
    const int B = c.B;
    const EdgesPlan& p = edges_plan_;
    const Call::Rows src = c.rows_of(c.dp[STAGE_EDGES].src), dst = c.rows_of(c.dp[STAGE_EDGES].dst);
    if (ed_fades_stale_) {
        const std::vector<float> t = edges_fades(p);
        if (ed_fades_) {
            // (the previous desc's tables: nothing reads them any more once the device is idle, and hipFree waits for that)
            owned_.erase(std::remove(owned_.begin(), owned_.end(), (void*)ed_fades_), owned_.end());
            hipFree(ed_fades_);
            weight_bytes -= (int64_t)ed_fades_n_ * 4;
            ed_fades_ = nullptr, ed_fades_n_ = 0;
        }
        if (!t.empty()) {
            if (!(ed_fades_ = upload(t))) {
                err = "fade tables: device allocation failed";
                return -1;
            }
            ed_fades_n_ = t.size();
        }
        ed_fades_stale_ = false;
    }
    EdgesCall ec;
    ec.x = src.p;
    ec.x_stride = src.stride;
    ec.lens = c.behind[STAGE_EDGES - 1].dev;
    ec.y = dst.p;
    ec.y_stride = dst.stride;
    ec.batch = B;
    ec.max_len = c.behind[STAGE_EDGES - 1].max;
    ec.plan = p;
    ec.fades = ed_fades_;
    ec.scratch = c.s2.ed_scratch;
    ec.lens_out = edges_lens();  // (= behind[STAGE_EDGES].dev: run_stage_two set it when it grew the rows)
    ec.rows = ed_.dev();
    const int64_t samples = c.wave_samples();
    // one multiply-add per sample in fp64; the samples read once, one double per window written
    if (p.mode != VITS_EDGES_PAD) PROF_LAUNCH("edges_window", 2.0 * (double)samples, 4.0 * (double)samples + 8.0 * (double)samples / p.W, launch_edges_window(ec, stream));
    PROF_LAUNCH("edges_bounds", 0, 8.0 * (double)samples / p.W, launch_edges_bounds(ec, stream));
    // two multiplies per sample; the samples read once, the bound written once
    PROF_LAUNCH("edges_apply", 2.0 * (double)samples, 8.0 * (double)samples + 4.0 * (double)B * (p.Pl + p.Pt), launch_edges_apply(ec, stream));
    HIP_OK(ed_.queue_copy(a1_slot_, B, stream));
    prof.fence();
    return 0;
}

void Engine::edges_lengths(const int64_t* rows, int B, int64_t* lengths) const {
    ResamplePlan plan;  // (the identity without an output rate)
    std::string ignored;
    if (output_rate_) resample_plan(hp.sampling_rate, output_rate_, plan, ignored);  // (accepted by set_rates already)
    for (int b = 0; b < B; ++b) lengths[b] = plan.out_len(rows[(size_t)4 * b + 2]);
}

// the streaming table of a call (WindowPlan::range_table: what every window makes final of every utterance) on the host and, synchronously, on the device
int Engine::upload_ranges(Call& c, std::vector<int>& table, int* dev, const std::function<int(int, int64_t)>& final_of) {
    std::string& err = c.err;
    c.win.range_table(table, final_of);
    HIP_OK(hipMemcpyAsync(dev, table.data(), sizeof(int) * table.size(), hipMemcpyHostToDevice, stream));
    prof.fence();
    HIP_OK(hipStreamSynchronize(stream));  // (pageable source; a streaming call is never a pipelined one)
    return 0;
}

// A stage whose N' is host arithmetic from a ratio and the row in front of it (tempo, pitch): plan(b, N, row, why) fills the row of the stage's report
// [B][4] = {the ratio as the stage holds it, N, N', a count of the stage's own}, or says why not. Fills behind[stage] from behind[stage - 1] (its rows hold at
// most twice theirs: the smallest ratio is 0.5) and the report; returns the largest count, or -1 with the call's message set.
template <class Plan>
static int64_t ratio_stage_rows(Call& c, int stage, const char* at_its, std::vector<int64_t>& report, Plan&& plan) {
    const Call::RowSet& in = c.behind[stage - 1];
    Call::RowSet& out = c.behind[stage];
    out.max = 0;
    out.stride = 2 * in.stride;
    report.resize((size_t)4 * c.B);
    int64_t most = 0;
    for (int b = 0; b < c.B; ++b) {
        int64_t row[4];
        std::string why;
        if (!plan(b, in.len[(size_t)b], row, why)) {
            c.err = "utterance " + std::to_string(b) + ": " + why;
            return -1;
        }
        if (row[2] > (int64_t)INT32_MAX - 64) {
            c.err = "utterance " + std::to_string(b) + " has " + std::to_string(row[2]) + " samples at its " + at_its + ": too long";
            return -1;
        }
        out.len[(size_t)b] = (int)row[2];
        out.max = std::max(out.max, out.len[(size_t)b]);
        most = std::max(most, row[3]);
        std::copy_n(row, 4, report.begin() + (size_t)4 * b);
    }
    return most;
}

// ---- what the host knows of the rows a call delivers (engine.h): host arithmetic from the frame counts, nothing is queued here
int Engine::plan_rows(Call& c) {
    if (c.rows_planned) return 0;
    std::string& err = c.err;
    const vits_process_opts& o = c.o;
    const int B = c.B, n_up = c.n_up;
    if (plan_delivery(o, c.dp, err, c.join != nullptr)) return -1;
    // the row sets behind every stage, in chain order (Call::behind): each starts as the set in front of it and changes what the stage changes; the strides are
    // computed here and nowhere else (delivery_plan.h DeliveryStride explains them)
    Call::RowSet* const set = c.behind;
    Call::RowSet& voc = set[STAGE_VOCODER];
    voc.n = B;
    voc.len = c.slen[n_up];
    voc.max = c.smax[n_up];
    voc.stride = round_up(voc.max, 32);
    set[STAGE_TEMPO] = voc;
    if (c.tempoed()) {
        const int64_t most = ratio_stage_rows(c, STAGE_TEMPO, "tempo", c.tem_rows, [&](int b, int n, int64_t* row, std::string& why) {
            TempoPlan tp;
            if (!tempo_plan(hp.sampling_rate, c.tempo[b], n, tp, why)) return false;
            row[0] = tp.Q, row[1] = n, row[2] = tp.n_out, row[3] = tp.F;
            return true;
        });
        if (most < 0) return -1;
        c.tem_starts = most + 1;
    }
    set[STAGE_PITCH] = set[STAGE_TEMPO];
    if (c.pitched()) {
        const int64_t most = ratio_stage_rows(c, STAGE_PITCH, "pitch ratio", c.pit_rows, [&](int b, int n, int64_t* row, std::string& why) {
            PitchPlan pp;
            if (!pitch_plan(c.pitch[b], n, pp, why)) return false;
            row[0] = pp.P, row[1] = n, row[2] = pp.n_out, row[3] = pp.K;  // (N' at most 2^31: N <= 2^30 and p >= 0.5; what does not fit is refused)
            return true;
        });
        if (most < 0) return -1;
    }
    // stated edges (vits_model_set_edges): the stage runs behind the last window; what the host knows of its output is every row's bound N + Pl + Pt
    Call::RowSet& ed = set[STAGE_EDGES] = set[STAGE_PITCH];
    if (c.dp[STAGE_EDGES].runs) {
        for (int b = 0; b < B; ++b) {
            const int64_t n = edges_plan_.bound(ed.len[(size_t)b]);
            if (n > (int64_t)INT32_MAX - 64) {
                err = "utterance " + std::to_string(b) + " has " + std::to_string(n) + " samples with its pads: too long";
                return -1;
            }
            ed.len[(size_t)b] = (int)n;
        }
        ed.max = *std::max_element(ed.len.begin(), ed.len.end());
        ed.stride = round_up(std::max(ed.max, 1), 32);
    }
    Call::RowSet& jn = set[STAGE_JOIN] = ed;
    const char* row_name = "utterance ";
    if (c.join) {
        // a joined call: the rows behind the join are the tracks, and what the host knows of each is its bound (the utterances' bounds and the positive gaps)
        const std::vector<int64_t> ub(ed.len.begin(), ed.len.end());
        std::string why;
        if (!join_bounds(*c.join, ub.data(), why)) {
            err = "vits_model_process_joined: " + why;
            return -1;
        }
        jn.n = c.join->tracks;
        jn.len.assign(c.join->bound.begin(), c.join->bound.end());  // (each at most kEdgesMaxLen = 2^30)
        jn.max = (int)c.join->max_bound;
        jn.stride = round_up(std::max(jn.max, 1), 32);
        row_name = "track ";
    }
    set[STAGE_LEVEL] = jn;  // (levelling changes no length, and a levelled buffer follows its input's stride)
    Call::RowSet& pcm = set[STAGE_RESAMPLE] = jn;
    if (output_rate_) {
        ResamplePlan plan;  // (the plan of the handle's table: set_rates accepted the pair)
        if (!resample_plan(hp.sampling_rate, output_rate_, plan, err)) return -1;
        pcm.max = 0;
        for (int r = 0; r < pcm.n; ++r) {
            const int64_t n = plan.out_len(pcm.len[(size_t)r]);
            if (n > (int64_t)INT32_MAX - 64) {
                err = row_name + std::to_string(r) + " has " + std::to_string(n) + " samples at the output rate: too long";
                return -1;
            }
            pcm.len[(size_t)r] = (int)n;
            pcm.max = std::max(pcm.max, (int)n);
        }
        pcm.stride = round_up(std::max(pcm.max, 1), 32);
    }
    if (o.out_device && !o.frames_only) {
        const bool rs = output_rate_ != 0;
        const std::vector<int>& len = pcm.len;
        const int longest = pcm.max;
        if (o.out_device_stride < longest) {
            if (c.join) {
                const int g = (int)(std::find_if(len.begin(), len.end(), [&](int n) { return n > o.out_device_stride; }) - len.begin());
                err = "vits_model_process_joined: out_device_stride = " + std::to_string(o.out_device_stride) + " is below track " + std::to_string(g) + "'s " +
                      std::to_string(len[(size_t)g]) + " samples";
            } else err = "out_device_stride is smaller than the longest utterance";
            if (rs) err += " (" + std::to_string(longest) + " samples at the output rate of " + std::to_string(output_rate_) + " Hz)";
            return -1;
        }
    }
    c.rows_planned = true;
    return 0;
}

// the ratios [B] of a stage on their way to the device, through pinned memory that outlives the copy
int Engine::upload_ratios(const Call& c, const float* ratios, PinnedBuf<float>& pin, float* dev) {
    std::string& err = c.err;
    HIP_OK(pin.ensure((size_t)c.B, (size_t)c.B + 64));
    std::copy_n(ratios, c.B, pin.p);
    HIP_OK(hipMemcpyAsync(dev, pin.p, sizeof(float) * (size_t)c.B, hipMemcpyHostToDevice, stream));
    prof.fence();
    return 0;
}

// ---- the pitch stage of a call: the vocoder's rows -> the stage's destination (the plan's), N' of every row on the device (c.s2.pitch_lens = behind[STAGE_PITCH].dev: what the stages
// behind it read their rows' lengths from). One launch serves every ratio of the batch; rows with ratio 1 are copied.
int Engine::run_pitch(Call& c) {
    std::string& err = c.err;
    const int B = c.B;
    const Call::Rows src = c.rows_of(c.dp[STAGE_PITCH].src), dst = c.rows_of(c.dp[STAGE_PITCH].dst);
    if (!pitch_table_ && !(pitch_table_ = upload(pitch_table_pairs()))) {  // (owned by the handle and counted in weight_bytes from here on)
        err = "pitch table: device allocation failed";
        return -1;
    }
    if (upload_ratios(c, c.pitch, *c.pitch_pin, c.s2.pitch_ratios)) return -1;
    PitchCall pc;
    pc.x = src.p;
    pc.x_stride = src.stride;
    pc.lens = c.behind[STAGE_PITCH - 1].dev;  // (the vocoder's sample counts, or behind a tempo stage what its search wrote)
    pc.ratios = c.s2.pitch_ratios;
    pc.y = dst.p;
    pc.y_stride = dst.stride;
    pc.table = pitch_table_;
    pc.lens_out = c.s2.pitch_lens;
    pc.batch = B;
    pc.max_out = c.behind[STAGE_PITCH].max;
    double taps = 0, in_s = 0, out_s = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t* row = c.pit_rows.data() + (size_t)4 * b;
        in_s += (double)row[1], out_s += (double)row[2];
        if (row[0] != kPitchOne) taps += (double)row[2] * (double)row[3];
    }
    // K fused multiply-adds a sample and the tap's own; every row read once and written once
    PROF_LAUNCH("pitch", 4.0 * taps, 4.0 * (in_s + out_s), launch_pitch(pc, stream));
    prof.fence();
    return 0;
}

// ---- the tempo stage of a conversion: the vocoder's rows -> the stage's destination (the plan's), N' of every row on the device (c.s2.tempo_lens = behind[STAGE_TEMPO].dev: what the
// stages behind it read their rows' lengths from). Two launches serve every tempo of the batch: the search (one block per row, its
// segments a chain) and the overlap-add; rows with tempo 1 are copied.
int Engine::run_tempo(Call& c) {
    std::string& err = c.err;
    const int B = c.B;
    const Call::Rows src = c.rows_of(c.dp[STAGE_TEMPO].src), dst = c.rows_of(c.dp[STAGE_TEMPO].dst);
    if (upload_ratios(c, c.tempo, tempo_host_, c.s2.tempo_q)) return -1;
    TempoCall tc;
    tc.x = src.p;
    tc.x_stride = src.stride;
    tc.lens = c.behind[STAGE_TEMPO - 1].dev;
    tc.tempos = c.s2.tempo_q;
    tc.rate = hp.sampling_rate;
    tc.starts = c.s2.tempo_starts;
    tc.starts_stride = c.tem_starts;
    tc.y = dst.p;
    tc.y_stride = dst.stride;
    tc.lens_out = c.s2.tempo_lens;
    tc.batch = B;
    tc.max_out = c.behind[STAGE_TEMPO].max;
    double diffs = 0, out_s = 0, steps = 0;
    TempoPlan tp;
    std::string ignored;
    tempo_plan(hp.sampling_rate, 1.f, 0, tp, ignored);  // (H and D: resolve_conversion_prosody accepted the rate)
    for (int b = 0; b < B; ++b) {
        const int64_t* row = c.tem_rows.data() + (size_t)4 * b;
        out_s += (double)row[2];
        if (row[0] != kTempoOne) steps += (double)row[3], diffs += (double)row[3] * (2.0 * tp.D + 1.0) * tp.H;
    }
    // an absolute difference and an add per candidate sample; a window of samples read per step, the starts written
    PROF_LAUNCH("tempo_search", 2.0 * diffs, 4.0 * steps * (2.0 * tp.D + 2.0 * tp.H) + 4.0 * steps, launch_tempo_search(tc, stream));
    // two products and an add a sample; two samples read and one written
    PROF_LAUNCH("tempo_ola", 3.0 * out_s, 12.0 * out_s, launch_tempo_ola(tc, stream));
    prof.fence();
    return 0;
}

// ---- the join of a joined call: the rows behind the edges stage -> the tracks (join.hip), the offsets and the track lengths on the device, and the joins'
// rows on their way to the slot's pinned copy
int Engine::run_join(Call& c) {
    std::string& err = c.err;
    const JoinPlan& p = *c.join;
    const int B = c.B;
    const Call::Rows src = c.rows_of(c.dp[STAGE_JOIN].src), dst = c.rows_of(c.dp[STAGE_JOIN].dst);
    const std::vector<int64_t> table = join_table(p);
    HIP_OK(join_table_host_.ensure(table.size(), table.size() + table.size() / 4 + 64));
    std::memcpy(join_table_host_.p, table.data(), sizeof(int64_t) * table.size());
    HIP_OK(hipMemcpyAsync(c.s2.join_table, join_table_host_.p, sizeof(int64_t) * table.size(), hipMemcpyHostToDevice, stream));
    prof.fence();
    JoinCall jc;
    jc.plan = &p;
    jc.x = src.p;
    jc.x_stride = src.stride;
    jc.lens = c.behind[STAGE_JOIN - 1].dev;
    jc.y = dst.p;
    jc.y_stride = dst.stride;
    jc.table = c.s2.join_table;
    jc.rows = jn_.dev();
    jc.track_lens = track_lens(B);  // (= behind[STAGE_JOIN].dev: run_stage_two set it when it grew the rows)
    int64_t in_s = 0, out_s = 0;
    for (const int64_t n : p.ubound) in_s += n;
    for (const int64_t n : p.bound) out_s += n;
    PROF_LAUNCH("join_offsets", 0, 20.0 * (double)B, launch_join_offsets(jc, stream));
    // at most one add per sample; every utterance read once, every track's bound written once
    PROF_LAUNCH("join_apply", (double)in_s, 4.0 * ((double)in_s + (double)out_s), launch_join_apply(jc, stream));
    HIP_OK(jn_.queue_copy(a1_slot_, B, stream));
    prof.fence();
    return 0;
}

// the call of the output resampler: what the plan routes into the stage -> what the call delivers, at the lengths the stages in front of it left
ResampleCall Engine::resample_out_call(const Call& c) const {
    const Call::Rows x = c.rows_of(c.dp[STAGE_RESAMPLE].src), y = c.rows_of(c.dp.delivered);
    ResampleCall rsc;
    rsc.x = x.p;
    rsc.x_stride = x.stride;
    rsc.lens = c.behind[STAGE_RESAMPLE - 1].dev;  // (device: every utterance's samples at the model's rate, the trimmed ones under stated edges)
    rsc.y = y.p;
    rsc.y_stride = y.stride;
    rsc.taps = c.rate_out->taps;
    rsc.plan = c.rate_out->plan;
    rsc.batch = c.behind[STAGE_RESAMPLE].n;
    return rsc;
}

// ---- everything behind the last vocoder window: the stages the call's plan runs, each reading what the one in front of it wrote (Call::rows_of of the plan's
// routes), their taps, and the last window's chunks of a streaming call (last_chunks: null without a sink; -1 with the call's message set)
int Engine::run_delivery_tail(Call& c, const std::function<int()>& last_chunks) {
    std::string& err = c.err;
    const vits_process_opts& o = c.o;
    const DeliveryPlan& dp = c.dp;
    const int B = c.B;
    const bool rs = dp[STAGE_RESAMPLE].runs;
    auto tap = [&](const char* name, const DeliveryRoute& r, int max_len, const std::vector<int>& lens) {
        const Call::Rows rows = c.rows_of(r);
        TensorRef t;
        t.p = rows.p;
        t.bs = rows.stride;
        t.cs = (int)t.bs;
        snapshot(name, t, 1, max_len, B, lens);
    };
    // what levelling and the taps behind it see of the model-rate rows on the host: the vocoder's sample counts, or (stated edges, taps only) the trimmed ones
    const Call::RowSet& pcm = c.behind[STAGE_RESAMPLE];
    std::vector<int> tap_len = c.behind[STAGE_PITCH].len, tap_out_len = pcm.len;
    int tap_max = c.behind[STAGE_PITCH].max, tap_out_max = pcm.max;
    if (dp[STAGE_TEMPO].runs) {
        if (run_tempo(c)) return -1;
        if (o.collect_taps) tap("waveform_tempo", dp[STAGE_TEMPO].after, c.behind[STAGE_TEMPO].max, c.behind[STAGE_TEMPO].len);
    }
    if (dp[STAGE_PITCH].runs) {
        if (run_pitch(c)) return -1;
        if (o.collect_taps) tap("waveform_pitch", dp[STAGE_PITCH].after, tap_max, tap_len);
    }
    if (dp[STAGE_EDGES].runs) {
        if (run_edges(c)) return -1;
        if (o.collect_taps) {
            // (a tap carries its rows' lengths: this debugging path reads the trimmed ones here, the call proper at its own synchronisation)
            HIP_OK(hipStreamSynchronize(stream));
            prof.fence();
            const int64_t* rows = ed_.slot_rows(a1_slot_);
            tap_max = tap_out_max = 0;
            for (int b = 0; b < B; ++b) {
                tap_len[b] = (int)rows[(size_t)4 * b + 2];
                tap_max = std::max(tap_max, tap_len[b]);
                if (rs) tap_out_max = std::max(tap_out_max, tap_out_len[b] = (int)c.rate_out->plan.out_len(tap_len[b]));
            }
            tap("waveform_edges", dp[STAGE_EDGES].after, tap_max, tap_len);
        }
    }
    if (dp[STAGE_JOIN].runs && run_join(c)) return -1;
    if (dp[STAGE_LEVEL].runs) {
        if (run_level(c)) return -1;
        if (o.collect_taps) tap("waveform_level", dp[STAGE_LEVEL].after, tap_max, tap_len);
    }
    if (rs && !o.on_chunk) {
        // nobody waits for parts of it: one launch over every utterance, behind the last window
        ResampleCall rsc = resample_out_call(c);
        rsc.max_range = pcm.max;
        HIP_OK(resample("resample_out", rsc, c.wave_samples(), std::accumulate(pcm.len.begin(), pcm.len.end(), (int64_t)0)));
    }
    if (rs && o.collect_taps) tap("waveform_out", dp[STAGE_RESAMPLE].after, tap_out_max, tap_out_len);
    return last_chunks ? last_chunks() : 0;
}

}  // namespace vits
