// engine_internal.h — shared by the engine's translation units only (engine.cpp: one call from ids to PCM; engine_delivery.cpp: the delivery chain behind the vocoder; engine_load.cpp:
// weights; engine_stage1.cpp: text encoder + duration predictor; engine_flow.cpp: prior sampling + coupling flow;
// engine_vocoder.cpp: HiFiGAN; engine_convert.cpp / engine_align.cpp: voice conversion and forced alignment; engine_support.cpp: profiler, arenas,
// tokenizer, noise, roctx ranges).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "engine.h"
#include "window_plan.h"

namespace vits {

// ---- roctx ranges (VITS_ROCTX=1): the phases of a call as marker ranges for `rocprofv3 --marker-trace --kernel-trace` ---------
// The marker library is looked up at run time (librocprofiler-sdk-roctx.so, else libroctx64.so): no link-time dependency, and
// nothing at all happens unless the variable is set. Host-side ranges: they bracket the ENQUEUE of a phase's kernels (the call
// is asynchronous up to the one frame-count read-back), which is what a timeline viewer lines up with the kernel trace.
struct RoctxApi {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    RoctxApi();
};
const RoctxApi& roctx_api();
// consecutive phases of one call: phase(n) closes the previous range and opens the next; the destructor closes the last
struct RoctxPhases {
    bool open = false;
    void phase(const char* name) {
        const RoctxApi& a = roctx_api();
        if (!a.push) return;
        if (open) a.pop();
        a.push(name);
        open = true;
    }
    ~RoctxPhases() {
        if (open) roctx_api().pop();
    }
};
// a nested range (one vocoder stage)
struct RoctxRange {
    bool open = false;
    explicit RoctxRange(const char* name) {
        const RoctxApi& a = roctx_api();
        if (a.push) {
            a.push(name);
            open = true;
        }
    }
    ~RoctxRange() {
        if (open) roctx_api().pop();
    }
};

#define HIP_OK(expr)                                                 \
    do {                                                             \
        hipError_t e_ = (expr);                                      \
        if (e_ != hipSuccess) {                                      \
            err = std::string(#expr) + ": " + hipGetErrorString(e_); \
            return -1;                                               \
        }                                                            \
    } while (0)

#define KPROF(name, call)                  \
    do {                                   \
        prof.begin(name, 0, 0, stream);    \
        hipError_t e__ = (call);           \
        prof.end(stream);                  \
        if (e__ != hipSuccess) return e__; \
    } while (0)

// one profiled launch of the delivery chain and the streaming loop (chain: it reads what the launch in front of it wrote); -1 + err when it fails
#define PROF_LAUNCH(name, flops, bytes, call)                          \
    do {                                                               \
        prof.begin(name, flops, bytes, stream, /*chain=*/true);        \
        const hipError_t e = (call);                                   \
        prof.end(stream);                                              \
        HIP_OK(e);                                                     \
    } while (0)

// the ranges the entry points accept, and a float as their messages print it
inline bool rate_ok(float r) { return std::isfinite(r) && r >= 0.1f && r <= 10.f; }
inline bool noise_scale_ok(float v) { return std::isfinite(v) && v >= 0.f && v <= 10.f; }
inline std::string fmt_float(float v) {
    char buf[32];
    std::snprintf(buf, sizeof(buf), "%.9g", (double)v);
    return buf;
}

static inline TensorRef make_ref(float* p, int channels, int stride) {
    TensorRef t;
    t.p = p;
    t.cs = stride;
    t.bs = (int64_t)channels * stride;
    return t;
}
static inline TensorRef sub_rows(TensorRef t, int c0) {
    t.p += (int64_t)c0 * t.cs;
    return t;
}

// The buffers of one phase in an arena: `layout` runs once on a measuring arena and once on the real one, grown in between if it has to be (behind
// a stream synchronisation: growing frees memory that queued kernels may still read). 0, or -1 with err set.
template <class Layout>
int arena_layout(Arena& a, hipStream_t stream, std::string& err, Layout&& layout) {
    Arena measure;
    measure.cap = (size_t)1 << 60;
    layout(measure);
    const size_t need = measure.off + 4096;
    measure.cap = 0;
    if (need > a.cap) HIP_OK(hipStreamSynchronize(stream));
    HIP_OK(a.reserve(need));
    layout(a);
    return 0;
}

// a member that holds another value for a while: the stream being queued on, the arithmetic of the convs being queued, the stage-one slot
template <class T>
struct ScopedSet {
    T& slot;
    T saved;
    ScopedSet(T& s, T to) : slot(s), saved(s) { slot = to; }
    void restore() { slot = saved; }
    ~ScopedSet() { slot = saved; }
};

// "this call does not take opts.X": the first option of the list that the caller set, or null
struct OptSet {
    const char* name;
    bool set;
};
inline const char* first_set(std::initializer_list<OptSet> opts) {
    for (const OptSet& s : opts)
        if (s.set) return s.name;
    return nullptr;
}
// the per-utterance prosody of a text-to-speech call, which neither conversion nor alignment has a use for
inline const char* prosody_opt_set(const vits_process_opts& o) {
    return first_set({{"speaking_rates", o.speaking_rates != nullptr},
                      {"noise_scales", o.noise_scales != nullptr},
                      {"noise_scale_durations", o.noise_scale_durations != nullptr},
                      {"duration_override", o.duration_override != nullptr},
                      {"durations_out", o.durations_out != nullptr}});
}

void reference_noise_fill(float* dst, size_t n);  // the reference's process-global libstdc++ stream (vits.cpp:31)

// ---- everything one vits_model_process_batch call carries from phase to phase -------------------------------------------------
struct Call {
    const vits_process_opts& o;
    std::string& err;
    const int32_t* ids;
    int B, id_stride;
    int md = 0;  // resolved semantics mode
    bool refmode = true;
    int Tmax = 0, ts = 0, n_up = 0;
    std::vector<int> tlen;
    int64_t sum_t = 0;  // (profiler accounting: real work = sum of the utterance lengths)
    RoctxPhases rx;

    // stage one (sized by B x T)
    struct S1 {
        int *ids, *lens, *cum, *frames, *stage_lens, *stage_mul, *stage_add, *seed_off, *spk_row;
        // per-utterance prosody (header sections present only when the call passes the array, null otherwise): length scale 1 / rate,
        // prior noise scale, duration noise scale [B]; duration overrides [B][id_stride]
        float *len_scale, *noise_scale, *noise_scale_dur;
        int* dur_ovr;
        // a stated duration (Engine::run_fit; null unless the call fits): the groups [B] and the targets [B] by group in the header, and from the arena
        // e [B][id_stride], the override rows the kernel writes [B][id_stride], the group rows [B][kFitRowInts]
        int* fit_group;
        int* fit_target;
        float* fit_e;
        int* fit_ovr;
        int64_t* fit_rows;
        float *x, *qkv, *att, *tmp, *ffn, *stats, *dpx, *dpy, *dpp, *cond, *z, *u, *dur;
        float *ex_scores, *ex_tok;  // emulated-ggml mode 1 only
        uint16_t* x16;
    } s1{};
    std::vector<int> smul, sadd;  // vocoder stage lengths as affine functions of the frame count: len_i = L * smul[i] + sadd[i]
    int c_first = 0;              // physical row of z holding the log-durations after the duration predictor's flips
    // multi-speaker calls: the effective-bias table row of every utterance (device [B]: speaker + 1) — null when every utterance of the call is
    // speaker -1, so that such a call queues exactly the kernels (and reads exactly the biases) of a single-speaker model
    const int* spk = nullptr;
    std::vector<double> fit_report;            // ... and its rows [B][6] for vits_model_last_fit, once the group rows have landed beside the frame counts
    const Engine::ResolvedFit* fit = nullptr;  // a stated duration: the call's resolved fit (null: nothing is fitted, nothing is queued or allocated for it)
    RefNoiseAhead* ref_ahead = nullptr;  // batch 1, reference noise: the prior noise drawn while stage one runs (engine.cpp)
    // voice conversion (engine_convert.cpp): the call's input and the two speaker row arrays; null for text-to-speech
    struct Vc {
        float *pcm = nullptr, *spec = nullptr, *stats = nullptr;
        int* nsamp = nullptr;  // device [B]
        int64_t pcm_stride = 0;
        const int *spk_src = nullptr, *spk_tgt = nullptr;  // device [B] effective-bias rows, or null (every utterance -1)
        float eps_scale = 1.f;  // scale of the posterior draw (alignment's noise_scale; conversion: 1, VITS's draw)
    };
    Vc* vc = nullptr;

    // the one data-dependent shape (vits.cpp:1133)
    std::vector<int> frames;
    int Lmax = 0;
    std::vector<std::vector<int>> slen;  // [stage][utterance]
    std::vector<int> smax;               // [stage] longest
    int64_t sum_frames = 0;
    // `frames` is known (and smul / sadd): the longest, the sum, and every utterance's length at every vocoder stage
    void frames_known() {
        for (int f : frames) {
            Lmax = std::max(Lmax, f);
            sum_frames += f;
        }
        slen.assign(n_up + 1, std::vector<int>(B));
        smax.assign(n_up + 1, 0);
        for (int i = 0; i <= n_up; ++i)
            for (int b = 0; b < B; ++b) {
                slen[i][b] = frames[b] * smul[i] + sadd[i];
                smax[i] = std::max(smax[i], slen[i][b]);
            }
    }

    // the vocoder's waveform of the whole call, in samples (profiler accounting of the stages behind it)
    int64_t wave_samples() const { return sum_frames * smul[n_up] + (int64_t)B * sadd[n_up]; }
    // the frames of every track of a joined call: the sums over its utterances
    std::vector<int64_t> track_frames() const {
        std::vector<int64_t> tf((size_t)join->tracks, 0);
        for (int g = 0; g < join->tracks; ++g)
            for (int b = join->first[(size_t)g]; b < join->first[(size_t)g + 1]; ++b) tf[(size_t)g] += frames[b];
        return tf;
    }

    // vocoder windows (long-form / streaming): window_plan.h, planned where stage two begins (Engine::run_stage_two)
    WindowPlan win;

    // stage two (sized by B x L after the host read of the frame counts)
    struct S2 {
        float *zp, *noise, *hout, *gate, *h0, *bu, *bul, *by[3], *bt[3], *byl[3], *bs, *bs16, *pre, *wave;
        uint16_t* x16[3];
        uint16_t *sp_u, *sp_t[3], *sp_y[3];  // VITS_ARITH_F32_SPLIT: split planes of the stage input, and per concurrent resblock of t and of the stream
        int* win_lens;  // [window][n_up + 2][B]: stage lengths of each utterance inside the window, then its emit end
        float* wave_out;    // output rate set, no out_device: the delivered PCM [B][out_ws]
        int* out_ranges;    // output rate set, streaming: [window][2][B]: the output samples [j0, j1) of each utterance that window w finalises
        float* wave_lvl;    // a level that multiplies (VITS_LEVEL_GAIN ..), unless it goes straight to out_device: the levelled waveform [B][S_stride]
        void* lvl_scratch;  // a level set: level_scratch_bytes of loudness.hip
        void* lim_scratch;  // the limiter on: limit_scratch_bytes of limiter.hip
        float* wave_edge;   // stated edges on, unless the stage writes straight to out_device: its output [B][E_stride]
        void* ed_scratch;   // stated edges on: edges_scratch_bytes of edges.hip
        int* lvl_ranges;    // VITS_LEVEL_GAIN, streaming: [window][2][B]: the model-rate samples [j0, j1) of each utterance that window w finalises
        TileEntry* tile_maps;  // ragged fp32 calls: the lists of existing tiles of every window (tm_total entries), or null
        float* wave_join;      // a joined call, unless the join writes straight to out_device: the tracks [G][J_stride]
        int64_t* join_table;   // a joined call: join_table(plan)
        float* wave_pitch;     // a stated pitch, unless the stage writes straight to out_device: the varispeed rows [B][P_stride]
        float* pitch_ratios;   // a stated pitch: the ratios [B]
        int* pitch_lens;       // ... and N' of every row [B], written by the stage
        float* wave_tempo;     // a stated tempo, unless the stage writes straight to out_device: the stretched rows [B][T_stride]
        float* tempo_q;        // a stated tempo: the tempos [B]
        int* tempo_lens;       // ... N' of every row [B], written by the search
        int* tempo_starts;     // ... and the segment starts [B][tem_starts]: written by the search, read by the overlap-add
    } s2{};
    // Ragged batches, exact fp32 vocoder: the lists of existing tiles (tile_map.h) of the large launches whose dense grid would hold empty blocks. One list per
    // (window, length vector, tile width): length vector i = the lengths at vocoder stage i (conv_pre, the stage's resblocks), convt = upsampler i (columns
    // len_i + 1, output lengths of stage i + 1). Planned once the frame counts are known (Engine::plan_tile_maps), filled into pinned memory while the flow runs
    // and copied in-stream (Engine::upload_tile_maps); a call that needs none (a batch of one, equal lengths, small grids) plans none.
    struct TileMapJob {
        int win, vec, width;
        bool convt;
        int64_t off, n;  // first entry in s2.tile_maps, entries
    };
    std::vector<TileMapJob> tm_jobs;
    int64_t tm_total = 0;
    int ls = 0, lws = 0;
    size_t big = 0;        // floats of the largest vocoder activation (of one window)
    std::vector<int> sts;  // [stage] time stride of that stage's buffers
    bool fast16 = false, fuse16 = false;
    const int* d_len_full[8] = {};
    // The delivery chain behind the vocoder (delivery_plan.h), planned once per call (Engine::plan_delivery): who runs, and which buffer each stage reads and
    // writes. layout_stage_two allocates what the plan needs; rows_of is the ONE place where a buffer id of the plan becomes this call's pointer and row stride.
    DeliveryPlan dp;
    // What the chain holds BEHIND every stage, in the plan's order. A stage that does not run, or only reads (VITS_LEVEL_MEASURE), holds the set of the stage in
    // front of it: what stage X reads is always behind[X - 1], and what the call hands out is behind[STAGE_RESAMPLE]. Each field is filled where it becomes
    // known: n, len, max and stride by Engine::plan_rows (host arithmetic from the frame counts), dev by run_stage_two (behind the arena layout and the growth
    // of the edges' and the joins' rows, whose tails the trimmed and the track lengths are).
    struct RowSet {
        int n = 0;                 // rows: the utterances, or (from the join on) the tracks
        std::vector<int> len;      // what the host knows of each row: exact, or its bound (edges: N + Pl + Pt; join: the track's)
        int max = 0;               // the longest of them
        const int* dev = nullptr;  // the rows' lengths on the device [n], at the model's rate (null behind the resampler, which writes none)
        int stride = 0;            // row stride of the stage's own buffer (delivery_plan.h DeliveryStride states each)
    };
    RowSet behind[STAGE_COUNT];
    struct Rows {
        float* p = nullptr;
        int64_t stride = 0;
    };
    Rows rows_of(const DeliveryRoute& r) const {
        Rows out;
        switch (r.buf) {
            case BUF_WAVE: out.p = s2.wave; break;
            case BUF_EDGE: out.p = s2.wave_edge; break;
            case BUF_LVL: out.p = s2.wave_lvl; break;
            case BUF_OUT: out.p = s2.wave_out; break;
            case BUF_CALLER: out.p = (float*)o.out_device; break;
            case BUF_JOIN: out.p = s2.wave_join; break;
            case BUF_PITCH: out.p = s2.wave_pitch; break;
            case BUF_TEMPO: out.p = s2.wave_tempo; break;
            default: break;
        }
        switch (r.stride) {
            case STRIDE_S: out.stride = behind[STAGE_VOCODER].stride; break;
            case STRIDE_T: out.stride = behind[STAGE_TEMPO].stride; break;
            case STRIDE_P: out.stride = behind[STAGE_PITCH].stride; break;
            case STRIDE_E: out.stride = behind[STAGE_EDGES].stride; break;
            case STRIDE_J: out.stride = behind[STAGE_JOIN].stride; break;
            case STRIDE_OUT_WS: out.stride = behind[STAGE_RESAMPLE].stride; break;
            case STRIDE_CALLER: out.stride = o.out_device_stride; break;
            default: break;
        }
        return out;
    }
    const RateTable* rate_out = nullptr;  // output rate set (Engine::output_rate): the filter
    // a level set (Engine::level_kind): the kind of this call (dp.multiplies: every kind but VITS_LEVEL_MEASURE; dp.limits: through the limiter)
    int lev = 0;
    // a joined call (vits_model_process_joined): its tracks and gaps, and its bounds once plan_rows has run
    JoinPlan* join = nullptr;
    // A stated pitch (the call's resolved ratios [B], Engine::resolve_pitch or a conversion's; null: the stage is off): pit_rows = the report [B][4] = {P, N, N', K},
    // pitch_pin = the pinned memory the ratios travel through (the slot's for a pipelined batch)
    const float* pitch = nullptr;
    bool pitched() const { return pitch != nullptr; }
    std::vector<int64_t> pit_rows;
    PinnedBuf<float>* pitch_pin = nullptr;
    // A stated tempo (the call's resolved tempos [B], Engine::resolve_conversion_prosody; null: the stage is off): tem_rows = the report [B][4] = {Q, N, N', F};
    // tem_starts = the longest row's F + 1, the row stride of s2.tempo_starts
    const float* tempo = nullptr;
    bool tempoed() const { return tempo != nullptr; }
    std::vector<int64_t> tem_rows;
    int64_t tem_starts = 0;
    bool rows_planned = false;

    Call(const vits_process_opts& o_, std::string& err_, const int32_t* ids_, int B_, int id_stride_) : o(o_), err(err_), ids(ids_), B(B_), id_stride(id_stride_) {}
};

// one vocoder window, window-local lengths
struct WinCtx {
    size_t wi;
    WindowPlan::Win wn;
    int Lw;
    const int* d_len[8];
    std::vector<int> smax;      // window-local maxima per stage
    std::vector<int64_t> ssum;  // (profiler accounting) sum over utterances of the stage lengths inside this window
    const int* emit_hi;
    int emit_lo;
    TensorRef zwin, pre, wv;
    float final_slope;
    // the lists of existing tiles of this window (Call::tm_jobs): maps[i] for the launches over d_len[i], maps_up[i] for upsampler i; empty sets = dense grids
    TileMapSet maps[9], maps_up[8];
};

}  // namespace vits
