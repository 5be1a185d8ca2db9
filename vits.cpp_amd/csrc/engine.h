// engine.h — host orchestrator: owns the device-resident (pre-packed) weights, the activation arenas, the HIP
// stream, and issues the kernel sequence that replaces the reference's two ggml graphs
// (/root/reference/src/vits.cpp:975-1080 build_graph_part_one/two, :1082-1099 execute_graph, :1101-1191 process).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <functional>
#include <initializer_list>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/vits.h"
#include "delivery_plan.h"
#include "kernels.h"
#include "model_file.h"
#include "vocoder_plan.h"

namespace vits {

struct Tokenizer {
    std::vector<std::pair<std::string, int32_t>> vocab;  // sorted by descending key length
    int32_t blank_id = 0;
    bool add_blank = true;
    // config key "phonetic" == "1" (vits_model_data.cpp:92-94 -> vits_tokenizer::set_phonetic): the model was trained on espeak-ng phonemes. The
    // reference built without VITS_ESPEAK asserts out at load (vits_tokenizer.cpp:176-178); espeak is out of scope here, so the model
    // loads and the TEXT entry points refuse (tokenize_checked) — the id entry points are what such a model is driven through.
    bool phonetic = false;
    void init(const ModelFile& f);
    std::vector<int32_t> tokenize(const std::string& text) const;
    // the text entry points of the C ABI: false + message for a phonetic model; add_blank == 0 gives the reference's EMPTY id list (Q11,
    // vits_tokenizer.cpp:200-208: tokens_final is only filled under add_blank), which the callers report as "empty input"
    bool tokenize_checked(const std::string& text, std::vector<int32_t>& ids, std::string& err) const;
};

struct Profiler {
    struct Rec {
        int name_id;
        hipEvent_t a, b;
        double flop, bytes;
        bool a_shared;  // a is the previous record's b (back-to-back launches share one event)
        hipEvent_t spare = nullptr;  // dispatch-attached stop event that a multi-launch span replaced by a recorded one
    };
    bool attach = true;  // events ride on the kernel's dispatch packet (kernels.h: LaunchTimer); false: hipEventRecord around every launch
    bool on = false;
    std::vector<std::string> names;
    std::unordered_map<std::string, int> ids;
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    struct Agg {
        long calls = 0;
        double ms = 0, flop = 0, bytes = 0;
    };
    std::vector<Agg> agg;
    hipEvent_t get();
    // chain = true: if the previous timed launch ended on the same stream with nothing in between, its end event doubles as
    // this launch's start (an event is a barrier packet on the queue: half as many of them in the timed region)
    void begin(const char* name, double flop, double bytes, hipStream_t s, bool chain = false);
    void fence() { last_ok = false; }  // something un-timed was queued (or the host waited): do not chain across it
    hipEvent_t last_b = nullptr;
    hipStream_t last_s = nullptr;
    bool last_ok = false;
    void end(hipStream_t s);
    void collect();  // after a stream sync
    void reset();
    std::string report();
    ~Profiler();
};

struct Arena {
    char* base = nullptr;
    size_t cap = 0, off = 0;
    hipError_t reserve(size_t bytes);  // grow-only; invalidates previous contents
    void reset() { off = 0; }
    template <class T>
    T* alloc(size_t n) {
        off = (off + 255) & ~(size_t)255;
        T* p = reinterpret_cast<T*>(base + off);
        off += n * sizeof(T);
        return off <= cap ? p : nullptr;
    }
    ~Arena();
};

// Grow-only pinned host memory. ensure(n, grown): room for n elements, allocating `grown` (>= n: the site's own slack) when it has to grow; the
// old contents are gone then.
template <class T>
struct PinnedBuf {
    T* p = nullptr;
    size_t cap = 0;  // elements
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    hipError_t ensure(size_t n, size_t grown) {
        if (cap >= n) return hipSuccess;
        if (p) hipHostFree(p);
        p = nullptr;
        cap = 0;
        const hipError_t e = hipHostMalloc((void**)&p, sizeof(T) * grown, hipHostMallocDefault);
        if (e == hipSuccess) cap = grown;
        return e;
    }
    void swap(PinnedBuf& o) {
        std::swap(p, o.p);
        std::swap(cap, o.cap);
    }
    ~PinnedBuf() {
        if (p) hipHostFree(p);
    }
};

// The report rows of one delivery stage (levels and limits: float, edges: int64), one life cycle for all three: the device rows [cap][4] of the call being
// queued (grow-only; stream-ordered, so one buffer serves both pipeline slots) with `tail_bytes` more bytes per row behind them (the edges' trimmed lengths,
// int32 [cap]), their pinned host copy per pipeline slot, and the rows of the most recently completed call on the host (copied out of the pinned slot once
// they have landed: a later submit into that slot overwrites it).
template <class T>
class ReportRows {
  public:
    explicit ReportRows(size_t tail_bytes = 0) : per_row_(sizeof(T) * 4 + tail_bytes) {}
    T* dev() const { return dev_; }
    void* tail() const { return dev_ + (size_t)4 * cap_; }
    // room for B rows on the device. A fresh buffer takes the old one's place in `owned` and is counted in `weight_bytes` (the old rows are the previous
    // call's, already on their way to the host in stream order: hipFree waits for them)
    hipError_t grow(int B, std::vector<void*>& owned, int64_t& weight_bytes) {
        if (B <= cap_) return hipSuccess;
        const int cap = std::max(B, 64);
        T* fresh = nullptr;
        if (hipError_t e = hipMalloc((void**)&fresh, per_row_ * (size_t)cap)) return e;
        if (dev_) {
            for (void*& p : owned)
                if (p == dev_) p = fresh;
            hipFree(dev_);
        } else owned.push_back(fresh);
        weight_bytes += (int64_t)per_row_ * (cap - cap_);
        dev_ = fresh, cap_ = cap;
        return hipSuccess;
    }
    // the B device rows of the call being queued, on their way to the slot's pinned copy
    hipError_t queue_copy(int slot, int B, hipStream_t stream) {
        PinnedBuf<T>& host = host_[slot & 1];
        if (hipError_t e = host.ensure((size_t)4 * B, (size_t)4 * std::max(B, 64) + 64)) return e;
        return hipMemcpyAsync(host.p, dev_, sizeof(T) * 4 * (size_t)B, hipMemcpyDeviceToHost, stream);
    }
    const T* slot_rows(int slot) const { return host_[slot & 1].p; }
    // the first n rows of the slot's pinned copy have landed: they are the last call's rows (append: they follow the ones already kept)
    void landed(int slot, int n, bool append = false) {
        if (!append) store_.clear();
        const T* rows = host_[slot & 1].p;
        if (n > 0) store_.insert(store_.end(), rows, rows + (size_t)4 * n);
        rows_ = (int)(store_.size() / 4);
        unlanded_ = -1;
    }
    // a call that returned with its device work queued: n rows, valid once settle() has run behind a synchronisation
    void expect(int slot, int n) {
        store_.assign((size_t)4 * n, T());
        rows_ = n;
        unlanded_ = n > 0 ? slot : -1;
    }
    void settle() {
        if (unlanded_ >= 0) landed(unlanded_, rows_);
    }
    void clear() { rows_ = 0, unlanded_ = -1; }
    // rows [n][4] made on the host from what has landed (the joins': the device holds {o_b, n_b}, the report adds the index and the track)
    void store(std::vector<T> rows, bool append = false) {
        if (append) store_.insert(store_.end(), rows.begin(), rows.end());
        else store_ = std::move(rows);
        rows_ = (int)(store_.size() / 4);
        unlanded_ = -1;
    }
    // the rows [rows][4] of the most recently completed call (0 rows: it ran without the stage)
    const T* read(int& rows) const {
        rows = rows_;
        return store_.data();
    }

  private:
    size_t per_row_;
    T* dev_ = nullptr;
    int cap_ = 0;
    PinnedBuf<T> host_[2];
    std::vector<T> store_;
    int rows_ = 0;
    int unlanded_ = -1;  // the slot whose pinned copy an async call's rows are still on their way to
};

struct Tap {
    float* dev = nullptr;  // snapshot [batch][channels][stride]
    int channels = 0, stride = 0;
    std::vector<int> lens;   // per utterance
    std::vector<int> chans;  // per utterance channel counts (align_logp: [T_b][L_b]); empty = `channels` for every utterance
};

struct EncoderLayerW {
    PackedConv qkv, out, ffn1, ffn2;
    float *rel_k, *rel_v, *ln1_g, *ln1_b, *ln2_g, *ln2_b;
};
struct DdsW {
    std::vector<float*> dw_w, dw_b, n1_g, n1_b, n2_g, n2_b;
    std::vector<PackedConv> pw;
};
struct DpFlowW {
    float *pre_w, *pre_b;
    DdsW dds;
    PackedConv proj;
};
struct FlowLayerW {
    PackedConv pre, post;
    std::vector<PackedConv> in_layers, res_skip;
};
// Every VITS_* environment knob of the orchestrator, read ONCE when the model is loaded (never on the call path: getenv is
// not thread-safe against setenv, and a per-layer lookup is host time inside the caller's timed region). INTEGRATION.md §9.
struct Knobs {
    int rb_streams = 3;          // VITS_RB_STREAMS (1 serialises the three resblocks of a stage on the main stream)
    int lat16_lazy_tokens = 4096;  // VITS_LAT16_LAZY_TOKENS: a call of at most this many ids (batch x longest utterance) first makes the latency kernels' weight copy (0: never)
    bool lat16_eager = false;      // VITS_LAT16_EAGER: make that copy at load
    int rb16_serial_max_frames = 1300;  // VITS_RB16_SERIAL_MAX_FRAMES: 16-bit vocoder windows of at most this many frames (all utterances) use one stream ...
    int rb32_sum3_max_frames = 2000;   // VITS_RB32_SUM3_MAX_FRAMES: fp32 vocoder: the resblocks of a stage side by side + one sum launch while the call has fewer frames than this (batch 1 ... 8 x 128 ids: 2.80 -> 2.65, 5.06 -> 4.85 (3), 6.14 -> 5.89 (4), 10.82 -> 10.76 ms (8); 0: never)
    int rb16_serial_min_frames = 600;   // VITS_RB16_SERIAL_MIN_FRAMES: ... unless they have fewer than this (one or two 128-id utterances: kernels of 15-60 blocks, three of which side by side fill more of the chip than the fork / join costs — round 6, batch 1 / 2 / 4: 1.70 -> 1.60 / 1.77 -> 1.71 / 2.09 -> 2.17 ms with three streams)
    int lrelu_copy_minc = 128;   // VITS_LRELU_COPY_MINC: stages at least this wide also store leaky_relu(y)
    bool no_dds_fuse = false;    // VITS_NO_DDS_FUSE: DDS layer as three launches
    bool no_wn_fuse = false;     // VITS_NO_WN_FUSE: WaveNet layer as two launches
    bool no_group16 = false;     // VITS_NO_GROUP16: 16-bit vocoder through the fp32-layout (converter) path
    bool no_fuse16 = false;      // VITS_NO_FUSE16: 16-bit resblock conv pairs as two launches
    bool no_rbblock16 = false;   // VITS_NO_RBBLOCK16: 16-bit narrow-stage resblocks as three fused pairs instead of one kernel
    bool no_fuse32 = false;      // VITS_NO_FUSE32: fp32 resblock conv pairs as two launches
    bool no_rbblock32 = false;   // VITS_NO_RBBLOCK32: fp32 3-tap resblocks of the narrow stages as three fused pairs instead of one kernel
    bool no_rb_group = false;    // VITS_NO_RB_GROUP: the resblocks of a stage as separate launches (no grouped launch)
    bool rb_group_always = false;  // VITS_RB_GROUP=1: grouped launches also when the three streams are available
    bool no_flow_fuse = false;   // VITS_NO_FLOW_FUSE: 16-bit modes: a coupling layer of the flow as nine launches instead of one kernel
    bool prof_attach = true;     // VITS_PROF_ATTACH=0: per-kernel profiler with recorded events instead of dispatch-attached ones
    int front_prio = 1;          // VITS_FRONT_PRIO=0: the front-end stream of pipelined batches at normal instead of high priority
    bool keep_stage_sum32 = false;  // VITS_KEEP_STAGE_SUM32: 16-bit vocoder: also store the fp32 resblock sum of a stage's last resblock (nobody reads it)
    int split_min_batch = 128;   // VITS_SPLIT_MIN_BATCH: vits_model_process_batch splits batches of at least this many utterances in two pipelined parts (0: never).
                                 // Measured (f16, 128 ids): B = 64 split 32 + 32 LOSES (14.98 vs 14.34 ms: two half-size vocoder passes cost more than the hidden stage one)
    int split_first_pct = 50;    // VITS_SPLIT_FIRST_PCT: share of the utterances in the first part (its stage one is the exposed one)
    int flow_chains = 2;         // VITS_FLOW_CHAINS: 16-bit modes: the fused coupling layers of the flow as two independent chains of launches over halves of the batch (1: one chain)
    int flow_chain_min_blocks = 256;  // VITS_FLOW_CHAIN_MIN_BLOCKS: ... when a layer has more blocks than this (one block per CU at a time: 256 = one full round)
    int ref_ahead_frames_per_id = 6;  // VITS_REF_AHEAD_FRAMES_PER_ID: batch-1 calls with the reference noise stream draw the prior noise ahead, into a block sized for this many frames per id
                                      // (it grows if the utterance turns out longer; 0 = draw behind stage one as the reference does)
    bool no_pipeline = false;    // VITS_NO_PIPELINE: vits_model_submit_batch queues both stages on the main stream (no overlap)
    KernelKnobs kernel;          // the launch functions' own tuning knobs (kernels.h), installed per call by KernelKnobsScope
    void read();
};

// the reference stream of one batch-1 call drawn on a helper thread (engine_support.cpp): start, duration_noise, finish(n)
class RefNoiseAhead {
  public:
    RefNoiseAhead();
    ~RefNoiseAhead();
    RefNoiseAhead(const RefNoiseAhead&) = delete;
    RefNoiseAhead& operator=(const RefNoiseAhead&) = delete;
    void start(size_t n_dur, float* prior, size_t cap);  // draws n_dur values (the [T, 2] tensor), then the prior stream into `prior` (up to cap values)
    const float* duration_noise();                       // waits for the first tensor
    void rebase(float* prior, size_t cap);               // a larger prior buffer (values [0, drawn) copied by the caller), only when drawn() == capacity()
    void finish(size_t n);   // the prior tensor has n values: the global engine ends where exactly n draws leave it; joins the thread
    bool active() const { return active_; }
    size_t drawn() const;
    size_t capacity() const;

  private:
    struct Impl;
    Impl* impl_;
    bool active_ = false;
};

// sample-rate conversion (resample.hip): the filter of one (input rate, output rate) pair on the device, built at the pair's first use
struct RateTable {
    ResamplePlan plan;
    const float* taps = nullptr;  // device [K][L]
};

struct Call;    // engine_internal.h: the state of one process_batch call
struct WinCtx;  // engine_internal.h: one vocoder window

class Engine {
  public:
    ~Engine();
    bool load(const uint8_t* bytes, size_t size, std::string& err);
    // host-only: everything load() checks (format, hyper-parameters, every tensor's shape) without touching a device
    bool validate(const uint8_t* bytes, size_t size, std::string& err);
    int process_batch(const int32_t* ids, const int32_t* id_lens, int batch, int id_stride, const vits_process_opts& o, vits_batch_result* out,
                      std::string& err);
    // the utterances of a batch laid end to end inside the call (include/vits.h vits_model_process_joined): the batch runs per utterance up to and including
    // the edges stage, join.hip lays it into the tracks of (track, gap_ms) — as vits_join_plan takes them —, and the handle's level or limiter and the
    // resampler run on the tracks. Synchronous, never split, never pipelined. index [batch]: what the joins report names each utterance (null: b)
    int process_joined(const int32_t* ids, const int32_t* id_lens, int batch, int id_stride, const vits_process_opts& o, const int32_t* track, const float* gap_ms,
                       const int32_t* index, vits_batch_result* out, std::string& err);
    // the rows [B][4] = {index, track, o_b, n_b} (model rate) of the most recently completed joined call (empty: the last call did not join)
    const int64_t* last_joins(int& rows) const { return jn_.read(rows); }
    // pipelined batches (include/vits.h vits_model_submit_batch / vits_model_wait): up to two in flight
    // (part: a half of a batch split inside vits_model_process_batch, which has resolved the call's pitch — off, or it would not split)
    int submit_batch(const int32_t* ids, const int32_t* id_lens, int batch, int id_stride, const vits_process_opts& o, std::string& err, bool part = false);
    int wait_batch(vits_batch_result* out, std::string& err);
    int pending() const { return (int)(submit_seq_.load(std::memory_order_acquire) - wait_seq_.load(std::memory_order_acquire)); }  // (any thread may ask)
    // the refusal of every entry point that must not run beside submitted batches: true + the message while some are in flight
    bool refuse_pending(std::string& err) const {
        if (!pending()) return false;
        err = "batches in flight: call vits_model_wait for every submitted batch first";
        return true;
    }
    int sync(std::string& err);
    // One call at a time per handle (the reference's contract too: process writes member tensors, src/include/vits.h:22-30). The ABI
    // takes this flag around every entry point that touches the engine; a second thread gets "model busy" instead of a race.
    std::atomic<bool> busy{false};
    int set_arith(int arith, std::string& err);  // VITS_ARITH_*: packs the 16-bit weight fragments on first use
    // voice conversion (engine_convert.cpp, include/vits.h vits_model_convert_batch): prepare_conversion builds the posterior encoder, its speaker
    // terms and the forward-flow packs on the device (once; a handle that never converts never pays for them)
    int prepare_conversion(std::string& err);
    int convert_batch(const float* pcm, const int64_t* pcm_lens, int B, int64_t pcm_stride, const int32_t* src, const int32_t* tgt, const vits_process_opts& o,
                      vits_batch_result* out, std::string& err);
    // forced alignment (engine_align.cpp, include/vits.h vits_model_align_batch): text encoder (prior statistics per token) + the conversion front end (z_p of
    // the recording) -> align_logp -> align_mas (align.hip); durations [B][id_stride], frames [B] (optional), scores [B] (optional) on the host
    int align_batch(const float* pcm, const int64_t* pcm_lens, int B, int64_t pcm_stride, const int32_t* ids, const int32_t* id_lens, int id_stride,
                    const int32_t* speakers, float noise_scale, const vits_process_opts& o, int32_t* durations, int64_t* frames, float* scores, std::string& err);
    // speaker conditioning (multi-speaker models): the speaker of utterances the call does not name (vits_process_opts::speaker_ids == NULL,
    // vits_model_process / _ids); -1 = none
    int speaker = -1;
    int num_speakers() const { return hp.num_speakers > 1 ? hp.num_speakers : 1; }
    // 0, or -1 + a message naming the utterance: every speaker of the call in [-1, num_speakers), none >= 0 on a single-speaker model or with
    // the exact-order stage one (ggml_tables == 1)
    int check_speakers(const vits_process_opts& o, int B, std::string& err) const;
    // one speaker id against the rule of every speaker check: 0, or -1 + `who` and what is wrong with it (a single-speaker model takes -1 only;
    // otherwise -1 <= s < speaker_limit()). `outside`: the wording between `who` and the range (vits_model_set_speaker has its own)
    int check_speaker(int s, const std::string& who, std::string& err, const char* outside = " is outside [-1, ") const;
    // custom voices (engine_voices.cpp, include/vits.h vits_model_add_voices): speaker embeddings registered at run time. Voice k has the id
    // num_speakers + k and row 1 + num_speakers + k of the effective-bias tables, so the per-call row upload (speaker + 1) and every kernel stay as they are.
    // The ONE range rule of every speaker check (check_speaker): -1 <= s < speaker_limit().
    int num_voices() const { return hp.speaker_embedding_size > 0 ? (int)(voices_.size() / (size_t)hp.speaker_embedding_size) : 0; }
    int speaker_limit() const { return hp.num_speakers + num_voices(); }
    bool speaker_in_range(int s) const { return s >= -1 && s < speaker_limit(); }
    // each returns 0, or -1 + a message with the handle unchanged; none runs with batches in flight (the ABI checks pending() first)
    int add_voices(const float* emb, int n, int32_t* ids_out, std::string& err);
    int set_voice(int id, const float* emb, std::string& err);
    int clear_voices(std::string& err);
    int get_speaker_embedding(int id, float* dst, size_t cap, std::string& err) const;  // E, or -1
    int speaker_of(const vits_process_opts& o, int b) const { return o.speaker_ids ? o.speaker_ids[b] : speaker; }
    // prosody (include/vits.h vits_model_set_prosody): the values of every utterance a call gives none for (the prosody arrays of
    // vits_process_opts == NULL, vits_model_process / _ids); the model file's speaking_rate / noise_scale / noise_scale_duration at load
    float speaking_rate = 1.f, noise_scale = 0.667f, noise_scale_dur = 0.8f;
    // 0, or -1 + a message (the handle keeps its values): rate finite in [0.1, 10], noise scales finite in [0, 10]
    int set_prosody(float rate, float ns, float nsd, std::string& err);
    // 0, or -1 + a message naming the utterance (and the token): the call's prosody arrays in range, neither speaking_rates nor
    // duration_override together with fixed_duration
    int check_prosody(const vits_process_opts& o, int B, int id_stride, const int32_t* id_lens, std::string& err) const;
    // a stated pitch (include/vits.h "a stated pitch"; pitch.hip): the ratio of every utterance of a call that no per-utterance ratios were given for; 1 = off.
    // 0, or -1 + a message with the handle unchanged (a ratio that is not finite or outside [0.5, 2]). Nothing touches the device here: the table is uploaded
    // by the first call that shifts.
    float pitch_ratio = 1.f;
    int set_pitch(float ratio, std::string& err);
    // A value given for the NEXT call alone (vits_model_set_pitch_ratios, the two arrays of vits_model_set_conversion_ratios): give() copies it, NULL or n = 0
    // drops what was given; take() hands it to whichever entry point runs next, which uses it or refuses it: whatever becomes of that call, it is gone.
    struct TakeOnce {
        std::vector<float> v;
        void give(const float* p, int n) { v.assign(p, p + (p && n > 0 ? n : 0)); }
        bool take(std::vector<float>& out) {  // true: something had been given
            out.clear();
            out.swap(v);
            return !out.empty();
        }
    };
    // the per-utterance ratios of the next call. 0, or -1 + a message: n < 0, ratios NULL with n > 0
    int set_pitch_ratios(const float* ratios, int n, std::string& err);
    bool take_pitch_ratios(std::vector<float>& given) { return pitch_given_.take(given); }
    // A call's pitch. An entry point constructs it first of all: that takes the ratios given for this call, whatever becomes of the call. resolve_pitch then
    // decides: when some utterance's ratio is not 1, `pitch` points at `ratios` (the given ones, or the model value, per utterance) and o.speaking_rates at
    // `rates` (r'_b = (float)((double)rate_b / (double)p_b)); with every ratio 1, `pitch` stays NULL and `o` the caller's struct as it was.
    struct ResolvedPitch {
        vits_process_opts o;
        std::vector<float> given, ratios, rates;
        bool have;  // (declared behind `given`, which its initialiser fills)
        const float* pitch = nullptr;
        ResolvedPitch(Engine& e, const vits_process_opts& opts) : o(opts), have(e.take_pitch_ratios(given)) {}
    };
    // 0, or -1 + a message naming the utterance: another count of ratios than utterances; a ratio that is not finite or outside [0.5, 2]; fixed_duration > 0
    // or duration_override on an utterance whose ratio is not 1; an r'_b outside [0.1, 10]. The call's speaking_rates have passed check_prosody.
    int resolve_pitch(int B, int id_stride, const int32_t* id_lens, ResolvedPitch& rp, std::string& err) const;
    // the rows [B][4] = {P, N, N', K} of the most recently completed call (empty: it shifted nothing)
    const int64_t* last_pitch(int& rows) const { return pt_.read(rows); }
    // A stated duration (include/vits.h "a stated duration"; fit.hip): the fit of the NEXT call alone, given and taken like the ratios above (TakeOnce's
    // rule for a value that is not one float array). total: the call's utterances form one group whose target is targets[0], whatever their number.
    struct FitGiven {
        bool set = false, total = false, has_groups = false;
        std::vector<int64_t> targets;
        std::vector<int32_t> groups;
        float min_rate = kFitMinRate, max_rate = kFitMaxRate;
        void give(FitGiven g) { *this = std::move(g); }
        bool take(FitGiven& out) {  // true: something had been given
            out = std::move(*this);
            *this = FitGiven();
            return out.set;
        }
    };
    // 0, or -1 + a message (the shape of the arguments alone: n < 0, targets NULL with n > 0). NULL or n = 0 drops what was given.
    int set_fit(const int64_t* targets, const int32_t* groups, int n, float min_rate, float max_rate, std::string& err);
    int set_fit_total(int64_t total, float min_rate, float max_rate, std::string& err);
    bool take_fit(FitGiven& given) { return fit_given_.take(given); }
    // (vits_model_speak holds the total form while it cuts the text, and hands it to the joined call it then makes)
    void give_fit(FitGiven given) { fit_given_.give(std::move(given)); }
    // A call's fit. An entry point constructs it first of all, beside its ResolvedPitch: that takes what was given for this call. resolve_fit then decides:
    // `on` when some group has a target; group / target [B] are what the kernel reads (the header carries them to the device), s_lo / s_hi its limits.
    struct ResolvedFit {
        FitGiven given;
        bool have;  // (declared behind `given`, which its initialiser fills)
        bool on = false;
        std::vector<int> group;
        std::vector<int64_t> target;
        float s_lo = 1.f, s_hi = 1.f;
        explicit ResolvedFit(Engine& e) : have(e.take_fit(given)) {}
    };
    // 0, or -1 + a message naming the group or the utterance: another n than utterances; a group outside [0, B); a target outside [1, 2^22] and not 0;
    // rates outside 0.1 <= min <= max <= 10; fixed_duration > 0, async or the exact-order stage one with some group fitted; a fitted utterance whose
    // resolved pitch ratio (pitch [B], or NULL: all 1) is not 1
    int resolve_fit(int B, const vits_process_opts& o, const float* pitch, ResolvedFit& rf, std::string& err) const;
    // the largest L with L hop + sadd <= seconds x the model's rate, at least 1 (the model's mode decides sadd: set_stage_affine)
    int64_t fit_frames(double seconds) const;
    // the rows [B][6] = {group, F, sum d of the group, s*, R, status} of the most recently completed call (empty: it fitted nothing)
    const double* last_fit(int& rows) const {
        rows = (int)(fit_rows_.size() / 6);
        return fit_rows_.data();
    }
    // A conversion's rate and pitch (include/vits.h "a stated tempo": in a conversion; tempo.hip + pitch.hip): a conversion predicts no durations, so an
    // utterance with rate r and pitch p is time-stretched by q = (float)((double)r / (double)p) behind the vocoder and, when p != 1, played back p times faster by
    // the varispeed behind that. vc_rate / vc_pitch: the values of every utterance of a conversion that no pair was given for; 1 = off.
    // set_conversion_prosody: 0, or -1 + a message with the handle unchanged (a value that is not finite or outside [0.5, 2]).
    float vc_rate = 1.f, vc_pitch = 1.f;
    int set_conversion_prosody(float rate, float pitch, std::string& err);
    // the per-utterance pairs of the NEXT conversion (vits_model_set_conversion_ratios): copied here, taken by convert_batch alone, which constructs a
    // ResolvedConversion first of all. Either array may be NULL (the model value for every utterance); both NULL or n = 0 drops what was given.
    int set_conversion_ratios(const float* rates, const float* pitches, int n, std::string& err);
    struct ResolvedConversion {
        std::vector<float> rates, pitches;  // as given (empty: not given)
        int n = 0;
        bool have = false;
        std::vector<float> tempos, ratios;  // resolved: q_b and p_b [B]
        const float* tempo = nullptr;       // non-null: some q_b != 1, the tempo stage runs
        const float* pitch = nullptr;       // non-null: some p_b != 1, the pitch stage runs behind it
        explicit ResolvedConversion(Engine& e) {
            const bool r = e.vc_rates_given_.take(rates), p = e.vc_pitches_given_.take(pitches);
            have = r || p;
            n = (int)std::max(rates.size(), pitches.size());
        }
    };
    // 0, or -1 + a message naming the utterance: another count of pairs than utterances; r, p or q not finite or outside [0.5, 2]; on_chunk with any r or p
    // other than 1; a model rate the stretch does not take
    int resolve_conversion_prosody(int B, const vits_process_opts& o, ResolvedConversion& rc, std::string& err) const;
    // the rows [B][4] = {Q, N, N', F} of the most recently completed call (empty: it stretched nothing)
    const int64_t* last_tempo(int& rows) const { return tm_.read(rows); }
    // any sample rate (include/vits.h vits_model_set_rates): 0 = the model's own rate (a rate equal to it is stored as 0). input: the PCM given to
    // conversion and alignment; output: every PCM the handle delivers. 0, or -1 + a message with the handle unchanged (a rate outside the range, a
    // table that is too large). Nothing touches the device here: a pair's table is uploaded by the first call that uses it (rate_table).
    int set_rates(int in_rate, int out_rate, std::string& err);
    int input_rate() const { return input_rate_; }
    int output_rate() const { return output_rate_; }
    // a stated level (include/vits.h vits_model_set_level; loudness.hip): what every PCM the handle delivers is measured and multiplied by. 0, or -1 + a
    // message with the handle unchanged (an unknown kind, a value outside the kind's range). Nothing touches the device here: the row buffer is
    // allocated by the first call that levels.
    int set_level(int kind, float value_db, float ceiling_db, std::string& err);
    int level_kind() const { return level_kind_; }
    float level_value_db() const { return level_value_; }
    float level_ceiling_db() const { return level_ceiling_; }
    // the rows [B][4] of the most recently completed call (empty: it ran without a level). After an async call they are valid after sync().
    const float* last_levels(int& rows) const { return lv_.read(rows); }
    // the loudness target under a ceiling (include/vits.h vits_model_set_limiter; limiter.hip): with a mode set, the levelling kinds that multiply deliver
    // through the true-peak meter and the limiter. 0, or -1 + a message with the handle unchanged (an unknown mode, a model rate above 48000 Hz). Nothing
    // touches the device here: the 4x table and the row buffer are allocated by the first call that limits.
    int set_limiter(int mode, std::string& err);
    int limiter_mode() const { return limit_mode_; }
    // the rows [B][4] = {TP(x), TP(y), min s, share} of the most recently completed call (empty: it ran without the limiter)
    const float* last_limits(int& rows) const { return lm_.read(rows); }
    // stated edges (include/vits.h vits_model_set_edges; edges.hip): with a mode set, what the vocoder made is trimmed, faded and padded in front of
    // levelling. NULL or VITS_EDGES_OFF switches the stage off. 0, or -1 + a message with the handle unchanged (what edges_plan refuses). Nothing touches
    // the device here: the fade tables and the row buffer are allocated by the first call that runs the stage.
    int set_edges(const vits_edges_desc* d, std::string& err);
    const vits_edges_desc& edges_desc() const { return edges_desc_; }
    // the rows [B][4] = {a, b, N', n_active} of the most recently completed call (empty: it ran with the stage off)
    const int64_t* last_edges(int& rows) const { return ed_.read(rows); }
    // EMULATED ggml fp16 lookup tables for ggml_gelu / ggml_soft_max (Q8; inferred from upstream ggml, the fork is absent): builds the two
    // tables on the host as ggml_init does and uploads them on first use
    // mode 1: stage one additionally runs in the exact order of include/vits_exact_math.h (exact_stage1.hip), shared with the oracle: durations are
    // bit-identical to the oracle's. mode 2: the tables inside the throughput kernels (their own summation order: statistical agreement only).
    int set_ggml_tables(int mode, std::string& err);
    int ggml_tables = 0;
    int arith = VITS_ARITH_F32;
    // which convolutions a 16-bit arithmetic mode applies to (include/vits.h VITS_ARITH_SCOPE_*)
    int arith_scope = VITS_ARITH_SCOPE_FLOW_VOCODER;
    Knobs knobs;
    int64_t get_tap(const char* name, int utt, float* dst, size_t cap);

    HParams hp;
    Tokenizer tok;
    int mode = VITS_MODE_REFERENCE;
    int64_t weight_bytes = 0;
    Profiler prof;
    hipStream_t stream = nullptr;

  private:
    // weights
    float* emb_ = nullptr;
    std::vector<EncoderLayerW> enc_;
    PackedConv enc_proj_;
    PackedConv dp_pre_, dp_proj_;
    DdsW dp_dds_;
    float *dp_translate_ = nullptr, *dp_logscale_ = nullptr;
    std::vector<DpFlowW> dp_flows_;  // index f-1 for flows.f, f = 1..dp_flows
    // the deterministic duration predictor (hp.stochastic_duration == false; dp_det.hip), fp32 in every arithmetic mode: conv_1, conv_2, proj with their
    // 16x16x4 fragments made at load, the two LayerNorms. `in`: no conv at all — the H-channel segment of the effective-bias table that holds the speaker
    // term of the predictor's INPUT (plain "bias" zero, row 1 + s = cond.W g_s + cond.b); the kernels add its row on load, inside the utterance only
    struct DetDpW {
        PackedConv c1, c2, proj, in;
        float *g1 = nullptr, *be1 = nullptr, *g2 = nullptr, *be2 = nullptr;
    } dp_det_;
    bool load_det_predictor(const ModelFile& f, std::string& err);
    bool make_lat16(PackedConv& pc, std::string& err);  // pc.wp_l16 now, from the device copy of the packed weights (what ensure_lat16 does for every layer at the first small call)
    int run_duration_predictor_det(Call& c);
    DpDetCall det_call(const Call& c) const;
    std::vector<FlowLayerW> flow_;
    // voice conversion (engine_convert.cpp): host copies of what prepare_conversion packs (posterior_encoder.*, every flow.flows.*.conv_post, embed_speaker),
    // kept at load; then the packed posterior encoder, the forward flow's conv_post (x1 += mean: not negated), the posterior's effective-bias table and
    // the STFT tables
    std::vector<TensorEntry> vc_src_;
    bool vc_ready_ = false;
    struct PosteriorW {
        PackedConv pre, proj;
        std::vector<PackedConv> in_layers, res_skip;
    } post_;
    std::vector<PackedConv> flow_fwd_post_;
    float* stft_tw_ = nullptr;  // [n_fft / 2] complex
    float* stft_win_ = nullptr;
    int n_fft_ = 0, hop_ = 0, stft_pad_ = 0;
    PackedConv dec_pre_;
    std::vector<UpStageW> ups_;
    float* dec_post_w_ = nullptr;
    int dec_post_cin_ = 0, dec_post_k_ = 0;
    // host copies of every Conv1d / ConvTranspose1d weight (torch layout, after the flip / negation folds, in the file's storage
    // type), kept so that set_arith can pack the 16-bit A fragments on demand. Linear layers (q/k/v/out) are not listed: they stay fp32 (Q7).
    struct PackSrc {
        PackedConv* pc;  // (points into enc_/flow_/ups_...: those vectors are sized before their entries are packed and never resized)
        std::vector<float> w32;     // fp32-stored tensors
        std::vector<uint16_t> w16;  // fp16 / bf16-stored tensors, as stored
        uint32_t dtype;
        int cout, cin, k, epi, ct_stride;
        std::vector<float> widen() const {
            if (dtype != DT_F16 && dtype != DT_BF16) return w32;
            std::vector<float> w(w16.size());
            for (size_t e = 0; e < w.size(); ++e) w[e] = dtype == DT_F16 ? f16_to_f32(w16[e]) : bf16_to_f32(w16[e]);
            return w;
        }
    };
    std::vector<PackSrc> packs_;
    // the 16-bit A fragments of one conv on the device (VITS_ARITH_F16 / _BF16). *d is the buffer as soon as it is allocated: the caller owns it, also when
    // the upload behind it failed
    hipError_t pack16_device(const PackSrc& ps, int arith16, uint16_t** d, int64_t* bytes);
    struct Lat16Lazy {
        PackedConv* pc;
        size_t n;  // floats of the packed array
    };
    std::vector<Lat16Lazy> lat16_lazy_;  // layers that get a wp_l16 copy at the first small call (ensure_lat16)
    bool lat16_ready_ = false;
    int ensure_lat16(std::string& err);
    Ref16 x16_[3];           // per-stream scratch for the 16-bit copy of a conv input (transparent 16-bit path)
    size_t x16_cap_[3] = {0, 0, 0};
    // the scratch of the layout just made: `elems` elements behind every pointer that is not null
    void set_x16_scratch(uint16_t* p0, uint16_t* p1, uint16_t* p2, size_t elems) {
        uint16_t* const p[3] = {p0, p1, p2};
        for (int j = 0; j < 3; ++j) {
            x16_[j] = Ref16();
            x16_[j].p = p[j];
            x16_cap_[j] = p[j] ? elems : 0;
        }
    }
    bool vocoder_group_ok_ = false;  // every vocoder channel count is a multiple of 8: group-layout fast path available
    hipError_t conv16_transparent(const char* name, const PackedConv& w, const ConvCall& c, hipStream_t stream);
    hipError_t conv16(const char* name, const PackedConv& w, const Conv16Call& c, hipStream_t stream, double bytes);
    std::vector<void*> owned_;  // every device allocation made at load
    bool dry_run_ = false;

    // stage-one arenas: one per pipeline slot (a batch's stage two reads its stage-one results while the next batch's stage one runs)
    Arena a1_[2], a2_;
    int a1_slot_ = 0;
    Arena& a1() { return a1_[a1_slot_]; }
    // A batch submitted with submit_batch and not yet waited for. Its results are known on the host when submit returns (the frame
    // counts were read there); `done` marks the end of its device work, `host` is pinned staging for the PCM when a host copy was asked for.
    struct Pending {
        bool active = false;
        int B = 0;
        size_t stride = 0;
        std::vector<int64_t> lengths, frames;
        bool host_copy = false;
        PinnedBuf<char> host;  // (sized in bytes; read as float [B][stride])
        PinnedBuf<int> frames_pinned;
        PinnedBuf<int> win_pinned;    // vocoder-window length table of a windowed batch (host side of its H2D copy)
        PinnedBuf<TileEntry> map_pinned;  // lists of existing tiles of a ragged batch (host side of their H2D copy)
        PinnedBuf<float> dur_pinned;  // opts.durations_out: the batch's durations, copied beside the frame counts
        int lv_rows = 0;              // levelling: rows of the slot's pinned copy this batch fills (0: no level was set)
        int lm_rows = 0;              // the limiter: likewise (0: it was off)
        int ed_rows = 0;              // stated edges: likewise (0: off); `lengths` is derived from them once `done` has passed
        PinnedBuf<float> pitch_pinned;  // a stated pitch: the batch's ratios (host side of their H2D copy)
        std::vector<int64_t> pt_rows;   // ... and its report rows [B][4], host arithmetic (empty: it shifted nothing)
        PinnedBuf<int64_t> fit_pinned;  // a stated duration: the batch's group rows, copied beside the frame counts
        std::vector<double> fit_rows;   // ... and its report rows [B][6] (empty: it fitted nothing)
        hipEvent_t s1_done = nullptr, done = nullptr;
    } pend_[2];
    std::atomic<uint64_t> submit_seq_{0}, wait_seq_{0};  // batch n lives in pend_[n & 1]; written under the busy flag, read by vits_model_pending
    hipStream_t front_ = nullptr;             // stage one of pipelined batches (created on first use)
    // batch-1 calls with the reference noise stream: the prior noise is drawn into pinned memory while stage one runs (engine.cpp)
    PinnedBuf<float> ref_noise_pinned_;
    RefNoiseAhead ref_ahead_;
    PinnedBuf<float> dur_noise_pinned_;  // the [T, 2] duration noise of such a call
    hipEvent_t dur_noise_ev_ = nullptr;
    bool async_tail_ = false;                 // the last process_batch returned with device work still queued (opts.async)
    hipEvent_t ev_async_ = nullptr;           // orders the front-end stream behind that tail
    int process_split(const int32_t* ids, const int32_t* id_lens, int batch, int id_stride, const vits_process_opts& o, vits_batch_result* out, std::string& err);
    int process_impl(const int32_t* ids, const int32_t* id_lens, int batch, int id_stride, const vits_process_opts& o, vits_batch_result* out, std::string& err,
                     Pending* pend, JoinPlan* join = nullptr);
    int frames_only_result(Call& c, vits_batch_result* out);  // opts.frames_only: lengths[] and frames[] from the frame counts, no audio
    // a synchronous entry point's error return: whatever the failed call queued has run before the handle takes another (submit_batch does the same)
    void drain_streams();
    hipError_t copy_durations(const Call& c, PinnedBuf<float>& pinned);
    void store_durations(const Call& c, const float* pinned) const;
    // The three resblocks of a vocoder stage (kernel sizes 3/7/11) are independent chains of six convolutions; they run on
    // three streams so that the tail of one kernel's grid overlaps the head of another's. side_[j-1] carries resblock j.
    hipStream_t side_[2] = {nullptr, nullptr};
    hipEvent_t ev_fork_ = nullptr, ev_done_[3] = {nullptr, nullptr, nullptr};
    // How a stage's resblock chains are spread over them (engine_vocoder.cpp). par: chain jj on side_[jj - 1], the first on the main stream, else all on the
    // main stream. The last launch of chain j waits for chain j - 1's (the additions into the shared sum keep the reference's order) unless the resblocks run
    // side by side (sum3: own outputs + one sum launch behind the join of ALL chains); those may be enqueued longest (last) first.
    struct RbChains {
        size_t nk;
        bool par, sum3, longest_first;
        size_t resblock(size_t jj) const { return longest_first ? nk - 1 - jj : jj; }  // the jj-th chain enqueued
    };
    hipStream_t rb_stream(const RbChains& r, size_t jj) const { return r.par && jj > 0 ? side_[jj - 1] : stream; }
    hipError_t rb_fork(size_t n_side);                                          // the first n_side side streams behind what the main stream holds now
    hipError_t rb_chain_wait(const RbChains& r, size_t j, hipStream_t sj);     // in front of the last launch of resblock j's chain
    hipError_t rb_chain_done(const RbChains& r, size_t j, hipStream_t sj);     // behind it
    hipError_t rb_join(const RbChains& r);                                      // the main stream behind the chains
    int halo_frames_ = 0;      // receptive field of the vocoder in frames, one side (computed at load)
    PinnedBuf<char> pinned_;       // staging for streamed PCM (sized in bytes)
    PinnedBuf<int> frames_host_;   // destination of a synchronous call's frame-count copy (into pageable memory the copy went through a staging buffer: + 15 us at batch 1)
    PinnedBuf<int> align_host_;    // durations and scores of an alignment call (engine_align.cpp)
    PinnedBuf<float> dur_host_;    // a synchronous call's durations for opts.durations_out, copied beside the frame counts
    PinnedBuf<TileEntry> tile_map_host_;  // a synchronous call's lists of existing tiles (host side of their H2D copy; a call that returns with work queued builds none)
    // arithmetic of the convolutions being queued right now: `arith`, or fp32 while stage one runs under
    // VITS_ARITH_SCOPE_FLOW_VOCODER (every conv wrapper and fused kernel reads this one, never `arith` itself)
    int arith_now_ = VITS_ARITH_F32;
    // VITS_ARITH_F32_SPLIT: every dispatch sees VITS_ARITH_F32 (arith_kernels()); only the vocoder's resblock scheduling asks split_on()
    int arith_kernels() const { return arith == VITS_ARITH_F32_SPLIT ? VITS_ARITH_F32 : arith; }
    bool split_on() const { return arith == VITS_ARITH_F32_SPLIT; }
    // emulated-ggml mode 1: the stage-one tensors as the file holds them (host, storage type) and their fp32 device copies (first use)
    std::vector<TensorEntry> exact_src_;
    struct ExactTensor {
        const float* d = nullptr;
        int rank = 0;
        int64_t ne[4] = {1, 1, 1, 1};
    };
    std::map<std::string, ExactTensor> exact_w_;
    int run_stage_one_exact(Call& c);
    GgmlTables ggml_tabs_;              // what the stage-one kernels receive: null pointers unless ggml_tables
    uint16_t* ggml_tab_dev_ = nullptr;  // [2][65536]: gelu, exp
    struct HStage {  // pinned staging of the per-call host header (ids, lengths, stage tables)
        PinnedBuf<int> buf;
        hipEvent_t ev = nullptr;
        bool pending = false;
    } hstage_[2];
    int hstage_next_ = 0;
    std::map<std::string, Tap> taps_;
    int tap_batch_ = 0;
    int input_rate_ = 0, output_rate_ = 0;
    std::map<std::pair<int, int>, RateTable> rate_tabs_;  // keyed by (fi, fo); device tables are owned_ and counted in weight_bytes
    const RateTable* rate_table(int fi, int fo, std::string& err);  // null + message: the pair is refused, or the upload failed
    // The delivery chain behind the vocoder (delivery_plan.h): what this handle and the call's options ask for -> the call's plan. 0, or -1 + the message of
    // the combination the plan refuses (on_chunk with a level that needs the whole utterance, with the limiter, with edges; async with edges). Called before
    // stage one is queued by every entry point that can be refused, and by run_stage_two, which keeps the plan in the call.
    int plan_delivery(const vits_process_opts& o, DeliveryPlan& plan, std::string& err, bool joined = false) const;
    // What the host knows of the rows a call delivers, from the frame counts alone (no device work): the call's plan and the row set behind every stage of it
    // (Call::behind: rows, lengths or bounds, the longest, the row stride — N' behind tempo and pitch, the edges' pads, the tracks' bounds of a joined call,
    // the lengths at the output rate), and the refusals that follow from them — an utterance or track that is too long, an out_device_stride that cannot
    // hold the longest row. Runs before anything is queued when the frame counts are
    // host arithmetic (fixed_duration > 0), else as the first thing of stage two, directly behind the frame-count synchronise. Once per call.
    int plan_rows(Call& c);
    // the report rows of the stages (ReportRows: device rows owned_ and counted in weight_bytes); the edges' carry the trimmed lengths int32 [cap] behind them.
    // The joins' device rows of a call of B utterances hold {o_b, n_b} [B][2] and, behind them, the track lengths T_g int32 [G]
    ReportRows<float> lv_, lm_;
    ReportRows<int64_t> ed_{sizeof(int)}, jn_;
    // the pitch stage's rows are host arithmetic (P, N and N' follow from the ratio and the frame count): the report never touches the device
    ReportRows<int64_t> pt_;
    // ... and so are the tempo stage's (Q, N, N' and F follow from the tempo and the frame count)
    ReportRows<int64_t> tm_;
    // the device lengths behind those rows: the trimmed lengths [B] that run_edges writes, and the track lengths T_g [G] that run_join writes behind the
    // joins' {o_b, n_b} rows of a call of B utterances (device rows, or a slot's landed copy). What Call::behind[STAGE_EDGES].dev and behind[STAGE_JOIN].dev are when the stage runs
    int* edges_lens() { return static_cast<int*>(ed_.tail()); }
    static const int* track_lens(const int64_t* join_rows, int B) { return reinterpret_cast<const int*>(join_rows + (size_t)2 * B); }
    int* track_lens(int B) { return const_cast<int*>(track_lens(jn_.dev(), B)); }
    void clear_reports() { lv_.clear(), lm_.clear(), ed_.clear(), jn_.clear(), pt_.clear(), tm_.clear(), fit_rows_.clear(); }
    // a stated duration: the next call's fit, the resolved fit of the call being queued (non-null MEANS that the kernel runs), a synchronous call's group
    // rows on their way from the device, the report of the last completed call, and the kernel in front of either launch_durations: it returns the override
    // rows that launch takes (the call's own where nothing is fitted)
    FitGiven fit_given_;
    const ResolvedFit* call_fit_ = nullptr;
    PinnedBuf<int64_t> fit_host_;
    std::vector<double> fit_rows_;
    int run_fit(Call& c, TensorRef logw, int row, const int*& ovr);
    hipError_t copy_fit_rows(const Call& c, PinnedBuf<int64_t>& pinned);
    std::vector<double> fit_report(const Call& c, const int64_t* pinned) const;
    // a stated pitch: the interleaved table on the device (uploaded by the first call that shifts), a synchronous call's ratios on their way there, and the
    // stage from its source into its destination, as the call's plan routes them: queued behind the last vocoder window, in front of run_edges
    float* pitch_table_ = nullptr;
    PinnedBuf<float> pitch_host_;
    TakeOnce pitch_given_;                // vits_model_set_pitch_ratios: the next call's ratios
    const float* call_pitch_ = nullptr;   // the resolved ratios [B] of the call being queued (ResolvedPitch::pitch): non-null MEANS that the stage runs
    int run_pitch(Call& c);
    // a stated tempo: the next conversion's pairs, the resolved tempos [B] of the conversion being queued (non-null MEANS that the stage runs), their pinned
    // memory on the way to the device, and the stage (search, then overlap-add) from its source into its destination, as the call's plan routes them: queued
    // behind the last vocoder window, in front of run_pitch
    TakeOnce vc_rates_given_, vc_pitches_given_;
    const float* call_tempo_ = nullptr;
    PinnedBuf<float> tempo_host_;
    int run_tempo(Call& c);
    // the ratios [B] of either stage through `pin` (pinned: it outlives the copy) to `dev`, queued in front of the stage's launches
    int upload_ratios(const Call& c, const float* ratios, PinnedBuf<float>& pin, float* dev);
    PinnedBuf<int64_t> join_table_host_;  // a joined call's table (host side of its H2D copy)
    std::vector<int32_t> join_index_;     // ... and what its report names each utterance (process_joined: b, or the caller's index)
    // the join of a joined call (join.hip) from its source into its destination, as the call's plan routes them: queued behind the edges stage, in front of run_level
    int run_join(Call& c);
    // levelling: the handle's setting and the plan at the model's rate
    int level_kind_ = VITS_LEVEL_NONE;
    float level_value_ = 0.f, level_ceiling_ = 0.f;
    LoudnessPlan level_plan_;
    float level_gain() const { return (float)std::pow(10.0, (double)level_value_ / 20.0); }  // VITS_LEVEL_GAIN's factor, the float the levels rows report
    // measures the level stage's source and multiplies (or limits) it into the stage's destination, as the call's plan routes them (engine_delivery.cpp); queued behind
    // the last vocoder window
    int run_level(Call& c);
    // the limiter: the handle's mode and the plan at the model's rate
    int limit_mode_ = VITS_LIMIT_OFF;
    LimiterPlan limit_plan_;
    // stated edges: the handle's desc (VITS_EDGES_OFF and zeros when off), its plan at the model's rate, the fade tables on the device (uploaded by the first
    // call that needs them, and again after a set_edges that changed them)
    vits_edges_desc edges_desc_{(uint32_t)sizeof(vits_edges_desc), VITS_EDGES_OFF, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    EdgesPlan edges_plan_;
    float* ed_fades_ = nullptr;
    size_t ed_fades_n_ = 0;
    bool ed_fades_stale_ = false;
    bool edges_on() const { return edges_desc_.mode != VITS_EDGES_OFF; }
    // the stage from its source into its destination, as the call's plan routes them (engine_delivery.cpp): queued behind the last vocoder window, in front of run_level
    int run_edges(Call& c);
    // what a call delivers per utterance once its rows [B][4] have landed: N', or its length at the output rate
    void edges_lengths(const int64_t* rows, int B, int64_t* lengths) const;
    // the rows of a batch that has completed in pipeline slot `slot` -> the three reports (append: a second part of the same call); the batch's lengths become
    // its trimmed ones when the edges stage ran
    void batch_landed(Pending& p, int slot, bool append = false);
    // everything behind the last vocoder window (engine_delivery.cpp): the plan's stages in chain order (tempo, pitch, edges, join, level or limiter, the resampler), their taps, and the chunks of the
    // last window of a streaming call (last_chunks: null without a sink; -1 with the call's message set: the sink aborted, or the wait failed)
    int run_delivery_tail(Call& c, const std::function<int()>& last_chunks);
    ResampleCall resample_out_call(const Call& c) const;
    // a streaming call's table [window][2][B] (WindowPlan::range_table) on the host and on the device (dev): the samples [j0, j1) of every utterance that
    // each window makes final, in the unit of `final_of(b, e)`: what is final of utterance b once its model-rate samples [0, e) are
    int upload_ranges(Call& c, std::vector<int>& table, int* dev, const std::function<int(int, int64_t)>& final_of);
    // the streaming state of a call with a sink (engine.cpp), and the hand-over of a call's results: the pipelined slot, the synchronous result, the async tail
    struct ChunkStream;
    int upload_window_table(Call& c, Pending* pend);         // the device table of a windowed call; through the slot's pinned memory for a pipelined batch
    void window_ctx(const Call& c, size_t wi, WinCtx& w) const;  // what the vocoder's window functions see of window wi
    int hand_over(Call& c, vits_batch_result* out, Pending* pend, bool want_async, const float* streamed);
    // one profiled resample launch ("resample_out" / "resample_in"): 2 K flops per output sample, the input read once and the output written once
    hipError_t resample(const char* name, const ResampleCall& rc, int64_t in_samples, int64_t out_samples);

    float* upload(const std::vector<float>& v);
    struct ConvShape {
        int cout, cin, k;
    };
    float* upload_tensor(const ModelFile& f, const std::string& name, std::string& err, std::initializer_list<int64_t> want);
    bool pack(const ModelFile& f, const std::string& wname, const std::string& bname, int epi, ConvShape want, PackedConv& out, std::string& err,
              int ct_stride = 0, int transform = 0);
    bool load_dds(const ModelFile& f, const std::string& base, DdsW& d, std::string& err);
    // multi-speaker models: the effective-bias table (speaker_bias_kernel) and the conditioned layers pointed into its row 0
    bool load_speakers(const ModelFile& f, std::string& err);
    // An effective-bias table that can grow: rows 0 .. num_speakers are built at load (load_speakers; the posterior encoder's by prepare_conversion),
    // voices append rows (voices.hip). The conditioned PackedConvs point into row 0, so a table that moves repoints them (voice_rows); the 16-bit and
    // latency packs hold weights only and read the bias through the PackedConv at launch. The conditioning convs stay on the host until the first
    // registration makes them resident (d_w / d_b / d_segs).
    struct VoiceTable {
        float* table = nullptr;
        int64_t rs = 0;    // row stride, floats
        int cap_rows = 0;  // rows allocated
        struct Seg {
            PackedConv* pc;
            int n;
            int64_t off;
        };
        std::vector<Seg> segs;
        std::vector<float> cond_w, cond_b;  // host: the segments' conv rows, concatenated [sum n][E] / [sum n] (released once resident)
        float *d_w = nullptr, *d_b = nullptr;
        VoiceSeg* d_segs = nullptr;
        int tiles = 0;
    } vt_main_, vt_post_;
    // Builds the table of vt (segments, row stride and the segments' host conv rows filled in by the caller) for the file's speakers: allocates
    // num_speakers + 1 rows, one speaker_bias launch per segment (row 0 = the conv's plain bias), repoints the segments' convs into row 0. false: the
    // device failed (the convs keep their biases; the caller has the message)
    bool build_speaker_table(VoiceTable& vt, const std::vector<float>& emb);
    std::vector<float> spk_emb_;  // host [num_speakers][E]: embed_speaker widened to fp32 (vits_model_get_speaker_embedding, Model.add_voice_mix)
    std::vector<float> voices_;   // host [num_voices][E]: the registered vectors
    struct VoiceResident;  // engine_voices.cpp: a table's conditioning convs staged on the device, not yet the table's
    int voice_table_stage(VoiceTable& t, VoiceResident& r, std::string& err);
    // rows row_first .. row_first + n - 1 of every table in `tabs` from n host vectors: grows a table that is too small (capacity doubling, device-to-device
    // copy of rows [0, row_first), PackedConvs repointed), makes the conditioning convs resident on first use, one launch per table, one synchronisation;
    // every allocation is staged and handed over at the end: on failure nothing has changed, weight_bytes included
    int voice_rows(const std::vector<VoiceTable*>& tabs, const float* emb, int n, int row_first, std::string& err);
    hipError_t conv(const char* name, const PackedConv& w, ConvCall c, hipStream_t on = nullptr);  // on == nullptr: the main stream
    hipError_t run_dds(const DdsW& d, TensorRef x, TensorRef y, TensorRef p, const int* lens, int batch, int tmax, int64_t sum_t);
    // The DDS block on the latency kernels (stage1_lat.hip) with the per-token ops around it fused in: the head (a conv flow's 1 -> H conv +
    // conditioning, or an H -> H 1x1 conv of head_x) and the 1x1 conv behind the block (tail -> tail_y). Scratch a, b: [B][H][ts].
    struct DdsEnds {
        const float *head_w = nullptr, *head_b = nullptr;  // conv flow: pre weights / bias, latent z row zc, conditioning
        TensorRef z, cond;
        int zc = 0;
        const PackedConv* head_conv = nullptr;  // or: 1x1 conv of head_x
        TensorRef head_x;
        const int* spk = nullptr;  // head_conv's effective-bias table rows (multi-speaker calls)
        const PackedConv* tail_conv = nullptr;
        TensorRef tail_y;
    };
    bool dds_lat_ok(const DdsW& d, const DdsEnds& e, int batch, int tmax) const;
    hipError_t run_dds_lat(const DdsW& d, const DdsEnds& e, TensorRef a, TensorRef b, const int* lens, int batch, int tmax, int64_t sum_t);
    void snapshot(const char* name, TensorRef t, int channels, int stride, int batch, const std::vector<int>& lens);
    void clear_taps();
    // the phases of one call (engine_stage1.cpp, engine_flow.cpp, engine_vocoder.cpp); each returns 0 or -1 with c.err set
    int layout_stage_one(Call& c);
    int run_text_encoder(Call& c);
    int run_duration_predictor(Call& c);
    int layout_stage_two(Call& c);
    // ragged batches on lists of existing tiles (tile_map.h; Call::tm_jobs): which lists the call's fp32 vocoder launches take, from the host's lengths and the
    // planners (no device work); the fill into `pinned` + one in-stream copy; a window's sets as its launches find them
    void plan_tile_maps(Call& c);
    VocPolicy voc_policy(const Call& c) const;  // what the vocoder planner reads of the handle and the call (vocoder_plan.h); aligned: true until the window tests its buffers
    hipError_t upload_tile_maps(Call& c, PinnedBuf<TileEntry>& pinned);
    void window_tile_maps(const Call& c, WinCtx& w) const;
    int run_prior_sampling(Call& c);
    int run_flow(Call& c) { return run_coupling(c, false); }
    int run_coupling(Call& c, bool forward);  // the residual coupling flow: reverse (TTS), or forward (voice conversion)
    // One WaveNet stack (the flow's coupling layers, the posterior encoder) over h = rows [0, H) of s2.hout: zeroes the skip accumulator (rows [H, 2H)), then
    // every layer as one fused launch where the kernels take it, else as gated conv + res/skip 1x1. Speaker rows: c.spk.
    struct WaveNetLabels {
        const char *layer, *gated_conv, *conv1x1;  // profiler entries
    };
    int run_wavenet(Call& c, const std::vector<PackedConv>& in_layers, const std::vector<PackedConv>& res_skip, int n_layers, const WaveNetLabels& lab);
    int upload_host_noise(Call& c);  // opts.noise_prior or the reference stream -> s2.noise for every utterance, and the noise_prior tap
    void set_stage_affine(Call& c) const;  // c.smul / c.sadd: vocoder stage lengths as affine functions of the frame count
    int run_conversion_front(Call& c);        // spectrogram -> posterior encoder -> forward flow (engine_convert.cpp)
    // the PCM side of a conversion or alignment call (engine_convert.cpp): lengths checked, then frame counts, arena (current stage-one slot), uploads
    int check_conversion_pcm(const int64_t* pcm_lens, int B, int64_t pcm_stride, int64_t& nmax, std::vector<int64_t>& n_model, std::string& err) const;
    int layout_conversion(Call& c, const float* pcm, const int64_t* pcm_lens, int64_t pcm_stride, const int32_t* src, const int32_t* tgt, int64_t nmax,
                          const std::vector<int64_t>& n_model);
    int run_stage_two(Call& c, vits_batch_result* out, Pending* pend, bool want_async);
    // a tap of a tensor held with its channels reversed (the flow's physical layout for an odd number of coupling layers)
    void snapshot_flipped(const char* name, TensorRef t, int channels, int stride, int batch, const std::vector<int>& lens);
    int run_vocoder_window32(Call& c, WinCtx& w);
    int run_vocoder_window16(Call& c, WinCtx& w);
};

}  // namespace vits

struct vits_model {
    vits::Engine eng;
};
