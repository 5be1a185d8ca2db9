// abi.cpp — the C ABI of include/vits.h. Nothing below throws across the boundary (the reference lets
// std::runtime_error escape and calls exit(1) from ASSERT: /root/reference/src/vits_model_data.cpp:102,144,
// src/include/debug.h:29-36); failures return NULL / {NULL,0} / -1 and set vits_last_error().
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <fstream>
#include <new>
#include <string>
#include <vector>

#include "../../include/vits.h"
#include "busy_guard.h"
#include "engine.h"
#include "pcm_gather.h"

namespace vits {
void reference_noise_seed(uint32_t seed);
}

static thread_local std::string g_last_error;
static void set_err(const std::string& e) { g_last_error = e; }

#define VITS_TRY try {
#define VITS_CATCH(ret)                           \
    }                                             \
    catch (const std::exception& e) {             \
        set_err(e.what());                        \
        return ret;                               \
    }                                             \
    catch (...) {                                 \
        set_err("unknown exception");             \
        return ret;                               \
    }

VITS_API const char* vits_last_error(void) { return g_last_error.c_str(); }

// One call at a time per model handle, enforced (busy_guard.h). Distinct handles run concurrently.
#define VITS_ENTER(model, ret)                                                                                                          \
    vits::BusyGuard busy_guard_((model) ? &const_cast<vits_model*>(model)->eng.busy : nullptr);                                        \
    vits::KernelKnobsScope kernel_knobs_scope_((model) ? &(model)->eng.knobs.kernel : nullptr);                                        \
    if ((model) && !busy_guard_.entered()) {                                                                                                 \
        set_err("model busy: another call is in progress on this handle (one call at a time per model; use one handle per thread)"); \
        return ret;                                                                                                                     \
    }

// ... and none beside submitted batches, for the entry points that change what those read (Engine::refuse_pending has the message)
#define VITS_ENTER_IDLE(model, ret)                          \
    VITS_ENTER(model, ret)                                   \
    {                                                        \
        std::string pending_err_;                            \
        if ((model)->eng.refuse_pending(pending_err_)) {     \
            set_err(pending_err_);                           \
            return ret;                                      \
        }                                                    \
    }

// the options of a call: the defaults, then what the caller gave (as much of it as the caller's struct_size and ours have in common)
static vits_process_opts default_opts(const vits_process_opts* given, int noise_kind) {
    vits_process_opts o;
    std::memset(&o, 0, sizeof(o));
    o.struct_size = sizeof(o);
    o.mode = VITS_MODE_DEFAULT;
    o.noise_kind = noise_kind;
    if (given) std::memcpy(&o, given, std::min<size_t>(sizeof(o), given->struct_size ? given->struct_size : sizeof(o)));
    return o;
}

// One engine call, run(err) -> 0 or an error code: on failure the message is set and a half-filled *out goes back — also when the engine throws
// (std::bad_alloc on the PCM buffer: nothing half-filled reaches the caller, *out is left zeroed, a waited-for batch stays waitable)
template <class Run>
static int run_engine(vits_batch_result* out, Run&& run) {
    std::string err;
    int rc;
    try {
        rc = run(err);
    } catch (...) {
        if (out) vits_free_batch_result(out);
        throw;
    }
    if (rc != 0) {
        set_err(err);
        if (out) vits_free_batch_result(out);
    }
    return rc;
}

// The result of a one-utterance batch as a vits_result (vits.cpp:1226-1231: a buffer of exactly `size` samples owned by the library). One utterance:
// stride == its length, so its row IS the result (no second buffer, no copy); the copy is for a result that is not of that shape. Empties br.
static vits_result take_row(vits_batch_result& br) {
    vits_result r{nullptr, (size_t)br.lengths[0]};
    if (br.batch == 1 && br.stride >= r.size) {
        r.data = br.data;
        br.data = nullptr;
    } else {
        r.data = new float[r.size];
        std::memcpy(r.data, br.data, sizeof(float) * r.size);
    }
    vits_free_batch_result(&br);
    return r;
}

// reference: src/vits.cpp:1205-1215
VITS_API vits_model* vits_model_load_from_bytes(const char* bytes, size_t size) {
    VITS_TRY
    if (!bytes) {
        set_err("null model bytes");
        return nullptr;
    }
    vits_model* m = new vits_model();
    std::string err;
    if (!m->eng.load(reinterpret_cast<const uint8_t*>(bytes), size, err)) {
        set_err(err);
        delete m;
        return nullptr;
    }
    return m;
    VITS_CATCH(nullptr)
}

// reference: src/vits.cpp:1193-1203 -> vits_model_data::from_file src/vits_model_data.cpp:99-109
VITS_API vits_model* vits_model_load_from_file(const char* path) {
    VITS_TRY
    if (!path) {
        set_err("null path");
        return nullptr;
    }
    std::ifstream f(path, std::ios::binary);
    if (!f.is_open()) {
        set_err(std::string("[ERROR] failed to open file: ") + path);  // message of vits_model_data.cpp:102
        return nullptr;
    }
    std::vector<char> buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    return vits_model_load_from_bytes(buf.data(), buf.size());
    VITS_CATCH(nullptr)
}

// reference: src/vits.cpp:1217-1219
// A handle another thread is inside (or that a callback is running on) is NOT freed: the call would go on using the engine it
// runs on. The refusal path does not touch the flag (the compare-exchange fails without writing: the flag stays the in-flight call's and is
// released when that call returns, so the retry the message asks for succeeds); the success path takes the flag and deletes the handle with it.
VITS_API void vits_free_model(vits_model* model) {
    if (!model) return;
    bool expected = false;
    if (!model->eng.busy.compare_exchange_strong(expected, true, std::memory_order_acquire)) {
        set_err("vits_free_model: model busy (a call is in progress on this handle); not freed — call again when it has returned");
        return;
    }
    try {
        delete model;
    } catch (...) {
    }
}

// reference: src/vits.cpp:1221-1223 (scalar delete on new[] there, Q12; both sides are ours here)
VITS_API void vits_free_result(vits_result result) { delete[] result.data; }

static vits_result process_ids_impl(vits_model* model, const int32_t* ids, size_t n) {
    vits_result r{nullptr, 0};
    if (!model || !ids || n == 0) {
        set_err(n == 0 ? "empty input (no known symbols in the text)" : "null argument");
        return r;
    }
    VITS_ENTER(model, r)
    const vits_process_opts o = default_opts(nullptr, VITS_NOISE_REFERENCE);
    vits_batch_result br;
    std::memset(&br, 0, sizeof(br));
    const int32_t len = (int32_t)n;
    if (run_engine(&br, [&](std::string& err) { return model->eng.process_batch(ids, &len, 1, (int)n, o, &br, err); }) != 0) return r;
    return take_row(br);
}

// reference: src/vits.cpp:1225-1232 -> vits_model::process :1101-1191
VITS_API vits_result vits_model_process(vits_model* model, const char* phonemes) {
    vits_result none{nullptr, 0};
    VITS_TRY
    if (!model || !phonemes) {
        set_err("null argument");
        return none;
    }
    std::vector<int32_t> ids;
    std::string terr;
    if (!model->eng.tok.tokenize_checked(phonemes, ids, terr)) {  // vits.cpp:1109 (a phonetic model: refused, see engine.h Tokenizer)
        set_err(terr);
        return none;
    }
    if (ids.empty() && !model->eng.tok.add_blank) {  // Q11: the reference's tokenizer returns no ids at all without add_blank
        set_err("empty input: the model file says add_blank = 0, for which the reference tokenizer returns no ids (vits_tokenizer.cpp:200-208); pass ids");
        return none;
    }
    return process_ids_impl(model, ids.data(), ids.size());
    VITS_CATCH(none)
}

VITS_API vits_result vits_model_process_ids(vits_model* model, const int32_t* ids, size_t n_ids) {
    vits_result none{nullptr, 0};
    VITS_TRY
    return process_ids_impl(model, ids, n_ids);
    VITS_CATCH(none)
}

VITS_API int vits_model_set_mode(vits_model* model, int mode) {
    if (!model || (mode != VITS_MODE_REFERENCE && mode != VITS_MODE_HF)) {
        set_err("bad mode");
        return -1;
    }
    VITS_ENTER(model, -1)
    model->eng.mode = mode;
    return 0;
}
VITS_API int vits_model_get_mode(const vits_model* model) { return model ? model->eng.mode : -1; }
VITS_API void vits_reference_noise_seed(uint32_t seed) { vits::reference_noise_seed(seed); }
VITS_API int vits_model_set_arith(vits_model* model, int arith) {
    VITS_TRY
    if (!model || (arith != VITS_ARITH_F32 && arith != VITS_ARITH_BF16 && arith != VITS_ARITH_F16 && arith != VITS_ARITH_F32_SPLIT)) {
        set_err("bad arithmetic mode");
        return -1;
    }
    VITS_ENTER_IDLE(model, -1)
    return run_engine(nullptr, [&](std::string& err) { return model->eng.set_arith(arith, err); });
    VITS_CATCH(-1)
}
VITS_API int vits_model_get_arith(const vits_model* model) { return model ? model->eng.arith : -1; }
VITS_API int vits_model_set_arith_scope(vits_model* model, int scope) {
    if (!model || (scope != VITS_ARITH_SCOPE_FLOW_VOCODER && scope != VITS_ARITH_SCOPE_ALL_CONVS)) {
        set_err("bad arithmetic scope");
        return -1;
    }
    VITS_ENTER_IDLE(model, -1)
    model->eng.arith_scope = scope;
    return 0;
}
VITS_API int vits_model_get_arith_scope(const vits_model* model) { return model ? model->eng.arith_scope : -1; }
VITS_API int vits_model_set_ggml_tables(vits_model* model, int on) {
    VITS_TRY
    if (!model) {
        set_err("null argument");
        return -1;
    }
    VITS_ENTER_IDLE(model, -1)
    return run_engine(nullptr, [&](std::string& err) { return model->eng.set_ggml_tables(on, err); });
    VITS_CATCH(-1)
}
VITS_API int vits_model_get_ggml_tables(const vits_model* model) { return model ? model->eng.ggml_tables : -1; }
VITS_API int vits_model_set_speaker(vits_model* model, int32_t speaker) {
    if (!model) {
        set_err("null argument");
        return -1;
    }
    VITS_ENTER(model, -1)
    std::string err;  // (file speakers + registered voices: the range rule of every speaker check)
    if (speaker != -1 && model->eng.check_speaker(speaker, "vits_model_set_speaker(" + std::to_string(speaker) + ")", err, ": outside [-1, ")) {
        set_err(err);
        return -1;
    }
    model->eng.speaker = speaker;
    return 0;
}
VITS_API int32_t vits_model_get_speaker(const vits_model* model) { return model ? model->eng.speaker : -2; }
VITS_API int32_t vits_model_num_speakers(const vits_model* model) { return model ? model->eng.num_speakers() : -1; }

// ---- custom voices (engine_voices.cpp) ----------------------------------------------------------------------------------------
VITS_API int32_t vits_model_speaker_embedding_size(const vits_model* model) {
    return model && model->eng.hp.num_speakers > 1 ? model->eng.hp.speaker_embedding_size : 0;
}
VITS_API int32_t vits_model_num_voices(const vits_model* model) { return model ? model->eng.num_voices() : 0; }
VITS_API int vits_model_get_speaker_embedding(vits_model* model, int32_t id, float* dst, size_t cap) {
    VITS_TRY
    if (!model || (!dst && cap)) {
        set_err("null argument");
        return -1;
    }
    VITS_ENTER(model, -1)
    std::string err;
    const int rc = model->eng.get_speaker_embedding(id, dst, cap, err);
    if (rc < 0) set_err(err);
    return rc;
    VITS_CATCH(-1)
}
// the three mutating calls: never with batches in flight (VITS_ENTER_IDLE: a growing table moves under the kernels that read it), never from inside a
// callback (VITS_ENTER: "model busy")
VITS_API int vits_model_add_voices(vits_model* model, const float* emb, int32_t n, int32_t* ids_out) {
    VITS_TRY
    if (!model || !emb || !ids_out) {
        set_err("null argument");
        return -1;
    }
    VITS_ENTER_IDLE(model, -1)
    return run_engine(nullptr, [&](std::string& err) { return model->eng.add_voices(emb, n, ids_out, err); });
    VITS_CATCH(-1)
}
VITS_API int vits_model_set_voice(vits_model* model, int32_t voice_id, const float* emb) {
    VITS_TRY
    if (!model || !emb) {
        set_err("null argument");
        return -1;
    }
    VITS_ENTER_IDLE(model, -1)
    return run_engine(nullptr, [&](std::string& err) { return model->eng.set_voice(voice_id, emb, err); });
    VITS_CATCH(-1)
}
VITS_API int vits_model_clear_voices(vits_model* model) {
    VITS_TRY
    if (!model) {
        set_err("null argument");
        return -1;
    }
    VITS_ENTER_IDLE(model, -1)
    return run_engine(nullptr, [&](std::string& err) { return model->eng.clear_voices(err); });
    VITS_CATCH(-1)
}

VITS_API int vits_model_set_prosody(vits_model* model, float speaking_rate, float noise_scale, float noise_scale_duration) {
    if (!model) {
        set_err("null argument");
        return -1;
    }
    VITS_ENTER(model, -1)
    return run_engine(nullptr, [&](std::string& err) { return model->eng.set_prosody(speaking_rate, noise_scale, noise_scale_duration, err); });
}
VITS_API int vits_model_get_prosody(const vits_model* model, float* speaking_rate, float* noise_scale, float* noise_scale_duration) {
    if (!model) {
        set_err("null argument");
        return -1;
    }
    if (speaking_rate) *speaking_rate = model->eng.speaking_rate;
    if (noise_scale) *noise_scale = model->eng.noise_scale;
    if (noise_scale_duration) *noise_scale_duration = model->eng.noise_scale_dur;
    return 0;
}

VITS_API int vits_model_process_batch(vits_model* model, const int32_t* ids, const int32_t* id_lengths, int32_t batch, int32_t id_stride,
                                      const vits_process_opts* opts, vits_batch_result* out) {
    VITS_TRY
    if (out) std::memset(out, 0, sizeof(*out));
    if (!model || !ids) {
        set_err("null argument");
        return -1;
    }
    VITS_ENTER(model, -1)
    const vits_process_opts o = default_opts(opts, VITS_NOISE_COUNTER);
    return run_engine(out, [&](std::string& err) { return model->eng.process_batch(ids, id_lengths, batch, id_stride, o, out, err); });
    VITS_CATCH(-1)
}

VITS_API int vits_model_prepare_conversion(vits_model* model) {
    VITS_TRY
    if (!model) {
        set_err("null argument");
        return -1;
    }
    VITS_ENTER(model, -1)
    return run_engine(nullptr, [&](std::string& err) { return model->eng.prepare_conversion(err); });
    VITS_CATCH(-1)
}

VITS_API int vits_model_convert_batch(vits_model* model, const float* pcm, const int64_t* pcm_lengths, int32_t batch, int64_t pcm_stride,
                                      const int32_t* src_speakers, const int32_t* tgt_speakers, const vits_process_opts* opts, vits_batch_result* out) {
    VITS_TRY
    if (out) std::memset(out, 0, sizeof(*out));
    if (!model || !pcm || !pcm_lengths) {
        set_err("null argument");
        return -1;
    }
    VITS_ENTER(model, -1)
    const vits_process_opts o = default_opts(opts, VITS_NOISE_COUNTER);
    return run_engine(out, [&](std::string& err) { return model->eng.convert_batch(pcm, pcm_lengths, batch, pcm_stride, src_speakers, tgt_speakers, o, out, err); });
    VITS_CATCH(-1)
}

VITS_API int vits_model_align_batch(vits_model* model, const float* pcm, const int64_t* pcm_lengths, int32_t batch, int64_t pcm_stride, const int32_t* ids,
                                    const int32_t* id_lengths, int32_t id_stride, const int32_t* speakers, float noise_scale, const vits_process_opts* opts,
                                    int32_t* durations, int64_t* frames, float* scores) {
    VITS_TRY
    if (!model || !pcm || !pcm_lengths || !ids || !durations) {
        set_err("null argument");
        return -1;
    }
    VITS_ENTER(model, -1)
    const vits_process_opts o = default_opts(opts, VITS_NOISE_COUNTER);
    return run_engine(nullptr, [&](std::string& err) {
        return model->eng.align_batch(pcm, pcm_lengths, batch, pcm_stride, ids, id_lengths, id_stride, speakers, noise_scale, o, durations, frames, scores, err);
    });
    VITS_CATCH(-1)
}

VITS_API int64_t vits_model_align(vits_model* model, const float* pcm, size_t n, const char* text, int32_t speaker, int32_t* ids, int32_t* durations, size_t cap) {
    VITS_TRY
    if (!model || !pcm || !text || n == 0 || (cap && (!ids || !durations))) {
        set_err(n == 0 && model && pcm && text ? "empty input (no samples)" : "null argument");
        return -1;
    }
    VITS_ENTER(model, -1)
    std::vector<int32_t> v;
    std::string err;
    if (!model->eng.tok.tokenize_checked(text, v, err)) {
        set_err(err);
        return -1;
    }
    if (v.empty()) {
        set_err("empty input (no ids)");
        return -1;
    }
    const vits_process_opts o = default_opts(nullptr, VITS_NOISE_COUNTER);  // (noise_scale 0: nothing is drawn)
    std::vector<int32_t> d(v.size(), 0);
    const int64_t len = (int64_t)n;
    if (run_engine(nullptr, [&](std::string& e) { return model->eng.align_batch(pcm, &len, 1, len, v.data(), nullptr, (int)v.size(), &speaker, 0.f, o, d.data(), nullptr, nullptr, e); }) != 0)
        return -1;
    for (size_t i = 0; i < v.size() && i < cap; ++i) {
        ids[i] = v[i];
        durations[i] = d[i];
    }
    return (int64_t)v.size();
    VITS_CATCH(-1)
}

VITS_API vits_result vits_model_convert(vits_model* model, const float* pcm, size_t n, int32_t src_speaker, int32_t tgt_speaker) {
    vits_result r{nullptr, 0};
    VITS_TRY
    if (!model || !pcm || n == 0) {
        set_err(n == 0 ? "empty input (no samples)" : "null argument");
        return r;
    }
    VITS_ENTER(model, r)
    const vits_process_opts o = default_opts(nullptr, VITS_NOISE_REFERENCE);
    vits_batch_result br;
    std::memset(&br, 0, sizeof(br));
    const int64_t len = (int64_t)n;
    if (run_engine(&br, [&](std::string& err) { return model->eng.convert_batch(pcm, &len, 1, len, &src_speaker, &tgt_speaker, o, &br, err); }) != 0) return r;
    return take_row(br);
    VITS_CATCH(r)
}

VITS_API int vits_model_submit_batch(vits_model* model, const int32_t* ids, const int32_t* id_lengths, int32_t batch, int32_t id_stride,
                                     const vits_process_opts* opts) {
    VITS_TRY
    if (!model || !ids) {
        set_err("null argument");
        return -1;
    }
    VITS_ENTER(model, -1)
    const vits_process_opts o = default_opts(opts, VITS_NOISE_COUNTER);
    return run_engine(nullptr, [&](std::string& err) { return model->eng.submit_batch(ids, id_lengths, batch, id_stride, o, err); });
    VITS_CATCH(-1)
}

VITS_API int vits_model_wait(vits_model* model, vits_batch_result* out) {
    VITS_TRY
    if (out) std::memset(out, 0, sizeof(*out));
    if (!model) {
        set_err("null argument");
        return -1;
    }
    VITS_ENTER(model, -1)
    return run_engine(out, [&](std::string& err) { return model->eng.wait_batch(out, err); });
    VITS_CATCH(-1)
}

VITS_API int vits_model_pending(const vits_model* model) { return model ? model->eng.pending() : -1; }

VITS_API void vits_free_batch_result(vits_batch_result* r) {
    if (!r) return;
    delete[] r->data;
    delete[] r->lengths;
    delete[] r->frames;
    std::memset(r, 0, sizeof(*r));
}

VITS_API int vits_model_sync(vits_model* model) {
    VITS_TRY
    if (!model) return -1;
    VITS_ENTER(model, -1)
    return run_engine(nullptr, [&](std::string& err) { return model->eng.sync(err); });
    VITS_CATCH(-1)
}

VITS_API int64_t vits_model_tokenize(vits_model* model, const char* text, int32_t* ids, size_t cap) {
    VITS_TRY
    if (!model || !text || (cap && !ids)) {
        set_err("null argument");
        return -1;
    }
    std::vector<int32_t> v;
    std::string terr;
    if (!model->eng.tok.tokenize_checked(text, v, terr)) {
        set_err(terr);
        return -1;
    }
    for (size_t i = 0; i < v.size() && i < cap; ++i) ids[i] = v[i];
    return (int64_t)v.size();
    VITS_CATCH(-1)
}

VITS_API int32_t vits_model_sampling_rate(const vits_model* model) { return model ? model->eng.hp.sampling_rate : 0; }
VITS_API int32_t vits_model_hop(const vits_model* model) {
    if (!model) return 0;
    int hop = 1;
    for (int r : model->eng.hp.up_rates) hop *= r;
    return hop;
}
// ---- any sample rate (include/vits.h: the filter and what the rates mean) ---------------------------------------------------------------
VITS_API int vits_model_set_rates(vits_model* model, int32_t input_rate, int32_t output_rate) {
    VITS_TRY
    if (!model) {
        set_err("null argument");
        return -1;
    }
    VITS_ENTER_IDLE(model, -1)
    return run_engine(nullptr, [&](std::string& err) { return model->eng.set_rates(input_rate, output_rate, err); });
    VITS_CATCH(-1)
}
VITS_API int vits_model_get_rates(const vits_model* model, int32_t* input_rate, int32_t* output_rate) {
    if (!model) {
        set_err("null argument");
        return -1;
    }
    if (input_rate) *input_rate = model->eng.input_rate();
    if (output_rate) *output_rate = model->eng.output_rate();
    return 0;
}
VITS_API int vits_resample_plan(int32_t in_rate, int32_t out_rate, int32_t* L, int32_t* M, int32_t* K) {
    VITS_TRY
    vits::ResamplePlan p;
    std::string err;
    if (!vits::resample_plan(in_rate, out_rate, p, err)) {
        set_err("vits_resample_plan: " + err);
        return -1;
    }
    if (L) *L = p.L;
    if (M) *M = p.M;
    if (K) *K = p.K;
    return 0;
    VITS_CATCH(-1)
}
VITS_API int64_t vits_resample_taps(int32_t in_rate, int32_t out_rate, float* dst, size_t cap) {
    VITS_TRY
    vits::ResamplePlan p;
    std::string err;
    if (!vits::resample_plan(in_rate, out_rate, p, err)) {
        set_err("vits_resample_taps: " + err);
        return -1;
    }
    const size_t n = (size_t)p.L * p.K;
    if (!dst && cap) {
        set_err("vits_resample_taps: null argument (dst is NULL with cap > 0)");
        return -1;
    }
    if (dst && cap >= n) {
        const std::vector<float> h = vits::resample_taps(p);
        std::memcpy(dst, h.data(), sizeof(float) * n);
    }
    return (int64_t)n;
    VITS_CATCH(-1)
}
VITS_API int64_t vits_resample_length(int32_t in_rate, int32_t out_rate, int64_t n) {
    VITS_TRY
    vits::ResamplePlan p;
    std::string err;
    if (!vits::resample_plan(in_rate, out_rate, p, err)) {
        set_err("vits_resample_length: " + err);
        return -1;
    }
    if (n < 0 || n > ((int64_t)1 << 40)) {
        set_err("vits_resample_length: n = " + std::to_string(n) + " is outside [0, 2^40]");
        return -1;
    }
    return p.out_len(n);
    VITS_CATCH(-1)
}
// ---- a stated level (include/vits.h: the definition and the kinds) -------------------------------------------------------------------
VITS_API int vits_model_set_level(vits_model* model, int32_t kind, float value_db, float ceiling_db) {
    VITS_TRY
    if (!model) {
        set_err("null argument");
        return -1;
    }
    VITS_ENTER_IDLE(model, -1)
    return run_engine(nullptr, [&](std::string& err) { return model->eng.set_level(kind, value_db, ceiling_db, err); });
    VITS_CATCH(-1)
}
VITS_API int vits_model_get_level(const vits_model* model, int32_t* kind, float* value_db, float* ceiling_db) {
    if (!model) {
        set_err("null argument");
        return -1;
    }
    if (kind) *kind = model->eng.level_kind();
    if (value_db) *value_db = model->eng.level_value_db();
    if (ceiling_db) *ceiling_db = model->eng.level_ceiling_db();
    return 0;
}
VITS_API int64_t vits_model_last_levels(vits_model* model, float* dst, size_t cap) {
    VITS_TRY
    if (!model || (!dst && cap)) {
        set_err("null argument");
        return -1;
    }
    VITS_ENTER(model, -1)
    int rows = 0;
    const float* p = model->eng.last_levels(rows);
    const size_t n = (size_t)4 * rows;
    if (n && dst && cap >= n) std::memcpy(dst, p, sizeof(float) * n);
    return (int64_t)n;
    VITS_CATCH(-1)
}
VITS_API int vits_loudness_plan(int32_t rate, double coef[10], int32_t* segment) {
    VITS_TRY
    vits::LoudnessPlan p;
    std::string err;
    if (!vits::loudness_plan(rate, p, err)) {
        set_err("vits_loudness_plan: " + err);
        return -1;
    }
    if (coef) std::memcpy(coef, p.coef.c, sizeof(double) * 10);
    if (segment) *segment = p.S;
    return 0;
    VITS_CATCH(-1)
}
VITS_API int vits_loudness_host(const float* pcm, size_t n, int32_t rate, double* lufs, double* peak, int32_t* blocks) {
    VITS_TRY
    vits::LoudnessPlan p;
    std::string err;
    if (!vits::loudness_plan(rate, p, err)) {
        set_err("vits_loudness_host: " + err);
        return -1;
    }
    if (!pcm && n) {
        set_err("vits_loudness_host: null argument (pcm is NULL with n > 0)");
        return -1;
    }
    int nb = 0;
    vits::loudness_host(pcm, n, p, lufs, peak, &nb);
    if (blocks) *blocks = nb;
    return 0;
    VITS_CATCH(-1)
}
// ---- the loudness target under a ceiling (include/vits.h: the definition) --------------------------------------------------------------
VITS_API int vits_model_set_limiter(vits_model* model, int32_t mode) {
    VITS_TRY
    if (!model) {
        set_err("null argument");
        return -1;
    }
    VITS_ENTER_IDLE(model, -1)
    return run_engine(nullptr, [&](std::string& err) { return model->eng.set_limiter(mode, err); });
    VITS_CATCH(-1)
}
VITS_API int vits_model_get_limiter(const vits_model* model, int32_t* mode) {
    if (!model) {
        set_err("null argument");
        return -1;
    }
    if (mode) *mode = model->eng.limiter_mode();
    return 0;
}
VITS_API int64_t vits_model_last_limits(vits_model* model, float* dst, size_t cap) {
    VITS_TRY
    if (!model || (!dst && cap)) {
        set_err("null argument");
        return -1;
    }
    VITS_ENTER(model, -1)
    int rows = 0;
    const float* p = model->eng.last_limits(rows);
    const size_t n = (size_t)4 * rows;
    if (n && dst && cap >= n) std::memcpy(dst, p, sizeof(float) * n);
    return (int64_t)n;
    VITS_CATCH(-1)
}
VITS_API int vits_limiter_plan(int32_t rate, int32_t* A, int32_t* H, int32_t* tile) {
    VITS_TRY
    vits::LimiterPlan p;
    std::string err;
    if (!vits::limiter_plan(rate, p, err)) {
        set_err("vits_limiter_plan: " + err);
        return -1;
    }
    if (A) *A = p.A;
    if (H) *H = p.H;
    if (tile) *tile = p.tile;
    return 0;
    VITS_CATCH(-1)
}
VITS_API int vits_limiter_host(const float* pcm, size_t n, int32_t rate, double g0, double ceiling_db, double* y, double limits[4]) {
    VITS_TRY
    vits::LimiterPlan p;
    std::string err;
    if (!vits::limiter_plan(rate, p, err)) {
        set_err("vits_limiter_host: " + err);
        return -1;
    }
    if (!pcm && n) {
        set_err("vits_limiter_host: null argument (pcm is NULL with n > 0)");
        return -1;
    }
    if (!(std::isfinite(g0) && g0 > 0.0) || !(std::isfinite(ceiling_db) && ceiling_db >= -60.0 && ceiling_db <= 0.0)) {
        set_err("vits_limiter_host: g0 must be finite and positive, ceiling_db in [-60, 0] dB");
        return -1;
    }
    const std::vector<float> h = vits::resample_taps(p.up);
    vits::limiter_host(pcm, n, p, h.data(), g0, std::pow(10.0, ceiling_db / 20.0), y, limits);
    return 0;
    VITS_CATCH(-1)
}
// ---- stated edges (include/vits.h: the definition) -----------------------------------------------------------------------------------------
VITS_API int vits_model_set_edges(vits_model* model, const vits_edges_desc* desc) {
    VITS_TRY
    if (!model) {
        set_err("null argument");
        return -1;
    }
    VITS_ENTER_IDLE(model, -1)
    return run_engine(nullptr, [&](std::string& err) { return model->eng.set_edges(desc, err); });
    VITS_CATCH(-1)
}
VITS_API int vits_model_get_edges(const vits_model* model, vits_edges_desc* desc) {
    if (!model) {
        set_err("null argument");
        return -1;
    }
    if (desc) *desc = model->eng.edges_desc();
    return 0;
}
VITS_API int64_t vits_model_last_edges(vits_model* model, int64_t* dst, size_t cap) {
    VITS_TRY
    if (!model || (!dst && cap)) {
        set_err("null argument");
        return -1;
    }
    VITS_ENTER(model, -1)
    int rows = 0;
    const int64_t* p = model->eng.last_edges(rows);
    const size_t n = (size_t)4 * rows;
    if (n && dst && cap >= n) std::memcpy(dst, p, sizeof(int64_t) * n);
    return (int64_t)n;
    VITS_CATCH(-1)
}
VITS_API int vits_edges_plan(int32_t rate, const vits_edges_desc* desc, int64_t out[8]) {
    VITS_TRY
    vits::EdgesPlan p;
    std::string err;
    if (!desc) {
        set_err("vits_edges_plan: null argument");
        return -1;
    }
    if (!vits::edges_plan(rate, *desc, p, err)) {
        set_err("vits_edges_plan: " + err);
        return -1;
    }
    if (out) {
        const int64_t v[8] = {p.W, p.Kh, p.Kt, p.Fi, p.Fo, p.Pl, p.Pt, p.tile};
        std::memcpy(out, v, sizeof(v));
    }
    return 0;
    VITS_CATCH(-1)
}
VITS_API int vits_edges_host(const float* pcm, size_t n, int32_t rate, const vits_edges_desc* desc, float* y, size_t y_cap, int64_t row[4]) {
    VITS_TRY
    vits::EdgesPlan p;
    std::string err;
    if (!desc || (!pcm && n)) {
        set_err("vits_edges_host: null argument (desc, or pcm with n > 0)");
        return -1;
    }
    if (!vits::edges_plan(rate, *desc, p, err)) {
        set_err("vits_edges_host: " + err);
        return -1;
    }
    if (p.mode == VITS_EDGES_OFF) {
        set_err("vits_edges_host: VITS_EDGES_OFF delivers the row as it is: there is nothing to evaluate");
        return -1;
    }
    if (n > (size_t)vits::kEdgesMaxLen) {
        set_err("vits_edges_host: the row is too long (" + std::to_string(n) + " samples)");
        return -1;
    }
    if (y && y_cap < (size_t)p.bound((int64_t)n)) {
        set_err("vits_edges_host: y_cap = " + std::to_string(y_cap) + " is below the row's bound n + Pl + Pt = " + std::to_string(p.bound((int64_t)n)));
        return -1;
    }
    const std::vector<float> fades = vits::edges_fades(p);
    vits::edges_host(pcm, (int64_t)n, p, fades.data(), y, row);
    return 0;
    VITS_CATCH(-1)
}
VITS_API int32_t vits_model_vocab_size(const vits_model* model) { return model ? model->eng.hp.vocab_size : 0; }
VITS_API int64_t vits_model_weight_bytes(const vits_model* model) { return model ? model->eng.weight_bytes : 0; }
VITS_API int32_t vits_model_duration_predictor_kind(const vits_model* model) { return model ? (model->eng.hp.stochastic_duration ? 0 : 1) : -1; }

VITS_API int64_t vits_model_get_tap(vits_model* model, const char* name, int32_t utt, float* dst, size_t cap) {
    VITS_TRY
    if (!model || !name) return 0;
    VITS_ENTER(model, 0)
    return model->eng.get_tap(name, utt, dst, cap);
    VITS_CATCH(0)
}

VITS_API int vits_synth_model_bytes(uint64_t seed, int32_t arch, char** bytes, size_t* size) {
    VITS_TRY
    if (!bytes || !size) return -1;
    vits::ModelFile f = vits::make_synthetic_model(seed, arch);
    std::vector<uint8_t> v = f.serialize();
    *bytes = new char[v.size()];
    std::memcpy(*bytes, v.data(), v.size());
    *size = v.size();
    return 0;
    VITS_CATCH(-1)
}
VITS_API void vits_free_bytes(char* bytes) { delete[] bytes; }

VITS_API int vits_model_file_reserialize(const char* in, size_t in_size, char** out, size_t* out_size) {
    VITS_TRY
    if (!in || !out || !out_size) return -1;
    vits::ModelFile f;
    std::string err;
    if (!f.parse(reinterpret_cast<const uint8_t*>(in), in_size, err)) {
        set_err(err);
        return -1;
    }
    std::vector<uint8_t> v = f.serialize();
    *out = new char[v.size()];
    std::memcpy(*out, v.data(), v.size());
    *out_size = v.size();
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_model_file_validate(const char* bytes, size_t size) {
    VITS_TRY
    if (!bytes) {
        set_err("null argument");
        return -1;
    }
    vits::Engine e;
    std::string err;
    if (!e.validate(reinterpret_cast<const uint8_t*>(bytes), size, err)) {
        set_err(err);
        return -1;
    }
    return 0;
    VITS_CATCH(-1)
}

VITS_API int64_t vits_model_file_tokenize(const char* model_bytes, size_t size, const char* text, int32_t* ids, size_t cap) {
    VITS_TRY
    if (!model_bytes || !text) return -1;
    vits::ModelFile f;
    std::string err;
    if (!f.parse(reinterpret_cast<const uint8_t*>(model_bytes), size, err)) {
        set_err(err);
        return -1;
    }
    if (cap && !ids) {
        set_err("null argument");
        return -1;
    }
    vits::Tokenizer t;
    t.init(f);
    std::vector<int32_t> v;
    if (!t.tokenize_checked(text, v, err)) {
        set_err(err);
        return -1;
    }
    for (size_t i = 0; i < v.size() && i < cap; ++i) ids[i] = v[i];
    return (int64_t)v.size();
    VITS_CATCH(-1)
}

VITS_API int vits_prof_enable(vits_model* model, int32_t on) {
    if (!model) return -1;
    VITS_ENTER_IDLE(model, -1)
    model->eng.prof.on = on != 0;
    return 0;
}
VITS_API int vits_prof_reset(vits_model* model) {
    if (!model) return -1;
    VITS_ENTER(model, -1)
    hipStreamSynchronize(model->eng.stream);
    model->eng.prof.reset();
    return 0;
}
VITS_API int64_t vits_prof_report(vits_model* model, char* buf, size_t cap) {
    VITS_TRY
    if (!model || !buf || !cap) return -1;
    VITS_ENTER(model, -1)
    hipStreamSynchronize(model->eng.stream);
    std::string s = model->eng.prof.report();
    const size_t n = std::min(cap - 1, s.size());
    std::memcpy(buf, s.data(), n);
    buf[n] = 0;
    return (int64_t)s.size();
    VITS_CATCH(-1)
}

// reference: test/main.cpp:31-33 (static_cast<short>(clamp(x, -1, 1) * 32767))
VITS_API void vits_pcm16_from_float(const float* pcm, size_t n, int16_t* out) {
    for (size_t i = 0; i < n; ++i) out[i] = static_cast<int16_t>(std::max(-1.0f, std::min(1.0f, pcm[i])) * 32767);
}

VITS_API int vits_pcm16_from_float_device(const float* src, int64_t src_stride, int16_t* dst, int64_t dst_stride, const int64_t* lengths, int32_t rows,
                                          int64_t cols, void* hip_stream) {
    VITS_TRY
    if ((!src || !dst) && rows > 0 && cols > 0) {
        set_err("null argument");
        return -1;
    }
    const hipError_t e = vits::launch_pcm16(src, src_stride, dst, dst_stride, lengths, rows, cols, (hipStream_t)hip_stream);
    if (e != hipSuccess) {
        set_err(std::string("pcm16 kernel launch failed: ") + hipGetErrorString(e));
        return -1;
    }
    return 0;
    VITS_CATCH(-1)
}

// reference: test/main.cpp:23-63 (struct WAVHeader + write_wav)
VITS_API int vits_write_wav16(const char* path, const float* pcm, size_t n, int32_t sample_rate) {
    VITS_TRY
    if (!path || (!pcm && n)) return -1;
    std::vector<int16_t> s(n);
    vits_pcm16_from_float(pcm, n, s.data());
    const int32_t channels = 1, bits = 16;
    const int32_t data_bytes = (int32_t)(n * 2);
    unsigned char h[44];
    auto put32 = [&](int off, int32_t v) { std::memcpy(h + off, &v, 4); };
    auto put16 = [&](int off, int16_t v) { std::memcpy(h + off, &v, 2); };
    std::memcpy(h, "RIFF", 4);
    put32(4, 4 + (8 + 16) + (8 + data_bytes));
    std::memcpy(h + 8, "WAVE", 4);
    std::memcpy(h + 12, "fmt ", 4);
    put32(16, 16);
    put16(20, 1);
    put16(22, (int16_t)channels);
    put32(24, sample_rate);
    put32(28, sample_rate * channels * (bits / 8));
    put16(32, (int16_t)(channels * (bits / 8)));
    put16(34, (int16_t)bits);
    std::memcpy(h + 36, "data", 4);
    put32(40, data_bytes);
    std::ofstream f(path, std::ios::binary);
    if (!f.is_open()) {
        set_err(std::string("cannot open ") + path);
        return -1;
    }
    f.write(reinterpret_cast<const char*>(h), 44);
    f.write(reinterpret_cast<const char*>(s.data()), data_bytes);
    return f.good() ? 0 : -1;
    VITS_CATCH(-1)
}

VITS_API int vits_set_device(int32_t device) {
    if (hipSetDevice(device) != hipSuccess) {
        set_err("hipSetDevice failed");
        return -1;
    }
    return 0;
}

VITS_API int vits_device_info(char* name, size_t cap, int32_t* cu_count, int32_t* clock_mhz, int64_t* hbm_bytes) {
    VITS_TRY
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        set_err("no HIP device");
        return -1;
    }
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, dev) != hipSuccess) {
        set_err("hipGetDeviceProperties failed");
        return -1;
    }
    if (name && cap) {
        std::snprintf(name, cap, "%s (%s)", p.name, p.gcnArchName);
    }
    if (cu_count) *cu_count = p.multiProcessorCount;
    if (clock_mhz) *clock_mhz = p.clockRate / 1000;
    if (hbm_bytes) *hbm_bytes = (int64_t)p.totalGlobalMem;
    return 0;
    VITS_CATCH(-1)
}

// ---- operator-level entry points: host in, host out ---------------------------------------------------------
namespace {
struct DevBuf {
    float* p = nullptr;
    ~DevBuf() {
        if (p) hipFree(p);
    }
    bool put(const float* h, size_t n) {
        if (hipMalloc((void**)&p, std::max<size_t>(n, 1) * 4) != hipSuccess) return false;
        if (h) return hipMemcpy(p, h, n * 4, hipMemcpyHostToDevice) == hipSuccess;
        return hipMemset(p, 0, n * 4) == hipSuccess;
    }
};
struct DevInts {
    int* p = nullptr;
    ~DevInts() {
        if (p) hipFree(p);
    }
    bool put(const int32_t* h, size_t n) {
        if (!h) return true;
        if (hipMalloc((void**)&p, n * 4) != hipSuccess) return false;
        return hipMemcpy(p, h, n * 4, hipMemcpyHostToDevice) == hipSuccess;
    }
};
vits::TensorRef tref(float* p, int channels, int stride) {
    vits::TensorRef t;
    t.p = p;
    t.cs = stride;
    t.bs = (int64_t)channels * stride;
    return t;
}
int fail(const char* what) {
    set_err(what);
    return -1;
}
thread_local int g_op_arith = VITS_ARITH_F32;
// one operator-level conv in the selected arithmetic: the fp32 MFMA kernel, or (16-bit modes) the converter + conv16 pair the
// engine uses for fp32-layout tensors
hipError_t run_op_conv(vits::PackedConv& pc, const vits::ConvCall& c, const float* w_torch, int k, DevBuf& w16, DevBuf& x16) {
    using namespace vits;
    if (g_op_arith == VITS_ARITH_F32) return launch_conv(pc, c, nullptr);
    const std::vector<uint16_t> packed = pack_conv_weights16(w_torch, pc.cout, pc.cin, k, pc.epi, pc.ct_stride, g_op_arith);
    if (!w16.put(nullptr, packed.size() / 2 + 1)) return hipErrorOutOfMemory;
    if (hipMemcpy(w16.p, packed.data(), packed.size() * 2, hipMemcpyHostToDevice) != hipSuccess) return hipErrorUnknown;
    pc.wp16 = reinterpret_cast<uint16_t*>(w16.p);
    Ref16 r;
    r.ts = (c.t_in + 7) / 8 * 8;
    r.bs = (int64_t)((pc.cin + 7) / 8) * r.ts * 8;
    if (!x16.put(nullptr, (size_t)c.batch * r.bs / 2 + 1)) return hipErrorOutOfMemory;
    r.p = reinterpret_cast<uint16_t*>(x16.p);
    hipError_t e = launch_to_group16(c.x, c.len_in, c.batch, pc.cin, c.t_in, c.pre_act ? c.slope : 1.0f, r, g_op_arith, nullptr);
    if (e != hipSuccess) return e;
    Conv16Call q;
    q.x = r;
    q.len_in = c.len_in;
    q.len_out = c.len_out;
    q.batch = c.batch;
    q.t_in = c.t_in;
    q.t_out = c.t_out;
    q.dil = c.dil;
    q.pad_l = c.pad_l;
    q.post_act = c.post_act;
    q.post_slope = c.post_slope;
    q.scale = c.scale;
    q.scale_div = c.scale_div;
    q.ct_crop = c.ct_crop;
    q.y = c.y;
    q.res = c.res;
    q.acc = c.acc;
    q.tile = c.tile;
    return launch_conv16(pc, q, g_op_arith, nullptr);
}

// ---- VITS_ARITH_F32_SPLIT at operator level: the engine's own sequence (pack_conv_weights_split, launch_split_planes, launch_conv_split) or a refusal
// that names its cause — never another kernel, so that a test cannot believe the split kernels ran when they did not.
struct DevU16 {
    uint16_t* p = nullptr;
    ~DevU16() {
        if (p) hipFree(p);
    }
    bool fill(size_t n, int byte) { return hipMalloc((void**)&p, std::max<size_t>(n, 1) * 2) == hipSuccess && hipMemset(p, byte, n * 2) == hipSuccess; }
    bool put(const std::vector<uint16_t>& h) { return hipMalloc((void**)&p, std::max<size_t>(h.size(), 1) * 2) == hipSuccess && hipMemcpy(p, h.data(), h.size() * 2, hipMemcpyHostToDevice) == hipSuccess; }
};
// three-plane activation buffer [batch][3][channels / 8][ts][8], every byte 0xFF (bf16 NaN): a slot the writer skips (t >= len[b]) and a conv reads shows in the result
bool split3_nan(DevU16& d, int batch, int channels, int ts, vits::Split3Ref* r) {
    if (!d.fill((size_t)batch * 3 * channels * ts, 0xFF)) return false;
    r->p = d.p;
    r->ts = ts;
    r->ps = (int64_t)channels * ts;
    r->bs = 3 * r->ps;
    return true;
}
// why the split kernels do not take a conv (conv_plan.cpp conv_split_candidate / conv_split_supported), or "" if they do
std::string split_refusal(int cin, int cout, int k, int dil) {
    char m[200] = "";
    if (cin < 128 || (cin & 31)) std::snprintf(m, sizeof(m), "VITS_ARITH_F32_SPLIT: c_in = %d is not taken by the split kernels (a multiple of 32, at least 128)", cin);
    else if (cout < 128 || (cout & 127)) std::snprintf(m, sizeof(m), "VITS_ARITH_F32_SPLIT: c_out = %d is not taken by the split kernels (a multiple of 128)", cout);
    else if (k != 3 && k != 7 && k != 11) std::snprintf(m, sizeof(m), "VITS_ARITH_F32_SPLIT: k = %d taps are not taken by the split kernels (3, 7 or 11)", k);
    else if (dil != 1 && dil != 3 && dil != 5) std::snprintf(m, sizeof(m), "VITS_ARITH_F32_SPLIT: dilation %d is not taken by the split kernels (1, 3 or 5)", dil);
    return m;
}
// the split weight planes and the bias of one conv on the device; `why` names the cause when the split kernels do not take it
bool split_conv_upload(const float* w, const float* bias, int cout, int cin, int k, int dil, vits::PackedConv& pc, DevU16& dw, DevBuf& db, std::string& why) {
    using namespace vits;
    why = split_refusal(cin, cout, k, dil);
    if (!why.empty()) return false;
    std::vector<uint16_t> packed;
    if (!pack_conv_weights_split(w, cout, cin, k, packed)) {
        why = "VITS_ARITH_F32_SPLIT: a weight is not the exact sum of two bf16 values (the split kernels take fp16- or bf16-valued weights)";
        return false;
    }
    if (!dw.put(packed) || (bias && !db.put(bias, cout))) {
        why = "device allocation failed";
        return false;
    }
    pc.cin = cin;
    pc.cout = cout;
    pc.kt = k;
    pc.epi = EPI_STD;
    pc.nchunks = (cin + 31) / 32;
    pc.wps = dw.p;
    pc.bytes_s = (int64_t)packed.size() * 2;
    pc.bias = db.p;
    if (!conv_split_supported(pc, dil)) {
        why = "VITS_ARITH_F32_SPLIT: conv_split_supported refuses this conv";
        return false;
    }
    return true;
}
bool split_lens_ok(const int32_t* lens, int batch, int t, int t_stride) {
    if (batch < 1 || t < 1 || t_stride < t) return false;
    for (int b = 0; lens && b < batch; ++b)
        if (lens[b] < 0 || lens[b] > t) return false;
    return true;
}
int op_conv1d_split(const vits_conv1d_desc* d, const float* x, const float* w, const float* bias, const float* residual, const float* accum, const int32_t* lens, float* y) {
    using namespace vits;
    if (d->post_act != 0) return fail("VITS_ARITH_F32_SPLIT: post_act (relu / gate) does not exist on the split kernels");
    if (!split_lens_ok(lens, d->batch, d->t, d->t_stride)) return fail("VITS_ARITH_F32_SPLIT: 0 <= lens[b] <= t <= t_stride is required");
    PackedConv pc;
    DevU16 dw, dxs;
    DevBuf db, dx, dy, dr, da;
    DevInts dl;
    std::string why;
    if (!split_conv_upload(w, bias, d->cout, d->cin, d->k, d->dilation, pc, dw, db, why)) return fail(why.c_str());
    const size_t nx = (size_t)d->batch * d->cin * d->t_stride, ny = (size_t)d->batch * d->cout * d->t_stride;
    Split3Ref xs;
    if (!dx.put(x, nx) || !dy.put(nullptr, ny) || !dl.put(lens, d->batch) || !split3_nan(dxs, d->batch, d->cin, d->t_stride, &xs)) return fail("device allocation failed");
    if (residual && !dr.put(residual, ny)) return fail("device allocation failed");
    if (accum && !da.put(accum, ny)) return fail("device allocation failed");
    hipError_t e = launch_split_planes(tref(dx.p, d->cin, d->t_stride), d->cin, dl.p, d->batch, d->t, d->pre_act ? d->pre_slope : 1.0f, xs, nullptr);
    if (e == hipSuccess) {
        ConvCall c;
        c.xs3 = xs;
        c.y = tref(dy.p, d->cout, d->t_stride);
        if (residual) c.res = tref(dr.p, d->cout, d->t_stride);
        if (accum) c.acc = tref(da.p, d->cout, d->t_stride);
        c.len_in = c.len_out = dl.p;
        c.batch = d->batch;
        c.t_in = c.t_out = d->t;
        c.dil = d->dilation;
        c.pad_l = d->pad_left;
        c.scale = d->out_scale;
        e = launch_conv_split(pc, c, nullptr);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(hipGetErrorString(e));
    if (hipMemcpy(y, dy.p, ny * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail("copy back failed");
    return 0;
}
}  // namespace

VITS_API int vits_op_set_arith(int32_t arith) {
    if (arith != VITS_ARITH_F32 && arith != VITS_ARITH_BF16 && arith != VITS_ARITH_F16 && arith != VITS_ARITH_F32_SPLIT) return fail("bad arithmetic mode");
    g_op_arith = arith;
    return 0;
}

VITS_API int vits_op_conv1d(const vits_conv1d_desc* d, const float* x, const float* w, const float* bias, const float* residual, const float* accum,
                            const int32_t* lens, float* y) {
    VITS_TRY
    using namespace vits;
    if (!d || !x || !w || !y) return fail("null argument");
    if (g_op_arith == VITS_ARITH_F32_SPLIT) return op_conv1d_split(d, x, w, bias, residual, accum, lens, y);
    const int gate = d->post_act == 2;
    const int cy = gate ? d->cout / 2 : d->cout;
    PackedConv pc;
    pc.cin = d->cin;
    pc.cout = d->cout;
    pc.kt = d->k;
    pc.epi = gate ? EPI_GATE : EPI_STD;
    std::vector<float> packed = pack_conv_weights(w, d->cout, d->cin, d->k, pc.epi, 0, &pc.rows, &pc.mtiles_used, &pc.mtiles, &pc.nchunks);
    DevBuf dw, dwl, db, dx, dy, dr, da;
    DevInts dl;
    const size_t nx = (size_t)d->batch * d->cin * d->t_stride, ny = (size_t)d->batch * cy * d->t_stride;
    if (conv_lat16_candidate(pc.epi, d->k, d->cin)) {
        const std::vector<float> pl = repack_conv_weights_l16(packed, pc.mtiles, pc.nchunks, d->k);
        if (!dwl.put(pl.data(), pl.size())) return fail("device allocation failed");
        pc.wp_l16 = dwl.p;
    }
    if (!dw.put(packed.data(), packed.size()) || !dx.put(x, nx) || !dy.put(nullptr, ny) || !dl.put(lens, d->batch)) return fail("device allocation failed");
    if (bias && !db.put(bias, d->cout)) return fail("device allocation failed");
    if (residual && !dr.put(residual, ny)) return fail("device allocation failed");
    if (accum && !da.put(accum, ny)) return fail("device allocation failed");
    pc.wp = dw.p;
    pc.bias = db.p;
    ConvCall c;
    c.x = tref(dx.p, d->cin, d->t_stride);
    c.y = tref(dy.p, cy, d->t_stride);
    if (residual) c.res = tref(dr.p, cy, d->t_stride);
    if (accum) c.acc = tref(da.p, cy, d->t_stride);
    c.len_in = dl.p;
    c.len_out = dl.p;
    c.batch = d->batch;
    c.t_in = c.t_out = d->t;
    c.dil = d->dilation;
    c.pad_l = d->pad_left;
    c.pre_act = d->pre_act;
    c.slope = d->pre_slope;
    c.post_act = d->post_act == 1 ? 1 : 0;
    c.scale = d->out_scale;
    DevBuf w16, x16;
    hipError_t e = run_op_conv(pc, c, w, d->k, w16, x16);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(hipGetErrorString(e));
    if (hipMemcpy(y, dy.p, ny * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail("copy back failed");
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_op_resblock_pair(const vits_resblock_pair_desc* d, const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                                   const int32_t* lens, float* y) {
    VITS_TRY
    using namespace vits;
    if (!d || !x || !w1 || !w2 || !y) return fail("null argument");
    if (g_op_arith != VITS_ARITH_F32 && g_op_arith != VITS_ARITH_F32_SPLIT) return fail("vits_op_resblock_pair: VITS_ARITH_F32 or VITS_ARITH_F32_SPLIT only");
    if (!split_lens_ok(lens, d->batch, d->t, d->t_stride)) return fail("vits_op_resblock_pair: 0 <= lens[b] <= t <= t_stride is required");
    if (d->channels < 1 || d->k < 1 || !(d->k & 1) || d->dilation < 1) return fail("vits_op_resblock_pair: an odd tap count and a dilation >= 1 are required");
    const int C = d->channels, k = d->k;
    const size_t n = (size_t)d->batch * C * d->t_stride;
    DevBuf dx, dy, db1, db2;
    DevInts dl;
    if (!dx.put(x, n) || !dy.put(nullptr, n) || !dl.put(lens, d->batch)) return fail("device allocation failed");
    const TensorRef bx = tref(dx.p, C, d->t_stride), by = tref(dy.p, C, d->t_stride);
    // conv 1 / conv 2 of a pair as engine_vocoder.cpp builds them (mk_c1 / mk_c2)
    ConvCall c1, c2;
    c1.len_in = c1.len_out = dl.p;
    c1.batch = d->batch;
    c1.t_in = c1.t_out = d->t;
    c1.dil = d->dilation;
    c1.pad_l = (k * d->dilation - d->dilation) / 2;
    c2 = c1;
    c2.dil = 1;
    c2.pad_l = (k - 1) / 2;
    c2.res = bx;
    c2.y = by;
    PackedConv p1, p2;
    hipError_t e;
    DevU16 ws1, ws2, du, dt;
    DevBuf dw1, dw2, dwl1, dwl2, bt;
    if (g_op_arith == VITS_ARITH_F32_SPLIT) {
        std::string why;
        if (!split_conv_upload(w1, b1, C, C, k, d->dilation, p1, ws1, db1, why) || !split_conv_upload(w2, b2, C, C, k, 1, p2, ws2, db2, why)) return fail(why.c_str());
        Split3Ref su, st;
        if (!split3_nan(du, d->batch, C, d->t_stride, &su) || !split3_nan(dt, d->batch, C, d->t_stride, &st)) return fail("device allocation failed");
        // the un-fused split resblock: planes of leaky_relu(x); conv 1 writes ONLY the planes of leaky_relu(t); conv 2 reads them, res = x
        c1.xs3 = su;
        c1.ys3 = st;
        c1.ys3_slope = d->slope;
        c2.xs3 = st;
        e = launch_split_planes(bx, C, dl.p, d->batch, d->t, d->slope, su, nullptr);
        if (e == hipSuccess) e = launch_conv_split(p1, c1, nullptr);
        if (e == hipSuccess) e = launch_conv_split(p2, c2, nullptr);
    } else {
        auto upload = [&](const float* w, const float* b, PackedConv& pc, DevBuf& dw, DevBuf& dwl, DevBuf& db) {
            pc.cin = pc.cout = C;
            pc.kt = k;
            pc.epi = EPI_STD;
            const std::vector<float> packed = pack_conv_weights(w, C, C, k, EPI_STD, 0, &pc.rows, &pc.mtiles_used, &pc.mtiles, &pc.nchunks);
            if (conv_lat16_candidate(EPI_STD, k, C)) {
                const std::vector<float> pl = repack_conv_weights_l16(packed, pc.mtiles, pc.nchunks, k);
                if (!dwl.put(pl.data(), pl.size())) return false;
                pc.wp_l16 = dwl.p;
            }
            if (!dw.put(packed.data(), packed.size()) || (b && !db.put(b, C))) return false;
            pc.wp = dw.p;
            pc.bias = db.p;
            return true;
        };
        if (!upload(w1, b1, p1, dw1, dwl1, db1) || !upload(w2, b2, p2, dw2, dwl2, db2) || !bt.put(nullptr, n)) return fail("device allocation failed");
        c1.x = bx;
        c1.y = tref(bt.p, C, d->t_stride);
        c1.pre_act = 1;
        c1.slope = d->slope;
        c1.post_act = 2;  // t is stored activated: its only reader is conv 2
        c1.post_slope = d->slope;
        c2.x = c1.y;
        e = launch_conv(p1, c1, nullptr);
        if (e == hipSuccess) e = launch_conv(p2, c2, nullptr);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(hipGetErrorString(e));
    if (hipMemcpy(y, dy.p, n * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail("copy back failed");
    return 0;
    VITS_CATCH(-1)
}

// ---- vits_op_resblock: which kernel a descriptor names (host arithmetic only: launch_plan.h), then the engine's call structs on staged tensors ------------
namespace {
struct RbOpPlan {
    int variant = 0;
    std::string kernel;
    int bo = 0, adv = 0, halo = 0, seg = 0, tiles = 1, nr = 0, launches = 0;
    vits::LaunchGrid g;
};
bool rb_fail(std::string& why, const std::string& m) {
    why = "vits_op_resblock: " + m;
    return false;
}
bool resblock_resolve(const vits_resblock_desc* d, int arith, RbOpPlan& r, std::string& why) {
    using namespace vits;
    if (arith != VITS_ARITH_F32 && arith != VITS_ARITH_F16 && arith != VITS_ARITH_BF16)
        return rb_fail(why, "VITS_ARITH_F32, VITS_ARITH_F16 or VITS_ARITH_BF16 only (the split arithmetic keeps vits_op_resblock_pair)");
    const int C = d->channels, k = d->k, B = d->batch, T = d->t, nd = d->ndil;
    if (B < 1 || T < 1 || d->t_stride < T) return rb_fail(why, "batch >= 1 and 1 <= t <= t_stride are required");
    if (C < 32 || (C & 31)) return rb_fail(why, "channels = " + std::to_string(C) + ": a multiple of 32 is required");
    if (k < 1 || !(k & 1)) return rb_fail(why, "k = " + std::to_string(k) + ": an odd tap count is required");
    if (nd < 1 || nd > 3) return rb_fail(why, "ndil = " + std::to_string(nd) + ": one to three conv pairs");
    for (int p = 0; p < nd; ++p)
        if (d->dil[p] < 1) return rb_fail(why, "dilation " + std::to_string(d->dil[p]) + ": >= 1 is required");
    if (d->variant < 0 || d->variant > 4) return rb_fail(why, "variant " + std::to_string(d->variant) + ": 0 (the engine's choice), 1 (un-fused), 2 (fused pairs), 3 (whole ResBlock), 4 (segments of tiles)");
    const bool f32 = arith == VITS_ARITH_F32, bf = arith == VITS_ARITH_BF16;
    const bool d135 = nd == 3 && d->dil[0] == 1 && d->dil[1] == 3 && d->dil[2] == 5;
    const std::string shape = "C = " + std::to_string(C) + ", k = " + std::to_string(k);
    char name[96];
    int v = d->variant;
    if (v == 0) {  // engine_vocoder.cpp's order: the whole-ResBlock kernel, fused pairs (all pairs or none), two launches per pair
        if (f32) {
            bool pairs = true;
            for (int p = 0; p < nd; ++p) pairs = pairs && rbpair32_supported(C, k, d->dil[p]);
            v = pairs && rbblock32_supported(C, k, d->dil, nd) ? 3 : pairs ? 2 : 1;
        } else if (rbblock16_supported(C, k, d->dil, nd, B, T)) {
            v = plan_rbblock16(C, k, B, T).nt > 1 ? 4 : 3;
        } else {
            bool pairs = true, lat = C >= 128;
            for (int p = 0; p < nd; ++p) pairs = pairs && rbpair16_supported(C, k, d->dil[p]), lat = lat && conv16_lat_shape_ok(C, k, d->dil[p], B, T);
            v = pairs && !lat ? 2 : 1;
        }
    }
    r.variant = v;
    if (v == 1) {
        r.kernel = f32 ? "launch_conv" : "launch_conv16";
        r.launches = 2 * nd;
        return true;
    }
    if (v == 2) {
        if (d->nr != 0 && (f32 || C < 128)) return rb_fail(why, "nr = " + std::to_string(d->nr) + ": only the 16-bit pairs at C >= 128 have a choice of column tiles");
        for (int p = 0; p < nd; ++p) {
            const int dil = d->dil[p];
            LaunchGrid g;
            int nr = 0;
            if (f32) {
                if (!rbpair32_exists(k, dil, C)) return rb_fail(why, "variant 2: no rbpair32_kernel for " + shape + ", dilation " + std::to_string(dil) + " (k in {3, 7, 11}, dilation in {1, 3, 5}, C = 32, 64, or 128 with k = 3)");
                g = plan_rbpair32(C, k, dil, B, T);
                if (!g.ok) return rb_fail(why, "variant 2: plan_rbpair32 refuses " + shape + " (VITS_FUSE32_C128=0)");
            } else {
                const RbPair16Plan pl = d->nr ? plan_rbpair16(C, k, dil, B, T, d->nr) : plan_rbpair16(C, k, dil, B, T);
                if (!pl.ok) return rb_fail(why, "variant 2: no rbpair16_kernel for " + shape + ", dilation " + std::to_string(dil) + ", nr = " + std::to_string(d->nr) + " (k in {3, 7, 11}, dilation in {1, 3, 5}, C in {32, 64, 128, 256}, nr 4 or " + std::to_string(VITS_RB16_NARROW_NR) + " at C >= 128)");
                g = pl, nr = pl.nr;
            }
            if (p > 0) continue;  // the plan query describes the first pair; every pair is checked
            r.g = g, r.nr = nr;
            if (f32) {
                const RbPair32Geom ge = rbpair32_geom(k, dil, C);
                r.bo = ge.bo;
                std::snprintf(name, sizeof(name), "rbpair32_kernel<%d, %d, %d>", k, dil, C);
            } else {
                const RbPair16Geom ge = rbpair16_geom(k, dil, C, nr);
                r.bo = ge.bo;
                std::snprintf(name, sizeof(name), "rbpair16_kernel<%d, %d, %d, %d, %s, %s>", k, dil, C, nr, bf ? "true" : "false", ge.rows ? "true" : "false");
            }
            r.adv = r.seg = r.bo;
            r.halo = (k - 1) / 2 * (1 + dil);
            r.kernel = name;
        }
        r.launches = nd;
        return true;
    }
    // variants 3 and 4: the whole-ResBlock kernels
    if (!d135) return rb_fail(why, "variant " + std::to_string(v) + ": the whole-ResBlock kernels take three pairs with dilations 1, 3, 5");
    if (v == 4 && f32) return rb_fail(why, "variant 4: segments of tiles exist in the 16-bit modes only (rbblock32_kernel is one tile per block)");
    if (d->variant == 4 && d->tiles < 2) return rb_fail(why, "variant 4: tiles = " + std::to_string(d->tiles) + ", at least 2 are required");
    if (f32) {
        const RbBlock32Plan pl = plan_rbblock32(C, k, B, T);
        if (!pl.ok) return rb_fail(why, "variant 3: no rbblock32_kernel for " + shape + " (k = 3, C = 32 or 64)");
        const RbBlock32Geom ge = rbblock32_geom(C, pl.nr);
        r.g = pl, r.nr = pl.nr, r.bo = r.adv = r.seg = ge.bo, r.halo = ge.h;
        std::snprintf(name, sizeof(name), "rbblock32_kernel<%d, %d>", C, pl.nr);
    } else {
        const int nt = d->variant == 0 ? plan_rbblock16(C, k, B, T).nt : v == 4 ? d->tiles : 1;
        const RbBlock16Plan pl = plan_rbblock16(C, k, B, T, false, nt);
        if (!pl.ok) return rb_fail(why, "variant " + std::to_string(v) + ": no rbblock16_kernel for " + shape + " (k in {3, 7, 11} at C = 32 or 64, k = 3 at C = 128)");
        const RbBlock16Geom ge = rbblock16_geom(k, C);
        r.g = pl, r.tiles = nt, r.bo = ge.bo, r.adv = nt > 1 ? ge.adv : ge.bo, r.seg = ge.seg_out(nt), r.halo = ge.h;
        std::snprintf(name, sizeof(name), "rbblock16_kernel<%d, %d, %d, %d, %d, 1, 3, 5, %s, %s>", k, C, pl.tile.nstrip, pl.tile.nrw, pl.tile.mrw, bf ? "true" : "false", nt > 1 ? "true" : "false");
    }
    r.kernel = name;
    r.launches = 1;
    return true;
}
// device memory with every byte `byte` (0xFF: fp32, f16 and bf16 NaNs alike)
struct DevBytes {
    void* p = nullptr;
    ~DevBytes() {
        if (p) hipFree(p);
    }
    bool fill(size_t bytes, int byte) { return hipMalloc(&p, std::max<size_t>(bytes, 16)) == hipSuccess && hipMemset(p, byte, std::max<size_t>(bytes, 16)) == hipSuccess; }
    bool put(const void* h, size_t bytes) { return hipMalloc(&p, std::max<size_t>(bytes, 16)) == hipSuccess && hipMemcpy(p, h, bytes, hipMemcpyHostToDevice) == hipSuccess; }
    float* f() const { return static_cast<float*>(p); }
    uint16_t* h() const { return static_cast<uint16_t*>(p); }
};
}  // namespace

VITS_API int vits_op_resblock_plan(const vits_resblock_desc* d, vits_resblock_plan* out) {
    VITS_TRY
    if (!d || !out) return fail("vits_op_resblock_plan: null argument");
    RbOpPlan r;
    std::string why;
    if (!resblock_resolve(d, g_op_arith, r, why)) return fail(why.c_str());
    std::memset(out, 0, sizeof(*out));
    std::snprintf(out->kernel, sizeof(out->kernel), "%s", r.kernel.c_str());
    out->variant = r.variant, out->bo = r.bo, out->advance = r.adv, out->halo = r.halo, out->segment = r.seg, out->tiles = r.tiles, out->nr = r.nr;
    out->grid_x = r.g.gx, out->grid_y = r.g.gy, out->grid_z = r.g.ok ? r.g.gz : 0, out->block = r.g.block, out->lds = (int64_t)r.g.lds, out->launches = r.launches;
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_op_resblock(const vits_resblock_desc* d, const float* x, const float* w1, const float* b1, const float* w2, const float* b2, const float* accum,
                              const int32_t* lens, float* y) {
    VITS_TRY
    using namespace vits;
    if (!d || !x || !w1 || !b1 || !w2 || !b2 || !y) return fail("vits_op_resblock: null argument (x, w1, b1, w2, b2 and y are required)");
    const int arith = g_op_arith;
    RbOpPlan r;
    std::string why;
    if (!resblock_resolve(d, arith, r, why)) return fail(why.c_str());
    const int B = d->batch, C = d->channels, T = d->t, k = d->k, nd = d->ndil, ts = round_up(T, 32);
    for (int b = 0; lens && b < B; ++b)
        if (lens[b] < 0 || lens[b] > T) return fail("vits_op_resblock: 0 <= lens[b] <= t is required");
    const bool f32 = arith == VITS_ARITH_F32;
    const size_t n = (size_t)B * C * ts, wn = (size_t)C * C * k;
    // the convs on the device
    struct Conv {
        PackedConv pc;
        DevBytes w, wl, w16, b;
    };
    std::vector<Conv> cv(2 * nd);  // pair p: conv 1 = cv[2 p], conv 2 = cv[2 p + 1]
    for (int i = 0; i < 2 * nd; ++i) {
        Conv& c = cv[i];
        PackedConv& pc = c.pc;
        const float* w = (i & 1 ? w2 : w1) + (size_t)(i / 2) * wn;
        const float* bias = (i & 1 ? b2 : b1) + (size_t)(i / 2) * C;
        pc.cin = pc.cout = C, pc.kt = k, pc.epi = EPI_STD;
        const std::vector<float> packed = pack_conv_weights(w, C, C, k, EPI_STD, 0, &pc.rows, &pc.mtiles_used, &pc.mtiles, &pc.nchunks);
        if (!c.b.put(bias, (size_t)C * 4)) return fail("device allocation failed");
        pc.bias = c.b.f();
        if (f32) {
            if (!c.w.put(packed.data(), packed.size() * 4)) return fail("device allocation failed");
            pc.wp = c.w.f(), pc.bytes = (int64_t)packed.size() * 4;
            if (conv_lat16_candidate(EPI_STD, k, C)) {
                const std::vector<float> pl = repack_conv_weights_l16(packed, pc.mtiles, pc.nchunks, k);
                if (!c.wl.put(pl.data(), pl.size() * 4)) return fail("device allocation failed");
                pc.wp_l16 = c.wl.f();
            }
        } else {
            const std::vector<uint16_t> p16 = pack_conv_weights16(w, C, C, k, EPI_STD, 0, arith);
            if (!c.w16.put(p16.data(), p16.size() * 2)) return fail("device allocation failed");
            pc.wp16 = c.w16.h(), pc.bytes16 = (int64_t)p16.size() * 2;
        }
    }
    // host staging: NaN everywhere, then the valid columns. std: [b][C][ts]; group: [b][C/8][ts][8]
    const float qnan = std::numeric_limits<float>::quiet_NaN();
    auto len_of = [&](int b) { return lens ? lens[b] : T; };
    auto stage = [&](const float* src, bool group) {
        std::vector<float> h(n, qnan);
        for (int b = 0; b < B; ++b)
            for (int c = 0; c < C; ++c) {
                const float* s = src + ((size_t)b * C + c) * d->t_stride;
                if (!group) {
                    std::memcpy(&h[((size_t)b * C + c) * ts], s, sizeof(float) * (size_t)len_of(b));
                    continue;
                }
                float* g = &h[(size_t)b * C * ts + (size_t)(c / 8) * ts * 8 + (c & 7)];
                for (int t = 0; t < len_of(b); ++t) g[(size_t)t * 8] = s[t];
            }
        return h;
    };
    DevInts dl;
    DevBytes dx, dxg, dacc, dout, dp[2], dt, dx16, dn16[2], dt16;
    if (!dl.put(lens, B)) return fail("device allocation failed");
    {
        const std::vector<float> hx = stage(x, false);
        if (!dx.put(hx.data(), n * 4) || !dout.fill(n * 4, 0) || !dp[0].fill(n * 4, 0xFF) || !dp[1].fill(n * 4, 0xFF)) return fail("device allocation failed");
        if (accum) {
            const std::vector<float> ha = stage(accum, !f32);
            if (!dacc.put(ha.data(), n * 4)) return fail("device allocation failed");
        }
    }
    hipError_t e = hipSuccess;
    const float scale = d->out_scale;
    if (f32) {
        if (r.variant == 1 && !dt.fill(n * 4, 0xFF)) return fail("device allocation failed");
        const TensorRef bx = tref(dx.f(), C, ts), bout = tref(dout.f(), C, ts), bacc = accum ? tref(dacc.f(), C, ts) : TensorRef();
        if (r.variant == 3) {
            const PackedConv *c1[3] = {&cv[0].pc, &cv[2].pc, &cv[4].pc}, *c2[3] = {&cv[1].pc, &cv[3].pc, &cv[5].pc};
            RbBlock32Call f;
            f.x = bx, f.y = bout, f.acc = bacc, f.lens = dl.p, f.batch = B, f.tmax = T, f.slope = d->slope, f.scale = scale, f.scale_div = d->scale_div;
            e = launch_rbblock32(c1, c2, f, nullptr);
        } else {
            TensorRef in = bx;
            for (int p = 0; p < nd && e == hipSuccess; ++p) {
                const bool last = p + 1 == nd;
                const TensorRef out = last ? bout : tref(dp[p & 1].f(), C, ts);  // a pair never writes the buffer it reads
                if (r.variant == 2) {
                    RbPair32Call f;
                    f.x = in, f.y = out, f.lens = dl.p, f.batch = B, f.tmax = T, f.dil = d->dil[p], f.slope = d->slope;
                    if (last) f.acc = bacc, f.scale = scale, f.scale_div = d->scale_div;
                    e = launch_rbpair32(cv[2 * p].pc, cv[2 * p + 1].pc, f, nullptr);
                } else {
                    // conv 1 / conv 2 as engine_vocoder.cpp builds them (mk_c1 / mk_c2): t is stored activated, its only reader is conv 2
                    ConvCall c1, c2;
                    c1.len_in = c1.len_out = dl.p;
                    c1.batch = B;
                    c1.t_in = c1.t_out = T;
                    c1.dil = d->dil[p];
                    c1.pad_l = (k * d->dil[p] - d->dil[p]) / 2;
                    c2 = c1;
                    c1.x = in, c1.y = tref(dt.f(), C, ts);
                    c1.pre_act = 1, c1.slope = d->slope, c1.post_act = 2, c1.post_slope = d->slope;
                    c2.x = c1.y, c2.dil = 1, c2.pad_l = (k - 1) / 2, c2.res = in, c2.y = out;
                    if (last) c2.acc = bacc, c2.scale = scale, c2.scale_div = d->scale_div;
                    e = launch_conv(cv[2 * p].pc, c1, nullptr);
                    if (e == hipSuccess) e = launch_conv(cv[2 * p + 1].pc, c2, nullptr);
                }
                in = out;
            }
        }
    } else {
        // group layout: the fp32 stream, and the 16-bit copy of leaky_relu(y_0) from the engine's converter
        const std::vector<float> hg = stage(x, true);
        const int64_t g_bs = (int64_t)C * ts;
        auto r16 = [&](const DevBytes& m) {
            Ref16 q;
            q.p = m.h(), q.ts = ts, q.bs = g_bs;
            return q;
        };
        if (!dxg.put(hg.data(), n * 4)) return fail("device allocation failed");
        const float* accg = accum ? dacc.f() : nullptr;
        if (r.variant >= 3) {
            const PackedConv *c1[3] = {&cv[0].pc, &cv[2].pc, &cv[4].pc}, *c2[3] = {&cv[1].pc, &cv[3].pc, &cv[5].pc};
            RbBlock16Call f;
            f.y0 = dxg.f(), f.lens = dl.p, f.batch = B, f.tmax = T, f.slope = d->slope, f.yg = dout.f(), f.accg = accg, f.g_bs = g_bs, f.g_ts = ts;
            f.scale = scale, f.scale_div = d->scale_div, f.force_nt = r.tiles;
            e = launch_rbblock16(c1, c2, f, arith, nullptr);
        } else {
            if (!dx16.fill(n * 2, 0xFF) || !dn16[0].fill(n * 2, 0xFF) || !dn16[1].fill(n * 2, 0xFF) || (r.variant == 1 && !dt16.fill(n * 2, 0xFF))) return fail("device allocation failed");
            e = launch_to_group16(tref(dx.f(), C, ts), dl.p, B, C, T, d->slope, r16(dx16), arith, nullptr);
            const float* ing = dxg.f();
            Ref16 in16 = r16(dx16);
            for (int p = 0; p < nd && e == hipSuccess; ++p) {
                const bool last = p + 1 == nd;
                float* outg = last ? dout.f() : dp[p & 1].f();
                const Ref16 out16 = last ? Ref16() : r16(dn16[p & 1]);
                if (r.variant == 2) {
                    RbPair16Call f;
                    f.x = in16, f.lens = dl.p, f.batch = B, f.tmax = T, f.dil = d->dil[p], f.slope = d->slope, f.yg = outg, f.resg = ing, f.g_bs = g_bs, f.g_ts = ts;
                    f.y16 = out16, f.y16_slope = last ? 1.f : d->slope, f.force_nr = r.nr;
                    if (last) f.accg = accg, f.scale = scale, f.scale_div = d->scale_div;
                    e = launch_rbpair16(cv[2 * p].pc, cv[2 * p + 1].pc, f, arith, nullptr);
                } else {
                    // conv 1 / conv 2 as engine_vocoder.cpp builds them (mk_pair): conv 1 writes only the 16-bit t, conv 2 the stream and its 16-bit copy
                    Conv16Call c1, c2;
                    c1.x = in16;
                    c1.len_in = c1.len_out = dl.p;
                    c1.batch = B;
                    c1.t_in = c1.t_out = T;
                    c1.dil = d->dil[p];
                    c1.pad_l = (k * d->dil[p] - d->dil[p]) / 2;
                    c1.y16 = r16(dt16);
                    c1.y16_slope = d->slope;
                    c2 = c1;
                    c2.x = c1.y16, c2.dil = 1, c2.pad_l = (k - 1) / 2, c2.g_bs = g_bs, c2.g_ts = ts, c2.resg = ing, c2.yg = outg;
                    c2.y16 = out16, c2.y16_slope = last ? 1.f : d->slope;
                    if (last) c2.accg = accg, c2.scale = scale, c2.scale_div = d->scale_div;
                    e = launch_conv16(cv[2 * p].pc, c1, arith, nullptr);
                    if (e == hipSuccess) e = launch_conv16(cv[2 * p + 1].pc, c2, arith, nullptr);
                }
                ing = outg, in16 = out16;
            }
        }
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail((std::string("vits_op_resblock: ") + r.kernel + ": " + hipGetErrorString(e)).c_str());
    std::vector<float> ho(n);
    if (hipMemcpy(ho.data(), dout.p, n * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail("copy back failed");
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < C; ++c) {
            float* dst = y + ((size_t)b * C + c) * d->t_stride;
            if (f32) {
                std::memcpy(dst, &ho[((size_t)b * C + c) * ts], sizeof(float) * (size_t)T);
                continue;
            }
            const float* g = &ho[(size_t)b * C * ts + (size_t)(c / 8) * ts * 8 + (c & 7)];
            for (int t = 0; t < T; ++t) dst[t] = g[(size_t)t * 8];
        }
    return 0;
    VITS_CATCH(-1)
}

// ---- vits_op_flow_coupling: which kernel a descriptor names (host arithmetic only: launch_plan.h), then the engine's call structs on staged tensors ---------
namespace {
struct FlowOpPlan {
    int variant = 0;
    std::string kernel;
    int bo = 0, halo = 0, ncw = 0, nct = 0, launches = 0;
    vits::LaunchGrid g;
};
bool fc_fail(std::string& why, const std::string& m) {
    why = "vits_op_flow_coupling: " + m;
    return false;
}
bool flow_resolve(const vits_flow_coupling_desc* d, int arith, FlowOpPlan& r, std::string& why) {
    using namespace vits;
    if (arith != VITS_ARITH_F32 && arith != VITS_ARITH_F16 && arith != VITS_ARITH_BF16)
        return fc_fail(why, "VITS_ARITH_F32, VITS_ARITH_F16 or VITS_ARITH_BF16 only (the split arithmetic has no flow kernels)");
    const int H = d->hidden, HF = d->half, k = d->k, B = d->batch, T = d->t, NL = d->layers;
    if (B < 1 || T < 1 || d->t_stride < T) return fc_fail(why, "batch >= 1 and 1 <= t <= t_stride are required");
    if (H < 32 || (H & 31)) return fc_fail(why, "hidden = " + std::to_string(H) + ": a multiple of 32 is required");
    if (HF < 32 || (HF & 31)) return fc_fail(why, "half = " + std::to_string(HF) + ": a multiple of 32 is required");
    if (k < 1 || !(k & 1)) return fc_fail(why, "k = " + std::to_string(k) + ": an odd tap count is required");
    if (NL < 1 || NL > 16) return fc_fail(why, "layers = " + std::to_string(NL) + ": 1 to 16 WaveNet layers");
    if (d->rate < 1 || (d->rate > 1 && NL > 8)) return fc_fail(why, "rate = " + std::to_string(d->rate) + ": >= 1 is required (and at most 8 layers of a dilated stack)");
    if (d->flipped != 0 && d->flipped != 1) return fc_fail(why, "flipped = " + std::to_string(d->flipped) + ": 0 (x0 first) or 1 (x1 first)");
    if (d->n_bias_rows < 1) return fc_fail(why, "n_bias_rows = " + std::to_string(d->n_bias_rows) + ": the b_in table has at least one row");
    if (d->variant < 0 || d->variant > 3) return fc_fail(why, "variant " + std::to_string(d->variant) + ": 0 (the engine's choice), 1 (un-fused), 2 (fused WaveNet layers), 3 (the coupling kernel)");
    if (d->ncw < 0 || d->nct < 0) return fc_fail(why, "(ncw, nct) = (" + std::to_string(d->ncw) + ", " + std::to_string(d->nct) + "): negative");
    const bool f32 = arith == VITS_ARITH_F32, bf = arith == VITS_ARITH_BF16;
    const std::string tile = "(ncw, nct) = (" + std::to_string(d->ncw) + ", " + std::to_string(d->nct) + ")";
    char name[96];
    int v = d->variant;
    if (v == 0) {  // engine_flow.cpp's order: the coupling kernel (16-bit modes), the fused WaveNet layers on large grids, nine launches
        if (d->ncw || d->nct) return fc_fail(why, tile + ": variant 0 takes the planner's tile");
        const bool wn = f32 ? plan_wavenet32(H, k, d->rate, B, T).ok : plan_wavenet16(H, k, d->rate, B, T).ok;
        v = !f32 && plan_flow_couple16(H, HF, k, d->rate, NL, B, T).ok ? 3 : wn && (int64_t)blocks_for(T, 32) * B >= 384 ? 2 : 1;
    }
    r.variant = v;
    if (v == 1) {
        if (d->ncw || d->nct) return fc_fail(why, tile + ": variant 1 has no tile to choose");
        r.kernel = f32 ? "launch_conv" : "launch_conv16";
        r.launches = 2 * NL + 2;
        return true;
    }
    if (v == 2) {
        const char* fam = f32 ? "wavenet32_kernel" : "wavenet16_kernel";
        if (H != 192) return fc_fail(why, std::string("variant 2: no ") + fam + " for hidden = " + std::to_string(H) + " (hidden = 192, k = 5, rate = 1)");
        if (k != 5) return fc_fail(why, std::string("variant 2: no ") + fam + " for k = " + std::to_string(k) + " (hidden = 192, k = 5, rate = 1)");
        if (d->rate != 1) return fc_fail(why, std::string("variant 2: no ") + fam + " for rate = " + std::to_string(d->rate) + " (hidden = 192, k = 5, rate = 1)");
        if (d->nct) return fc_fail(why, tile + ": variant 2 has no nct (a block is two column tiles)");
        if (f32 && d->ncw) return fc_fail(why, tile + ": wavenet32_kernel has one form (ncw = 0)");
        const WaveNetPlan pl = f32 ? plan_wavenet32(H, k, 1, B, T) : plan_wavenet16(H, k, 1, B, T, d->ncw);
        if (!pl.ok) return fc_fail(why, tile + ": no such wavenet16_kernel (ncw = 1 or 2)");
        r.g = pl, r.ncw = pl.ncw, r.bo = kWaveNetBM, r.halo = (k - 1) / 2, r.launches = NL + 2;
        if (f32) std::snprintf(name, sizeof(name), "wavenet32_kernel<%d, %d>", H, k);
        else std::snprintf(name, sizeof(name), "wavenet16_kernel<%d, %d, %s, %d>", H, k, bf ? "true" : "false", pl.ncw);
        r.kernel = name;
        return true;
    }
    if (f32) return fc_fail(why, "variant 3: flow_couple16_kernel exists in the 16-bit modes only");
    const char* only = " (hidden = 192, half = 96, k = 5, rate = 1, layers = 4)";
    if (H != 192) return fc_fail(why, "variant 3: no flow_couple16_kernel for hidden = " + std::to_string(H) + only);
    if (HF != 96) return fc_fail(why, "variant 3: no flow_couple16_kernel for half = " + std::to_string(HF) + only);
    if (k != 5) return fc_fail(why, "variant 3: no flow_couple16_kernel for k = " + std::to_string(k) + only);
    if (d->rate != 1) return fc_fail(why, "variant 3: no flow_couple16_kernel for rate = " + std::to_string(d->rate) + only);
    if (NL != 4) return fc_fail(why, "variant 3: no flow_couple16_kernel for layers = " + std::to_string(NL) + only);
    const FlowCouple16Plan pl = plan_flow_couple16(H, HF, k, 1, NL, B, T, d->ncw, d->nct);
    if (!pl.ok) return fc_fail(why, tile + ": no such flow_couple16_kernel ((1, 1), (1, 2) or (2, 2))");
    const FlowCouple16Geom ge = flow_couple16_geom(pl.ncw, pl.nct);
    r.g = pl, r.ncw = pl.ncw, r.nct = pl.nct, r.bo = ge.bo, r.halo = ge.halo, r.launches = 1;
    std::snprintf(name, sizeof(name), "flow_couple16_kernel<%s, %d, %d>", bf ? "true" : "false", pl.ncw, pl.nct);
    r.kernel = name;
    return true;
}
}  // namespace

VITS_API int vits_op_flow_coupling_plan(const vits_flow_coupling_desc* d, vits_flow_coupling_plan* out) {
    VITS_TRY
    if (!d || !out) return fail("vits_op_flow_coupling_plan: null argument");
    FlowOpPlan r;
    std::string why;
    if (!flow_resolve(d, g_op_arith, r, why)) return fail(why.c_str());
    std::memset(out, 0, sizeof(*out));
    std::snprintf(out->kernel, sizeof(out->kernel), "%s", r.kernel.c_str());
    out->variant = r.variant, out->bo = r.bo, out->halo = r.halo, out->ncw = r.ncw, out->nct = r.nct;
    out->grid_x = r.g.gx, out->grid_y = r.g.gy, out->grid_z = r.g.ok ? r.g.gz : 0, out->block = r.g.block, out->lds = (int64_t)r.g.lds, out->launches = r.launches;
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_op_flow_coupling(const vits_flow_coupling_desc* d, float* z, const float* w_pre, const float* b_pre, const float* w_in, const float* b_in,
                                   const float* w_rs, const float* b_rs, const float* w_post, const float* b_post, const int32_t* bias_rows, const int32_t* lens) {
    VITS_TRY
    using namespace vits;
    if (!d || !z || !w_pre || !b_pre || !w_in || !b_in || !w_rs || !b_rs || !w_post || !b_post)
        return fail("vits_op_flow_coupling: null argument (z and every weight and bias are required)");
    const int arith = g_op_arith;
    FlowOpPlan r;
    std::string why;
    if (!flow_resolve(d, arith, r, why)) return fail(why.c_str());
    const int B = d->batch, H = d->hidden, HF = d->half, T = d->t, k = d->k, NL = d->layers, ts = round_up(T, 32);
    for (int b = 0; b < B; ++b) {
        if (lens && (lens[b] < 0 || lens[b] > T)) return fail("vits_op_flow_coupling: 0 <= lens[b] <= t is required");
        if (bias_rows && (bias_rows[b] < 0 || bias_rows[b] >= d->n_bias_rows)) return fail("vits_op_flow_coupling: 0 <= bias_rows[b] < n_bias_rows is required");
    }
    const bool f32 = arith == VITS_ARITH_F32;
    // the convs on the device: pre, in[l], rs[l], post
    struct Conv {
        PackedConv pc;
        DevBytes w, wl, w16, b;
    };
    std::vector<Conv> cv(2 * NL + 2);
    DevBytes dtab;  // the b_in table [n_bias_rows][layers][2H]: in[l] points at its segment of row 0, one row stride for all (engine_load.cpp load_speakers)
    if (!dtab.put(b_in, (size_t)d->n_bias_rows * NL * 2 * H * 4)) return fail("device allocation failed");
    auto upload = [&](Conv& c, const float* w, const float* bias, int cout, int cin, int kt, int epi) {
        PackedConv& pc = c.pc;
        pc.cin = cin, pc.cout = cout, pc.kt = kt, pc.epi = epi;
        const std::vector<float> packed = pack_conv_weights(w, cout, cin, kt, epi, 0, &pc.rows, &pc.mtiles_used, &pc.mtiles, &pc.nchunks);
        if (bias) {
            if (!c.b.put(bias, (size_t)cout * 4)) return false;
            pc.bias = c.b.f();
        }
        if (f32) {
            if (!c.w.put(packed.data(), packed.size() * 4)) return false;
            pc.wp = c.w.f(), pc.bytes = (int64_t)packed.size() * 4;
            if (conv_lat16_candidate(epi, kt, cin)) {
                const std::vector<float> pl = repack_conv_weights_l16(packed, pc.mtiles, pc.nchunks, kt);
                if (!c.wl.put(pl.data(), pl.size() * 4)) return false;
                pc.wp_l16 = c.wl.f();
            }
        } else {
            const std::vector<uint16_t> p16 = pack_conv_weights16(w, cout, cin, kt, epi, 0, arith);
            if (!c.w16.put(p16.data(), p16.size() * 2)) return false;
            pc.wp16 = c.w16.h(), pc.bytes16 = (int64_t)p16.size() * 2;
        }
        return true;
    };
    Conv &pre = cv[0], &post = cv[2 * NL + 1];
    if (!upload(pre, w_pre, b_pre, H, HF, 1, EPI_STD) || !upload(post, w_post, b_post, HF, H, 1, EPI_STD)) return fail("device allocation failed");
    std::vector<PackedConv> in(NL), rs(NL);
    for (int l = 0; l < NL; ++l) {
        const int rows = l + 1 < NL ? 2 * H : H;
        if (!upload(cv[1 + 2 * l], w_in + (size_t)l * 2 * H * H * k, nullptr, 2 * H, H, k, EPI_GATE) ||
            !upload(cv[2 + 2 * l], w_rs + (size_t)l * 2 * H * H, b_rs + (size_t)l * 2 * H, rows, H, 1, EPI_STD))
            return fail("device allocation failed");
        in[l] = cv[1 + 2 * l].pc, rs[l] = cv[2 + 2 * l].pc;
        in[l].bias = dtab.f() + (size_t)l * 2 * H;
        in[l].bias_rs = bias_rows ? (int64_t)NL * 2 * H : 0;
    }
    // host staging: NaN everywhere, then the valid columns
    const float qnan = std::numeric_limits<float>::quiet_NaN();
    auto len_of = [&](int b) { return lens ? lens[b] : T; };
    const size_t nz = (size_t)B * 2 * HF * ts, nh = (size_t)B * 2 * H * ts, ng = (size_t)B * H * ts;
    std::vector<float> hz(nz);
    std::memset(hz.data(), 0xFF, nz * 4);
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < 2 * HF; ++c)
            std::memcpy(&hz[((size_t)b * 2 * HF + c) * ts], z + ((size_t)b * 2 * HF + c) * d->t_stride, sizeof(float) * (size_t)len_of(b));
    DevInts dl, dspk;
    DevBytes dz, dhout, dgate, dx16;
    if (!dl.put(lens, B) || !dspk.put(bias_rows, B) || !dz.put(hz.data(), nz * 4)) return fail("device allocation failed");
    const TensorRef zr = tref(dz.f(), 2 * HF, ts);
    TensorRef x0 = zr, x1 = zr;
    (d->flipped ? x0 : x1).p += (size_t)HF * ts;
    hipError_t e = hipSuccess;
    if (r.variant == 3) {
        FlowCouple16Call fc;
        fc.x0 = x0, fc.x1 = x1, fc.lens = dl.p, fc.spk = dspk.p, fc.batch = B, fc.tmax = T, fc.hidden = H, fc.half = HF;
        fc.force_ncw = r.ncw, fc.force_nct = r.nct;
        e = launch_flow_couple16(pre.pc, in.data(), rs.data(), post.pc, fc, arith, nullptr);
    } else {
        // hout: h = rows [0, H), the skip sum `outputs` = rows [H, 2H), zero on the valid columns (launch_fill_rows of the engine); gate: the gated conv's
        // output, and the other h buffer of the fused layers
        {
            std::vector<float> hh(nh, qnan);
            for (int b = 0; b < B; ++b)
                for (int c = H; c < 2 * H; ++c) std::fill_n(&hh[((size_t)b * 2 * H + c) * ts], len_of(b), 0.f);
            if (!dhout.put(hh.data(), nh * 4) || !dgate.fill(ng * 4, 0xFF)) return fail("device allocation failed");
        }
        const size_t x16_bytes = f32 ? 0 : (size_t)B * (std::max(H, HF) / 8) * round_up(T, 8) * 8 * 2;
        if (!f32 && !dx16.fill(x16_bytes, 0xFF)) return fail("device allocation failed");
        // a conv of the fp32-layout orchestration (Engine::conv): the fp32 kernel, or the converter + the 16-bit-operand kernel (Engine::conv16_transparent)
        auto conv = [&](const PackedConv& w, const ConvCall& c) -> hipError_t {
            if (f32) return launch_conv(w, c, nullptr);
            Ref16 x16;
            x16.p = dx16.h(), x16.ts = round_up(c.t_in, 8), x16.bs = (int64_t)((w.cin + 7) / 8) * x16.ts * 8;
            if (hipMemsetAsync(dx16.p, 0xFF, x16_bytes, nullptr) != hipSuccess) return hipErrorUnknown;
            hipError_t e2 = launch_to_group16(c.x, c.len_in, c.batch, w.cin, c.t_in, 1.0f, x16, arith, nullptr);
            if (e2 != hipSuccess) return e2;
            Conv16Call q;
            q.x = x16, q.len_in = c.len_in, q.len_out = c.len_out, q.spk = c.spk, q.batch = c.batch, q.t_in = c.t_in, q.t_out = c.t_out, q.dil = c.dil, q.pad_l = c.pad_l;
            q.y = c.y, q.res = c.res;
            return launch_conv16(w, q, arith, nullptr);
        };
        auto mk = [&](TensorRef xin, TensorRef yout) {
            ConvCall c;
            c.x = xin, c.y = yout, c.len_in = c.len_out = dl.p, c.spk = dspk.p, c.batch = B, c.t_in = c.t_out = T;
            return c;
        };
        const TensorRef hout = tref(dhout.f(), 2 * H, ts), gate = tref(dgate.f(), H, ts);
        TensorRef outputs = hout;
        outputs.p += (size_t)H * ts;
        e = conv(pre.pc, mk(x0, hout));
        TensorRef hcur = hout;
        for (int l = 0, dil = 1; l < NL && e == hipSuccess; ++l, dil *= d->rate) {
            const bool last = l + 1 == NL;
            if (r.variant == 2) {
                WaveNet32Call w;
                w.h = hcur, w.h_out = last ? TensorRef() : (hcur.p == gate.p ? hout : gate), w.outputs = outputs;
                w.lens = dl.p, w.spk = dspk.p, w.batch = B, w.tmax = T, w.hidden = H, w.dil = dil, w.force_ncw = r.ncw;
                e = f32 ? launch_wavenet32(in[l], rs[l], w, nullptr) : launch_wavenet16(in[l], rs[l], w, arith, nullptr);
                if (w.h_out.p) hcur = w.h_out;
                continue;
            }
            ConvCall g = mk(hout, gate);
            g.dil = dil, g.pad_l = (k * dil - dil) / 2;
            e = conv(in[l], g);
            ConvCall q = mk(gate, last ? outputs : hout);
            q.res = q.y;
            if (e == hipSuccess) e = conv(rs[l], q);
        }
        if (e == hipSuccess) {
            ConvCall pc = mk(outputs, x1);
            pc.res = x1;
            e = conv(post.pc, pc);
        }
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail((std::string("vits_op_flow_coupling: ") + r.kernel + ": " + hipGetErrorString(e)).c_str());
    if (hipMemcpy(hz.data(), dz.p, nz * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail("copy back failed");
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < 2 * HF; ++c) std::memcpy(z + ((size_t)b * 2 * HF + c) * d->t_stride, &hz[((size_t)b * 2 * HF + c) * ts], sizeof(float) * (size_t)T);
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_op_conv_transpose1d(const vits_convt1d_desc* d, const float* x, const float* w, const float* bias, const int32_t* lens, float* y) {
    VITS_TRY
    using namespace vits;
    if (!d || !x || !w || !y) return fail("null argument");
    if (d->k != 2 * d->stride) return fail("kernel must be 2*stride");
    if (g_op_arith == VITS_ARITH_F32_SPLIT) return fail("VITS_ARITH_F32_SPLIT: the transposed conv has no split kernel");
    PackedConv pc;
    pc.cin = d->cin;
    pc.cout = d->cout;
    pc.kt = 2;
    pc.epi = EPI_CONVT;
    pc.ct_stride = d->stride;
    std::vector<float> packed = pack_conv_weights(w, d->cout, d->cin, d->k, EPI_CONVT, d->stride, &pc.rows, &pc.mtiles_used, &pc.mtiles, &pc.nchunks);
    DevBuf dw, db, dx, dy;
    DevInts dl, dlo;
    const size_t nx = (size_t)d->batch * d->cin * d->t_stride, ny = (size_t)d->batch * d->cout * d->t_out_stride;
    std::vector<int32_t> lo;
    if (lens) {
        lo.resize(d->batch);
        for (int b = 0; b < d->batch; ++b) lo[b] = d->stride * lens[b] + d->k - d->stride - 2 * d->crop;
    }
    if (!dw.put(packed.data(), packed.size()) || !dx.put(x, nx) || !dy.put(nullptr, ny) || !dl.put(lens, d->batch) || !dlo.put(lens ? lo.data() : nullptr, d->batch))
        return fail("device allocation failed");
    if (bias && !db.put(bias, d->cout)) return fail("device allocation failed");
    pc.wp = dw.p;
    pc.bias = db.p;
    ConvCall c;
    c.x = tref(dx.p, d->cin, d->t_stride);
    c.y = tref(dy.p, d->cout, d->t_out_stride);
    c.len_in = dl.p;
    c.len_out = dlo.p;
    c.batch = d->batch;
    c.t_in = d->t;
    c.t_out = d->stride * d->t + d->k - d->stride - 2 * d->crop;
    c.pre_act = d->pre_slope != 1.0f;
    c.slope = d->pre_slope;
    c.ct_crop = d->crop;
    DevBuf w16, x16;
    hipError_t e = run_op_conv(pc, c, w, d->k, w16, x16);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(hipGetErrorString(e));
    if (hipMemcpy(y, dy.p, ny * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail("copy back failed");
    return 0;
    VITS_CATCH(-1)
}

// ---- vits_op_upsample16: which kernel a descriptor names (host arithmetic only: launch_plan.h, conv_plan.h), then the engine's Conv16Call on staged tensors ----------
namespace {
struct UpOpPlan {
    int variant = 0, bn = 0, t_out = 0;
    std::string kernel;
    char tag[16] = "";
    vits::LaunchGrid g;
    vits::PackedConv pc;  // the shape fields; the op adds the device pointers
};
bool up_fail(std::string& why, const std::string& m) {
    why = "vits_op_upsample16: " + m;
    return false;
}
// (runs under the caller's KernelKnobsScope over the knobs' defaults: no environment variable reaches the choice)
bool upsample16_resolve(const vits_upsample16_desc* d, int arith, UpOpPlan& r, std::string& why) {
    using namespace vits;
    if (arith != VITS_ARITH_F16 && arith != VITS_ARITH_BF16)
        return up_fail(why, "VITS_ARITH_F16 or VITS_ARITH_BF16 only (the fp32 upsampler is vits_op_conv_transpose1d; the split arithmetic has no transposed conv)");
    const int B = d->batch, cin = d->cin, cout = d->cout, T = d->t, s = d->stride;
    if (B < 1 || T < 1 || d->t_stride < T) return up_fail(why, "batch >= 1 and 1 <= t <= t_stride are required");
    if (s < 1) return up_fail(why, "stride = " + std::to_string(s) + ": >= 1 is required (the kernel size is 2 x stride)");
    if (d->crop < 0 || 2 * d->crop > s) return up_fail(why, "crop = " + std::to_string(d->crop) + ": 0 <= 2 crop <= stride is required");
    if (cin < 8 || (cin & 7) || cout < 8 || (cout & 7)) return up_fail(why, "c_in = " + std::to_string(cin) + ", c_out = " + std::to_string(cout) + ": the group layout takes multiples of 8");
    r.t_out = s * T + s - 2 * d->crop;
    if (d->t_out_stride < r.t_out) return up_fail(why, "t_out_stride = " + std::to_string(d->t_out_stride) + " < t_out = " + std::to_string(r.t_out));
    if (d->variant < 0 || d->variant > 2) return up_fail(why, "variant " + std::to_string(d->variant) + ": 0 (the engine's choice), 1 (GEMM tile), 2 (streaming kernel)");
    if (!(d->split == 0 || d->split == 1 || d->split == 2 || d->split == 4)) return up_fail(why, "split = " + std::to_string(d->split) + ": 0 (the planner's), 1, 2 or 4");
    PackedConv& pc = r.pc;
    pc.cin = cin, pc.cout = cout, pc.kt = 2, pc.epi = EPI_CONVT, pc.ct_stride = s;
    const ConvPackDims pd = conv_pack_dims(cout, cin, 2 * s, EPI_CONVT, s);
    pc.rows = pd.rows, pc.mtiles_used = pd.mtiles_used, pc.mtiles = pd.mtiles, pc.nchunks = pd.nchunks;
    const bool bf = arith == VITS_ARITH_BF16;
    const ConvT16Plan policy = plan_convt16(pc, B, T);
    std::snprintf(r.tag, sizeof(r.tag), "%s", policy.tag);
    const int v = d->variant ? d->variant : policy.supported ? 2 : 1;  // engine_vocoder.cpp: convt16_stream_supported, else conv16
    r.variant = v;
    char name[96];
    if (v == 2) {
        const std::string shape = "c_in = " + std::to_string(cin) + ", c_out = " + std::to_string(cout) + ", stride = " + std::to_string(s);
        if (cin % 64) return up_fail(why, "variant 2: " + shape + ": c_in is not a multiple of 64");
        if (cout % 32) return up_fail(why, "variant 2: " + shape + ": c_out is not a multiple of 32");
        if (cin > 512) return up_fail(why, "variant 2: " + shape + ": c_in > 512 (the input tile of all channels does not fit LDS)");
        if (pc.rows > 128 && s % 4 != 0) return up_fail(why, "variant 2: " + shape + ": rows = stride x c_out = " + std::to_string(pc.rows) + " > 128 and stride is not a multiple of 4");
        const bool lines = policy.lines_bn != 0;
        if (d->split && !lines) return up_fail(why, "split = " + std::to_string(d->split) + ": only convt16_lines_kernel deals its units over gridDim.z, this shape runs on convt16_kernel (" + policy.tag + ")");
        const ConvT16Plan pl = plan_convt16(pc, B, T, d->split);
        if (!pl.supported || !pl.ok) return up_fail(why, "variant 2: plan_convt16 refuses " + shape);
        r.g = pl, r.bn = pl.lines_bn ? pl.lines_bn : convt16_bn(pl.nr, pl.csplit);
        if (lines) std::snprintf(name, sizeof(name), "convt16_lines_kernel<%d, %s>", pl.lines_bn, bf ? "true" : "false");
        else std::snprintf(name, sizeof(name), "convt16_kernel<%d, %d, %d, %s>", pl.nr, pl.csplit, pl.rs, bf ? "true" : "false");
        r.kernel = name;
        return true;
    }
    if (d->split) return up_fail(why, "split = " + std::to_string(d->split) + ": only convt16_lines_kernel deals its units over gridDim.z, variant 1 runs conv16_kernel");
    Conv16Call c;
    c.batch = B, c.t_in = T, c.t_out = r.t_out, c.ct_crop = d->crop;
    c.yg = reinterpret_cast<float*>(sizeof(float));  // (never dereferenced: to plan_conv16 a non-null yg means "group outputs")
    const Conv16Plan pl = plan_conv16(pc, c);
    if (pl.lat || pl.epi16 != C16_CONVT_GROUP || pl.xwp > 384 || pl.dil_ct == kNoKernel || !conv16_tile_exists(pl.epi16, pl.dil_ct, pl.tile))
        return up_fail(why, "variant 1: plan_conv16 has no conv16_kernel for this transposed conv");
    const TileShape ts = tile16_shape(pl.tile);
    r.bn = ts.bn();
    r.g.ok = true, r.g.gx = pl.gx, r.g.gy = pl.gy, r.g.gz = pl.gz, r.g.block = 320, r.g.lds = pl.lds;
    std::snprintf(name, sizeof(name), "conv16_kernel<2, -1, %d, %d, %d, %d, %d, %s>", ts.wm, ts.wn, ts.mr, ts.nr, (int)C16_CONVT_GROUP, bf ? "true" : "false");
    r.kernel = name;
    return true;
}
}  // namespace

VITS_API int vits_op_upsample16_plan(const vits_upsample16_desc* d, vits_upsample16_plan* out) {
    VITS_TRY
    if (!d || !out) return fail("vits_op_upsample16_plan: null argument");
    const vits::KernelKnobs defaults;
    vits::KernelKnobsScope scope(&defaults);
    UpOpPlan r;
    std::string why;
    if (!upsample16_resolve(d, g_op_arith, r, why)) return fail(why.c_str());
    std::memset(out, 0, sizeof(*out));
    std::snprintf(out->kernel, sizeof(out->kernel), "%s", r.kernel.c_str());
    std::snprintf(out->tag, sizeof(out->tag), "%s", r.tag);
    out->variant = r.variant, out->bn = r.bn;
    out->grid_x = r.g.gx, out->grid_y = r.g.gy, out->grid_z = r.g.gz, out->block = r.g.block, out->lds = (int64_t)r.g.lds;
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_op_upsample16(const vits_upsample16_desc* d, const float* x, const float* w, const float* bias, const int32_t* lens, float* y, uint16_t* y16,
                                uint16_t* x16) {
    VITS_TRY
    using namespace vits;
    if (!d || !x || !w || !y) return fail("vits_op_upsample16: null argument (x, w and y are required)");
    const KernelKnobs defaults;
    KernelKnobsScope scope(&defaults);
    const int arith = g_op_arith;
    UpOpPlan r;
    std::string why;
    if (!upsample16_resolve(d, arith, r, why)) return fail(why.c_str());
    const int B = d->batch, cin = d->cin, cout = d->cout, T = d->t, s = d->stride, t_out = r.t_out;
    for (int b = 0; lens && b < B; ++b)
        if (lens[b] < 0 || lens[b] > T) return fail("vits_op_upsample16: 0 <= lens[b] <= t is required");
    // the conv on the device
    PackedConv& pc = r.pc;
    DevBytes dw16, db;
    {
        const std::vector<uint16_t> p16 = pack_conv_weights16(w, cout, cin, 2 * s, EPI_CONVT, s, arith);
        if (!dw16.put(p16.data(), p16.size() * 2) || (bias && !db.put(bias, (size_t)cout * 4))) return fail("device allocation failed");
        pc.wp16 = dw16.h(), pc.bytes16 = (int64_t)p16.size() * 2, pc.bias = bias ? db.f() : nullptr;
    }
    // staging, as engine_vocoder.cpp hands a stage to its upsampler
    const int x_ts = round_up(T, 32), g_ts = round_up(t_out, 32);
    const size_t nx = (size_t)B * cin * d->t_stride, nx16 = (size_t)B * cin * x_ts, ng = (size_t)B * cout * g_ts;
    std::vector<int32_t> lo;
    if (lens) {
        lo.resize(B);
        for (int b = 0; b < B; ++b) lo[b] = s * lens[b] + s - 2 * d->crop;
    }
    DevInts dl, dlo;
    DevBytes dx, dx16, dyg, dy16;
    if (!dl.put(lens, B) || !dlo.put(lens ? lo.data() : nullptr, B) || !dx.put(x, nx * 4) || !dx16.fill(nx16 * 2, 0xFF) || !dyg.fill(ng * 4, 0) || (y16 && !dy16.fill(ng * 2, 0)))
        return fail("device allocation failed");
    Conv16Call cu;
    cu.x.p = dx16.h(), cu.x.ts = x_ts, cu.x.bs = (int64_t)cin * x_ts;
    cu.len_in = dl.p;
    cu.len_out = dlo.p;
    cu.batch = B;
    cu.t_in = T;
    cu.t_out = t_out;
    cu.ct_crop = d->crop;
    cu.yg = dyg.f();
    cu.g_bs = (int64_t)cout * g_ts;
    cu.g_ts = g_ts;
    if (y16) {
        cu.y16.p = dy16.h(), cu.y16.ts = g_ts, cu.y16.bs = (int64_t)cout * g_ts;
        cu.y16_slope = d->y16_slope;
    }
    cu.force_split = d->split;
    hipError_t e = launch_to_group16(tref(dx.f(), cin, d->t_stride), dl.p, B, cin, T, d->pre_slope, cu.x, arith, nullptr);
    if (e == hipSuccess) e = r.variant == 2 ? launch_convt16_stream(pc, cu, arith, nullptr) : launch_conv16(pc, cu, arith, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail((std::string("vits_op_upsample16: ") + r.kernel + ": " + hipGetErrorString(e)).c_str());
    // group layout [b][c / 8][ts][8] -> [b][c][stride]
    {
        std::vector<float> hg(ng);
        if (hipMemcpy(hg.data(), dyg.p, ng * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail("copy back failed");
        for (int b = 0; b < B; ++b)
            for (int c = 0; c < cout; ++c) {
                const float* g = &hg[(size_t)b * cout * g_ts + (size_t)(c / 8) * g_ts * 8 + (c & 7)];
                float* dst = y + ((size_t)b * cout + c) * d->t_out_stride;
                for (int n = 0; n < t_out; ++n) dst[n] = g[(size_t)n * 8];
            }
    }
    auto ungroup16 = [&](const DevBytes& m, int C, int ts, int cols, int stride, uint16_t* out) {
        std::vector<uint16_t> h((size_t)B * C * ts);
        if (hipMemcpy(h.data(), m.p, h.size() * 2, hipMemcpyDeviceToHost) != hipSuccess) return false;
        for (int b = 0; b < B; ++b)
            for (int c = 0; c < C; ++c) {
                const uint16_t* g = &h[(size_t)b * C * ts + (size_t)(c / 8) * ts * 8 + (c & 7)];
                uint16_t* dst = out + ((size_t)b * C + c) * stride;
                for (int n = 0; n < cols; ++n) dst[n] = g[(size_t)n * 8];
            }
        return true;
    };
    if (y16 && !ungroup16(dy16, cout, g_ts, t_out, d->t_out_stride, y16)) return fail("copy back failed");
    if (x16 && !ungroup16(dx16, cin, x_ts, T, d->t_stride, x16)) return fail("copy back failed");
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_op_rel_attention(int32_t batch, int32_t heads, int32_t head_dim, int32_t t, int32_t t_stride, int32_t window, const float* q, const float* k,
                                   const float* v, const float* rel_k, const float* rel_v, const int32_t* lens, float* out) {
    VITS_TRY
    using namespace vits;
    const int C = heads * head_dim;
    const size_t n = (size_t)batch * C * t_stride, nr = (size_t)(2 * window + 1) * head_dim;
    DevBuf dq, dk, dv, drk, drv, dout;
    DevInts dl;
    if (!dq.put(q, n) || !dk.put(k, n) || !dv.put(v, n) || !drk.put(rel_k, nr) || !drv.put(rel_v, nr) || !dout.put(nullptr, n) || !dl.put(lens, batch))
        return fail("device allocation failed");
    hipError_t e = launch_rel_attention(tref(dq.p, C, t_stride), tref(dk.p, C, t_stride), tref(dv.p, C, t_stride), drk.p, drv.p, tref(dout.p, C, t_stride), dl.p, batch,
                                        heads, head_dim, t, window, 1.0f, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(hipGetErrorString(e));
    if (hipMemcpy(out, dout.p, n * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail("copy back failed");
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_op_add_layer_norm(int32_t batch, int32_t channels, int32_t t, int32_t t_stride, float eps, const float* x, const float* residual,
                                    const float* gamma, const float* beta, float* y) {
    VITS_TRY
    using namespace vits;
    const size_t n = (size_t)batch * channels * t_stride;
    DevBuf dx, dr, dg, db, dy;
    if (!dx.put(x, n) || !dg.put(gamma, channels) || !db.put(beta, channels) || !dy.put(nullptr, n)) return fail("device allocation failed");
    if (residual && !dr.put(residual, n)) return fail("device allocation failed");
    TensorRef none;
    hipError_t e = launch_add_layer_norm(tref(dx.p, channels, t_stride), residual ? tref(dr.p, channels, t_stride) : none, dg.p, db.p, tref(dy.p, channels, t_stride),
                                         nullptr, batch, channels, t, eps, 0, none, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(hipGetErrorString(e));
    if (hipMemcpy(y, dy.p, n * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail("copy back failed");
    return 0;
    VITS_CATCH(-1)
}

// ---- vits_op_attention / vits_op_layer_norm / vits_op_norm_conv: which kernel a descriptor names (host arithmetic only: launch_plan.h, conv_plan.h), then the text
// encoder's launches on staged tensors. (The resolvers run under the caller's KernelKnobsScope over the knobs' defaults: no environment variable reaches the choice)
namespace {
// [batch][rows][pitch] floats on the device: 0xFF bytes (NaN), then columns [0, lens[b]) of src's rows (host pitch src_pitch); src NULL: 0xFF only
bool stage_ff(DevBytes& dst, const float* src, int batch, int rows, int src_pitch, int pitch, const int32_t* lens, int t) {
    const size_t n = (size_t)batch * rows * pitch;
    std::vector<float> h(std::max<size_t>(n, 4));
    std::memset(h.data(), 0xFF, h.size() * 4);
    for (int b = 0; src && b < batch; ++b)
        for (int c = 0; c < rows; ++c)
            std::memcpy(&h[((size_t)b * rows + c) * pitch], src + ((size_t)b * rows + c) * src_pitch, sizeof(float) * (size_t)(lens ? lens[b] : t));
    return dst.put(h.data(), h.size() * 4);
}
bool op_fail(std::string& why, const char* op, const std::string& m) {
    why = std::string(op) + ": " + m;
    return false;
}
const char* tf(bool v) { return v ? "true" : "false"; }

struct AttOpPlan {
    int variant = 0;
    std::string kernel;
    vits::AttentionPlan p;
};
bool attention_resolve(const vits_attention_desc* d, AttOpPlan& r, std::string& why) {
    using namespace vits;
    const char* op = "vits_op_attention";
    const int hd = d->head_dim, v = d->variant;
    if (d->batch < 1 || d->heads < 1 || d->t < 1 || d->t_stride < d->t) return op_fail(why, op, "batch >= 1, heads >= 1 and 1 <= t <= t_stride are required");
    if (d->window < 0) return op_fail(why, op, "window = " + std::to_string(d->window) + ": at least 0");
    if (v < 0 || v > 6)
        return op_fail(why, op, "variant " + std::to_string(v) + ": 0 (the planner's choice), 1 / 2 (rel_attention_kernel<1024> / <256>), 3 ... 6 (rel_attention_mfma_kernel<4, 32, false, false>, <8, 32, false, false>, <4, 24, true, false>, <8, 24, false, true>)");
    if (hd < 1 || hd > 128) return op_fail(why, op, "head_dim = " + std::to_string(hd) + ": no attention kernel above 128 (1 to 128)");
    if (v >= 3 && (hd & 15)) return op_fail(why, op, "variant " + std::to_string(v) + ": head_dim = " + std::to_string(hd) + " is not a multiple of 16 (the matrix-core kernel's d tiles)");
    if (v >= 5 && hd > 96) return op_fail(why, op, "variant " + std::to_string(v) + ": head_dim = " + std::to_string(hd) + " is above 96 (the register arrays of the 24-step kernels)");
    if (v >= 3 && att_mfma_lds(hd, d->t, d->window) > kLdsMax)
        return op_fail(why, op, "variant " + std::to_string(v) + ": rel_attention_mfma_kernel needs " + std::to_string(att_mfma_lds(hd, d->t, d->window)) + " bytes of LDS, the limit is " + std::to_string(kLdsMax));
    if ((v == 1 || v == 2) && att_valu_lds(hd, d->t, d->window, 3) > kLdsSoft)
        return op_fail(why, op, "variant " + std::to_string(v) + ": rel_attention_kernel needs " + std::to_string(att_valu_lds(hd, d->t, d->window, 3)) + " bytes of LDS, the limit is " + std::to_string(kLdsSoft));
    r.p = plan_rel_attention(d->batch, d->heads, hd, d->t, d->window, v);
    if (!r.p.ok) return op_fail(why, op, v ? "variant " + std::to_string(v) + ": plan_rel_attention refuses the shape" : "no attention kernel takes this shape (the scores of one block pass the LDS limit)");
    char name[96];
    if (r.p.mfma) {
        r.variant = r.p.lat ? 6 : r.p.sh ? 5 : r.p.nw == 8 ? 4 : 3;
        std::snprintf(name, sizeof(name), "rel_attention_mfma_kernel<%d, %d, %s, %s>", r.p.nw, r.p.maxs, tf(r.p.sh), tf(r.p.lat));
    } else {
        r.variant = r.p.block == 1024 ? 1 : 2;
        std::snprintf(name, sizeof(name), "rel_attention_kernel<%d>", r.p.block);
    }
    r.kernel = name;
    return true;
}

bool layer_norm_resolve(const vits_layer_norm_desc* d, bool has_tab, vits::LayerNormPlan& p, std::string& why) {
    using namespace vits;
    const char* op = "vits_op_layer_norm";
    if (d->batch < 1 || d->channels < 1 || d->t < 1 || d->t_stride < d->t) return op_fail(why, op, "batch >= 1, channels >= 1 and 1 <= t <= t_stride are required");
    if (!(d->eps > 0.f)) return op_fail(why, op, "eps must be positive");
    if (d->tw != 0 && d->tw != 32 && d->tw != 64) return op_fail(why, op, "tw = " + std::to_string(d->tw) + ": 0 (the planner's choice), 32 or 64 time steps per block");
    if ((d->post_gelu != 0 && d->post_gelu != 1) || (d->add_to != 0 && d->add_to != 1)) return op_fail(why, op, "post_gelu and add_to are 0 or 1");
    if (has_tab && !d->post_gelu) return op_fail(why, op, "gelu_tab without post_gelu: the table is the GELU's");
    p = plan_add_layer_norm(d->channels, d->batch, d->t, d->tw);
    if (!p.ok) {
        const int tw = d->tw ? d->tw : 32;
        return op_fail(why, op, "add_layer_norm_kernel<" + std::to_string(tw) + "> needs " + std::to_string(layer_norm_lds(d->channels, tw)) + " bytes of LDS for channels = " +
                                    std::to_string(d->channels) + ", the limit is " + std::to_string(kLdsSoft));
    }
    return true;
}

struct NormConvOpPlan {
    int variant = 0, pitch = 0, launches = 0;
    bool ln_ok = false;
    std::string ln_why;
    vits::ConvPlan cp;    // of the conv that runs
    vits::PackedConv pc;  // the shape fields; the op adds the device pointers
};
const char* conv_tile_name(int tile) {
    static const char* const names[] = {"TILE_128x128", "TILE_64x256", "TILE_32x256", "TILE_64x64", "TILE_32x64", "TILE_NARROW", "TILE_LAT16"};
    return tile >= 0 && tile <= 6 ? names[tile] : "?";
}
// the two calls of the op for the planner: `fused` with LayerNorm on load, `plain` on the normalised tensor (pointers: only whether they are set and equal matters)
void norm_conv_calls(const vits_norm_conv_desc* d, const int* lens, vits::ConvCall& plain, vits::ConvCall& fused) {
    plain.len_in = plain.len_out = lens;
    plain.batch = d->batch, plain.t_in = plain.t_out = d->t;
    plain.pad_l = d->pad_left, plain.post_act = d->post_act;
    fused = plain;
    fused.ln_gamma = fused.ln_beta = reinterpret_cast<const float*>(sizeof(float));  // (the op replaces them; to plan_conv non-null means "with the statistics' LDS")
    fused.ln_eps = d->eps;
}
bool norm_conv_resolve(const vits_norm_conv_desc* d, int arith, NormConvOpPlan& r, std::string& why) {
    using namespace vits;
    const char* op = "vits_op_norm_conv";
    if (arith != VITS_ARITH_F32) return op_fail(why, op, "VITS_ARITH_F32 only (the engine normalises on load in fp32 alone)");
    if (d->batch < 1 || d->cin < 1 || d->cout < 1 || d->t < 1 || d->t_stride < d->t) return op_fail(why, op, "batch, cin, cout >= 1 and 1 <= t <= t_stride are required");
    r.pitch = d->pitch ? d->pitch : round_up(d->t, 32);
    if (r.pitch < d->t) return op_fail(why, op, "pitch = " + std::to_string(d->pitch) + " < t = " + std::to_string(d->t));
    if (d->k < 1 || d->k > 64) return op_fail(why, op, "k = " + std::to_string(d->k) + ": 1 to 64 taps");
    if (d->pad_left < 0 || d->pad_left > d->k - 1) return op_fail(why, op, "pad_left = " + std::to_string(d->pad_left) + ": 0 to k - 1 (every output reads its own column)");
    if (d->post_act != 0 && d->post_act != 1) return op_fail(why, op, "post_act " + std::to_string(d->post_act) + ": 0 (none) or 1 (relu)");
    if (!(d->eps > 0.f)) return op_fail(why, op, "eps must be positive");
    if (d->variant < 0 || d->variant > 2) return op_fail(why, op, "variant " + std::to_string(d->variant) + ": 0 (the engine's choice), 1 (LayerNorm launch + conv), 2 (LayerNorm on load)");
    PackedConv& pc = r.pc;
    pc.cin = d->cin, pc.cout = d->cout, pc.kt = d->k, pc.epi = EPI_STD;
    const ConvPackDims pd = conv_pack_dims(d->cout, d->cin, d->k, EPI_STD, 0);
    pc.rows = pd.rows, pc.mtiles_used = pd.mtiles_used, pc.mtiles = pd.mtiles, pc.nchunks = pd.nchunks;
    if (conv_lat16_candidate(EPI_STD, d->k, d->cin)) pc.wp_l16 = reinterpret_cast<float*>(sizeof(float));  // (as the engine's load gives the layer its second copy; the op replaces it)
    ConvCall plain, fused;
    norm_conv_calls(d, nullptr, plain, fused);
    const ConvPlan pf = plan_conv(pc, fused), pp = plan_conv(pc, plain);
    r.ln_ok = pf.ln_ok, r.ln_why = pf.ln_why ? pf.ln_why : "";
    r.variant = d->variant ? d->variant : pf.ln_ok ? 2 : 1;  // Engine::run_text_encoder's conv_of_norm
    if (r.variant == 2 && !pf.ln_ok) return op_fail(why, op, "variant 2: conv_ln_on_load_ok refuses: " + r.ln_why);
    r.cp = r.variant == 2 ? pf : pp;
    if (!r.cp.ok) return op_fail(why, op, "variant " + std::to_string(r.variant) + ": plan_conv has no kernel for this conv");
    if (r.variant == 1 && !plan_add_layer_norm(d->cin, d->batch, d->t).ok) return op_fail(why, op, "variant 1: add_layer_norm_kernel has no tile for channels = " + std::to_string(d->cin));
    r.launches = r.variant == 2 ? 1 : 2;
    return true;
}
bool op_lens_ok(const int32_t* lens, int batch, int t) {
    for (int b = 0; lens && b < batch; ++b)
        if (lens[b] < 0 || lens[b] > t) return false;
    return true;
}
}  // namespace

VITS_API int vits_op_attention_plan(const vits_attention_desc* d, vits_attention_plan* out) {
    VITS_TRY
    if (!d || !out) return fail("vits_op_attention_plan: null argument");
    const vits::KernelKnobs defaults;
    vits::KernelKnobsScope scope(&defaults);
    AttOpPlan r;
    std::string why;
    if (!attention_resolve(d, r, why)) return fail(why.c_str());
    std::memset(out, 0, sizeof(*out));
    std::snprintf(out->kernel, sizeof(out->kernel), "%s", r.kernel.c_str());
    out->variant = r.variant, out->nw = r.p.nw, out->maxs = r.p.maxs, out->vshift = r.p.mfma ? 0 : r.p.vshift;
    out->grid_x = r.p.gx, out->grid_y = r.p.gy, out->grid_z = r.p.gz, out->block = r.p.block, out->lds = (int64_t)r.p.lds;
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_op_attention(const vits_attention_desc* d, const float* q, const float* k, const float* v, const float* rel_k, const float* rel_v,
                               const uint16_t* exp_tab, const int32_t* lens, float* out) {
    VITS_TRY
    using namespace vits;
    if (!d || !q || !k || !v || !rel_k || !rel_v || !out) return fail("vits_op_attention: null argument");
    const KernelKnobs defaults;
    KernelKnobsScope scope(&defaults);
    AttOpPlan r;
    std::string why;
    if (!attention_resolve(d, r, why)) return fail(why.c_str());
    const int B = d->batch, C = d->heads * d->head_dim, T = d->t, ts = d->t_stride;
    if (!op_lens_ok(lens, B, T)) return fail("vits_op_attention: 0 <= lens[b] <= t <= t_stride is required");
    const size_t nr = (size_t)(2 * d->window + 1) * d->head_dim;
    DevBytes dq, dk, dv, dout, drk, drv, dtab;
    DevInts dl;
    if (!stage_ff(dq, q, B, C, ts, ts, lens, T) || !stage_ff(dk, k, B, C, ts, ts, lens, T) || !stage_ff(dv, v, B, C, ts, ts, lens, T) || !stage_ff(dout, nullptr, B, C, ts, ts, lens, T) ||
        !drk.put(rel_k, nr * 4) || !drv.put(rel_v, nr * 4) || !dl.put(lens, B) || (exp_tab && !dtab.put(exp_tab, 65536 * 2)))
        return fail("device allocation failed");
    GgmlTables tabs;
    tabs.exp = exp_tab ? dtab.h() : nullptr;
    hipError_t e = launch_rel_attention(tref(dq.f(), C, ts), tref(dk.f(), C, ts), tref(dv.f(), C, ts), drk.f(), drv.f(), tref(dout.f(), C, ts), dl.p, B, d->heads, d->head_dim, T,
                                        d->window, d->q_scale, nullptr, tabs, r.variant);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail((std::string("vits_op_attention: ") + r.kernel + ": " + hipGetErrorString(e)).c_str());
    if (hipMemcpy(out, dout.p, (size_t)B * C * ts * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail("copy back failed");
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_op_layer_norm_plan(const vits_layer_norm_desc* d, vits_layer_norm_plan* out) {
    VITS_TRY
    if (!d || !out) return fail("vits_op_layer_norm_plan: null argument");
    const vits::KernelKnobs defaults;
    vits::KernelKnobsScope scope(&defaults);
    vits::LayerNormPlan p;
    std::string why;
    if (!layer_norm_resolve(d, false, p, why)) return fail(why.c_str());
    std::memset(out, 0, sizeof(*out));
    std::snprintf(out->kernel, sizeof(out->kernel), "add_layer_norm_kernel<%d>", p.tw);
    out->tw = p.tw, out->grid_x = p.gx, out->grid_y = p.gy, out->block = p.block, out->lds = (int64_t)p.lds;
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_op_layer_norm(const vits_layer_norm_desc* d, const float* x, const float* residual, const float* gamma, const float* beta, const uint16_t* gelu_tab,
                                const int32_t* lens, float* y) {
    VITS_TRY
    using namespace vits;
    if (!d || !x || !gamma || !beta || !y) return fail("vits_op_layer_norm: null argument");
    const KernelKnobs defaults;
    KernelKnobsScope scope(&defaults);
    LayerNormPlan p;
    std::string why;
    if (!layer_norm_resolve(d, gelu_tab != nullptr, p, why)) return fail(why.c_str());
    const int B = d->batch, C = d->channels, T = d->t, ts = d->t_stride;
    if (!op_lens_ok(lens, B, T)) return fail("vits_op_layer_norm: 0 <= lens[b] <= t <= t_stride is required");
    DevBytes dx, dr, dy, dg, db, dtab;
    DevInts dl;
    if (!stage_ff(dx, x, B, C, ts, ts, lens, T) || (residual && !stage_ff(dr, residual, B, C, ts, ts, lens, T)) || !stage_ff(dy, d->add_to ? y : nullptr, B, C, ts, ts, lens, T) ||
        !dg.put(gamma, (size_t)C * 4) || !db.put(beta, (size_t)C * 4) || !dl.put(lens, B) || (gelu_tab && !dtab.put(gelu_tab, 65536 * 2)))
        return fail("device allocation failed");
    GgmlTables tabs;
    tabs.gelu = gelu_tab ? dtab.h() : nullptr;
    TensorRef none;
    const TensorRef yr = tref(dy.f(), C, ts);
    hipError_t e = launch_add_layer_norm(tref(dx.f(), C, ts), residual ? tref(dr.f(), C, ts) : none, dg.f(), db.f(), d->add_to ? none : yr, dl.p, B, C, T, d->eps, d->post_gelu,
                                         d->add_to ? yr : none, nullptr, tabs, p.tw);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail((std::string("vits_op_layer_norm: ") + hipGetErrorString(e)).c_str());
    if (hipMemcpy(y, dy.p, (size_t)B * C * ts * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail("copy back failed");
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_op_norm_conv_plan(const vits_norm_conv_desc* d, vits_norm_conv_plan* out) {
    VITS_TRY
    if (!d || !out) return fail("vits_op_norm_conv_plan: null argument");
    const vits::KernelKnobs defaults;
    vits::KernelKnobsScope scope(&defaults);
    NormConvOpPlan r;
    std::string why;
    if (!norm_conv_resolve(d, g_op_arith, r, why)) return fail(why.c_str());
    std::memset(out, 0, sizeof(*out));
    std::snprintf(out->tile, sizeof(out->tile), "%s", conv_tile_name(r.cp.tile));
    std::snprintf(out->ln_why, sizeof(out->ln_why), "%s", r.ln_why.c_str());
    out->variant = r.variant, out->pitch = r.pitch, out->ln_ok = r.ln_ok ? 1 : 0, out->launches = r.launches;
    out->grid_x = r.cp.gx, out->grid_y = r.cp.gy, out->grid_z = r.cp.gz, out->block = r.cp.block, out->lds = (int64_t)r.cp.lds;
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_op_norm_conv(const vits_norm_conv_desc* d, const float* x, const float* gamma, const float* beta, const float* w, const float* bias,
                               const float* residual, const int32_t* lens, float* y, float* ln_out) {
    VITS_TRY
    using namespace vits;
    if (!d || !x || !gamma || !beta || !w || !y || !ln_out) return fail("vits_op_norm_conv: null argument (bias and residual alone are optional)");
    const KernelKnobs defaults;
    KernelKnobsScope scope(&defaults);
    NormConvOpPlan r;
    std::string why;
    if (!norm_conv_resolve(d, g_op_arith, r, why)) return fail(why.c_str());
    const int B = d->batch, cin = d->cin, cout = d->cout, T = d->t, ts = d->t_stride, P = r.pitch;
    if (!op_lens_ok(lens, B, T)) return fail("vits_op_norm_conv: 0 <= lens[b] <= t <= t_stride is required");
    PackedConv& pc = r.pc;
    DevBytes dw, dwl, dbias, dg, dbe, dx, dln, dy, dres;
    DevInts dl;
    {
        const std::vector<float> packed = pack_conv_weights(w, cout, cin, d->k, EPI_STD, 0, &pc.rows, &pc.mtiles_used, &pc.mtiles, &pc.nchunks);
        if (!dw.put(packed.data(), packed.size() * 4)) return fail("device allocation failed");
        pc.wp = dw.f(), pc.bytes = (int64_t)packed.size() * 4;
        if (pc.wp_l16) {
            const std::vector<float> pl = repack_conv_weights_l16(packed, pc.mtiles, pc.nchunks, d->k);
            if (!dwl.put(pl.data(), pl.size() * 4)) return fail("device allocation failed");
            pc.wp_l16 = dwl.f();
        }
    }
    if ((bias && !dbias.put(bias, (size_t)cout * 4)) || !dg.put(gamma, (size_t)cin * 4) || !dbe.put(beta, (size_t)cin * 4) || !dl.put(lens, B) ||
        !stage_ff(dx, x, B, cin, ts, P, lens, T) || !stage_ff(dln, nullptr, B, cin, ts, P, lens, T) || !stage_ff(dy, nullptr, B, cout, ts, P, lens, T) ||
        (residual && !stage_ff(dres, residual, B, cout, ts, P, lens, T)))
        return fail("device allocation failed");
    pc.bias = bias ? dbias.f() : nullptr;
    ConvCall plain, fused;
    norm_conv_calls(d, dl.p, plain, fused);
    const TensorRef xr = tref(dx.f(), cin, P), lnr = tref(dln.f(), cin, P);
    plain.y = fused.y = tref(dy.f(), cout, P);
    if (residual) plain.res = fused.res = tref(dres.f(), cout, P);
    hipError_t e;
    if (r.variant == 2) {  // Engine::run_text_encoder's conv_of_norm: the un-normalised tensor in, the normalised one out of the conv's first row group
        fused.x = xr, fused.ln_gamma = dg.f(), fused.ln_beta = dbe.f(), fused.ln_out = lnr;
        e = launch_conv(pc, fused, nullptr);
    } else {  // its fallback: norm_now, then the conv on the normalised tensor
        TensorRef none;
        e = launch_add_layer_norm(xr, none, dg.f(), dbe.f(), lnr, dl.p, B, cin, T, d->eps, 0, none, nullptr);
        plain.x = lnr;
        if (e == hipSuccess) e = launch_conv(pc, plain, nullptr);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail((std::string("vits_op_norm_conv: variant ") + std::to_string(r.variant) + ": " + hipGetErrorString(e)).c_str());
    auto back = [&](const DevBytes& src, int rows, float* dst) {  // columns [0, t) of every row, as the device holds them
        return hipMemcpy2D(dst, (size_t)ts * 4, src.p, (size_t)P * 4, (size_t)T * 4, (size_t)B * rows, hipMemcpyDeviceToHost) == hipSuccess;
    };
    if (!back(dy, cout, y) || !back(dln, cin, ln_out)) return fail("copy back failed");
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_op_duration_predictor(const vits_duration_predictor_desc* d, const float* x, const float* w1, const float* b1, const float* g1, const float* be1,
                                        const float* w2, const float* b2, const float* g2, const float* be2, const float* wp, const float* bp, const float* spk_rows,
                                        const int32_t* lens, float* logw) {
    VITS_TRY
    using namespace vits;
    if (!d || !x || !w1 || !b1 || !g1 || !be1 || !w2 || !b2 || !g2 || !be2 || !wp || !bp || !logw) return fail("vits_op_duration_predictor: null argument");
    const int B = d->batch, H = d->hidden, Fc = d->filter, T = d->t, ts = d->t_stride, k = d->k;
    if (B < 1 || H < 1 || Fc < 1 || T < 1 || ts < T || k < 1 || !(k & 1)) return fail("vits_op_duration_predictor: batch, hidden, filter, t >= 1, t <= t_stride and an odd k are required");
    if (d->variant < 0 || d->variant > 3) return fail("vits_op_duration_predictor: variant 0 (planner), 1 (16-token tile), 2 (wide tile) or 3 (un-fused)");
    if (!split_lens_ok(lens, B, T, ts)) return fail("vits_op_duration_predictor: 0 <= lens[b] <= t <= t_stride is required");
    const DpDetPlan plan = plan_dp_det(H, Fc, k, B, T, d->variant);
    if ((d->variant == 1 || d->variant == 2) && !plan.ok)
        return fail(("vits_op_duration_predictor: the fused kernel has no instantiation for hidden " + std::to_string(H) + ", filter " + std::to_string(Fc) + ", k " + std::to_string(k) +
                     " (variant " + std::to_string(d->variant) + " never falls back)").c_str());
    // x behind every utterance's length is NaN on the device: a read past an utterance shows in the result
    const size_t nx = (size_t)B * H * ts;
    std::vector<float> xs(nx, std::numeric_limits<float>::quiet_NaN());
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < H; ++c) std::memcpy(&xs[((size_t)b * H + c) * ts], x + ((size_t)b * H + c) * ts, sizeof(float) * (size_t)(lens ? lens[b] : T));
    struct Conv {
        PackedConv pc;
        DevBuf w, wl, b;
    } cv[3];
    auto upload = [&](Conv& c, const float* w, const float* bias, int cout, int cin, int taps) {
        PackedConv& pc = c.pc;
        pc.cin = cin, pc.cout = cout, pc.kt = taps, pc.epi = EPI_STD;
        const std::vector<float> packed = pack_conv_weights(w, cout, cin, taps, EPI_STD, 0, &pc.rows, &pc.mtiles_used, &pc.mtiles, &pc.nchunks);
        const std::vector<float> pl = repack_conv_weights_l16(packed, pc.mtiles, pc.nchunks, taps);
        if (!c.w.put(packed.data(), packed.size()) || !c.wl.put(pl.data(), pl.size()) || !c.b.put(bias, cout)) return false;
        pc.wp = c.w.p, pc.wp_l16 = c.wl.p, pc.bias = c.b.p;
        pc.bytes = (int64_t)packed.size() * 4;
        return true;
    };
    DevBuf dx, dg1, dbe1, dg2, dbe2, drows, dlogw, dxp, da, db;
    DevInts dl;
    if (!upload(cv[0], w1, b1, Fc, H, k) || !upload(cv[1], w2, b2, Fc, Fc, k) || !upload(cv[2], wp, bp, 1, Fc, 1) || !dx.put(xs.data(), nx) || !dg1.put(g1, Fc) || !dbe1.put(be1, Fc) ||
        !dg2.put(g2, Fc) || !dbe2.put(be2, Fc) || !dlogw.put(logw, (size_t)B * ts) || !dl.put(lens, B) || (spk_rows && !drows.put(spk_rows, (size_t)B * H)))
        return fail("device allocation failed");
    DpDetCall c;
    c.x = tref(dx.p, H, ts);
    c.logw = tref(dlogw.p, 1, ts);
    c.c1 = &cv[0].pc, c.c2 = &cv[1].pc, c.proj = &cv[2].pc;
    c.g1 = dg1.p, c.be1 = dbe1.p, c.g2 = dg2.p, c.be2 = dbe2.p;
    if (spk_rows) c.rows = drows.p, c.row_rs = H;  // (row b for utterance b)
    c.lens = dl.p;
    c.batch = B, c.hidden = H, c.filter = Fc, c.tmax = T, c.k = k;
    c.eps = d->eps;
    c.variant = d->variant == 3 ? 0 : d->variant;
    hipError_t e = hipSuccess;
    if (plan.ok) {
        e = launch_dp_det(c, nullptr);
    } else {
        // the un-fused sequence: the function Engine::run_duration_predictor_det calls
        const size_t na = (size_t)B * Fc * ts;
        if (!da.put(nullptr, na) || !db.put(nullptr, na) || (spk_rows && !dxp.put(nullptr, nx))) return fail("device allocation failed");
        e = launch_dp_det_unfused(c, spk_rows ? tref(dxp.p, H, ts) : TensorRef(), tref(da.p, Fc, ts), tref(db.p, Fc, ts), nullptr);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(hipGetErrorString(e));
    if (hipMemcpy(logw, dlogw.p, (size_t)B * ts * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail("copy back failed");
    return 0;
    VITS_CATCH(-1)
}

// ---- vits_op_dds_block: which kernels a descriptor names (host arithmetic only: launch_plan.h), then the engine's launch sequences on staged tensors --------
namespace {
struct DdsOpPlan {
    int variant = 0, nt = 0, launches = 0;
    std::string kernel, kernel_last;
    int halo[8] = {0}, dil[8] = {0};
    size_t lds[8] = {0};
    vits::LaunchGrid g;
};
bool dds_fail(std::string& why, const std::string& m) {
    why = "vits_op_dds_block: " + m;
    return false;
}
bool dds_resolve(const vits_dds_block_desc* d, int arith, DdsOpPlan& r, std::string& why) {
    using namespace vits;
    if (arith != VITS_ARITH_F32 && arith != VITS_ARITH_F16 && arith != VITS_ARITH_BF16)
        return dds_fail(why, "VITS_ARITH_F32, VITS_ARITH_F16 or VITS_ARITH_BF16 only (the split arithmetic has no DDS kernels)");
    const int H = d->channels, k = d->k, B = d->batch, T = d->t, NL = d->layers;
    if (B < 1 || T < 1 || d->t_stride < T) return dds_fail(why, "batch >= 1 and 1 <= t <= t_stride are required");
    if (H < 1) return dds_fail(why, "channels = " + std::to_string(H) + ": at least 1");
    if (k < 1 || k > 64) return dds_fail(why, "k = " + std::to_string(k) + ": 1 to 64 taps");
    if (NL < 1 || NL > 8) return dds_fail(why, "layers = " + std::to_string(NL) + ": 1 to 8 layers");
    if (!(d->eps > 0.f)) return dds_fail(why, "eps must be positive");
    if (d->variant < 0 || d->variant > 3)
        return dds_fail(why, "variant " + std::to_string(d->variant) + ": 0 (the engine's choice), 1 (three launches per layer), 2 (dds_layer_kernel), 3 (dds_layer_lat_kernel)");
    if (d->head < 0 || d->head > 2) return dds_fail(why, "head " + std::to_string(d->head) + ": 0 (none), 1 (1 -> H conv of a latent row + conditioning), 2 (H -> H 1x1 conv)");
    if (d->tail < 0 || d->tail > 1) return dds_fail(why, "tail " + std::to_string(d->tail) + ": 0 (none) or 1 (a tail_rows x H 1x1 projection)");
    if (d->tail == 1 && d->tail_rows < 1) return dds_fail(why, "tail_rows = " + std::to_string(d->tail_rows) + ": at least 1");
    if (d->head == 1 && d->zc != 0 && d->zc != 1) return dds_fail(why, "zc = " + std::to_string(d->zc) + ": latent row 0 or 1");
    if (d->head == 2 && d->n_bias_rows < 1) return dds_fail(why, "n_bias_rows = " + std::to_string(d->n_bias_rows) + ": the head conv's bias table has at least one row");
    int64_t dl = 1;
    for (int i = 0; i < NL; ++i, dl *= k) {
        if (dl * (k - 1) > 8192) return dds_fail(why, "layer " + std::to_string(i) + ": dilation " + std::to_string(dl) + " is out of range");
        r.dil[i] = (int)dl;
        r.halo[i] = (int)((k * dl - dl) / 2);
    }
    const bool f32 = arith == VITS_ARITH_F32;
    // why dds_layer_kernel (lat false) / dds_layer_lat_kernel (lat true) has no instantiation for this block, or ""
    auto refusal = [&](bool lat) -> std::string {
        const char* fam = lat ? "dds_layer_lat_kernel" : "dds_layer_kernel";
        if (lat && !f32) return std::string("variant 3: ") + fam + " exists in fp32 only";
        if (H < 32 || (H & 31) || H > 256)
            return std::string("no ") + fam + " for channels = " + std::to_string(H) + " (32 to 256 in steps of 32)";
        for (int i = 0; i < NL; ++i) {
            const std::string at = "layer " + std::to_string(i) + " (k = " + std::to_string(k) + ", dilation " + std::to_string(r.dil[i]) + "): ";
            if ((k * r.dil[i] - r.dil[i]) & 1) return at + "(k - 1) * dilation is odd: no symmetric halo for " + fam;
            const size_t lds = lat ? dds_lat_lds(H, k, r.dil[i], true, H) : dds_layer_lds(H, k, r.dil[i]);
            if (lds > kLdsSoft) return at + fam + " needs " + std::to_string(lds) + " bytes of LDS, the limit is " + std::to_string(kLdsSoft);
            if (!(lat ? plan_dds_layer_lat(H, k, r.dil[i], true, B, T).ok : plan_dds_layer(H, k, r.dil[i], B, T).ok)) return at + "the planner refuses " + fam;
        }
        if (lat && d->tail == 1 && d->tail_rows > H) return "variant 3: tail_rows = " + std::to_string(d->tail_rows) + " exceeds channels = " + std::to_string(H);
        return "";
    };
    int v = d->variant;
    if (v == 0)  // Engine::dds_lat_ok, then Engine::run_dds
        v = f32 && NL >= 2 && dds_lat_grid_ok(B, T) && refusal(true).empty() ? 3 : NL >= 2 && refusal(false).empty() ? 2 : 1;
    r.variant = v;
    const int ends = (d->head ? 1 : 0) + (d->tail ? 1 : 0);
    char name[96];
    if (v == 1) {
        for (int i = 0; i < NL; ++i) {
            const LaunchGrid g = plan_dds_depthwise(H, k, r.dil[i], B, T);
            r.lds[i] = dds_depthwise_lds(H, k, r.dil[i]);
            if (!g.ok)
                return dds_fail(why, "variant 1: layer " + std::to_string(i) + ": dds_depthwise_kernel needs " + std::to_string(r.lds[i]) + " bytes of LDS, the limit is " +
                                         std::to_string(kLdsSoft));
            if (i == 0) r.g = g;
        }
        if (!plan_add_layer_norm(H, B, T).ok) return dds_fail(why, "variant 1: add_layer_norm_kernel has no tile for channels = " + std::to_string(H));
        r.kernel = r.kernel_last = "dds_depthwise_kernel";
        r.nt = 64, r.launches = 3 * NL + ends;
        return true;
    }
    const std::string no = refusal(v == 3);
    if (!no.empty()) return dds_fail(why, (no.rfind("variant", 0) == 0 ? "" : "variant " + std::to_string(v) + ": ") + no);
    if (v == 2) {
        const DdsLayerPlan pl = plan_dds_layer(H, k, 1, B, T);
        std::snprintf(name, sizeof(name), "dds_layer_kernel<%d, %d>", arith, pl.m);
        r.kernel = r.kernel_last = name;
        for (int i = 0; i < NL; ++i) r.lds[i] = dds_layer_lds(H, k, r.dil[i]);
        r.g = pl, r.nt = 32, r.launches = NL + ends;
        return true;
    }
    const DdsLayerPlan pl = plan_dds_layer_lat(H, k, 1, d->head == 2, B, T);
    std::snprintf(name, sizeof(name), "dds_layer_lat_kernel<%d, %d, %d>", d->head, NL == 1 ? d->tail : 0, pl.m);
    r.kernel = name;
    std::snprintf(name, sizeof(name), "dds_layer_lat_kernel<%d, %d, %d>", NL == 1 ? d->head : 0, d->tail, pl.m);
    r.kernel_last = name;
    for (int i = 0; i < NL; ++i) r.lds[i] = dds_lat_lds(H, k, r.dil[i], i == 0 && d->head == 2, H);
    r.g = pl, r.nt = kLatNT, r.launches = NL;
    return true;
}
}  // namespace

VITS_API int vits_op_dds_block_plan(const vits_dds_block_desc* d, vits_dds_block_plan* out) {
    VITS_TRY
    if (!d || !out) return fail("vits_op_dds_block_plan: null argument");
    DdsOpPlan r;
    std::string why;
    if (!dds_resolve(d, g_op_arith, r, why)) return fail(why.c_str());
    std::memset(out, 0, sizeof(*out));
    std::snprintf(out->kernel, sizeof(out->kernel), "%s", r.kernel.c_str());
    std::snprintf(out->kernel_last, sizeof(out->kernel_last), "%s", r.kernel_last.c_str());
    out->variant = r.variant, out->nt = r.nt, out->layers = d->layers, out->launches = r.launches;
    for (int i = 0; i < d->layers; ++i) out->halo[i] = r.halo[i], out->lds[i] = (int64_t)r.lds[i];
    out->grid_x = r.g.gx, out->grid_y = r.g.gy, out->block = r.g.block;
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_op_dds_block(const vits_dds_block_desc* d, const float* x, const float* z, const float* cond, const float* head_w, const float* head_b,
                               const int32_t* bias_rows, const float* dw_w, const float* dw_b, const float* g1, const float* b1, const float* pw_w,
                               const float* pw_b, const float* g2, const float* b2, const float* tail_w, const float* tail_b, const int32_t* lens, float* y,
                               float* y2) {
    VITS_TRY
    using namespace vits;
    if (!d || !dw_w || !dw_b || !g1 || !b1 || !pw_w || !pw_b || !g2 || !b2) return fail("vits_op_dds_block: null argument (every per-layer parameter is required)");
    const int arith = g_op_arith;
    DdsOpPlan r;
    std::string why;
    if (!dds_resolve(d, arith, r, why)) return fail(why.c_str());
    const int B = d->batch, H = d->channels, T = d->t, ts = d->t_stride, k = d->k, NL = d->layers, TR = d->tail ? d->tail_rows : 0;
    if (d->head != 1 && !x) return fail("vits_op_dds_block: x is required with head 0 and head 2");
    if (d->head == 1 && (!z || !cond)) return fail("vits_op_dds_block: z and cond are required with head 1");
    if (d->head && (!head_w || !head_b)) return fail("vits_op_dds_block: head_w and head_b are required with a head");
    if (d->tail && (!tail_w || !tail_b || !y2)) return fail("vits_op_dds_block: tail_w, tail_b and y2 are required with a tail");
    if (!d->tail && !y) return fail("vits_op_dds_block: y is required without a tail");
    for (int b = 0; b < B; ++b) {
        if (lens && (lens[b] < 0 || lens[b] > T)) return fail("vits_op_dds_block: 0 <= lens[b] <= t is required");
        if (d->head == 2 && bias_rows && (bias_rows[b] < 0 || bias_rows[b] >= d->n_bias_rows)) return fail("vits_op_dds_block: 0 <= bias_rows[b] < n_bias_rows is required");
    }
    const bool f32 = arith == VITS_ARITH_F32;
    struct Conv {
        PackedConv pc;
        DevBytes w, wl, w16, b;
    };
    auto upload = [&](Conv& c, const float* w, const float* bias, size_t bias_n, int cout, int cin) {
        PackedConv& pc = c.pc;
        pc.cin = cin, pc.cout = cout, pc.kt = 1, pc.epi = EPI_STD;
        const std::vector<float> packed = pack_conv_weights(w, cout, cin, 1, EPI_STD, 0, &pc.rows, &pc.mtiles_used, &pc.mtiles, &pc.nchunks);
        if (!c.b.put(bias, bias_n * 4)) return false;
        pc.bias = c.b.f();
        if (f32) {
            if (!c.w.put(packed.data(), packed.size() * 4)) return false;
            pc.wp = c.w.f(), pc.bytes = (int64_t)packed.size() * 4;
            const std::vector<float> pl = repack_conv_weights_l16(packed, pc.mtiles, pc.nchunks, 1);
            if (!c.wl.put(pl.data(), pl.size() * 4)) return false;
            pc.wp_l16 = c.wl.f();
        } else {
            const std::vector<uint16_t> p16 = pack_conv_weights16(w, cout, cin, 1, EPI_STD, 0, arith);
            if (!c.w16.put(p16.data(), p16.size() * 2)) return false;
            pc.wp16 = c.w16.h(), pc.bytes16 = (int64_t)p16.size() * 2;
        }
        return true;
    };
    std::vector<Conv> pw(NL);
    Conv hconv, tconv;
    DevBytes ddw_w, ddw_b, dg1, db1, dg2, db2, dhw, dhb;
    const size_t nlh = (size_t)NL * H;
    if (!ddw_w.put(dw_w, nlh * k * 4) || !ddw_b.put(dw_b, nlh * 4) || !dg1.put(g1, nlh * 4) || !db1.put(b1, nlh * 4) || !dg2.put(g2, nlh * 4) || !db2.put(b2, nlh * 4))
        return fail("device allocation failed");
    for (int i = 0; i < NL; ++i)
        if (!upload(pw[i], pw_w + (size_t)i * H * H, pw_b + (size_t)i * H, H, H, H)) return fail("device allocation failed");
    if (d->head == 1 && (!dhw.put(head_w, (size_t)H * 4) || !dhb.put(head_b, (size_t)H * 4))) return fail("device allocation failed");
    if (d->head == 2) {
        if (!upload(hconv, head_w, head_b, (size_t)d->n_bias_rows * H, H, H)) return fail("device allocation failed");
        hconv.pc.bias_rs = bias_rows ? H : 0;
    }
    if (d->tail && !upload(tconv, tail_w, tail_b, TR, TR, H)) return fail("device allocation failed");
    // host staging: NaN everywhere, then the valid columns; buffers nobody uploads into are NaN bytes
    auto len_of = [&](int b) { return lens ? lens[b] : T; };
    auto stage = [&](DevBytes& dst, const float* src, int rows) {
        const size_t n = (size_t)B * rows * ts;
        std::vector<float> h(n);
        std::memset(h.data(), 0xFF, n * 4);
        for (int b = 0; src && b < B; ++b)
            for (int c = 0; c < rows; ++c) std::memcpy(&h[((size_t)b * rows + c) * ts], src + ((size_t)b * rows + c) * ts, sizeof(float) * (size_t)len_of(b));
        return dst.put(h.data(), n * 4);
    };
    DevInts dl, dspk;
    DevBytes dx, da, dbb, dc, dz, dcond, dy2, dx16;
    if (!dl.put(lens, B) || !dspk.put(d->head == 2 ? bias_rows : nullptr, B)) return fail("device allocation failed");
    if (!stage(dx, d->head == 1 ? nullptr : x, H) || !stage(da, nullptr, H) || !stage(dbb, nullptr, H) || !stage(dc, nullptr, H)) return fail("device allocation failed");
    if (d->head == 1 && (!stage(dz, z, 2) || !stage(dcond, cond, H))) return fail("device allocation failed");
    if (d->tail && !stage(dy2, nullptr, TR)) return fail("device allocation failed");
    const size_t x16_bytes = f32 ? 0 : (size_t)B * (H / 8 + 1) * round_up(T, 8) * 8 * 2;
    if (!f32 && !dx16.fill(x16_bytes, 0xFF)) return fail("device allocation failed");
    // a conv of the fp32-layout orchestration (Engine::conv): the fp32 kernel, or the converter + the 16-bit-operand kernel (Engine::conv16_transparent)
    auto conv = [&](const PackedConv& w, TensorRef xin, TensorRef yout) -> hipError_t {
        ConvCall c;
        c.x = xin, c.y = yout, c.len_in = c.len_out = dl.p, c.spk = dspk.p, c.batch = B, c.t_in = c.t_out = T;
        if (f32) return launch_conv(w, c, nullptr);
        Ref16 x16;
        x16.p = dx16.h(), x16.ts = round_up(T, 8), x16.bs = (int64_t)((w.cin + 7) / 8) * x16.ts * 8;
        if (hipMemsetAsync(dx16.p, 0xFF, x16_bytes, nullptr) != hipSuccess) return hipErrorUnknown;
        hipError_t e2 = launch_to_group16(c.x, c.len_in, B, w.cin, T, 1.0f, x16, arith, nullptr);
        if (e2 != hipSuccess) return e2;
        Conv16Call q;
        q.x = x16, q.len_in = c.len_in, q.len_out = c.len_out, q.spk = c.spk, q.batch = B, q.t_in = q.t_out = T, q.y = c.y;
        return launch_conv16(w, q, arith, nullptr);
    };
    const TensorRef xin = tref(dx.f(), H, ts), ba = tref(da.f(), H, ts), bb = tref(dbb.f(), H, ts), bc = tref(dc.f(), H, ts);
    const TensorRef zr = tref(dz.f(), 2, ts), cr = tref(dcond.f(), H, ts), y2r = tref(dy2.f(), std::max(TR, 1), ts);
    auto lw = [&](const DevBytes& p, int i, int per) { return p.f() + (size_t)i * H * per; };
    TensorRef none, out;  // out: where the block's output lies
    hipError_t e = hipSuccess;
    if (r.variant == 3) {
        // Engine::run_dds_lat: a, b ping-pong; the last layer writes the output buffer (or, with a tail, only y2)
        TensorRef src;
        out = d->tail ? none : bc;
        for (int i = 0; i < NL && e == hipSuccess; ++i) {
            DdsLatCall c;
            c.dw_w = lw(ddw_w, i, k), c.dw_b = lw(ddw_b, i, 1), c.g1 = lw(dg1, i, 1), c.b1 = lw(db1, i, 1), c.g2 = lw(dg2, i, 1), c.b2 = lw(db2, i, 1);
            c.pw = &pw[i].pc;
            c.lens = dl.p;
            c.batch = B, c.channels = H, c.tmax = T, c.k = k, c.dil = r.dil[i];
            c.eps = d->eps;
            if (i == 0) {
                if (d->head == 1) c.head_w = dhw.f(), c.head_b = dhb.f(), c.z = zr, c.cond = cr, c.zc = d->zc;
                else if (d->head == 2) c.head_conv = &hconv.pc, c.x = xin, c.spk = dspk.p;
                else c.x = xin;
            } else
                c.x = src;
            const TensorRef dst = src.p == ba.p ? bb : ba;
            if (i == NL - 1 && d->tail) c.tail_conv = &tconv.pc, c.y2 = y2r;
            else c.y = i == NL - 1 ? bc : dst;
            e = launch_dds_layer_lat(c, nullptr);
            src = dst;
        }
    } else {
        // head as its own launch, then Engine::run_dds on (x, y, p) = (cur, ba, bb), then the tail conv
        TensorRef cur = xin;
        if (d->head == 1) {
            cur = bc;
            e = launch_pointwise_from1(zr, d->zc, dhw.f(), dhb.f(), cr, cur, dl.p, B, H, T, nullptr, arith);
        } else if (d->head == 2) {
            cur = bc;
            e = conv(hconv.pc, xin, cur);
        }
        out = cur;
        if (r.variant == 2) {
            TensorRef src = cur;
            for (int i = 0; i < NL && e == hipSuccess; ++i) {
                // (Engine::run_dds takes this path from two layers on, so that the last layer can write x again; one layer writes y here)
                const TensorRef dst = NL == 1 ? ba : i == NL - 1 ? cur : (src.p == ba.p ? bb : ba);
                e = launch_dds_layer(src, dst, lw(ddw_w, i, k), lw(ddw_b, i, 1), lw(dg1, i, 1), lw(db1, i, 1), pw[i].pc, lw(dg2, i, 1), lw(db2, i, 1), dl.p, B, H, T, k, r.dil[i],
                                     d->eps, arith, nullptr);
                src = dst;
            }
            if (NL == 1) out = ba;
        } else {
            for (int i = 0; i < NL && e == hipSuccess; ++i) {
                e = launch_dds_depthwise(cur, none, lw(ddw_w, i, k), lw(ddw_b, i, 1), lw(dg1, i, 1), lw(db1, i, 1), ba, dl.p, B, H, T, k, r.dil[i], d->eps, nullptr, arith);
                if (e == hipSuccess) e = conv(pw[i].pc, ba, bb);
                if (e == hipSuccess) e = launch_add_layer_norm(bb, none, lw(dg2, i, 1), lw(db2, i, 1), none, dl.p, B, H, T, d->eps, 1, cur, nullptr);
            }
        }
        if (e == hipSuccess && d->tail) e = conv(tconv.pc, out, y2r);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail((std::string("vits_op_dds_block: ") + r.kernel + ": " + hipGetErrorString(e)).c_str());
    if (y) {
        if (out.p) {
            if (hipMemcpy(y, out.p, (size_t)B * H * ts * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail("copy back failed");
        } else
            std::memset(y, 0xFF, (size_t)B * H * ts * 4);
    }
    if (d->tail && hipMemcpy(y2, dy2.p, (size_t)B * TR * ts * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail("copy back failed");
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_op_spline(int32_t batch, int32_t t, int32_t t_stride, int32_t bins, float tail, float inv_sqrt, int32_t mode, int32_t zc, const float* u,
                            float* z, const int32_t* lens) {
    VITS_TRY
    using namespace vits;
    if (!u || !z) return fail("vits_op_spline: null argument");
    if (batch < 1 || t < 1 || t_stride < t) return fail("vits_op_spline: batch >= 1 and 1 <= t <= t_stride are required");
    if (bins < 1 || bins > 16) return fail(("vits_op_spline: bins = " + std::to_string(bins) + ": spline_kernel takes 1 to 16 bins").c_str());
    if (t > 4096) return fail(("vits_op_spline: t = " + std::to_string(t) + ": spline_kernel takes at most 4096 tokens").c_str());
    if (mode != VITS_MODE_HF && mode != VITS_MODE_REFERENCE) return fail("vits_op_spline: mode is VITS_MODE_HF or VITS_MODE_REFERENCE");
    if (zc != 0 && zc != 1) return fail("vits_op_spline: zc is latent row 0 or 1");
    if (!(tail > 0.f)) return fail("vits_op_spline: tail must be positive");
    if (!split_lens_ok(lens, batch, t, t_stride)) return fail("vits_op_spline: 0 <= lens[b] <= t <= t_stride is required");
    const int rows = 3 * bins - 1;
    const size_t nu = (size_t)batch * rows * t_stride, nz = (size_t)batch * 2 * t_stride;
    std::vector<float> hu(nu);
    std::memset(hu.data(), 0xFF, nu * 4);
    for (int b = 0; b < batch; ++b)
        for (int c = 0; c < rows; ++c)
            std::memcpy(&hu[((size_t)b * rows + c) * t_stride], u + ((size_t)b * rows + c) * t_stride, sizeof(float) * (size_t)(lens ? lens[b] : t));
    DevBytes du, dz;
    DevInts dl;
    if (!du.put(hu.data(), nu * 4) || !dz.put(z, nz * 4) || !dl.put(lens, batch)) return fail("device allocation failed");
    hipError_t e = launch_spline(tref(du.f(), rows, t_stride), tref(dz.f(), 2, t_stride), zc, dl.p, batch, t, bins, tail, inv_sqrt, mode, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail((std::string("vits_op_spline: ") + hipGetErrorString(e)).c_str());
    if (hipMemcpy(z, dz.p, nz * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail("copy back failed");
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_op_durations(int32_t batch, int32_t rows, int32_t row, int32_t t_stride, const float* logw, const int32_t* lens, float length_scale,
                               const float* length_scales, const int32_t* ovr, int32_t fixed, int32_t n_stage, const int32_t* stage_mul,
                               const int32_t* stage_add, float* dur, int32_t* cum, int32_t* frames, int32_t* stage_lens) {
    VITS_TRY
    using namespace vits;
    if (!logw || !dur || !cum || !frames) return fail("vits_op_durations: null argument");
    if (batch < 1 || rows < 1 || row < 0 || row >= rows || t_stride < 1) return fail("vits_op_durations: batch, rows, t_stride >= 1 and 0 <= row < rows are required");
    if (n_stage < 0 || n_stage > 16 || (n_stage && (!stage_mul || !stage_add || !stage_lens))) return fail("vits_op_durations: 0 to 16 stages, each with a multiplier and an addend");
    if (!split_lens_ok(lens, batch, t_stride, t_stride)) return fail("vits_op_durations: 0 <= lens[b] <= t_stride is required");
    const size_t nt = (size_t)batch * t_stride;
    DevBytes dlogw, dls, dovr, ddur, dcum, dfr, dsl, dmul, dadd;
    DevInts dl;
    if (!dlogw.put(logw, nt * rows * 4) || !dl.put(lens, batch) || !ddur.fill(nt * 4, 0xFF) || !dcum.fill(nt * 4, 0xFF) || !dfr.fill((size_t)batch * 4, 0xFF) ||
        !dsl.fill((size_t)std::max(n_stage, 1) * batch * 4, 0xFF) || (length_scales && !dls.put(length_scales, (size_t)batch * 4)) || (ovr && !dovr.put(ovr, nt * 4)) ||
        (n_stage && (!dmul.put(stage_mul, (size_t)n_stage * 4) || !dadd.put(stage_add, (size_t)n_stage * 4))))
        return fail("device allocation failed");
    hipError_t e = launch_durations(tref(dlogw.f(), rows, t_stride), row, dl.p, batch, t_stride, length_scale, dls.f(), static_cast<const int*>(dovr.p), fixed, ddur.f(),
                                    static_cast<int*>(dcum.p), static_cast<int*>(dfr.p), static_cast<int*>(dsl.p), n_stage, static_cast<const int*>(dmul.p),
                                    static_cast<const int*>(dadd.p), nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail((std::string("vits_op_durations: ") + hipGetErrorString(e)).c_str());
    if (hipMemcpy(dur, ddur.p, nt * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(cum, dcum.p, nt * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(frames, dfr.p, (size_t)batch * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        (n_stage && hipMemcpy(stage_lens, dsl.p, (size_t)n_stage * batch * 4, hipMemcpyDeviceToHost) != hipSuccess))
        return fail("copy back failed");
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_op_align(int32_t batch, const int32_t* T, const int32_t* L, int32_t F, const float* m, const float* ls, const float* z, int32_t* durations,
                           float* scores) {
    VITS_TRY
    using namespace vits;
    if (batch <= 0 || !T || !L || F <= 0 || !m || !ls || !z || !durations) return fail("null argument or empty batch");
    int tmax = 0, lmax = 0;
    for (int b = 0; b < batch; ++b) {
        if (T[b] < 1 || T[b] > L[b]) return fail("vits_op_align: 1 <= T[b] <= L[b] is required");
        tmax = std::max(tmax, T[b]);
        lmax = std::max(lmax, L[b]);
    }
    if (tmax > 4096) return fail("vits_op_align: at most 4096 tokens");
    const int ts = (tmax + 31) / 32 * 32, lstr = (lmax + 31) / 32 * 32;
    const size_t bit_words = align_mas_bits_in_lds(tmax, lmax) ? 0 : align_mas_bits_words(tmax, lmax);
    DevBuf dm, ds, dz, da, dq, dc, dlp, dbits, dscore;
    DevInts dt, dl, ddur;
    if (!dm.put(m, (size_t)batch * F * tmax) || !ds.put(ls, (size_t)batch * F * tmax) || !dz.put(z, (size_t)batch * F * lmax) ||
        !da.put(nullptr, (size_t)batch * 2 * F * ts) || !dq.put(nullptr, (size_t)batch * 2 * F * lstr) || !dc.put(nullptr, (size_t)batch * ts) ||
        !dlp.put(nullptr, (size_t)batch * ts * lstr) || !dbits.put(nullptr, (size_t)batch * bit_words * 2) || !dscore.put(nullptr, batch) || !dt.put(T, batch) ||
        !dl.put(L, batch) || hipMalloc((void**)&ddur.p, (size_t)batch * tmax * 4) != hipSuccess)
        return fail("device allocation failed");
    AlignCall c;
    c.mean = tref(dm.p, F, tmax);
    c.logs = tref(ds.p, F, tmax);
    c.z = tref(dz.p, F, lmax);
    c.tlens = dt.p;
    c.frames = dl.p;
    c.channels = F;
    c.batch = batch;
    c.tmax = tmax;
    c.lmax = lmax;
    c.t_stride = ts;
    c.l_stride = lstr;
    c.plane_a = da.p;
    c.plane_z = dq.p;
    c.ct = dc.p;
    c.logp = dlp.p;
    c.bits = bit_words ? reinterpret_cast<unsigned long long*>(dbits.p) : nullptr;
    c.dur = ddur.p;
    c.dur_stride = tmax;
    c.score = dscore.p;
    hipError_t e = launch_align_logp(c, nullptr);
    if (e == hipSuccess) e = launch_align_mas(c, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(hipGetErrorString(e));
    if (hipMemcpy(durations, ddur.p, (size_t)batch * tmax * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail("copy back failed");
    if (scores && hipMemcpy(scores, dscore.p, (size_t)batch * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail("copy back failed");
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_op_resample(int32_t in_rate, int32_t out_rate, int32_t batch, const float* x, int64_t x_stride, const int64_t* lens, float* y, int64_t y_stride) {
    VITS_TRY
    using namespace vits;
    if (batch <= 0 || !x || !y || x_stride <= 0 || y_stride <= 0) return fail("vits_op_resample: null argument or empty batch");
    ResamplePlan p;
    std::string err;
    if (!resample_plan(in_rate, out_rate, p, err)) return fail(("vits_op_resample: " + err).c_str());
    std::vector<int32_t> n(batch);
    int64_t longest = 0, longest_b = 0;
    for (int b = 0; b < batch; ++b) {
        const int64_t len = lens ? lens[b] : x_stride;
        if (len < 0 || len > x_stride) return fail(("vits_op_resample: lens[" + std::to_string(b) + "] = " + std::to_string(len) + " is outside [0, x_stride = " + std::to_string(x_stride) + "]").c_str());
        if (len > ((int64_t)1 << 30) || p.out_len(len) > INT32_MAX) return fail(("vits_op_resample: row " + std::to_string(b) + " is too long (" + std::to_string(len) + " samples)").c_str());
        n[b] = (int32_t)len;
        if (p.out_len(len) > longest) longest = p.out_len(len), longest_b = b;
    }
    if (y_stride < longest)
        return fail(("vits_op_resample: y_stride = " + std::to_string(y_stride) + " is shorter than the longest output row (row " + std::to_string(longest_b) + ": " +
                     std::to_string(n[longest_b]) + " samples in, " + std::to_string(longest) + " out)").c_str());
    if (p.L == 1 && p.M == 1) {  // equal rates copy
        for (int b = 0; b < batch; ++b) std::memcpy(y + (size_t)b * y_stride, x + (size_t)b * x_stride, sizeof(float) * (size_t)n[b]);
        return 0;
    }
    // taps as the kernel reads them: [K][L]
    const std::vector<float> h = resample_taps(p);
    std::vector<float> ht(h.size());
    for (int ph = 0; ph < p.L; ++ph)
        for (int k = 0; k < p.K; ++k) ht[(size_t)k * p.L + ph] = h[(size_t)ph * p.K + k];
    DevBuf dx, dy, dh;
    DevInts dn;
    // (y goes up too: what lies behind a row's output samples must come back as it was)
    if (!dx.put(x, (size_t)batch * x_stride) || !dy.put(y, (size_t)batch * y_stride) || !dh.put(ht.data(), ht.size()) || !dn.put(n.data(), batch))
        return fail("device allocation failed");
    ResampleCall c;
    c.x = dx.p;
    c.x_stride = x_stride;
    c.lens = dn.p;
    c.y = dy.p;
    c.y_stride = y_stride;
    c.taps = dh.p;
    c.plan = p;
    c.batch = batch;
    c.max_range = longest;
    hipError_t e = launch_resample(c, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(hipGetErrorString(e));
    if (hipMemcpy(y, dy.p, (size_t)batch * y_stride * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail("copy back failed");
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_op_level(const vits_level_desc* d, const float* x, const int64_t* lens, float* y, float* levels) {
    VITS_TRY
    using namespace vits;
    if (!d || !x || !levels || d->batch <= 0 || d->x_stride <= 0 || (y && d->y_stride <= 0)) return fail("vits_op_level: null argument or empty batch");
    if (d->kind == VITS_LEVEL_NONE) return fail("vits_op_level: VITS_LEVEL_NONE measures and applies nothing (use VITS_LEVEL_MEASURE)");
    LoudnessPlan plan;
    std::string err;
    if (!loudness_plan(d->rate, plan, err)) return fail(("vits_op_level: " + err).c_str());
    if (!level_values_ok(d->kind, d->value_db, d->ceiling_db, err)) return fail(("vits_op_level: " + err).c_str());
    const int B = d->batch;
    std::vector<int32_t> n(B);
    int64_t longest = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t len = lens ? lens[b] : d->x_stride;
        if (len < 0 || len > d->x_stride)
            return fail(("vits_op_level: lens[" + std::to_string(b) + "] = " + std::to_string(len) + " is outside [0, x_stride = " + std::to_string(d->x_stride) + "]").c_str());
        if (len > ((int64_t)1 << 30)) return fail(("vits_op_level: row " + std::to_string(b) + " is too long (" + std::to_string(len) + " samples)").c_str());
        n[b] = (int32_t)len;
        longest = std::max(longest, len);
    }
    if (y && d->y_stride < longest) return fail(("vits_op_level: y_stride = " + std::to_string(d->y_stride) + " is shorter than the longest row (" + std::to_string(longest) + " samples)").c_str());
    // the engine's staging: rows at a stride of a multiple of 32 samples, NaN behind every utterance: a read past one shows in the result
    const int64_t xs = (longest + 31) / 32 * 32 + 32;
    std::vector<float> hx((size_t)B * xs, std::numeric_limits<float>::quiet_NaN());
    for (int b = 0; b < B; ++b) std::memcpy(&hx[(size_t)b * xs], x + (size_t)b * d->x_stride, sizeof(float) * (size_t)n[b]);
    const size_t scratch = level_scratch_bytes(B, longest, plan.S);
    DevBuf dx, dy, dlv, dscr;
    DevInts dn;
    // (y goes up too: what lies behind a row's samples must come back as it was)
    if (!dx.put(hx.data(), hx.size()) || !dlv.put(nullptr, (size_t)B * 4) || !dscr.put(nullptr, (scratch + 3) / 4) || !dn.put(n.data(), B) ||
        (y && !dy.put(y, (size_t)B * d->y_stride)))
        return fail("device allocation failed");
    LevelCall c;
    c.x = dx.p;
    c.x_stride = xs;
    c.lens = dn.p;
    c.batch = B;
    c.max_len = longest;
    c.plan = plan;
    c.scratch = dscr.p;
    c.kind = d->kind;
    c.value_db = d->value_db;
    c.ceiling_db = d->ceiling_db;
    c.gain = (float)std::pow(10.0, (double)d->value_db / 20.0);
    c.levels = dlv.p;
    hipError_t e = launch_level_measure(c, nullptr);
    if (e == hipSuccess && y) {
        LevelScale sc;
        sc.x = dx.p;
        sc.x_stride = xs;
        sc.y = dy.p;
        sc.y_stride = d->y_stride;
        sc.lens = dn.p;
        sc.levels = dlv.p;
        sc.batch = B;
        sc.max_range = longest;
        e = launch_level_scale(sc, nullptr);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(hipGetErrorString(e));
    if (hipMemcpy(levels, dlv.p, (size_t)B * 4 * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail("copy back failed");
    if (y && hipMemcpy(y, dy.p, (size_t)B * d->y_stride * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail("copy back failed");
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_op_limit(const vits_limit_desc* ld, const float* x, const int64_t* lens, float* y, float* levels, float* limits) {
    VITS_TRY
    using namespace vits;
    if (!ld || !x || !y || !levels || !limits || ld->level.batch <= 0 || ld->level.x_stride <= 0 || ld->level.y_stride <= 0)
        return fail("vits_op_limit: null argument or empty batch");
    const vits_level_desc* d = &ld->level;
    if (ld->mode != VITS_LIMIT_TRUE_PEAK)
        return fail(ld->mode == VITS_LIMIT_OFF ? "vits_op_limit: VITS_LIMIT_OFF limits nothing (use vits_op_level)" : ("vits_op_limit: unknown mode " + std::to_string(ld->mode)).c_str());
    if (d->kind == VITS_LEVEL_NONE || d->kind == VITS_LEVEL_MEASURE) return fail("vits_op_limit: VITS_LEVEL_NONE and VITS_LEVEL_MEASURE apply nothing: there is nothing to limit");
    LoudnessPlan plan;
    LimiterPlan lplan;
    std::string err;
    if (!limiter_plan(d->rate, lplan, err) || !loudness_plan(d->rate, plan, err)) return fail(("vits_op_limit: " + err).c_str());
    if (!level_values_ok(d->kind, d->value_db, d->ceiling_db, err) || (d->kind == VITS_LEVEL_GAIN && !level_values_ok(VITS_LEVEL_LOUDNESS, 0.f, d->ceiling_db, err)))
        return fail(("vits_op_limit: " + err).c_str());
    const int B = d->batch;
    std::vector<int32_t> n(B);
    int64_t longest = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t len = lens ? lens[b] : d->x_stride;
        if (len < 0 || len > d->x_stride)
            return fail(("vits_op_limit: lens[" + std::to_string(b) + "] = " + std::to_string(len) + " is outside [0, x_stride = " + std::to_string(d->x_stride) + "]").c_str());
        if (len > ((int64_t)1 << 30)) return fail(("vits_op_limit: row " + std::to_string(b) + " is too long (" + std::to_string(len) + " samples)").c_str());
        n[b] = (int32_t)len;
        longest = std::max(longest, len);
    }
    if (d->y_stride < longest) return fail(("vits_op_limit: y_stride = " + std::to_string(d->y_stride) + " is shorter than the longest row (" + std::to_string(longest) + " samples)").c_str());
    // the engine's staging: rows at a stride of a multiple of 32 samples, NaN behind every utterance: a read past one shows in the result
    const int64_t xs = (longest + 31) / 32 * 32 + 32;
    std::vector<float> hx((size_t)B * xs, std::numeric_limits<float>::quiet_NaN());
    for (int b = 0; b < B; ++b) std::memcpy(&hx[(size_t)b * xs], x + (size_t)b * d->x_stride, sizeof(float) * (size_t)n[b]);
    // the 4x table as the kernels read it, [K][L]
    const std::vector<float> h = resample_taps(lplan.up);
    std::vector<float> ht(h.size());
    for (int p = 0; p < lplan.up.L; ++p)
        for (int k = 0; k < lplan.up.K; ++k) ht[(size_t)k * lplan.up.L + p] = h[(size_t)p * lplan.up.K + k];
    const size_t scratch = level_scratch_bytes(B, longest, plan.S), lscratch = limit_scratch_bytes(B, longest);
    DevBuf dx, dy, dlv, dlm, dscr, dlscr, dt;
    DevInts dn;
    // (y goes up too: what lies behind a row's samples must come back as it was)
    if (!dx.put(hx.data(), hx.size()) || !dlv.put(nullptr, (size_t)B * 4) || !dlm.put(nullptr, (size_t)B * 4) || !dscr.put(nullptr, (scratch + 3) / 4) ||
        !dlscr.put(nullptr, (lscratch + 3) / 4) || !dt.put(ht.data(), ht.size()) || !dn.put(n.data(), B) || !dy.put(y, (size_t)B * d->y_stride))
        return fail("device allocation failed");
    LevelCall c;
    c.x = dx.p;
    c.x_stride = xs;
    c.lens = dn.p;
    c.batch = B;
    c.max_len = longest;
    c.plan = plan;
    c.scratch = dscr.p;
    c.kind = d->kind;
    c.value_db = d->value_db;
    c.ceiling_db = d->ceiling_db;
    c.gain = (float)std::pow(10.0, (double)d->value_db / 20.0);
    c.levels = dlv.p;
    hipError_t e = launch_level_measure(c, nullptr);
    if (e == hipSuccess) {
        LimitCall mc;
        mc.x = dx.p;
        mc.x_stride = xs;
        mc.y = dy.p;
        mc.y_stride = d->y_stride;
        mc.lens = dn.p;
        mc.batch = B;
        mc.max_len = longest;
        mc.plan = lplan;
        mc.taps = dt.p;
        mc.scratch = dlscr.p;
        mc.kind = d->kind;
        mc.value_db = d->value_db;
        mc.gain = c.gain;
        mc.ceiling = (float)std::pow(10.0, (double)(d->kind == VITS_LEVEL_PEAK ? 0.f : d->ceiling_db) / 20.0);
        mc.levels = dlv.p;
        mc.limits = dlm.p;
        e = launch_limit(mc, nullptr);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(hipGetErrorString(e));
    if (hipMemcpy(levels, dlv.p, (size_t)B * 4 * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(limits, dlm.p, (size_t)B * 4 * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(y, dy.p, (size_t)B * d->y_stride * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return fail("copy back failed");
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_op_edges(int32_t rate, const vits_edges_desc* desc, int32_t batch, const float* x, int64_t x_stride, const int32_t* lens, float* y, int64_t y_stride,
                           int32_t* lens_out, int64_t* rows) {
    VITS_TRY
    using namespace vits;
    if (!desc || !x || !lens || !y || !lens_out || !rows || batch <= 0 || x_stride <= 0 || y_stride <= 0) return fail("vits_op_edges: null argument or empty batch");
    EdgesPlan plan;
    std::string err;
    if (!edges_plan(rate, *desc, plan, err)) return fail(("vits_op_edges: " + err).c_str());
    if (plan.mode == VITS_EDGES_OFF) return fail("vits_op_edges: VITS_EDGES_OFF delivers the rows as they are: there is nothing to run");
    if (batch > 65535) return fail("vits_op_edges: more than 65535 rows");
    if (x == y) return fail("vits_op_edges: y must not be x");
    // (the one host read: the grids, the scratch and the y_stride check need the longest row)
    std::vector<int32_t> n((size_t)batch);
    if (hipMemcpy(n.data(), lens, sizeof(int32_t) * (size_t)batch, hipMemcpyDeviceToHost) != hipSuccess) return fail("vits_op_edges: reading lens from the device failed");
    int64_t longest = 0;
    for (int b = 0; b < batch; ++b) {
        if (n[b] < 0 || n[b] > x_stride)
            return fail(("vits_op_edges: lens[" + std::to_string(b) + "] = " + std::to_string(n[b]) + " is outside [0, x_stride = " + std::to_string(x_stride) + "]").c_str());
        if (n[b] > kEdgesMaxLen) return fail(("vits_op_edges: row " + std::to_string(b) + " is too long (" + std::to_string(n[b]) + " samples)").c_str());
        longest = std::max<int64_t>(longest, n[b]);
    }
    if (y_stride < plan.bound(longest))
        return fail(("vits_op_edges: y_stride = " + std::to_string(y_stride) + " is below the largest bound (" + std::to_string(longest) + " samples + Pl + Pt = " +
                     std::to_string(plan.bound(longest)) + ")").c_str());
    const std::vector<float> fades = edges_fades(plan);
    DevBuf dscr, df;
    if (!dscr.put(nullptr, (edges_scratch_bytes(batch, longest, plan.W) + 3) / 4) || (!fades.empty() && !df.put(fades.data(), fades.size()))) return fail("device allocation failed");
    EdgesCall c;
    c.x = x;
    c.x_stride = x_stride;
    c.lens = lens;
    c.y = y;
    c.y_stride = y_stride;
    c.batch = batch;
    c.max_len = longest;
    c.plan = plan;
    c.fades = df.p;
    c.scratch = dscr.p;
    c.lens_out = lens_out;
    c.rows = rows;
    hipError_t e = launch_edges_window(c, nullptr);
    if (e == hipSuccess) e = launch_edges_bounds(c, nullptr);
    if (e == hipSuccess) e = launch_edges_apply(c, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(hipGetErrorString(e));
    return 0;
    VITS_CATCH(-1)
}

// ---- multi-GPU PCM gather (pcm_gather.cpp) ---------------------------------------------------------------------------------------
struct vits_gather_ctx {
    vits::PcmGather g;
    std::atomic<bool> busy{false};
};

VITS_API int vits_pcm_gather_unique_id(char* id_out) {
    VITS_TRY
    if (!id_out) {
        set_err("null argument");
        return -1;
    }
    const vits::RcclApi& api = vits::RcclApi::get();
    if (!api.ok()) {
        set_err(api.why);
        return -1;
    }
    vits::RcclApi::UniqueId uid;
    std::memset(&uid, 0, sizeof(uid));
    const int r = api.GetUniqueId(&uid);
    if (r != 0) {
        set_err(std::string("ncclGetUniqueId: ") + api.GetErrorString(r));
        return -1;
    }
    std::memcpy(id_out, uid.internal, sizeof(uid.internal));
    return 0;
    VITS_CATCH(-1)
}

VITS_API vits_gather_ctx* vits_pcm_gather_init(const char* id, size_t id_bytes, int32_t rank, int32_t world, int32_t rows, int64_t row_capacity, int32_t elem_bytes) {
    VITS_TRY
    vits_gather_ctx* h = new vits_gather_ctx();
    std::string err;
    if (!h->g.init(id, id_bytes, rank, world, rows, row_capacity, elem_bytes, err)) {
        set_err(err);
        delete h;
        return nullptr;
    }
    return h;
    VITS_CATCH(nullptr)
}

VITS_API int vits_pcm_gather(vits_gather_ctx* g, const void* pcm_device, int64_t pcm_stride, const int64_t* lengths_host, void* hip_stream, vits_gather_result* out) {
    VITS_TRY
    if (!g || !out) {  // (nothing to hand a result to, or no communicator to tell the peers through)
        set_err("null argument");
        return -1;
    }
    std::memset(out, 0, sizeof(*out));
    vits::BusyGuard guard(&g->busy);
    if (!guard.entered()) {
        set_err("gather busy: one call at a time per gather object");
        return -1;
    }
    vits::PcmGather::Result r;
    std::string err;
    if (g->g.gather(pcm_device, pcm_stride, lengths_host, (hipStream_t)hip_stream, &r, err) != 0) {
        set_err(err);
        return -1;
    }
    out->data = r.data;
    out->stride = r.stride;
    out->lengths = r.lengths;
    out->rows_total = r.rows_total;
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_pcm_gather_verdict(const int64_t* table, int32_t world, int32_t rows, int64_t* stride_out) {
    VITS_TRY
    if (!table || !stride_out || world < 1 || rows < 1) {
        set_err("null argument");
        return -1;
    }
    std::string err;
    if (vits::PcmGather::verdict(table, world, rows, stride_out, err) != 0) {
        set_err(err);
        return -1;
    }
    return 0;
    VITS_CATCH(-1)
}

VITS_API void vits_pcm_gather_destroy(vits_gather_ctx* g) {
    try {
        delete g;
    } catch (...) {
    }
}
