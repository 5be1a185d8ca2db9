// abi.cpp — the C ABI of include/vits.h. Nothing below throws across the boundary (the reference lets
// std::runtime_error escape and calls exit(1) from ASSERT: /root/reference/src/vits_model_data.cpp:102,144,
// src/include/debug.h:29-36); failures return NULL / {NULL,0} / -1 and set vits_last_error().
// This file is the model-level ABI (load, process, convert, align, voices, levels, edges, sinks, device, PCM gather). The operator-level entry points (vits_op_*)
// are in abi_ops_conv.cpp, abi_ops_stage1.cpp and abi_ops_pcm.cpp over the staging layer of abi_ops_common.h; abi_internal.h is what they share with this file.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <new>
#include <string>
#include <vector>

#include "../../include/vits.h"
#include "abi_internal.h"
#include "busy_guard.h"
#include "engine.h"
#include "pcm_gather.h"

namespace vits {
void reference_noise_seed(uint32_t seed);
}

static thread_local std::string g_last_error;
void vits::set_err(const std::string& e) { g_last_error = e; }  // (abi_internal.h: the operator files set the same string)

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
// the report rows [rows][4] of the most recently completed call (vits_model_last_levels / _last_limits / _last_edges): returns 4 rows, and copies them when dst has room
template <class T, class Read>
static int64_t last_rows(vits_model* model, T* dst, size_t cap, Read read) {
    VITS_TRY
    if (!model || (!dst && cap)) {
        set_err("null argument");
        return -1;
    }
    VITS_ENTER(model, -1)
    int rows = 0;
    const T* p = read(model->eng, rows);
    const size_t n = (size_t)4 * rows;
    if (n && dst && cap >= n) std::memcpy(dst, p, sizeof(T) * n);
    return (int64_t)n;
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
    return last_rows(model, dst, cap, [](const vits::Engine& e, int& rows) { return e.last_levels(rows); });
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
    return last_rows(model, dst, cap, [](const vits::Engine& e, int& rows) { return e.last_limits(rows); });
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
    return last_rows(model, dst, cap, [](const vits::Engine& e, int& rows) { return e.last_edges(rows); });
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

// ---- joined tracks (include/vits.h: the definition): the host-only side -------------------------------------------------------------------
VITS_API int vits_join_plan(int32_t rate, int32_t batch, const int32_t* track, const float* gap_ms, const int64_t* utt_bounds, int32_t* tracks_out,
                            int64_t* track_bounds_out, int32_t* tile_out) {
    VITS_TRY
    if (!utt_bounds) return fail("vits_join_plan: null argument (utt_bounds)");
    vits::JoinPlan p;
    std::string err;
    if (!vits::join_plan(rate, batch, track, gap_ms, p, err) || !vits::join_bounds(p, utt_bounds, err)) return fail("vits_join_plan: " + err);
    if (tracks_out) *tracks_out = p.tracks;
    if (track_bounds_out) std::copy(p.bound.begin(), p.bound.end(), track_bounds_out);
    if (tile_out) *tile_out = vits::kJoinTile;
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_join_host(int32_t rate, int32_t batch, const float* x, int64_t x_stride, const int64_t* lens, const int32_t* track, const float* gap_ms, float* y,
                            int64_t y_stride, int64_t* track_lens_out, int64_t* offsets_out) {
    VITS_TRY
    if (!lens || (y && !x)) return fail("vits_join_host: null argument (lens, or x with y given)");
    vits::JoinPlan p;
    std::string err;
    if (!vits::join_plan(rate, batch, track, gap_ms, p, err)) return fail("vits_join_host: " + err);
    for (int b = 0; b < batch; ++b)
        if (y && lens[b] > x_stride) return fail("vits_join_host: lens[" + std::to_string(b) + "] = " + std::to_string(lens[b]) + " is above x_stride = " + std::to_string(x_stride));
    if (!vits::join_bounds(p, lens, err)) return fail("vits_join_host: " + err);
    if (y && y_stride < p.max_bound) return fail("vits_join_host: y_stride = " + std::to_string(y_stride) + " is below the largest track bound (" + std::to_string(p.max_bound) + " samples)");
    vits::join_host(p, x, x_stride, lens, y, y_stride, track_lens_out, offsets_out);
    return 0;
    VITS_CATCH(-1)
}

// ---- text in: the sentences of a paragraph ---------------------------------------------------------------------------------------------------------
VITS_API int64_t vits_split_sentences(const char* text, int64_t* starts, int64_t* ends, int32_t* kinds, size_t cap) {
    VITS_TRY
    if (!text) return fail("vits_split_sentences: null argument (text)");
    return vits::split_sentences(text, starts, ends, kinds, cap);
    VITS_CATCH(-1)
}

// ---- a batch joined inside the call; a whole text spoken (include/vits.h) ------------------------------------------------------------------------------
VITS_API int vits_model_process_joined(vits_model* model, const int32_t* ids, const int32_t* id_lengths, int32_t batch, int32_t id_stride,
                                       const vits_process_opts* opts, const int32_t* track, const float* gap_ms, vits_batch_result* out) {
    VITS_TRY
    if (out) std::memset(out, 0, sizeof(*out));
    if (!model || !ids) {
        set_err("vits_model_process_joined: null argument");
        return -1;
    }
    VITS_ENTER(model, -1)
    const vits_process_opts o = default_opts(opts, VITS_NOISE_COUNTER);
    return run_engine(out, [&](std::string& err) { return model->eng.process_joined(ids, id_lengths, batch, id_stride, o, track, gap_ms, nullptr, out, err); });
    VITS_CATCH(-1)
}
VITS_API int64_t vits_model_last_joins(vits_model* model, int64_t* dst, size_t cap) {
    return last_rows(model, dst, cap, [](const vits::Engine& e, int& rows) { return e.last_joins(rows); });
}

VITS_API int vits_model_speak(vits_model* model, const char* text, const vits_speak_opts* opts, vits_batch_result* out) {
    VITS_TRY
    const std::string who = "vits_model_speak: ";
    if (out) std::memset(out, 0, sizeof(*out));
    if (!model) return fail(who + "null argument (model)");
    {
        std::vector<float> given;  // (taken first: whatever becomes of this call, the ratios given for it are gone)
        if (model->eng.take_pitch_ratios(given))
            return fail(who + "the ratios of vits_model_set_pitch_ratios are one per utterance, and the text decides how many utterances there are: use "
                              "vits_model_set_pitch, or vits_split_sentences and vits_model_process_joined");
    }
    // (the fit of the next call: taken here like the ratios; the total form goes on to the joined call this one makes, once the text has said how many utterances it has)
    vits::Engine::FitGiven fit;
    if (model->eng.take_fit(fit) && !fit.total)
        return fail(who + "the targets of vits_model_set_fit are one per group of utterances, and the text decides how many utterances there are: use "
                          "vits_model_set_fit_total, or vits_split_sentences and vits_model_process_joined");
    vits_speak_opts so;
    std::memset(&so, 0, sizeof(so));
    so.struct_size = sizeof(so);
    if (opts) std::memcpy(&so, opts, std::min<size_t>(sizeof(so), opts->struct_size ? opts->struct_size : sizeof(so)));
    const vits_process_opts o = default_opts(so.process, VITS_NOISE_COUNTER);
    // (the per-utterance arrays are as long as the batch, which the caller does not know before the text is cut)
    const std::pair<const char*, bool> arrays[] = {{"speaker_ids", o.speaker_ids != nullptr},
                                                   {"speaking_rates", o.speaking_rates != nullptr},
                                                   {"noise_scales", o.noise_scales != nullptr},
                                                   {"noise_scale_durations", o.noise_scale_durations != nullptr},
                                                   {"duration_override", o.duration_override != nullptr},
                                                   {"durations_out", o.durations_out != nullptr},
                                                   {"noise_seed_offsets", o.noise_seed_offsets != nullptr},
                                                   {"noise_dur", o.noise_dur != nullptr},
                                                   {"noise_prior", o.noise_prior != nullptr}};
    for (const auto& [name, set] : arrays)
        if (set)
            return fail(who + "process->" + name + " is a per-utterance array, and the text decides how many utterances there are: use the model-level settings, or "
                              "vits_split_sentences and vits_model_process_joined");
    if (o.noise_kind != VITS_NOISE_COUNTER) return fail(who + "process->noise_kind must be VITS_NOISE_COUNTER");
    const vits::Tokenizer& tok = model->eng.tok;
    struct Ctx {
        const vits::Tokenizer& tok;
    } ctx{tok};
    const vits::SpeakTokenize tokenize = [](void* user, const std::string& span, std::vector<int32_t>& ids, std::string& err) {
        const vits::Tokenizer& t = static_cast<Ctx*>(user)->tok;
        if (!t.tokenize_checked(span, ids, err)) return false;  // (a phonetic model: refused with the text entry points' message)
        if (t.add_blank && ids.size() == 1) ids.clear();        // (the lone blank of a span without a known symbol: nothing to say)
        return true;
    };
    if (text && *text && !tok.phonetic && !tok.add_blank)  // Q11, as vits_model_process: the reference's tokenizer returns no ids at all without add_blank
        return fail(who + "empty input: the model file says add_blank = 0, for which the reference tokenizer returns no ids (vits_tokenizer.cpp:200-208); pass ids");
    vits::SpeakPlan p;
    std::string err;
    if (!vits::speak_plan(text, so.sentence_gap_ms, so.paragraph_gap_ms, so.track_per_paragraph != 0, tokenize, &ctx, p, err)) return fail(who + err);
    VITS_ENTER(model, -1)
    if (fit.set) model->eng.give_fit(std::move(fit));
    return run_engine(out, [&](std::string& e) {
        return model->eng.process_joined(p.ids.data(), p.id_lens.data(), p.batch, p.id_stride, o, p.track.data(), p.gap_ms.data(), p.index.data(), out, e);
    });
    VITS_CATCH(-1)
}

// ---- a stated pitch (include/vits.h: the definition) ---------------------------------------------------------------------------------------------------
VITS_API float vits_pitch_ratio(float semitones) { return (float)std::exp2((double)semitones / 12.0); }
VITS_API int vits_pitch_plan(float ratio, int64_t n, int64_t* P, int64_t* S, int32_t* R, int64_t* n_out) {
    VITS_TRY
    vits::PitchPlan p;
    std::string err;
    if (!vits::pitch_plan(ratio, n, p, err)) return fail("vits_pitch_plan: " + err);
    if (P) *P = p.P;
    if (S) *S = p.S;
    if (R) *R = p.R;
    if (n_out) *n_out = p.n_out;
    return 0;
    VITS_CATCH(-1)
}
VITS_API int64_t vits_pitch_table(float* dst, size_t cap) {
    VITS_TRY
    const size_t n = (size_t)2 * vits::kPitchTableN;
    if (!dst && cap) return fail("vits_pitch_table: null argument (dst is NULL with cap > 0)");
    if (dst && cap >= n) {
        const std::vector<float> t = vits::pitch_table();
        std::memcpy(dst, t.data(), sizeof(float) * n);
    }
    return (int64_t)n;
    VITS_CATCH(-1)
}
VITS_API int64_t vits_pitch_host(const float* x, int64_t n, float ratio, double* y, size_t cap) {
    VITS_TRY
    vits::PitchPlan p;
    std::string err;
    if (!y || (!x && n)) return fail("vits_pitch_host: null argument (y, or x with n > 0)");
    if (!vits::pitch_plan(ratio, n, p, err)) return fail("vits_pitch_host: " + err);
    if (cap < (size_t)p.n_out) return fail("vits_pitch_host: cap = " + std::to_string(cap) + " is below the row's " + std::to_string(p.n_out) + " output samples");
    const std::vector<float> t = vits::pitch_table();
    vits::pitch_host(x, n, p, t.data(), y);
    return p.n_out;
    VITS_CATCH(-1)
}
VITS_API int vits_model_set_pitch(vits_model* model, float ratio) {
    if (!model) {
        set_err("null argument");
        return -1;
    }
    VITS_ENTER(model, -1)
    return run_engine(nullptr, [&](std::string& err) { return model->eng.set_pitch(ratio, err); });
}
VITS_API int vits_model_set_pitch_ratios(vits_model* model, const float* ratios, int32_t n) {
    VITS_TRY
    if (!model) {
        set_err("null argument");
        return -1;
    }
    VITS_ENTER(model, -1)
    return run_engine(nullptr, [&](std::string& err) { return model->eng.set_pitch_ratios(ratios, n, err); });
    VITS_CATCH(-1)
}
VITS_API int vits_model_get_pitch(const vits_model* model, float* ratio) {
    if (!model) {
        set_err("null argument");
        return -1;
    }
    if (ratio) *ratio = model->eng.pitch_ratio;
    return 0;
}
VITS_API int64_t vits_model_last_pitch(vits_model* model, int64_t* dst, size_t cap) {
    VITS_TRY
    if (!model || (!dst && cap)) {
        set_err("null argument");
        return -1;
    }
    VITS_ENTER(model, -1)
    int rows = 0;
    const int64_t* p = model->eng.last_pitch(rows);  // [rows][4]: P, N, N', K
    if (rows && dst && cap >= (size_t)3 * rows)
        for (int b = 0; b < rows; ++b) std::copy_n(p + (size_t)4 * b, 3, dst + (size_t)3 * b);
    return rows;
    VITS_CATCH(-1)
}

// ---- a stated duration (include/vits.h: the definition) ------------------------------------------------------------------------------------------------
VITS_API int vits_fit_host(int32_t batch, int32_t t_stride, const float* e, const int32_t* fixed, const int32_t* lens, const int32_t* groups,
                           const int64_t* target_frames, float min_rate, float max_rate, int32_t* dur_out, double* group_rows_out) {
    VITS_TRY
    const std::string who = "vits_fit_host: ";
    if (!e || !target_frames || !dur_out || !group_rows_out) return fail(who + "null argument (e, target_frames, dur_out or group_rows_out)");
    vits::FitGroups g;
    std::string err;
    if (!vits::fit_check_rows(batch, t_stride, fixed, lens, err) || !vits::fit_check(batch, groups, target_frames, err) ||
        !vits::fit_limits(min_rate, max_rate, g.s_lo, g.s_hi, err))
        return fail(who + err);
    const std::vector<int> tgt(target_frames, target_frames + batch);
    std::vector<int64_t> rows((size_t)batch * vits::kFitRowInts);
    g.group = groups, g.target = tgt.data();
    vits::fit_host(batch, t_stride, e, fixed, lens, g, dur_out, rows.data());
    vits::fit_rows_double(batch, rows.data(), group_rows_out);
    return 0;
    VITS_CATCH(-1)
}
VITS_API int vits_model_set_fit(vits_model* model, const int64_t* target_frames, const int32_t* groups, int32_t n, float min_rate, float max_rate) {
    VITS_TRY
    if (!model) {
        set_err("null argument");
        return -1;
    }
    VITS_ENTER(model, -1)
    return run_engine(nullptr, [&](std::string& err) { return model->eng.set_fit(target_frames, groups, n, min_rate, max_rate, err); });
    VITS_CATCH(-1)
}
VITS_API int vits_model_set_fit_total(vits_model* model, int64_t total_frames, float min_rate, float max_rate) {
    VITS_TRY
    if (!model) {
        set_err("null argument");
        return -1;
    }
    VITS_ENTER(model, -1)
    return run_engine(nullptr, [&](std::string& err) { return model->eng.set_fit_total(total_frames, min_rate, max_rate, err); });
    VITS_CATCH(-1)
}
VITS_API int64_t vits_model_fit_frames(const vits_model* model, double seconds) {
    if (!model) {
        set_err("null argument");
        return -1;
    }
    const int64_t L = model->eng.fit_frames(seconds);
    if (L < 0) set_err("vits_model_fit_frames: seconds is not finite");
    return L;
}
VITS_API int64_t vits_model_last_fit(vits_model* model, double* dst, size_t cap) {
    VITS_TRY
    if (!model || (!dst && cap)) {
        set_err("null argument");
        return -1;
    }
    VITS_ENTER(model, -1)
    int rows = 0;
    const double* p = model->eng.last_fit(rows);  // [rows][6]
    if (rows && dst && cap >= (size_t)6 * rows) std::copy_n(p, (size_t)6 * rows, dst);
    return rows;
    VITS_CATCH(-1)
}

// ---- a stated tempo (include/vits.h: the definition) ---------------------------------------------------------------------------------------------------
VITS_API int vits_tempo_plan(int32_t rate, float tempo, int64_t n, int32_t* H, int32_t* D, int64_t* Q, int64_t* F, int64_t* n_out) {
    VITS_TRY
    vits::TempoPlan p;
    std::string err;
    if (!vits::tempo_plan(rate, tempo, n, p, err)) return fail("vits_tempo_plan: " + err);
    if (H) *H = p.H;
    if (D) *D = p.D;
    if (Q) *Q = p.Q;
    if (F) *F = p.F;
    if (n_out) *n_out = p.n_out;
    return 0;
    VITS_CATCH(-1)
}
VITS_API int64_t vits_tempo_host(const float* x, int64_t n, int32_t rate, float tempo, float* y, size_t y_cap, int32_t* offsets, size_t offsets_cap) {
    VITS_TRY
    vits::TempoPlan p;
    std::string err;
    if (!y || (!x && n) || (!offsets && offsets_cap)) return fail("vits_tempo_host: null argument (y, x with n > 0, or offsets with offsets_cap > 0)");
    if (!vits::tempo_plan(rate, tempo, n, p, err)) return fail("vits_tempo_host: " + err);
    if (y_cap < (size_t)p.n_out) return fail("vits_tempo_host: y_cap = " + std::to_string(y_cap) + " is below the row's " + std::to_string(p.n_out) + " output samples");
    if (offsets && offsets_cap < (size_t)p.F)
        return fail("vits_tempo_host: offsets_cap = " + std::to_string(offsets_cap) + " is below the row's " + std::to_string(p.F) + " segments");
    vits::tempo_host(x, n, p, y, offsets);
    return p.n_out;
    VITS_CATCH(-1)
}

VITS_API int vits_model_set_conversion_prosody(vits_model* model, float rate, float pitch) {
    if (!model) {
        set_err("null argument");
        return -1;
    }
    VITS_ENTER(model, -1)
    return run_engine(nullptr, [&](std::string& err) { return model->eng.set_conversion_prosody(rate, pitch, err); });
}
VITS_API int vits_model_get_conversion_prosody(const vits_model* model, float* rate, float* pitch) {
    if (!model) {
        set_err("null argument");
        return -1;
    }
    if (rate) *rate = model->eng.vc_rate;
    if (pitch) *pitch = model->eng.vc_pitch;
    return 0;
}
VITS_API int vits_model_set_conversion_ratios(vits_model* model, const float* rates, const float* pitches, int32_t n) {
    VITS_TRY
    if (!model) {
        set_err("null argument");
        return -1;
    }
    VITS_ENTER(model, -1)
    return run_engine(nullptr, [&](std::string& err) { return model->eng.set_conversion_ratios(rates, pitches, n, err); });
    VITS_CATCH(-1)
}
VITS_API int64_t vits_model_last_tempo(vits_model* model, int64_t* dst, size_t cap) {
    VITS_TRY
    if (!model || (!dst && cap)) {
        set_err("null argument");
        return -1;
    }
    VITS_ENTER(model, -1)
    int rows = 0;
    const int64_t* p = model->eng.last_tempo(rows);  // [rows][4]: Q, N, N', F
    if (rows && dst && cap >= (size_t)4 * rows) std::copy_n(p, (size_t)4 * rows, dst);
    return rows;
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
