/*
 * vits.h — C ABI of the MI355X-native VITS inference library (libvits_hip.so).
 *
 * DROP-IN BOUNDARY. The first five entry points are byte-compatible with the reference's exported C API
 * (/root/reference/src/include/vits.h:87-102, implemented at /root/reference/src/vits.cpp:1193-1232):
 * same names, same argument meaning, same ownership rules. `vits_model` is opaque here (the reference exposes
 * a C++ class with ggml-typed members, vits.h:17-85, which cannot survive without ggml; every reference
 * caller — test/main.cpp:68-78, test/bench_e2e.cpp:68-91, test/bench.cpp:204-206 — only passes the pointer).
 *
 * Differences from the reference, all deliberate:
 *   - no exception / exit(1) crosses the boundary (reference: std::runtime_error from
 *     src/vits_model_data.cpp:102,144 and ASSERT->exit at src/include/debug.h:29-36). Failures return
 *     NULL / {NULL,0}; the message is available from vits_last_error().
 *   - nothing is printed to stdout (reference prints at src/vits.cpp:27,1200 and in the loaders).
 *   - everything below "extensions" is new: id-level and batched entry points (the reference is batch-1,
 *     text-only), pipelined batches on one handle, synthetic model generation, taps, profiling, operator-level
 *     entry points for parity tests.
 *   - threading: one call at a time per model handle, as in the reference (vits_model::process writes member
 *     tensors, vits.h:22-30) — but ENFORCED: an entry point entered while another call on the same handle is in
 *     progress (from a second thread, or from an on_chunk callback) returns its failure value with
 *     vits_last_error() = "model busy: ...". Distinct handles may be used from distinct threads concurrently.
 *
 * Plain C types only: pointers, sizes, PODs. No torch / HIP types appear in any signature; device buffers are
 * passed as `void*` device addresses.
 */
#ifndef VITS_HIP_H
#define VITS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
#define VITS_API extern "C" __attribute__((visibility("default")))
#else
#define VITS_API __attribute__((visibility("default")))
#endif

typedef struct vits_model vits_model; /* opaque */

/* reference: src/include/vits.h:89-92 */
typedef struct vits_result {
    float* data; /* mono fp32 PCM in [-1,1]; owned by the library until vits_free_result */
    size_t size; /* samples */
} vits_result;

/* ---- the reference's five symbols ------------------------------------------------------------------- */

/* reference: vits.h:94, vits.cpp:1205-1215. Copies what it needs; caller may free `bytes` on return. */
VITS_API vits_model* vits_model_load_from_bytes(const char* bytes, size_t size);
/* reference: vits.h:96, vits.cpp:1193-1203 */
VITS_API vits_model* vits_model_load_from_file(const char* path);
/* reference: vits.h:98, vits.cpp:1217-1219. A handle that another thread (or a streaming callback) is inside is NOT freed: the call returns with
 * vits_last_error() = "vits_free_model: model busy ..." and leaves the handle exactly as it was (the busy flag belongs to the call in progress and is
 * released when that call returns) — call vits_free_model again then. The function returns void as in the reference: check vits_last_error(). */
VITS_API void vits_free_model(vits_model* model);
/* reference: vits.h:100, vits.cpp:1221-1223 */
VITS_API void vits_free_result(vits_result result);
/* reference: vits.h:102, vits.cpp:1225-1232 -> vits_model::process vits.cpp:1101-1191.
 * Text is lower-cased, greedily matched against the model vocabulary and interspersed with blanks
 * (src/vits_tokenizer.cpp:182-208). Noise comes from the reference's process-global libstdc++ stream
 * (VITS_NOISE_REFERENCE), mode is the model default (VITS_MODE_REFERENCE unless changed).
 * Two model-file flags decide what the TEXT entry points (this one, vits_model_tokenize, vits_model_file_tokenize) do:
 *   config "phonetic" = "1" (vits_model_data.cpp:92-94): the model expects espeak-ng phonemes. The reference asserts out at load unless built with
 *     VITS_ESPEAK (vits_tokenizer.cpp:176-178); espeak is out of scope here, so the model LOADS and the text entry points fail with
 *     vits_last_error() = "model expects espeak phonemes ... pass ids"; the id entry points are unaffected.
 *   add_blank = 0: the reference's tokenizer returns an EMPTY id list (Q11, vits_tokenizer.cpp:200-208) and its process() an empty result; the same
 *     here ({NULL, 0} with a message that says so; vits_model_tokenize returns 0). */
VITS_API vits_result vits_model_process(vits_model* model, const char* phonemes);

/* ---- extensions ------------------------------------------------------------------------------------- */

/* Thread-local message of the last failure in this thread ("" if none). */
VITS_API const char* vits_last_error(void);

/* Semantics mode:
 *   VITS_MODE_REFERENCE: what /root/reference/src/vits.cpp literally computes: ConvTranspose1d without
 *     crop (Q1, vits.cpp:187), final LeakyReLU slope 0.1 (Q2, :638), spline width affine (Q3, :720),
 *     index -1 wrap on the last token (Q4, ggml-util.h:235), exp(+log_scale) (Q5, :913-918), and the masked get / set
 *     pair of the spline tails as implemented (Q6, :832-849 with custom-ops.h:739-752,829-862: masked_get keeps the
 *     shape, masked_set consumes compacted values — a latent outside [-5, 5] shifts the log-durations of every later
 *     token; the identity permutation while every latent is inside).
 *   VITS_MODE_HF: what transformers.VitsModel (the model the reference ports, vits.cpp:113) computes. */
#define VITS_MODE_DEFAULT (-1)
#define VITS_MODE_REFERENCE 0
#define VITS_MODE_HF 1
VITS_API int vits_model_set_mode(vits_model* model, int mode);
VITS_API int vits_model_get_mode(const vits_model* model);

/* Conv arithmetic. The reference's conv is fp16 x fp16 -> fp32: weights are cast to fp16 by the exporter
 * (scripts/export_vits.py:87) and the activations are rounded to fp16 by the im2col in front of every conv
 * (src/include/custom-ops.h:684-690).
 *   VITS_ARITH_F32 (default): activations stay fp32, weights are the stored 16-bit values widened exactly, fp32 MFMA
 *     (v_mfma_f32_32x32x2_f32) — the exact-arithmetic parity mode the headline is measured in.
 *   VITS_ARITH_F16: the literal Q7 arithmetic: conv inputs rounded to fp16 (round-to-nearest-even) where the tile is staged,
 *     fp16 weights, fp32 accumulation on v_mfma_f32_32x32x16_f16.
 *   VITS_ARITH_BF16: the same with bf16 operands (BASELINE.json configs[4]: bf16 weights) on v_mfma_f32_32x32x16_bf16.
 *   VITS_ARITH_F32_SPLIT (round 6, opt-in): fp32-ACCURATE results on the bf16 matrix cores. The ResBlock convolutions of the vocoder's wide stages
 *     (C >= 128: 64 % of the path's FLOPs) take their fp16-valued weights as the exact sum of two bf16 values and their fp32 activations as the exact sum of
 *     three, and accumulate the five significant cross products in fp32 (csrc/conv_split.hip): the same accuracy against the exact sum as the fp32 fmaf
 *     chain (measured, tools/split_micro.hip), at 1.8x its matrix-core rate — but NOT the same bits (another summation order), so "batch 1 == row of a
 *     batch, bit for bit" is asserted for VITS_ARITH_F32 only. Everything else, stage one included (durations bit-exact), is the VITS_ARITH_F32 path.
 *     The scope setting does not apply. Weights that are not exactly two bf16 pieces (an fp32-stored conv) keep the fp32 kernels.
 * 16-bit modes apply to the Conv1d / ConvTranspose1d of the scope chosen with vits_model_set_arith_scope (never to the Linear
 * layers q/k/v/out, which are ggml_mul_mat on f32 x f32 in the reference, vits.cpp:287-289,358); everything else (layer norms,
 * attention softmax, splines, gates, residual adds, accumulators) stays fp32. Set between calls, not during one. */
#define VITS_ARITH_F32 0
#define VITS_ARITH_BF16 1
#define VITS_ARITH_F16 2
#define VITS_ARITH_F32_SPLIT 3
VITS_API int vits_model_set_arith(vits_model* model, int arith);
VITS_API int vits_model_get_arith(const vits_model* model);
/* Which convolutions a 16-bit arithmetic mode applies to.
 *   VITS_ARITH_SCOPE_FLOW_VOCODER (default): the coupling flow and HiFiGAN (99 % of the FLOPs) run on 16-bit operands; stage one
 *     (text encoder, duration predictor, prior projection: vits.cpp:244-440,927-972) stays EXACT fp32, so the durations — the
 *     path's only integer output, ceil(exp(logw) * length_scale) at vits.cpp:996-1001 — the frame counts and the sample counts
 *     are bit-identical to the fp32 path's (and to the oracle's) in every arithmetic mode.
 *   VITS_ARITH_SCOPE_ALL_CONVS: the literal Q7 arithmetic — every Conv1d / ConvTranspose1d of the path, stage one included
 *     (custom-ops.h:684-690 rounds the im2col of EVERY conv). Durations then carry the mode's rounding noise: a log-duration
 *     within an fp16 ulp of a ceil() boundary may land on either side.
 * Set between calls, not during one. */
#define VITS_ARITH_SCOPE_FLOW_VOCODER 0
#define VITS_ARITH_SCOPE_ALL_CONVS 1
VITS_API int vits_model_set_arith_scope(vits_model* model, int scope);
VITS_API int vits_model_get_arith_scope(const vits_model* model);

/* EMULATED ggml lookup tables — INFERRED from upstream ggerganov/ggml of the reference's era: the maxilevi/ggml fork the
 * reference is built against is absent (empty submodule), so this is a labelled emulation of what `ggml_gelu` (vits.cpp:673,687) and
 * `ggml_soft_max` (vits.cpp:329,719,735) most probably compute there, not a pinned restatement:
 *   ggml_gelu:     y = fp16->fp32( table_gelu_f16[ fp32->fp16(x) ] ), the table holding fp16( 0.5 x (1 + tanh(sqrt(2/pi) x (1 + 0.044715 x^2))) );
 *   ggml_soft_max: e_i = fp16->fp32( table_exp_f16[ fp32->fp16(x_i - max) ] ), the sum in double, p_i = e_i * (float)(1 / sum).
 * The GELU of the duration predictor's DDS layers and the soft-max of the text encoder's attention and of the spline bins go through those tables
 * (built on the host with the C library, as ggml_init does). Default 0: erf-GELU (what transformers.VitsModel computes) and fp32 soft-max — the
 * mode every parity fixture is in. Set between calls.
 *   on = 1: a table turns a last-bit difference of its argument into a 5e-4 step of its value, so in this mode STAGE ONE (text encoder + duration
 *           predictor, ~1 % of the work) runs in ONE fixed order of operations — include/vits_exact_math.h: one device thread per output element,
 *           sequential sums, fp contraction off, polynomial exp / log instead of the device library's — which the oracle shares
 *           (vo_opts.ggml_tables = 1): log-durations, durations, frame and sample counts are BIT-IDENTICAL to the oracle's (GPU test). A
 *           measurement instrument (how far do ggml's tables move the durations: ~0.1 % of the ids), not a serving configuration: stage one takes
 *           several times longer than the throughput kernels; everything behind the durations is the default path. Needs fp32 stage-one
 *           arithmetic (VITS_ARITH_SCOPE_FLOW_VOCODER, the default).
 *   on = 2: the same tables inside the THROUGHPUT kernels (MFMA summation order, the device library's exp / log): agrees with the oracle's loops
 *           (vo_opts.ggml_tables = 2) statistically only — a few durations per ten thousand ids differ. Kept for that comparison. */
VITS_API int vits_model_set_ggml_tables(vits_model* model, int on);
VITS_API int vits_model_get_ggml_tables(const vits_model* model);

/* ---- speaker conditioning (multi-speaker VITS files: num_speakers > 1, speaker_embedding_size > 0) ----------------------
 * transformers VitsModel(speaker_id=s): the embedding g = embed_speaker[s] enters the duration predictor (conv_pre(x) + cond(g)),
 * every WaveNet layer of the flow (in_layers[i](h) + its slice of cond_layer(g), before tanh * sigmoid) and the decoder
 * (conv_pre(spec) + cond(g)). The three speaker terms are folded into a per-speaker table of biases built once at load. The
 * reference defines no speakers (vits.cpp:461,603,936 assert them away), so conditioning is the same in both modes.
 * vits_model_set_speaker sets the speaker of every utterance a call does not name (vits_model_process, vits_model_process_ids,
 * and vits_process_opts.speaker_ids == NULL); the default is -1 = none. Returns 0, or -1 for a speaker outside
 * [-1, num_speakers) or >= 0 on a single-speaker model. */
VITS_API int vits_model_set_speaker(vits_model* model, int32_t speaker);
VITS_API int32_t vits_model_get_speaker(const vits_model* model);
VITS_API int32_t vits_model_num_speakers(const vits_model* model); /* 1 for a single-speaker model */

/* ---- custom voices: speaker embeddings registered at run time (multi-speaker models) -----------------------------------
 * A voice is a vector of E = vits_model_speaker_embedding_size floats that is NOT a row of the file's embed_speaker: a blend of two speakers, a
 * fine-tuned or externally estimated embedding. Registering it appends one row to the per-speaker bias tables (the same 1x1 conditioning convs as the
 * file's speakers, in the same order of operations: a voice whose vector equals a file speaker's embedding gives that speaker's audio bit for bit) and
 * returns a VOICE ID. Ids are num_speakers + k, k = 0, 1, ... in order of registration, stable until vits_model_clear_voices;
 * vits_model_num_speakers keeps returning the file's count. A voice id is accepted wherever a speaker index is: vits_process_opts.speaker_ids,
 * vits_model_set_speaker, vits_model_submit_batch, src_speakers / tgt_speakers of vits_model_convert_batch / vits_model_convert, speakers of
 * vits_model_align_batch / vits_model_align; one batch may mix -1, file speakers and voices, and such a call queues exactly the kernels of a call
 * with file speakers. Every speaker check then reads "outside [-1, num_speakers + num_voices)".
 *   vits_model_speaker_embedding_size  E; 0 for a single-speaker model (and for NULL).
 *   vits_model_get_speaker_embedding   id in [0, num_speakers): the file's embed_speaker row, widened exactly to fp32; id of a voice: the vector as
 *                                      registered. Copies min(E, cap) floats to dst and returns E; -1 + message otherwise.
 *   vits_model_add_voices              emb: host [n][E], ids_out: [n]. All n voices or none. Returns 0.
 *   vits_model_set_voice               overwrites a registered voice in place (its id stays).
 *   vits_model_clear_voices            forgets every voice; ids start again at num_speakers. The device memory is kept for the next registration.
 *   vits_model_num_voices              registered voices (0 for NULL).
 * Refused with -1 and a message, the handle unchanged: a single-speaker model, n <= 0, a NULL pointer, a value that is not finite (the message names
 * voice and element), an id that is not a registered voice (set_voice) or neither speaker nor voice (get_speaker_embedding), any of the three mutating
 * calls while batches are in flight ("batches in flight") or from inside an on_chunk callback ("model busy"), vits_model_clear_voices while the handle's
 * default speaker is a voice (reset it first), a device allocation that fails (the registry keeps what it had). With
 * vits_model_set_ggml_tables(model, 1) voices are refused by the calls exactly as speakers are.
 * Memory: a handle that never registers a voice allocates nothing. The first registration makes the conditioning convs resident (MMS-TTS architecture
 * with speakers: 6,848 x 256 fp32 = 7 MB, plus the posterior encoder's once conversion is prepared); each voice then costs one table row (27 KB, plus
 * the posterior's 24 KB); capacity doubles as the registry grows. All of it is counted in vits_model_weight_bytes. Voices registered before
 * vits_model_prepare_conversion and after it give the same conversion. */
VITS_API int32_t vits_model_speaker_embedding_size(const vits_model* model);
VITS_API int vits_model_get_speaker_embedding(vits_model* model, int32_t id, float* dst, size_t cap);
VITS_API int vits_model_add_voices(vits_model* model, const float* emb, int32_t n, int32_t* ids_out);
VITS_API int vits_model_set_voice(vits_model* model, int32_t voice_id, const float* emb);
VITS_API int vits_model_clear_voices(vits_model* model);
VITS_API int32_t vits_model_num_voices(const vits_model* model);

/* Noise source for the two N(0,1) draws (vits.cpp:948 [T,2] and :1059 [L,192]). */
#define VITS_NOISE_REFERENCE 0 /* libstdc++ minstd_rand0 + normal_distribution<float>, global, host-serial */
#define VITS_NOISE_COUNTER 1   /* include/vits_synth_noise.h, evaluated on the device                       */
#define VITS_NOISE_EXPLICIT 2  /* caller-provided host buffers                                             */
/* Re-seed the reference noise stream (the reference never does: default seed 1, vits.cpp:31). */
VITS_API void vits_reference_noise_seed(uint32_t seed);

/* Streaming sink: `pcm` points at samples [offset, offset+n) of utterance `utt` (host memory owned by the library,
 * valid during the call only). Chunks of one utterance arrive in order and tile it exactly. With an output rate set (vits_model_set_rates)
 * offset and n count samples at that rate, and the chunks tile [0, lengths[b]) of the delivered PCM. */
typedef int (*vits_chunk_callback)(void* user, int32_t utt, size_t offset, const float* pcm, size_t n);

typedef struct vits_process_opts {
    uint32_t struct_size;       /* = sizeof(vits_process_opts) */
    int32_t mode;                /* VITS_MODE_*; VITS_MODE_DEFAULT = model default */
    int32_t noise_kind;          /* VITS_NOISE_* */
    uint64_t noise_seed;         /* VITS_NOISE_COUNTER: utterance u uses seed noise_seed + u */
    const float* noise_dur;      /* VITS_NOISE_EXPLICIT: host [B][2][id_stride] */
    const float* noise_prior;    /* VITS_NOISE_EXPLICIT: host [B][192][noise_prior_stride] */
    int64_t noise_prior_stride;  /* frames between channels in noise_prior */
    int32_t fixed_duration;      /* >0: every id lasts this many frames (pinned-length benchmark run) */
    int32_t collect_taps;        /* 1: keep stage outputs for vits_model_get_tap */
    void* out_device;            /* optional device buffer [B][out_device_stride] fp32 to receive the PCM */
    int64_t out_device_stride;   /* samples; must be >= the longest utterance (as delivered: at the output rate if one is set) */
    int32_t skip_host_copy;      /* 1: leave PCM on the device only (requires out_device or tap access) */
    int32_t async;               /* 1: return without synchronising the stream (requires skip_host_copy and
                                    fixed_duration>0, the only case with no data-dependent host read);
                                    call vits_model_sync() before touching out_device */
    /* ---- long-form / streaming (the reference cannot run 1024-id inputs at all: its 512 MB
     * arena at vits.cpp:1145 overflows) ---- */
    int32_t vocoder_chunk_frames; /* >0: run HiFiGAN over windows of this many frames (plus the exact receptive-
                                     field halo on both sides) instead of the whole utterance: activation memory is
                                     bounded by the window, and the PCM is BIT-IDENTICAL to the unchunked result.
                                     Ignored with collect_taps. 0 = whole utterance. */
    int32_t frames_only;          /* 1: run the text encoder and the duration predictor only: the result carries frames[] and
                                     lengths[] (samples) per utterance and no audio. For dispatchers: sizing out_device,
                                     balancing utterance shards by predicted frames. Same noise -> same durations
                                     as the full call. */
    vits_chunk_callback on_chunk; /* optional: called on the calling thread as each window's PCM reaches the host,
                                     while the device already works on the next windows (needs vocoder_chunk_frames>0
                                     and a host copy, i.e. skip_host_copy=0). Non-zero return aborts the call. */
    void* on_chunk_user;
    const int32_t* noise_seed_offsets; /* VITS_NOISE_COUNTER, optional host [B]: utterance b draws from the stream with seed
                                          noise_seed + noise_seed_offsets[b] instead of noise_seed + b. Lets a dispatcher
                                          re-order or re-shard utterances (e.g. balance ranks by frames) without changing
                                          any utterance's audio. */
    const int32_t* speaker_ids;   /* optional host [B]: the speaker of utterance b (multi-speaker models, vits_model_num_speakers > 1);
                                     -1 = no speaker conditioning (transformers VitsModel with speaker_id=None). Every utterance of a
                                     batch may have its own speaker. NULL = every utterance uses the model default (vits_model_set_speaker).
                                     Copied when the call returns (vits_model_submit_batch included). A speaker outside
                                     [-1, num_speakers), any speaker >= 0 on a single-speaker model, or one with
                                     vits_model_set_ggml_tables(model, 1) fails the call with -1 and a message naming the utterance. */
    /* ---- prosody and token timings (transformers VitsModel.speaking_rate / noise_scale / noise_scale_duration, per utterance) ----
     * Each array is optional host memory, NULL = every utterance uses the model value (vits_model_set_prosody). The arrays are copied
     * when the call returns (vits_model_submit_batch included). Only the scales change: every noise draw stays where it is. Refused
     * (-1, the message names the utterance / token): a rate that is not finite or outside [0.1, 10], a noise scale that is not finite or
     * outside [0, 10], an override outside [-1, 10000], speaking_rates or duration_override with fixed_duration > 0. */
    const float* speaking_rates;        /* [B]: d = ceil(exp(logw) * (float)(1.0 / rate)) (vits.cpp:996) */
    const float* noise_scales;          /* [B]: scale of the prior draw (vits.cpp:1061) */
    const float* noise_scale_durations; /* [B]: scale of the [2][T] duration draw (vits.cpp:948-949). Validated as always and without effect on a
                                           model with the deterministic duration predictor, which draws nothing */
    const int32_t* duration_override;   /* [B][id_stride]: >= 0: token t of utterance b lasts that many frames; -1: the predicted duration
                                           (scaled by the utterance's rate). The predictor still runs and (the stochastic one) still draws its noise. Frames
                                           L = max(1, sum of d), as always. */
    int32_t* durations_out;             /* [B][id_stride]: receives the frames of every token as used, 0 past id_lengths[b]. Filled before
                                           the call returns, before the first on_chunk call, and (vits_model_submit_batch) no later than the
                                           matching vits_model_wait: the buffer must stay valid until then. With fixed_duration > 0 every
                                           token holds fixed_duration. frames_only fills it too. */
} vits_process_opts;

/* The model-level prosody: what vits_model_process, vits_model_process_ids and every call whose prosody arrays are NULL use. Initially the
 * model file's speaking_rate, noise_scale and noise_scale_duration. Returns 0, or -1 (the handle keeps its values) for a rate that is not
 * finite or outside [0.1, 10], or a noise scale that is not finite or outside [0, 10]. Voice conversion ignores these values (it has no
 * duration prediction, and VITS's posterior draw has no noise scale); vits_model_convert_batch refuses the five per-utterance fields.
 * On a model with the deterministic duration predictor (vits_model_duration_predictor_kind == 1) noise_scale_duration is validated
 * and stored as always and has no effect: that predictor draws no noise. */
VITS_API int vits_model_set_prosody(vits_model* model, float speaking_rate, float noise_scale, float noise_scale_duration);
VITS_API int vits_model_get_prosody(const vits_model* model, float* speaking_rate, float* noise_scale, float* noise_scale_duration);

typedef struct vits_batch_result {
    float* data;      /* host [batch][stride] PCM (NULL when skip_host_copy) */
    size_t stride;    /* samples between utterances */
    int64_t* lengths; /* [batch] samples per utterance (at the handle's output rate, vits_model_set_rates; default: the model's) */
    int64_t* frames;  /* [batch] spectrogram frames per utterance (L) */
    size_t batch;
} vits_batch_result;

/* One utterance from ids (already blank-interspersed, i.e. what input_ids_tensor holds at vits.cpp:1109-1111);
 * same noise/mode behaviour as vits_model_process. */
VITS_API vits_result vits_model_process_ids(vits_model* model, const int32_t* ids, size_t n_ids);

/* B independent utterances; ids is host [B][id_stride], id_lengths[b] <= id_stride valid ids in row b.
 * Utterances never interact: results equal B separate batch-1 calls. Returns 0 on success. */
VITS_API int vits_model_process_batch(vits_model* model, const int32_t* ids, const int32_t* id_lengths, int32_t batch,
                                      int32_t id_stride, const vits_process_opts* opts, vits_batch_result* out);
VITS_API void vits_free_batch_result(vits_batch_result* r);

/* ---- voice conversion (VITS SynthesizerTrn.voice_conversion) -------------------------------------------------------------
 * Speech of speaker A in, the same speech in speaker B's voice out. Per utterance b, with PCM y_b of pcm_lengths[b] = N_b samples at
 * the model's sampling rate (a recording at another rate: vits_model_set_rates' input rate resamples it on the device first, and N_b below is
 * the resampled count):
 *   spec   = |STFT(y_b)| (periodic Hann, n_fft = 2 (spectrogram_bins - 1), hop = product of the upsample rates, reflection pad of
 *            (n_fft - hop) / 2 at the utterance's own ends, center = False, sqrt(re^2 + im^2 + 1e-6)): L_b = floor(N_b / hop) frames
 *   z_q    = posterior_encoder(spec, g_src): mean + eps * exp(log_std), eps the [F][L_b] draw prior sampling makes (same noise kinds)
 *   z_p    = flow(z_q, g_src) forward;  z = flow(z_p, g_tgt) reverse;  PCM = decoder(z, g_tgt), as in vits_model_process_batch
 * src_speakers / tgt_speakers: host [B], -1 = no conditioning (a single-speaker model takes -1 only). src = tgt resynthesises.
 * Options: mode, the noise fields, collect_taps, out_device(_stride), skip_host_copy, vocoder_chunk_frames and on_chunk mean what they
 * mean for vits_model_process_batch; fixed_duration, frames_only, async, speaker_ids and the five prosody fields (speaking_rates ..
 * durations_out) are refused, and the model-level prosody (vits_model_set_prosody) has no effect. vits_model_set_ggml_tables affects
 * stage one only, which a conversion never runs: it has no effect here. out: frames[b] = L_b, lengths / stride / data as in TTS.
 * Taps (collect_taps): "spec" [bins][L], "post_mean" / "post_logstd" / "z_q" [F][L], and "noise_prior" (eps), "z_p" (the forward
 * flow's output), "z_flow", "pre_tanh", "waveform".
 * vits_model_prepare_conversion builds what a conversion needs on the device (posterior encoder, its speaker terms, the forward-flow
 * packs); the first conversion runs it implicitly. A handle that never converts keeps its TTS memory and weight_bytes. Returns 0,
 * or -1 + message (no posterior encoder in the file, a tensor of the wrong shape). */
VITS_API int vits_model_prepare_conversion(vits_model* model);
VITS_API int vits_model_convert_batch(vits_model* model, const float* pcm, const int64_t* pcm_lengths, int32_t batch, int64_t pcm_stride,
                                      const int32_t* src_speakers, const int32_t* tgt_speakers, const vits_process_opts* opts,
                                      vits_batch_result* out);
/* One utterance; the model's default mode and the reference noise stream, like vits_model_process. */
VITS_API vits_result vits_model_convert(vits_model* model, const float* pcm, size_t n, int32_t src_speaker, int32_t tgt_speaker);

/* ---- forced alignment: token timings of recorded speech ----------------------------------------------------------------------
 * VITS's own monotonic alignment search (the one it is trained with: SynthesizerTrn.forward, monotonic_align.maximum_path) between the
 * text encoder's prior statistics per token and z_p of a recording. Per utterance b, T = id_lengths[b] tokens, L = floor(N_b / hop) frames:
 *   m, ls  = the prior mean and log-deviation per token, exactly as vits_model_process_batch computes them for these ids (taps
 *            "prior_mean", "prior_logvar"; the text encoder takes no speaker term)
 *   z      = z_p exactly as vits_model_convert_batch computes it for this PCM with src = speakers[b], except that the posterior draw
 *            is z_q = mean + noise_scale * eps * exp(log_std): 1 = VITS's training draw (the conversion's z_q bit for bit), 0 = the
 *            posterior mean (deterministic: no noise is drawn, whatever the noise fields say)
 *   logp[t][j] = sum_c(-0.5 log 2pi - ls[c][t]) - 0.5 sum_c (z[c][j] - m[c][t])^2 exp(-2 ls[c][t]), in fp32 in every arithmetic mode
 *   v[y][x] = logp[x][y] + max(v[y-1][x-1], v[y-1][x]) over the band max(0, T + y - L) <= x <= min(T - 1, y) (-1e9 outside, v[-1][-1] = 0);
 *            the path is read back from (L - 1, T - 1), stepping down a token iff x == y or v[y-1][x] < v[y-1][x-1] (a tie stays)
 * durations[b][t] = frames of token t (>= 1 each, summing to frames[b]; 0 past id_lengths[b]); scores[b] = v[L-1][T-1], the
 * log-likelihood of the best path. The durations are what opts.duration_override of vits_model_process_batch takes: "say this text with
 * the rhythm of that recording". No duration predictor, reverse flow or vocoder runs, and the reference noise stream is advanced by
 * the posterior draw only (not at all with noise_scale 0).
 * Options: mode, the noise fields and collect_taps mean what they mean for vits_model_convert_batch; fixed_duration, frames_only, async,
 * out_device, skip_host_copy, vocoder_chunk_frames, on_chunk, speaker_ids and the five prosody fields are refused, as are a noise_scale
 * that is not finite or outside [0, 10], a speaker outside the model's range, a file without a posterior encoder, batches in flight and
 * an utterance with more tokens than frames (no monotonic path exists; the message names the utterance, its tokens and its frames).
 * vits_model_set_ggml_tables mode 1 governs the duration predictor's stage one only, which an alignment never runs: it is ignored here,
 * as in conversion. The first alignment prepares the conversion weights (vits_model_prepare_conversion) if nothing did before.
 * Taps (collect_taps): "prior_mean", "prior_logvar" [F][T]; "spec", "post_mean", "post_logstd", "z_q", "z_p" as in conversion;
 * "align_logp" [T][L]; "align_path" [L]: the token index of every frame, as floats. Returns 0, or -1 + message. */
VITS_API int vits_model_align_batch(vits_model* model,
        const float* pcm, const int64_t* pcm_lengths, int32_t batch, int64_t pcm_stride,   /* as vits_model_convert_batch */
        const int32_t* ids, const int32_t* id_lengths, int32_t id_stride,                  /* as vits_model_process_batch */
        const int32_t* speakers,        /* host [B] or NULL (= -1 everywhere): the speaker of the recording (posterior encoder, forward flow) */
        float noise_scale,              /* scale of the posterior draw: 1 = VITS's training draw, 0 = the posterior mean (deterministic) */
        const vits_process_opts* opts,  /* mode, noise fields, collect_taps; everything else refused, see above */
        int32_t* durations,             /* out, host [B][id_stride]: frames per token, 0 past id_lengths[b]; sums to frames[b] */
        int64_t* frames,                /* out, host [B], optional */
        float* scores);                 /* out, host [B], optional: log-likelihood of the best path */
/* One utterance from text, through the model's tokenizer; the posterior mean (noise_scale 0). Writes up to cap ids and durations,
 * returns the token count, -1 on failure. Phonetic models refuse as the other text entry points do. */
VITS_API int64_t vits_model_align(vits_model* model, const float* pcm, size_t n, const char* text, int32_t speaker,
                                  int32_t* ids, int32_t* durations, size_t cap);
/* Samples per frame (the product of the vocoder's upsample rates = the STFT hop): token t of an alignment starts at
 * sum(durations[0 .. t)) * hop / sampling_rate seconds. In audio delivered with vits_model_set_edges on, token t of durations_out starts at
 * (sum(d[0 .. t)) * hop - a + Pl) / sampling_rate seconds, a from vits_model_last_edges and Pl = samples(lead_ms) from vits_edges_plan. */
VITS_API int32_t vits_model_hop(const vits_model* model);

/* ---- any sample rate: a device resampler on both sides of the model -----------------------------------------------------------
 * The model speaks one rate (vits_model_sampling_rate). With an OUTPUT rate set, every PCM the handle delivers (vits_model_process,
 * _process_ids, _process_batch, _submit_batch / _wait, _convert, _convert_batch) is the model-rate waveform resampled on the device:
 * lengths[], stride, the out_device_stride check, out_device, the host copy and on_chunk's offsets and counts are all in OUTPUT
 * samples (lengths[b] = ceil(N_b L / M) for a model-rate waveform of N_b samples); frames[] and durations_out are unchanged, and
 * frames_only reports lengths[] at the output rate. Streaming still tiles: after every vocoder window the output samples whose
 * filter taps all lie in finished model-rate samples are delivered, so chunks arrive in order and tile [0, lengths[b]) exactly, the
 * concatenation equals the unchunked result bit for bit, and a window that finalises nothing for an utterance makes no call for it.
 * With an INPUT rate set, the PCM given to vits_model_convert(_batch) and vits_model_align(_batch) is at that rate: it is uploaded and
 * resampled to the model's rate on the device, N' = ceil(N L / M) samples, L_b = floor(N' / hop) frames; the length checks apply to N'
 * (their messages name both counts). Alignment timings stay frames * hop / sampling_rate seconds. 0 = the model's own rate (a rate equal
 * to the model's is stored as 0): no resampling kernel is queued, nothing is allocated, every bit is what it was.
 * Taps: "waveform" stays the model-rate waveform; "waveform_out" [1][lengths[b]] is the delivered PCM (output rate set); "pcm_model"
 * [1][N'] the resampled recording (input rate set).
 *
 * The filter (one definition, both directions). fi -> fo, d = gcd(fi, fo), L = fo / d, M = fi / d. Output sample j sits at input time
 * j M / L: q = j M (64-bit), n_c = q / L, p = q % L. Prototype: a Kaiser-windowed sinc with Z = 32 zero crossings, rolloff = 0.92,
 * beta = 9: s = rolloff min(1, L / M), W = Z / s, R = ceil(W), K = 2 R + 1,
 *   g(t) = s sinc(s t) I0(beta sqrt(1 - (t / W)^2)) / I0(beta) for |t| < W, else 0      (sinc(x) = sin(pi x) / (pi x))
 *   h[p][k] = g(R - k + p / L), computed in double on the host and rounded once to fp32 (no per-phase renormalisation)
 *   y[j] = sum_k h[p][k] x[n_c - R + k], x = 0 outside the utterance's own [0, N); N_out = ceil(N L / M)
 * evaluated as ONE ascending chain per output sample: acc = 0; acc = fmaf(h[p][k], x[.], acc) for k = 0 .. K - 1. Nothing about tiles,
 * batch position or streaming windows enters a sample. Rates in [4000, 192000] Hz; a pair whose table exceeds 2^20 floats (L K, e.g.
 * 16000 -> 44101) is refused with a message naming L and K. The table of a pair is built and uploaded at its first use, kept with the
 * handle and counted in vits_model_weight_bytes.
 *
 * vits_model_set_rates: 0, or -1 + message with the handle unchanged: a rate outside the range other than 0, a table that is too large,
 * batches in flight, or a call from inside on_chunk ("model busy"). */
VITS_API int vits_model_set_rates(vits_model* model, int32_t input_rate, int32_t output_rate);
VITS_API int vits_model_get_rates(const vits_model* model, int32_t* input_rate, int32_t* output_rate);
/* The filter itself: host only, no device needed. vits_resample_plan: 0 and L, M, K (each pointer optional), or -1 + message.
 * vits_resample_taps: writes h as [L][K] when cap >= L K (dst may be NULL with cap 0 to ask for the size); returns L K, -1 on failure.
 * vits_resample_length: ceil(n L / M), -1 on failure. */
VITS_API int vits_resample_plan(int32_t in_rate, int32_t out_rate, int32_t* L, int32_t* M, int32_t* K);
VITS_API int64_t vits_resample_taps(int32_t in_rate, int32_t out_rate, float* dst, size_t cap);
VITS_API int64_t vits_resample_length(int32_t in_rate, int32_t out_rate, int64_t n);

/* ---- a stated level: gain, sample peak and ITU-R BS.1770-4 integrated loudness, on the device -----------------------------------
 * The vocoder's tanh output comes out as it falls; vits_model_set_level(model, kind, value_db, ceiling_db) makes every PCM the handle
 * delivers (vits_model_process, _process_ids, _process_batch, _submit_batch / _wait, _convert, _convert_batch; out_device, skip_host_copy
 * and async included: there is no host read) leave at a stated level. The model-rate waveform x of N samples (tap "waveform", unchanged)
 * is measured, multiplied by one gain g per utterance, and THEN resampled if an output rate is set (vits_model_set_rates): levelling
 * comes before the resampler, never after. Alignment is unaffected. Levelling is the same arithmetic in every VITS_ARITH_* mode.
 *
 * The measurement, at rate fs, mono. K-weighting = two biquads whose coefficients are computed in double on the host from the analogue
 * prototypes (at 48 kHz they are the table of BS.1770):
 *   stage 1 (shelf): f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196, K = tan(pi f0 / fs), Vh = 10^(G / 20),
 *     Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K^2,
 *     b = [Vh + Vb K / Q + K^2, 2 (K^2 - Vh), Vh - Vb K / Q + K^2] / a0,  a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0]
 *   stage 2 (high-pass): f0 = 38.13547087602444, Q = 0.5003270373238773, the same K and a0 formulas,
 *     b = [1, -2, 1],  a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0]
 * S = (fs + 5) / 10 (integer division) samples make a 100 ms segment; segment i covers the utterance's own samples [i S, (i + 1) S);
 * z_i = the mean square of the K-weighted signal over it (filter state zero before sample 0, carried through the whole utterance); a
 * trailing partial segment is dropped. Block j = mean(z_j .. z_(j+3)), j = 0 .. n_seg - 4 (400 ms, 75 % overlap), l_j = -0.691 + 10
 * log10(block_j). Gates: keep the blocks with l_j > -70; Gamma = -0.691 + 10 log10(mean of the kept blocks) - 10; keep those of them with
 * l_j > Gamma; L = -0.691 + 10 log10(mean of those), in LUFS. Fewer than four segments, or no block above -70: the utterance is
 * UNMEASURABLE, L = -inf. P = max |x| over [0, N) is the SAMPLE peak, not the true (inter-sample) peak of BS.1770 annex 2.
 * On the device filter, sums and gates are fp64; L and P are reported in fp32 and g is computed from the reported values.
 *
 *   kind                  gain g (linear)
 *   VITS_LEVEL_NONE       (default) nothing is queued, nothing is allocated, every bit is what it was
 *   VITS_LEVEL_MEASURE    1: measured, nothing applied, the PCM bits unchanged
 *   VITS_LEVEL_GAIN       10^(value_db / 20)
 *   VITS_LEVEL_PEAK       10^(value_db / 20) / P; 1 if P == 0
 *   VITS_LEVEL_LOUDNESS   min(10^((value_db - L) / 20), 10^(ceiling_db / 20) / P); 1 if unmeasurable or P == 0
 * Delivered sample = x * g, one fp32 multiply: no clamp, no limiter beyond the ceiling rule (unless vits_model_set_limiter, below, is on), no dither.
 * vits_model_set_level: 0, or -1 + message with the handle unchanged: an unknown kind, a value that is not finite, value_db outside
 * [-70, 0] (LOUDNESS), [-60, 0] (PEAK) or [-60, 40] (GAIN), ceiling_db outside [-60, 0] (LOUDNESS only; the other kinds ignore it),
 * batches in flight, or a call from inside on_chunk ("model busy").
 * Streaming: with on_chunk only VITS_LEVEL_GAIN is accepted (every window's finished samples are multiplied once, so the chunks still
 * tile the utterance and their concatenation equals the unchunked result bit for bit); the other kinds need the whole utterance before
 * the first sample can leave and are refused with a message that says so. vocoder_chunk_frames without on_chunk works with every kind:
 * levelling runs behind the last window. Taps: "waveform_level" [1][N] is the multiplied model-rate waveform (the waveform itself under
 * VITS_LEVEL_MEASURE); "waveform_out" stays the delivered PCM.
 *
 * vits_model_last_levels: the rows [B][4] = {L in LUFS (-inf: unmeasurable), P linear, g linear, blocks that passed both gates} of the
 * most recently completed call on the handle (process*, convert*, or the batch vits_model_wait returned last), written to dst when cap
 * >= 4 B. Returns 4 B, 0 when that call ran under VITS_LEVEL_NONE, -1 on a null argument. After an async call the values are valid
 * after vits_model_sync. The device row buffer is counted in vits_model_weight_bytes once allocated. */
#define VITS_LEVEL_NONE 0
#define VITS_LEVEL_MEASURE 1
#define VITS_LEVEL_GAIN 2
#define VITS_LEVEL_PEAK 3
#define VITS_LEVEL_LOUDNESS 4
VITS_API int vits_model_set_level(vits_model* model, int32_t kind, float value_db, float ceiling_db);
VITS_API int vits_model_get_level(const vits_model* model, int32_t* kind, float* value_db, float* ceiling_db);
VITS_API int64_t vits_model_last_levels(vits_model* model, float* dst, size_t cap);
/* The measurement itself: host only, no device needed. vits_loudness_plan: the two biquads as b0 b1 b2 a1 a2 each (coef, optional) and
 * S (segment, optional) at a rate in [4000, 192000]; 0, or -1 + message. vits_loudness_host: the definition above in double, sequentially,
 * on n samples at `rate`: *lufs (-inf: unmeasurable), *peak, *blocks (each optional); 0, or -1 + message (a refused rate, pcm NULL with n > 0). */
VITS_API int vits_loudness_plan(int32_t rate, double coef[10], int32_t* segment);
VITS_API int vits_loudness_host(const float* pcm, size_t n, int32_t rate, double* lufs, double* peak, int32_t* blocks);

/* ---- the loudness target under a ceiling: a 4x true-peak meter and a look-ahead limiter, on the device -------------------------------
 * The ceiling rule of VITS_LEVEL_LOUDNESS cuts the gain of a whole utterance when its peaks are high: the utterance leaves quieter than asked,
 * by another amount each time. vits_model_set_limiter(model, VITS_LIMIT_TRUE_PEAK) delivers the gain that was asked for and turns down only
 * the neighbourhood of what would pass the ceiling. It is a stage of the levelling tail (vocoder -> measure -> limiter in place of the plain
 * multiply -> resampler), defined WITHOUT a recurrence, so batch rows, pipelined and split batches, windows and a device buffer give the same
 * bits, in every VITS_ARITH_* mode. With VITS_LIMIT_OFF (the default) nothing is queued or allocated and every bit is what it was.
 *
 * The definition. Model-rate row x[0, N) at rate fs in [4000, 48000] (4 fs is then a rate the resampler accepts); integer divisions truncate.
 *   A = (fs + 100) / 200   5 ms of look-ahead and attack          H = (fs + 10) / 20   50 ms of hold (longer than a pitch period: the gain does
 *                                                                                      not ride the glottal pulses)
 *   u[0, 4N) = x resampled fs -> 4 fs by the filter of vits_model_set_rates (L = 4, M = 1, K = 71): the same table, the same ascending fmaf
 *     chain, bit for bit what vits_op_resample(fs, 4 fs) returns for the row. Nothing behind N is read. The project's own filter is the meter:
 *     this is not the coefficient table of BS.1770 annex 2.
 *   TP(x) = max(P, max_j |u[j]|), P the sample peak: the true peak, exact in fp32 (a maximum does not round)
 *   e[n] = max(|x[n]|, |u[j]| for j in [4n - 2, 4n + 2] within [0, 4N)): the detection envelope; every oversampled point belongs to some n
 *   g0, the gain before limiting:   VITS_LEVEL_GAIN      10^(value_db / 20)
 *                                   VITS_LEVEL_LOUDNESS  10^((value_db - L) / 20), 1 if unmeasurable: the ceiling no longer reduces it
 *                                   VITS_LEVEL_PEAK      10^(value_db / 20) / TP, 1 if TP == 0: true-peak normalisation, delivered by the plain
 *                                                        multiply (no limiter stage: under the stated peak by construction)
 *   c = 10^(ceiling_db / 20); with the limiter on, vits_model_set_level checks and keeps ceiling_db in [-60, 0] under VITS_LEVEL_GAIN too (set the
 *     limiter first: with it off a gain's ceiling is ignored and not kept)
 *   1. r[k] = min(1, c / (g0 e[k])) for k in [0, N), 1 where e[k] == 0 and outside [0, N)
 *   2. m[j] = min(r[j - H .. j + A]) for j in [-A, N): a sliding minimum, exact
 *   3. s[n] = mean(m[n - A .. n]), in fp64, rounded once to fp32
 *   4. y[n] = x[n] * (g0 * s[n]): two fp32 multiplies
 * Every window m[n - A .. n] contains n, so s[n] <= r[n] and |y[n]| <= c in exact arithmetic. Where nothing passes the ceiling s == 1 exactly
 * and the row is x * g0, bit for bit what VITS_LEVEL_GAIN delivers without the limiter. The guarantee holds at the model's rate: a resampler
 * behind the limiter can overshoot slightly, which is not corrected. A, H and the factor 4 are constants of this definition, not knobs. How
 * often a ceiling binds on real speech, and what the limiter does to it audibly, has not been judged: the project's fixtures are synthetic.
 *
 * vits_model_set_limiter: 0, or -1 + message with the handle unchanged: an unknown mode, a model rate above 48000 Hz, batches in flight, a
 * call from inside on_chunk ("model busy"). Under VITS_LEVEL_NONE and _MEASURE nothing is queued. With the limiter on vits_model_last_levels
 * reports g = g0, tap "waveform_level" is the limited model-rate row, and voice conversion delivers through it as through levelling.
 * on_chunk with the limiter on and a kind that multiplies is REFUSED: a sample's gain looks A ahead and H + A back, and the halo of finished
 * samples per window that streaming needs is not built; the message says so. vocoder_chunk_frames without on_chunk works: the limiter runs
 * behind the last window, where levelling runs.
 *
 * vits_model_last_limits: the rows [B][4] = {TP(x) linear, TP(y) linear (a second meter pass over the delivered model-rate row), min_n s[n],
 * the share of samples with s[n] < 1} of the most recently completed call; the return conventions of vits_model_last_levels, 0 when that
 * call ran without the limiter. The device rows are counted in vits_model_weight_bytes once allocated, as is the 4x table. */
#define VITS_LIMIT_OFF 0
#define VITS_LIMIT_TRUE_PEAK 1
VITS_API int vits_model_set_limiter(vits_model* model, int32_t mode);
VITS_API int vits_model_get_limiter(const vits_model* model, int32_t* mode);
VITS_API int64_t vits_model_last_limits(vits_model* model, float* dst, size_t cap);
/* Host only, no device needed. vits_limiter_plan: A, H and the time tile of the device kernels (each optional) at a rate in [4000, 48000]; 0,
 * or -1 + message. vits_limiter_host: the definition above in double, sequentially (u from vits_resample_taps, nothing rounded to fp32), on n
 * samples at `rate` with the gain g0 > 0 and the ceiling ceiling_db in [-60, 0]: y[n] (optional) and limits[4] = {TP(x), TP(y), min s, share}
 * (optional); 0, or -1 + message (a refused rate or value, pcm NULL with n > 0). */
VITS_API int vits_limiter_plan(int32_t rate, int32_t* A, int32_t* H, int32_t* tile);
VITS_API int vits_limiter_host(const float* pcm, size_t n, int32_t rate, double g0, double ceiling_db, double* y, double limits[4]);

/* ---- stated edges: trimmed silence, pauses and fades, on the device ---------------------------------------------------------------------
 * A VITS vocoder delivers frames x hop samples, whatever is in them: the leading and trailing blank tokens of a model come out as near-silence
 * of arbitrary length. vits_model_set_edges states where the delivered audio begins and ends: the near-silence at both ends is trimmed (or
 * kept, VITS_EDGES_PAD), both ends are faded, and digital silence of a stated length is put in front and behind. It is a stage of the delivery
 * tail, in front of levelling (vocoder -> edges -> measure / multiply / limiter -> resampler), so what is measured is what is delivered. It has
 * no atomics and every sum has one shape, so batch rows, pipelined and split batches, vocoder windows and a device buffer give the same bits, in
 * every VITS_ARITH_* mode. With VITS_EDGES_OFF (the default) nothing is queued or allocated and every bit, length and vits_model_weight_bytes is
 * what it was.
 *
 * The definition. Model-rate row x[0, N) at rate fs in [4000, 192000]; integer divisions truncate.
 *   samples(ms) = (int64) floor((double) ms * fs / 1000 + 0.5): Kh, Kt, Fi, Fo, Pl, Pt of the six durations of the desc, in field order
 *   W = (fs + 50) / 100   10 ms. Window i covers [i W, min((i + 1) W, N)), i < n_win = ceil(N / W): the partial last window counts, over its own
 *     samples. q_i = the mean of x^2 over window i in fp64 (a square of an fp32 value is exact in fp64). The association of the sum is the
 *     implementation's; it is fixed per window and depends on nothing outside the window (not on the batch row, not on a tile).
 *   f = 10^(threshold_db / 10), computed once in double on the host. T = q_max f (one fp64 multiply; q_max = the largest q_i that is not a NaN, 0
 *     if there is none) under VITS_EDGES_TRIM_RELATIVE, T = f under VITS_EDGES_TRIM_ABSOLUTE (relative to a mean square of 1).
 *   Window i is active iff q_i >= T and q_i > 0 (a NaN compares false); n_active counts them; i_first and i_last are the first and the last.
 *   a = max(0, i_first W - Kh), b = min(N, (i_last + 1) W + Kt); with no active window a = b = 0. Under VITS_EDGES_PAD a = 0, b = N, nothing is
 *     measured and n_active = 0. M = b - a.
 *   win[k] = 0.5 - 0.5 cos(pi (k + 0.5) / Fi), k < Fi, and wout[k] likewise with Fo: computed in double on the host, rounded once to fp32.
 *   The delivered row has N' = Pl + M + Pt samples: y[j] = +0 for j < Pl and for j >= Pl + M; y[Pl + k] = (x[a + k] * wi) * wo, two fp32
 *     multiplies, wi = win[k] if k < Fi, else 1; wo = wout[M - 1 - k] if M - 1 - k < Fo, else 1. A multiply by 1 is exact: a row that nothing
 *     touches is x bit for bit. Fades longer than M simply overlap; nothing is rescaled.
 *   The bound of a row is N + Pl + Pt >= N': [N', bound) is written as zero, nothing is written behind the bound.
 * Which threshold separates speech from a model's near-silence has not been judged on real speech: the project's fixtures are synthetic.
 *
 * vits_model_set_edges: NULL or mode VITS_EDGES_OFF switches the stage off. 0, or -1 + message with the handle unchanged: a struct_size that is
 * not sizeof(vits_edges_desc), an unknown mode, a value that is not finite or outside its range (threshold_db is not looked at under
 * VITS_EDGES_PAD), batches in flight, a call from inside on_chunk ("model busy"). vits_model_get_edges: the desc as it was set (mode
 * VITS_EDGES_OFF and zeros when off).
 * With the stage on: lengths[b] is N'_b (passed through vits_resample_length when an output rate is set), read from the device after the call's
 * own synchronisation or at vits_model_wait; stride and the out_device_stride check use the bound N_max + Pl + Pt (at the output rate when one
 * is set), which the host knows before the call; frames[] and durations_out are unchanged. frames_only reports lengths[] for the bound: exact
 * under VITS_EDGES_PAD, an upper bound under the TRIM modes: the size to allocate. Levelling, the limiter and the resampler read the trimmed
 * row: vits_model_last_levels and _last_limits describe it. Taps: "waveform" is unchanged, "waveform_edges" [1][N'] is the output of the stage,
 * "waveform_level" and "waveform_out" follow it. Voice conversion delivers through the stage; alignment is unaffected. vocoder_chunk_frames
 * without on_chunk works: the stage runs behind the last window. REFUSED with the stage on, with the reason: on_chunk (the end of the utterance
 * decides what leaves) and async (the lengths need a host read).
 * In the delivered audio token t of durations_out starts at (sum(d[0 .. t)) * hop - a + Pl) / fs seconds (see vits_model_hop).
 *
 * vits_model_last_edges: the rows int64 [B][4] = {a, b, N', n_active} of the most recently completed call, with the conventions of
 * vits_model_last_levels: returns 4 B (dst is filled when cap >= 4 B), or 0 when that call ran with the stage off. The device rows and the fade
 * tables are counted in vits_model_weight_bytes once allocated (by the first call that runs the stage). */
#define VITS_EDGES_OFF 0
#define VITS_EDGES_PAD 1
#define VITS_EDGES_TRIM_RELATIVE 2
#define VITS_EDGES_TRIM_ABSOLUTE 3
typedef struct vits_edges_desc {
    uint32_t struct_size;
    int32_t mode;                     /* VITS_EDGES_OFF 0 | _PAD 1 | _TRIM_RELATIVE 2 | _TRIM_ABSOLUTE 3 */
    float threshold_db;               /* [-120, 0]: relative to the loudest window (RELATIVE) or to mean square 1 (ABSOLUTE); ignored by PAD */
    float keep_head_ms, keep_tail_ms; /* [0, 2000]: original signal kept in front of the first / behind the last active window */
    float fade_in_ms, fade_out_ms;    /* [0, 2000] */
    float lead_ms, tail_ms;           /* [0, 2000]: digital silence put in front / behind */
} vits_edges_desc;
VITS_API int vits_model_set_edges(vits_model* model, const vits_edges_desc* desc);
VITS_API int vits_model_get_edges(const vits_model* model, vits_edges_desc* desc);
VITS_API int64_t vits_model_last_edges(vits_model* model, int64_t* dst, size_t cap);
/* Host only, no device needed. vits_edges_plan: out = {W, Kh, Kt, Fi, Fo, Pl, Pt, the time tile of the device's window kernel (a multiple of W)}
 * at a rate in [4000, 192000]; 0, or -1 + message (what vits_model_set_edges refuses about the desc; mode VITS_EDGES_OFF is accepted here).
 * vits_edges_host: the definition above evaluated sequentially on n samples at `rate`, with the same two fp32 multiplies, so y is comparable bit
 * for bit with the device's: y (optional, y_cap floats, y_cap >= n + Pl + Pt) gets the delivered row and zeros up to the bound, row =
 * {a, b, N', n_active}; 0, or -1 + message (a refused desc or rate, mode VITS_EDGES_OFF, pcm NULL with n > 0, a y_cap below the bound). */
VITS_API int vits_edges_plan(int32_t rate, const vits_edges_desc* desc, int64_t out[8]);
VITS_API int vits_edges_host(const float* pcm, size_t n, int32_t rate, const vits_edges_desc* desc, float* y, size_t y_cap, int64_t row[4]);

/* ---- joined tracks: the utterances of a batch laid end to end, on the device ------------------------------------------------------------
 * The stages above state rate, level, ceiling and edges of ONE utterance; a paragraph is several, laid end to end with a stated gap or overlap.
 * This section states that layout and gives it as a device operator (vits_op_join, on model-rate rows: the rows a call delivers with no level
 * and no output rate set) with its host-only plan and sequential definition, and as a model-level call that joins inside the engine, in front
 * of the handle's level, limiter and resampler (vits_model_process_joined below; vits_model_speak takes a whole text).
 *
 * The definition. Model-rate rows x_b[0, n_b), b = 0 .. B - 1, at rate fs: n_b is the utterance's delivered length, N'_b as the edges stage
 * leaves it, or the vocoder's sample count with the stage off. Integer divisions truncate.
 *   track[b]   the track of utterance b: track[0] = 0 and each step track[b] - track[b - 1] is 0 or 1, so the utterances of a track are
 *              consecutive and in order. NULL: one track. G = track[B - 1] + 1.
 *   gap_ms[b]  a finite float in [-2000, 60000]: the distance between utterance b and its predecessor in the same track. NULL: 0 everywhere. For
 *              the first utterance of a track it is validated and ignored.
 *   g_b = sign(ms) * floor(|ms| * fs / 1000 + 0.5) as int64: the rounding of samples(ms) of the edges definition.
 *   step_b (b not first in its track) = g_b if g_b >= 0, else -v_b with v_b = min(-g_b, n_(b-1) / 2, n_b / 2): no utterance gives more than half
 *              of itself to either neighbour.
 *   o_b = 0 for the first of a track, else o_(b-1) + n_(b-1) + step_b. The track's length is T_g = o_last + n_last.
 *   y_g[j], 0 <= j < T_g, by the utterances of track g with o_b <= j < o_b + n_b: none: +0; one: x_b[j - o_b], bit for bit; two:
 *              x_(b-1)[j - o_(b-1)] + x_b[j - o_b], one fp32 add.
 *   There are never three, and the two are neighbours. o_b - o_(b-1) = n_(b-1) + step_b >= n_(b-1) - n_(b-1) / 2 >= 0 and (o_b + n_b) -
 *   (o_(b-1) + n_(b-1)) = step_b + n_b >= n_b - n_b / 2 >= 0: starts and ends are non-decreasing along a track. And the end of b - 1 is
 *   o_b - step_b <= o_b + n_b / 2 <= o_b + n_b - n_b / 2 <= o_(b+1): utterance b - 1 has ended where b + 1 begins.
 *   bound_g = sum of bound(n_b) + sum of max(g_b, 0) over the track, bound(n_b) being what the host knows of n_b before the rows are read
 *   (N + Pl + Pt under the edges stage, n_b itself where the lengths are on the host): [T_g, bound_g) is written as zero, nothing is written
 *   behind the bound, nothing behind n_b is read.
 * Cross-fades: with the edges stage on and fade_out_ms = fade_in_ms = -gap_ms (and no lead or tail pad), the two raised-cosine tables sum to 1
 * sample by sample (0.5 - 0.5 cos(pi (k + 0.5) / F) and its mirror image), so the overlap is a constant-gain cross-fade, unless the half rule
 * shortened it. With the stage off an overlap is a plain sum, and that is the caller's business. How such a cross-fade sounds on real speech
 * has not been judged: the project's fixtures are synthetic.
 * Only a copy and one add touch a sample: batch position, track partition, tiles and streams enter no bit. */
/* Host only, no device needed. vits_join_plan: utt_bounds [batch] = bound(n_b) of every utterance at `rate` (from a frames_only call, or the
 * lengths themselves), track and gap_ms as defined above -> *tracks_out = G, track_bounds_out [G] (room for `batch` entries) = bound_g,
 * *tile_out = the samples of a track per block of the device's kernel: what a caller sizes the tracks' buffer with. Any output may be NULL. 0,
 * or -1 + message: a batch outside [1, 65535], a track[0] that is not 0 or a step other than 0 or 1, a gap that is not finite or out of range
 * (naming the utterance), a rate outside [4000, 192000], an utterance bound outside [0, 2^30], a track bound above 2^30 (from its pauses alone,
 * or with its utterances).
 * vits_join_host: the definition evaluated sequentially, with the same single fp32 add, so y is comparable bit for bit with the device's. x
 * [batch][x_stride], lens [batch] = n_b (they are their own bounds), y [G][y_stride] (optional; row g gets its bound_g samples, T_g of the
 * track, then zeros), track_lens_out [G] = T_g and offsets_out [batch][2] = {o_b, n_b} (both optional). 0, or -1 + message (as above, a lens[b]
 * above x_stride, a y_stride below the largest bound). */
VITS_API int vits_join_plan(int32_t rate, int32_t batch, const int32_t* track, const float* gap_ms, const int64_t* utt_bounds, int32_t* tracks_out,
                            int64_t* track_bounds_out, int32_t* tile_out);
VITS_API int vits_join_host(int32_t rate, int32_t batch, const float* x, int64_t x_stride, const int64_t* lens, const int32_t* track,
                            const float* gap_ms, float* y, int64_t y_stride, int64_t* track_lens_out, int64_t* offsets_out);

/* ---- text in: the sentences of a paragraph ------------------------------------------------------------------------------------------------------
 * vits_split_sentences (host only) works on the bytes of a NUL-terminated text. A sentence ends at the end of the text, after a run of '.', '!',
 * '?' that ASCII whitespace follows ("a.b" is one span; "wait... what?! ok" is three), or after U+3002, U+FF01 or U+FF1F, which need no
 * whitespace. A whitespace run that holds two or more '\n' ends a span too, and the paragraph: the last span in front of it is of kind 1, every
 * other of kind 0. Leading and trailing ASCII whitespace is dropped from each span; a span that is empty, or holds terminators alone, is not
 * reported. Returns the number of spans; the first `cap` of them are written as byte ranges [starts[i], ends[i]) and kinds[i] (any array may be
 * NULL), so a call with cap = 0 sizes the arrays. -1 + message: text NULL.
 * The kinds are what a caller picks the gap in front of the next sentence by (vits_join_plan: gap_ms). */
VITS_API int64_t vits_split_sentences(const char* text, int64_t* starts, int64_t* ends, int32_t* kinds, size_t cap);

/* ---- a batch joined inside the call; a whole text spoken ----------------------------------------------------------------------------------------
 * vits_model_process_joined is vits_model_process_batch with the join of the section above inside it: the batch runs per utterance up to and
 * including the edges stage (vits_model_set_edges; off: the vocoder's rows), the utterances are laid into the tracks of (track, gap_ms) —
 * exactly vits_join_plan's arguments at the model's rate: NULL = one track, gaps of 0 — with n_b the utterance's delivered length at that
 * point and bound(n_b) what the host knows of it, and the handle's level or limiter and its resampler then run on the G TRACKS: a level is
 * measured over the programme, not over each sentence. The result has out->batch = G rows: lengths[g] = T_g (at the output rate if one is set),
 * frames[g] = the sum of the frames of the track's utterances, data [G][stride]; out_device is [G][out_device_stride] and must hold the largest
 * track's bound at the delivered rate (a frames_only call returns exactly those bounds as lengths[g], and the summed frames; a full call stays
 * within them). With the join as the last stage, [T_g, bound_g) of a row is +0 and nothing is written behind bound_g.
 * Reports: vits_model_last_edges keeps its B rows; vits_model_last_levels and vits_model_last_limits have G rows, one per track;
 * vits_model_last_joins writes int64 [B][4] = {index, track, o_b, n_b} of the most recently completed joined call (0 rows after any other
 * call), o_b and n_b in samples at the MODEL's rate, index = b (under vits_model_speak: the span's index). With an output rate set, the
 * position of utterance b in its delivered track is vits_resample_length(model rate, output rate, o_b) samples: the same integer rule that
 * gives lengths[g] from T_g. Returns the number of rows, -1: model NULL.
 * Synchronous, and simple on purpose: it never splits the batch across the front-end stream and has no submit form. Taken: the host copy,
 * out_device, skip_host_copy, vocoder_chunk_frames (without on_chunk), fixed_duration, durations_out, every prosody and speaker field, every
 * arithmetic mode, frames_only. Refused with a message under the prefix "vits_model_process_joined:": on_chunk, async, collect_taps (the taps
 * in front of the join are per utterance, those behind it per track), a noise kind other than VITS_NOISE_COUNTER or VITS_NOISE_EXPLICIT,
 * everything vits_join_plan refuses, an out_device_stride below a track's bound (naming the track and the samples it needs); and "batches in
 * flight". What the host can decide from the arguments is refused before anything is queued: with fixed_duration > 0 that is every bound; with
 * predicted durations the bounds are checked directly behind the read of the frame counts, before the flow and the vocoder are queued. A call
 * that fails later (an allocation) returns with the device idle.
 *
 * vits_model_speak: vits_split_sentences cuts `text`, every span is tokenised with the model's tokenizer, and the spans that have ids form ONE
 * batch of one joined call with noise VITS_NOISE_COUNTER. The gap in front of a span is sentence_gap_ms, or paragraph_gap_ms where the span in
 * front of it ended a paragraph (both in vits_join_plan's range); track_per_paragraph = 1 gives each paragraph its own track, 0 one track. A
 * span that tokenises to no ids (no symbol the tokenizer knows: the lone blank of an add_blank model counts as none) is dropped, and if it
 * ended its paragraph the span in front of it does. `index` of vits_model_last_joins is the
 * span's index in vits_split_sentences order, so the caller keeps the byte ranges. opts NULL: gaps of 0, one track. opts->process (optional)
 * carries what vits_model_process_joined takes of vits_process_opts — speaker through the handle's default or voices, the model-level
 * prosody, noise_seed, mode, out_device, skip_host_copy, frames_only ... — except the per-utterance arrays, whose length a caller cannot know
 * before the text is cut: speaker_ids, speaking_rates, noise_scales, noise_scale_durations, duration_override, durations_out,
 * noise_seed_offsets and noise_prior are refused, as is a noise_kind other than VITS_NOISE_COUNTER. Also refused: a NULL or empty text, a text
 * without a speakable span, a span above 2048 ids (naming it), a phonetic model and an add_blank = 0 file as the other text entry points
 * refuse them. */
typedef struct vits_speak_opts {
    uint32_t struct_size;
    float sentence_gap_ms, paragraph_gap_ms; /* the gap in front of a sentence / in front of the first sentence of a paragraph; vits_join_plan's range */
    int32_t track_per_paragraph;             /* 0: one track; 1: each paragraph its own track */
    const vits_process_opts* process;        /* optional: speaker, prosody (model-level values), noise_seed, arithmetic mode, out_device ... */
} vits_speak_opts;
VITS_API int vits_model_process_joined(vits_model* model, const int32_t* ids, const int32_t* id_lengths, int32_t batch, int32_t id_stride,
                                       const vits_process_opts* opts, const int32_t* track, const float* gap_ms, vits_batch_result* out);
VITS_API int64_t vits_model_last_joins(vits_model* model, int64_t* dst, size_t cap);
VITS_API int vits_model_speak(vits_model* model, const char* text, const vits_speak_opts* opts, vits_batch_result* out);

/* ---- a stated pitch: a ratio per utterance, varispeed on the device -----------------------------------------------------------------------
 * VITS has no F0 input. What it has is a free time stretch: speaking slower by p is the duration predictor's own length scale. So an utterance
 * with pitch ratio p is (1) spoken at the speaking rate r' = (float)((double)rate / (double)p) and (2) played back p times faster by the
 * band-limited interpolator below, at the model's rate, in front of the edges stage: the delivered duration is what it would have been without a
 * pitch, and every frequency of the voice is multiplied by p. Pitch and formants move together, as with any varispeed: fine for the 2 or 3
 * semitones the control is used for. Formant-preserving shifting is not built.
 *
 * The definition. p is a float in [0.5, 2]; vits_pitch_ratio(semitones) = (float)exp2((double)semitones / 12); p = 1 means off. All positions are
 * integers, so device, host and any restatement agree on every index:
 *   P = p 2^24 (an exact integer for every float in the range). A row of N samples gives N' = ceil(N 2^24 / P) samples.
 *   Output m sits at t = m P (64-bit): n0 = t >> 24, f = t & (2^24 - 1).
 *   Prototype: the resampler's Kaiser-windowed sinc (Z = 32 zero crossings, beta = 9, rolloff 0.92), tabulated at Q = 256 points per zero crossing:
 *     G[i] = fp32(g0(i / Q)), g0(u) = sinc(u) I0(beta sqrt(1 - (u / Z)^2)) / I0(beta), i = 0 .. Z Q - 1;  G[Z Q] = G[Z Q + 1] = 0
 *     D[i] = G[i + 1] - G[i] in fp32, i = 0 .. Z Q;  D[Z Q + 1] = 0.        Both tables are public: vits_pitch_table.
 *   Per row: S0 = 15435038 (= floor(0.92 2^24)); S = S0 when P <= 2^24, else (S0 << 24) / P (integer division); a = S / 2^24 (exact in fp32);
 *     R = ceil(2^29 / S), K = 2 R + 1: 71 taps up to p = 1, 141 at p = 2.
 *   Tap k of output m: tau = |(k - R) 2^24 - f|, u = (tau S) >> 24, i = u >> 16, fr = (u & 65535) 2^-16;
 *     h = 0 where i >= Z Q, else h = a fmaf(fr, D[i], G[i]).
 *   y[m] is ONE ascending chain: acc = 0; acc = fmaf(h, x[n0 - R + k], acc) for k = 0 .. K - 1, x = 0 outside the row's own [0, N).
 *   A row with P = 2^24 is copied bit for bit (the filter at p = 1 is a 0.92-Nyquist low-pass, not an identity).
 * Rows are finite: where h = 0 the device still runs fmaf(+0, x, acc), so an Inf or NaN sample poisons the outputs within R samples of it even where its
 * weight is 0 (vits_pitch_host skips such a tap); for finite rows the bits are the same either way.
 * Nothing about tiles, batch position or neighbouring rows enters a sample. Restated in float64 (tests/pitch_ref.py): a 440 Hz tone comes out
 * within 0.03 Hz of 440 p from -12 to +12 semitones; tones whose shifted frequency passes Nyquist come out at -95 dB or lower; the table with
 * linear interpolation differs from the exact sinc by at most 3.3e-5 of the output RMS on white noise.
 *
 * In a call. The model value (vits_model_set_pitch, initially 1) holds for every utterance of every call. vits_model_set_pitch_ratios(model, ratios,
 * n) gives the NEXT call one ratio per utterance instead (host [n], copied at once); NULL or n = 0 drops them. Exactly these calls take them, as the
 * first thing they do once the engine has the call, and they are gone when the call returns, whether it succeeded or not: vits_model_process,
 * _process_ids, _process_batch, _submit_batch, _process_joined, _speak, _convert, _convert_batch, _align and _align_batch. A call that never reaches
 * the engine — a NULL model, ids, PCM or text, an empty input, a text the tokenizer refuses, "model busy" from inside on_chunk — leaves them where
 * they are. Nothing else touches them: not vits_model_wait or _sync, not a setter, a getter, a tap or a report. A caller whose call may have
 * been refused that early drops them itself before it goes on (the Python wrappers do). vits_process_opts keeps its size: like every delivery
 * setting, pitch is stated on the handle, not in a field. Taken by vits_model_process, _process_ids, _process_batch, _submit_batch / _wait (bit for bit
 * what _process_batch gives) and vits_model_process_joined (per utterance: a programme may mix pitches); n must be the call's batch. vits_model_speak
 * takes the model value only and refuses given ratios as it refuses the per-utterance arrays. For an utterance with p_b != 1
 * the call is, bit for bit, the same call with speaking rate r'_b — refused, naming the utterance, when r'_b leaves [0.1, 10] — followed by the
 * varispeed of its vocoder row. Everything behind the vocoder sees the final audio: edges, join, level, limiter, the output resampler, PCM16.
 * lengths[] (and so frames_only, the out_device_stride check and a joined call's bounds) derive from N'; frames[] and durations_out stay the
 * model's frames: token t of durations_out starts at sum(d[0 .. t)) * hop * 2^24 / P model-rate samples (with the edges stage on, minus a plus
 * Pl as in vits_model_hop's note). Taken with vocoder_chunk_frames (without on_chunk), out_device and skip_host_copy.
 * Refused before anything is queued, each with a message: on_chunk or async with any ratio != 1 (streaming pitch is not built); fixed_duration >
 * 0 or duration_override on an utterance with ratio != 1 (the stretch is the duration predictor's); a ratio that is not finite or outside [0.5,
 * 2]; given ratios in vits_model_convert_batch and vits_model_align_batch, where the model value has no effect either, as with prosody.
 * A vits_model_process_batch call that shifts is never split across the front-end stream inside the call (one launch serves the whole batch and the
 * report has a row per utterance); its bits are the unsplit call's either way.
 * Tap "waveform_pitch" [1][N'] is the stage's output; "waveform" stays the vocoder's row. vits_model_last_pitch writes int64 [B][3] = {P, N, N'}
 * of the most recently completed call, 0 rows when it shifted nothing; returns the number of rows, -1: model NULL. With every ratio 1 nothing is
 * queued and nothing is allocated: every bit and vits_model_weight_bytes are what they were. The interleaved table (64 KiB) is uploaded by the
 * first call that shifts, kept with the handle and counted in vits_model_weight_bytes.
 *
 * vits_model_set_pitch: 0, or -1 + message with the handle unchanged (a ratio that is not finite or outside [0.5, 2]). vits_model_set_pitch_ratios: 0,
 * or -1 + message (n < 0, ratios NULL with n > 0); the values are checked by the call that takes them, whose message names the utterance.
 * Host only, no device needed. vits_pitch_plan: 0 and P, S, R, N' of a row of n samples (each pointer optional), or -1 + message (a ratio that
 * is not finite or outside [0.5, 2], n outside [0, 2^30]). vits_pitch_table: writes [2][Z Q + 2] floats, G then D, when cap holds them (dst may
 * be NULL with cap 0 to ask for the size); returns 2 (Z Q + 2), -1 on failure. vits_pitch_host: the definition evaluated in double,
 * sequentially, from the same two tables: y (cap >= N' doubles) gets the row; returns N', -1 + message on failure. */
VITS_API float vits_pitch_ratio(float semitones);
VITS_API int vits_pitch_plan(float ratio, int64_t n, int64_t* P, int64_t* S, int32_t* R, int64_t* n_out);
VITS_API int64_t vits_pitch_table(float* dst, size_t cap);
VITS_API int64_t vits_pitch_host(const float* x, int64_t n, float ratio, double* y, size_t cap);
VITS_API int vits_model_set_pitch(vits_model* model, float ratio);
VITS_API int vits_model_get_pitch(const vits_model* model, float* ratio);
VITS_API int vits_model_set_pitch_ratios(vits_model* model, const float* ratios, int32_t n);
VITS_API int64_t vits_model_last_pitch(vits_model* model, int64_t* dst, size_t cap);

/* ---- a stated tempo: a pitch-preserving time stretch of PCM, on the device -------------------------------------------------------------------
 * A voice conversion predicts no durations, so it has no free stretch to pay for a rate or a pitch with. What serves it is a time stretch of the
 * PCM itself: waveform-similarity overlap-add, with every decision made in integers, so that device, host and any restatement agree bit for bit.
 *
 * The definition. The stage runs per row: N samples at the rate sr, and a tempo q, a float in [0.5, 2]; q > 1 is faster, q = 1 is off.
 *   Plan: H = 4 floor(sr / 400) is the hop and the cross-fade length (160 at 16 kHz, 220 at 22.05 kHz); D = 4 floor(sr / 500) the search radius (128,
 *     176); Q = q 2^24 (an exact integer); N' = ceil(N 2^24 / Q) (vits_pitch_plan's formula); F = ceil(N' / H) segments.
 *   Search signal: xq[n] = 0 for a NaN sample, else clamp(rint(x[n] 32768), -32768, 32767) (to nearest even; the product is exact); xq[n] = 0 and
 *     x[n] = 0 outside the row's own [0, N).
 *   Segment starts s_k, k = 0 .. F: s_0 = 0. For k >= 1, a_k = (k H Q) >> 24 in 64 bits and c_k = s_(k-1) + H, where the segment before would go
 *     on. SAD_k(d) = sum over i < H of |xq[c_k + i] - xq[a_k + d + i]| for d in [-D, D], exact in integers. s_k = a_k + d*, d* the FIRST minimum in
 *     the order 0, -1, +1, -2, +2, .., -D, +D: ties go to the smallest |d|, of two equal |d| to the negative one. Silence keeps d = 0.
 *   Output, for m = k H + i < N', 0 <= i < H: w[i] = fp32(2 i + 1) / fp32(2 H) (one correctly rounded division), v[i] = w[H - 1 - i],
 *     y[m] = fp32(fp32(v[i] x[s_(k-1) + H + i]) + fp32(w[i] x[s_k + i])), with s_(-1) = -H: two rounded products and one rounded add, never
 *     contracted into a fused multiply-add.
 *   A row with Q = 2^24 is copied bit for bit.
 * Nothing about tiles, batch position or neighbouring rows enters a sample or an offset. Measured on the restatement (tests/tempo_ref.py) with
 * five-harmonic tones, F0 83 to 311 Hz, 1 s at 16 kHz, q from 0.5 to 2: the energy outside +-8 Hz of the harmonics stays below -33 dB of the
 * total (the same overlap-add with every d = 0 scores about 0 dB), the spectral peak within 0.1 Hz, the RMS within 0.1 %.
 *
 * In a conversion. vits_model_set_conversion_prosody(model, rate, pitch) states the rate r and the pitch p of every utterance of every conversion (both
 * initially 1; vits_model_get_conversion_prosody reads them, each pointer optional). vits_model_set_conversion_ratios(model, rates, pitches, n) gives the
 * NEXT conversion one pair per utterance instead (host [n] each, copied at once; either array may be NULL: the model value for every utterance; both
 * NULL or n = 0 drops what was given). Only vits_model_convert and vits_model_convert_batch take the pairs, as the first thing they do once the engine
 * has the call, and they are gone when that call returns, whether it succeeded or not. Nothing else touches them: no text-to-speech call, no alignment,
 * no setter, getter, tap or report. vits_process_opts keeps its size. Per utterance q = (float)((double)r / (double)p): the time stretch runs with
 * q on the vocoder's row at the model's rate, and when p != 1 the varispeed of "a stated pitch" then runs with p on the stage's output (it restores
 * the duration the rate asks for and multiplies every frequency by p). The result is, bit for bit, the plain conversion followed by vits_op_tempo, then
 * vits_op_pitch. Everything behind them sees the final audio: edges, level, limiter, the output resampler, PCM16. lengths[] derives from the final
 * length; frames[] stays floor(N / hop). Taken with vocoder_chunk_frames (without on_chunk), out_device and skip_host_copy.
 * Refused before anything is queued, each with a message that names the utterance: r, p or q not finite or outside [0.5, 2]; another count of pairs
 * than utterances; on_chunk with any r or p other than 1; a model rate outside [8000, 48000] with any r or p other than 1. The ratios of
 * vits_model_set_pitch_ratios and the prosody fields stay refused in a conversion, and vits_model_set_pitch has no effect there.
 * Tap "waveform_tempo" [1][N'] is the stage's output ("waveform_pitch" the varispeed's behind it; "waveform" stays the vocoder's row).
 * vits_model_last_tempo writes int64 [B][4] = {Q, N, N', F} of the most recently completed call (cap >= 4 B), 0 rows when it stretched nothing; returns
 * the number of rows, -1: model NULL. With r = p = 1 everywhere nothing is queued and nothing is allocated: every bit and vits_model_weight_bytes are
 * what they were. The stage keeps no table on the device.
 * vits_model_set_conversion_prosody: 0, or -1 + message with the handle unchanged. vits_model_set_conversion_ratios: 0, or -1 + message (n < 0); the
 * values are checked by the conversion that takes them.
 *
 * Host only, no device needed. vits_tempo_plan: 0 and H, D, Q, F, N' of a row of n samples (each pointer optional), or -1 + message (a rate
 * outside [8000, 48000], a tempo that is not finite or outside [0.5, 2], n outside [0, 2^30]). vits_tempo_host: the definition evaluated
 * sequentially: y (y_cap >= N' floats) gets the row and offsets (optional; offsets_cap >= F) d*_k for k = 1 .. F; returns N', -1 + message on
 * failure. */
VITS_API int vits_tempo_plan(int32_t rate, float tempo, int64_t n, int32_t* H, int32_t* D, int64_t* Q, int64_t* F, int64_t* n_out);
VITS_API int64_t vits_tempo_host(const float* x, int64_t n, int32_t rate, float tempo, float* y, size_t y_cap, int32_t* offsets, size_t offsets_cap);
VITS_API int vits_model_set_conversion_prosody(vits_model* model, float rate, float pitch);
VITS_API int vits_model_get_conversion_prosody(const vits_model* model, float* rate, float* pitch);
VITS_API int vits_model_set_conversion_ratios(vits_model* model, const float* rates, const float* pitches, int32_t n);
VITS_API int64_t vits_model_last_tempo(vits_model* model, int64_t* dst, size_t cap);

/* ---- a stated duration: the length scale fitted to a target frame count, on the device ---------------------------------------------------------
 * A dubbing, subtitle or prompt slot gives a sentence a time. VITS has the lever, the duration predictor's length scale, d = ceil(exp(logw) s), but the
 * sum of those steps cannot be inverted from outside the call. The fit finds the scale inside stage one, directly in front of the durations kernel.
 *
 * The definition. IEEE fp32 multiply, ceil and integer arithmetic only: device, host (vits_fit_host) and any restatement (tests/fit_ref.py) agree on
 * every integer. A group is a set of utterances of one call, taken in batch order, each with its tokens in order.
 *   Token t has e_t = expf(logw_t), the value the durations kernel evaluates, and fixed_t: the caller's duration_override, or -1.
 *   The group has a target F in [1, 2^22] frames and the call the rate limits 0.1 <= min_rate <= max_rate <= 10.
 *   A free token lasts c_t(s) = (int64) min(ceilf(e_t s), 16777216.f) frames at the scale s; a fixed token c_t = fixed_t. n(s) = sum c_t(s) in int64:
 *     non-decreasing in the bit pattern of a positive s.
 *   Scale limits, the engine's own expression for a rate: s_lo = (float)(1.0 / (double)max_rate), s_hi = (float)(1.0 / (double)min_rate).
 *   If n(s_lo) > F: s* = s_lo, status 1 (the text does not fit even at the fastest rate allowed; the frames exceed the target).
 *   Else if n(s_hi) <= F: s* = s_hi, status 0 when n = F and 2 otherwise (the frames fall short of the target).
 *   Otherwise bisect on the unsigned bit patterns between s_lo and s_hi (lo, hi; mid = lo + (hi - lo) / 2; n(mid) <= F moves lo, else hi; until
 *     hi - lo = 1): s* = the largest float with n(s*) <= F, in at most 26 steps on the full range.
 *   Remainder: s+ = the next float after s*, R = F - n(s*) >= 0; non-zero only where several tokens step at the same float, as with equal logw. The
 *     R frames go to the free tokens in (utterance, token) order, token t receiving min(c_t(s+) - c_t(s*), what is left). n(s+) > F, so this ends
 *     with sum d = F: status 0.
 *   Per token d_t = c_t(s*) plus its share of the remainder; per group {F, sum d, s*, R, status}.
 * A clamped group (status 1 or 2, or 0 at s_hi) has R = 0 and the durations of a speaking_rates call at max_rate or min_rate.
 *
 * In a call. vits_model_set_fit(model, target_frames, groups, n, min_rate, max_rate) states the fit of the NEXT call on the handle (arrays copied at once):
 * groups[b] in [0, n) is the group of utterance b, NULL = utterance b is its own group; target_frames[g] is the target of group g, 0 = the group is not
 * fitted and its utterances run as always; n must be the call's batch. NULL with n = 0 drops a pending fit. vits_model_set_fit_total(model,
 * total_frames, min_rate, max_rate): the next call's utterances form ONE group, whatever their number: a whole text at one tempo in a stated time. The
 * argument shape is checked by the setter; the values by the call that takes them, whose message names the group. vits_process_opts keeps its size:
 * like a pitch, the fit is stated on the handle. Exactly the calls that take the ratios of vits_model_set_pitch_ratios take it, at the same moment,
 * and it is gone when that call returns, whether it succeeded or not. vits_model_process, _process_ids, _process_batch, _submit_batch / _wait (bit
 * for bit what _process_batch gives) and _process_joined use it; vits_model_speak uses the total form and refuses the per-group form, as it refuses
 * per-utterance arrays; conversion and alignment, which predict no durations, refuse it.
 * The fit writes the override rows the durations kernel then reads: the call is, bit for bit, the same call with duration_override = its own
 * durations_out, and nothing behind stage one knows that a fit happened. Taken with frames_only, durations_out, duration_override (those tokens stay
 * fixed), speakers and voices, both duration predictors, every arithmetic mode and scope, vocoder_chunk_frames and on_chunk. A fitted utterance's
 * speaking rate is the fit's result: the model-level rate and speaking_rates[b] are validated as always and not used for that utterance.
 * A call that fits is never split across the front-end stream inside the call (a group stays in one launch); its bits are the unsplit call's.
 * frames[] stays max(1, sum d) per utterance, as with any duration_override: a member of a larger group whose tokens are ALL fixed at 0 still reports (and
 * is spoken as) one frame, so the summed frames[] of such a group exceed F by one per such member while vits_model_last_fit reports sum d = F.
 * Refused before anything is queued, each with a message: fixed_duration > 0; vits_model_set_ggml_tables(model, 1), whose duration is not exp x scale;
 * async; a fitted utterance with a pitch ratio other than 1 (the varispeed's stretch and the fit both own the length scale); a target outside [1,
 * 2^22]; rates outside the range; n different from the batch.
 * A target counts spoken frames only: gaps, trimmed edges and pads of a joined call are the caller's to subtract. vits_model_fit_frames(model,
 * seconds) is the largest L with L hop + sadd <= seconds x the model's rate (the frames-to-samples rule of INTEGRATION.md §5, in the model's mode), at
 * least 1; -1: model NULL or seconds not finite.
 * Tap "fit_exp" [1][T] is e. vits_model_last_fit writes double [B][6] = {group, F, sum d of the group, s*, R, status} per utterance of the most recently
 * completed call (cap >= 6 B; an utterance whose group was not fitted: F = 0, status -1), 0 rows when it fitted nothing; returns the number of rows,
 * -1: model NULL. With nothing set no kernel is queued and no scratch is taken: every bit and vits_model_weight_bytes are what they were.
 *
 * Host only, no device needed. vits_fit_host: e and fixed (optional) host [batch][t_stride], lens [batch] (optional: t_stride each), groups [batch]
 * (optional), target_frames [batch] by group -> dur_out int32 [batch][t_stride] (d_t of a fitted utterance's tokens, fixed_t of every other token, -1
 * behind every length) and group_rows_out double [batch][5] = {F, sum d, s*, R, status} by group (status -1: not fitted, or no utterance names the
 * group). 0, or -1 + message: a null argument, an empty batch, a length outside [0, t_stride], a fixed value below -1 or above 2^24, a group outside
 * [0, batch), a target outside [1, 2^22] and not 0, rates that are not finite or not 0.1 <= min_rate <= max_rate <= 10. */
VITS_API int vits_fit_host(int32_t batch, int32_t t_stride, const float* e, const int32_t* fixed, const int32_t* lens, const int32_t* groups,
                           const int64_t* target_frames, float min_rate, float max_rate, int32_t* dur_out, double* group_rows_out);
VITS_API int vits_model_set_fit(vits_model* model, const int64_t* target_frames, const int32_t* groups, int32_t n, float min_rate, float max_rate);
VITS_API int vits_model_set_fit_total(vits_model* model, int64_t total_frames, float min_rate, float max_rate);
VITS_API int64_t vits_model_fit_frames(const vits_model* model, double seconds);
VITS_API int64_t vits_model_last_fit(vits_model* model, double* dst, size_t cap);

/* Block until everything queued by this model has finished. */
VITS_API int vits_model_sync(vits_model* model);

/* ---- pipelined batches on ONE handle ------------------------------------------------------------------------------------
 * vits_model_process_batch is one call in, one result out: its stage one (text encoder + duration predictor, vits.cpp:244-440,
 * 927-972: ~110 small, latency-bound launches in exact fp32) runs with the matrix cores mostly idle, and the host read of the
 * frame counts (vits.cpp:1133) drains the device once per call. The pair below keeps up to TWO batches in flight on one model
 * handle: vits_model_submit_batch(i + 1) queues stage one of batch i + 1 on the handle's front-end stream (its own stage-one
 * arena), where it runs UNDER the flow / vocoder kernels of batch i, reads its frame counts while the device is busy, queues its
 * flow + vocoder behind batch i's on the main stream and returns; vits_model_wait() returns the results of the OLDEST submitted
 * batch (in submission order). Every kernel is batch-invariant and runs on the same operands as in vits_model_process_batch, so
 * the PCM, lengths and frames are BIT-IDENTICAL to it (GPU test). Typical loop:
 *     submit(0); for (i = 1; i < n; ++i) { submit(i); wait(&r[i-1]); } wait(&r[n-1]);
 * Restrictions (checked; -1 + vits_last_error): VITS_NOISE_COUNTER only (no host noise buffers outlive the call), no collect_taps,
 * on_chunk, frames_only or async; at most two batches in flight; opts.out_device buffers of in-flight batches must be distinct.
 * While batches are in flight the other entry points that use the device (process*, set_arith, taps) refuse with "batches in flight".
 * With the per-kernel profiler enabled the two stages run serialised on the main stream (events need non-overlapping kernels).
 * Both return 0 on success. vits_model_pending = number of submitted batches not yet waited for (0..2). */
VITS_API int vits_model_submit_batch(vits_model* model, const int32_t* ids, const int32_t* id_lengths, int32_t batch, int32_t id_stride,
                                     const vits_process_opts* opts);
VITS_API int vits_model_wait(vits_model* model, vits_batch_result* out);
VITS_API int vits_model_pending(const vits_model* model);

/* Tokenizer only (src/vits_tokenizer.cpp:182-208). Writes up to cap ids, returns the count (0 for a model file with add_blank = 0, as the
 * reference; -1 with vits_last_error() for a phonetic model or a NULL argument). */
VITS_API int64_t vits_model_tokenize(vits_model* model, const char* text, int32_t* ids, size_t cap);

/* Model facts. */
VITS_API int32_t vits_model_sampling_rate(const vits_model* model);
VITS_API int32_t vits_model_vocab_size(const vits_model* model);
VITS_API int64_t vits_model_weight_bytes(const vits_model* model);
/* The model's duration predictor: 0 = the stochastic, flow-based one (use_stochastic_duration_prediction = True), 1 = the deterministic one
 * (False: transformers VitsDurationPredictor), -1 for NULL. A deterministic model computes, per utterance of T tokens with text-encoder output
 * x [H][T] and speaker embedding g (or none, speaker -1):
 *   x'[c][t] = x[c][t] + (cond.W g + cond.b)[c] for 0 <= t < T, 0 outside            (the speaker term is added to the INPUT of a padded conv: the
 *                                                                                     first and last k / 2 tokens see zeros, not cond(g), beyond the ends)
 *   a1 = LayerNorm_channels(relu(conv_1(x'))), a2 = LayerNorm_channels(relu(conv_2(a1))), each 0 outside [0, T); logw = proj(a2)
 *   d[t] = ceil(exp(logw[t]) * length_scale), with duration_override and fixed_duration as for the stochastic predictor
 * in fp32 in every VITS_ARITH_* mode and both arithmetic scopes, the same in VITS_MODE_REFERENCE and VITS_MODE_HF (the reference refuses such
 * models, vits.cpp:993: there is no reference arithmetic to reproduce). It draws NO noise: VITS_NOISE_REFERENCE does not advance the
 * process-global stream for a duration draw, VITS_NOISE_EXPLICIT does not need noise_dur, "noise_dur" is not a tap, and noise_scale_duration
 * (vits_model_set_prosody, opts.noise_scale_durations) is validated and has no effect. One fused kernel where an instantiation exists
 * ((hidden, filter, k) = (192, 256, 3), (192, 256, 5), (16, 32, 3)), bit for bit the un-fused sequence of existing kernels that every other shape
 * runs; VITS_NO_DP_DET_FUSE (read at load) forces the un-fused sequence, VITS_DP_DET_LAT_MAX_BLOCKS moves the threshold between the kernel's
 * two tiles (default 96 blocks of 16 tokens). vits_model_set_ggml_tables(model, 1) — stage one in the exact order shared with the oracle, which
 * has no such predictor — makes calls on such a model fail with a message saying so; mode 2 (the attention soft-max only) is allowed. */
VITS_API int32_t vits_model_duration_predictor_kind(const vits_model* model);

/* Stage outputs of the LAST call with collect_taps=1, for utterance `utt`, copied to host as a dense
 * [channels][len] fp32 array. Names: "enc_out" [192][T], "prior_mean" [192][T], "prior_logvar" [192][T],
 * "log_duration" [1][T], "durations" [1][T] (integer-valued), "z_p" [192][L], "z_flow" [192][L],
 * "pre_tanh" [1][S], "waveform" [1][S], plus "noise_dur" [2][T] (stochastic duration predictor only) and "noise_prior" [192][L].
 * Returns the element count (0 = unknown tap), copies min(count, cap) floats. */
VITS_API int64_t vits_model_get_tap(vits_model* model, const char* name, int32_t utt, float* dst, size_t cap);

/* ---- synthetic model files (no real checkpoint is available) --------------------------
 * Builds a complete model file in the reference's on-disk format (writer
 * scripts/export_vits.py:5-70) with the default MMS-TTS architecture (or the tiny test architecture) and
 * deterministic weights derived from `seed`. Conv weights are stored as fp16 like export_vits.py:87. */
#define VITS_SYNTH_FULL 0 /* VitsConfig defaults == facebook/mms-tts-* architecture */
#define VITS_SYNTH_TINY 1 /* hidden 16 / small vocoder: small enough to commit as a fixture */
#define VITS_SYNTH_BF16 0x100 /* OR-ed in: store conv weights as bf16 (tensor type tag 2, an extension of the format) */
#define VITS_SYNTH_SPEAKERS 0x200 /* OR-ed in: a multi-speaker model (TINY: 4 speakers, embedding 8; FULL: 109 speakers, embedding 256): the
                                     tensors of the model without the flag, unchanged, then embed_speaker and the three kinds of cond layers */
#define VITS_SYNTH_POSTERIOR 0x400 /* OR-ed in: append posterior_encoder.* (transformers names and shapes; FULL: 513 bins, 16 WaveNet layers;
                                      TINY: 9 bins, 2 layers) behind every other tensor, for voice conversion */
#define VITS_SYNTH_DETERMINISTIC 0x800 /* OR-ed in: the deterministic duration predictor (use_stochastic_duration_prediction = False; filter channels
                                          FULL 256, TINY 32) in the stochastic one's place; every other tensor keeps its name, place and values.
                                          duration_predictor_filter_channels is written only when it is not 256, as the exporter does */
VITS_API int vits_synth_model_bytes(uint64_t seed, int32_t arch, char** bytes, size_t* size);
VITS_API void vits_free_bytes(char* bytes);
/* Parse a model file and write it back (host only): byte-exact round trip of the reference's format
 * (reader src/vits_model_data.cpp:29-97 + src/vits_tokenizer.cpp:22-55, writer scripts/export_vits.py:5-70). */
VITS_API int vits_model_file_reserialize(const char* in, size_t in_size, char** out, size_t* out_size);
/* Everything vits_model_load_from_bytes checks before it uploads (container format, hyper-parameters, the shape of every
 * tensor against them), on the host only. 0 = loadable; -1 = rejected (vits_last_error says which tensor and why). */
VITS_API int vits_model_file_validate(const char* bytes, size_t size);
/* Tokenize with the vocabulary stored in a model file, without loading the model onto a device. */
VITS_API int64_t vits_model_file_tokenize(const char* model_bytes, size_t size, const char* text, int32_t* ids, size_t cap);

/* ---- profiling (HIP events on the library's own stream) ------------------------------------------------
 * While enabled every kernel launch is bracketed by hipEventRecord on the launch stream. The report is a
 * JSON object {"kernels":[{"name":..,"calls":..,"ms":..,"flop":..,"bytes":..},...]} written into buf. */
VITS_API int vits_prof_enable(vits_model* model, int32_t on);
VITS_API int vits_prof_reset(vits_model* model);
VITS_API int64_t vits_prof_report(vits_model* model, char* buf, size_t cap);

/* ---- operator-level entry points (host buffers in, host buffers out; for parity tests) ---------------
 * Each mirrors one reference operator so a test can compare the HIP kernel with the oracle's restatement
 * of the same reference lines. All tensors are dense fp32, layout [batch][channels][time], time fastest
 * (== the reference's ggml ne order [time, channels, batch]). lens may be NULL (all = T). */

/* Arithmetic of the operator-level conv entry points below on this thread (VITS_ARITH_*; default fp32).
 * VITS_ARITH_F32_SPLIT: vits_op_conv1d and vits_op_resblock_pair run the split kernels (conv_split.hip) exactly as the
 * engine launches them — weights packed as two bf16 planes, the input converted to its three planes (leaky_relu(pre_slope)
 * first), bias / residual / accum + out_scale in the epilogue — or return -1 with the cause in vits_last_error: a shape the
 * split kernels do not take (c_in a multiple of 32 and >= 128, c_out a multiple of 128, k in {3, 7, 11}, dilation in
 * {1, 3, 5}), post_act != 0, a weight that is not the exact sum of two bf16 values. They never fall back to another kernel.
 * The plane buffers are filled with bf16 NaNs before the conversion, so a read past an utterance's length shows in the
 * result. vits_op_conv_transpose1d has no split form (the upsamplers are fp32 kernels in that mode) and refuses. */
VITS_API int vits_op_set_arith(int32_t arith);
/* Launches of this process (engine and operator calls alike) that ran over a list of existing tiles instead of their dense grid (ragged batches,
 * VITS_TILE_MAP / VITS_NO_TILE_MAP). A counter for tests: the results never depend on the form of a launch. */
VITS_API uint64_t vits_op_tile_map_launches(void);
/* The byte every output buffer of vits_op_conv1d, vits_op_conv_transpose1d, vits_op_resblock_pair and vits_op_resblock holds on the device before the kernels
 * run, on this thread: 0 (the default: what no kernel wrote comes back zero) or 0xFF (an fp32 NaN: a test sees a stray store of any value, zero included). */
VITS_API int vits_op_set_output_fill(int32_t byte);
/* The same-position convolutions of two or three ResBlocks of a vocoder stage as ONE launch (conv_group_kernel; over the lists of existing tiles:
 * conv_group_list_kernel), as the engine's grouped schedule launches them: member i is y_i = leaky_relu(b_i + conv_i(leaky_relu(x_i))) with k[i] taps (11, 7 or 3,
 * each at most once) at `dilation` (1, 3 or 5), channels a multiple of 128, fp32 only. x, y: host [n][batch][channels][t_stride]; w: the members' weights one
 * behind the other, member i [C][C][k[i]] (torch layout); bias: [n][C] or NULL; lens optional. Columns the kernels do not write come back as 0xFF bytes. */
typedef struct vits_conv_group_desc {
    int32_t batch, channels, t, t_stride;
    int32_t n, k[3], dilation;
    float slope;
} vits_conv_group_desc;
VITS_API int vits_op_conv_group(const vits_conv_group_desc* d, const float* x, const float* w, const float* bias, const int32_t* lens, float* y);

/* conv1d_with_bias (vits.cpp:171-176 -> custom-ops.h:680-694) with the fusions the engine uses.
 * y = post( conv(pre(x)) + bias ), pre: 0 none, 1 leaky_relu(slope); post: 0 none, 1 relu,
 * 2 gated tanh*sigmoid over channel halves (vits.cpp:442-450; Cout must be even, output has Cout/2 channels);
 * then y = (y + residual) if residual, y = (y + accum) * out_scale if accum.
 * w is [Cout][Cin][K] (torch layout). pad_left/pad_right zero padding; output length T (same-length conv
 * requires pad_left + pad_right == (K-1)*dilation). */
typedef struct vits_conv1d_desc {
    int32_t batch, cin, cout, t, t_stride;
    int32_t k, dilation, pad_left;
    int32_t pre_act; /* 0 none, 1 leaky_relu */
    float pre_slope;
    int32_t post_act; /* 0 none, 1 relu, 2 gate */
    float out_scale;  /* applied when accum != NULL */
} vits_conv1d_desc;
VITS_API int vits_op_conv1d(const vits_conv1d_desc* d, const float* x, const float* w, const float* bias,
                            const float* residual, const float* accum, const int32_t* lens, float* y);

/* One conv pair of a HiFiGAN ResBlock (vits.cpp:545-581), C -> C, k odd, "same" padding, one slope:
 *   y = x + b2 + conv2(leaky_relu(b1 + conv1(leaky_relu(x)))),  conv1 at `dilation`, conv2 at dilation 1.
 * VITS_ARITH_F32: two conv launches (the intermediate is stored activated). VITS_ARITH_F32_SPLIT: the launch sequence of the
 * engine's un-fused split ResBlocks — the converter writes the planes of leaky_relu(x), conv1 writes ONLY the three planes of
 * its activated result, conv2 reads them with x as its residual — or a refusal as for vits_op_conv1d. The 16-bit modes
 * refuse. w1, w2 are [C][C][K] (torch layout); b1, b2 may be NULL. */
typedef struct vits_resblock_pair_desc {
    int32_t batch, channels, t, t_stride;
    int32_t k, dilation;
    float slope;
} vits_resblock_pair_desc;
VITS_API int vits_op_resblock_pair(const vits_resblock_pair_desc* d, const float* x, const float* w1, const float* b1,
                                   const float* w2, const float* b2, const int32_t* lens, float* y);

/* One whole HiFiGAN ResBlock (vits.cpp:545-581, 622-635) on caller tensors, through the kernel the caller names:
 *   y_{p+1} = y_p + b2_p + conv2_p(leaky_relu(b1_p + conv1_p(leaky_relu(y_p)))),  p < ndil,  conv1_p at dil[p], conv2_p at dilation 1,
 *   out = y_ndil, or with accum: (accum + y_ndil) * out_scale (scale_div: / out_scale).
 * x, accum (optional), y: host [batch][channels][t_stride] fp32; w1, w2: [ndil][C][C][k] (torch layout per conv); b1, b2: [ndil][C] (required: the fused
 * kernels take convs with a bias); lens optional, 0 <= lens[b] <= t <= t_stride. Arithmetic: vits_op_set_arith, VITS_ARITH_F32 / F16 / BF16 (the split
 * arithmetic keeps vits_op_resblock_pair). Columns [0, t) of every row of y are written back: what no kernel wrote comes back zero.
 * variant: 0 the engine's choice for this shape and grid; 1 un-fused: two conv launches per pair as the engine builds them (fp32: launch_conv; 16-bit:
 * launch_conv16 with the group-layout epilogue); 2 one fused pair kernel per pair (rbpair32_kernel / rbpair16_kernel; nr: the column tiles per wave of the
 * C >= 128 16-bit pairs, 4 or VITS_RB16_NARROW_NR (2), 0 = the planner's); 3 the whole-ResBlock kernel, one tile per block (rbblock32_kernel / rbblock16_kernel;
 * C = 64, k = 11 included, which the engine only takes in segments); 4 the 16-bit whole-ResBlock kernel walking segments of `tiles` (>= 2) tiles. Variants 1-4
 * return -1 with the cause in vits_last_error where no such instantiation exists (ndil != 3 or dilations other than 1, 3, 5 for variants 3 and 4; C = 128,
 * k = 7 for variant 2 in fp32; variant 4 in fp32; ...): they never fall back to another variant. Every refusal is made before the first device call.
 * Staging is the engine's: fp32 tensors [b][C][ts] with ts = t rounded up to 32, in the 16-bit modes the group layout [b][C/8][ts][8] for the fp32 stream
 * and the 16-bit copy of leaky_relu(y_0) (written by the engine's converter kernel); every pair writes a buffer it does not read. Every staged input and every
 * intermediate buffer holds NaNs (fp32, f16 / bf16) behind lens[b] before the valid part goes in: a read past an utterance shows in the result.
 * All variants give the same bits. Variant 1 gives the bits of vits_op_conv1d called twice per pair (pre_slope, residual, accum / out_scale on the last
 * pair) in the same arithmetic; scale_div has no counterpart there. */
typedef struct vits_resblock_desc {
    int32_t batch, channels, t, t_stride;
    int32_t k, ndil;
    int32_t dil[3];
    float slope, out_scale;
    int32_t scale_div;
    int32_t variant, tiles, nr;
} vits_resblock_desc;
VITS_API int vits_op_resblock(const vits_resblock_desc* d, const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                              const float* accum, const int32_t* lens, float* y);
/* What vits_op_resblock would launch for d in the arithmetic of vits_op_set_arith, or -1 and the cause of its refusal. Host arithmetic only: no device call,
 * so it answers on a machine without a GPU. kernel: the instantiation as the launch-plan tables print it (variant 1: the launcher; its tiles are the conv
 * planner's and the geometry fields are 0). bo: output columns of a block's first tile; advance: of every later tile of a segment (= bo for one-tile
 * kernels); halo: input columns a tile reads beyond its outputs, per side; segment: output columns of a block = bo + (tiles - 1) advance; launches: kernel
 * launches for the whole ResBlock. */
typedef struct vits_resblock_plan {
    char kernel[96];
    int32_t variant; /* the variant that runs (1-4; what 0 resolved to) */
    int32_t bo, advance, halo, segment, tiles, nr;
    int32_t grid_x, grid_y, grid_z, block;
    int64_t lds;
    int32_t launches;
} vits_resblock_plan;
VITS_API int vits_op_resblock_plan(const vits_resblock_desc* d, vits_resblock_plan* plan);

/* One residual-coupling layer of the flow (vits.cpp:500-517, 452-498) on caller tensors, through the kernel the caller names. With H = hidden, per utterance
 * (the sequence is zero outside [0, lens[b])):
 *   h = W_pre x0 + b_pre;  out = 0
 *   l < layers:  g = Conv_k(h, dilation rate^l) + b_in[row_b][l];  a = tanh(g[0:H]) * sigmoid(g[H:2H]);  rs = W_rs[l] a + b_rs[l]
 *                l + 1 < layers: h += rs[0:H], out += rs[H:2H];  the last layer: out += rs
 *   x1' = x1 + (W_post out + b_post);  x0 unchanged
 * The post conv is passed as it is launched: the reverse direction (synthesis) passes the negated weights and bias, as the engine's load does, the forward
 * direction (voice conversion) the plain ones. flipped: 0 = x0 is channels [0, half) of z and x1 channels [half, 2 half); 1 = the other way round (the engine's
 * two placements). z: host [batch][2 half][t_stride] fp32, in and out. Weights in torch layout: w_pre [H][half][1]; w_in [layers][2H][H][k]; w_rs: layers - 1
 * blocks [2H][H][1], then one [H][H][1], concatenated (b_rs the same: layers - 1 times 2H values, then H); w_post [half][H][1]. b_in [n_bias_rows][layers][2H]:
 * the effective-bias table of a multi-speaker model (PackedConv::bias_rs); bias_rows [batch] (optional, NULL = row 0) names each utterance's row. lens optional,
 * 0 <= lens[b] <= t <= t_stride. Arithmetic: vits_op_set_arith, VITS_ARITH_F32 / F16 / BF16 (the split arithmetic is refused).
 * variant: 0 the engine's choice for this arithmetic and grid; 1 un-fused: the 1x1 pre conv, per layer the gated conv and the 1x1 res/skip conv, the post conv
 * with residual x1, as Engine::run_coupling / run_wavenet build them; 2 the fused WaveNet layers between the un-fused pre and post convs (fp32:
 * wavenet32_kernel, whatever the grid; 16-bit: wavenet16_kernel with ncw = 1 or 2 column tiles per wave, 0 = the planner's); 3 flow_couple16_kernel, 16-bit
 * modes only, (ncw, nct) = (1, 1), (1, 2) or (2, 2), (0, 0) = the planner's. Variants 1-3 never fall back to another variant: where no such instantiation exists
 * (variant 2: hidden != 192, k != 5, rate != 1; variant 3 also half != 96, layers != 4, fp32; an (ncw, nct) that does not exist) they return -1 with the cause in
 * vits_last_error. Every refusal is made before the first device call.
 * Staging is the engine's: rows of pitch t rounded up to 32; h lives in rows [0, H) and out in rows [H, 2H) of one [2H] buffer, and in variant 2 h alternates
 * between that buffer and the gate buffer; 16-bit operands through the existing packers and the converter kernel. Every staged input and every intermediate
 * buffer holds NaNs (0xFF bytes) behind lens[b] before the valid part goes in: a read past an utterance shows in the result. Columns [0, t) of every row of z
 * are written back as the device holds them: behind lens[b] that is the staged NaN (all bits set) unless a kernel wrote there.
 * All variants give the same bits; variant 1 gives the bits of the composition of vits_op_conv1d calls in the same arithmetic. */
typedef struct vits_flow_coupling_desc {
    int32_t batch, hidden, half, t, t_stride;
    int32_t k, layers, rate;
    int32_t flipped;
    int32_t n_bias_rows;
    int32_t variant, ncw, nct;
} vits_flow_coupling_desc;
VITS_API int vits_op_flow_coupling(const vits_flow_coupling_desc* d, float* z, const float* w_pre, const float* b_pre, const float* w_in, const float* b_in,
                                   const float* w_rs, const float* b_rs, const float* w_post, const float* b_post, const int32_t* bias_rows, const int32_t* lens);
/* What vits_op_flow_coupling would launch for d in the arithmetic of vits_op_set_arith, or -1 and the cause of its refusal. Host arithmetic only: no device
 * call. kernel: the instantiation as the launch-plan tables print it (variant 1: the launcher, geometry fields 0); bo: output frames per block (64 / 48 / 16);
 * halo: input frames a block reads beyond its outputs, per side (2 for a WaveNet layer, 8 for the coupling kernel); launches: kernel launches for the layer
 * (the converter launches of the 16-bit un-fused convs not counted). */
typedef struct vits_flow_coupling_plan {
    char kernel[96];
    int32_t variant; /* the variant that runs (1-3; what 0 resolved to) */
    int32_t bo, halo, ncw, nct;
    int32_t grid_x, grid_y, grid_z, block;
    int64_t lds;
    int32_t launches;
} vits_flow_coupling_plan;
VITS_API int vits_op_flow_coupling_plan(const vits_flow_coupling_desc* d, vits_flow_coupling_plan* plan);

/* conv_transpose_1d_with_bias (vits.cpp:178-193). w is [Cin][Cout][K] (torch layout), K == 2*stride.
 * crop = (K-stride)/2 in HF mode (HF modeling_vits.py:483-490), 0 in reference mode (vits.cpp:187, Q1).
 * Output length = stride*T + K - stride - 2*crop. pre-activation leaky_relu(slope) is fused (vits.cpp:613). */
typedef struct vits_convt1d_desc {
    int32_t batch, cin, cout, t, t_stride, t_out_stride;
    int32_t k, stride, crop;
    float pre_slope; /* leaky_relu slope applied to x first; 1.0 = none */
} vits_convt1d_desc;
VITS_API int vits_op_conv_transpose1d(const vits_convt1d_desc* d, const float* x, const float* w, const float* bias,
                                      const int32_t* lens, float* y);

/* One HiFiGAN upsampler (vits.cpp:178-193, 613-618; kernel = 2 x stride) of the 16-bit modes in the GROUP layout, through the kernel the caller names — what
 * engine_vocoder.cpp launches per stage and vits_op_conv_transpose1d does not reach (its 16-bit form has standard-layout fp32 outputs: another epilogue). Per
 * utterance, with L = lens[b], s = stride, x' = round16(leaky_relu(x, pre_slope)), w' = round16(w), x'[-1] = x'[L] = 0:
 *   n in [0, s L + s - 2 crop):  q = (n + crop) / s,  ph = (n + crop) % s,
 *   y[co][n] = bias[co] + sum_ci x'[ci][q] w'[ci][co][ph] + x'[ci][q - 1] w'[ci][co][ph + s]   (fp32 accumulation on the matrix cores),
 *   y16[co][n] = round16(leaky_relu(y[co][n], y16_slope))                                       (the conv input of the stage's ResBlocks).
 * x: host [batch][cin][t_stride] fp32; w: [cin][cout][2 stride] (torch layout); bias [cout] or NULL; lens optional, 0 <= lens[b] <= t. y: host
 * [batch][cout][t_out_stride] fp32; y16 (optional): the 16-bit copy as raw bit patterns, same shape; x16 (optional): the converter's output, raw bit patterns
 * [batch][cin][t_stride]. Columns [0, t_out) of every row of y / y16 with t_out = stride t + stride - 2 crop, and [0, t) of x16, are written back as the device
 * holds them. With y16 == NULL the kernels get no 16-bit destination (the engine's form for stages of whole-ResBlock kernels).
 * Arithmetic: vits_op_set_arith, VITS_ARITH_F16 or VITS_ARITH_BF16 only (the fp32 upsampler is vits_op_conv_transpose1d).
 * variant: 0 the engine's choice as engine_vocoder.cpp writes it: the streaming kernel where convt16_stream_supported, else the GEMM tile; 1 the GEMM tile:
 * launch_conv16 with the group outputs (conv16_kernel<2, -1, ..., E16_CONVT_GROUP>); 2 launch_convt16_stream (convt16_kernel / convt16_lines_kernel), or -1 with
 * the failing condition named for a shape plan_convt16 does not take (c_in a multiple of 64 and <= 512, c_out a multiple of 32, stride x c_out <= 128 or stride
 * a multiple of 4). split: 0 the planner's gridDim.z; 1, 2 or 4 force that many blocks per position tile, lines kernels only — on any other kernel, and for
 * any other value, a refusal. Variants 1 and 2 never fall back. Neither the variant nor the split depends on an environment knob: the launch policy runs on the
 * knobs' defaults. Every refusal is made before the first device call.
 * Staging is the engine's: the 16-bit input buffer [b][cin/8][ts][8] (ts = t rounded up to 32) holds 0xFF bytes (NaN in both types) before the engine's converter
 * (launch_to_group16 with pre_slope) writes t < lens[b], so a read past an utterance shows in the result; the outputs (fp32 [b][cout/8][g_ts][8], g_ts = t_out
 * rounded up to 32, and the 16-bit copy) are zero-filled, so a store past len_out[b] = stride lens[b] + stride - 2 crop shows; an utterance with lens[b] = 0
 * gets no store at all. All variants and splits give the same bits. */
typedef struct vits_upsample16_desc {
    int32_t batch, cin, cout, t, t_stride, t_out_stride;
    int32_t stride, crop;
    float pre_slope, y16_slope; /* 1.0 = none */
    int32_t variant, split;
} vits_upsample16_desc;
VITS_API int vits_op_upsample16(const vits_upsample16_desc* d, const float* x, const float* w, const float* bias, const int32_t* lens, float* y, uint16_t* y16,
                                uint16_t* x16);
/* What vits_op_upsample16 would launch for d in the arithmetic of vits_op_set_arith, or -1 and the cause of its refusal. Host arithmetic only: no device call.
 * kernel: the instantiation as rocprofv3 prints it (convt16_kernel<NR, CSPLIT, RS, BF>, convt16_lines_kernel<BN, BF>, conv16_kernel<2, -1, WM, WN, MR, NR, 4, BF>);
 * tag: convt16_stream_tag's (what the streaming kernel of this shape would be, also where the GEMM tile runs); bn: input positions per block. */
typedef struct vits_upsample16_plan {
    char kernel[96];
    char tag[16];
    int32_t variant; /* the variant that runs (1 or 2; what 0 resolved to) */
    int32_t bn;
    int32_t grid_x, grid_y, grid_z, block;
    int64_t lds;
} vits_upsample16_plan;
VITS_API int vits_op_upsample16_plan(const vits_upsample16_desc* d, vits_upsample16_plan* plan);

/* Relative-position multi-head self-attention core (vits.cpp:296-356):
 * q,k,v [B][H*hd][T] (q already scaled), rel_k/rel_v [2w+1][hd] shared by heads; out [B][H*hd][T]. */
VITS_API int vits_op_rel_attention(int32_t batch, int32_t heads, int32_t head_dim, int32_t t, int32_t t_stride,
                                   int32_t window, const float* q, const float* k, const float* v,
                                   const float* rel_k, const float* rel_v, const int32_t* lens, float* out);

/* layer_norm over channels of (x + residual) (vits.cpp:115-120,365-372). */
VITS_API int vits_op_add_layer_norm(int32_t batch, int32_t channels, int32_t t, int32_t t_stride, float eps,
                                    const float* x, const float* residual, const float* gamma, const float* beta,
                                    float* y);

/* The same attention core through the kernel the caller names, with everything the text encoder's call passes: q is multiplied by q_scale on load, and exp_tab
 * (optional, NULL = expf) is ggml's 65536-entry fp16 exponential table, indexed by the fp16 bits of the argument, as vits_model_set_ggml_tables builds it; with
 * it the soft-max sums in double. q, k, v, out: host [batch][heads * head_dim][t_stride] fp32; rel_k, rel_v [2 window + 1][head_dim]; lens optional,
 * 0 <= lens[b] <= t <= t_stride. The device rows have the pitch t_stride as given: a pitch that is no multiple of 4 takes the matrix-core kernel's scalar V loads.
 * variant: 0 the planner's choice; 1 rel_attention_kernel<1024>; 2 rel_attention_kernel<256>; 3 rel_attention_mfma_kernel<4, 32, false, false>; 4 <8, 32, false,
 * false>; 5 <4, 24, true, false> (the short-sequence variant); 6 <8, 24, false, true> (the latency variant). Every kernel's loops run over the utterance's own
 * length and every block works for itself, so variants 5 and 6 are launchable at any length and grid. Variants 1-6 never fall back: a shape no instantiation can run
 * (head_dim above 128; variants 3-6: head_dim no multiple of 16; variants 5 and 6: head_dim above 96; the block's LDS beyond the limit) returns -1 with the cause in
 * vits_last_error. Neither the variant nor anything else depends on an environment knob: the launch policy runs on the knobs' defaults. Every refusal is made before
 * the first device call.
 * Staging: q, k and v hold 0xFF bytes (NaN) behind lens[b] before the valid part goes in, so a read past an utterance shows in the result; out is staged as 0xFF
 * bytes and comes back, all of [batch][heads * head_dim][t_stride], as the device holds it. Variants 3-6 give the same bits as each other, 1 and 2 as each other. */
typedef struct vits_attention_desc {
    int32_t batch, heads, head_dim, t, t_stride, window;
    float q_scale;
    int32_t variant;
} vits_attention_desc;
VITS_API int vits_op_attention(const vits_attention_desc* d, const float* q, const float* k, const float* v, const float* rel_k, const float* rel_v,
                               const uint16_t* exp_tab, const int32_t* lens, float* out);
/* What vits_op_attention would launch for d, or -1 and the cause of its refusal. Host arithmetic only: no device call. kernel: the instantiation as the launch-plan
 * tables print it; nw, maxs: waves per block and k-steps of the register arrays (matrix-core kernel; 0 otherwise); vshift: log2 of the V chunk (VALU kernel). */
typedef struct vits_attention_plan {
    char kernel[96];
    int32_t variant; /* the variant that runs (1-6; what 0 resolved to) */
    int32_t nw, maxs, vshift;
    int32_t grid_x, grid_y, grid_z, block;
    int64_t lds;
} vits_attention_plan;
VITS_API int vits_op_attention_plan(const vits_attention_desc* d, vits_attention_plan* plan);

/* add_layer_norm_kernel with every argument its callers pass: v = LayerNorm_channels(x + residual) * gamma + beta, post_gelu: v = GELU(v) (erf, or gelu_tab:
 * ggml's 65536-entry fp16 table as vits_model_set_ggml_tables builds it); add_to 0: y = v; add_to 1: y += v (y is read and written, as the DDS layers' residual).
 * x, residual (optional), y: host [batch][channels][t_stride] fp32, device rows of the same pitch; lens optional, 0 <= lens[b] <= t <= t_stride. tw: time steps
 * per block, 32 or 64, 0 = the planner's (on the knobs' defaults: no environment knob reaches the choice); both give the same bits. Refused (-1, the cause in
 * vits_last_error, before the first device call): any other tw, a tile beyond the LDS limit, gelu_tab without post_gelu.
 * Staging: x, residual and (add_to) y hold 0xFF bytes behind lens[b]; without add_to y is staged as 0xFF bytes. y comes back, all of it, as the device holds it. */
typedef struct vits_layer_norm_desc {
    int32_t batch, channels, t, t_stride;
    float eps;
    int32_t tw, post_gelu, add_to;
} vits_layer_norm_desc;
VITS_API int vits_op_layer_norm(const vits_layer_norm_desc* d, const float* x, const float* residual, const float* gamma, const float* beta, const uint16_t* gelu_tab,
                                const int32_t* lens, float* y);
typedef struct vits_layer_norm_plan {
    char kernel[96]; /* add_layer_norm_kernel<32 | 64> */
    int32_t tw, grid_x, grid_y, block;
    int64_t lds;
} vits_layer_norm_plan;
VITS_API int vits_op_layer_norm_plan(const vits_layer_norm_desc* d, vits_layer_norm_plan* plan);

/* A conv of a LayerNorm, as the text encoder runs its QKV, FFN and projection convs (Engine::run_text_encoder), fp32:
 *   ln_out = LayerNorm_channels(x) * gamma + beta;  y = post(conv_k(ln_out) + bias) [+ residual],  post_act 0: none, 1: relu; zero padding, pad_left on the left.
 * x, ln_out: host [batch][cin][t_stride]; y, residual (optional): [batch][cout][t_stride]; w [cout][cin][k] (torch layout); lens optional, 0 <= lens[b] <= t <=
 * t_stride. pitch: the device rows' pitch, 0 = the engine's (t rounded up to 32); any other value >= t is taken as given, so that a pitch that is no multiple
 * of 4 reaches the kernels' element-wise fill.
 * variant: 1 launch_add_layer_norm, then launch_conv on the normalised tensor (the engine's fallback); 2 one launch_conv that normalises on load (ConvCall::ln_gamma,
 * conv_lat16_kernel), or -1 with the failing condition of plan_conv's ln_ok named; 0 what the engine does: 2 where that is admissible, else 1. Variants 1 and 2 never
 * fall back; the launch policy runs on the knobs' defaults; every refusal is made before the first device call. Both variants give the same bits in y and in ln_out.
 * Staging: x and residual hold 0xFF bytes behind lens[b]; y and ln_out are staged as 0xFF bytes, and columns [0, t) of their rows come back as the device holds them. */
typedef struct vits_norm_conv_desc {
    int32_t batch, cin, cout, t, t_stride, pitch;
    int32_t k, pad_left, post_act;
    float eps;
    int32_t variant;
} vits_norm_conv_desc;
VITS_API int vits_op_norm_conv(const vits_norm_conv_desc* d, const float* x, const float* gamma, const float* beta, const float* w, const float* bias,
                               const float* residual, const int32_t* lens, float* y, float* ln_out);
/* What vits_op_norm_conv would launch, or -1 and the cause. Host arithmetic only. tile: the conv's tile as conv_plan.h names it (TILE_LAT16, TILE_NARROW, ...);
 * ln_ok: LayerNorm on load is admissible for this conv (ln_why: the condition that fails, or ""); launches: 1 or 2. */
typedef struct vits_norm_conv_plan {
    char tile[16];
    char ln_why[96];
    int32_t variant; /* the variant that runs (1 or 2; what 0 resolved to) */
    int32_t pitch, ln_ok, launches;
    int32_t grid_x, grid_y, grid_z, block;
    int64_t lds;
} vits_norm_conv_plan;
VITS_API int vits_op_norm_conv_plan(const vits_norm_conv_desc* d, vits_norm_conv_plan* plan);

/* The deterministic duration predictor (see vits_model_duration_predictor_kind) on caller-supplied tensors, fp32:
 *   logw = proj(LN2(relu(conv_2(LN1(relu(conv_1(x + spk_row))))))), x + spk_row inside [0, lens[b]) and 0 outside, LN outputs 0 outside.
 * x host [batch][hidden][t_stride]; w1 [filter][hidden][k], w2 [filter][filter][k], wp [1][filter][1] (torch layout); b1, b2 [filter], bp [1];
 * g1, be1, g2, be2 [filter] (LayerNorm weight and bias); spk_rows host [batch][hidden] (utterance b's speaker term) or NULL (none); lens may be
 * NULL; logw out, host [batch][t_stride], entries t < lens[b] written. variant: 0 = the planner's choice, 1 = the fused kernel's 16-token tile,
 * 2 = its wide tile, 3 = the un-fused sequence (row add, conv, LayerNorm, conv, LayerNorm, 1x1 conv). Variants 1 and 2 return -1 with a message
 * for a (hidden, filter, k) without an instantiation: they never fall back. All variants give the same bits. The staging buffer of x is filled
 * with NaNs behind each lens[b] before the valid part is uploaded, so a read past an utterance shows in the result. */
typedef struct vits_duration_predictor_desc {
    int32_t batch, hidden, filter, t, t_stride, k;
    float eps;
    int32_t variant;
} vits_duration_predictor_desc;
VITS_API int vits_op_duration_predictor(const vits_duration_predictor_desc* d, const float* x, const float* w1, const float* b1, const float* g1,
                                        const float* be1, const float* w2, const float* b2, const float* g2, const float* be2, const float* wp,
                                        const float* bp, const float* spk_rows, const int32_t* lens, float* logw);

/* One DDS block of the stochastic duration predictor (`layers` layers of depthwise conv, LayerNorm, GELU, 1x1 conv, LayerNorm, GELU, residual; layer i
 * has dilation k^i and zero padding (k - 1) k^i / 2, as Engine::run_dds builds them) on caller-supplied tensors, in the arithmetic of vits_op_set_arith
 * (fp32, f16, bf16; the split arithmetic is refused), optionally with the per-token op in front of it and the 1x1 conv behind it:
 *   head 0: the block's input is x [batch][channels][t_stride];
 *   head 1: the conv flow's 1 -> H conv of latent row zc plus conditioning: input = head_w[c] * z[zc][t] + head_b[c] + cond[c][t]; z [batch][2][t_stride],
 *           cond [batch][channels][t_stride], head_w [channels], head_b [channels]; x is not read;
 *   head 2: an H -> H 1x1 conv of x: head_w [channels][channels], head_b [n_bias_rows][channels] (the effective-bias table of a multi-speaker model);
 *           bias_rows [batch] (optional, NULL = row 0) names each utterance's row;
 *   tail 0: the block's output goes to y [batch][channels][t_stride];
 *   tail 1: y2 = tail_w . output + tail_b, tail_w [tail_rows][channels], tail_b [tail_rows], y2 [batch][tail_rows][t_stride].
 * Per-layer parameters, layer-major: dw_w [layers][channels][k], dw_b, g1, b1 [layers][channels], pw_w [layers][channels][channels], pw_b, g2, b2
 * [layers][channels]. lens optional, 0 <= lens[b] <= t <= t_stride.
 * variant: 0 the engine's choice for this arithmetic and grid; 1 three launches per layer (dds_depthwise_kernel, the 1x1 conv, add_layer_norm_kernel with GELU
 * and residual); 2 dds_layer_kernel, one launch per layer; 3 dds_layer_lat_kernel, fp32 only, at most `channels` tail rows. Variants 1 and 2 run head and
 * tail as launches of their own (launch_pointwise_from1, the engine's conv); variant 3 fuses them into the first and the last layer as Engine::run_dds_lat does.
 * Variants 1-3 never fall back to another variant: a shape without an instantiation (channels no multiple of 32 or beyond 256, (k - 1) * dilation odd, a layer
 * whose tile passes the LDS limit, 16-bit arithmetic in variant 3) returns -1 with the cause in vits_last_error. Every refusal is made before the first device call.
 * Staging is the engine's: the ping-pong buffers of run_dds / run_dds_lat. Every staged input and every intermediate buffer holds NaNs (0xFF bytes)
 * behind lens[b] before the valid part goes in: a read past an utterance shows in the result. y and y2 (either may be NULL) come back as the device holds
 * them, columns [0, t_stride): the staged NaN wherever no kernel wrote. With a tail, variant 3 has no y to write: it comes back all NaN; variants 1 and 2
 * hold the block's output there. All variants give the same bits. */
typedef struct vits_dds_block_desc {
    int32_t batch, channels, t, t_stride;
    int32_t k, layers;
    float eps;
    int32_t variant, head, tail, tail_rows, zc, n_bias_rows;
} vits_dds_block_desc;
VITS_API int vits_op_dds_block(const vits_dds_block_desc* d, const float* x, const float* z, const float* cond, const float* head_w, const float* head_b,
                               const int32_t* bias_rows, const float* dw_w, const float* dw_b, const float* g1, const float* b1, const float* pw_w,
                               const float* pw_b, const float* g2, const float* b2, const float* tail_w, const float* tail_b, const int32_t* lens, float* y,
                               float* y2);
/* What vits_op_dds_block would launch for d in the arithmetic of vits_op_set_arith, or -1 and the cause of its refusal. Host arithmetic only: no device call.
 * kernel / kernel_last: the first and the last layer's instantiation as the launch-plan tables print it (variant 3: the head is part of the first name, the
 * tail of the last; layers between them are <0, 0, M>; variant 1: dds_depthwise_kernel); nt: tokens per block (64 / 32 / 16); halo[i], lds[i]: layer i's halo
 * columns per side and LDS bytes (at most 8 layers); launches: kernel launches for the block with head and tail (the converter launches of 16-bit convs not counted). */
typedef struct vits_dds_block_plan {
    char kernel[96], kernel_last[96];
    int32_t variant; /* the variant that runs (1-3; what 0 resolved to) */
    int32_t nt, layers;
    int32_t halo[8];
    int64_t lds[8];
    int32_t grid_x, grid_y, block;
    int32_t launches;
} vits_dds_block_plan;
VITS_API int vits_op_dds_block_plan(const vits_dds_block_desc* d, vits_dds_block_plan* plan);

/* The inverse rational-quadratic spline of a conv flow (launch_spline) on caller-supplied tensors: u host [batch][3 bins - 1][t_stride] (widths, heights,
 * inner derivatives), z host [batch][2][t_stride], in and out: row zc is transformed on [0, lens[b]), everything else keeps its bits. mode: VITS_MODE_HF
 * (identity outside [-tail, tail], bounds inclusive) or VITS_MODE_REFERENCE (the reference's width scaling, last-token row and masked get / set pair).
 * u is staged with NaNs behind lens[b]. bins 1..16 and t <= 4096, or -1 with the cause, before the first device call. lens optional. */
VITS_API int vits_op_spline(int32_t batch, int32_t t, int32_t t_stride, int32_t bins, float tail, float inv_sqrt, int32_t mode, int32_t zc, const float* u,
                            float* z, const int32_t* lens);

/* The durations kernel (launch_durations, the device library's expf) on caller-supplied log-durations: logw host [batch][rows][t_stride], row `row` is read
 * on [0, lens[b]); dur = ceil(exp(logw) * scale), scale = length_scales[b] (optional) or length_scale; ovr [batch][t_stride] (optional): entries >= 0 replace
 * the token's duration; fixed > 0 replaces every duration. Outputs: dur (float, integer-valued) and cum (inclusive sums) [batch][t_stride], 0 and INT32_MAX
 * behind lens[b]; frames [batch] = max(1, sum); stage_lens [n_stage][batch] = frames * stage_mul[s] + stage_add[s]. The outputs are staged as 0xFF bytes. */
VITS_API int vits_op_durations(int32_t batch, int32_t rows, int32_t row, int32_t t_stride, const float* logw, const int32_t* lens, float length_scale,
                               const float* length_scales, const int32_t* ovr, int32_t fixed, int32_t n_stage, const int32_t* stage_mul,
                               const int32_t* stage_add, float* dur, int32_t* cum, int32_t* frames, int32_t* stage_lens);

/* The fit kernel ("a stated duration"; launch_fit_durations) on caller-supplied log-durations: logw host [batch][rows][t_stride], row `row` is read on
 * [0, lens[b]) and staged with NaN behind it; fixed [batch][t_stride] (optional) the override rows, groups [batch] (optional: utterance b is group b),
 * target_frames [batch] by group (0: not fitted). Outputs: e_out [batch][t_stride] = expf(logw) on [0, lens[b]) (the output fill behind it), dur_out
 * [batch][t_stride] and group_rows_out double [batch][5] as vits_fit_host writes them. Refused like vits_fit_host, before the first device call. */
VITS_API int vits_op_fit_durations(int32_t batch, int32_t rows, int32_t row, int32_t t_stride, const float* logw, const int32_t* lens, const int32_t* fixed,
                                   const int32_t* groups, const int64_t* target_frames, float min_rate, float max_rate, float* e_out, int32_t* dur_out,
                                   double* group_rows_out);

/* The kernels between the conv families at operator level. Host arrays in, host arrays out; inputs are staged with 0xFF bytes (NaN) behind every utterance's
 * length and between a row's extent and its device pitch, outputs hold the byte of vits_op_set_output_fill wherever no kernel writes. Each runs the engine's
 * own launcher; what the launcher or the engine refuses is refused here with the cause named, before the first device call.
 *
 * vits_op_spectrogram: the linear magnitude spectrogram of voice conversion and alignment (launch_spectrogram; spectrogram_torch with center = False: reflection
 * pad (n_fft - hop) / 2, periodic Hann, sqrt(re^2 + im^2 + 1e-6)). pcm host [batch][pcm_stride], n_samples host [batch]; utterance b has n_samples[b] / hop
 * frames (the engine's rule); out host [batch][bins][t_stride], bins <= n_fft / 2 + 1: frame t < frames[b] in column t, +0 up to the batch's longest frame
 * count, the fill behind that. Geometry as the engine checks it: n_fft a power of two in [16, 2048], 1 <= hop <= n_fft, n_fft - hop even, every
 * n_samples[b] >= max(hop, pad + 1). */
VITS_API int vits_op_spectrogram(int32_t n_fft, int32_t hop, int32_t bins, int32_t batch, const float* pcm, int64_t pcm_stride, const int32_t* n_samples,
                                 int32_t t_stride, float* out);
/* vits_op_prior_sample: prior sampling through the alignment as a gather (launch_zp): zp[b][c][j] = mean[b][c][a] + eps * exp(logvar[b][c][a]) * scale for
 * j < frames[b], a = the first token with cum[b][a] > j (none: mean 0, logvar 0). mean, logvar host [batch][channels][t_tok]; cum host [batch][t_tok]
 * (inclusive duration sums, uploaded as given: INT32_MAX behind tok_lens[b] as the durations kernel leaves it); tok_lens host [batch] or NULL (t_tok);
 * frames host [batch], 0 <= frames[b] <= t_stride; zp host [batch][channels][t_stride]. eps: noise host [batch][channels][t_stride], or NULL = the counter
 * stream vits_counter_normal(seed + (seed_offsets ? seed_offsets[b] : b), VITS_STREAM_NOISE_PRIOR, c * frames[b] + j). scale = noise_scales[b] (optional) or
 * noise_scale. */
VITS_API int vits_op_prior_sample(int32_t batch, int32_t channels, int32_t t_tok, int32_t t_stride, const float* mean, const float* logvar, const int32_t* cum,
                                  const int32_t* tok_lens, const int32_t* frames, const float* noise, uint64_t seed, const int32_t* seed_offsets, float noise_scale,
                                  const float* noise_scales, float* zp);
/* vits_op_posterior_sample: zq[b][row][j] = mean[b][c][j] + (eps * eps_scale) * exp(logstd[b][c][j]) for j < frames[b] (launch_posterior_sample), row = c, or
 * channels - 1 - c with flip = 1; every tensor host [batch][channels][t_stride]; eps as in vits_op_prior_sample. eps_scale = 0 is the mean: no noise is drawn or read. */
VITS_API int vits_op_posterior_sample(int32_t batch, int32_t channels, int32_t t_stride, const float* mean, const float* logstd, const int32_t* frames,
                                      const float* noise, uint64_t seed, const int32_t* seed_offsets, int32_t flip, float eps_scale, float* zq);
/* vits_op_conv_post: leaky_relu(slope) -> Conv1d(cin -> 1, k, no bias) -> tanh, the vocoder's last kernel. x host [batch][cin][t], on the device at x_pitch
 * floats per row; w host [cin][k]; lens host [batch] or NULL; wave host [batch][t]; pre host [batch][t] or NULL: the sums before the tanh, on the device at
 * pre_pitch floats per row. Samples [emit_lo, min(emit_hi[b], lens[b])) of each row are written (emit_hi NULL: up to lens[b]), the streaming vocoder's window.
 * VITS_ARITH_F32 runs launch_conv_post. In a 16-bit arithmetic (vits_op_set_arith) layout chooses: VITS_CONV_POST_FP32_LAYOUT = the same kernel with the operands
 * rounded on load; VITS_CONV_POST_STREAM = launch_to_group16 with the slope, then launch_conv_post16, as the 16-bit vocoder runs them (cin a multiple of 8). */
#define VITS_CONV_POST_FP32_LAYOUT 0
#define VITS_CONV_POST_STREAM 1
typedef struct vits_conv_post_desc {
    int32_t batch, cin, k, t;
    int32_t x_pitch, pre_pitch;
    float slope;
    int32_t emit_lo;
    int32_t layout;
} vits_conv_post_desc;
VITS_API int vits_op_conv_post(const vits_conv_post_desc* d, const float* x, const float* w, const int32_t* lens, const int32_t* emit_hi, float* pre, float* wave);
/* vits_op_resblock_sum: out = ((y0 + y1) [+ y2]) * scale (scale_div = 1: / scale) [then leaky_relu(slope) where act = 1] on [0, lens[b]) (launch_rb_sum3_std, the
 * fp32 vocoder's sum over a stage's side-by-side resblocks). y0, y1, y2 (optional), out host [batch][channels][t]; on the device the addends lie at in_pitch
 * and out at out_pitch floats per row. VITS_ARITH_F32 only. */
VITS_API int vits_op_resblock_sum(int32_t batch, int32_t channels, int32_t t, int32_t in_pitch, int32_t out_pitch, float scale, int32_t scale_div, int32_t act,
                                  float slope, const float* y0, const float* y1, const float* y2, const int32_t* lens, float* out);

/* The alignment kernels (align_logp + align_mas; see vits_model_align_batch) on caller-supplied statistics: m, ls host [batch][F][Tmax] (prior mean and
 * log-deviation per token), z host [batch][F][Lmax], Tmax = max T[b], Lmax = max L[b], 1 <= T[b] <= L[b]. durations: out, host [batch][Tmax] (0 past
 * T[b]); scores: out, host [batch], optional. */
VITS_API int vits_op_align(int32_t batch, const int32_t* T, const int32_t* L, int32_t F, const float* m, const float* ls, const float* z,
                           int32_t* durations, float* scores);

/* The resampling kernel (see vits_model_set_rates for the filter) on a ragged batch: x host [batch][x_stride] at in_rate, lens host
 * [batch] (samples of each row, 0 <= lens[b] <= x_stride; NULL: every row has x_stride), y host [batch][y_stride] at out_rate. Row b gets
 * its ceil(lens[b] L / M) output samples; everything behind them in y is left as it was, and nothing behind lens[b] in x is read. Equal
 * rates copy. Refused (-1 + message): a pair vits_resample_plan refuses, a length outside its row, a y_stride shorter than the longest
 * output row. */
VITS_API int vits_op_resample(int32_t in_rate, int32_t out_rate, int32_t batch, const float* x, int64_t x_stride, const int64_t* lens,
                              float* y, int64_t y_stride);

/* The varispeed kernel (see "a stated pitch" for the definition) on a ragged batch with a ratio per row: x host [batch][x_stride], lens host
 * [batch] (0 <= lens[b] <= x_stride; NULL: every row has x_stride), ratios host [batch], y host [batch][y_stride], n_out host [batch] = N' of
 * every row. The device copy of x keeps the caller's stride and the caller's alignment within 16 bytes and holds 0xFF bytes behind every
 * lens[b], so a read past a row shows; the device copy of y holds the vits_op_set_output_fill byte before the kernel runs and comes back whole,
 * so a write behind N' shows. Refused (-1 + message): what vits_pitch_plan refuses (naming the row), a length outside its row, a y_stride
 * shorter than the longest output row. */
VITS_API int vits_op_pitch(int32_t batch, const float* x, int64_t x_stride, const int64_t* lens, const float* ratios, float* y, int64_t y_stride,
                           int64_t* n_out);

/* The time-stretch kernels (see "a stated tempo" for the definition) on a ragged batch at `rate` with a tempo per row: x host [batch][x_stride],
 * lens host [batch] (0 <= lens[b] <= x_stride; NULL: every row has x_stride), tempos host [batch], y host [batch][y_stride], n_out host [batch] =
 * N' of every row, offsets host int32 [batch][offsets_stride] or NULL = d*_1 .. d*_F of every row. The device copies of x and y keep the caller's
 * strides and the caller's alignment within 16 bytes; x holds 0xFF bytes behind every lens[b], so a read past a row shows; y and offsets hold
 * the vits_op_set_output_fill byte before the kernels run and come back whole, so a write behind N' or behind F shows. Refused (-1 + message): what
 * vits_tempo_plan refuses (naming the row), a length outside its row, a y_stride shorter than the longest output row, an offsets_stride below
 * the largest F. */
VITS_API int vits_op_tempo(int32_t rate, int32_t batch, const float* x, int64_t x_stride, const int64_t* lens, const float* tempos, float* y,
                           int64_t y_stride, int64_t* n_out, int32_t* offsets, int64_t offsets_stride);

/* The levelling kernels (see vits_model_set_level for the definition) on a ragged batch, staged exactly as the engine stages it: x host
 * [batch][x_stride] at `rate`, lens host [batch] (0 <= lens[b] <= x_stride; NULL: every row has x_stride). The device copy of x holds NaNs
 * behind every lens[b], so a read past an utterance shows. levels: out, host [batch][4] = {L, P, g, blocks}. y: host [batch][y_stride] or
 * NULL (measure only); row b gets its lens[b] samples x * g, everything behind them is left as it was. kind: VITS_LEVEL_MEASURE .. _LOUDNESS,
 * values as vits_model_set_level checks them. Refused (-1 + message): what vits_model_set_level refuses, VITS_LEVEL_NONE, a rate outside
 * [4000, 192000], a length outside its row, a y_stride shorter than the longest row. */
typedef struct vits_level_desc {
    int32_t rate;
    int32_t batch;
    int64_t x_stride;
    int64_t y_stride;
    int32_t kind;
    float value_db;
    float ceiling_db;
} vits_level_desc;
VITS_API int vits_op_level(const vits_level_desc* d, const float* x, const int64_t* lens, float* y, float* levels);

/* The levelling tail with the limiter (see vits_model_set_limiter for the definition) on a ragged batch, staged exactly as the engine stages it
 * (the device copy of x holds NaNs behind every lens[b]): measure, true-peak meter, g0, limiter (VITS_LEVEL_GAIN, _LOUDNESS) or the plain
 * multiply (VITS_LEVEL_PEAK), meter of y. y: host [batch][y_stride], required; row b gets its lens[b] samples, everything behind them is left
 * as it was. levels: out, host [batch][4] with g = g0. limits: out, host [batch][4] = {TP(x), TP(y), min s, share}. Refused (-1 + message):
 * what vits_op_level refuses, a rate above 48000, VITS_LEVEL_NONE and _MEASURE, an unknown mode or VITS_LIMIT_OFF, a ceiling_db outside
 * [-60, 0] (VITS_LEVEL_GAIN too), a NULL y. */
typedef struct vits_limit_desc {
    vits_level_desc level;
    int32_t mode; /* VITS_LIMIT_TRUE_PEAK */
} vits_limit_desc;
VITS_API int vits_op_limit(const vits_limit_desc* d, const float* x, const int64_t* lens, float* y, float* levels, float* limits);

/* The edges stage (see vits_model_set_edges for the definition) on a ragged batch that is ON THE DEVICE already: every pointer is a device
 * pointer. x [batch][x_stride] at `rate`; lens [batch] int32, 0 <= lens[b] <= x_stride: nothing behind a row's samples is read; y
 * [batch][y_stride], not x: row b gets its lens[b] + Pl + Pt samples (the delivered row, then zeros up to that bound), everything behind them
 * is left as it was; lens_out [batch]: N' of every row; rows [batch][4] = {a, b, N', n_active}. Runs on the default stream and returns after
 * hipDeviceSynchronize, as vits_op_level does. Refused (-1 + message): what vits_edges_plan refuses, mode VITS_EDGES_OFF, a NULL pointer, an
 * empty batch, a lens[b] outside [0, x_stride] or above 2^30, a y_stride below the largest bound. */
VITS_API int vits_op_edges(int32_t rate, const vits_edges_desc* desc, int32_t batch, const float* x, int64_t x_stride, const int32_t* lens, float* y,
                           int64_t y_stride, int32_t* lens_out, int64_t* rows);

/* The join kernels (see "joined tracks" above for the definition) on a ragged batch: host arrays in, host arrays out, staged as
 * vits_op_level stages its rows. x [batch][x_stride] at `rate` goes up as it is; lens [batch] int32, 0 <= lens[b] <= x_stride, are the
 * utterances' own bounds: nothing behind a row's samples is read; track and gap_ms as in vits_join_plan; y [G][y_stride] goes up too and comes
 * back: row g gets its bound_g samples (T_g of the track, then zeros), everything behind them is as it was; track_lens_out [G] int32 = T_g;
 * offsets_out [batch][2] int64 = {o_b, n_b}. Refused (-1 + message): what vits_join_plan refuses, a NULL x, lens, y, track_lens_out or
 * offsets_out, a lens[b] outside [0, x_stride], a y_stride below the largest bound. */
VITS_API int vits_op_join(int32_t rate, int32_t batch, const float* x, int64_t x_stride, const int32_t* lens, const int32_t* track, const float* gap_ms,
                          float* y, int64_t y_stride, int32_t* track_lens_out, int64_t* offsets_out);

/* ---- PCM16 / WAV sink (reference driver test/main.cpp:23-63: clamp to [-1,1], * 32767, truncate; 16 kHz mono) ------ */
VITS_API void vits_pcm16_from_float(const float* pcm, size_t n, int16_t* out);
/* The same conversion on the device, row by row: src [rows][src_stride] fp32 -> dst [rows][dst_stride] int16, the first
 * `cols` samples of each row (or lengths[r] of them when `lengths`, a DEVICE int64 array, is given). All pointers are
 * device pointers; runs on `hip_stream` (a hipStream_t, NULL = the default stream) without synchronising. Halves the
 * bytes of the multi-GPU PCM gather and of the host copy. Returns 0 on success. */
VITS_API int vits_pcm16_from_float_device(const float* src, int64_t src_stride, int16_t* dst, int64_t dst_stride,
                                          const int64_t* lengths, int32_t rows, int64_t cols, void* hip_stream);
/* Writes a canonical 44-byte-header RIFF/WAVE file exactly like test/main.cpp:36-60. Returns 0 on success. */
VITS_API int vits_write_wav16(const char* path, const float* pcm, size_t n, int32_t sample_rate);

/* ---- multi-GPU: the path's one exchange for C / C++ / Swift hosts -------------------------------------------------------
 * The reference synthesises one utterance per call (vits.cpp:184,303; callers test/main.cpp:68-78), so a batch shards by utterance:
 * ONE PROCESS PER GPU, each with its own model handle (vits_set_device(local_rank), weights replicated), rank r synthesising its own
 * rows — no data-path collective until the end, where every rank wants the whole batch's PCM. These three calls are that end: a
 * ragged all-gather over RCCL (xGMI inside a node) — the per-utterance lengths first (fixed size), then the rows padded to the longest
 * utterance of any rank. It is what vits.cpp_amd/multi_gpu.py does through torch.distributed, without Python. RCCL is loaded with
 * dlopen on first use (VITS_RCCL_LIB overrides the library name): single-GPU users need nothing, and world == 1 never touches it.
 *   rank 0:     char id[VITS_GATHER_ID_BYTES]; vits_pcm_gather_unique_id(id);  -> hand the 128 bytes to the other ranks (file, socket, MPI ...)
 *   every rank: g = vits_pcm_gather_init(id, sizeof id, rank, world, rows, row_capacity, 4);           (collective: all ranks call it)
 *   per batch:  vits_model_process_batch(..., opts.out_device = pcm, opts.skip_host_copy = 1, &r);
 *               vits_pcm_gather(g, pcm, stride, r.lengths, NULL, &all);                                 (collective)
 *               -> all.data: DEVICE [world * rows][all.stride], rank blocks in rank order; all.lengths: host [world * rows]
 *   end:        vits_pcm_gather_destroy(g);
 * rows is the same on every rank (pad a short shard with zero-length rows); row_capacity >= the longest utterance anywhere, in elements.
 * elem_bytes 4 = fp32 PCM, 2 = PCM16 (vits_pcm16_from_float_device first: half the bytes on the links). `hip_stream` = the stream the PCM was
 * produced on (the exchange is ordered behind it without a host wait), NULL when the producer has been synchronised — vits_model_process_batch
 * without opts.async has. The call returns when the gathered block is complete; it stays valid until the next call on the same object.
 * One call at a time per object. Return 0 / non-NULL on success, else -1 / NULL with vits_last_error().
 * Failure is COLLECTIVE as well: the first all-gather carries every rank's row_capacity and lengths, a rank whose own arguments are unusable
 * (NULL buffer, a negative length, a row longer than its pcm_stride or than row_capacity) sends -1 for the row instead of returning early, and
 * every rank derives the same verdict from the same table — all ranks return -1 with the offending (rank, row) in vits_last_error(), none is left
 * blocked in RCCL, and the object stays usable. pcm_stride need only reach the rank's OWN longest row. A HIP / RCCL error inside an exchange aborts
 * the communicator (ncclCommAbort) and the object refuses further calls: destroy it on every rank. Elements of a gathered row between its length
 * and `stride` are UNSPECIFIED (padding; rows are not zero-filled).
 * vits_pcm_gather_verdict is that decision as a pure host function of the gathered table (per rank: row_capacity, then `rows` lengths with -1 for an
 * unusable row): 0 and the common row width in *stride_out, or -1 with the message in vits_last_error(). */
#define VITS_GATHER_ID_BYTES 128
typedef struct vits_gather_ctx vits_gather_ctx;
typedef struct vits_gather_result {
    const void* data;       /* device [rows_total][stride] elements, owned by the gather object */
    int64_t stride;         /* elements between rows = the longest utterance of any rank */
    const int64_t* lengths; /* host [rows_total]: elements per utterance, rank blocks in rank order */
    int32_t rows_total;     /* world * rows */
} vits_gather_result;
VITS_API int vits_pcm_gather_unique_id(char* id_out /* [VITS_GATHER_ID_BYTES] */);
VITS_API vits_gather_ctx* vits_pcm_gather_init(const char* id, size_t id_bytes, int32_t rank, int32_t world, int32_t rows, int64_t row_capacity,
                                               int32_t elem_bytes);
VITS_API int vits_pcm_gather(vits_gather_ctx* g, const void* pcm_device, int64_t pcm_stride, const int64_t* lengths_host, void* hip_stream,
                             vits_gather_result* out);
VITS_API void vits_pcm_gather_destroy(vits_gather_ctx* g);
VITS_API int vits_pcm_gather_verdict(const int64_t* table, int32_t world, int32_t rows, int64_t* stride_out);

/* Select the HIP device used by subsequent loads on this thread (one process per GPU: pass LOCAL_RANK). */
VITS_API int vits_set_device(int32_t device);

/* Device facts (for the bench's roofline block). */
VITS_API int vits_device_info(char* name, size_t cap, int32_t* cu_count, int32_t* clock_mhz, int64_t* hbm_bytes);

#endif /* VITS_HIP_H */
