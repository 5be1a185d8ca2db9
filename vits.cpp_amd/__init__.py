"""Host-side Python mirror of the C ABI in ``include/vits.h`` (ctypes; no compute happens here).

The product is ``csrc/libvits_hip.so`` (hand-written HIP kernels for gfx950 + a C++ host orchestrator). This
module only loads it and marshals plain pointers, mirroring the reference's operator interface
(``vits_model_load_from_*`` / ``vits_model_process`` / ``vits_free_*``, /root/reference/src/include/vits.h:87-102)
plus the extensions declared in ``include/vits.h``. There is NO fallback: if the shared library (or a GPU,
for the compute entry points) is missing, calls fail loudly.

The directory is named ``vits.cpp_amd`` (with a dot), so it is imported by path; see ``load_package()`` in
``tests/conftest.py`` / ``bench.py``:  ``importlib.util.spec_from_file_location("vits_cpp_amd", ".../__init__.py")``.
"""
import ctypes as C
import json
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VITS_HIP_LIB", os.path.join(_HERE, "csrc", "libvits_hip.so"))

MODE_DEFAULT, MODE_REFERENCE, MODE_HF = -1, 0, 1
NOISE_REFERENCE, NOISE_COUNTER, NOISE_EXPLICIT = 0, 1, 2
SYNTH_FULL, SYNTH_TINY, SYNTH_BF16, SYNTH_SPEAKERS, SYNTH_POSTERIOR = 0, 1, 0x100, 0x200, 0x400
SYNTH_DETERMINISTIC = 0x800  # OR-ed in: the deterministic duration predictor in the stochastic one's place
DP_STOCHASTIC, DP_DETERMINISTIC = 0, 1  # Model.duration_predictor_kind
DP_VARIANT_PLAN, DP_VARIANT_LAT, DP_VARIANT_WIDE, DP_VARIANT_UNFUSED = 0, 1, 2, 3  # op_duration_predictor
RB_VARIANT_PLAN, RB_VARIANT_UNFUSED, RB_VARIANT_PAIRS, RB_VARIANT_BLOCK, RB_VARIANT_SEGMENTS = 0, 1, 2, 3, 4  # op_resblock
FLOW_VARIANT_PLAN, FLOW_VARIANT_UNFUSED, FLOW_VARIANT_WAVENET, FLOW_VARIANT_COUPLING = 0, 1, 2, 3  # op_flow_coupling
UP16_VARIANT_PLAN, UP16_VARIANT_TILE, UP16_VARIANT_STREAM = 0, 1, 2  # op_upsample16
DDS_VARIANT_PLAN, DDS_VARIANT_UNFUSED, DDS_VARIANT_LAYER, DDS_VARIANT_LAT = 0, 1, 2, 3  # op_dds_block
DDS_HEAD_NONE, DDS_HEAD_FROM1, DDS_HEAD_CONV = 0, 1, 2
# op_attention: the planner's choice, rel_attention_kernel<1024 | 256>, rel_attention_mfma_kernel<4, 32, false, false | 8, 32, false, false | 4, 24, true, false | 8, 24, false, true>
ATT_VARIANT_PLAN, ATT_VARIANT_VALU1024, ATT_VARIANT_VALU256, ATT_VARIANT_MFMA4, ATT_VARIANT_MFMA8, ATT_VARIANT_SHORT, ATT_VARIANT_LAT = 0, 1, 2, 3, 4, 5, 6
NC_VARIANT_PLAN, NC_VARIANT_SEPARATE, NC_VARIANT_ON_LOAD = 0, 1, 2  # op_norm_conv
CONV_POST_FP32_LAYOUT, CONV_POST_STREAM = 0, 1  # op_conv_post in a 16-bit arithmetic: conv_post_kernel with rounded operands | the converter + conv_post16_kernel
ARITH_F32, ARITH_BF16, ARITH_F16, ARITH_F32_SPLIT = 0, 1, 2, 3
# vits_model_set_level: what every PCM a handle delivers is measured and multiplied by (include/vits.h)
LEVEL_NONE, LEVEL_MEASURE, LEVEL_GAIN, LEVEL_PEAK, LEVEL_LOUDNESS = 0, 1, 2, 3, 4
# vits_model_set_limiter: the levelling kinds that multiply deliver through the true-peak meter and the look-ahead limiter
LIMIT_OFF, LIMIT_TRUE_PEAK = 0, 1
# vits_model_set_edges: where the delivered audio begins and ends (trimmed near-silence, fades, pauses of digital silence)
EDGES_OFF, EDGES_PAD, EDGES_TRIM_RELATIVE, EDGES_TRIM_ABSOLUTE = 0, 1, 2, 3
SCOPE_FLOW_VOCODER, SCOPE_ALL_CONVS = 0, 1

#: every symbol include/vits.h declares (checked by tests/test_abi.py)
EXPORTED_SYMBOLS = [
    "vits_model_load_from_bytes", "vits_model_load_from_file", "vits_free_model", "vits_free_result",
    "vits_model_process", "vits_last_error", "vits_model_set_mode", "vits_model_get_mode",
    "vits_reference_noise_seed", "vits_model_process_ids", "vits_model_process_batch", "vits_free_batch_result",
    "vits_model_sync", "vits_model_tokenize", "vits_model_sampling_rate", "vits_model_vocab_size",
    "vits_model_weight_bytes", "vits_model_get_tap", "vits_synth_model_bytes", "vits_free_bytes",
    "vits_prof_enable", "vits_prof_reset", "vits_prof_report", "vits_op_conv1d", "vits_op_conv_transpose1d",
    "vits_op_rel_attention", "vits_op_add_layer_norm", "vits_device_info", "vits_set_device", "vits_model_file_reserialize",
    "vits_model_file_tokenize", "vits_pcm16_from_float", "vits_write_wav16", "vits_pcm16_from_float_device",
    "vits_model_set_arith", "vits_model_get_arith", "vits_model_file_validate", "vits_op_set_arith", "vits_op_tile_map_launches", "vits_op_set_output_fill", "vits_op_conv_group",
    "vits_model_set_arith_scope", "vits_model_get_arith_scope", "vits_model_submit_batch", "vits_model_wait", "vits_model_pending",
    "vits_model_set_ggml_tables", "vits_model_get_ggml_tables",
    "vits_model_set_speaker", "vits_model_get_speaker", "vits_model_num_speakers",
    "vits_model_speaker_embedding_size", "vits_model_get_speaker_embedding", "vits_model_add_voices", "vits_model_set_voice",
    "vits_model_clear_voices", "vits_model_num_voices",
    "vits_model_set_prosody", "vits_model_get_prosody",
    "vits_model_prepare_conversion", "vits_model_convert_batch", "vits_model_convert",
    "vits_model_align_batch", "vits_model_align", "vits_model_hop", "vits_op_align", "vits_op_resblock_pair",
    "vits_model_set_rates", "vits_model_get_rates", "vits_resample_plan", "vits_resample_taps", "vits_resample_length", "vits_op_resample",
    "vits_model_set_level", "vits_model_get_level", "vits_model_last_levels", "vits_loudness_plan", "vits_loudness_host", "vits_op_level",
    "vits_model_set_limiter", "vits_model_get_limiter", "vits_model_last_limits", "vits_limiter_plan", "vits_limiter_host", "vits_op_limit",
    "vits_model_set_edges", "vits_model_get_edges", "vits_model_last_edges", "vits_edges_plan", "vits_edges_host", "vits_op_edges",
    "vits_pitch_ratio", "vits_pitch_plan", "vits_pitch_table", "vits_pitch_host", "vits_op_pitch",
    "vits_model_set_pitch", "vits_model_get_pitch", "vits_model_set_pitch_ratios", "vits_model_last_pitch",
    "vits_tempo_plan", "vits_tempo_host", "vits_op_tempo",
    "vits_model_set_conversion_prosody", "vits_model_get_conversion_prosody", "vits_model_set_conversion_ratios", "vits_model_last_tempo",
    "vits_fit_host", "vits_op_fit_durations", "vits_model_set_fit", "vits_model_set_fit_total", "vits_model_fit_frames", "vits_model_last_fit",
    "vits_join_plan", "vits_join_host", "vits_op_join", "vits_split_sentences", "vits_model_process_joined", "vits_model_last_joins", "vits_model_speak",
    "vits_model_duration_predictor_kind", "vits_op_duration_predictor", "vits_op_resblock", "vits_op_resblock_plan",
    "vits_op_flow_coupling", "vits_op_flow_coupling_plan", "vits_op_upsample16", "vits_op_upsample16_plan",
    "vits_op_dds_block", "vits_op_dds_block_plan", "vits_op_spline", "vits_op_durations",
    "vits_op_attention", "vits_op_attention_plan", "vits_op_layer_norm", "vits_op_layer_norm_plan", "vits_op_norm_conv", "vits_op_norm_conv_plan",
    "vits_op_spectrogram", "vits_op_prior_sample", "vits_op_posterior_sample", "vits_op_conv_post", "vits_op_resblock_sum",
    "vits_pcm_gather_unique_id", "vits_pcm_gather_init", "vits_pcm_gather", "vits_pcm_gather_destroy", "vits_pcm_gather_verdict",
]


class VitsResult(C.Structure):
    _fields_ = [("data", C.POINTER(C.c_float)), ("size", C.c_size_t)]


# int on_chunk(void* user, int32 utt, size_t offset, const float* pcm, size_t n)  (include/vits.h vits_chunk_callback)
ChunkCallback = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_size_t, C.POINTER(C.c_float), C.c_size_t)


class LevelDesc(C.Structure):
    """vits_level_desc"""
    _fields_ = [("rate", C.c_int32), ("batch", C.c_int32), ("x_stride", C.c_int64), ("y_stride", C.c_int64), ("kind", C.c_int32),
                ("value_db", C.c_float), ("ceiling_db", C.c_float)]


class LimitDesc(C.Structure):
    """vits_limit_desc"""
    _fields_ = [("level", LevelDesc), ("mode", C.c_int32)]


class EdgesDesc(C.Structure):
    """vits_edges_desc"""
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32), ("threshold_db", C.c_float), ("keep_head_ms", C.c_float), ("keep_tail_ms", C.c_float),
                ("fade_in_ms", C.c_float), ("fade_out_ms", C.c_float), ("lead_ms", C.c_float), ("tail_ms", C.c_float)]


def edges_desc(mode=EDGES_OFF, threshold_db=0.0, keep_head_ms=0.0, keep_tail_ms=0.0, fade_in_ms=0.0, fade_out_ms=0.0, lead_ms=0.0, tail_ms=0.0):
    """a filled vits_edges_desc"""
    return EdgesDesc(C.sizeof(EdgesDesc), int(mode), float(threshold_db), float(keep_head_ms), float(keep_tail_ms), float(fade_in_ms), float(fade_out_ms),
                     float(lead_ms), float(tail_ms))


class ProcessOpts(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("mode", C.c_int32), ("noise_kind", C.c_int32), ("noise_seed", C.c_uint64),
        ("noise_dur", C.c_void_p), ("noise_prior", C.c_void_p), ("noise_prior_stride", C.c_int64),
        ("fixed_duration", C.c_int32), ("collect_taps", C.c_int32), ("out_device", C.c_void_p),
        ("out_device_stride", C.c_int64), ("skip_host_copy", C.c_int32), ("async_", C.c_int32),
        ("vocoder_chunk_frames", C.c_int32), ("frames_only", C.c_int32), ("on_chunk", ChunkCallback), ("on_chunk_user", C.c_void_p),
        ("noise_seed_offsets", C.c_void_p), ("speaker_ids", C.c_void_p),
        ("speaking_rates", C.c_void_p), ("noise_scales", C.c_void_p), ("noise_scale_durations", C.c_void_p),
        ("duration_override", C.c_void_p), ("durations_out", C.c_void_p),
    ]


class BatchResult(C.Structure):
    _fields_ = [("data", C.POINTER(C.c_float)), ("stride", C.c_size_t), ("lengths", C.POINTER(C.c_int64)),
                ("frames", C.POINTER(C.c_int64)), ("batch", C.c_size_t)]


class SpeakOpts(C.Structure):
    """vits_speak_opts"""
    _fields_ = [("struct_size", C.c_uint32), ("sentence_gap_ms", C.c_float), ("paragraph_gap_ms", C.c_float), ("track_per_paragraph", C.c_int32),
                ("process", C.POINTER(ProcessOpts))]


class Conv1dDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32), ("t", C.c_int32), ("t_stride", C.c_int32),
                ("k", C.c_int32), ("dilation", C.c_int32), ("pad_left", C.c_int32), ("pre_act", C.c_int32),
                ("pre_slope", C.c_float), ("post_act", C.c_int32), ("out_scale", C.c_float)]


class ResblockPairDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("channels", C.c_int32), ("t", C.c_int32), ("t_stride", C.c_int32), ("k", C.c_int32),
                ("dilation", C.c_int32), ("slope", C.c_float)]


class ConvGroupDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("channels", C.c_int32), ("t", C.c_int32), ("t_stride", C.c_int32), ("n", C.c_int32), ("k", C.c_int32 * 3),
                ("dilation", C.c_int32), ("slope", C.c_float)]


class ResblockDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("channels", C.c_int32), ("t", C.c_int32), ("t_stride", C.c_int32), ("k", C.c_int32), ("ndil", C.c_int32),
                ("dil", C.c_int32 * 3), ("slope", C.c_float), ("out_scale", C.c_float), ("scale_div", C.c_int32), ("variant", C.c_int32),
                ("tiles", C.c_int32), ("nr", C.c_int32)]


class ResblockPlan(C.Structure):
    _fields_ = [("kernel", C.c_char * 96), ("variant", C.c_int32), ("bo", C.c_int32), ("advance", C.c_int32), ("halo", C.c_int32),
                ("segment", C.c_int32), ("tiles", C.c_int32), ("nr", C.c_int32), ("grid_x", C.c_int32), ("grid_y", C.c_int32),
                ("grid_z", C.c_int32), ("block", C.c_int32), ("lds", C.c_int64), ("launches", C.c_int32)]


class FlowCouplingDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("hidden", C.c_int32), ("half", C.c_int32), ("t", C.c_int32), ("t_stride", C.c_int32), ("k", C.c_int32),
                ("layers", C.c_int32), ("rate", C.c_int32), ("flipped", C.c_int32), ("n_bias_rows", C.c_int32), ("variant", C.c_int32),
                ("ncw", C.c_int32), ("nct", C.c_int32)]


class FlowCouplingPlan(C.Structure):
    _fields_ = [("kernel", C.c_char * 96), ("variant", C.c_int32), ("bo", C.c_int32), ("halo", C.c_int32), ("ncw", C.c_int32), ("nct", C.c_int32),
                ("grid_x", C.c_int32), ("grid_y", C.c_int32), ("grid_z", C.c_int32), ("block", C.c_int32), ("lds", C.c_int64), ("launches", C.c_int32)]


class DdsBlockDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("channels", C.c_int32), ("t", C.c_int32), ("t_stride", C.c_int32), ("k", C.c_int32), ("layers", C.c_int32),
                ("eps", C.c_float), ("variant", C.c_int32), ("head", C.c_int32), ("tail", C.c_int32), ("tail_rows", C.c_int32), ("zc", C.c_int32),
                ("n_bias_rows", C.c_int32)]


class DdsBlockPlan(C.Structure):
    _fields_ = [("kernel", C.c_char * 96), ("kernel_last", C.c_char * 96), ("variant", C.c_int32), ("nt", C.c_int32), ("layers", C.c_int32),
                ("halo", C.c_int32 * 8), ("lds", C.c_int64 * 8), ("grid_x", C.c_int32), ("grid_y", C.c_int32), ("block", C.c_int32), ("launches", C.c_int32)]


class DurationPredictorDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("hidden", C.c_int32), ("filter", C.c_int32), ("t", C.c_int32), ("t_stride", C.c_int32),
                ("k", C.c_int32), ("eps", C.c_float), ("variant", C.c_int32)]


class ConvT1dDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32), ("t", C.c_int32), ("t_stride", C.c_int32),
                ("t_out_stride", C.c_int32), ("k", C.c_int32), ("stride", C.c_int32), ("crop", C.c_int32),
                ("pre_slope", C.c_float)]


class Upsample16Desc(C.Structure):
    """vits_upsample16_desc"""
    _fields_ = [("batch", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32), ("t", C.c_int32), ("t_stride", C.c_int32), ("t_out_stride", C.c_int32),
                ("stride", C.c_int32), ("crop", C.c_int32), ("pre_slope", C.c_float), ("y16_slope", C.c_float), ("variant", C.c_int32), ("split", C.c_int32)]


class Upsample16Plan(C.Structure):
    """vits_upsample16_plan"""
    _fields_ = [("kernel", C.c_char * 96), ("tag", C.c_char * 16), ("variant", C.c_int32), ("bn", C.c_int32), ("grid_x", C.c_int32), ("grid_y", C.c_int32),
                ("grid_z", C.c_int32), ("block", C.c_int32), ("lds", C.c_int64)]


class AttentionDesc(C.Structure):
    """vits_attention_desc"""
    _fields_ = [("batch", C.c_int32), ("heads", C.c_int32), ("head_dim", C.c_int32), ("t", C.c_int32), ("t_stride", C.c_int32), ("window", C.c_int32),
                ("q_scale", C.c_float), ("variant", C.c_int32)]


class AttentionPlan(C.Structure):
    """vits_attention_plan"""
    _fields_ = [("kernel", C.c_char * 96), ("variant", C.c_int32), ("nw", C.c_int32), ("maxs", C.c_int32), ("vshift", C.c_int32), ("grid_x", C.c_int32),
                ("grid_y", C.c_int32), ("grid_z", C.c_int32), ("block", C.c_int32), ("lds", C.c_int64)]


class LayerNormDesc(C.Structure):
    """vits_layer_norm_desc"""
    _fields_ = [("batch", C.c_int32), ("channels", C.c_int32), ("t", C.c_int32), ("t_stride", C.c_int32), ("eps", C.c_float), ("tw", C.c_int32),
                ("post_gelu", C.c_int32), ("add_to", C.c_int32)]


class LayerNormPlan(C.Structure):
    """vits_layer_norm_plan"""
    _fields_ = [("kernel", C.c_char * 96), ("tw", C.c_int32), ("grid_x", C.c_int32), ("grid_y", C.c_int32), ("block", C.c_int32), ("lds", C.c_int64)]


class NormConvDesc(C.Structure):
    """vits_norm_conv_desc"""
    _fields_ = [("batch", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32), ("t", C.c_int32), ("t_stride", C.c_int32), ("pitch", C.c_int32), ("k", C.c_int32),
                ("pad_left", C.c_int32), ("post_act", C.c_int32), ("eps", C.c_float), ("variant", C.c_int32)]


class ConvPostDesc(C.Structure):
    _fields_ = [("batch", C.c_int32), ("cin", C.c_int32), ("k", C.c_int32), ("t", C.c_int32), ("x_pitch", C.c_int32), ("pre_pitch", C.c_int32),
                ("slope", C.c_float), ("emit_lo", C.c_int32), ("layout", C.c_int32)]


class NormConvPlan(C.Structure):
    """vits_norm_conv_plan"""
    _fields_ = [("tile", C.c_char * 16), ("ln_why", C.c_char * 96), ("variant", C.c_int32), ("pitch", C.c_int32), ("ln_ok", C.c_int32), ("launches", C.c_int32),
                ("grid_x", C.c_int32), ("grid_y", C.c_int32), ("grid_z", C.c_int32), ("block", C.c_int32), ("lds", C.c_int64)]


_lib = None


def source_sha16():
    """sha256 (first 16 hex digits) over the library's sources (csrc/*.hip|cpp|h, include/*.h): identifies the kernel build
    that a profile artefact (profiles/*_pmc_*.json) was collected with. The GPU box has no .git, so a commit hash is not
    available there; this changes exactly when the code that runs changes."""
    import glob
    import hashlib
    h = hashlib.sha256()
    root = os.path.dirname(_HERE)
    files = sorted(glob.glob(os.path.join(_HERE, "csrc", "*.hip")) + glob.glob(os.path.join(_HERE, "csrc", "*.cpp")) +
                   glob.glob(os.path.join(_HERE, "csrc", "*.h")) + glob.glob(os.path.join(root, "include", "*.h")))
    for f in files:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def lib():
    """Load libvits_hip.so (once). Raises if it has not been built — there is no CPU fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not found: build it first (python -c 'import __graft_entry__ as g; g.build()')")
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, u64, sz, f32p = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_size_t, C.c_void_p
    L.vits_model_load_from_bytes.restype = vp
    L.vits_model_load_from_bytes.argtypes = [C.c_char_p, sz]
    L.vits_model_load_from_file.restype = vp
    L.vits_model_load_from_file.argtypes = [C.c_char_p]
    L.vits_free_model.restype = None
    L.vits_free_model.argtypes = [vp]
    L.vits_free_result.restype = None
    L.vits_free_result.argtypes = [VitsResult]
    L.vits_model_process.restype = VitsResult
    L.vits_model_process.argtypes = [vp, C.c_char_p]
    L.vits_last_error.restype = C.c_char_p
    L.vits_last_error.argtypes = []
    L.vits_model_set_mode.restype = i32
    L.vits_model_set_mode.argtypes = [vp, i32]
    L.vits_model_get_mode.restype = i32
    L.vits_model_get_mode.argtypes = [vp]
    L.vits_model_set_arith.restype = i32
    L.vits_model_set_arith.argtypes = [vp, i32]
    L.vits_model_get_arith.restype = i32
    L.vits_model_get_arith.argtypes = [vp]
    L.vits_model_set_arith_scope.restype = i32
    L.vits_model_set_arith_scope.argtypes = [vp, i32]
    L.vits_model_get_arith_scope.restype = i32
    L.vits_model_get_arith_scope.argtypes = [vp]
    L.vits_reference_noise_seed.restype = None
    L.vits_reference_noise_seed.argtypes = [C.c_uint32]
    L.vits_model_process_ids.restype = VitsResult
    L.vits_model_process_ids.argtypes = [vp, vp, sz]
    L.vits_model_process_batch.restype = i32
    L.vits_model_process_batch.argtypes = [vp, vp, vp, i32, i32, C.POINTER(ProcessOpts), C.POINTER(BatchResult)]
    L.vits_free_batch_result.restype = None
    L.vits_free_batch_result.argtypes = [C.POINTER(BatchResult)]
    L.vits_model_sync.restype = i32
    L.vits_model_sync.argtypes = [vp]
    L.vits_model_set_ggml_tables.restype = i32
    L.vits_model_set_ggml_tables.argtypes = [vp, i32]
    L.vits_model_get_ggml_tables.restype = i32
    L.vits_model_get_ggml_tables.argtypes = [vp]
    L.vits_model_set_speaker.restype = i32
    L.vits_model_set_speaker.argtypes = [vp, i32]
    L.vits_model_get_speaker.restype = i32
    L.vits_model_get_speaker.argtypes = [vp]
    L.vits_model_num_speakers.restype = i32
    L.vits_model_num_speakers.argtypes = [vp]
    L.vits_model_speaker_embedding_size.restype = i32
    L.vits_model_speaker_embedding_size.argtypes = [vp]
    L.vits_model_get_speaker_embedding.restype = i32
    L.vits_model_get_speaker_embedding.argtypes = [vp, i32, f32p, sz]
    L.vits_model_add_voices.restype = i32
    L.vits_model_add_voices.argtypes = [vp, f32p, i32, vp]
    L.vits_model_set_voice.restype = i32
    L.vits_model_set_voice.argtypes = [vp, i32, f32p]
    L.vits_model_clear_voices.restype = i32
    L.vits_model_clear_voices.argtypes = [vp]
    L.vits_model_num_voices.restype = i32
    L.vits_model_num_voices.argtypes = [vp]
    L.vits_model_set_prosody.restype = i32
    L.vits_model_set_prosody.argtypes = [vp, C.c_float, C.c_float, C.c_float]
    L.vits_model_get_prosody.restype = i32
    L.vits_model_get_prosody.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.vits_model_prepare_conversion.restype = i32
    L.vits_model_prepare_conversion.argtypes = [vp]
    L.vits_model_convert_batch.restype = i32
    L.vits_model_convert_batch.argtypes = [vp, vp, vp, i32, i64, vp, vp, C.POINTER(ProcessOpts), C.POINTER(BatchResult)]
    L.vits_model_convert.restype = VitsResult
    L.vits_model_convert.argtypes = [vp, vp, C.c_size_t, i32, i32]
    L.vits_model_align_batch.restype = i32
    L.vits_model_align_batch.argtypes = [vp, vp, vp, i32, i64, vp, vp, i32, vp, C.c_float, C.POINTER(ProcessOpts), vp, vp, vp]
    L.vits_model_align.restype = i64
    L.vits_model_align.argtypes = [vp, vp, C.c_size_t, C.c_char_p, i32, vp, vp, C.c_size_t]
    L.vits_model_hop.restype = i32
    L.vits_model_hop.argtypes = [vp]
    L.vits_op_align.restype = i32
    L.vits_op_align.argtypes = [i32, vp, vp, i32, vp, vp, vp, vp, vp]
    L.vits_model_set_rates.restype = i32
    L.vits_model_set_rates.argtypes = [vp, i32, i32]
    L.vits_model_get_rates.restype = i32
    L.vits_model_get_rates.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.vits_resample_plan.restype = i32
    L.vits_resample_plan.argtypes = [i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.vits_resample_taps.restype = i64
    L.vits_resample_taps.argtypes = [i32, i32, f32p, sz]
    L.vits_resample_length.restype = i64
    L.vits_resample_length.argtypes = [i32, i32, i64]
    L.vits_op_resample.restype = i32
    L.vits_op_resample.argtypes = [i32, i32, i32, vp, i64, vp, vp, i64]
    L.vits_model_set_level.restype = i32
    L.vits_model_set_level.argtypes = [vp, i32, C.c_float, C.c_float]
    L.vits_model_get_level.restype = i32
    L.vits_model_get_level.argtypes = [vp, C.POINTER(i32), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.vits_model_last_levels.restype = i64
    L.vits_model_last_levels.argtypes = [vp, vp, sz]
    L.vits_loudness_plan.restype = i32
    L.vits_loudness_plan.argtypes = [i32, vp, C.POINTER(i32)]
    L.vits_loudness_host.restype = i32
    L.vits_loudness_host.argtypes = [vp, sz, i32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(i32)]
    L.vits_op_level.restype = i32
    L.vits_op_level.argtypes = [C.POINTER(LevelDesc), vp, vp, vp, vp]
    L.vits_model_set_limiter.restype = i32
    L.vits_model_set_limiter.argtypes = [vp, i32]
    L.vits_model_get_limiter.restype = i32
    L.vits_model_get_limiter.argtypes = [vp, C.POINTER(i32)]
    L.vits_model_last_limits.restype = i64
    L.vits_model_last_limits.argtypes = [vp, vp, sz]
    L.vits_limiter_plan.restype = i32
    L.vits_limiter_plan.argtypes = [i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.vits_limiter_host.restype = i32
    L.vits_limiter_host.argtypes = [vp, sz, i32, C.c_double, C.c_double, vp, vp]
    L.vits_op_limit.restype = i32
    L.vits_op_limit.argtypes = [C.POINTER(LimitDesc), vp, vp, vp, vp, vp]
    L.vits_model_set_edges.restype = i32
    L.vits_model_set_edges.argtypes = [vp, C.POINTER(EdgesDesc)]
    L.vits_model_get_edges.restype = i32
    L.vits_model_get_edges.argtypes = [vp, C.POINTER(EdgesDesc)]
    L.vits_pitch_ratio.restype = C.c_float
    L.vits_pitch_ratio.argtypes = [C.c_float]
    L.vits_pitch_plan.restype = i32
    L.vits_pitch_plan.argtypes = [C.c_float, i64, C.POINTER(i64), C.POINTER(i64), C.POINTER(i32), C.POINTER(i64)]
    L.vits_pitch_table.restype = i64
    L.vits_pitch_table.argtypes = [f32p, sz]
    L.vits_pitch_host.restype = i64
    L.vits_pitch_host.argtypes = [vp, i64, C.c_float, vp, sz]
    L.vits_op_pitch.restype = i32
    L.vits_op_pitch.argtypes = [i32, vp, i64, vp, vp, vp, i64, vp]
    L.vits_model_set_pitch.restype = i32
    L.vits_model_set_pitch.argtypes = [vp, C.c_float]
    L.vits_model_get_pitch.restype = i32
    L.vits_model_get_pitch.argtypes = [vp, C.POINTER(C.c_float)]
    L.vits_model_set_pitch_ratios.restype = i32
    L.vits_model_set_pitch_ratios.argtypes = [vp, vp, i32]
    L.vits_model_last_pitch.restype = i64
    L.vits_model_last_pitch.argtypes = [vp, vp, sz]
    L.vits_tempo_plan.restype = i32
    L.vits_tempo_plan.argtypes = [i32, C.c_float, i64, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    L.vits_tempo_host.restype = i64
    L.vits_tempo_host.argtypes = [vp, i64, i32, C.c_float, vp, sz, vp, sz]
    L.vits_model_set_conversion_prosody.restype = i32
    L.vits_model_set_conversion_prosody.argtypes = [vp, C.c_float, C.c_float]
    L.vits_model_get_conversion_prosody.restype = i32
    L.vits_model_get_conversion_prosody.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.vits_model_set_conversion_ratios.restype = i32
    L.vits_model_set_conversion_ratios.argtypes = [vp, vp, vp, i32]
    L.vits_model_last_tempo.restype = i64
    L.vits_model_last_tempo.argtypes = [vp, vp, sz]
    L.vits_fit_host.restype = i32
    L.vits_fit_host.argtypes = [i32, i32, vp, vp, vp, vp, vp, C.c_float, C.c_float, vp, vp]
    L.vits_op_fit_durations.restype = i32
    L.vits_op_fit_durations.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp, C.c_float, C.c_float, vp, vp, vp]
    L.vits_model_set_fit.restype = i32
    L.vits_model_set_fit.argtypes = [vp, vp, vp, i32, C.c_float, C.c_float]
    L.vits_model_set_fit_total.restype = i32
    L.vits_model_set_fit_total.argtypes = [vp, i64, C.c_float, C.c_float]
    L.vits_model_fit_frames.restype = i64
    L.vits_model_fit_frames.argtypes = [vp, C.c_double]
    L.vits_model_last_fit.restype = i64
    L.vits_model_last_fit.argtypes = [vp, vp, sz]
    L.vits_op_tempo.restype = i32
    L.vits_op_tempo.argtypes = [i32, i32, vp, i64, vp, vp, vp, i64, vp, vp, i64]
    L.vits_model_last_edges.restype = i64
    L.vits_model_last_edges.argtypes = [vp, vp, sz]
    L.vits_edges_plan.restype = i32
    L.vits_edges_plan.argtypes = [i32, C.POINTER(EdgesDesc), vp]
    L.vits_edges_host.restype = i32
    L.vits_edges_host.argtypes = [vp, sz, i32, C.POINTER(EdgesDesc), vp, sz, vp]
    L.vits_op_edges.restype = i32
    L.vits_op_edges.argtypes = [i32, C.POINTER(EdgesDesc), i32, vp, i64, vp, vp, i64, vp, vp]
    L.vits_join_plan.restype = i32
    L.vits_join_plan.argtypes = [i32, i32, vp, vp, vp, vp, vp, vp]
    L.vits_join_host.restype = i32
    L.vits_join_host.argtypes = [i32, i32, vp, i64, vp, vp, vp, vp, i64, vp, vp]
    L.vits_op_join.restype = i32
    L.vits_op_join.argtypes = [i32, i32, vp, i64, vp, vp, vp, vp, i64, vp, vp]
    L.vits_split_sentences.restype = i64
    L.vits_split_sentences.argtypes = [C.c_char_p, vp, vp, vp, sz]
    L.vits_model_process_joined.restype = i32
    L.vits_model_process_joined.argtypes = [vp, vp, vp, i32, i32, C.POINTER(ProcessOpts), vp, vp, C.POINTER(BatchResult)]
    L.vits_model_last_joins.restype = i64
    L.vits_model_last_joins.argtypes = [vp, vp, sz]
    L.vits_model_speak.restype = i32
    L.vits_model_speak.argtypes = [vp, C.c_char_p, C.POINTER(SpeakOpts), C.POINTER(BatchResult)]
    L.vits_model_submit_batch.restype = i32
    L.vits_model_submit_batch.argtypes = [vp, vp, vp, i32, i32, C.POINTER(ProcessOpts)]
    L.vits_model_wait.restype = i32
    L.vits_model_wait.argtypes = [vp, C.POINTER(BatchResult)]
    L.vits_model_pending.restype = i32
    L.vits_model_pending.argtypes = [vp]
    L.vits_model_tokenize.restype = i64
    L.vits_model_tokenize.argtypes = [vp, C.c_char_p, vp, sz]
    L.vits_model_sampling_rate.restype = i32
    L.vits_model_sampling_rate.argtypes = [vp]
    L.vits_model_vocab_size.restype = i32
    L.vits_model_vocab_size.argtypes = [vp]
    L.vits_model_weight_bytes.restype = i64
    L.vits_model_weight_bytes.argtypes = [vp]
    L.vits_model_duration_predictor_kind.restype = i32
    L.vits_model_duration_predictor_kind.argtypes = [vp]
    L.vits_op_duration_predictor.restype = i32
    L.vits_op_duration_predictor.argtypes = [vp] * 15
    L.vits_model_get_tap.restype = i64
    L.vits_model_get_tap.argtypes = [vp, C.c_char_p, i32, f32p, sz]
    L.vits_synth_model_bytes.restype = i32
    L.vits_synth_model_bytes.argtypes = [u64, i32, C.POINTER(C.c_void_p), C.POINTER(sz)]
    L.vits_free_bytes.restype = None
    L.vits_free_bytes.argtypes = [vp]
    L.vits_prof_enable.restype = i32
    L.vits_prof_enable.argtypes = [vp, i32]
    L.vits_prof_reset.restype = i32
    L.vits_prof_reset.argtypes = [vp]
    L.vits_prof_report.restype = i64
    L.vits_prof_report.argtypes = [vp, C.c_char_p, sz]
    L.vits_op_conv1d.restype = i32
    L.vits_op_conv1d.argtypes = [C.POINTER(Conv1dDesc), vp, vp, vp, vp, vp, vp, vp]
    L.vits_op_resblock_pair.restype = i32
    L.vits_op_resblock_pair.argtypes = [C.POINTER(ResblockPairDesc), vp, vp, vp, vp, vp, vp, vp]
    L.vits_op_resblock.restype = i32
    L.vits_op_resblock.argtypes = [C.POINTER(ResblockDesc), vp, vp, vp, vp, vp, vp, vp, vp]
    L.vits_op_resblock_plan.restype = i32
    L.vits_op_resblock_plan.argtypes = [C.POINTER(ResblockDesc), C.POINTER(ResblockPlan)]
    L.vits_op_flow_coupling.restype = i32
    L.vits_op_flow_coupling.argtypes = [C.POINTER(FlowCouplingDesc)] + [vp] * 11
    L.vits_op_flow_coupling_plan.restype = i32
    L.vits_op_flow_coupling_plan.argtypes = [C.POINTER(FlowCouplingDesc), C.POINTER(FlowCouplingPlan)]
    L.vits_op_dds_block.restype = i32
    L.vits_op_dds_block.argtypes = [C.POINTER(DdsBlockDesc)] + [vp] * 19
    L.vits_op_dds_block_plan.restype = i32
    L.vits_op_dds_block_plan.argtypes = [C.POINTER(DdsBlockDesc), C.POINTER(DdsBlockPlan)]
    L.vits_op_spline.restype = i32
    L.vits_op_spline.argtypes = [i32, i32, i32, i32, C.c_float, C.c_float, i32, i32, vp, vp, vp]
    L.vits_op_durations.restype = i32
    L.vits_op_durations.argtypes = [i32, i32, i32, i32, vp, vp, C.c_float, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]
    L.vits_op_conv_transpose1d.restype = i32
    L.vits_op_conv_transpose1d.argtypes = [C.POINTER(ConvT1dDesc), vp, vp, vp, vp, vp]
    L.vits_op_upsample16.restype = i32
    L.vits_op_upsample16.argtypes = [C.POINTER(Upsample16Desc), vp, vp, vp, vp, vp, vp, vp]
    L.vits_op_upsample16_plan.restype = i32
    L.vits_op_upsample16_plan.argtypes = [C.POINTER(Upsample16Desc), C.POINTER(Upsample16Plan)]
    L.vits_op_attention.restype = i32
    L.vits_op_attention.argtypes = [C.POINTER(AttentionDesc)] + [vp] * 8
    L.vits_op_attention_plan.restype = i32
    L.vits_op_attention_plan.argtypes = [C.POINTER(AttentionDesc), C.POINTER(AttentionPlan)]
    L.vits_op_layer_norm.restype = i32
    L.vits_op_layer_norm.argtypes = [C.POINTER(LayerNormDesc)] + [vp] * 7
    L.vits_op_layer_norm_plan.restype = i32
    L.vits_op_layer_norm_plan.argtypes = [C.POINTER(LayerNormDesc), C.POINTER(LayerNormPlan)]
    L.vits_op_norm_conv.restype = i32
    L.vits_op_norm_conv.argtypes = [C.POINTER(NormConvDesc)] + [vp] * 9
    L.vits_op_norm_conv_plan.restype = i32
    L.vits_op_norm_conv_plan.argtypes = [C.POINTER(NormConvDesc), C.POINTER(NormConvPlan)]
    L.vits_op_spectrogram.restype = i32
    L.vits_op_spectrogram.argtypes = [i32, i32, i32, i32, vp, i64, vp, i32, vp]
    L.vits_op_prior_sample.restype = i32
    L.vits_op_prior_sample.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, u64, vp, C.c_float, vp, vp]
    L.vits_op_posterior_sample.restype = i32
    L.vits_op_posterior_sample.argtypes = [i32, i32, i32, vp, vp, vp, vp, u64, vp, i32, C.c_float, vp]
    L.vits_op_conv_post.restype = i32
    L.vits_op_conv_post.argtypes = [C.POINTER(ConvPostDesc), vp, vp, vp, vp, vp, vp]
    L.vits_op_resblock_sum.restype = i32
    L.vits_op_resblock_sum.argtypes = [i32, i32, i32, i32, i32, C.c_float, i32, i32, C.c_float, vp, vp, vp, vp, vp]
    L.vits_op_rel_attention.restype = i32
    L.vits_op_rel_attention.argtypes = [i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.vits_op_add_layer_norm.restype = i32
    L.vits_op_add_layer_norm.argtypes = [i32, i32, i32, i32, C.c_float, vp, vp, vp, vp, vp]
    L.vits_model_file_reserialize.restype = i32
    L.vits_model_file_reserialize.argtypes = [C.c_char_p, sz, C.POINTER(C.c_void_p), C.POINTER(sz)]
    L.vits_model_file_tokenize.restype = i64
    L.vits_model_file_tokenize.argtypes = [C.c_char_p, sz, C.c_char_p, vp, sz]
    L.vits_pcm16_from_float.restype = None
    L.vits_pcm16_from_float.argtypes = [vp, sz, vp]
    L.vits_write_wav16.restype = i32
    L.vits_write_wav16.argtypes = [C.c_char_p, vp, sz, i32]
    L.vits_set_device.restype = i32
    L.vits_set_device.argtypes = [i32]
    L.vits_device_info.restype = i32
    L.vits_device_info.argtypes = [C.c_char_p, sz, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64)]
    _lib = L
    return L


class VitsError(RuntimeError):
    pass


def last_error():
    return lib().vits_last_error().decode("utf-8", "replace")


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def _prosody(o, B, stride, speaking_rate, noise_scale, noise_scale_duration, duration_override, durations_out):
    """Fills the prosody fields of a ProcessOpts; returns the arrays it points at (the caller keeps them alive for the call).
    Scalars are broadcast to the batch, None leaves a field NULL (the model value)."""
    keep = []
    for name, v in (("speaking_rates", speaking_rate), ("noise_scales", noise_scale), ("noise_scale_durations", noise_scale_duration)):
        if v is None:
            continue
        if np.ndim(v) and np.size(v) not in (1, B):
            raise ValueError("%s needs a scalar or one value per utterance" % name)
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float32).ravel() if np.ndim(v) else np.float32(v), (B,)))
        setattr(o, name, _ptr(a))
        keep.append(a)
    if duration_override is not None:
        a = np.ascontiguousarray(duration_override, dtype=np.int32).reshape(B, -1)
        if a.shape[1] != stride:
            raise ValueError("duration_override needs [B, id_stride] = [%d, %d] entries" % (B, stride))
        o.duration_override = _ptr(a)
        keep.append(a)
    if durations_out is not None:
        if not (isinstance(durations_out, np.ndarray) and durations_out.dtype == np.int32 and durations_out.flags.c_contiguous
                and durations_out.size == B * stride and durations_out.flags.writeable):
            raise ValueError("durations_out must be a writeable C-contiguous int32 array of [B, id_stride] = [%d, %d]" % (B, stride))
        o.durations_out = _ptr(durations_out)
        keep.append(durations_out)
    return keep


def _opts(B, mode=MODE_DEFAULT, noise_kind=NOISE_COUNTER, noise_seed=4321, noise_dur=None, noise_prior=None, fixed_duration=0, collect_taps=False,
          out_device=None, out_device_stride=0, skip_host_copy=False, async_=False, vocoder_chunk_frames=0, frames_only=False, noise_seed_offsets=None,
          speaker_ids=None):
    """A ProcessOpts with the fields every batch call shares. Returns (opts, keep): keep holds the arrays opts points at (the caller keeps
    it alive for the call)."""
    o = ProcessOpts()
    o.struct_size = C.sizeof(ProcessOpts)
    o.mode, o.noise_kind, o.noise_seed = mode, noise_kind, noise_seed
    nd, npr = _f32(noise_dur), _f32(noise_prior)
    o.noise_dur, o.noise_prior = _ptr(nd), _ptr(npr)
    o.noise_prior_stride = 0 if npr is None else npr.shape[-1]
    o.fixed_duration, o.collect_taps = fixed_duration, int(collect_taps)
    o.out_device = out_device
    o.out_device_stride = out_device_stride
    o.skip_host_copy, o.async_ = int(skip_host_copy), int(async_)
    o.vocoder_chunk_frames = int(vocoder_chunk_frames)
    o.frames_only = int(frames_only)
    nso = None if noise_seed_offsets is None else np.ascontiguousarray(noise_seed_offsets, dtype=np.int32)
    if nso is not None and nso.size != B:
        raise ValueError("noise_seed_offsets needs one entry per utterance")
    o.noise_seed_offsets = _ptr(nso)
    spk = None if speaker_ids is None else np.ascontiguousarray(speaker_ids, dtype=np.int32).ravel()
    if spk is not None and spk.size != B:
        raise ValueError("speaker_ids needs one entry per utterance")
    o.speaker_ids = _ptr(spk)
    return o, [nd, npr, nso, spk]


def _refused_fields(refused, B, noise_scale_arg="noise_scale"):
    """Keyword arguments that a call refuses travel in its options all the same, so that the library says why: pops them from `refused` (anything
    left over is unknown: TypeError) and returns ({ProcessOpts field: value}, the arrays the values point at). noise_scale_arg: the keyword
    that carries opts.noise_scales (alignment has a noise_scale argument of its own)."""
    fields = {"fixed_duration": int(refused.pop("fixed_duration", 0)), "frames_only": int(refused.pop("frames_only", False)),
              "async_": int(refused.pop("async_", False))}
    spk = refused.pop("speaker_ids", None)
    keep = [None if spk is None else np.ascontiguousarray(spk, dtype=np.int32).ravel()]
    fields["speaker_ids"] = _ptr(keep[0])
    for arg, field, dtype in (("speaking_rate", "speaking_rates", np.float32), (noise_scale_arg, "noise_scales", np.float32),
                              ("noise_scale_duration", "noise_scale_durations", np.float32), ("duration_override", "duration_override", np.int32),
                              ("durations_out", "durations_out", np.int32)):
        v = refused.pop(arg, None)
        if v is not None:
            keep.append(np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype).ravel(), (max(B, np.size(v)),))))
            fields[field] = _ptr(keep[-1])
    if refused:
        raise TypeError("unknown arguments: %s" % sorted(refused))
    return fields, keep


def _chunk_sink(o, on_chunk):
    """Points o.on_chunk at a wrapper of the caller's sink on_chunk(utt, offset, pcm ndarray). Returns the list that receives an exception the sink
    raised (the wrapper then asks the library to abort: an exception must never unwind through the C frames)."""
    cb_error = []
    if on_chunk is not None:
        def _cb(_user, utt, offset, pcm, n):
            try:
                return 1 if on_chunk(int(utt), int(offset), np.ctypeslib.as_array(pcm, shape=(n,)).copy()) else 0
            except BaseException as e:
                cb_error.append(e)
                return 1
        o.on_chunk = ChunkCallback(_cb)
    return cb_error


def _take_result(res, B, keep_pcm):
    """(list of per-utterance PCM arrays or None, lengths, frames) of a BatchResult, which is freed"""
    try:
        lengths = np.ctypeslib.as_array(res.lengths, shape=(B,)).copy()
        frames = np.ctypeslib.as_array(res.frames, shape=(B,)).copy()
        pcm = None
        if res.data and keep_pcm:
            full = np.ctypeslib.as_array(res.data, shape=(B, res.stride))
            pcm = [full[b, : lengths[b]].copy() for b in range(B)]
        return pcm, lengths, frames
    finally:
        lib().vits_free_batch_result(C.byref(res))


def synth_model_bytes(seed=0x5EED, arch=SYNTH_FULL):
    """Deterministic synthetic model file in the reference's on-disk format (host-only, no GPU needed)."""
    p, n = C.c_void_p(), C.c_size_t()
    if lib().vits_synth_model_bytes(seed, arch, C.byref(p), C.byref(n)) != 0:
        raise VitsError(last_error())
    try:
        return C.string_at(p, n.value)
    finally:
        lib().vits_free_bytes(p)


def reserialize(data):
    """parse + write back a model file (host only)"""
    p, n = C.c_void_p(), C.c_size_t()
    if lib().vits_model_file_reserialize(data, len(data), C.byref(p), C.byref(n)) != 0:
        raise VitsError(last_error())
    try:
        return C.string_at(p, n.value)
    finally:
        lib().vits_free_bytes(p)


def validate(data):
    """Host-only load check of a model file (vits_model_file_validate); raises VitsError with the reason."""
    f = lib().vits_model_file_validate
    f.restype, f.argtypes = C.c_int32, [C.c_char_p, C.c_size_t]
    if f(data, len(data)) != 0:
        raise VitsError(last_error())


def file_tokenize(data, text):
    buf = np.zeros(4 * len(text.encode("utf-8")) + 8, np.int32)
    n = lib().vits_model_file_tokenize(data, len(data), text.encode("utf-8"), _ptr(buf), buf.size)
    if n < 0:
        raise VitsError(last_error())
    return buf[:n].copy()


def synth_ids(batch, n_ids, vocab=38, ids_seed=1234):
    """Synthetic phoneme ids of include/vits_synth_noise.h (blank-interleaved, uniform over the vocabulary)."""
    M = (1 << 64) - 1

    def mix(z):
        z = (z + 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    def hash3(seed, stream, index):
        h = mix(seed ^ 0xD1B54A32D192ED03)
        h = mix(h ^ ((stream * 0x9E3779B97F4A7C15) & M))
        return mix(h ^ index)

    out = np.zeros((batch, n_ids), np.int32)
    for u in range(batch):
        for t in range(1, n_ids, 2):
            out[u, t] = 1 + (hash3((ids_seed + u) & M, 3, t) >> 33) % (vocab - 1)
    return out


class Model:
    """One loaded model on the current HIP device (mirror of the reference's opaque ``vits_model*``)."""

    def __init__(self, data=None, path=None):
        L = lib()
        if path is not None:
            self._h = L.vits_model_load_from_file(os.fsencode(path))
        else:
            self._h = L.vits_model_load_from_bytes(data, len(data))
        if not self._h:
            raise VitsError(last_error())

    def close(self):
        if getattr(self, "_h", None):
            lib().vits_free_model(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- reference entry points ---------------------------------------------------------------------
    def process(self, text):
        r = lib().vits_model_process(self._h, text.encode("utf-8"))
        if not r.data:
            raise VitsError(last_error())
        try:
            return np.ctypeslib.as_array(r.data, shape=(r.size,)).copy()
        finally:
            lib().vits_free_result(r)

    def process_ids(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        r = lib().vits_model_process_ids(self._h, _ptr(ids), ids.size)
        if not r.data:
            raise VitsError(last_error())
        try:
            return np.ctypeslib.as_array(r.data, shape=(r.size,)).copy()
        finally:
            lib().vits_free_result(r)

    # -- extensions -----------------------------------------------------------------------------------
    def set_mode(self, mode):
        if lib().vits_model_set_mode(self._h, mode) != 0:
            raise VitsError(last_error())

    def set_arith(self, arith):
        """ARITH_F32 (exact, default) | ARITH_BF16 | ARITH_F16: conv operand precision (include/vits.h VITS_ARITH_*)"""
        if lib().vits_model_set_arith(self._h, arith) != 0:
            raise VitsError(last_error())

    @property
    def arith(self):
        return lib().vits_model_get_arith(self._h)

    def set_arith_scope(self, scope):
        """SCOPE_FLOW_VOCODER (default: stage one stays exact fp32, durations bit-identical to the fp32 path) | SCOPE_ALL_CONVS
        (the literal Q7 arithmetic: every conv of the path) — include/vits.h VITS_ARITH_SCOPE_*"""
        if lib().vits_model_set_arith_scope(self._h, scope) != 0:
            raise VitsError(last_error())

    def set_ggml_tables(self, on):
        """EMULATED ggml fp16 lookup tables for ggml_gelu / ggml_soft_max (Q8; inferred from upstream ggml, the reference's fork is absent)"""
        if lib().vits_model_set_ggml_tables(self._h, int(on)) != 0:
            raise VitsError(last_error())

    def set_speaker(self, speaker):
        """the speaker of every utterance a call does not name (process_ids / the text entry point / speaker_ids=None); -1 = none"""
        if lib().vits_model_set_speaker(self._h, int(speaker)) != 0:
            raise VitsError(last_error())

    @property
    def speaker(self):
        return int(lib().vits_model_get_speaker(self._h))

    @property
    def num_speakers(self):
        """1 for a single-speaker model"""
        return int(lib().vits_model_num_speakers(self._h))

    # -- custom voices: speaker embeddings registered at run time (include/vits.h vits_model_add_voices) ---------------------------
    @property
    def speaker_embedding_size(self):
        """E, the length of a speaker embedding; 0 for a single-speaker model"""
        return int(lib().vits_model_speaker_embedding_size(self._h))

    @property
    def num_voices(self):
        return int(lib().vits_model_num_voices(self._h))

    def speaker_embedding(self, id):
        """fp32 [E]: the file's embed_speaker row of a speaker, or the vector a voice was registered with"""
        out = np.zeros(max(self.speaker_embedding_size, 1), np.float32)
        n = lib().vits_model_get_speaker_embedding(self._h, int(id), _ptr(out), out.size)
        if n < 0:
            raise VitsError(last_error())
        return out[:n]

    def add_voices(self, emb):
        """registers the rows of emb ([n][E], or one vector [E]) as voices; returns their ids (num_speakers + k, in order of registration), which
        every speaker argument accepts from then on"""
        emb = np.ascontiguousarray(emb, dtype=np.float32)
        E = self.speaker_embedding_size
        if emb.ndim == 1 and E > 0:
            emb = emb[None]
        if E > 0 and (emb.ndim != 2 or emb.shape[1] != E):
            raise ValueError("voices are rows of %d floats" % E)
        n = int(emb.shape[0]) if emb.ndim >= 1 else 0
        ids = np.zeros(max(n, 1), np.int32)
        if lib().vits_model_add_voices(self._h, _ptr(emb), n, _ptr(ids)) != 0:
            raise VitsError(last_error())
        return ids[:n].tolist()

    def set_voice(self, voice_id, emb):
        """overwrites a registered voice in place"""
        emb = np.ascontiguousarray(emb, dtype=np.float32).ravel()
        if emb.size != self.speaker_embedding_size and self.speaker_embedding_size > 0:
            raise ValueError("a voice is %d floats" % self.speaker_embedding_size)
        if lib().vits_model_set_voice(self._h, int(voice_id), _ptr(emb)) != 0:
            raise VitsError(last_error())

    def clear_voices(self):
        """forgets every voice; ids start again at num_speakers"""
        if lib().vits_model_clear_voices(self._h) != 0:
            raise VitsError(last_error())

    def add_voice_mix(self, ids, weights):
        """registers sum(weights[k] * speaker_embedding(ids[k])) — fp32, accumulated left to right in numpy — as one voice and returns its id
        (a blend of speakers and / or voices; Python only: the C ABI has one way in, vits_model_add_voices)"""
        ids, weights = list(ids), np.asarray(weights, np.float32).ravel()
        if len(ids) != weights.size or not ids:
            raise ValueError("one weight per id, at least one")
        acc = np.zeros(self.speaker_embedding_size, np.float32)
        for k, i in enumerate(ids):
            acc = (acc + weights[k] * self.speaker_embedding(i)).astype(np.float32)
        return self.add_voices(acc)[0]

    # -- a stated pitch: the model-level ratio (vits_model_set_pitch) ------------------------------------------------------------
    @property
    def pitch(self):
        """the model-level pitch ratio (1 = off): what every utterance a call gives no pitch_ratio for is shifted by"""
        v = C.c_float()
        if lib().vits_model_get_pitch(self._h, C.byref(v)) != 0:
            raise VitsError(last_error())
        return float(v.value)

    def set_pitch(self, ratio=1.0):
        """vits_model_set_pitch: a ratio in [0.5, 2] (pitch_ratio(semitones)); 1 switches the stage off"""
        if lib().vits_model_set_pitch(self._h, float(ratio)) != 0:
            raise VitsError(last_error())

    def set_pitch_ratios(self, ratios=None):
        """vits_model_set_pitch_ratios: one ratio per utterance for the NEXT call on this handle (None drops what was given); the pitch_ratio keyword of
        process_batch, submit_batch and process_joined does this"""
        a = None if ratios is None else np.ascontiguousarray(ratios, dtype=np.float32).ravel()
        if lib().vits_model_set_pitch_ratios(self._h, _ptr(a), 0 if a is None else a.size) != 0:
            raise VitsError(last_error())

    def _with_pitch(self, pitch_ratio, B, c_call):
        """The pitch_ratio keyword of a call: runs c_call() (the library call itself, with nothing of Python's between the two) with the ratios given to
        the handle and returns what it returns. A scalar is broadcast to the batch; None gives nothing (the model value). Whatever happens, no ratio given
        here is left on the handle for a later call."""
        if pitch_ratio is None:
            return c_call()
        if np.ndim(pitch_ratio) and np.size(pitch_ratio) not in (1, B):
            raise ValueError("pitch_ratio needs a scalar or one value per utterance")
        self.set_pitch_ratios(np.broadcast_to(np.asarray(pitch_ratio, np.float32).ravel(), (B,)))
        try:
            return c_call()
        finally:
            self.set_pitch_ratios(None)

    def last_pitch(self):
        """vits_model_last_pitch: int64 [B, 3] = (P, N, N') of the most recently completed call, or None when it shifted nothing"""
        n = lib().vits_model_last_pitch(self._h, None, 0)
        if n < 0:
            raise VitsError(last_error())
        if n == 0:
            return None
        out = np.zeros((n, 3), np.int64)
        if lib().vits_model_last_pitch(self._h, _ptr(out), out.size) != n:
            raise VitsError(last_error())
        return out

    # -- a stated duration: the length scale fitted to a target frame count (vits_model_set_fit) ---------------------------------------
    def set_fit(self, targets=None, groups=None, min_rate=0.1, max_rate=10.0):
        """vits_model_set_fit: the fit of the NEXT call on this handle (None drops what was given). targets: int64 [n], one target in frames per group (0: the
        group is not fitted); groups: int32 [n], the group of every utterance (None: utterance b is group b); n must be that call's batch. The fit= keyword of
        process_batch, submit_batch and process_joined does this."""
        t = None if targets is None else np.ascontiguousarray(targets, dtype=np.int64).ravel()
        g = None if groups is None or t is None else np.ascontiguousarray(groups, dtype=np.int32).ravel()
        if g is not None and g.size != t.size:
            raise ValueError("groups needs one entry per target")
        if lib().vits_model_set_fit(self._h, _ptr(t), _ptr(g), 0 if t is None else t.size, float(min_rate), float(max_rate)) != 0:
            raise VitsError(last_error())

    def set_fit_total(self, frames, min_rate=0.1, max_rate=10.0):
        """vits_model_set_fit_total: the NEXT call's utterances form one group that lasts `frames` frames, whatever their number (what speak takes)"""
        if lib().vits_model_set_fit_total(self._h, int(frames), float(min_rate), float(max_rate)) != 0:
            raise VitsError(last_error())

    def fit_frames(self, seconds):
        """vits_model_fit_frames: the largest frame count whose samples fit into `seconds` at the model's rate, at least 1"""
        n = lib().vits_model_fit_frames(self._h, float(seconds))
        if n < 0:
            raise VitsError(last_error())
        return int(n)

    def _with_fit(self, fit, c_call):
        """The fit= keyword of a call: None gives nothing; an int is set_fit_total's frames; a dict holds set_fit's or set_fit_total's keywords (targets or
        frames, groups, min_rate, max_rate). Runs c_call() with the fit given to the handle and returns what it returns. Whatever happens, no fit given here is
        left on the handle for a later call."""
        if fit is None:
            return c_call()
        kw = dict(fit) if isinstance(fit, dict) else {"frames": fit}
        if "frames" in kw:
            self.set_fit_total(**kw)
        else:
            self.set_fit(**kw)
        try:
            return c_call()
        finally:
            self.set_fit(None)

    def last_fit(self):
        """vits_model_last_fit: float64 [B, 6] = (group, F, sum d of the group, s*, R, status) per utterance of the most recently completed call, or None when
        it fitted nothing"""
        n = lib().vits_model_last_fit(self._h, None, 0)
        if n < 0:
            raise VitsError(last_error())
        if n == 0:
            return None
        out = np.zeros((n, 6), np.float64)
        if lib().vits_model_last_fit(self._h, _ptr(out), out.size) != n:
            raise VitsError(last_error())
        return out

    # -- a conversion's rate and pitch: the model-level values (vits_model_set_conversion_prosody) ------------------------------------
    @property
    def conversion_prosody(self):
        """(rate, pitch) of every utterance of a conversion that vc_rate / vc_pitch give none for (1, 1 = off)"""
        r, p = C.c_float(), C.c_float()
        if lib().vits_model_get_conversion_prosody(self._h, C.byref(r), C.byref(p)) != 0:
            raise VitsError(last_error())
        return float(r.value), float(p.value)

    def set_conversion_prosody(self, rate=1.0, pitch=1.0):
        """vits_model_set_conversion_prosody: the rate and the pitch of a conversion, each in [0.5, 2]; 1, 1 switches both stages off"""
        if lib().vits_model_set_conversion_prosody(self._h, float(rate), float(pitch)) != 0:
            raise VitsError(last_error())

    def set_conversion_ratios(self, rates=None, pitches=None):
        """vits_model_set_conversion_ratios: one (rate, pitch) pair per utterance for the NEXT conversion on this handle (None for one of them: the model
        value; None for both drops what was given); the vc_rate / vc_pitch keywords of convert_batch and convert do this"""
        r = None if rates is None else np.ascontiguousarray(rates, dtype=np.float32).ravel()
        p = None if pitches is None else np.ascontiguousarray(pitches, dtype=np.float32).ravel()
        if r is not None and p is not None and r.size != p.size:
            raise ValueError("rates and pitches need the same count")
        n = 0 if r is None and p is None else (r if r is not None else p).size
        if lib().vits_model_set_conversion_ratios(self._h, _ptr(r), _ptr(p), n) != 0:
            raise VitsError(last_error())

    def _with_conversion_ratios(self, vc_rate, vc_pitch, B, c_call):
        """The vc_rate / vc_pitch keywords of a conversion: runs c_call() with the pairs given to the handle and returns what it returns. A scalar is broadcast
        to the batch; None gives nothing (the model value). Whatever happens, no pair given here is left on the handle for a later call."""
        if vc_rate is None and vc_pitch is None:
            return c_call()
        given = []
        for v in (vc_rate, vc_pitch):
            if v is not None and np.ndim(v) and np.size(v) not in (1, B):
                raise ValueError("vc_rate and vc_pitch need a scalar or one value per utterance")
            given.append(None if v is None else np.broadcast_to(np.asarray(v, np.float32).ravel(), (B,)))
        self.set_conversion_ratios(*given)
        try:
            return c_call()
        finally:
            self.set_conversion_ratios(None, None)

    def last_tempo(self):
        """vits_model_last_tempo: int64 [B, 4] = (Q, N, N', F) of the most recently completed call, or None when it stretched nothing"""
        n = lib().vits_model_last_tempo(self._h, None, 0)
        if n < 0:
            raise VitsError(last_error())
        if n == 0:
            return None
        out = np.zeros((n, 4), np.int64)
        if lib().vits_model_last_tempo(self._h, _ptr(out), out.size) != n:
            raise VitsError(last_error())
        return out

    # -- prosody: the transformers.VitsModel attributes, the model-level values (vits_model_set_prosody) --------------------------
    def get_prosody(self):
        """(speaking_rate, noise_scale, noise_scale_duration) the reference entry points and calls without per-utterance values use"""
        v = [C.c_float() for _ in range(3)]
        if lib().vits_model_get_prosody(self._h, *[C.byref(x) for x in v]) != 0:
            raise VitsError(last_error())
        return tuple(float(x.value) for x in v)

    def set_prosody(self, speaking_rate=None, noise_scale=None, noise_scale_duration=None):
        """sets the given values (None keeps the current one); a rejected value leaves all three unchanged"""
        cur = self.get_prosody()
        new = [cur[i] if v is None else float(v) for i, v in enumerate((speaking_rate, noise_scale, noise_scale_duration))]
        if lib().vits_model_set_prosody(self._h, *new) != 0:
            raise VitsError(last_error())

    @property
    def speaking_rate(self):
        return self.get_prosody()[0]

    @speaking_rate.setter
    def speaking_rate(self, v):
        self.set_prosody(speaking_rate=v)

    @property
    def noise_scale(self):
        return self.get_prosody()[1]

    @noise_scale.setter
    def noise_scale(self, v):
        self.set_prosody(noise_scale=v)

    @property
    def noise_scale_duration(self):
        return self.get_prosody()[2]

    @noise_scale_duration.setter
    def noise_scale_duration(self, v):
        self.set_prosody(noise_scale_duration=v)

    # -- a stated level (vits_model_set_level): gain, sample peak or BS.1770 loudness of every PCM the handle delivers ------------------------------
    @property
    def level(self):
        """(kind, value_db, ceiling_db) of the handle; kind is one of LEVEL_NONE .. LEVEL_LOUDNESS"""
        k, v, c = C.c_int32(), C.c_float(), C.c_float()
        if lib().vits_model_get_level(self._h, C.byref(k), C.byref(v), C.byref(c)) != 0:
            raise VitsError(last_error())
        return int(k.value), float(v.value), float(c.value)

    def set_level(self, kind=LEVEL_NONE, value_db=0.0, ceiling_db=0.0):
        """vits_model_set_level: LEVEL_NONE (nothing is queued), LEVEL_MEASURE (measured only), LEVEL_GAIN (value_db of gain), LEVEL_PEAK (sample peak at
        value_db) or LEVEL_LOUDNESS (value_db LUFS, the sample peak kept at or below ceiling_db). The model-rate waveform is measured and multiplied on
        the device, before the resampler; last_levels() reads what was measured."""
        if lib().vits_model_set_level(self._h, int(kind), float(value_db), float(ceiling_db)) != 0:
            raise VitsError(last_error())

    def last_levels(self):
        """vits_model_last_levels: float32 [B, 4] = (L in LUFS, -inf = unmeasurable; sample peak; gain; blocks that passed both gates) of the most
        recently completed call, or None when it ran with LEVEL_NONE. After an async call: valid after sync()."""
        n = lib().vits_model_last_levels(self._h, None, 0)
        if n < 0:
            raise VitsError(last_error())
        if n == 0:
            return None
        out = np.zeros((n // 4, 4), np.float32)
        if lib().vits_model_last_levels(self._h, _ptr(out), out.size) != n:
            raise VitsError(last_error())
        return out

    # -- the loudness target under a ceiling (vits_model_set_limiter): true-peak meter and look-ahead limiter behind the level ---------------------
    @property
    def limiter(self):
        """the handle's limiter mode: LIMIT_OFF or LIMIT_TRUE_PEAK"""
        m = C.c_int32()
        if lib().vits_model_get_limiter(self._h, C.byref(m)) != 0:
            raise VitsError(last_error())
        return int(m.value)

    def set_limiter(self, mode=LIMIT_OFF):
        """vits_model_set_limiter: with LIMIT_TRUE_PEAK, LEVEL_GAIN and LEVEL_LOUDNESS deliver the gain that was asked for through a look-ahead limiter that
        keeps the model-rate row at or below ceiling_db, and LEVEL_PEAK normalises the true peak; last_limits() reads what it did."""
        if lib().vits_model_set_limiter(self._h, int(mode)) != 0:
            raise VitsError(last_error())

    def last_limits(self):
        """vits_model_last_limits: float32 [B, 4] = (true peak of the waveform; true peak of the delivered model-rate row; the smallest limiter gain; the share
        of samples it turned down) of the most recently completed call, or None when it ran without the limiter. After an async call: valid after sync()."""
        n = lib().vits_model_last_limits(self._h, None, 0)
        if n < 0:
            raise VitsError(last_error())
        if n == 0:
            return None
        out = np.zeros((n // 4, 4), np.float32)
        if lib().vits_model_last_limits(self._h, _ptr(out), out.size) != n:
            raise VitsError(last_error())
        return out

    # -- stated edges (vits_model_set_edges): trimmed silence, fades and pauses in front of levelling ------------------------------------------------
    @property
    def edges(self):
        """the handle's vits_edges_desc as a dict (mode EDGES_OFF and zeros when the stage is off)"""
        d = EdgesDesc()
        if lib().vits_model_get_edges(self._h, C.byref(d)) != 0:
            raise VitsError(last_error())
        return {name: getattr(d, name) for name, _ in EdgesDesc._fields_ if name != "struct_size"}

    def set_edges(self, mode=EDGES_OFF, **fields):
        """vits_model_set_edges: EDGES_OFF (nothing is queued), EDGES_PAD (fades and pads only), EDGES_TRIM_RELATIVE / _ABSOLUTE (the near-silence at both
        ends is trimmed first: threshold_db relative to the loudest 10 ms window, or to mean square 1). Fields: threshold_db, keep_head_ms, keep_tail_ms,
        fade_in_ms, fade_out_ms, lead_ms, tail_ms. lengths of every result are then the trimmed, padded ones; last_edges() reads where each row was cut."""
        d = edges_desc(mode, **fields)
        if lib().vits_model_set_edges(self._h, C.byref(d)) != 0:
            raise VitsError(last_error())

    def last_edges(self):
        """vits_model_last_edges: int64 [B, 4] = (a, b, N', n_active) of the most recently completed call, or None when it ran with EDGES_OFF"""
        n = lib().vits_model_last_edges(self._h, None, 0)
        if n < 0:
            raise VitsError(last_error())
        if n == 0:
            return None
        out = np.zeros((n // 4, 4), np.int64)
        if lib().vits_model_last_edges(self._h, _ptr(out), out.size) != n:
            raise VitsError(last_error())
        return out

    # -- any sample rate (vits_model_set_rates): 0 = the model's own rate --------------------------------------------------------------
    @property
    def rates(self):
        """(input_rate, output_rate) of the handle; 0 = the model's own rate (a rate equal to it reads back as 0)"""
        v = [C.c_int32(), C.c_int32()]
        if lib().vits_model_get_rates(self._h, C.byref(v[0]), C.byref(v[1])) != 0:
            raise VitsError(last_error())
        return int(v[0].value), int(v[1].value)

    def set_rates(self, input_rate=None, output_rate=None):
        """vits_model_set_rates: input_rate = the rate of the PCM given to convert* / align*, output_rate = the rate of every PCM the handle delivers
        (lengths, strides and on_chunk offsets are then in output samples). None leaves a rate as it is, 0 = the model's rate."""
        cur = self.rates
        new = [int(cur[i] if v is None else v) for i, v in enumerate((input_rate, output_rate))]
        if lib().vits_model_set_rates(self._h, *new) != 0:
            raise VitsError(last_error())

    @property
    def ggml_tables(self):
        return bool(lib().vits_model_get_ggml_tables(self._h))

    @property
    def ggml_tables_mode(self):
        """0 off, 1 tables + stage one in the exact order shared with the oracle, 2 tables inside the throughput kernels"""
        return int(lib().vits_model_get_ggml_tables(self._h))

    @property
    def arith_scope(self):
        return lib().vits_model_get_arith_scope(self._h)

    @property
    def mode(self):
        return lib().vits_model_get_mode(self._h)

    @property
    def sampling_rate(self):
        return lib().vits_model_sampling_rate(self._h)

    @property
    def vocab_size(self):
        return lib().vits_model_vocab_size(self._h)

    @property
    def weight_bytes(self):
        return lib().vits_model_weight_bytes(self._h)

    @property
    def duration_predictor_kind(self):
        """DP_STOCHASTIC (0), or DP_DETERMINISTIC (1): use_stochastic_duration_prediction = False — durations without noise (noise_scale_duration is
        validated and has no effect, "noise_dur" is no tap, NOISE_EXPLICIT needs no noise_dur)."""
        return lib().vits_model_duration_predictor_kind(self._h)

    def tokenize(self, text):
        buf = np.zeros(4 * len(text.encode("utf-8")) + 8, np.int32)
        n = lib().vits_model_tokenize(self._h, text.encode("utf-8"), _ptr(buf), buf.size)
        if n < 0:
            raise VitsError(last_error())
        return buf[:n].copy()

    def process_batch(self, ids, id_lengths=None, mode=MODE_DEFAULT, noise_kind=NOISE_COUNTER, noise_seed=4321,
                      noise_dur=None, noise_prior=None, fixed_duration=0, collect_taps=False, out_device=None,
                      out_device_stride=0, skip_host_copy=False, async_=False, vocoder_chunk_frames=0, on_chunk=None, frames_only=False, noise_seed_offsets=None, keep_pcm=True,
                      speaker_ids=None, speaking_rate=None, noise_scale=None, noise_scale_duration=None, duration_override=None, durations_out=None,
                      pitch_ratio=None, fit=None):
        """ids: int32 [B, id_stride]. Returns (list of per-utterance PCM arrays or None, lengths, frames).
        vocoder_chunk_frames > 0 runs the vocoder window by window (bit-identical PCM, bounded activations);
        on_chunk(utt, offset, pcm ndarray) is then called as each window's samples reach the host (return True to abort).
        speaker_ids: one speaker per utterance (-1 = none; None = the model default, set_speaker).
        speaking_rate / noise_scale / noise_scale_duration: a scalar for the whole batch or one value per utterance (None = the model values);
        duration_override: int32 [B, id_stride] (>= 0: the token's frames, -1: the prediction); durations_out: a caller-owned int32 [B, id_stride]
        array that receives every token's frames. pitch_ratio: a scalar or one ratio per utterance in [0.5, 2] (pitch_ratio(semitones); None = the
        model value, set_pitch): the utterance is spoken slower by it and played back faster by it, on the device. fit: the frames the whole batch lasts as one
        group (an int), or a dict of set_fit's keywords (targets, groups, min_rate, max_rate) or set_fit_total's (frames, min_rate, max_rate): the length scale is
        fitted on the device; last_fit() reads the result."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        if ids.ndim == 1:
            ids = ids[None, :]
        B, stride = ids.shape
        lens = np.full(B, stride, np.int32) if id_lengths is None else np.ascontiguousarray(id_lengths, dtype=np.int32)
        o, keep = _opts(B, mode, noise_kind, noise_seed, noise_dur, noise_prior, fixed_duration, collect_taps, out_device, out_device_stride, skip_host_copy,
                        async_, vocoder_chunk_frames, frames_only, noise_seed_offsets, speaker_ids)
        keep += _prosody(o, B, stride, speaking_rate, noise_scale, noise_scale_duration, duration_override, durations_out)
        cb_error = _chunk_sink(o, on_chunk)
        res = BatchResult()
        call = lambda: lib().vits_model_process_batch(self._h, _ptr(ids), _ptr(lens), B, stride, C.byref(o), C.byref(res))
        if self._with_fit(fit, lambda: self._with_pitch(pitch_ratio, B, call)) != 0:
            if cb_error:
                raise cb_error[0]
            raise VitsError(last_error())
        return _take_result(res, B, keep_pcm)

    @staticmethod
    def _joined_opts(B, stride, mode=MODE_DEFAULT, noise_kind=NOISE_COUNTER, noise_seed=4321, noise_dur=None, noise_prior=None, fixed_duration=0, collect_taps=False,
                     out_device=None, out_device_stride=0, skip_host_copy=False, async_=False, vocoder_chunk_frames=0, on_chunk=None, frames_only=False,
                     noise_seed_offsets=None, speaker_ids=None, speaking_rate=None, noise_scale=None, noise_scale_duration=None, duration_override=None,
                     durations_out=None, pitch_ratio=None, fit=None):
        """the options of process_batch's keywords (what a joined call refuses travels too, so that the library says why) -> (opts, keep, cb_error).
        pitch_ratio and fit are no fields of the options: the caller gives them to the handle (Model._with_pitch, Model._with_fit)"""
        o, keep = _opts(B, mode, noise_kind, noise_seed, noise_dur, noise_prior, fixed_duration, collect_taps, out_device, out_device_stride, skip_host_copy,
                        async_, vocoder_chunk_frames, frames_only, noise_seed_offsets, speaker_ids)
        keep += _prosody(o, B, stride, speaking_rate, noise_scale, noise_scale_duration, duration_override, durations_out)
        return o, keep, _chunk_sink(o, on_chunk)

    def process_joined(self, ids, id_lengths=None, track=None, gap_ms=None, keep_pcm=True, **kw):
        """vits_model_process_joined: process_batch with the utterances laid end to end into tracks inside the call, in front of the handle's level, limiter and
        resampler. track: int32 [B] (None: one track), gap_ms: float32 [B] (None: 0), as join_plan takes them; the other keywords are process_batch's.
        Returns (list of per-TRACK PCM arrays or None, lengths [G], frames [G]); last_joins() reads where every utterance lies."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        if ids.ndim == 1:
            ids = ids[None, :]
        B, stride = ids.shape
        lens = np.full(B, stride, np.int32) if id_lengths is None else np.ascontiguousarray(id_lengths, dtype=np.int32)
        tr = None if track is None else np.ascontiguousarray(track, dtype=np.int32).ravel()
        gp = None if gap_ms is None else np.ascontiguousarray(gap_ms, dtype=np.float32).ravel()
        for name, v in (("track", tr), ("gap_ms", gp)):
            if v is not None and v.size != B:
                raise ValueError("%s needs one entry per utterance" % name)
        o, keep, cb_error = self._joined_opts(B, stride, **kw)
        res = BatchResult()
        call = lambda: lib().vits_model_process_joined(self._h, _ptr(ids), _ptr(lens), B, stride, C.byref(o), _ptr(tr), _ptr(gp), C.byref(res))
        if self._with_fit(kw.get("fit"), lambda: self._with_pitch(kw.get("pitch_ratio"), B, call)) != 0:
            if cb_error:
                raise cb_error[0]
            raise VitsError(last_error())
        return _take_result(res, int(res.batch), keep_pcm)

    def speak(self, text, sentence_gap_ms=0.0, paragraph_gap_ms=0.0, track_per_paragraph=False, keep_pcm=True, **kw):
        """vits_model_speak: a whole text -> one programme. split_sentences cuts it, the model's tokenizer turns every span into ids, and the spans that have
        some run as one process_joined call: sentence_gap_ms in front of a sentence, paragraph_gap_ms in front of the first sentence of a paragraph, every
        paragraph its own track if track_per_paragraph. The other keywords are process_batch's (the per-utterance arrays are refused). Returns (list of
        per-track PCM arrays or None, lengths, frames); last_joins()[:, 0] are the span indices of split_sentences(text)."""
        so = SpeakOpts()
        so.struct_size = C.sizeof(SpeakOpts)
        so.sentence_gap_ms, so.paragraph_gap_ms, so.track_per_paragraph = float(sentence_gap_ms), float(paragraph_gap_ms), int(bool(track_per_paragraph))
        o, keep, cb_error = self._joined_opts(max(1, np.size(kw.get("speaker_ids", 0))), 1, **kw)
        so.process = C.pointer(o)
        res = BatchResult()
        raw = None if text is None else text.encode("utf-8")
        # (given ratios are refused by the library: one per utterance, and the text decides how many there are)
        call = lambda: lib().vits_model_speak(self._h, raw, C.byref(so), C.byref(res))
        # (so is the per-group form of a fit; the total form, fit=frames, is what a whole text takes)
        if self._with_fit(kw.get("fit"), lambda: self._with_pitch(kw.get("pitch_ratio"), max(1, np.size(kw.get("pitch_ratio"))), call)) != 0:
            if cb_error:
                raise cb_error[0]
            raise VitsError(last_error())
        return _take_result(res, int(res.batch), keep_pcm)

    def last_joins(self):
        """vits_model_last_joins: int64 [B, 4] = (index, track, o_b, n_b) of the most recently completed joined call (o_b, n_b at the model's rate; with an
        output rate set, resample_length(o_b) is the position in the delivered track), or None when the last call did not join"""
        n = lib().vits_model_last_joins(self._h, None, 0)
        if n < 0:
            raise VitsError(last_error())
        if n == 0:
            return None
        out = np.zeros((n // 4, 4), np.int64)
        if lib().vits_model_last_joins(self._h, _ptr(out), out.size) != n:
            raise VitsError(last_error())
        return out

    def prepare_conversion(self):
        """vits_model_prepare_conversion: build the posterior encoder and the forward-flow weights now (the first conversion does it otherwise)"""
        if lib().vits_model_prepare_conversion(self._h) != 0:
            raise VitsError(last_error())

    def convert_batch(self, pcm, lengths=None, src=-1, tgt=-1, mode=MODE_DEFAULT, noise_kind=NOISE_COUNTER, noise_seed=4321, noise_prior=None,
                      collect_taps=False, out_device=None, out_device_stride=0, skip_host_copy=False, vocoder_chunk_frames=0, on_chunk=None,
                      noise_seed_offsets=None, keep_pcm=True, vc_rate=None, vc_pitch=None, **refused):
        """Voice conversion (vits_model_convert_batch). pcm: float32 [B, stride] (or one 1-D utterance) at the model's sampling rate; lengths:
        valid samples per row (None = the whole row); src / tgt: the source and target speaker, one int for every utterance or one per
        utterance (-1 = none). Returns (list of per-utterance PCM arrays or None, lengths, frames) like process_batch. Keyword arguments
        that conversion refuses (fixed_duration, frames_only, async_, speaker_ids, and the prosody arguments of process_batch) are passed on, so that
        the library says why. The model-level prosody (speaking_rate, noise_scale, noise_scale_duration) does not affect a conversion. vc_rate / vc_pitch:
        a scalar or one value per utterance in [0.5, 2] (None = the model value, set_conversion_prosody): the converted audio is time-stretched to that rate
        and shifted to that pitch on the device."""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        if pcm.ndim == 1:
            pcm = pcm[None, :]
        B, stride = pcm.shape
        lens = np.full(B, stride, np.int64) if lengths is None else np.ascontiguousarray(lengths, dtype=np.int64).ravel()
        if lens.size != B:
            raise ValueError("lengths needs one entry per utterance")
        sp = [np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.int32), (B,))) for v in (src, tgt)]
        pitch_ratio = refused.pop("pitch_ratio", None)
        fit = refused.pop("fit", None)
        fields, keep = _refused_fields(refused, B)
        o, kept = _opts(B, mode, noise_kind, noise_seed, noise_prior=noise_prior, collect_taps=collect_taps, out_device=out_device,
                        out_device_stride=out_device_stride, skip_host_copy=skip_host_copy, vocoder_chunk_frames=vocoder_chunk_frames,
                        noise_seed_offsets=noise_seed_offsets)
        keep += kept
        for field, v in fields.items():
            setattr(o, field, v)
        cb_error = _chunk_sink(o, on_chunk)
        res = BatchResult()
        call = lambda: lib().vits_model_convert_batch(self._h, _ptr(pcm), _ptr(lens), B, stride, _ptr(sp[0]), _ptr(sp[1]), C.byref(o), C.byref(res))
        if self._with_fit(fit, lambda: self._with_conversion_ratios(vc_rate, vc_pitch, B, lambda: self._with_pitch(pitch_ratio, B, call))) != 0:
            if cb_error:
                raise cb_error[0]
            raise VitsError(last_error())
        return _take_result(res, B, keep_pcm)

    def convert(self, pcm, src=-1, tgt=-1, vc_rate=None, vc_pitch=None):
        """vits_model_convert: one utterance, the model's default mode and the reference noise stream (like process); vc_rate / vc_pitch as in convert_batch"""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32).ravel()
        r = self._with_conversion_ratios(vc_rate, vc_pitch, 1, lambda: lib().vits_model_convert(self._h, _ptr(pcm), pcm.size, int(src), int(tgt)))
        if not r.data:
            raise VitsError(last_error())
        try:
            return np.ctypeslib.as_array(r.data, shape=(r.size,)).copy()
        finally:
            lib().vits_free_result(r)

    def align_batch(self, pcm, ids, lengths=None, id_lengths=None, speakers=-1, noise_scale=0.0, mode=MODE_DEFAULT, noise_kind=NOISE_COUNTER,
                    noise_seed=4321, noise_prior=None, collect_taps=False, noise_seed_offsets=None, **refused):
        """Forced alignment (vits_model_align_batch): which frames of each recording belong to which token of its transcript, by VITS's monotonic
        alignment search. pcm: float32 [B, stride] (or one 1-D utterance), lengths: valid samples per row; ids: int32 [B, id_stride] (or 1-D),
        id_lengths: tokens per row; speakers: the speaker of the recordings, one int or one per utterance (-1 = none); noise_scale: scale of the
        posterior draw (0 = the posterior mean, deterministic; 1 = VITS's training draw). Returns (durations int32 [B, id_stride]: frames per token,
        0 past id_lengths[b]; frames int64 [B]; scores float32 [B]: log-likelihood of the best path). durations is what process_batch takes as
        duration_override. Keyword arguments the call refuses (those of convert_batch, and out_device, skip_host_copy, vocoder_chunk_frames) are
        passed on, so that the library says why."""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        if pcm.ndim == 1:
            pcm = pcm[None, :]
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        if ids.ndim == 1:
            ids = ids[None, :]
        B, stride = pcm.shape
        if ids.shape[0] != B:
            raise ValueError("pcm and ids need one row per utterance each")
        id_stride = ids.shape[1]
        lens = np.full(B, stride, np.int64) if lengths is None else np.ascontiguousarray(lengths, dtype=np.int64).ravel()
        ilens = np.full(B, id_stride, np.int32) if id_lengths is None else np.ascontiguousarray(id_lengths, dtype=np.int32).ravel()
        if lens.size != B or ilens.size != B:
            raise ValueError("lengths and id_lengths need one entry per utterance")
        sp = np.ascontiguousarray(np.broadcast_to(np.asarray(speakers, np.int32), (B,)))
        own = {k: refused.pop(k) for k in ("out_device", "skip_host_copy", "vocoder_chunk_frames") if k in refused}
        on_chunk = refused.pop("on_chunk", None)
        pitch_ratio = refused.pop("pitch_ratio", None)
        fit = refused.pop("fit", None)
        fields, keep = _refused_fields(refused, B, noise_scale_arg="noise_scales")
        o, kept = _opts(B, mode, noise_kind, noise_seed, noise_prior=noise_prior, collect_taps=collect_taps, noise_seed_offsets=noise_seed_offsets, **own)
        keep += kept
        for field, v in fields.items():
            setattr(o, field, v)
        if on_chunk is not None:
            o.on_chunk = ChunkCallback(lambda _user, utt, offset, p, n: 1)  # (refused before anything could call it)
        durations = np.zeros((B, id_stride), np.int32)
        frames = np.zeros(B, np.int64)
        scores = np.zeros(B, np.float32)
        call = lambda: lib().vits_model_align_batch(self._h, _ptr(pcm), _ptr(lens), B, stride, _ptr(ids), _ptr(ilens), id_stride, _ptr(sp), float(noise_scale),
                                                    C.byref(o), _ptr(durations), _ptr(frames), _ptr(scores))
        if self._with_fit(fit, lambda: self._with_pitch(pitch_ratio, B, call)) != 0:
            raise VitsError(last_error())
        return durations, frames, scores

    def align(self, pcm, text, speaker=-1):
        """vits_model_align: one utterance from text through the model's tokenizer, the posterior mean. Returns (ids, durations)."""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32).ravel()
        raw = text.encode() if isinstance(text, str) else bytes(text)
        cap = 2 * len(raw) + 8
        ids = np.zeros(cap, np.int32)
        durations = np.zeros(cap, np.int32)
        n = lib().vits_model_align(self._h, _ptr(pcm), pcm.size, raw, int(speaker), _ptr(ids), _ptr(durations), cap)
        if n < 0:
            raise VitsError(last_error())
        if n > cap:  # (cannot happen with a tokenizer that emits at most one id and one blank per byte; ask again rather than truncate)
            cap = int(n)
            ids = np.zeros(cap, np.int32)
            durations = np.zeros(cap, np.int32)
            n = lib().vits_model_align(self._h, _ptr(pcm), pcm.size, raw, int(speaker), _ptr(ids), _ptr(durations), cap)
            if n < 0:
                raise VitsError(last_error())
        return ids[:n].copy(), durations[:n].copy()

    @property
    def hop(self):
        """samples per frame (vits_model_hop)"""
        return int(lib().vits_model_hop(self._h))

    def submit_batch(self, ids, id_lengths=None, mode=MODE_DEFAULT, noise_seed=4321, fixed_duration=0, out_device=None, out_device_stride=0,
                     skip_host_copy=False, vocoder_chunk_frames=0, noise_seed_offsets=None, speaker_ids=None, speaking_rate=None, noise_scale=None,
                     noise_scale_duration=None, duration_override=None, durations_out=None, pitch_ratio=None, fit=None):
        """vits_model_submit_batch: queue one batch on this handle's pipeline (at most two in flight); its stage one runs under the
        previous batch's vocoder. Results come from wait(), in submission order, bit-identical to process_batch. The prosody arguments are
        those of process_batch; durations_out is filled by the matching wait() at the latest (this handle keeps it alive until then)."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        if ids.ndim == 1:
            ids = ids[None, :]
        B, stride = ids.shape
        lens = np.full(B, stride, np.int32) if id_lengths is None else np.ascontiguousarray(id_lengths, dtype=np.int32)
        o, keep = _opts(B, mode, NOISE_COUNTER, noise_seed, fixed_duration=fixed_duration, out_device=out_device, out_device_stride=out_device_stride,
                        skip_host_copy=skip_host_copy, vocoder_chunk_frames=vocoder_chunk_frames, noise_seed_offsets=noise_seed_offsets, speaker_ids=speaker_ids)
        keep += _prosody(o, B, stride, speaking_rate, noise_scale, noise_scale_duration, duration_override, durations_out)
        call = lambda: lib().vits_model_submit_batch(self._h, _ptr(ids), _ptr(lens), B, stride, C.byref(o))
        if self._with_fit(fit, lambda: self._with_pitch(pitch_ratio, B, call)) != 0:
            raise VitsError(last_error())
        if not hasattr(self, "_durations_in_flight"):
            self._durations_in_flight = []
        self._durations_in_flight.append(durations_out)  # (the library writes it no later than the matching wait)

    def wait(self, keep_pcm=True):
        """vits_model_wait: (pcm list or None, lengths, frames) of the oldest submitted batch."""
        res = BatchResult()
        if lib().vits_model_wait(self._h, C.byref(res)) != 0:
            raise VitsError(last_error())
        if getattr(self, "_durations_in_flight", None):
            self._durations_in_flight.pop(0)
        return _take_result(res, res.batch, keep_pcm)

    @property
    def pending(self):
        return lib().vits_model_pending(self._h)

    def sync(self):
        if lib().vits_model_sync(self._h) != 0:
            raise VitsError(last_error())

    def tap(self, name, utt=0):
        n = lib().vits_model_get_tap(self._h, name.encode(), utt, None, 0)
        if n <= 0:
            raise VitsError(f"no tap '{name}': {last_error()}")
        out = np.zeros(n, np.float32)
        lib().vits_model_get_tap(self._h, name.encode(), utt, _ptr(out), n)
        return out

    def prof_enable(self, on=True):
        lib().vits_prof_enable(self._h, int(on))

    def prof_reset(self):
        lib().vits_prof_reset(self._h)

    def prof_report(self):
        buf = C.create_string_buffer(1 << 20)
        n = lib().vits_prof_report(self._h, buf, len(buf))
        if n < 0:
            raise VitsError(last_error())
        return json.loads(buf.value.decode())


def durations_to_seconds(durations, model):
    """Start and end of every token in seconds from an alignment's durations (frames per token; 1-D, or [B, T] row by row): cumulative frames
    x hop / sampling rate. Returns (starts, ends), float64, shaped like durations."""
    d = np.asarray(durations, np.int64)
    ends = np.cumsum(d, axis=-1)
    scale = model.hop / float(model.sampling_rate)
    return (ends - d) * scale, ends * scale


# ---- operator-level wrappers (parity tests) ----------------------------------------------------------
def op_set_arith(arith):
    """Arithmetic of op_conv1d / op_conv_transpose1d / op_resblock_pair on this thread (ARITH_F32 | ARITH_BF16 | ARITH_F16 | ARITH_F32_SPLIT: the split
    kernels or a VitsError that names the cause, never another kernel — include/vits.h vits_op_set_arith)."""
    f = lib().vits_op_set_arith
    f.restype, f.argtypes = C.c_int32, [C.c_int32]
    if f(arith) != 0:
        raise VitsError(last_error())


def op_tile_map_launches():
    """Launches of this process that ran over a list of existing tiles instead of their dense grid (vits_op_tile_map_launches; ragged batches under
    VITS_TILE_MAP / by default on large grids). For tests: results never depend on it."""
    f = lib().vits_op_tile_map_launches
    f.restype, f.argtypes = C.c_uint64, []
    return int(f())


def op_set_output_fill(byte):
    """0 (default) or 0xFF: what the outputs of op_conv1d / op_conv_transpose1d / op_resblock_pair / op_resblock hold before the kernels run, on this thread
    (vits_op_set_output_fill; 0xFF = fp32 NaN, so that a stray store of ANY value behind an utterance's end shows)."""
    f = lib().vits_op_set_output_fill
    f.restype, f.argtypes = C.c_int32, [C.c_int32]
    if f(int(byte)) != 0:
        raise VitsError(last_error())


def op_conv_group(x, ws, biases, dilation, slope, lens=None):
    """The grouped launch of two or three same-position ResBlock convolutions (vits_op_conv_group): x [n, B, C, T]; ws a list of n weights [C, C, k_i] with
    k_i in {11, 7, 3}; biases [n, C] or None. Returns y [n, B, C, T], NaN (0xFF bytes) where no kernel wrote."""
    x = _f32(x)
    n, B, ch, T = x.shape
    assert len(ws) == n and all(w.shape[:2] == (ch, ch) for w in ws)
    w = np.concatenate([_f32(w).ravel() for w in ws])
    d = ConvGroupDesc(B, ch, T, T, n, (C.c_int32 * 3)(*([int(w.shape[2]) for w in ws] + [0, 0, 0])[:3]), dilation, slope)
    y = np.empty((n, B, ch, T), np.float32)
    biases = _f32(biases)
    lens = None if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
    f = lib().vits_op_conv_group
    f.restype, f.argtypes = C.c_int32, [C.POINTER(ConvGroupDesc)] + [C.c_void_p] * 5
    if f(C.byref(d), _ptr(x), _ptr(w), _ptr(biases), _ptr(lens), _ptr(y)) != 0:
        raise VitsError(last_error())
    return y


def op_conv1d(x, w, bias=None, dilation=1, pad_left=None, pre_slope=None, post_act=0, residual=None, accum=None,
              out_scale=1.0, lens=None):
    x, w = _f32(x), _f32(w)
    B, cin, T = x.shape
    cout, _, k = w.shape
    d = Conv1dDesc(B, cin, cout, T, T, k, dilation, (k - 1) * dilation // 2 if pad_left is None else pad_left,
                   0 if pre_slope is None else 1, 0.0 if pre_slope is None else pre_slope, post_act, out_scale)
    cy = cout // 2 if post_act == 2 else cout
    y = np.zeros((B, cy, T), np.float32)
    bias, residual, accum = _f32(bias), _f32(residual), _f32(accum)
    lens = None if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
    if lib().vits_op_conv1d(C.byref(d), _ptr(x), _ptr(w), _ptr(bias), _ptr(residual), _ptr(accum), _ptr(lens), _ptr(y)) != 0:
        raise VitsError(last_error())
    return y


def op_resblock_pair(x, w1, b1, w2, b2, dilation, slope, lens=None):
    """y = x + b2 + conv2(leaky_relu(b1 + conv1(leaky_relu(x)))), conv1 at `dilation`, conv2 at dilation 1 (vits_op_resblock_pair): two fp32 convs, or in
    ARITH_F32_SPLIT the engine's un-fused split ResBlock sequence (conv1 writes only the three planes conv2 reads)."""
    x, w1, w2, b1, b2 = _f32(x), _f32(w1), _f32(w2), _f32(b1), _f32(b2)
    B, ch, T = x.shape
    k = w1.shape[2]
    assert w1.shape == (ch, ch, k) and w2.shape == (ch, ch, k)
    d = ResblockPairDesc(B, ch, T, T, k, dilation, slope)
    y = np.zeros((B, ch, T), np.float32)
    lens = None if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
    if lib().vits_op_resblock_pair(C.byref(d), _ptr(x), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(lens), _ptr(y)) != 0:
        raise VitsError(last_error())
    return y


def _resblock_desc(B, ch, T, ts, k, dils, slope, out_scale, scale_div, variant, tiles, nr):
    dils = [int(v) for v in dils]
    return ResblockDesc(B, ch, T, ts, k, len(dils), (C.c_int32 * 3)(*(dils + [0] * 3)[:3]), slope, out_scale, int(scale_div), variant, tiles, nr)


def op_resblock_plan(channels, k, dils, t, batch=1, variant=RB_VARIANT_PLAN, tiles=0, nr=0):
    """What op_resblock would launch in the arithmetic of op_set_arith (vits_op_resblock_plan; host arithmetic, no GPU needed): a dict with kernel, variant (the
    one that runs), bo, advance, halo, segment, tiles, nr, grid, block, lds, launches — or a VitsError naming the cause of the refusal."""
    d = _resblock_desc(batch, channels, t, t, k, dils, 0.1, 1.0, 0, variant, tiles, nr)
    p = ResblockPlan()
    if lib().vits_op_resblock_plan(C.byref(d), C.byref(p)) != 0:
        raise VitsError(last_error())
    out = {n: getattr(p, n) for n in ("variant", "bo", "advance", "halo", "segment", "tiles", "nr", "block", "lds", "launches")}
    out["kernel"] = p.kernel.decode()
    out["grid"] = (p.grid_x, p.grid_y, p.grid_z)
    return out


def op_resblock(x, w1, b1, w2, b2, dils, slope, variant=RB_VARIANT_PLAN, tiles=0, nr=0, accum=None, out_scale=1.0, scale_div=False, lens=None, t=None):
    """One HiFiGAN ResBlock through the kernel `variant` names (vits_op_resblock): x [B, C, t_stride]; w1, w2 [ndil, C, C, k]; b1, b2 [ndil, C]; dils the
    dilations of the first convs; accum [B, C, t_stride] or None: out = (accum + y) * out_scale (scale_div: / out_scale); t = the longest utterance (default:
    t_stride). RB_VARIANT_UNFUSED | _PAIRS | _BLOCK | _SEGMENTS run that kernel or raise a VitsError naming the cause: never another one. Returns [B, C, t_stride],
    zero where nothing was written."""
    x, w1, w2, b1, b2, accum = _f32(x), _f32(w1), _f32(w2), _f32(b1), _f32(b2), _f32(accum)
    B, ch, ts = x.shape
    nd, _, _, k = w1.shape
    assert w1.shape == w2.shape == (nd, ch, ch, k) and b1.shape == b2.shape == (nd, ch) and len(dils) == nd
    assert accum is None or accum.shape == x.shape
    d = _resblock_desc(B, ch, ts if t is None else t, ts, k, dils, slope, out_scale, scale_div, variant, tiles, nr)
    y = np.zeros((B, ch, ts), np.float32)
    lens = None if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
    if lib().vits_op_resblock(C.byref(d), _ptr(x), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(accum), _ptr(lens), _ptr(y)) != 0:
        raise VitsError(last_error())
    return y


def op_flow_coupling_plan(t, batch=1, hidden=192, half=96, k=5, layers=4, rate=1, variant=FLOW_VARIANT_PLAN, ncw=0, nct=0):
    """What op_flow_coupling would launch in the arithmetic of op_set_arith (vits_op_flow_coupling_plan; host arithmetic, no GPU needed): a dict with kernel,
    variant (the one that runs), bo, halo, ncw, nct, grid, block, lds, launches — or a VitsError naming the cause of the refusal."""
    d = FlowCouplingDesc(batch, hidden, half, t, t, k, layers, rate, 0, 1, variant, ncw, nct)
    p = FlowCouplingPlan()
    if lib().vits_op_flow_coupling_plan(C.byref(d), C.byref(p)) != 0:
        raise VitsError(last_error())
    out = {n: getattr(p, n) for n in ("variant", "bo", "halo", "ncw", "nct", "block", "lds", "launches")}
    out["kernel"] = p.kernel.decode()
    out["grid"] = (p.grid_x, p.grid_y, p.grid_z)
    return out


def op_flow_coupling(z, w_pre, b_pre, w_in, b_in, w_rs, b_rs, w_post, b_post, flipped=0, rate=1, variant=FLOW_VARIANT_PLAN, ncw=0, nct=0, bias_rows=None,
                     lens=None, t=None):
    """One residual-coupling layer of the flow through the kernel `variant` names (vits_op_flow_coupling): z [B, 2 half, t_stride] (flipped 0: x0 = the first
    half of the channels, x1 the second; 1: the other way round); w_pre [H, half, 1]; w_in [layers, 2H, H, k]; w_rs / b_rs: a list of the layers' arrays
    ([2H, H, 1] / [2H], the last [H, H, 1] / [H]) or their concatenation; w_post [half, H, 1] as launched (reverse direction: negated, with b_post);
    b_in [rows, layers, 2H] (or [layers, 2H]); bias_rows [B] or None (row 0); t = the longest utterance (default: t_stride). FLOW_VARIANT_UNFUSED | _WAVENET |
    _COUPLING run that kernel or raise a VitsError naming the cause: never another one. Returns the new z: x1 updated on the valid columns, the staged NaN
    (all bits set) behind lens[b] up to t, the input's values from t on."""
    cat = lambda a: _f32(np.concatenate([np.asarray(v, np.float32).ravel() for v in a]) if isinstance(a, (list, tuple)) else a)
    z, w_pre, b_pre, w_in, b_in, w_post, b_post = _f32(z), _f32(w_pre), _f32(b_pre), _f32(w_in), _f32(b_in), _f32(w_post), _f32(b_post)
    w_rs, b_rs = cat(w_rs), cat(b_rs)
    B, F, ts = z.shape
    half = F // 2
    layers, H2, H, k = w_in.shape
    if b_in.ndim == 2:
        b_in = b_in[None]
    assert F == 2 * half and H2 == 2 * H and w_pre.shape == (H, half, 1) and w_post.shape == (half, H, 1) and b_pre.shape == (H,) and b_post.shape == (half,)
    assert b_in.shape[1:] == (layers, 2 * H) and w_rs.size == (2 * layers - 1) * H * H and b_rs.size == (2 * layers - 1) * H
    d = FlowCouplingDesc(B, H, half, ts if t is None else t, ts, k, layers, rate, int(flipped), b_in.shape[0], variant, ncw, nct)
    out = z.copy()
    lens = None if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
    bias_rows = None if bias_rows is None else np.ascontiguousarray(bias_rows, dtype=np.int32)
    assert (lens is None or lens.shape == (B,)) and (bias_rows is None or bias_rows.shape == (B,))
    if lib().vits_op_flow_coupling(C.byref(d), _ptr(out), _ptr(w_pre), _ptr(b_pre), _ptr(w_in), _ptr(b_in), _ptr(w_rs), _ptr(b_rs), _ptr(w_post), _ptr(b_post),
                                   _ptr(bias_rows), _ptr(lens)) != 0:
        raise VitsError(last_error())
    return out


def op_duration_predictor(x, w1, b1, g1, be1, w2, b2, g2, be2, wp, bp, spk_rows=None, lens=None, eps=1e-5, variant=DP_VARIANT_PLAN, t=None):
    """The deterministic duration predictor on caller-supplied tensors (vits_op_duration_predictor): x [B, H, t_stride], w1 [Fc, H, k], w2 [Fc, Fc, k],
    wp [1, Fc, 1], spk_rows [B, H] or None, lens [B] or None, t = the longest utterance (default: t_stride). variant: DP_VARIANT_PLAN | _LAT | _WIDE (the fused
    kernel's tiles, or a VitsError: never another path) | _UNFUSED. Returns logw [B, t_stride], zeros where nothing was written."""
    x, w1, w2, wp = _f32(x), _f32(w1), _f32(w2), _f32(wp)
    B, H, ts = x.shape
    Fc, _, k = w1.shape
    assert w1.shape == (Fc, H, k) and w2.shape == (Fc, Fc, k) and wp.size == Fc
    vec = [_f32(v).reshape(-1) for v in (b1, g1, be1, b2, g2, be2)]
    assert all(v.size == Fc for v in vec)
    b1, g1, be1, b2, g2, be2 = vec
    bp = _f32(bp).reshape(-1)
    spk_rows = None if spk_rows is None else _f32(spk_rows).reshape(B, H)
    lens = None if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
    d = DurationPredictorDesc(B, H, Fc, ts if t is None else t, ts, k, eps, variant)
    y = np.zeros((B, ts), np.float32)
    if lib().vits_op_duration_predictor(C.byref(d), _ptr(x), _ptr(w1), _ptr(b1), _ptr(g1), _ptr(be1), _ptr(w2), _ptr(b2), _ptr(g2), _ptr(be2), _ptr(wp), _ptr(bp),
                                        _ptr(spk_rows), _ptr(lens), _ptr(y)) != 0:
        raise VitsError(last_error())
    return y


def op_dds_block_plan(channels, k, layers, t, batch=1, variant=DDS_VARIANT_PLAN, head=DDS_HEAD_NONE, tail_rows=0):
    """What op_dds_block would launch in the arithmetic of op_set_arith (vits_op_dds_block_plan; host arithmetic, no GPU needed): a dict with kernel and
    kernel_last (the first and the last layer's instantiation), variant (the one that runs), nt (tokens per block), halo and lds (per layer), grid, block,
    launches — or a VitsError naming the cause of the refusal."""
    d = DdsBlockDesc(batch, channels, t, t, k, layers, 1e-5, variant, head, 1 if tail_rows else 0, tail_rows, 0, 1)
    p = DdsBlockPlan()
    if lib().vits_op_dds_block_plan(C.byref(d), C.byref(p)) != 0:
        raise VitsError(last_error())
    out = {n: getattr(p, n) for n in ("variant", "nt", "block", "launches")}
    out["kernel"], out["kernel_last"] = p.kernel.decode(), p.kernel_last.decode()
    out["halo"], out["lds"] = list(p.halo[:p.layers]), list(p.lds[:p.layers])
    out["grid"] = (p.grid_x, p.grid_y)
    return out


def op_dds_block(dw_w, dw_b, g1, b1, pw_w, pw_b, g2, b2, x=None, z=None, cond=None, zc=0, head_w=None, head_b=None, bias_rows=None, tail_w=None, tail_b=None,
                 lens=None, t=None, eps=1e-5, variant=DDS_VARIANT_PLAN):
    """One DDS block through the kernels `variant` names (vits_op_dds_block): dw_w [layers, H, k]; dw_b, g1, b1, pw_b, g2, b2 [layers, H]; pw_w [layers, H, H].
    Input: x [B, H, t_stride] (no head), or z [B, 2, t_stride] + cond [B, H, t_stride] + head_w [H] + head_b [H] (the 1 -> H conv of latent row zc plus
    conditioning), or x + head_w [H, H] + head_b [rows, H] (or [H]) + bias_rows [B] or None (an H -> H 1x1 conv in front). tail_w [R, H] + tail_b [R]: the 1x1
    projection behind the block. t = the longest utterance (default: t_stride). DDS_VARIANT_UNFUSED | _LAYER | _LAT run those kernels or raise a VitsError
    naming the cause: never others. Returns (y [B, H, t_stride], y2 [B, R, t_stride] or None) as the device holds them: the staged NaN (all bits set) wherever
    nothing was written."""
    dw_w, pw_w = _f32(dw_w), _f32(pw_w)
    layers, H, k = dw_w.shape
    vec = [_f32(v).reshape(layers, H) for v in (dw_b, g1, b1, pw_b, g2, b2)]
    assert pw_w.shape[:3] == (layers, H, H) and pw_w.size == layers * H * H
    x, z, cond, head_w, head_b, tail_w, tail_b = _f32(x), _f32(z), _f32(cond), _f32(head_w), _f32(head_b), _f32(tail_w), _f32(tail_b)
    if z is not None:
        head, (B, _, ts), rows = DDS_HEAD_FROM1, z.shape, 1
        assert x is None and z.shape[1] == 2 and cond.shape == (B, H, ts) and head_w.size == H and head_b.size == H
    else:
        B, _, ts = x.shape
        assert x.shape[1] == H
        head, rows = (DDS_HEAD_CONV, 1) if head_w is not None else (DDS_HEAD_NONE, 1)
        if head:
            head_b = head_b.reshape(-1, H)
            rows = head_b.shape[0]
            assert head_w.size == H * H
    R = 0
    if tail_w is not None:
        R = tail_b.size
        assert tail_w.size == R * H
    d = DdsBlockDesc(B, H, ts if t is None else t, ts, k, layers, eps, variant, head, 1 if R else 0, R, zc, rows)
    y = np.zeros((B, H, ts), np.float32)
    y2 = np.zeros((B, R, ts), np.float32) if R else None
    lens = None if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
    bias_rows = None if bias_rows is None else np.ascontiguousarray(bias_rows, dtype=np.int32)
    assert (lens is None or lens.shape == (B,)) and (bias_rows is None or bias_rows.shape == (B,))
    if lib().vits_op_dds_block(C.byref(d), _ptr(x), _ptr(z), _ptr(cond), _ptr(head_w), _ptr(head_b), _ptr(bias_rows), _ptr(dw_w), *[_ptr(v) for v in vec[:3]],
                               _ptr(pw_w), *[_ptr(v) for v in vec[3:]], _ptr(tail_w), _ptr(tail_b), _ptr(lens), _ptr(y), _ptr(y2)) != 0:
        raise VitsError(last_error())
    return y, y2


def op_spline(u, z, zc, bins, tail, inv_sqrt, mode, lens=None, t=None):
    """The inverse rational-quadratic spline of a conv flow on caller-supplied tensors (vits_op_spline): u [B, 3 bins - 1, t_stride], z [B, 2, t_stride]; row zc
    of z is transformed on [0, lens[b]) in MODE_HF or MODE_REFERENCE semantics. Returns the new z (every other bit as given)."""
    u, z = _f32(u), _f32(z)
    B, rows, ts = u.shape
    assert rows == 3 * bins - 1 and z.shape == (B, 2, ts)
    out = z.copy()
    lens = None if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
    if lib().vits_op_spline(B, ts if t is None else t, ts, bins, tail, inv_sqrt, mode, zc, _ptr(u), _ptr(out), _ptr(lens)) != 0:
        raise VitsError(last_error())
    return out


def op_durations(logw, row, lens, length_scale=1.0, length_scales=None, overrides=None, fixed=0, stage_mul=(), stage_add=()):
    """The durations kernel on caller-supplied log-durations (vits_op_durations): logw [B, rows, t_stride], row `row` is read. Returns (dur float32 [B, t_stride],
    cum int32 [B, t_stride], frames int32 [B], stage_lens int32 [n_stage, B])."""
    logw = _f32(logw)
    B, rows, ts = logw.shape
    lens = None if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
    length_scales = None if length_scales is None else _f32(length_scales).reshape(B)
    overrides = None if overrides is None else np.ascontiguousarray(overrides, dtype=np.int32).reshape(B, ts)
    mul, add = np.ascontiguousarray(stage_mul, dtype=np.int32), np.ascontiguousarray(stage_add, dtype=np.int32)
    assert mul.shape == add.shape and mul.ndim == 1
    dur, cum = np.zeros((B, ts), np.float32), np.zeros((B, ts), np.int32)
    frames, sl = np.zeros(B, np.int32), np.zeros((mul.size, B), np.int32)
    if lib().vits_op_durations(B, rows, row, ts, _ptr(logw), _ptr(lens), length_scale, _ptr(length_scales), _ptr(overrides), fixed, mul.size,
                               _ptr(mul) if mul.size else None, _ptr(add) if mul.size else None, _ptr(dur), _ptr(cum), _ptr(frames), _ptr(sl) if mul.size else None) != 0:
        raise VitsError(last_error())
    return dur, cum, frames, sl


def _fit_args(B, ts, lens, fixed, groups, targets):
    lens = None if lens is None else np.ascontiguousarray(lens, dtype=np.int32).reshape(B)
    fixed = None if fixed is None else np.ascontiguousarray(fixed, dtype=np.int32).reshape(B, ts)
    groups = None if groups is None else np.ascontiguousarray(groups, dtype=np.int32).reshape(B)
    targets = np.ascontiguousarray(targets, dtype=np.int64).reshape(B)
    return lens, fixed, groups, targets


def fit_host(e, targets, lens=None, fixed=None, groups=None, min_rate=0.1, max_rate=10.0):
    """vits_fit_host: the fit's definition on the host (no device). e: float32 [B, t_stride] = expf(logw); targets: int64 [B] by group (0: not fitted); lens,
    fixed (int32 [B, t_stride], -1: a free token), groups (int32 [B]) optional. Returns (dur int32 [B, t_stride], rows float64 [B, 5] = (F, sum d, s*, R,
    status) by group)."""
    e = _f32(e)
    B, ts = e.shape
    lens, fixed, groups, targets = _fit_args(B, ts, lens, fixed, groups, targets)
    dur, rows = np.zeros((B, ts), np.int32), np.zeros((B, 5), np.float64)
    if lib().vits_fit_host(B, ts, _ptr(e), _ptr(fixed), _ptr(lens), _ptr(groups), _ptr(targets), float(min_rate), float(max_rate), _ptr(dur), _ptr(rows)) != 0:
        raise VitsError(last_error())
    return dur, rows


def op_fit_durations(logw, row, targets, lens=None, fixed=None, groups=None, min_rate=0.1, max_rate=10.0):
    """The fit kernel on caller-supplied log-durations (vits_op_fit_durations): logw [B, rows, t_stride], row `row` is read. Returns (e float32 [B, t_stride],
    dur int32 [B, t_stride], rows float64 [B, 5]) as fit_host gives them."""
    logw = _f32(logw)
    B, rows_, ts = logw.shape
    lens, fixed, groups, targets = _fit_args(B, ts, lens, fixed, groups, targets)
    e, dur, rows = np.zeros((B, ts), np.float32), np.zeros((B, ts), np.int32), np.zeros((B, 5), np.float64)
    if lib().vits_op_fit_durations(B, rows_, row, ts, _ptr(logw), _ptr(lens), _ptr(fixed), _ptr(groups), _ptr(targets), float(min_rate), float(max_rate), _ptr(e),
                                   _ptr(dur), _ptr(rows)) != 0:
        raise VitsError(last_error())
    return e, dur, rows


def op_conv_transpose1d(x, w, bias, stride, crop, pre_slope=1.0, lens=None):
    x, w, bias = _f32(x), _f32(w), _f32(bias)
    B, cin, T = x.shape
    _, cout, k = w.shape
    To = stride * T + k - stride - 2 * crop
    d = ConvT1dDesc(B, cin, cout, T, T, To, k, stride, crop, pre_slope)
    y = np.zeros((B, cout, To), np.float32)
    lens = None if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
    if lib().vits_op_conv_transpose1d(C.byref(d), _ptr(x), _ptr(w), _ptr(bias), _ptr(lens), _ptr(y)) != 0:
        raise VitsError(last_error())
    return y


def op_upsample16_plan(cin, cout, stride, t, batch=1, crop=0, variant=UP16_VARIANT_PLAN, split=0):
    """What op_upsample16 would launch in the arithmetic of op_set_arith (vits_op_upsample16_plan; host arithmetic, no GPU needed): a dict with kernel (the
    instantiation as rocprofv3 prints it), tag (convt16_stream_tag), variant (the one that runs), bn (input positions per block), grid, block, lds — or a
    VitsError naming the cause of the refusal."""
    t_out = stride * t + stride - 2 * crop
    d = Upsample16Desc(batch, cin, cout, t, t, t_out, stride, crop, 0.1, 0.1, variant, split)
    p = Upsample16Plan()
    if lib().vits_op_upsample16_plan(C.byref(d), C.byref(p)) != 0:
        raise VitsError(last_error())
    out = {n: getattr(p, n) for n in ("variant", "bn", "block", "lds")}
    out["kernel"], out["tag"] = p.kernel.decode(), p.tag.decode()
    out["grid"] = (p.grid_x, p.grid_y, p.grid_z)
    return out


def op_upsample16(x, w, bias, stride, crop, pre_slope=0.1, y16_slope=0.1, variant=UP16_VARIANT_PLAN, split=0, lens=None, want_y16=True, want_x16=False, t=None,
                  t_out_stride=None):
    """One HiFiGAN upsampler of the 16-bit modes in the group layout through the kernel `variant` names (vits_op_upsample16): x [B, cin, t_stride]; w [cin, cout,
    2 stride]; bias [cout] or None; t = the longest utterance (default: t_stride); t_out_stride = row pitch of the outputs (default: t_out = stride t + stride -
    2 crop). UP16_VARIANT_TILE | _STREAM run that kernel or raise a VitsError naming the cause: never another one; split 1 / 2 / 4 forces the lines kernels' deal
    over gridDim.z. Returns a dict: y fp32 [B, cout, t_out_stride]; y16 (want_y16) and x16 (want_x16) as uint16 bit patterns [B, cout, t_out_stride] /
    [B, cin, t_stride]. What was not written back is zero in y / y16 and 0xFFFF in x16. want_y16=False gives the kernel no 16-bit destination."""
    x, w, bias = _f32(x), _f32(w), _f32(bias)
    B, cin, ts = x.shape
    T = ts if t is None else t
    if w.ndim != 3 or w.shape[0] != cin or w.shape[2] != 2 * stride:
        raise VitsError("vits_op_upsample16: w %s is not [c_in = %d][c_out][2 x stride = %d]: the descriptor has no kernel-size field, k = 2 x stride only"
                        % (list(w.shape), cin, 2 * stride))
    cout = w.shape[1]
    t_out = stride * T + stride - 2 * crop
    tos = t_out if t_out_stride is None else t_out_stride
    assert bias is None or bias.shape == (cout,)
    d = Upsample16Desc(B, cin, cout, T, ts, tos, stride, crop, pre_slope, y16_slope, variant, split)
    y = np.zeros((B, cout, max(tos, 0)), np.float32)
    y16 = np.zeros((B, cout, max(tos, 0)), np.uint16) if want_y16 else None
    x16 = np.full((B, cin, ts), 0xFFFF, np.uint16) if want_x16 else None
    lens = None if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
    assert lens is None or lens.shape == (B,)
    if lib().vits_op_upsample16(C.byref(d), _ptr(x), _ptr(w), _ptr(bias), _ptr(lens), _ptr(y), _ptr(y16), _ptr(x16)) != 0:
        raise VitsError(last_error())
    out = {"y": y}
    if want_y16:
        out["y16"] = y16
    if want_x16:
        out["x16"] = x16
    return out


def op_align(m, ls, z, T=None, L=None):
    """align_logp + align_mas on caller-supplied statistics (vits_op_align). m, ls: [B, F, Tmax]; z: [B, F, Lmax]; T, L: per-utterance token /
    frame counts (None = the whole rows). Returns (durations int32 [B, Tmax], scores float32 [B])."""
    m, ls, z = (np.ascontiguousarray(a, dtype=np.float32) for a in (m, ls, z))
    B, F, tmax = m.shape
    lmax = z.shape[2]
    T = np.full(B, tmax, np.int32) if T is None else np.ascontiguousarray(T, dtype=np.int32)
    L = np.full(B, lmax, np.int32) if L is None else np.ascontiguousarray(L, dtype=np.int32)
    if ls.shape != m.shape or z.shape[:2] != (B, F) or T.size != B or L.size != B or int(T.max()) != tmax or int(L.max()) != lmax:
        raise ValueError("op_align: m, ls [B, F, max T]; z [B, F, max L]")
    d = np.zeros((B, tmax), np.int32)
    sc = np.zeros(B, np.float32)
    if lib().vits_op_align(B, _ptr(T), _ptr(L), F, _ptr(m), _ptr(ls), _ptr(z), _ptr(d), _ptr(sc)) != 0:
        raise VitsError(last_error())
    return d, sc


def resample_plan(in_rate, out_rate):
    """vits_resample_plan: (L, M, K) of the polyphase filter in_rate -> out_rate (host only)"""
    v = [C.c_int32(), C.c_int32(), C.c_int32()]
    if lib().vits_resample_plan(int(in_rate), int(out_rate), *[C.byref(x) for x in v]) != 0:
        raise VitsError(last_error())
    return tuple(int(x.value) for x in v)


def resample_taps(in_rate, out_rate):
    """vits_resample_taps: the filter's fp32 tap table h [L, K] (host only)"""
    n = lib().vits_resample_taps(int(in_rate), int(out_rate), None, 0)
    if n < 0:
        raise VitsError(last_error())
    L, _, K = resample_plan(in_rate, out_rate)
    h = np.zeros((L, K), np.float32)
    if lib().vits_resample_taps(int(in_rate), int(out_rate), _ptr(h), h.size) != n:
        raise VitsError(last_error())
    return h


def resample_length(in_rate, out_rate, n):
    """vits_resample_length: ceil(n L / M), the samples at out_rate of n samples at in_rate (host only)"""
    r = lib().vits_resample_length(int(in_rate), int(out_rate), int(n))
    if r < 0:
        raise VitsError(last_error())
    return int(r)


def resample(x, in_rate, out_rate, lens=None, out=None):
    """The resampling kernel on a ragged batch (vits_op_resample). x: float32 [B, x_stride] (or one 1-D row) at in_rate; lens: samples per row (None =
    the whole row). Returns (y float32 [B, y_stride], n_out int64 [B]): row b holds its n_out[b] = ceil(lens[b] L / M) samples at out_rate, zeros behind them.
    out: a caller-owned float32 [B, y_stride] array to write into instead (what lies behind a row's samples stays as it was)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim == 1:
        x = x[None, :]
    B, stride = x.shape
    ln = np.full(B, stride, np.int64) if lens is None else np.ascontiguousarray(lens, dtype=np.int64).ravel()
    if ln.size != B:
        raise ValueError("lens needs one entry per row")
    if int(in_rate) == int(out_rate):
        n_out = ln.copy()
    else:
        n_out = np.array([resample_length(in_rate, out_rate, max(int(v), 0)) for v in ln], np.int64)
    if out is None:
        out = np.zeros((B, max(int(n_out.max()), 1)), np.float32)
    elif out.dtype != np.float32 or out.ndim != 2 or out.shape[0] != B or not out.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous float32 [B, y_stride] array")
    if lib().vits_op_resample(int(in_rate), int(out_rate), B, _ptr(x), stride, _ptr(ln), _ptr(out), out.shape[1]) != 0:
        raise VitsError(last_error())
    return out, n_out


def pitch_ratio(semitones):
    """vits_pitch_ratio: (float)2^(semitones / 12)"""
    return float(lib().vits_pitch_ratio(float(semitones)))


def pitch_plan(ratio, n):
    """vits_pitch_plan: (P, S, R, N') of a row of n samples at a pitch ratio (host only)"""
    P, S, R, n_out = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int64()
    if lib().vits_pitch_plan(float(ratio), int(n), C.byref(P), C.byref(S), C.byref(R), C.byref(n_out)) != 0:
        raise VitsError(last_error())
    return int(P.value), int(S.value), int(R.value), int(n_out.value)


def pitch_table():
    """vits_pitch_table: the prototype's two fp32 tables [2, Z Q + 2] = (G, D) (host only)"""
    n = lib().vits_pitch_table(None, 0)
    if n < 0:
        raise VitsError(last_error())
    t = np.zeros((2, n // 2), np.float32)
    if lib().vits_pitch_table(_ptr(t), t.size) != n:
        raise VitsError(last_error())
    return t


def pitch_host(x, ratio):
    """vits_pitch_host: the varispeed's definition evaluated in double, sequentially, on one row (host only) -> float64 [N']"""
    x = np.ascontiguousarray(x, dtype=np.float32).ravel()
    y = np.zeros(max(pitch_plan(ratio, x.size)[3], 1), np.float64)
    n = lib().vits_pitch_host(_ptr(x), x.size, float(ratio), _ptr(y), y.size)
    if n < 0:
        raise VitsError(last_error())
    return y[:n]


def pitch(x, ratios, lens=None, out=None):
    """The varispeed kernel on a ragged batch (vits_op_pitch). x: float32 [B, x_stride] (or one 1-D row), passed as it lies when it is C-contiguous float32
    (stride and alignment reach the device); ratios: a scalar or one ratio per row; lens: samples per row (None = the whole row). Returns (y float32
    [B, y_stride], n_out int64 [B]): row b holds its n_out[b] samples and, behind them, the byte of op_set_output_fill. out: a caller-owned float32
    [B, y_stride] array, which is overwritten whole."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim == 1:
        x = x[None, :]
    B, stride = x.shape
    ln = np.full(B, stride, np.int64) if lens is None else np.ascontiguousarray(lens, dtype=np.int64).ravel()
    r = np.ascontiguousarray(np.broadcast_to(np.asarray(ratios, np.float32).ravel(), (B,)))
    if ln.size != B:
        raise ValueError("lens needs one entry per row")
    if out is None:
        longest = max(-((-int(n) << 24) // max(int(float(p) * 2.0 ** 24), 1)) if np.isfinite(p) else 0 for n, p in zip(np.maximum(ln, 0), r))
        out = np.zeros((B, max(longest, 1)), np.float32)
    elif out.dtype != np.float32 or out.ndim != 2 or out.shape[0] != B or not out.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous float32 [B, y_stride] array")
    n_out = np.zeros(B, np.int64)
    if lib().vits_op_pitch(B, _ptr(x), stride, _ptr(ln), _ptr(r), _ptr(out), out.shape[1], _ptr(n_out)) != 0:
        raise VitsError(last_error())
    return out, n_out


def tempo_plan(rate, q, n):
    """vits_tempo_plan: (H, D, Q, F, N') of a row of n samples at `rate` and tempo q (host only)"""
    H, D, Q, F, n_out = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
    if lib().vits_tempo_plan(int(rate), float(q), int(n), C.byref(H), C.byref(D), C.byref(Q), C.byref(F), C.byref(n_out)) != 0:
        raise VitsError(last_error())
    return int(H.value), int(D.value), int(Q.value), int(F.value), int(n_out.value)


def tempo_host(x, rate, q):
    """vits_tempo_host: the time stretch's definition evaluated sequentially on one row (host only) -> (y float32 [N'], offsets int32 [F])"""
    x = np.ascontiguousarray(x, dtype=np.float32).ravel()
    _, _, _, F, n_out = tempo_plan(rate, q, x.size)
    y, off = np.zeros(max(n_out, 1), np.float32), np.zeros(max(F, 1), np.int32)
    n = lib().vits_tempo_host(_ptr(x), x.size, int(rate), float(q), _ptr(y), y.size, _ptr(off), off.size)
    if n < 0:
        raise VitsError(last_error())
    return y[:n], off[:F]


def tempo(x, rate, tempos, lens=None, out=None):
    """The time-stretch kernels on a ragged batch (vits_op_tempo). x: float32 [B, x_stride] (or one 1-D row), passed as it lies when it is C-contiguous float32
    (stride and alignment reach the device, as do out's); tempos: a scalar or one tempo per row; lens: samples per row (None = the whole row). Returns (y float32
    [B, y_stride], n_out int64 [B], offsets int32 [B, the largest F]): row b holds its n_out[b] samples and its F offsets and, behind them, the byte of
    op_set_output_fill. out: a caller-owned float32 [B, y_stride] array, which is overwritten whole."""
    x = np.asarray(x)
    if x.dtype != np.float32 or not x.flags.c_contiguous:
        x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim == 1:
        x = x[None, :]
    B, stride = x.shape
    ln = np.full(B, stride, np.int64) if lens is None else np.ascontiguousarray(lens, dtype=np.int64).ravel()
    r = np.ascontiguousarray(np.broadcast_to(np.asarray(tempos, np.float32).ravel(), (B,)))
    if ln.size != B:
        raise ValueError("lens needs one entry per row")
    longest = max(-((-int(n) << 24) // max(int(float(p) * 2.0 ** 24), 1)) if np.isfinite(p) else 0 for n, p in zip(np.maximum(ln, 0), r))
    if out is None:
        out = np.zeros((B, max(longest, 1)), np.float32)
    elif out.dtype != np.float32 or out.ndim != 2 or out.shape[0] != B or not out.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous float32 [B, y_stride] array")
    H = 4 * (int(rate) // 400)
    off = np.zeros((B, max(-(-longest // H) if H > 0 else 0, 1) + 1), np.int32)
    n_out = np.zeros(B, np.int64)
    if lib().vits_op_tempo(int(rate), B, _ptr(x), stride, _ptr(ln), _ptr(r), _ptr(out), out.shape[1], _ptr(n_out), _ptr(off), off.shape[1]) != 0:
        raise VitsError(last_error())
    return out, n_out, off


def loudness_plan(rate):
    """vits_loudness_plan: (coef float64 [2, 5] = b0 b1 b2 a1 a2 of the shelf and of the high-pass, S = samples per 100 ms segment) at `rate` (host only)"""
    coef, seg = np.zeros((2, 5), np.float64), C.c_int32()
    if lib().vits_loudness_plan(int(rate), _ptr(coef), C.byref(seg)) != 0:
        raise VitsError(last_error())
    return coef, int(seg.value)


def loudness_host(pcm, rate):
    """vits_loudness_host: (L in LUFS, -inf = unmeasurable; sample peak; blocks that passed both gates) of one utterance, the definition of
    include/vits.h in double on the host (no device needed)"""
    x = np.ascontiguousarray(pcm, dtype=np.float32).ravel()
    l, p, nb = C.c_double(), C.c_double(), C.c_int32()
    if lib().vits_loudness_host(_ptr(x), x.size, int(rate), C.byref(l), C.byref(p), C.byref(nb)) != 0:
        raise VitsError(last_error())
    return float(l.value), float(p.value), int(nb.value)


def level(x, rate, kind=LEVEL_MEASURE, value_db=0.0, ceiling_db=0.0, lens=None, out=None, apply=True):
    """The levelling kernels on a ragged batch (vits_op_level), staged as the engine stages it. x: float32 [B, x_stride] (or one 1-D row) at `rate`; lens:
    samples per row (None = the whole row). Returns (y, levels): levels float32 [B, 4] = (L, P, g, blocks); y float32 [B, y_stride] holds row b's lens[b]
    samples x * g (zeros, or what `out` held, behind them), or is None with apply=False (measure only)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim == 1:
        x = x[None, :]
    B, stride = x.shape
    ln = np.full(B, stride, np.int64) if lens is None else np.ascontiguousarray(lens, dtype=np.int64).ravel()
    if ln.size != B:
        raise ValueError("lens needs one entry per row")
    if not apply:
        out = None
    elif out is None:
        out = np.zeros((B, max(int(ln.max()), 1)), np.float32)
    elif out.dtype != np.float32 or out.ndim != 2 or out.shape[0] != B or not out.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous float32 [B, y_stride] array")
    d = LevelDesc(int(rate), B, max(stride, 1), out.shape[1] if out is not None else 0, int(kind), float(value_db), float(ceiling_db))
    levels = np.zeros((B, 4), np.float32)
    if lib().vits_op_level(C.byref(d), _ptr(x), _ptr(ln), _ptr(out) if out is not None else None, _ptr(levels)) != 0:
        raise VitsError(last_error())
    return out, levels


def limiter_plan(rate):
    """vits_limiter_plan: (A = look-ahead and attack, H = hold, tile = samples per block of the device kernels) at `rate` (host only)"""
    a, h, t = C.c_int32(), C.c_int32(), C.c_int32()
    if lib().vits_limiter_plan(int(rate), C.byref(a), C.byref(h), C.byref(t)) != 0:
        raise VitsError(last_error())
    return int(a.value), int(h.value), int(t.value)


def limiter_host(pcm, rate, g0, ceiling_db):
    """vits_limiter_host: (y float64 [n], limits float64 [4] = TP(x), TP(y), min s, share) of one row, the definition of include/vits.h in double on the
    host (no device needed)"""
    x = np.ascontiguousarray(pcm, dtype=np.float32).ravel()
    y, lim = np.zeros(max(x.size, 1), np.float64), np.zeros(4, np.float64)
    if lib().vits_limiter_host(_ptr(x), x.size, int(rate), float(g0), float(ceiling_db), _ptr(y), _ptr(lim)) != 0:
        raise VitsError(last_error())
    return y[:x.size], lim


def limit(x, rate, kind=LEVEL_GAIN, value_db=0.0, ceiling_db=0.0, lens=None, out=None, mode=LIMIT_TRUE_PEAK):
    """The levelling tail with the limiter on a ragged batch (vits_op_limit), staged as the engine stages it. x: float32 [B, x_stride] (or one 1-D row) at
    `rate`; lens: samples per row (None = the whole row). Returns (y, levels, limits): y float32 [B, y_stride] holds row b's lens[b] limited samples (zeros,
    or what `out` held, behind them); levels float32 [B, 4] = (L, P, g0, blocks); limits float32 [B, 4] = (TP(x), TP(y), min s, share)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim == 1:
        x = x[None, :]
    B, stride = x.shape
    ln = np.full(B, stride, np.int64) if lens is None else np.ascontiguousarray(lens, dtype=np.int64).ravel()
    if ln.size != B:
        raise ValueError("lens needs one entry per row")
    if out is None:
        out = np.zeros((B, max(int(ln.max()), 1)), np.float32)
    elif out.dtype != np.float32 or out.ndim != 2 or out.shape[0] != B or not out.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous float32 [B, y_stride] array")
    d = LimitDesc(LevelDesc(int(rate), B, max(stride, 1), out.shape[1], int(kind), float(value_db), float(ceiling_db)), int(mode))
    levels, limits = np.zeros((B, 4), np.float32), np.zeros((B, 4), np.float32)
    if lib().vits_op_limit(C.byref(d), _ptr(x), _ptr(ln), _ptr(out), _ptr(levels), _ptr(limits)) != 0:
        raise VitsError(last_error())
    return out, levels, limits


def edges_plan(rate, mode=EDGES_PAD, **fields):
    """vits_edges_plan: (W, Kh, Kt, Fi, Fo, Pl, Pt, tile) in samples at `rate` for a desc given as in Model.set_edges (host only)"""
    d = edges_desc(mode, **fields)
    out = np.zeros(8, np.int64)
    if lib().vits_edges_plan(int(rate), C.byref(d), _ptr(out)) != 0:
        raise VitsError(last_error())
    return tuple(int(v) for v in out)


def edges_host(pcm, rate, mode=EDGES_PAD, **fields):
    """vits_edges_host: (y float32 [N'], row int64 [4] = a, b, N', n_active, tail float32: what was written behind N' up to the bound) of one row, the
    definition of include/vits.h evaluated sequentially on the host (no device needed)"""
    x = np.ascontiguousarray(pcm, dtype=np.float32).ravel()
    d = edges_desc(mode, **fields)
    plan = np.zeros(8, np.int64)
    if lib().vits_edges_plan(int(rate), C.byref(d), _ptr(plan)) != 0:
        raise VitsError(last_error())
    y, row = np.full(x.size + int(plan[5]) + int(plan[6]) + 1, np.nan, np.float32), np.zeros(4, np.int64)
    if lib().vits_edges_host(_ptr(x), x.size, int(rate), C.byref(d), _ptr(y), y.size - 1, _ptr(row)) != 0:
        raise VitsError(last_error())
    assert np.isnan(y[-1])  # (nothing behind the bound)
    return y[:row[2]].copy(), row, y[row[2]:-1].copy()


_HIP = None


def _hip():
    """the HIP runtime the library is linked against, for the operator entry points that take device pointers"""
    global _HIP
    if _HIP is None:
        h = C.CDLL("libamdhip64.so")
        h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        h.hipFree.argtypes = [C.c_void_p]
        _HIP = h
    return _HIP


def edges(x, rate, mode=EDGES_PAD, lens=None, out=None, **fields):
    """The edges kernels on a ragged batch (vits_op_edges, which takes device pointers: the rows are staged here through the HIP runtime). x: float32
    [B, x_stride] (or one 1-D row) at `rate`, uploaded as it is (what lies behind a row's samples included); lens: samples per row (None = the whole row);
    out: float32 [B, y_stride] uploaded as the initial contents of y (None = zeros of the largest bound). Returns (y [B, y_stride], lens_out int32 [B],
    rows int64 [B, 4] = a, b, N', n_active)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim == 1:
        x = x[None, :]
    B, stride = x.shape
    ln = np.full(B, stride, np.int32) if lens is None else np.ascontiguousarray(lens, dtype=np.int32).ravel()
    if ln.size != B:
        raise ValueError("lens needs one entry per row")
    d = edges_desc(mode, **fields)
    if out is None:
        plan = np.zeros(8, np.int64)
        if lib().vits_edges_plan(int(rate), C.byref(d), _ptr(plan)) != 0:
            raise VitsError(last_error())
        out = np.zeros((B, max(int(ln.max()) + int(plan[5]) + int(plan[6]), 1)), np.float32)
    elif out.dtype != np.float32 or out.ndim != 2 or out.shape[0] != B or not out.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous float32 [B, y_stride] array")
    lens_out, rows = np.full(B, -1, np.int32), np.full((B, 4), -1, np.int64)
    hip = _hip()
    host = (x if x.size else np.zeros((B, 1), np.float32), ln, out, lens_out, rows)
    dev = [C.c_void_p() for _ in host]
    try:
        for p, a in zip(dev, host):
            if hip.hipMalloc(C.byref(p), max(a.nbytes, 4)) != 0 or hip.hipMemcpy(p, _ptr(a), a.nbytes, 1) != 0:
                raise VitsError("staging a batch for vits_op_edges: hipMalloc / hipMemcpy failed")
        if lib().vits_op_edges(int(rate), C.byref(d), B, dev[0], max(stride, 1), dev[1], dev[2], out.shape[1], dev[3], dev[4]) != 0:
            raise VitsError(last_error())
        for p, a in zip(dev[2:], host[2:]):
            if hip.hipMemcpy(_ptr(a), p, a.nbytes, 2) != 0:
                raise VitsError("reading the results of vits_op_edges: hipMemcpy failed")
    finally:
        for p in dev:
            if p.value:
                hip.hipFree(p)
    return out, lens_out, rows


def _join_args(B, track, gap_ms):
    tr = None if track is None else np.ascontiguousarray(track, dtype=np.int32).ravel()
    gp = None if gap_ms is None else np.ascontiguousarray(np.broadcast_to(np.asarray(gap_ms, np.float32).ravel(), (max(B, np.size(gap_ms)),)))
    return tr, gp


def join_plan(rate, utt_bounds, track=None, gap_ms=None):
    """vits_join_plan: (G, bounds int64 [G], tile) of utterances whose bounds (model-rate samples) are utt_bounds, laid into tracks by
    track (int32 [B], None = one track) and gap_ms (a scalar or float32 [B], None = 0), host only"""
    ub = np.ascontiguousarray(utt_bounds, dtype=np.int64).ravel()
    B = ub.size
    tr, gp = _join_args(B, track, gap_ms)
    G, tile, bounds = C.c_int32(0), C.c_int32(0), np.zeros(max(B, 1), np.int64)
    if lib().vits_join_plan(int(rate), B, _ptr(tr), _ptr(gp), _ptr(ub), C.byref(G), _ptr(bounds), C.byref(tile)) != 0:
        raise VitsError(last_error())
    return G.value, bounds[: G.value].copy(), tile.value


def join_host(x, rate, lens=None, track=None, gap_ms=None):
    """vits_join_host: the definition of include/vits.h evaluated sequentially on the host (no device needed). x: float32 [B, x_stride]; lens: samples per
    row (None = the whole row). Returns (y float32 [G, largest bound]: T_g samples of each track, then zeros up to its bound, track_lens int64 [G], rows
    int64 [B, 2] = o_b, n_b)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim == 1:
        x = x[None, :]
    B, stride = x.shape
    ln = np.full(B, stride, np.int64) if lens is None else np.ascontiguousarray(lens, dtype=np.int64).ravel()
    G, bounds, _ = join_plan(rate, ln, track, gap_ms)
    tr, gp = _join_args(B, track, gap_ms)
    ys = max(int(bounds.max()), 1)
    y, tl, rows = np.full((G, ys + 1), np.nan, np.float32), np.zeros(G, np.int64), np.zeros((B, 2), np.int64)
    if lib().vits_join_host(int(rate), B, _ptr(x), max(stride, 1), _ptr(ln), _ptr(tr), _ptr(gp), _ptr(y), ys + 1, _ptr(tl), _ptr(rows)) != 0:
        raise VitsError(last_error())
    for g in range(G):
        assert np.isnan(y[g, bounds[g]:]).all()  # (nothing behind the bound)
    return y[:, :ys], tl, rows


def join(x, rate, lens=None, track=None, gap_ms=None, out=None):
    """The join kernels on a ragged batch (vits_op_join). x: float32 [B, x_stride] at `rate`, uploaded as it is (what lies behind a row's samples
    included); lens: samples per row (None = the whole row); out: float32 [G, y_stride] uploaded as the initial contents of y (None = zeros of the largest
    bound). Returns (y [G, y_stride], track_lens int32 [G], rows int64 [B, 2] = o_b, n_b)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim == 1:
        x = x[None, :]
    B, stride = x.shape
    ln = np.full(B, stride, np.int32) if lens is None else np.ascontiguousarray(lens, dtype=np.int32).ravel()
    if ln.size != B:
        raise ValueError("lens needs one entry per row")
    tr, gp = _join_args(B, track, gap_ms)
    if out is None:
        G, bounds, _ = join_plan(rate, ln, track, gap_ms)
        out = np.zeros((G, max(int(bounds.max()), 1)), np.float32)
    elif out.dtype != np.float32 or out.ndim != 2 or not out.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous float32 [G, y_stride] array")
    xs = x if x.size else np.zeros((B, 1), np.float32)
    tl, rows = np.full(out.shape[0], -1, np.int32), np.full((B, 2), -1, np.int64)
    if lib().vits_op_join(int(rate), B, _ptr(xs), max(stride, 1), _ptr(ln), _ptr(tr), _ptr(gp), _ptr(out), out.shape[1], _ptr(tl), _ptr(rows)) != 0:
        raise VitsError(last_error())
    return out, tl, rows


def split_sentences(text):
    """vits_split_sentences: [(start, end, kind)] of the sentences of a text, byte offsets into its UTF-8 encoding; kind 1: the span ends a paragraph"""
    raw = text.encode("utf-8") if isinstance(text, str) else bytes(text)
    n = lib().vits_split_sentences(raw, None, None, None, 0)
    if n < 0:
        raise VitsError(last_error())
    st, en, kd = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int32)
    if lib().vits_split_sentences(raw, _ptr(st), _ptr(en), _ptr(kd), n) != n:
        raise VitsError(last_error())
    return [(int(st[i]), int(en[i]), int(kd[i])) for i in range(n)]


def op_rel_attention(q, k, v, rel_k, rel_v, heads, window, lens=None):
    q, k, v, rel_k, rel_v = map(_f32, (q, k, v, rel_k, rel_v))
    B, HD, T = q.shape
    out = np.zeros_like(q)
    lens = None if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
    if lib().vits_op_rel_attention(B, heads, HD // heads, T, T, window, _ptr(q), _ptr(k), _ptr(v), _ptr(rel_k), _ptr(rel_v),
                                   _ptr(lens), _ptr(out)) != 0:
        raise VitsError(last_error())
    return out


def op_add_layer_norm(x, residual, gamma, beta, eps=1e-5):
    x, residual, gamma, beta = map(_f32, (x, residual, gamma, beta))
    B, Cc, T = x.shape
    y = np.zeros_like(x)
    if lib().vits_op_add_layer_norm(B, Cc, T, T, eps, _ptr(x), _ptr(residual), _ptr(gamma), _ptr(beta), _ptr(y)) != 0:
        raise VitsError(last_error())
    return y


def _lens32(lens):
    return None if lens is None else np.ascontiguousarray(lens, dtype=np.int32)


def _tab16(tab):
    if tab is None:
        return None
    tab = np.ascontiguousarray(tab, dtype=np.uint16)
    assert tab.shape == (65536,), "a ggml table has 65536 fp16 entries (raw bits)"
    return tab


def op_attention_plan(heads, head_dim, t, batch=1, window=4, variant=ATT_VARIANT_PLAN):
    """What op_attention would launch (vits_op_attention_plan; host arithmetic, no GPU needed): a dict with kernel, variant (the one that runs), nw, maxs, vshift,
    grid, block, lds — or a VitsError naming the cause of the refusal."""
    d = AttentionDesc(batch, heads, head_dim, t, t, window, 1.0, variant)
    p = AttentionPlan()
    if lib().vits_op_attention_plan(C.byref(d), C.byref(p)) != 0:
        raise VitsError(last_error())
    out = {n: getattr(p, n) for n in ("variant", "nw", "maxs", "vshift", "block", "lds")}
    out["kernel"] = p.kernel.decode()
    out["grid"] = (p.grid_x, p.grid_y, p.grid_z)
    return out


def op_attention(q, k, v, rel_k, rel_v, heads, window, q_scale=1.0, variant=ATT_VARIANT_PLAN, exp_tab=None, lens=None, t=None):
    """The relative-position attention core through the kernel `variant` names (vits_op_attention): q, k, v [B, heads * head_dim, t_stride]; rel_k, rel_v
    [2 window + 1, head_dim]; exp_tab: ggml's fp16 exponential table (65536 raw uint16) or None (expf); t = the longest utterance (default: t_stride). The
    ATT_VARIANT_* other than _PLAN run that kernel or raise a VitsError naming the cause: never another one. Returns out [B, heads * head_dim, t_stride] as the
    device holds it: the staged NaN (all bits set) wherever no kernel wrote."""
    q, k, v, rel_k, rel_v = map(_f32, (q, k, v, rel_k, rel_v))
    B, HD, ts = q.shape
    hd = HD // heads
    assert HD == heads * hd and k.shape == q.shape and v.shape == q.shape and rel_k.shape == rel_v.shape == (2 * window + 1, hd)
    d = AttentionDesc(B, heads, hd, ts if t is None else t, ts, window, q_scale, variant)
    out = np.zeros_like(q)
    lens, exp_tab = _lens32(lens), _tab16(exp_tab)
    assert lens is None or lens.shape == (B,)
    if lib().vits_op_attention(C.byref(d), _ptr(q), _ptr(k), _ptr(v), _ptr(rel_k), _ptr(rel_v), _ptr(exp_tab), _ptr(lens), _ptr(out)) != 0:
        raise VitsError(last_error())
    return out


def op_layer_norm_plan(channels, t, batch=1, tw=0):
    """What op_layer_norm would launch (vits_op_layer_norm_plan; no GPU needed): a dict with kernel, tw, grid, block, lds — or a VitsError naming the cause."""
    d = LayerNormDesc(batch, channels, t, t, 1e-5, tw, 0, 0)
    p = LayerNormPlan()
    if lib().vits_op_layer_norm_plan(C.byref(d), C.byref(p)) != 0:
        raise VitsError(last_error())
    return dict(kernel=p.kernel.decode(), tw=p.tw, grid=(p.grid_x, p.grid_y, 1), block=p.block, lds=p.lds)


def op_layer_norm(x, gamma, beta, residual=None, eps=1e-5, tw=0, post_gelu=False, add_to=None, gelu_tab=None, lens=None, t=None):
    """add_layer_norm_kernel on the tile `tw` names (vits_op_layer_norm): v = LN(x + residual) * gamma + beta, GELU'd with post_gelu (gelu_tab: ggml's fp16 table);
    add_to [B, C, t_stride]: returns add_to + v computed in place on the device, otherwise v. Returned as the device holds it: the staged NaN behind lens[b]."""
    x, gamma, beta, residual, add_to = _f32(x), _f32(gamma), _f32(beta), _f32(residual), _f32(add_to)
    B, Cc, ts = x.shape
    assert gamma.shape == beta.shape == (Cc,) and (residual is None or residual.shape == x.shape) and (add_to is None or add_to.shape == x.shape)
    d = LayerNormDesc(B, Cc, ts if t is None else t, ts, eps, tw, int(bool(post_gelu)), 0 if add_to is None else 1)
    y = np.zeros_like(x) if add_to is None else add_to.copy()
    lens, gelu_tab = _lens32(lens), _tab16(gelu_tab)
    assert lens is None or lens.shape == (B,)
    if lib().vits_op_layer_norm(C.byref(d), _ptr(x), _ptr(residual), _ptr(gamma), _ptr(beta), _ptr(gelu_tab), _ptr(lens), _ptr(y)) != 0:
        raise VitsError(last_error())
    return y


def op_norm_conv_plan(cin, cout, k, t, batch=1, pad_left=None, pitch=0, post_act=0, variant=NC_VARIANT_PLAN):
    """What op_norm_conv would launch (vits_op_norm_conv_plan; no GPU needed): a dict with tile, variant (the one that runs), pitch, ln_ok, ln_why, launches,
    grid, block, lds — or a VitsError naming the cause of the refusal."""
    d = NormConvDesc(batch, cin, cout, t, t, pitch, k, (k - 1) // 2 if pad_left is None else pad_left, post_act, 1e-5, variant)
    p = NormConvPlan()
    if lib().vits_op_norm_conv_plan(C.byref(d), C.byref(p)) != 0:
        raise VitsError(last_error())
    out = {n: getattr(p, n) for n in ("variant", "pitch", "launches", "block", "lds")}
    out.update(tile=p.tile.decode(), ln_why=p.ln_why.decode(), ln_ok=bool(p.ln_ok), grid=(p.grid_x, p.grid_y, p.grid_z))
    return out


def op_norm_conv(x, gamma, beta, w, bias=None, residual=None, pad_left=None, post_act=0, eps=1e-5, pitch=0, variant=NC_VARIANT_PLAN, lens=None, t=None):
    """y = post(conv(LN(x)) + bias) [+ residual] and ln_out = LN(x) (vits_op_norm_conv): x [B, cin, t_stride], w [cout, cin, k]; NC_VARIANT_SEPARATE = the
    LayerNorm launch, then the conv; NC_VARIANT_ON_LOAD = one conv launch that normalises on load, or a VitsError naming the condition that fails; pitch: the
    device rows' pitch (0: t rounded up to 32). Returns (y [B, cout, t_stride], ln_out [B, cin, t_stride]): columns [0, t) as the device holds them (the staged
    NaN, all bits set, wherever no kernel wrote), NaN bits from t on."""
    x, gamma, beta, w, bias, residual = _f32(x), _f32(gamma), _f32(beta), _f32(w), _f32(bias), _f32(residual)
    B, cin, ts = x.shape
    cout, _, k = w.shape
    assert w.shape == (cout, cin, k) and gamma.shape == beta.shape == (cin,) and (bias is None or bias.shape == (cout,))
    assert residual is None or residual.shape == (B, cout, ts)
    d = NormConvDesc(B, cin, cout, ts if t is None else t, ts, pitch, k, (k - 1) // 2 if pad_left is None else pad_left, post_act, eps, variant)
    y = np.full((B, cout, ts), 0xFFFFFFFF, np.uint32).view(np.float32)
    ln_out = np.full((B, cin, ts), 0xFFFFFFFF, np.uint32).view(np.float32)
    lens = _lens32(lens)
    assert lens is None or lens.shape == (B,)
    if lib().vits_op_norm_conv(C.byref(d), _ptr(x), _ptr(gamma), _ptr(beta), _ptr(w), _ptr(bias), _ptr(residual), _ptr(lens), _ptr(y), _ptr(ln_out)) != 0:
        raise VitsError(last_error())
    return y, ln_out


def _filled(shape):
    """an output array of the operators below: they overwrite it whole, with the byte of op_set_output_fill wherever no kernel writes"""
    return np.zeros(shape, np.float32)


def op_spectrogram(pcm, n_fft, hop, bins=None, n_samples=None, t_stride=None):
    """The linear magnitude spectrogram (vits_op_spectrogram): pcm [B, pcm_stride] (or one row), n_samples [B] (None: every row whole). Returns
    [B, bins, t_stride] (bins None: n_fft / 2 + 1; t_stride None: the longest row's frames): frame t < n_samples[b] // hop in column t."""
    pcm = _f32(pcm)
    if pcm.ndim == 1:
        pcm = pcm[None]
    assert pcm.ndim == 2, "pcm is [B, pcm_stride]"
    B, stride = pcm.shape
    n = np.full(B, stride, np.int32) if n_samples is None else np.ascontiguousarray(n_samples, dtype=np.int32).reshape(-1)
    assert n.shape == (B,), "one n_samples per row"
    assert hop >= 1, "hop >= 1"
    bins = n_fft // 2 + 1 if bins is None else bins
    ts = max(1, int(n.max()) // hop) if t_stride is None else t_stride
    assert ts >= 1 and bins >= 1
    out = _filled((B, bins, ts))
    if lib().vits_op_spectrogram(n_fft, hop, bins, B, _ptr(pcm), stride, _ptr(n), ts, _ptr(out)) != 0:
        raise VitsError(last_error())
    return out


def _noise_args(B, noise, shape, seed_offsets, scales):
    if noise is not None:
        noise = _f32(noise)
        assert noise.shape == shape, "noise has the output's shape"
    if seed_offsets is not None:
        seed_offsets = np.ascontiguousarray(seed_offsets, dtype=np.int32)
        assert seed_offsets.shape == (B,), "one seed offset per row"
    if scales is not None:
        scales = _f32(scales)
        assert scales.shape == (B,), "one noise scale per row"
    return noise, seed_offsets, scales


def op_prior_sample(mean, logvar, cum, frames, t_stride=None, tok_lens=None, noise=None, seed=0, seed_offsets=None, noise_scale=1.0, noise_scales=None):
    """Prior sampling through the alignment (vits_op_prior_sample, zp_kernel): mean, logvar [B, C, t_tok], cum int32 [B, t_tok], frames [B]. noise [B, C, t_stride]
    or None = the counter stream of `seed` (+ seed_offsets[b], or b). Returns zp [B, C, t_stride]."""
    mean, logvar = _f32(mean), _f32(logvar)
    B, Cn, T = mean.shape
    assert logvar.shape == mean.shape
    cum = np.ascontiguousarray(cum, dtype=np.int32)
    frames = np.ascontiguousarray(frames, dtype=np.int32)
    assert cum.shape == (B, T) and frames.shape == (B,)
    tok_lens = None if tok_lens is None else np.ascontiguousarray(tok_lens, dtype=np.int32)
    assert tok_lens is None or tok_lens.shape == (B,)
    ts = max(1, int(frames.max())) if t_stride is None else t_stride
    noise, seed_offsets, noise_scales = _noise_args(B, noise, (B, Cn, ts), seed_offsets, noise_scales)
    zp = _filled((B, Cn, ts))
    if lib().vits_op_prior_sample(B, Cn, T, ts, _ptr(mean), _ptr(logvar), _ptr(cum), _ptr(tok_lens), _ptr(frames), _ptr(noise), seed, _ptr(seed_offsets), noise_scale,
                                  _ptr(noise_scales), _ptr(zp)) != 0:
        raise VitsError(last_error())
    return zp


def op_posterior_sample(mean, logstd, frames, noise=None, seed=0, seed_offsets=None, flip=False, eps_scale=1.0):
    """The posterior draw (vits_op_posterior_sample): mean, logstd [B, C, t_stride], frames [B]; noise as in op_prior_sample. flip: channel c goes to row C - 1 - c.
    Returns zq [B, C, t_stride]."""
    mean, logstd = _f32(mean), _f32(logstd)
    B, Cn, ts = mean.shape
    assert logstd.shape == mean.shape
    frames = np.ascontiguousarray(frames, dtype=np.int32)
    assert frames.shape == (B,)
    noise, seed_offsets, _ = _noise_args(B, noise, (B, Cn, ts), seed_offsets, None)
    zq = _filled((B, Cn, ts))
    if lib().vits_op_posterior_sample(B, Cn, ts, _ptr(mean), _ptr(logstd), _ptr(frames), _ptr(noise), seed, _ptr(seed_offsets), 1 if flip else 0, eps_scale, _ptr(zq)) != 0:
        raise VitsError(last_error())
    return zq


def op_conv_post(x, w, slope, lens=None, emit_lo=0, emit_hi=None, want_pre=True, x_pitch=None, pre_pitch=None, layout=CONV_POST_FP32_LAYOUT):
    """The vocoder's last kernel (vits_op_conv_post): x [B, cin, T], w [cin, k] (or [1, cin, k]). x_pitch / pre_pitch: floats per device row of x and of pre (None:
    T rounded up to 4). Returns (wave [B, T], pre [B, T] or None); only samples [emit_lo, min(emit_hi[b], lens[b])) are written."""
    x, w = _f32(x), _f32(w)
    if w.ndim == 3:
        assert w.shape[0] == 1, "conv_post has one output channel"
        w = w[0]
    B, cin, T = x.shape
    assert w.ndim == 2 and w.shape[0] == cin, "w is [cin, k]"
    w = np.ascontiguousarray(w)
    lens = None if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
    emit_hi = None if emit_hi is None else np.ascontiguousarray(emit_hi, dtype=np.int32)
    assert lens is None or lens.shape == (B,)
    assert emit_hi is None or emit_hi.shape == (B,)
    r4 = (T + 3) // 4 * 4
    d = ConvPostDesc(B, cin, w.shape[1], T, r4 if x_pitch is None else x_pitch, r4 if pre_pitch is None else pre_pitch, slope, emit_lo, layout)
    wave, pre = _filled((B, T)), _filled((B, T)) if want_pre else None
    if lib().vits_op_conv_post(C.byref(d), _ptr(x), _ptr(w), _ptr(lens), _ptr(emit_hi), _ptr(pre), _ptr(wave)) != 0:
        raise VitsError(last_error())
    return wave, pre


def op_resblock_sum(y0, y1, y2=None, scale=1.0, scale_div=False, act=False, slope=0.1, lens=None, in_pitch=None, out_pitch=None):
    """((y0 + y1) [+ y2]) * scale (or / scale) [+ leaky_relu(slope)] (vits_op_resblock_sum, rb_sum3_std_kernel): addends [B, C, T]; in_pitch / out_pitch: floats per
    device row (None: T). Returns [B, C, T]."""
    y0, y1 = _f32(y0), _f32(y1)
    y2 = None if y2 is None else _f32(y2)
    B, Cn, T = y0.shape
    assert y1.shape == y0.shape and (y2 is None or y2.shape == y0.shape)
    lens = None if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
    assert lens is None or lens.shape == (B,)
    out = _filled((B, Cn, T))
    if lib().vits_op_resblock_sum(B, Cn, T, T if in_pitch is None else in_pitch, T if out_pitch is None else out_pitch, scale, 1 if scale_div else 0, 1 if act else 0,
                                  slope, _ptr(y0), _ptr(y1), _ptr(y2), _ptr(lens), _ptr(out)) != 0:
        raise VitsError(last_error())
    return out


def pcm16(pcm):
    pcm = _f32(pcm)
    out = np.zeros(pcm.size, np.int16)
    lib().vits_pcm16_from_float(_ptr(pcm), pcm.size, _ptr(out))
    return out


def pcm16_device(src_ptr, src_stride, dst_ptr, dst_stride, rows, cols, lengths_ptr=None, stream=None):
    """Device fp32 -> int16 rows (vits_pcm16_from_float_device). All pointers are integer device addresses; lengths_ptr
    (optional) is a device int64 [rows] array; stream a hipStream_t value (None = default stream). Asynchronous."""
    f = lib().vits_pcm16_from_float_device
    f.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p]
    f.restype = C.c_int
    if f(src_ptr, src_stride, dst_ptr, dst_stride, lengths_ptr, rows, cols, stream) != 0:
        raise VitsError(last_error())


GATHER_ID_BYTES = 128


class GatherResult(C.Structure):
    _fields_ = [("data", C.c_void_p), ("stride", C.c_int64), ("lengths", C.POINTER(C.c_int64)), ("rows_total", C.c_int32)]


def gather_unique_id():
    """vits_pcm_gather_unique_id: the 128 bytes rank 0 creates and hands to the other ranks (the RCCL unique id)."""
    f = lib().vits_pcm_gather_unique_id
    f.restype, f.argtypes = C.c_int, [C.c_char_p]
    buf = C.create_string_buffer(GATHER_ID_BYTES)
    if f(buf) != 0:
        raise VitsError(last_error())
    return buf.raw


def gather_verdict(table, world, rows):
    """vits_pcm_gather_verdict: the decision every rank takes on the table of the first all-gather ([row_capacity, lengths...] per rank, -1 = a row
    its rank could not use). Returns the common row width; raises VitsError with the message every rank would report."""
    t = np.ascontiguousarray(table, dtype=np.int64).reshape(world, rows + 1)
    f = lib().vits_pcm_gather_verdict
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]
    out = C.c_int64(0)
    if f(_ptr(t), world, rows, C.byref(out)) != 0:
        raise VitsError(last_error())
    return int(out.value)


class PcmGather:
    """The C ABI's PCM all-gather (include/vits.h vits_pcm_gather_*: RCCL through dlopen, no torch): what a C / C++ / Swift host calls;
    multi_gpu.PcmExchange is the torch.distributed form of the same exchange."""

    def __init__(self, unique_id, rank, world, rows, row_capacity, elem_bytes=4):
        L = lib()
        L.vits_pcm_gather_init.restype = C.c_void_p
        L.vits_pcm_gather_init.argtypes = [C.c_char_p, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32]
        L.vits_pcm_gather.restype = C.c_int
        L.vits_pcm_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(GatherResult)]
        L.vits_pcm_gather_destroy.restype = None
        L.vits_pcm_gather_destroy.argtypes = [C.c_void_p]
        self._h = L.vits_pcm_gather_init(unique_id, len(unique_id) if unique_id is not None else 0, rank, world, rows, row_capacity, elem_bytes)
        if not self._h:
            raise VitsError(last_error())

    def gather(self, pcm_ptr, pcm_stride, lengths, stream=None):
        """pcm_ptr: integer device address of [rows][pcm_stride]; lengths: host int64 [rows]. Returns (device address of the gathered
        [rows_total][stride] block, stride, lengths of all rows as a numpy array)."""
        lengths = np.ascontiguousarray(lengths, dtype=np.int64)
        r = GatherResult()
        if lib().vits_pcm_gather(self._h, pcm_ptr, pcm_stride, _ptr(lengths), stream, C.byref(r)) != 0:
            raise VitsError(last_error())
        return r.data, int(r.stride), np.ctypeslib.as_array(r.lengths, shape=(r.rows_total,)).copy()

    def close(self):
        if self._h:
            lib().vits_pcm_gather_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def write_wav16(path, pcm, sample_rate=16000):
    pcm = _f32(pcm)
    if lib().vits_write_wav16(os.fsencode(path), _ptr(pcm), pcm.size, sample_rate) != 0:
        raise VitsError(last_error())


def set_device(index):
    if lib().vits_set_device(index) != 0:
        raise VitsError(last_error())


def device_info():
    name = C.create_string_buffer(256)
    cu, mhz, hbm = C.c_int32(), C.c_int32(), C.c_int64()
    if lib().vits_device_info(name, 256, C.byref(cu), C.byref(mhz), C.byref(hbm)) != 0:
        raise VitsError(last_error())
    return {"name": name.value.decode(), "cu_count": cu.value, "clock_mhz": mhz.value, "hbm_bytes": hbm.value}
