// kernels.h — launch interface of the hand-written gfx950 kernels (host side sees only these functions).
//
// Data layout everywhere: activations are fp32 [batch][channel][time], TIME CONTIGUOUS (== the reference's ggml
// ne order [time, channel, batch], so a wavefront's 64 lanes read 64 consecutive time steps = 256 B coalesced).
// Every tensor argument carries its own batch stride (bs) and channel stride (cs), in floats. Ragged batches:
// `len[b]` is the number of valid time steps of utterance b; loads beyond it read as ZERO (utterance boundaries
// behave exactly like the zero padding a batch-1 run sees) and stores beyond it are suppressed.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "tile_map.h"

struct vits_edges_desc;  // include/vits.h

namespace vits {

// Tuning knobs of the launch functions: which tile shape / kernel variant a launch takes. None of them changes a bit of a result (GPU test:
// tools/knob_identity.py). They are read from the environment ONCE per model handle, when it is loaded (Engine::knobs.kernel), and installed
// for the calling thread around every engine entry point (KernelKnobsScope in the ABI); the model-free entry points (vits_op_*) and the
// developer harnesses under tools/ see the process defaults, read at first use. Header-only so that the harnesses that include a single
// kernel file link without the engine.
struct KernelKnobs {
    int narrow_tiles = 64;       // VITS_NARROW_TILES: fp32 convs of at most this many rows take 128-column tiles (0: 256-column tiles)
    int tile128 = 1;             // VITS_TILE128=0: no 128 x 128 tiles in conv_mfma
    int min_blocks = 0;          // VITS_MIN_BLOCKS: grid size under which conv_mfma steps down to a smaller tile (0: 1024 for k <= 3, else 512)
    bool no_narrow = false;      // VITS_NO_NARROW: no 32-column strips for tiny grids / 1x1 convs
    int narrow_k1 = 1 << 30;     // VITS_NARROW_K1: longest sequence whose 1x1 convs take the narrow tile (0: small grids only)
    int nbuf = 0;                // VITS_NBUF=2|3: LDS ring depth of conv_mfma (0: chosen per launch)
    bool no_oneshot = false;     // VITS_NO_ONESHOT: no cooperative one-shot fill for latency-bound launches
    int db_min = 1;              // VITS_DB_MIN=2: register-staged kernels for single-chunk inputs
    int t16_tile0 = 0;           // VITS_T16_TILE0: conv16 tile for c_out multiples of 128 (0: 128 x 128)
    bool no_convt16s = false;    // VITS_NO_CONVT16S: 16-bit transposed convs through conv16's polyphase epilogue
    bool convt16s_all = false;   // VITS_CONVT16S_ALL: the one-row-tile streaming kernel also for stride 8
    bool no_convt16l = false;    // VITS_NO_CONVT16L: no four-phase lines kernel for strides that are multiples of 4
    bool no_att_lat = false;     // VITS_NO_ATT_LAT: small attention grids (at most 128 blocks) without the operand prefetch across phases (the eight-wave kernel of round 6's first step)
    bool att_valu = false;       // VITS_ATT_VALU: attention without the matrix cores
    int att_nw = 0;              // VITS_ATT_NW=4|8: waves per attention block (0: by LDS footprint)
    int att_short = 512;         // VITS_ATT_SHORT: longest sequence (tokens) for the short-sequence attention variant (0: off)
    int ln_tw = 32;              // VITS_LN_TW=64: LayerNorm tiles of 64 time steps (sixteen waves)
    bool rbb_c128 = true;        // VITS_RBB_C128=0: C = 128, k = 3 resblocks as fused pairs instead of rbblock16
    int rbb_c64k11 = -1;         // VITS_RBB_C64K11: C = 64, k = 11 resblocks through rbblock16 as well: 1 always, 0 never (three fused pairs), -1 where the grid is large enough for segments of tiles (VITS_RBB_STREAM_*)
    int rbb_stream_tiles = -1;   // VITS_RBB_STREAM_TILES: tiles a block of rbblock16 walks with the left halo taken from the previous tile (-1: per shape, see plan_rbblock16; 0 / 1: always one tile per block, both halos recomputed; N: N for every shape)
    int rbb_stream_min_blocks = 1536;  // VITS_RBB_STREAM_MIN_BLOCKS: ... while the segments still number at least this many blocks (two rounds of 3 x 256)
    int fuse16_maxc = 256;       // VITS_FUSE16_MAXC: widest stage whose 16-bit conv pairs are fused
    bool fuse32_c128 = true;     // VITS_FUSE32_C128=0: fp32 k = 3 pairs at C = 128 as two launches
    int wn16_ncw = 1;            // VITS_WN16_NCW=2: 16-bit WaveNet layer with six waves, both column tiles each
    int flow_ncw = 2;            // VITS_FLOW_NCW=1: 16-bit coupling-layer kernel with one column tile per wave
    int convt16_r128 = 0;        // VITS_CONVT16_R128: developer override of the streaming transposed conv's shape for 128-row layers (the 128 -> 64 stride-2 upsampler): nr * 100 + csplit * 10 + (rs == 16), e.g. 211 = <2, 1, 16>; 0 = default <4, 1, 16>
    int convt16_split_max = 64;  // VITS_CONVT16_SPLIT_MAX: 16-bit stride-8 upsamplers deal the units of a position tile out over up to four blocks while the launch has at most this many tiles (0: never)
    bool no_rbb_group3_c64 = false;   // VITS_NO_RBB_GROUP3_C64: ... only the C = 32 stage grouped
    bool no_rbb_group3 = false;       // VITS_NO_RBB_GROUP3: the C = 32 stage's three whole-resblock kernels always as three launches (small grids: not one grouped launch)
    bool no_rb_sum3_f32 = false;      // VITS_NO_RB_SUM3_F32: fp32 path: the resblocks of a small-grid stage always chained through the shared sum
    bool rb_sum3_in_order = false;    // VITS_RB_SUM3_IN_ORDER: side-by-side resblocks enqueued first to last, the first on the main stream (until round 6's last step; default: the last — longest — first and on the main stream)
    bool rb_sum3_block_only = false;  // VITS_RB_SUM3_BLOCK_ONLY: the separate sum launch only for stages whose resblocks are all whole-resblock kernels (until round 6's last step: every small-grid stage)
    bool no_rb_sum3 = false;     // VITS_NO_RB_SUM3: the resblocks of an all-whole-resblock stage always chained through the shared sum (no separate sum launch on small grids)
    int rb16_narrow_max = 128;   // VITS_RB16_NARROW_MAX: 16-bit fused pairs at C >= 128 on 64-column blocks while the 128-column tile would give at most this many blocks (0: never; 64 until round 6: batch 4 / 6 -1 ... -2 % with 128)
    int flow_narrow_max = 96;    // VITS_FLOW_NARROW_MAX: 16-bit coupling-layer kernel on 16-frame blocks while the 48-frame tile would give at most this many blocks (0: never)
    bool no_ln_fuse = false;     // VITS_NO_LN_FUSE: the encoder's LayerNorms always as their own launches (never applied on load by the consuming conv_lat16_kernel)
    bool no_dds_lat = false;     // VITS_NO_DDS_LAT: the duration predictor's DDS layers always on dds_layer_kernel (no 16-token latency kernel, no fused 1x1 convs around it)
    int dds_lat_max_blocks = 96; // VITS_DDS_LAT_MAX_BLOCKS: the latency kernel is taken while batch x ceil(tokens / 16) is at most this
    bool no_dp_det_fuse = false; // VITS_NO_DP_DET_FUSE: the deterministic duration predictor always as its un-fused sequence (row add, conv, LayerNorm, conv, LayerNorm, 1x1 conv)
    int dp_det_lat_max_blocks = 96;  // VITS_DP_DET_LAT_MAX_BLOCKS: dp_det_kernel takes its 16-token tile while batch x ceil(tokens / 16) is at most this, the wide tile above
    int lat16h_group_shape = 21;  // VITS_LAT16H_GROUP_SHAPE: 10 x row tiles + column tiles per block of conv16_lat_group_kernel (21, 41, 22, 42)
    bool no_lat16h_group = false; // VITS_NO_LAT16H_GROUP: the C = 256 stage's latency convs as 18 launches on three streams (not six grouped launches on one)
    bool no_lat16h_pre = false;  // VITS_NO_LAT16H_PRE: 16-bit modes: the vocoder's conv_pre always as converter launch + conv16_kernel
    bool no_lat16h = false;      // VITS_NO_LAT16H: 16-bit modes: the wide stages' resblock convs on small grids as fused pairs (rbpair16) / conv16_kernel, never conv16_lat_kernel
    int lat16h_max_tiles = 2048; // VITS_LAT16H_MAX_TILES: ... while a C = 256 conv has at most this many 32 x 32 output tiles (batch 1 ... 4 x 128 ids)
    int lat16h_max_tiles_c128 = 0;  // VITS_LAT16H_MAX_TILES_C128: the same for C = 128 (batch 1 = 1792 tiles measured + 6 ... 12 us against the fused pairs: off)
    int lat16h_shape = 21;       // VITS_LAT16H_SHAPE: 10 x waves per block + 32-column tiles per wave of conv16_lat_kernel (21, 22, 42)
    bool no_lat16 = false;       // VITS_NO_LAT16: tiny grids with long K chains on the 128 x 32 tile of conv_mfma instead of conv_lat16_kernel
    int lat16_max_waves = 768;   // VITS_LAT16_MAX_WAVES: standard convs with at most this many 32 x 32 output tiles take conv_lat16_kernel (0: tiny grids only)
    bool no_tile_map = false;    // VITS_NO_TILE_MAP: ragged batches always on the dense grid (blocks past an utterance's end load its length and return)
    bool tile_map = false;       // VITS_TILE_MAP: the list of existing tiles (tile_map.h) wherever a converted kernel runs, small grids and full grids included
    static KernelKnobs from_env() {
        KernelKnobs k;
        auto num = [](const char* name, int& v) {
            if (const char* e = getenv(name)) v = atoi(e);
        };
        auto flag = [](const char* name, bool& v) { v = getenv(name) != nullptr; };
        num("VITS_NARROW_TILES", k.narrow_tiles);
        flag("VITS_NO_DDS_LAT", k.no_dds_lat);
        flag("VITS_NO_LN_FUSE", k.no_ln_fuse);
        flag("VITS_NO_RB_SUM3", k.no_rb_sum3);
        flag("VITS_RB_SUM3_BLOCK_ONLY", k.rb_sum3_block_only);
        flag("VITS_RB_SUM3_IN_ORDER", k.rb_sum3_in_order);
        flag("VITS_NO_RB_SUM3_F32", k.no_rb_sum3_f32);
        flag("VITS_NO_RBB_GROUP3", k.no_rbb_group3);
        flag("VITS_NO_RBB_GROUP3_C64", k.no_rbb_group3_c64);
        num("VITS_DDS_LAT_MAX_BLOCKS", k.dds_lat_max_blocks);
        flag("VITS_NO_DP_DET_FUSE", k.no_dp_det_fuse);
        num("VITS_DP_DET_LAT_MAX_BLOCKS", k.dp_det_lat_max_blocks);
        num("VITS_TILE128", k.tile128);
        num("VITS_MIN_BLOCKS", k.min_blocks);
        flag("VITS_NO_NARROW", k.no_narrow);
        num("VITS_NARROW_K1", k.narrow_k1);
        num("VITS_NBUF", k.nbuf);
        flag("VITS_NO_ONESHOT", k.no_oneshot);
        num("VITS_DB_MIN", k.db_min);
        num("VITS_T16_TILE0", k.t16_tile0);
        flag("VITS_NO_CONVT16S", k.no_convt16s);
        flag("VITS_CONVT16S_ALL", k.convt16s_all);
        flag("VITS_NO_CONVT16L", k.no_convt16l);
        flag("VITS_ATT_VALU", k.att_valu);
        flag("VITS_NO_ATT_LAT", k.no_att_lat);
        num("VITS_ATT_NW", k.att_nw);
        num("VITS_ATT_SHORT", k.att_short);
        num("VITS_LN_TW", k.ln_tw);
        if (const char* e = getenv("VITS_RBB_C128")) k.rbb_c128 = atoi(e) != 0;
        num("VITS_RBB_C64K11", k.rbb_c64k11);
        num("VITS_RBB_STREAM_TILES", k.rbb_stream_tiles);
        num("VITS_RBB_STREAM_MIN_BLOCKS", k.rbb_stream_min_blocks);
        num("VITS_FUSE16_MAXC", k.fuse16_maxc);
        if (const char* e = getenv("VITS_FUSE32_C128")) k.fuse32_c128 = atoi(e) != 0;
        num("VITS_WN16_NCW", k.wn16_ncw);
        num("VITS_FLOW_NCW", k.flow_ncw);
        num("VITS_FLOW_NARROW_MAX", k.flow_narrow_max);
        num("VITS_RB16_NARROW_MAX", k.rb16_narrow_max);
        num("VITS_CONVT16_SPLIT_MAX", k.convt16_split_max);
        num("VITS_CONVT16_R128", k.convt16_r128);
        flag("VITS_NO_LAT16", k.no_lat16);
        flag("VITS_NO_LAT16H", k.no_lat16h);
        flag("VITS_NO_LAT16H_PRE", k.no_lat16h_pre);
        flag("VITS_NO_LAT16H_GROUP", k.no_lat16h_group);
        num("VITS_LAT16H_GROUP_SHAPE", k.lat16h_group_shape);
        num("VITS_LAT16H_MAX_TILES", k.lat16h_max_tiles);
        num("VITS_LAT16H_MAX_TILES_C128", k.lat16h_max_tiles_c128);
        num("VITS_LAT16H_SHAPE", k.lat16h_shape);
        num("VITS_LAT16_MAX_WAVES", k.lat16_max_waves);
        flag("VITS_NO_TILE_MAP", k.no_tile_map);
        flag("VITS_TILE_MAP", k.tile_map);
        return k;
    }
};
namespace detail {
inline thread_local const KernelKnobs* tl_kernel_knobs = nullptr;
}
inline const KernelKnobs& kernel_knobs() {
    if (detail::tl_kernel_knobs) return *detail::tl_kernel_knobs;
    static const KernelKnobs process_default = KernelKnobs::from_env();
    return process_default;
}
struct KernelKnobsScope {
    const KernelKnobs* prev;
    explicit KernelKnobsScope(const KernelKnobs* k) : prev(detail::tl_kernel_knobs) { detail::tl_kernel_knobs = k; }
    ~KernelKnobsScope() { detail::tl_kernel_knobs = prev; }
    KernelKnobsScope(const KernelKnobsScope&) = delete;
    KernelKnobsScope& operator=(const KernelKnobsScope&) = delete;
};

// A launch of fewer blocks than this is a small grid: under two blocks per CU (plan_conv steps its tile down below it, conv_plan.cpp).
constexpr int kSmallGridBlocks = 512;
// The list a ragged launch runs over instead of its dense grid (tile_map.h), or null = the dense grid. `maps`: the lists of the call's length vector (null: none
// were built — a batch of one, equal lengths, a 16-bit mode); width: the kernel's columns per block; dense_blocks: the whole dense grid. The list is taken where
// one of this width was built and the launch is large; VITS_TILE_MAP takes it wherever it exists, VITS_NO_TILE_MAP nowhere.
// launches of this process that were issued over a list (vits_op_tile_map_launches: a test sees which form ran). Counted by the launcher where it hands the
// list's extent to the grid: a launch that is skipped (an empty list) or falls back to the dense grid is not counted
inline std::atomic<uint64_t>& tile_map_launches() {
    static std::atomic<uint64_t> n{0};
    return n;
}
inline void tile_map_launch_issued() { tile_map_launches().fetch_add(1, std::memory_order_relaxed); }
inline const TileMapRef* tile_map_for(const TileMapSet* maps, int width, bool convt, int64_t dense_blocks) {
    const KernelKnobs& kn = kernel_knobs();
    if (!maps || kn.no_tile_map) return nullptr;
    const TileMapRef* m = maps->find(width, convt);
    if (!m || !m->dev) return nullptr;
    return kn.tile_map || dense_blocks >= kSmallGridBlocks ? m : nullptr;
}

// hipFuncAttributeMaxDynamicSharedMemorySize is an attribute of a function ON A DEVICE. A kernel instantiation that needs more than
// 64 KB of LDS raises its limit once per device: the once-flag is one bit per device, so a process that loads models on several
// devices (vits_set_device) raises it on each of them (a process-wide flag left the second device at 64 KB: launch failures there).
struct BigLdsOnce {
    std::atomic<uint64_t> mask{0};
    static uint64_t bit() {
        int d = 0;
        (void)hipGetDevice(&d);
        return 1ull << (d & 63);
    }
    bool needed() const { return !(mask.load(std::memory_order_acquire) & bit()); }
    void done() { mask.fetch_or(bit(), std::memory_order_release); }
    // before a launch with `lds` bytes of dynamic LDS: raise the kernel's limit to `limit`, the first time on this device that it needs more than 64 KB.
    // limit: the CU's 160 KB minus the kernel's static __shared__ bytes
    hipError_t raise(const void* kernel, size_t lds, int limit = 160 * 1024) {
        if (lds <= 64 * 1024 || !needed()) return hipSuccess;
        if (hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, limit)) return e;
        done();
        return hipSuccess;
    }
};

// Per-launch timing without extra queue packets. The engine's per-kernel profiler (bench.py's instrumented region) used to bracket
// every launch with hipEventRecord: a barrier packet each, ~300 of them per step, and durations that include the gap to the next packet.
// When the profiler has armed this thread's timer, the next kernel launch carries the two events on its OWN dispatch packet instead
// (hipExtLaunchKernel: start / end timestamps of the kernel's completion signal — the clock rocprofv3 reads), and only a span that
// launches several kernels falls back to a recorded stop event (Profiler::end). (Step time: the same, 76.8 against 76.9 ms.)
struct LaunchTimer {
    hipEvent_t start = nullptr, stop = nullptr;
    int launches = 0;
};
inline thread_local LaunchTimer vits_launch_timer;
#define VITS_KLAUNCH(kernel, grid, block, lds, stream, ...)                                                          \
    do {                                                                                                            \
        ::vits::LaunchTimer& lt_ = ::vits::vits_launch_timer;                                                       \
        if (lt_.start && lt_.launches++ == 0)                                                                       \
            hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, lt_.start, lt_.stop, 0, __VA_ARGS__);           \
        else                                                                                                        \
            hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);                                      \
    } while (0)

// THE way to launch a kernel with dynamic LDS, launch_lds<&kernel<...>>(grid, block, lds, stream, args...): raises the kernel's limit the first time on a
// device (BigLdsOnce, one per instantiation). LIMIT: see BigLdsOnce::raise
template <auto Kernel, int LIMIT = 160 * 1024, class... A>
inline hipError_t launch_lds(dim3 grid, dim3 block, size_t lds, hipStream_t s, const A&... args) {
    static BigLdsOnce once;
    if (hipError_t e = once.raise(reinterpret_cast<const void*>(Kernel), lds, LIMIT)) return e;
    VITS_KLAUNCH(Kernel, grid, block, lds, s, args...);
    return hipGetLastError();
}

#ifdef __HIPCC__
// The WaveNet gate tanh(a) * sigmoid(s) (vits.cpp:442-450) of every gated-conv epilogue (conv_mfma.hip, conv16.hip, wavenet32.hip), libm's
// tanhf / expf. (A version on the hardware exp2 / reciprocal — one v_exp_f32 per factor, |error| <= 2e-7 — measured +-0 on a fused WaveNet
// layer: the gate is 1.5 of its 37 us, tools/wn16_micro.hip; the exact functions stay.)
__device__ __forceinline__ float wavenet_gate(float a, float s) { return tanhf(a) * (1.0f / (1.0f + expf(-s))); }
#endif

struct TensorRef {
    float* p = nullptr;
    int64_t bs = 0;  // batch stride (floats)
    int32_t cs = 0;  // channel stride (floats)
};

// ---- MFMA convolution ---------------------------------------------------------------------------------
enum ConvEpilogue : int { EPI_STD = 0, EPI_GATE = 1, EPI_CONVT = 2 };
enum ConvTile : int {
    TILE_128x128 = 0,
    TILE_64x256 = 1,
    TILE_32x256 = 2,
    TILE_64x64 = 3,
    TILE_32x64 = 4,
    TILE_NARROW = 5,  // 128 rows x 32 columns (256 x 32 for the gated conv): tiny grids and 1x1 convs only (plan_conv, conv_plan.cpp)
    TILE_LAT16 = 6    // 64 rows x 16 columns on v_mfma_f32_16x16x4_f32 (conv_lat16_kernel): tiny grids with long K chains
};

// Weights pre-packed at load time in exact MFMA A-fragment order (see conv_mfma.hip), resident in HBM.
struct PackedConv {
    float* wp = nullptr;    // packed weights
    float* bias = nullptr;  // [cout] (original channel order) or nullptr
    // speaker-conditioned layers of a multi-speaker model (the duration predictor's conv_pre, every WaveNet in_layer, the decoder's conv_pre): bias
    // points into row 0 of the engine's effective-bias table (speaker -1 = the plain biases) and bias_rs is that table's row stride (floats). A call
    // with speakers passes one row index per utterance (ConvCall::spk ...); the kernels then read bias + bias_rs * spk[b]. 0: not conditioned.
    int64_t bias_rs = 0;
    int cin = 0, cout = 0, kt = 0;
    int rows = 0;      // GEMM M (cout, or cout*stride for the transposed conv)
    int mtiles = 0;       // number of 32-row tiles in the packed array (padded to a multiple of 4)
    int mtiles_used = 0;  // tiles that hold real rows
    int nchunks = 0;   // ceil(cin / 32)
    int epi = EPI_STD;
    int ct_stride = 0;  // EPI_CONVT: upsampling stride s
    int64_t bytes = 0;
    uint16_t* wp16 = nullptr;  // 16-bit A fragments of the VITS_ARITH_F16 / BF16 path (packed by Engine::set_arith)
    float* wp_l16 = nullptr;   // the same weights as v_mfma_f32_16x16x4_f32 A fragments (repack_conv_weights_l16) for conv_lat16_kernel, or nullptr
    int64_t bytes16 = 0;
    uint16_t* wps = nullptr;   // VITS_ARITH_F32_SPLIT: the weights as TWO bf16 planes of A fragments (conv_split.hip pack_conv_weights_split), or nullptr
    int64_t bytes_s = 0;
};

// 16-bit activation in "group layout" [batch][channel/8][time][8] (conv16.hip): one 16-byte slot = 8 channels of one time step
struct Ref16 {
    uint16_t* p = nullptr;
    int64_t bs = 0;  // batch stride (16-bit elements)
    int32_t ts = 0;  // slots per group row (time stride)
};

// a conv input of VITS_ARITH_F32_SPLIT (conv_split.hip): the three bf16 planes of an fp32 tensor in the group layout, [batch][plane 3][channel/8][time][8]
struct Split3Ref {
    uint16_t* p = nullptr;
    int64_t bs = 0;  // batch stride (16-bit elements)
    int64_t ps = 0;  // plane stride
    int32_t ts = 0;  // slots per group row (time stride)
};

struct ConvCall {
    TensorRef x, y, res, acc;  // res/acc optional (p == nullptr)
    const int* len_in = nullptr;   // per-utterance valid input length (nullptr: t_in)
    const int* len_out = nullptr;  // per-utterance valid output length (nullptr: t_out)
    const int* spk = nullptr;      // per-utterance row of the effective-bias table (device [batch]; read only when w.bias_rs != 0), or nullptr = row 0
    int batch = 1;
    int t_in = 0, t_out = 0;  // maximum lengths (grid extent)
    // profiler accounting only: sum over the batch of the per-utterance valid input / output lengths (< 0: batch * t_in / t_out).
    // Blocks past an utterance's length exit at once, so work and traffic are counted over the real lengths, not the padded extent.
    int64_t sum_in = -1, sum_out = -1;
    int dil = 1, pad_l = 0;
    int pre_act = 0;  // 1: leaky_relu(slope) on load
    float slope = 0.f;
    int post_act = 0;  // 1: relu; 2: leaky_relu(post_slope) of the stored value (EPI_STD)
    float post_slope = 0.f;
    float* y2 = nullptr;  // EPI_STD, optional: also store leaky_relu(post_slope) of the output here (layout of y)
    float scale = 1.f;  // applied when acc.p: y = (acc + v) * scale, or / scale when scale_div
    int scale_div = 0;
    int ct_crop = 0;  // EPI_CONVT: output crop
    int tile = -1;    // ConvTile override (-1: chosen from the shape)
    const TileMapSet* maps = nullptr;  // ragged batches: the lists of existing tiles of (len_in, len_out), per tile width (tile_map_for), or null = the dense grid
    // LayerNorm over the input channels applied ON LOAD (round 6; conv_lat16_kernel only — conv_ln_on_load_ok() tells, launch_conv refuses otherwise):
    // x is the UN-normalised tensor (add_layer_norm_kernel's input), every block normalises the columns of its input tile in that kernel's order of
    // operations, and ln_out (any layout) receives the normalised tensor — each column written once, by the blocks of the first row group.
    const float *ln_gamma = nullptr, *ln_beta = nullptr;
    float ln_eps = 0.f;
    TensorRef ln_out;
    // VITS_ARITH_F32_SPLIT (launch_conv_split only): the input as split planes (x is then unused), and — optional — the planes of leaky_relu(ys3_slope) of the
    // result for the next conv (y may then be null: a tensor whose only reader is the next conv is never stored in fp32)
    Split3Ref xs3, ys3;
    float ys3_slope = 1.f;
};
// VITS_ARITH_F32_SPLIT (conv_split.hip): fp32-accurate convs on the bf16 matrix cores by operand splitting — see the file's head comment
bool conv_split_candidate(int epi, int kt, int cin, int cout);  // the layers that get split weight planes at vits_model_set_arith
bool pack_conv_weights_split(const float* w, int cout, int cin, int k, std::vector<uint16_t>& out);  // w: torch layout [cout][cin][k]; false = not exactly two bf16 pieces
bool conv_split_supported(const PackedConv& w, int dil);
hipError_t launch_conv_split(const PackedConv& w, const ConvCall& c, hipStream_t s);
hipError_t launch_split_planes(TensorRef x, int channels, const int* lens, int batch, int tmax, float slope, Split3Ref out, hipStream_t s);

// host-side packing: w is torch layout [cout][cin][k] (EPI_STD / EPI_GATE) or [cin][cout][k] (EPI_CONVT)
std::vector<float> pack_conv_weights(const float* w, int cout, int cin, int k, int epi, int ct_stride, int* rows, int* mtiles_used, int* mtiles,
                                     int* nchunks);
// conv_lat16_kernel's A fragments from the packed array: [32-row tile][16-row half][quad = 16 input channels of one tap][lane][4] with lane l = row l & 15,
// component s = channel 4 s + (l >> 4) of the quad: one 16-byte load per lane feeds four consecutive MFMAs. Same size as `packed`.
std::vector<float> repack_conv_weights_l16(const std::vector<float>& packed, int mtiles, int nchunks, int kt);
bool conv_lat16_candidate(int epi, int kt, int cin);  // the layers that get a second copy of their fp32 weights for the latency kernel: every STD conv and the 5-tap GATE convs with >= 64 products per output
bool conv_ln_on_load_ok(const PackedConv& w, const ConvCall& c);  // plan_conv(w, c).ln_ok
hipError_t launch_conv(const PackedConv& w, const ConvCall& c, hipStream_t s);
double conv_flops(const PackedConv& w, const ConvCall& c, int64_t total_cols);
// The same-position convolutions of up to three ResBlocks (11 / 7 / 3 taps, one dilation of {1, 3, 5}, one channel count that is a
// multiple of 128) as ONE launch on the 128 x 128 tile; results are bit-identical to n launch_conv calls.
bool conv_group_supported(const PackedConv& w, int dil);
hipError_t launch_conv_group(const PackedConv* const* w, const ConvCall* c, int n, hipStream_t s);

// ---- 16-bit-operand convolution (conv16.hip): v_mfma_f32_32x32x16_{f16,bf16}, fp32 accumulate --------------------
struct Conv16Call {
    Ref16 x;  // input, group layout (already activated: the writer / converter applies the leaky_relu)
    const int* len_in = nullptr;
    const int* len_out = nullptr;
    const int* spk = nullptr;  // effective-bias table rows (see ConvCall::spk)
    int batch = 1, t_in = 0, t_out = 0, dil = 1, pad_l = 0;
    int post_act = 0;  // standard outputs: 1 relu, 2 leaky_relu(post_slope) of the stored value; group outputs: 1 relu
    float post_slope = 0.f;
    float scale = 1.f;
    int scale_div = 0;
    int ct_crop = 0;
    int tile = -1;
    // standard-layout fp32 outputs / inputs ([b][c][t]): used when neither yg nor y16 is set
    TensorRef y, res, acc;
    float* y2 = nullptr;
    // group-layout outputs: fp32 residual stream [b][c/8][g_ts][8] (yg / resg / accg share strides) and the 16-bit copy
    float* yg = nullptr;
    const float* resg = nullptr;
    const float* accg = nullptr;
    int64_t g_bs = 0;
    int g_ts = 0;
    Ref16 y16;
    float y16_slope = 1.f;  // leaky_relu fused into the 16-bit copy (1 = none)
    int64_t sum_in = -1, sum_out = -1;  // profiler accounting (see ConvCall)
    int force_split = 0;  // launch_convt16_stream, lines kernels: 1, 2 or 4 = the units of a position tile over that many blocks whatever the grid (vits_op_upsample16); 0: the planner's choice
};
// One HiFiGAN ResBlock conv pair as a single kernel (rbpair16.hip): y' = y + conv2(leaky_relu(conv1(x) + b1)) + b2 with x =
// the 16-bit leaky_relu(y); the intermediate stays in LDS. C = 32 / 64, k = 3 / 7 / 11, conv1 dilation 1 / 3 / 5.
struct RbPair16Call {
    Ref16 x;
    const int* lens = nullptr;
    int batch = 1, tmax = 0, dil = 1;
    float slope = 0.1f;
    float* yg = nullptr;
    const float* resg = nullptr;
    const float* accg = nullptr;
    int64_t g_bs = 0;
    int g_ts = 0;
    Ref16 y16;
    float y16_slope = 1.f;
    float scale = 1.f;
    int scale_div = 0;
    int force_nr = 0;  // C >= 128: 4 or VITS_RB16_NARROW_NR = that many column tiles per wave whatever the grid (vits_op_resblock); 0: the planner's choice
};
bool rbpair16_supported(int channels, int kt, int dil);
// One whole ResBlock (three pairs, dilations 1 / 3 / 5) as a single kernel (rbblock16.hip): the fp32 stream stays in registers across the
// pairs, HBM sees the stage input once and the resblock output once. C = 32 / 64, k = 3 / 7 / 11.
struct RbBlock16Call {
    const float* y0 = nullptr;  // stage input, fp32 group layout [b][C/8][g_ts][8]
    const int* lens = nullptr;
    int batch = 1, tmax = 0;
    float slope = 0.1f;
    float* yg = nullptr;  // output (same strides as y0)
    const float* accg = nullptr;
    int64_t g_bs = 0;
    int g_ts = 0;
    Ref16 y16;
    float y16_slope = 1.f;
    float scale = 1.f;
    int scale_div = 0;
    int force_nt = 0;  // N >= 1: every block walks N tiles (1: the one-tile form) whatever the grid and the knobs (vits_op_resblock); 0: the planner's choice
};
bool rbblock16_supported(int channels, int kt, const int* dils, int ndil, int batch, int tmax);  // (batch x tmax: the launch's grid — C = 64, k = 11 only where it is cut into segments)
hipError_t launch_rbblock16(const PackedConv* const* c1, const PackedConv* const* c2, const RbBlock16Call& c, int arith, hipStream_t s);
// the three resblocks (k = 3, 7, 11) of a C = 32 stage as ONE launch (small grids, side-by-side resblocks): c1[m] / c2[m] = member m's three conv pairs
bool rbblock16_group3_supported(int channels, const int* kts, int batch, int tmax);
hipError_t launch_rbblock16_group3(const PackedConv* const (*c1)[3], const PackedConv* const (*c2)[3], const RbBlock16Call* c, int arith, hipStream_t s);
// ((y0 + y1) [+ y2]) * scale (or / scale) over fp32 group-layout tensors, in the order and with the expressions of the resblocks' chained accumulation; the fp32 sum
// (optional) and / or its 16-bit copy behind leaky_relu(y16_slope) — small grids: the resblocks of a stage then need not run one behind the other
hipError_t launch_rb_sum3(const float* y0, const float* y1, const float* y2, int channels, int64_t g_bs, int g_ts, const int* lens, int batch, int tmax, float scale, int scale_div,
                          float* yg, Ref16 y16, float y16_slope, int arith, hipStream_t s);
// fp32 ResBlock conv pair as one kernel (rbpair32.hip): y = x + conv2(leaky_relu(conv1(leaky_relu(x)) + b1)) + b2; y must not alias x
struct RbPair32Call {
    TensorRef x, y, acc;
    const int* lens = nullptr;
    const TileMapSet* maps = nullptr;  // the lists of existing tiles of `lens` (see ConvCall::maps)
    int batch = 1, tmax = 0, dil = 1;
    float slope = 0.1f;
    float scale = 1.f;
    int scale_div = 0;
    int post_act = 0;
    float post_slope = 0.f;
};
bool rbpair32_supported(int channels, int kt, int dil);
// fp32: one WHOLE 3-tap ResBlock (dilations 1 / 3 / 5) of a narrow stage as one kernel (rbblock32.hip): the stream stays in registers across the three
// pairs; bit-identical to three launch_rbpair32 calls. y must not alias x (acc may alias y).
struct RbBlock32Call {
    TensorRef x, y, acc;
    const int* lens = nullptr;
    const TileMapSet* maps = nullptr;  // the lists of existing tiles of `lens` (see ConvCall::maps)
    int batch = 1, tmax = 0;
    float slope = 0.1f;
    float scale = 1.f;
    int scale_div = 0;
    int post_act = 0;
    float post_slope = 0.f;
};
bool rbblock32_supported(int channels, int kt, const int* dils, int ndil);
hipError_t launch_rbblock32(const PackedConv* const* c1, const PackedConv* const* c2, const RbBlock32Call& c, hipStream_t s);
// one WaveNet layer of the flow (gated conv + 1x1 res/skip conv + the two adds) as one fp32 kernel (wavenet32.hip); h_out must not alias h
struct WaveNet32Call {
    TensorRef h, h_out, outputs;
    const int* lens = nullptr;
    const int* spk = nullptr;  // effective-bias table rows of the gated conv's bias (see ConvCall::spk)
    int batch = 1, tmax = 0, hidden = 0, dil = 1;
    int force_ncw = 0;  // 16-bit kernel: 1 or 2 = that many column tiles per wave whatever VITS_WN16_NCW says (vits_op_flow_coupling); 0: the planner's choice
};
bool wavenet32_supported(int hidden, int kt, int dil, const PackedConv& in, const PackedConv& rs);
hipError_t launch_wavenet32(const PackedConv& in, const PackedConv& rs, const WaveNet32Call& c, hipStream_t s);
bool wavenet16_supported(int hidden, int kt, int dil, const PackedConv& in, const PackedConv& rs);  // the same layer on 16-bit operands
hipError_t launch_wavenet16(const PackedConv& in, const PackedConv& rs, const WaveNet32Call& c, int arith, hipStream_t s);
// one whole coupling layer of the flow (pre conv, four WaveNet layers, post conv, x1 += ...) as one kernel, 16-bit-operand modes (wavenet32.hip)
struct FlowCouple16Call {
    TensorRef x0, x1;  // conditioning half (read), updated half (in place): fp32 [b][F/2][t]
    const int* lens = nullptr;
    const int* spk = nullptr;  // effective-bias table rows of the in_layers' biases (see ConvCall::spk)
    int batch = 1, tmax = 0, hidden = 0, half = 0;
    int force_ncw = 0, force_nct = 0;  // both set: that (column tiles per wave, per block) whatever the grid and the knobs (vits_op_flow_coupling); 0, 0: the planner's choice
};
bool flow_couple16_supported(int hidden, int half, int kt, int rate, int layers, const PackedConv& pre, const PackedConv* in, const PackedConv* rs, const PackedConv& post);
hipError_t launch_flow_couple16(const PackedConv& pre, const PackedConv* in, const PackedConv* rs, const PackedConv& post, const FlowCouple16Call& c, int arith,
                                hipStream_t s);
hipError_t launch_rbpair32(const PackedConv& c1, const PackedConv& c2, const RbPair32Call& c, hipStream_t s);
hipError_t launch_rbpair16(const PackedConv& c1, const PackedConv& c2, const RbPair16Call& c, int arith, hipStream_t s);
std::vector<uint16_t> pack_conv_weights16(const float* w, int cout, int cin, int k, int epi, int ct_stride, int arith);
// conv16_lat.hip: the wide stages' group-layout resblock convs on small grids (batch 1 ... 4); launch_conv16 routes to it (profile tile tag T7)
bool conv16_lat_shape_ok(int channels, int kt, int dil, int batch, int tmax);
bool conv16_lat_wanted(const PackedConv& w, const Conv16Call& c);
struct Conv16LatPlan;  // block shape, pitch, grid, LDS bytes (conv_plan.h)
hipError_t launch_conv16_lat(const PackedConv& w, const Conv16Call& c, const Conv16LatPlan& l, int arith, hipStream_t s);  // (launch_conv16's lat route)
bool conv16_lat_group_wanted(const PackedConv* const* w, const Conv16Call* c);  // the same-position convs of a stage's three resblocks (k = 3, 7, 11) as ONE launch
hipError_t launch_conv16_lat_group(const PackedConv* const* w, const Conv16Call* c, int arith, hipStream_t s);
bool conv16_lat_pre_wanted(const PackedConv& w, int batch, int tmax);  // the vocoder's conv_pre on a small grid, straight from the fp32 flow output (no converter launch)
hipError_t launch_conv16_lat_pre(const PackedConv& w, TensorRef x, const int* lens, int batch, int tmax, Ref16 y16, float y16_slope, int arith, hipStream_t s,
                                 const int* spk = nullptr);
hipError_t launch_conv16(const PackedConv& w, const Conv16Call& c, int arith, hipStream_t s);
// ConvTranspose1d (kernel = 2 x stride) in the group layout as a streaming kernel (convt16.hip): all stride x c_out rows of a tile of input
// positions per block; bit-identical to launch_conv16 on the same call
bool convt16_stream_supported(const PackedConv& w);
hipError_t launch_convt16_stream(const PackedConv& w, const Conv16Call& c, int arith, hipStream_t s);
// tile tag of the instantiation launch_convt16_stream picks for `w` ("SL128" = convt16_lines_kernel<128>, "S4.1.16" = convt16_kernel<4, 1, 16>):
// the profiler label carries it, so that a profiler entry lines up with exactly one rocprofv3 kernel name (tools/pmc_common.py)
void convt16_stream_tag(const PackedConv& w, char* buf, size_t cap);
hipError_t launch_to_group16(TensorRef x, const int* lens, int batch, int channels, int tmax, float slope, Ref16 y, int arith, hipStream_t s);
hipError_t launch_conv_post16(Ref16 x, const float* w, int cin, int k, TensorRef pre, TensorRef wave, const int* lens, int batch, int tmax, int arith, hipStream_t s,
                              int emit_lo = 0, const int* emit_hi = nullptr);

// ---- the non-GEMM kernels, one block per file --------------------------------------------------------------
// EMULATED ggml lookup tables (INFERRED from upstream ggerganov/ggml of the reference's era, the maxilevi/ggml fork is
// absent): device copies of the two 65536-entry fp16 tables ggml builds at init — gelu[i] = fp16(tanh-GELU(fp16 value i)), exp[i] =
// fp16(expf(fp16 value i)) — built on the host with the C library (Engine::set_ggml_tables). Kernels that receive a non-null pointer route
// ggml_gelu (vits.cpp:673,687) / the exponential of ggml_soft_max (vits.cpp:329,719,735) through it; null = erf-GELU / fp32 soft-max.
struct GgmlTables {
    const uint16_t* gelu = nullptr;
    const uint16_t* exp = nullptr;
};
// ---- attention (attention.hip) ------------------------------------------------------------------------
hipError_t launch_rel_attention(TensorRef q, TensorRef k, TensorRef v, const float* rel_k, const float* rel_v, TensorRef out, const int* lens, int batch,
                                int heads, int head_dim, int tmax, int window, float q_scale, hipStream_t s, GgmlTables tabs = GgmlTables(), int force = 0);  // force: plan_rel_attention's
// ---- LayerNorm over channels (layer_norm.hip) ---------------------------------------------------------
hipError_t launch_add_layer_norm(TensorRef x, TensorRef res, const float* gamma, const float* beta, TensorRef y, const int* lens, int batch, int channels,
                                 int tmax, float eps, int post_gelu, TensorRef add_to, hipStream_t s, GgmlTables tabs = GgmlTables(), int force_tw = 0);  // force_tw: plan_add_layer_norm's
// ---- the duration predictor's DDS block (dds.hip; its latency kernel: stage1_lat.hip) -----------------
hipError_t launch_pointwise_from1(TensorRef z, int zc, const float* w, const float* bias, TensorRef cond, TensorRef y, const int* lens, int batch,
                                  int channels, int tmax, hipStream_t s, int arith = 0);
hipError_t launch_dds_depthwise(TensorRef x, TensorRef g, const float* w, const float* bias, const float* gamma, const float* beta, TensorRef y,
                                const int* lens, int batch, int channels, int tmax, int k, int dil, float eps, hipStream_t s, int arith = 0,
                                GgmlTables tabs = GgmlTables());
// one DDS layer (depthwise + LN + gelu + 1x1 conv + LN + gelu + residual) as one kernel; y must not alias x
bool dds_layer_supported(const PackedConv& pw, int channels, int k, int dil, int arith);
hipError_t launch_dds_layer(TensorRef x, TensorRef y, const float* dw_w, const float* dw_b, const float* g1, const float* b1, const PackedConv& pw, const float* g2,
                            const float* b2, const int* lens, int batch, int channels, int tmax, int k, int dil, float eps, int arith, hipStream_t s,
                            GgmlTables tabs = GgmlTables());
// The same layer for latency-bound launches (stage1_lat.hip: 16-token blocks, element-parallel phases, 16x16x4 MFMA tiles; bit-identical), optionally
// with the per-token op in front of the DDS block fused in (head_w: the conv flow's 1 -> H conv of latent row zc + conditioning, vits.cpp:864,651-653;
// head_conv: an H -> H 1x1 conv of x, vits.cpp:939) and the 1x1 conv behind it (tail_conv -> y2; y is then not written). fp32 arithmetic only.
struct DdsLatCall {
    TensorRef x, y;
    const float *dw_w = nullptr, *dw_b = nullptr, *g1 = nullptr, *b1 = nullptr, *g2 = nullptr, *b2 = nullptr;
    const PackedConv* pw = nullptr;
    const float *head_w = nullptr, *head_b = nullptr;
    TensorRef z, cond;
    int zc = 0;
    const PackedConv* head_conv = nullptr;
    const PackedConv* tail_conv = nullptr;
    TensorRef y2;
    const int* lens = nullptr;
    const int* spk = nullptr;  // effective-bias table rows of head_conv's bias (see ConvCall::spk)
    int batch = 1, channels = 0, tmax = 0, k = 3, dil = 1;
    float eps = 1e-5f;
    GgmlTables tabs;
};
bool dds_layer_lat_supported(const PackedConv& pw, int channels, int k, int dil);
hipError_t launch_dds_layer_lat(const DdsLatCall& c, hipStream_t s);
// ---- the deterministic duration predictor (dp_det.hip) ------------------------------------------------
// The deterministic duration predictor (transformers VitsDurationPredictor, eval mode) as ONE kernel (dp_det.hip), fp32 in every arithmetic mode:
//   x' = x + row (inside the utterance only; the speaker term, added ON LOAD), a1 = LN(relu(conv_1(x'))), a2 = LN(relu(conv_2(a1))), logw = proj(a2)
// with a1 / a2 zero outside [0, len). conv_1 / conv_2: k taps, zero padding k / 2; proj: 1x1 to one channel. Bit for bit the un-fused sequence
// launch_add_rows, launch_conv(post_act = 1), launch_add_layer_norm, launch_conv, launch_add_layer_norm, launch_conv (the engine's fallback).
// rows: a table of per-utterance rows [*][hidden] with row stride row_rs (floats); utterance b reads row row_idx[b], or row b when row_idx is null. rows == nullptr: no add.
struct DpDetCall {
    TensorRef x;     // [batch][hidden][t]
    TensorRef logw;  // [batch][1][t]: the row the durations kernel reads
    const PackedConv *c1 = nullptr, *c2 = nullptr, *proj = nullptr;  // wp_l16 fragments and biases
    const float *g1 = nullptr, *be1 = nullptr, *g2 = nullptr, *be2 = nullptr;
    const float* rows = nullptr;
    int64_t row_rs = 0;
    const int* row_idx = nullptr;
    const int* lens = nullptr;
    int batch = 1, hidden = 0, filter = 0, tmax = 0, k = 3;
    float eps = 1e-5f;
    int variant = 0;  // 0: the planner's tile; 1: the 16-token tile; 2: the wide tile
};
struct DpDetPlan;  // launch_plan.h
bool dp_det_supported(const DpDetCall& c);  // an instantiation exists for (hidden, filter, k) and the three convs carry their 16x16x4 fragments
hipError_t launch_dp_det(const DpDetCall& c, hipStream_t s);
// the un-fused sequence itself (six launches; xp is written only when c.rows): the engine's fallback and the operator's variant 3 are this one function
hipError_t launch_dp_det_unfused(const DpDetCall& c, TensorRef xp, TensorRef a, TensorRef b, hipStream_t s);
// y[b][c][t] = x[b][c][t] + rows[row(b)][c] for t < lens[b] (nothing is written behind an utterance): the un-fused predictor's first step
hipError_t launch_add_rows(TensorRef x, TensorRef y, const float* rows, int64_t row_rs, const int* row_idx, const int* lens, int batch, int channels, int tmax, hipStream_t s);
// ---- the element-wise part of the duration predictor's flows (spline.hip) -----------------------------
hipError_t launch_spline(TensorRef u, TensorRef z, int zc, const int* lens, int batch, int tmax, int bins, float tail, float inv_sqrt, int mode,
                         hipStream_t s, GgmlTables tabs = GgmlTables());
hipError_t launch_affine(TensorRef z, int c_first, const float* translate, const float* log_scale, int sign, const int* lens, int batch, int tmax,
                         hipStream_t s);
// Per-utterance prosody: launch_noise_dur, launch_scale_rows, launch_durations and launch_zp each take an optional device array next to their scalar
// (scales / length_scales / noise_scales [B]: utterance b's value instead of the scalar; null = the scalar for every utterance, as before).
hipError_t launch_noise_dur(TensorRef z, const int* lens, int batch, int tmax, uint64_t seed, const int* seed_off, float scale, const float* scales, hipStream_t s);
// x[b][c][t] *= scale, or scales[b] when scales (device [B]) is given
hipError_t launch_scale_rows(TensorRef x, int channels, float scale, const float* scales, int batch, int tmax, hipStream_t s);
// ---- exact-order stage one of the emulated-ggml mode (exact_stage1.hip; element functions: include/vits_exact_math.h) -----------------------
hipError_t launch_exact_conv(TensorRef x, const float* w, const float* bias, TensorRef y, TensorRef res, const int* lens, int batch, int cin, int cout, int K, int dil, int pad_l,
                             int tmax, bool relu, const float* post_scale, hipStream_t s);
hipError_t launch_exact_depthwise(TensorRef x, const float* w, const float* bias, TensorRef y, const int* lens, int batch, int channels, int K, int dil, int pad, int tmax,
                                  hipStream_t s);
hipError_t launch_exact_add(TensorRef x, TensorRef g, const int* lens, int batch, int channels, int tmax, hipStream_t s);
hipError_t launch_exact_layer_norm(TensorRef x, const float* gamma, const float* beta, const int* lens, int batch, int channels, int tmax, float eps, const uint16_t* gelu_tab,
                                   hipStream_t s);
hipError_t launch_exact_attention(TensorRef q, TensorRef k, TensorRef v, const float* ek, const float* ev, TensorRef out, float* scratch, int srow, const int* lens, int batch,
                                  int heads, int hd, int tmax, int window, const uint16_t* exp_tab, hipStream_t s);
hipError_t launch_exact_affine(TensorRef z, int c_first, float t0, float t1, float e0, float e1, const int* lens, int batch, int tmax, hipStream_t s);
hipError_t launch_exact_spline(TensorRef z, int row, TensorRef u, float* res, float* inside, float* tmp, int stride, const int* lens, int batch, int tmax, int nb, float B,
                               float inv_sqrt, float constant, bool refmode, const uint16_t* exp_tab, hipStream_t s);
// ---- stage one's glue (stage1_glue.hip) ---------------------------------------------------------------
hipError_t launch_embed(const int* ids, int id_stride, const int* lens, const float* table, int hidden, float scale, TensorRef x, int batch, int tmax,
                        hipStream_t s);
hipError_t launch_fill(float* p, size_t n, float v, hipStream_t s);
hipError_t launch_fill_rows(TensorRef x, int channels, float v, int batch, int tmax, hipStream_t s);
// (per-utterance prosody: see launch_noise_dur.) launch_durations also takes optional override rows ovr [B][tmax] (>= 0: the token's duration; -1: the prediction).
hipError_t launch_durations(TensorRef logw, int c, const int* lens, int batch, int tmax, float length_scale, const float* length_scales, const int* ovr, int fixed,
                            float* dur, int* cum, int* frames, int* stage_lens, int n_stage, const int* stage_mul, const int* stage_add, hipStream_t s,
                            bool exact = false);
hipError_t launch_zp(TensorRef mean, TensorRef logvar, const int* cum, int cum_stride, const int* tok_lens, const int* frames, TensorRef noise, int noise_kind,
                     uint64_t seed, const int* seed_off, float noise_scale, const float* noise_scales, TensorRef zp, int batch, int channels, int lmax, hipStream_t s);
// one segment of the effective-bias table of a multi-speaker model (built once at load): row 0 (speaker -1) = bias, row 1 + s =
// bias + (cond_w . emb[s] + cond_b) for the n channels of the segment; cond_w is the conditioning 1x1 conv [n][E], emb [n_spk][E]
hipError_t launch_speaker_bias(const float* bias, const float* cond_w, const float* cond_b, const float* emb, int n, int E, int n_spk, float* table,
                               int64_t row_stride, hipStream_t s);
// ---- voices registered at run time (voices.hip) -------------------------------------------------------
// rows of an effective-bias table for voices registered at run time: ONE launch for every segment of the table and all n_voices new rows.
// A segment = the n channels at float offset `off` of a table row, conditioned by rows w [n][E] / cb [n] of a 1x1 conv (device pointers); tile0 = the
// sum of voice_seg_tiles(n) over the segments before it, `tiles` the sum over all. Row row_first + v = row 0 + (w . emb[v] + cb) in speaker_bias_kernel's
// order of operations. The table must hold row_first + n_voices rows. Any n_voices: the launcher walks slices of the grid's y limit; few voices take a
// variant with one chain per thread (the same arithmetic per output).
struct VoiceSeg {
    const float* w;
    const float* cb;
    int64_t off;
    int n, tile0;
};
int voice_seg_tiles(int n);
hipError_t launch_voice_rows(const VoiceSeg* segs, int nseg, int tiles, const float* emb, int n_voices, int E, float* table, int64_t row_stride, int row_first,
                             hipStream_t s);
// ---- around the vocoder's convolutions, and the delivery's int16 PCM (vocoder_glue.hip) ---------------
hipError_t launch_rb_sum3_std(TensorRef y0, TensorRef y1, TensorRef y2, TensorRef out, int channels, const int* lens, int batch, int tmax, float scale, int scale_div, int post_act,
                              float post_slope, hipStream_t s);  // fp32 [b][c][t]: ((y0 + y1) [+ y2]) scaled [+ leaky_relu]: side-by-side resblocks of the fp32 path (small grids)
hipError_t launch_conv_post(TensorRef x, const float* w, int cin, int k, float slope, TensorRef pre_tanh, TensorRef wave, const int* lens, int batch,
                            int tmax, hipStream_t s, int emit_lo = 0, const int* emit_hi = nullptr, int arith = 0);
// fp32 -> int16 PCM rows on the device (test/main.cpp:31-33); lens (device, optional) limits each row
hipError_t launch_pcm16(const float* src, int64_t src_stride, int16_t* dst, int64_t dst_stride, const int64_t* lens, int rows, int64_t cols, hipStream_t s);

// ---- voice conversion front end (spectrogram.hip) -------------------------------------------------------------------------------
// Linear magnitude spectrogram (VITS spectrogram_torch, center = False): frame t of utterance b covers samples [t hop - pad, t hop - pad + n_fft)
// of its PCM, reflected at the utterance's own ends; out [b][bin][t] = sqrt(re^2 + im^2 + 1e-6) for t < frames[b], 0 for frames[b] <= t < tmax.
struct SpectrogramCall {
    const float* pcm = nullptr;  // device [batch][pcm_stride]
    int64_t pcm_stride = 0;
    const int* n_samples = nullptr;  // device [batch]: valid samples (pad < n_samples)
    const int* frames = nullptr;     // device [batch]
    const float2* tw = nullptr;      // device [n_fft / 2]: exp(-2 pi i m / n_fft), built in double on the host
    const float* win = nullptr;      // device [n_fft]: periodic Hann
    int n_fft = 0, hop = 0, pad = 0, bins = 0, batch = 0, tmax = 0;
    TensorRef out;
};
hipError_t launch_spectrogram(const SpectrogramCall& c, hipStream_t s);
// The STFT's geometry and tables, stated once for the engine (prepare_conversion, check_conversion_pcm) and for vits_op_spectrogram. Host arithmetic only.
// stft_geometry: empty where launch_spectrogram takes (n_fft, hop) — n_fft a power of two in [16, 2048], 1 <= hop <= n_fft, n_fft - hop even (a whole
// reflection pad on each side) —, else the cause. stft_min_samples: an utterance has at least one hop, and more samples than the pad (the reflection's reach).
std::string stft_geometry(int n_fft, int hop);
inline int stft_pad(int n_fft, int hop) { return (n_fft - hop) / 2; }
inline int stft_min_samples(int n_fft, int hop) { return std::max(hop, stft_pad(n_fft, hop) + 1); }
// tw [n_fft]: n_fft / 2 pairs (re, im) of exp(-2 pi i m / n_fft); win [n_fft]: the periodic Hann window (torch.hann_window(n)). In double, rounded once to fp32.
void stft_tables(int n_fft, std::vector<float>& tw, std::vector<float>& win);
// z_q = mean + (eps * eps_scale) * exp(log_std) over [0, frames[b]) (eps: the counter stream of prior sampling, or `noise`; eps_scale 1 is VITS's draw
// (eps * 1.0f is exact), 0 the posterior mean: no noise is drawn or read then); flip: channel c -> row channels - 1 - c
hipError_t launch_posterior_sample(TensorRef mean, TensorRef logstd, const int* frames, TensorRef noise, int noise_kind, uint64_t seed, const int* seed_off,
                                   TensorRef zq, int batch, int channels, int lmax, int flip, hipStream_t s, float eps_scale = 1.0f);
// Forced alignment (align.hip). launch_align_logp: logp [b][t_stride][l_stride] (fp32, entries t < tlens[b], j < frames[b]) from the prior statistics per
// token (mean, logs: [b][channels][t]) and z_p (z: [b][channels][j]) through the operand planes plane_a / plane_z ([b][2 channels][t_stride | l_stride]) and
// ct ([b][t_stride]); t_stride and l_stride are multiples of 32. launch_align_mas: the monotonic alignment search over logp: dur [b][dur_stride] (frames per
// token, 0 past tlens[b]), score [b], path [b][l_stride] (token of every frame, as floats; optional). `bits` (one decision bit per frame and token,
// align_mas_bits_words(tmax, lmax) 64-bit words per utterance) is needed only when align_mas_bits_in_lds(tmax, lmax) is false.
struct AlignCall {
    TensorRef mean, logs, z;
    const int* tlens = nullptr;   // device [batch]
    const int* frames = nullptr;  // device [batch]; tlens[b] <= frames[b] (checked on the host)
    int channels = 0, batch = 0, tmax = 0, lmax = 0, t_stride = 0, l_stride = 0;
    float *plane_a = nullptr, *plane_z = nullptr, *ct = nullptr, *logp = nullptr;
    unsigned long long* bits = nullptr;
    int* dur = nullptr;
    int dur_stride = 0;
    float *path = nullptr, *score = nullptr;
};
constexpr size_t kAlignLdsBitBytes = 128 * 1024;  // decision bits of one utterance stay in LDS up to this size (160 KB per CU, beside the row exchange)
size_t align_mas_bits_words(int tmax, int lmax);
bool align_mas_bits_in_lds(int tmax, int lmax);
hipError_t launch_align_logp(const AlignCall& c, hipStream_t s);
hipError_t launch_align_mas(const AlignCall& c, hipStream_t s);

// ---- sample-rate conversion (resample.hip; the filter: include/vits.h vits_resample_plan, DESIGN.md §8 "Any sample rate") ----------------
// fi -> fo as a rational L / M polyphase filter: output j of a row sits at input time j M / L; q = j M (int64), n_c = q / L, p = q % L,
// y[j] = sum_k h[p][k] x[n_c - R + k], x = 0 outside the row's own [0, len). h is a Kaiser-windowed sinc (32 zero crossings, roll-off 0.92, beta 9)
// built in double on the host and rounded once to fp32. The bits of y[j] are ONE ascending chain, acc = 0; acc = fmaf(h[p][k], x, acc) for k = 0 .. K - 1:
// nothing about tiles, batch position or the range asked for enters a sample.
constexpr int kResampleMinRate = 4000, kResampleMaxRate = 192000;
constexpr int64_t kResampleMaxTaps = (int64_t)1 << 20;  // floats of the largest table accepted (L K)
struct ResamplePlan {
    int L = 1, M = 1, R = 0, K = 1;
    double s = 1.0, W = 0.0;  // cutoff scale and half width (input samples) of the prototype
    int64_t out_len(int64_t n) const { return (n * L + M - 1) / M; }
    // the longest output prefix whose taps all lie in the final input samples [0, e) of a row of n samples (all of it once e == n: the zeros behind the
    // row's end are final)
    int64_t final_prefix(int64_t e, int64_t n) const {
        if (e >= n) return out_len(n);
        return e - R <= 0 ? 0 : std::min(out_len(n), ((e - R) * L + M - 1) / M);
    }
};
// host only. false + a message naming the cause: a rate outside [4000, 192000], or a table of more than 2^20 floats
bool resample_plan(int in_rate, int out_rate, ResamplePlan& p, std::string& err);
std::vector<float> resample_taps(const ResamplePlan& p);  // [L][K], h[p][k] = g(R - k + p / L)
constexpr int kResampleTile = 1024;  // output samples per block (halved down to 256 while the staged input span would not fit: steep downsampling)
struct ResampleCall {
    const float* x = nullptr;  // device [batch][x_stride]
    int64_t x_stride = 0;
    const int* lens = nullptr;  // device [batch]: valid input samples of each row (<= x_stride); nothing behind them is read
    const int *j0 = nullptr, *j1 = nullptr;  // device [batch], optional: the output range [j0, j1) of each row (clamped to its N_out); null = the whole row
    float* y = nullptr;  // device [batch][y_stride]; samples outside the range are left as they are
    int64_t y_stride = 0;
    const float* taps = nullptr;  // device [K][L] (the TRANSPOSE of resample_taps: threads of a wave differ in p)
    ResamplePlan plan;
    int batch = 0;
    int64_t max_range = 0;  // the longest range of the call (host side: sizes the grid)
};
hipError_t launch_resample(const ResampleCall& c, hipStream_t s);

// ---- levelling: BS.1770 loudness, sample peak and gain (loudness.hip; the definition: include/vits.h vits_model_set_level, DESIGN.md §8 "A stated level") ----
// The K-weighting cascade in transposed direct form II is the 4-state linear system v' = A v + B x, v = (s1, s2, t1, t2):
//   y1 = b0 x + s1;  s1' = b1 x - a1 y1 + s2;  s2' = b2 x - a2 y1;     y2 = d0 y1 + t1;  t1' = d1 y1 - e1 y2 + t2;  t2' = d2 y1 - e2 y2
// An utterance is cut into sub-segments of kLevelQ samples anchored at its sample 0 and into groups of kLevelGroup sub-segments: the cut, and so every bit
// of the result, depends on the utterance's own samples and length alone. Filter, sums and gates are double; the delivered sample is one fp32 multiply.
constexpr int kLevelQ = 64;      // samples per sub-segment (<= the shortest 100 ms segment, 400 at 4 kHz: a sub-segment touches at most two segments)
constexpr int kLevelGroup = 16;  // sub-segments per group of the state scan (level_scan_kernel)
struct LevelCoef {
    double c[10];   // b0 b1 b2 a1 a2 of the shelf, then of the high-pass
    double AQ[16];  // A^kLevelQ, row-major: the state after one sub-segment of zeros
    double AG[16];  // A^(kLevelQ kLevelGroup)
};
struct LoudnessPlan {
    int rate = 0, S = 0;  // S: samples per 100 ms segment, (rate + 5) / 10
    LevelCoef coef;
};
// host only (loudness_host.cpp). false + a message: a rate outside [4000, 192000]
bool loudness_plan(int rate, LoudnessPlan& p, std::string& err);
// the values a kind accepts (include/vits.h vits_model_set_level): false + a message naming the value and its range. kind: VITS_LEVEL_*
bool level_values_ok(int kind, float value_db, float ceiling_db, std::string& err);
// the definition in double, sequentially; lufs = -inf and blocks = 0 when unmeasurable
void loudness_host(const float* pcm, size_t n, const LoudnessPlan& p, double* lufs, double* peak, int* blocks);
// bytes of device scratch a measurement of `batch` rows of at most max_len samples needs (sub-segment states, partial sums, peaks, segment means)
size_t level_scratch_bytes(int batch, int64_t max_len, int S);
struct LevelCall {
    const float* x = nullptr;  // device [batch][x_stride]
    int64_t x_stride = 0;
    const int* lens = nullptr;  // device [batch]: valid samples of each row; nothing behind them is read
    int batch = 0;
    int64_t max_len = 0;  // the longest row (host side: sizes the grid and the scratch)
    LoudnessPlan plan;
    void* scratch = nullptr;  // device, level_scratch_bytes(batch, max_len, plan.S), 8-byte aligned (it holds doubles)
    int kind = 0;             // VITS_LEVEL_*
    float value_db = 0.f, ceiling_db = 0.f;
    float gain = 1.f;         // VITS_LEVEL_GAIN: (float)10^(value_db / 20), rounded on the host (the streaming windows multiply by the same float)
    float* levels = nullptr;  // device [batch][4]: L (LUFS; -inf: unmeasurable), P, g, blocks that passed both gates
};
// level_pass_kernel (states), level_scan_kernel, level_pass_kernel (sums), level_finish_kernel
hipError_t launch_level_measure(const LevelCall& c, hipStream_t s);
struct LevelScale {
    const float* x = nullptr;  // device [batch][x_stride]
    int64_t x_stride = 0;
    float* y = nullptr;  // device [batch][y_stride]; may be x
    int64_t y_stride = 0;
    const int* lens = nullptr;                // device [batch]
    const int *j0 = nullptr, *j1 = nullptr;  // device [batch], optional: the range [j0, j1) of each row (clamped to its length); null = the whole row
    const float* levels = nullptr;            // device [batch][4]: row b is multiplied by levels[4 b + 2]; null = by `gain`
    float gain = 1.f;
    int batch = 0;
    int64_t max_range = 0;  // the longest range of the call (host side: sizes the grid)
};
// y = x * g, one fp32 multiply per sample; samples outside a row's range are left as they are
hipError_t launch_level_scale(const LevelScale& c, hipStream_t s);

// ---- the loudness target under a ceiling: 4x true-peak meter and look-ahead limiter (limiter.hip; the definition: include/vits.h vits_model_set_limiter,
// DESIGN.md §8 "Under a ceiling") ----
// u = the row resampled fs -> 4 fs by the project's own filter (L = 4, M = 1, R = 35, K = 71: ResamplePlan), the same ascending fmaf chain as resample.hip;
// e[n] = max(|x[n]|, |u[4n - 2 .. 4n + 2]|); r = min(1, c / (g0 e)); m = sliding minimum of r over [j - H, j + A]; s = mean of m over [n - A, n] in fp64;
// y = x (g0 s). No recurrence: a sample depends on the row's own samples [n - H - A - R - 1, n + A + R] alone. Tiles of kLimitTile samples are anchored at
// the row's sample 0, nothing is accumulated with atomics, and only minima, maxima and integer counts cross a tile: no bit depends on the cut either.
constexpr int kLimitTile = 2048;      // samples of a row per block, in every kernel of limiter.hip
constexpr int kLimitMaxRate = 48000;  // 4 fs must be a rate the resampler accepts
constexpr int kLimitMaxA = (kLimitMaxRate + 100) / 200, kLimitMaxH = (kLimitMaxRate + 10) / 20;
struct LimiterPlan {
    int rate = 0;
    int A = 0;  // (rate + 100) / 200: 5 ms of look-ahead and attack
    int H = 0;  // (rate + 10) / 20: 50 ms of hold
    int tile = kLimitTile;
    ResamplePlan up;  // rate -> 4 rate
};
// host only (limiter_host.cpp). false + a message: a rate outside [4000, 48000]
bool limiter_plan(int rate, LimiterPlan& p, std::string& err);
// the definition in double, sequentially. taps: resample_taps(p.up), [4][K]. y (optional) gets n samples; limits = {TP(x), TP(y), min s, share of s < 1}
void limiter_host(const float* pcm, size_t n, const LimiterPlan& p, const float* taps, double g0, double c, double* y, double limits[4]);
// bytes of device scratch: the envelope [batch][max_len], two tile maxima and the tile statistics
size_t limit_scratch_bytes(int batch, int64_t max_len);
struct LimitCall {
    const float* x = nullptr;  // device [batch][x_stride]
    int64_t x_stride = 0;
    float* y = nullptr;  // device [batch][y_stride], not x: row b gets its lens[b] samples, the rest is left as it was
    int64_t y_stride = 0;
    const int* lens = nullptr;  // device [batch]; nothing behind a row's samples is read
    int batch = 0;
    int64_t max_len = 0;  // the longest row (host side: sizes the grid and the scratch)
    LimiterPlan plan;
    const float* taps = nullptr;  // device [K][4]: the table ResampleCall takes for rate -> 4 rate
    void* scratch = nullptr;      // device, limit_scratch_bytes(batch, max_len)
    int kind = 0;                 // VITS_LEVEL_GAIN, _PEAK or _LOUDNESS
    float value_db = 0.f;
    float gain = 1.f;     // VITS_LEVEL_GAIN: (float)10^(value_db / 20), rounded on the host
    float ceiling = 1.f;  // c = (float)10^(ceiling_db / 20)
    float* levels = nullptr;  // device [batch][4], filled by launch_level_measure: row[2] is REPLACED by g0 (no ceiling rule; true-peak normalisation)
    float* limits = nullptr;  // device [batch][4], out: TP(x), TP(y), min s, share of samples with s < 1
};
// meter(x), g0 and TP per row, then the limiter (GAIN, LOUDNESS) or the plain multiply (PEAK), then meter(y) and the rows
hipError_t launch_limit(const LimitCall& c, hipStream_t s);

// ---- stated edges: trimmed silence, pauses and fades (edges.hip; the definition: include/vits.h vits_model_set_edges, DESIGN.md §8 "Stated edges") ----
// Windows of W = (rate + 50) / 100 samples anchored at the row's sample 0; q_i = the mean of x^2 over window i in fp64; a window is active iff q_i >= T and
// q_i > 0 (T = q_max f or f, f = 10^(threshold_db / 10)); [a, b) = the first to the last active window widened by the keep margins; the delivered row is
// Pl zeros, x[a, b) under the two fade tables, Pt zeros. The sum of a window is ONE shape: lane l of a wave adds the squares of the window's samples l,
// l + 64, .. in ascending order, then the 64 partial sums meet in a butterfly (xor 32, 16, .. 1). It depends on the window's own samples and count alone.
constexpr int kEdgesTileTarget = 4096;  // samples of a row per block of edges_window_kernel: the largest multiple of W at or under it
constexpr int kEdgesApplyTile = 1024;   // delivered samples per block of edges_apply_kernel
constexpr int64_t kEdgesMaxLen = (int64_t)1 << 30;
struct EdgesPlan {
    int rate = 0, mode = 0;  // VITS_EDGES_*
    int W = 0;               // (rate + 50) / 100: 10 ms
    int64_t Kh = 0, Kt = 0, Fi = 0, Fo = 0, Pl = 0, Pt = 0;  // samples(ms) of the desc's six durations, in field order
    int tile = 0;    // (kEdgesTileTarget / W) W
    double f = 1.0;  // 10^(threshold_db / 10), computed once on the host
    int64_t bound(int64_t n) const { return n + Pl + Pt; }
};
// host only (edges_host.cpp). false + a message: a rate outside [4000, 192000], a wrong struct_size, an unknown mode, a value that is not finite or out of range
bool edges_plan(int rate, const ::vits_edges_desc& d, EdgesPlan& p, std::string& err);
// the two fade tables, win[Fi] then wout[Fo]: 0.5 - 0.5 cos(pi (k + 0.5) / F) in double, rounded once to fp32
std::vector<float> edges_fades(const EdgesPlan& p);
// the definition, sequentially. y (optional, at least p.bound(n) floats) gets the delivered row and zeros up to the bound; row = {a, b, N', n_active}
void edges_host(const float* pcm, int64_t n, const EdgesPlan& p, const float* fades, float* y, int64_t row[4]);
// bytes of device scratch: q [batch][ceil(max_len / W)] doubles
size_t edges_scratch_bytes(int batch, int64_t max_len, int W);
struct EdgesCall {
    const float* x = nullptr;  // device [batch][x_stride]
    int64_t x_stride = 0;
    const int* lens = nullptr;  // device [batch]: valid samples of each row; nothing behind them is read
    float* y = nullptr;         // device [batch][y_stride], not x: row b gets plan.bound(lens[b]) samples, the rest is left as it was
    int64_t y_stride = 0;
    int batch = 0;
    int64_t max_len = 0;  // the longest row (host side: sizes the grids and the scratch); y_stride >= plan.bound(max_len)
    EdgesPlan plan;
    const float* fades = nullptr;  // device [Fi + Fo]: edges_fades (null when both are 0)
    void* scratch = nullptr;       // device, edges_scratch_bytes(batch, max_len, plan.W), 8-byte aligned (unused under VITS_EDGES_PAD)
    int* lens_out = nullptr;       // device [batch]: N' of each row
    int64_t* rows = nullptr;       // device [batch][4]: a, b, N', n_active
};
// the three passes, in this order on one stream: q of every window (not under VITS_EDGES_PAD) | one block per row: q_max, T, the first and the last active
// window, the rows | the shifted copy with the fades, the pads and the zeros up to the bound
hipError_t launch_edges_window(const EdgesCall& c, hipStream_t s);
hipError_t launch_edges_bounds(const EdgesCall& c, hipStream_t s);
hipError_t launch_edges_apply(const EdgesCall& c, hipStream_t s);

// ---- joined tracks: the utterances of a batch laid end to end (join.hip; the definition: include/vits.h "joined tracks", DESIGN.md §8 "Joined
// tracks") ----
// Utterance b of track g lies at o_b: 0 for the first of a track, else o_(b-1) + n_(b-1) + step_b, step_b = g_b for a gap g_b >= 0 and
// -min(-g_b, n_(b-1) / 2, n_b / 2) for an overlap. The half rule makes o_b and o_b + n_b non-decreasing along a track, and lets at most two utterances, always
// neighbours, cover a sample: y is +0, a copy, or one fp32 add.
constexpr int kJoinTile = 1024;  // samples of a track per block of join_apply_kernel
constexpr float kJoinMinGapMs = -2000.f, kJoinMaxGapMs = 60000.f;
struct JoinPlan {
    int rate = 0, batch = 0, tracks = 0;
    std::vector<int> first;       // [tracks + 1]: track g holds the utterances [first[g], first[g + 1])
    std::vector<int64_t> gap;     // [batch]: g_b in samples; 0 for the first utterance of a track (validated and ignored)
    std::vector<int64_t> ubound;  // [batch]: what the host knows of n_b (the device clamps n_b to it); empty until join_bounds
    std::vector<int64_t> bound;   // [tracks]: the sum of the track's ubound and of its positive gaps; empty until join_bounds
    int64_t max_bound = 0, max_ubound = 0;
};
// host only (join_host.cpp). join_plan: the tracks and the gaps. false + a message: a rate outside [4000, 192000], batch outside [1, 65535], track[0] != 0 or a step
// other than 0 or 1, a gap that is not finite or outside [-2000, 60000] ms (naming the utterance), a track whose positive gaps alone pass kEdgesMaxLen. track NULL: one track; gap_ms NULL: 0 everywhere
bool join_plan(int rate, int batch, const int32_t* track, const float* gap_ms, JoinPlan& p, std::string& err);
// ... and the bounds, once the host knows every utterance's. false + a message: an utterance bound outside [0, kEdgesMaxLen], a track bound above kEdgesMaxLen
bool join_bounds(JoinPlan& p, const int64_t* utt_bounds, std::string& err);
// the table the kernels read, int64: [batch][2] = {g_b, ubound_b}, then [tracks][3] = {first, end, bound}
std::vector<int64_t> join_table(const JoinPlan& p);
inline size_t join_table_elems(int batch, int tracks) { return (size_t)2 * batch + (size_t)3 * tracks; }
// the definition, sequentially: lens [batch] (clamped to [0, ubound_b] as the device does), x [batch][x_stride] -> y [tracks][y_stride] (optional: row g gets
// bound_g samples), track_lens [tracks] = T_g, rows [batch][2] = {o_b, n_b} (both optional)
void join_host(const JoinPlan& p, const float* x, int64_t x_stride, const int64_t* lens, float* y, int64_t y_stride, int64_t* track_lens, int64_t* rows);
// vits_split_sentences (include/vits.h): the spans of a text, in bytes; returns how many there are (the first `cap` of them are written)
int64_t split_sentences(const char* text, int64_t* starts, int64_t* ends, int32_t* kinds, size_t cap);
// vits_model_speak's host side (join_host.cpp; no device, no model: the tokenizer comes in as a function): the text cut by split_sentences, every span
// tokenised, the spans that have ids as ONE batch for vits_model_process_joined. A span without ids is dropped; if it ended its paragraph, the kept span in
// front of it does. Kept span k > 0 gets paragraph_gap_ms when the kept span in front of it ended a paragraph (and, track_per_paragraph, opens the next
// track), else sentence_gap_ms. false + a message: a NULL or empty text, a gap that is not finite or outside vits_join_plan's range, what the tokenizer
// refuses, a span above kSpeakMaxIds ids (naming the span), no span with ids at all, more than 65535 of them.
constexpr int kSpeakMaxIds = 2048;
struct SpeakPlan {
    int batch = 0, id_stride = 0;
    std::vector<int32_t> index;    // [batch]: the span's index in split_sentences order
    std::vector<int32_t> track;    // [batch]
    std::vector<float> gap_ms;     // [batch]: 0 for the first span
    std::vector<int32_t> id_lens;  // [batch]
    std::vector<int32_t> ids;      // [batch][id_stride]: 0 past a span's length
};
typedef bool (*SpeakTokenize)(void* user, const std::string& span, std::vector<int32_t>& ids, std::string& err);
bool speak_plan(const char* text, float sentence_gap_ms, float paragraph_gap_ms, bool track_per_paragraph, SpeakTokenize tokenize, void* user, SpeakPlan& p,
                std::string& err);
struct JoinCall {
    const JoinPlan* plan = nullptr;  // host: what the table was made from (join_call_ok checks every index the kernels take from it)
    const float* x = nullptr;        // device [batch][x_stride]
    int64_t x_stride = 0;
    const int* lens = nullptr;  // device [batch]: valid samples of each row; nothing behind min(lens[b], ubound_b) is read
    float* y = nullptr;         // device [tracks][y_stride], not x: row g gets bound_g samples, the rest is left as it was
    int64_t y_stride = 0;
    const int64_t* table = nullptr;  // device: join_table(plan), 8-byte aligned
    int64_t* rows = nullptr;         // device [batch][2]: o_b, n_b
    int* track_lens = nullptr;       // device [tracks]: T_g
};
// the two passes, in this order on one stream: one block per track walks its utterances (rows, track_lens) | grid (tiles of the largest bound, tracks): a
// binary search over the monotone ends for the first utterance that reaches the tile, then a walk forward; every sample of [0, bound_g) is written once
hipError_t launch_join_offsets(const JoinCall& c, hipStream_t s);
hipError_t launch_join_apply(const JoinCall& c, hipStream_t s);

// ---- a stated pitch: varispeed by a ratio per row (pitch.hip; the definition: include/vits.h "a stated pitch", DESIGN.md §8 "A stated pitch") ----
// Row b of N samples is played back p_b times faster: P = p 2^24 (an integer for every float in [0.5, 2]), N' = ceil(N 2^24 / P), output m sits at t = m P
// (64-bit), n0 = t >> 24, f = t & (2^24 - 1). The prototype is the resampler's (Kaiser-windowed sinc, Z = 32, beta = 9, rolloff 0.92), tabulated at Q = 256
// points per zero crossing with its fp32 differences, and read with linear interpolation at an integer index: nothing about a tap's weight is floating point
// until fmaf(fr, D[i], G[i]). y[m] is ONE ascending chain of K = 2 R + 1 fused multiply-adds; a row with P = 2^24 is copied bit for bit.
constexpr int kPitchZ = 32, kPitchQ = 256, kPitchTableN = kPitchZ * kPitchQ + 2;  // G and D hold kPitchTableN floats each
constexpr int64_t kPitchOne = (int64_t)1 << 24;
constexpr int64_t kPitchS0 = 15435038;  // floor(0.92 2^24)
constexpr float kPitchMinRatio = 0.5f, kPitchMaxRatio = 2.0f;
constexpr int64_t kPitchMaxLen = (int64_t)1 << 30;
constexpr int kPitchMaxR = 70;  // R at the largest ratio (K = 141)
struct PitchPlan {
    int64_t P = kPitchOne, S = kPitchS0;
    int R = 35, K = 71;
    int64_t n_out = 0;
};
// host only (pitch_host.cpp). false + a message: a ratio that is not finite or outside [0.5, 2], n outside [0, 2^30]
bool pitch_plan(float ratio, int64_t n, PitchPlan& p, std::string& err);
// [2][kPitchTableN]: G, then D
std::vector<float> pitch_table();
// ... and as the kernel reads it, [kPitchTableN][2] = {G[i], D[i]}
std::vector<float> pitch_table_pairs();
// the definition in double, sequentially; y gets p.n_out samples
void pitch_host(const float* x, int64_t n, const PitchPlan& p, const float* table, double* y);
constexpr int kPitchTile = 1024;  // output samples per block
struct PitchCall {
    const float* x = nullptr;  // device [batch][x_stride]
    int64_t x_stride = 0;
    const int* lens = nullptr;      // device [batch]: valid input samples of each row (<= x_stride); nothing behind them is read
    const float* ratios = nullptr;  // device [batch]: p_b, each in [0.5, 2] (the host's check; the kernel clamps, so that no index depends on it)
    float* y = nullptr;             // device [batch][y_stride], not x; samples behind N' are left as they are
    int64_t y_stride = 0;
    const float* table = nullptr;  // device [kPitchTableN][2]: {G[i], D[i]} (pitch_table INTERLEAVED: one 8-byte load per tap)
    int* lens_out = nullptr;       // device [batch], optional: N' of each row
    int batch = 0;
    int64_t max_out = 0;  // the longest output row of the call (host side: sizes the grid); y_stride >= max_out
};
hipError_t launch_pitch(const PitchCall& c, hipStream_t s);

// ---- a stated tempo: pitch-preserving time stretch by a tempo per row (tempo.hip; the definition: include/vits.h "a stated tempo", DESIGN.md §8 "A stated tempo") ----
// Waveform-similarity overlap-add with every decision in integers. Row b of N samples at the rate sr is played q_b times faster: Q = q 2^24, N' = ceil(N 2^24 / Q),
// hop and cross-fade H = 4 floor(sr / 400), search radius D = 4 floor(sr / 500), F = ceil(N' / H) segments. Segment k starts at s_k = a_k + delta_k, a_k =
// (k H Q) >> 24, where delta_k in [-D, D] is the first minimum, in the order 0, -1, +1, -2, ..., of the sum of absolute differences between the 16-bit
// quantised row at s_(k-1) + H (where the segment before would go on) and at a_k + delta. y[k H + i] = v[i] x[s_(k-1) + H + i] + w[i] x[s_k + i], two rounded
// products and one rounded add, w[i] = (2 i + 1) / (2 H), v[i] = w[H - 1 - i]; a row with Q = 2^24 is copied bit for bit.
constexpr int64_t kTempoOne = (int64_t)1 << 24;
constexpr float kTempoMin = 0.5f, kTempoMax = 2.0f;
constexpr int kTempoMinRate = 8000, kTempoMaxRate = 48000;
constexpr int64_t kTempoMaxLen = (int64_t)1 << 30;
constexpr int kTempoMaxH = 4 * (kTempoMaxRate / 400), kTempoMaxD = 4 * (kTempoMaxRate / 500);  // 480, 384
struct TempoPlan {
    int H = 0, D = 0;
    int64_t Q = kTempoOne;
    int64_t F = 0, n_out = 0;
};
// host only (tempo_host.cpp). false + a message: a rate outside [8000, 48000], a tempo that is not finite or outside [0.5, 2], n outside [0, 2^30]
bool tempo_plan(int rate, float tempo, int64_t n, TempoPlan& p, std::string& err);
// the definition, sequentially: y gets p.n_out samples, offsets (optional) delta_k for k = 1 ... F
void tempo_host(const float* x, int64_t n, const TempoPlan& p, float* y, int32_t* offsets);
constexpr int kTempoTile = 1024;  // output samples per block of the overlap-add
struct TempoCall {
    const float* x = nullptr;  // device [batch][x_stride]
    int64_t x_stride = 0;
    const int* lens = nullptr;      // device [batch]: valid input samples of each row (<= x_stride); nothing behind them is read
    const float* tempos = nullptr;  // device [batch]: q_b, each in [0.5, 2] (the host's check; the kernels clamp, so that no index depends on it)
    int rate = 0;                   // sr, in [8000, 48000]
    int* starts = nullptr;          // device [batch][starts_stride]: s_0 ... s_F of each row, written by the search and read by the overlap-add
    int64_t starts_stride = 0;      // >= the largest F + 1
    int* offsets = nullptr;         // device [batch][offsets_stride], optional: delta_1 ... delta_F of each row
    int64_t offsets_stride = 0;
    float* y = nullptr;  // device [batch][y_stride], not x; samples behind N' are left as they are
    int64_t y_stride = 0;
    int* lens_out = nullptr;  // device [batch], optional: N' of each row
    int batch = 0;
    int64_t max_out = 0;  // the longest output row of the call (host side: sizes the grid); y_stride >= max_out
};
hipError_t launch_tempo_search(const TempoCall& c, hipStream_t s);
hipError_t launch_tempo_ola(const TempoCall& c, hipStream_t s);

// ---- a stated duration: the length scale fitted to a target frame count (fit.hip; the definition: include/vits.h "a stated duration") ----
// A group is a set of utterances of one call. Token t has e_t = expf(logw_t) and fixed_t (the caller's override, or -1). A free token lasts
// c_t(s) = (int64) min(ceilf(e_t * s), 2^24) frames at the scale s, a fixed one fixed_t; n(s) = sum c_t(s) is non-decreasing in the bit pattern of s > 0.
// s* = the largest float in [s_lo, s_hi] with n(s*) <= F (s_lo = (float)(1.0 / max_rate), s_hi = (float)(1.0 / min_rate)), found by bisection on the bit
// patterns; the R = F - n(s*) frames left go to the free tokens in (utterance, token) order, token t taking min(c_t(next s) - c_t(s*), what is left).
// status: 0 = the group lasts F frames, 1 = s* = s_lo and n > F, 2 = s* = s_hi and n < F, -1 = the group was not fitted (target 0).
constexpr int64_t kFitMaxTarget = (int64_t)1 << 22;
constexpr float kFitMaxTokenFrames = 16777216.f;
constexpr float kFitMinRate = 0.1f, kFitMaxRate = 10.f;
constexpr int kFitRowInts = 5;  // a group's row: {F, sum d, the bits of s*, R, status}, int64 each
struct FitGroups {
    const int* group = nullptr;       // [batch]: the group of every utterance, in [0, batch); NULL: utterance b is group b
    const int* target = nullptr;      // [batch], by group: F, or 0 = not fitted
    float s_lo = 1.f, s_hi = 1.f;
};
// the two scale limits; false + a message: rates that are not finite, outside [0.1, 10] or min_rate > max_rate
bool fit_limits(float min_rate, float max_rate, float& s_lo, float& s_hi, std::string& err);
// host only (fit_host.cpp): e, fixed (or NULL) and dur [batch][t_stride], lens [batch] (or NULL: t_stride each), rows [batch][kFitRowInts] by group. dur gets
// d_t of every token of a fitted utterance, fixed_t (or -1) of every other token and -1 behind every length. The values are the caller's to check (fit_check).
void fit_host(int batch, int t_stride, const float* e, const int* fixed, const int* lens, const FitGroups& g, int* dur, int64_t* rows);
// false + a message naming the group or the utterance: a group outside [0, batch), a target outside [1, 2^22] and not 0
bool fit_check(int batch, const int* group, const int64_t* target, std::string& err);  // (the caller's 64-bit targets; FitGroups holds them as ints)
// ... a batch or a stride below 1, a length outside [0, t_stride], a fixed value below -1 or above 2^24 in front of a length
bool fit_check_rows(int batch, int t_stride, const int* fixed, const int* lens, std::string& err);
// group rows as the entry points hand them out: double [groups][kFitRowInts] = {F, sum d, s* (0 where status is -1), R, status}
void fit_rows_double(int groups, const int64_t* rows, double* out);
struct FitCall {
    TensorRef logw;              // [batch][rows][t]: row c is read
    int c = 0;
    const int* lens = nullptr;   // device [batch] (or NULL: tmax each); nothing behind a length is read
    const int* fixed = nullptr;  // device [batch][tmax] (or NULL): the caller's override rows
    FitGroups g;                 // device pointers
    float* e = nullptr;          // device [batch][tmax]: e_t of every token (scratch of the search, and the tap)
    int* dur = nullptr;          // device [batch][tmax]: the override rows launch_durations then takes
    int64_t* rows = nullptr;     // device [batch][kFitRowInts]
    int batch = 0, tmax = 0;
};
hipError_t launch_fit_durations(const FitCall& c, hipStream_t s);

}  // namespace vits

#include "conv_plan.h"  // the convolutions' launch policy (plan_conv, plan_conv16): host arithmetic over the types above
#include "launch_plan.h"  // launch policy and geometry of the fused kernels: vocoder resblocks and upsamplers, the flow, attention / LayerNorm / DDS
