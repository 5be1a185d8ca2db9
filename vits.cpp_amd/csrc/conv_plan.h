// conv_plan.h — the launch policy of the four convolution families (conv_mfma.hip, conv16.hip, conv16_lat.hip, conv_split.hip) as plain host
// arithmetic: geometry helpers, which instantiations exist, and one plan per launch (conv_plan.cpp). No kernels, no HIP calls: the launchers in
// the .hip files copy fields and launch what the plan says; tests/conv_plan_dump.cpp links conv_plan.o alone and freezes the policy as a table.
#pragma once
#include "kernels.h"

namespace vits {

// ---- geometry, each rule once ------------------------------------------------------------------------------------------------------
constexpr int kConvCK = 32;  // input channels per LDS chunk (conv_mfma.hip's CK)
constexpr int kNoKernel = -99;  // conv_template_dil / conv16_template_dil: no dispatcher arm for this (epilogue, taps)
#ifndef VITS_XWP_GRAN
#define VITS_XWP_GRAN 16  // LDS row pitch granularity of conv_mfma's producer-wave path (see the kernel)
#endif
// GEMM columns of a launch's grid: the transposed conv's q runs over [0, L_in]
template <class Call>
inline int conv_ncols(const PackedConv& w, const Call& c) { return w.epi == EPI_CONVT ? c.t_in + 1 : c.t_out; }
// the dilation the kernel sees: -1 for the transposed conv (tap m reads x[q - m]), 1 for a 1x1 conv
template <class Call>
inline int conv_dil(const PackedConv& w, const Call& c) { return w.epi == EPI_CONVT ? -1 : (w.kt == 1 ? 1 : c.dil); }
struct TileShape {
    int wm, wn, mr, nr;
    constexpr int bn() const { return wn * nr * 32; }  // columns per block
    constexpr int bm() const { return wm * mr; }       // 32-row tiles per block
};
constexpr TileShape tile_shape(int tile) {
    switch (tile) {
        case TILE_128x128: return {2, 2, 2, 2};
        case TILE_64x256: return {1, 4, 2, 2};
        case TILE_32x256: return {1, 4, 1, 2};
        case TILE_64x64: return {1, 4, 2, 1};  // 64 x 128
        case TILE_LAT16:  // (conv_lat16_kernel has its own grid; parameters are set up as for the narrow tile)
        case TILE_NARROW: return {4, 1, 1, 1};  // 128 x 32: four row tiles of ONE 32-column strip
        default: return {1, 4, 1, 1};          // TILE_32x64: 32 x 128
    }
}
constexpr TileShape tile16_shape(int tile) {
    switch (tile) {
        case 0: return {2, 2, 2, 4};  // 128 x 256
        case 1: return {1, 4, 2, 2};  // 64 x 256
        case 2: return {1, 4, 1, 2};  // 32 x 256
        case 3: return {1, 4, 2, 1};  // 64 x 128
        case 5: return {2, 2, 2, 2};  // 128 x 128
        case 6: return {4, 1, 1, 4};  // 128 x 128, one row tile per wave: every A fragment feeds 4 MFMAs
        default: return {1, 4, 1, 1};  // 32 x 128
    }
}
// The tiles whose kernels can run over a list of existing tiles instead of the dense grid (tile_map.h): the throughput tiles, four 32 x 32 accumulators per wave.
// The small tiles serve the latency-bound launches; their kernels are compiled with the dense decode alone (their scalar registers are full).
constexpr bool conv_tile_mapped(int tile) { return tile != TILE_LAT16 && tile != TILE_NARROW && tile_shape(tile).mr * tile_shape(tile).nr >= 4; }
inline int64_t tile_blocks(TileShape t, int ncols, int mtiles_used, int batch) {
    return (int64_t)((ncols + t.bn() - 1) / t.bn()) * ((mtiles_used + t.bm() - 1) / t.bm()) * batch;
}
constexpr int padded_xw(int xw) { return (xw + 3 + VITS_XWP_GRAN - 1) / VITS_XWP_GRAN * VITS_XWP_GRAN; }  // (+3: 16-byte aligned origin)
constexpr int lat16_pitch(int span) { return span <= 4 ? 24 : span <= 20 ? 40 : span <= 52 ? 72 : 0; }  // conv_lat16_kernel's instantiated LDS pitches (0: none)
constexpr int kLnLoadMaxCin = 3 * 256;  // LayerNorm on load (conv_lat16_kernel): every thread of the block stages three elements of gamma and of beta
constexpr int conv16_lat_pitch(int nr, int kt, int dil) { return (32 * nr + (kt - 1) * dil + 7) / 8 * 8; }
// GEMM shape of a conv's packed weights (pack_conv_weights / pack_conv_weights16): the row tiles are padded so that every tile shape (1, 2 or 4 per block) divides them
struct ConvPackDims {
    int rows, kt, mtiles_used, mtiles, nchunks;
};
inline ConvPackDims conv_pack_dims(int cout, int cin, int k, int epi, int ct_stride) {
    ConvPackDims d;
    d.rows = epi == EPI_CONVT ? cout * ct_stride : cout;
    d.kt = epi == EPI_CONVT ? k / ct_stride : k;  // (transposed: == 2 taps per phase)
    d.mtiles_used = epi == EPI_GATE ? 2 * ((cout / 2 + 31) / 32) : (d.rows + 31) / 32;
    d.mtiles = (d.mtiles_used + 3) / 4 * 4;
    d.nchunks = (cin + kConvCK - 1) / kConvCK;
    return d;
}

// ---- which instantiations exist: the launchers' `if constexpr` and the planner's fallbacks read the same predicate ----------------------
// conv_mfma_kernel<KT, DIL, DB, tile, EPI>. Compile-time dilation for the combinations the MMS architecture uses; run-time dilation (0) otherwise
constexpr int conv_template_dil(int epi, int kt, int dil) {
#ifdef VITS_MICRO_KT  // developer microbenchmark (tools/conv_micro.hip): a single (taps, dilation) pair
    return VITS_MICRO_DIL;
#else
    if (epi == EPI_CONVT) return kt == 2 ? -1 : kNoKernel;
    if (epi == EPI_GATE) return kt != 5 ? kNoKernel : dil == 1 ? 1 : 0;
    if (kt == 1) return 1;
    if (kt == 5) return dil == 1 ? 1 : 0;
    if (kt == 3 || kt == 7 || kt == 11) return dil == 1 || dil == 3 || dil == 5 ? dil : 0;
    return kNoKernel;
#endif
}
// the layers of the narrow tile (at dilation 1): encoder / flow convs; gated conv: tanh / sigmoid row tiles on wave pairs, see the epilogue. By taps alone, as the
// planner's tiny-grid step asks: a standard conv with 2 taps has no tile kernel, and conv_lat16_kernel (taps at run time) takes it from there
constexpr bool conv_narrow_shape(int epi, int kt) { return (epi == EPI_STD && kt <= 3) || (epi == EPI_GATE && kt == 5); }
constexpr bool conv_tile_exists(int epi, int kt, int dil_ct, bool db, int tile) {
    switch (tile) {
        case TILE_64x256:
        case TILE_64x64: return true;
        case TILE_NARROW: return db && dil_ct == 1 && conv_narrow_shape(epi, kt);  // (on the producer-wave path only)
        case TILE_LAT16: return false;  // (conv_lat16_kernel: conv_lat16_exists)
        default: return epi != EPI_GATE;  // 128 x 128, 32 x 256, 32 x 128: the gate keeps its tanh / sigmoid row pairing (MR == 2)
    }
}
constexpr bool conv_lat16_exists(int epi, int pitch) { return pitch && (epi == EPI_STD || (epi == EPI_GATE && pitch == 24)); }
// conv16_kernel<KT, DIL, tile, EPI>: the epilogues of conv16.hip (its Epi16) ...
enum Conv16Epi : int { C16_STD = 0, C16_GATE = 1, C16_CONVT = 2, C16_GROUP = 3, C16_CONVT_GROUP = 4 };
constexpr int conv16_template_dil(int epi16, int kt, int dil) {
    const bool rb = kt == 3 || kt == 7 || kt == 11;
    if (epi16 == C16_CONVT || epi16 == C16_CONVT_GROUP) return kt == 2 ? -1 : kNoKernel;
    if (epi16 == C16_GATE) return kt == 5 || kt == 3 ? 0 : kNoKernel;
    if (kt == 1) return 1;
    if (epi16 == C16_STD) return rb || kt == 5 ? 0 : kNoKernel;
    return rb ? (dil == 1 || dil == 3 || dil == 5 ? dil : 0) : kt == 5 ? 0 : kNoKernel;
}
// ... and which tiles exist for which: the standard-layout epilogues (stage one, flow, transparent fallback) only come in the 64- and 32-row
// tiles; the gate needs MR == 2; run-time-dilation variants skip the 128-row tiles
constexpr bool conv16_tile_exists(int epi16, int dil_ct, int tile) {
    const bool group = epi16 == C16_GROUP || epi16 == C16_CONVT_GROUP;
    switch (tile) {
        case 0:
        case 5:
        case 6: return group && dil_ct != 0;
        case 1:
        case 3: return true;
        case 2: return group;
        default: return epi16 != C16_GATE;
    }
}
// conv16_lat_kernel<KT, C, WM, NR> / conv16_lat_group_kernel<256, WM, NR>: block shapes as 10 WM + NR (VITS_LAT16H_SHAPE / VITS_LAT16H_GROUP_SHAPE)
constexpr bool conv16_lat_shape_exists(int shape, bool group) { return shape == 21 || shape == 22 || shape == 42 || (group && shape == 41); }

// ---- one plan per launch --------------------------------------------------------------------------------------------------------------
struct ConvPlan {
    bool ok = false;  // false: launch_conv refuses (input tile too wide for LDS, taps past the staged columns, no such instantiation)
    int tile = 0;     // ConvTile; TILE_LAT16 = conv_lat16_kernel, every other the MFMA tile kernel
    int dil = 1;      // what the kernel sees (conv_dil)
    int dil_ct = 0;   // template dilation (0: run-time variant)
    bool db = false;  // producer-wave variant
    int gx = 0, gy = 0, gz = 0, block = 0;
    size_t lds = 0;
    int xw = 0, lds_off = 0, nbuf = 2, oneshot = 0;
    int pitch = 0;       // conv_lat16_kernel's LDS pitch for these taps (0: none)
    bool ln_ok = false;  // LayerNorm on load admissible (ConvCall::ln_gamma)
    const char* ln_why = nullptr;  // !ln_ok: the first condition that fails
};
ConvPlan plan_conv(const PackedConv& w, const ConvCall& c, int forced_tile = -1);  // (forced_tile: the grouped launch's members, always 128 x 128)
// block shape, pitch, grid and LDS bytes of a conv16_lat launch: `cin` channels in, `cout` rows out, grid z = `nz`
struct Conv16LatPlan {
    int wm = 0, nr = 0, pitch = 0, gx = 0, gy = 0, gz = 0, block = 0;
    size_t lds = 0;
};
Conv16LatPlan plan_conv16_lat(int cin, int cout, int kt, int dil, int shape, int tmax, int nz);
Conv16LatPlan plan_conv16_lat_group(int dil, int tmax, int batch);  // the grouped launch of a C = 256 stage's k = 3, 7, 11 convs: the LDS of the widest member (VITS_LAT16H_GROUP_SHAPE)
struct Conv16Plan {
    bool ok = false;
    bool lat = false;  // conv16_lat_kernel (profile tile tag T7): `l` says how; otherwise conv16_kernel on `tile`
    int epi16 = 0, chosen = 0, tile = 0;  // chosen: by shape and grid; tile: after the steps to an instantiation that exists
    int part = 0;  // the dispatcher (translation unit) that holds the instantiation
    int dil = 1, dil_ct = 0, gx = 0, gy = 0, gz = 0;
    size_t lds = 0;
    int xwp = 0, lds_off = 0, nbuf = 2;
    Conv16LatPlan l;
};
Conv16Plan plan_conv16(const PackedConv& w, const Conv16Call& c);

}  // namespace vits
