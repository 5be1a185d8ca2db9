// launch_plan.h — the launch policy of the fused kernels — the vocoder's (rbpair16.hip, rbblock16.hip, rbpair32.hip, rbblock32.hip, convt16.hip), the flow's
// (wavenet32.hip) and stage one's attention, LayerNorm and DDS layers (attention.hip, layer_norm.hip, dds.hip, stage1_lat.hip) — as plain host arithmetic, beside conv_plan.h: one constexpr geometry function per family, read by the kernel body AND by the planner; which instantiations exist; one
// plan per launch (launch_plan.cpp). No kernels, no HIP calls: the launchers copy fields and launch what the plan says; tests/launch_plan_dump.cpp links
// launch_plan.o alone and freezes the policy as a table. The knobs of these families are read in launch_plan.cpp and nowhere else.
#pragma once
#include "kernels.h"

namespace vits {

// ---- geometry, each rule once ------------------------------------------------------------------------------------------------------
constexpr int round_up(int v, int m) { return (v + m - 1) / m * m; }
constexpr int blocks_for(int cols, int per_block) { return (cols + per_block - 1) / per_block; }

// rbpair16_kernel<KT, DIL, C, NR, BF, ROWS>: ROWS (C >= 128) = one 32-row tile per wave over all 32 NR columns; otherwise four waves of NR column tiles each
struct RbPair16Geom {
    bool rows;
    int bm, bo, xwp, tw, block;  // mid columns / output columns per block, x tile and t tile pitch (16-byte slots), threads
    size_t lds;                      // C >= 64: the t tile takes the x tile's place
};
constexpr RbPair16Geom rbpair16_geom(int KT, int DIL, int C, int NR) {
    const bool rows = C >= 128;
    const int bm = (rows ? 1 : 4) * NR * 32, xwp = round_up(bm + (KT - 1) * DIL, 8), tw = round_up(bm + KT - 1, 8);
    return {rows, bm, bm - (KT - 1), xwp, tw, rows ? 2 * C : 256, (size_t)(C / 8) * (C >= 64 ? (xwp > tw ? xwp : tw) : xwp + tw) * 16};
}
#ifndef VITS_RB16_NARROW_NR
#define VITS_RB16_NARROW_NR 2
#endif
constexpr bool rbpair16_exists(int KT, int DIL, int C, int NR) {
    return (KT == 3 || KT == 7 || KT == 11) && (DIL == 1 || DIL == 3 || DIL == 5) &&
           (C == 32 || C == 64 ? NR == 2 : (C == 128 || C == 256) && (NR == 4 || NR == VITS_RB16_NARROW_NR));
}

// rbblock16_body<KT, C, NSTRIP, NRW, MRW, D0, D1, D2, BF, STREAM>: NSTRIP column strips x C / (32 MRW) row groups of waves, NRW 32-column tiles per strip
struct RbBlock16Geom {
    int w, p2, h, bo, adv, padx, pitch, block;  // tile columns, half taps, halo per side, outputs of a first / of every later tile, padding, LDS pitch, threads
    int c;
    constexpr size_t lds(bool stream) const { return (size_t)(c / 8) * pitch * 16 + (size_t)6 * c * sizeof(float) + (stream ? (size_t)(c / 8) * h * 16 : 0); }
    constexpr int seg_out(int nt) const { return bo + (nt - 1) * adv; }  // output columns of a segment of nt tiles
};
constexpr RbBlock16Geom rbblock16_geom(int KT, int C, int NSTRIP, int NRW, int MRW, int D0 = 1, int D1 = 3, int D2 = 5) {
    const int w = NSTRIP * NRW * 32, p2 = (KT - 1) / 2, dmax = D0 > D1 ? (D0 > D2 ? D0 : D2) : (D1 > D2 ? D1 : D2);
    const int h = p2 * (3 + D0 + D1 + D2);  // every pair costs P2 (second conv) + P2 * D_p (first conv)
    return {w, p2, h, w - 2 * h, w - h, p2 * dmax, round_up(w + 2 * p2 * dmax, 8), C / (32 * MRW) * NSTRIP * 64, C};
}
// the tile of a (taps, channels) pair: column strips x 32-column tiles per wave x row tiles per wave (nstrip 0: no such kernel). The measurements behind the
// table stand at launch_rbblock16
struct RbBlock16Tile {
    int nstrip, nrw, mrw;
};
constexpr RbBlock16Tile rbblock16_tile(int kt, int C) {
    if (!(kt == 3 || kt == 7 || kt == 11)) return {0, 0, 0};
    if (C == 32) return {4, 3, 1};
    if (C == 64) return kt == 11 ? RbBlock16Tile{4, 3, 1} : RbBlock16Tile{2, 4, 1};
    if (C == 128 && kt == 3) return {4, 2, 2};
    return {0, 0, 0};
}
constexpr RbBlock16Geom rbblock16_geom(int kt, int C) { return rbblock16_geom(kt, C, rbblock16_tile(kt, C).nstrip, rbblock16_tile(kt, C).nrw, rbblock16_tile(kt, C).mrw); }
constexpr bool rbblock16_exists(int kt, int C) { return rbblock16_tile(kt, C).nstrip != 0; }

// rbpair32_kernel<KT, DIL, C>
struct RbPair32Geom {
    int wn, nr, bm, bo, xwp, twp;  // (pitches in floats; x: + up to 3 columns of alignment shift)
    size_t lds;                    // (the last 1 KB DMA instruction may overhang the tile)
};
constexpr RbPair32Geom rbpair32_geom(int KT, int DIL, int C) {
    const int wn = 4 / (C / 32), nr = C >= 128 ? 4 : 2, bm = wn * nr * 32, xwp = round_up(bm + (KT - 1) * DIL + 3, 4);
    return {wn, nr, bm, bm - (KT - 1), xwp, round_up(bm + KT - 1, 4), ((size_t)C * xwp * sizeof(float) + 1023) / 1024 * 1024};
}
constexpr bool rbpair32_exists(int KT, int DIL, int C) {
    return (KT == 3 || KT == 7 || KT == 11) && (DIL == 1 || DIL == 3 || DIL == 5) && (C == 32 || C == 64 || (C == 128 && KT == 3));
}
// rbblock32_kernel<C, NR>: three taps, dilations 1 / 3 / 5
struct RbBlock32Geom {
    int w, p2, h, bo, padx, pitch;
    size_t lds;
};
constexpr RbBlock32Geom rbblock32_geom(int C, int NR) {
    const int w = 4 / (C / 32) * NR * 32, p2 = 1, h = p2 * (3 + 1 + 3 + 5), padx = p2 * 5, pitch = round_up(w + 2 * padx, 4);
    return {w, p2, h, w - 2 * h, padx, pitch, ((size_t)C * pitch + 6 * C) * sizeof(float)};
}
constexpr int rbblock32_nr(int C) { return C == 32 ? 2 : C == 64 ? 4 : 0; }  // (0: no such kernel)
constexpr bool rbblock32_exists(int C, int NR) { return (C == 32 && NR == 2) || (C == 64 && NR == 4); }

// convt16_kernel<NR, CSPLIT, RS, BF> (lines_bn == 0) / convt16_lines_kernel<BN, BF>: the x tile of bn input positions + 1
constexpr int convt16_bn(int nr, int csplit) { return nr * csplit * 32; }
constexpr int convt16_xw(int bn) { return round_up(bn + 1, 8); }
constexpr size_t convt16_lds(int cin, int bn) { return (size_t)(cin / 8) * convt16_xw(bn) * 16; }
constexpr bool convt16_exists(int lines_bn, int nr, int csplit, int rs) {
    return lines_bn ? lines_bn == 64 || lines_bn == 128 : (rs == 8 || rs == 16) && ((nr == 4 && (csplit == 1 || csplit == 2)) || (nr == 2 && csplit == 1));
}

// wavenet32_kernel<H, KT> / wavenet16_kernel<H, KT, BF, NCW>: blocks of 64 frames (two 32-frame column tiles)
constexpr int kWaveNetBM = 64;
constexpr int wavenet32_xwp(int KT) { return round_up(kWaveNetBM + KT - 1 + 3, 4); }  // h tile row pitch (floats): + up to 3 columns of alignment shift
constexpr size_t wavenet32_lds(int H, int KT) { return ((size_t)H * wavenet32_xwp(KT) * sizeof(float) + 1023) / 1024 * 1024; }
constexpr int wavenet16_xs(int KT) { return kWaveNetBM + KT - 1; }  // slots per group row of the h tile
constexpr size_t wavenet16_lds(int H, int KT) { return (size_t)(H / 8) * wavenet16_xs(KT) * 16; }
// flow_couple16_kernel<BF, NCW, NCT>: H = 192, four 5-tap layers; blocks of 32 NCT frames that yield all but a halo of 8 per side
struct FlowCouple16Geom {
    int bm, halo, bo, xs, lb_n, block;  // frames staged / halo / frames produced per block, slots per group row, floats of the bias area, threads
    size_t lds;
};
constexpr FlowCouple16Geom flow_couple16_geom(int NCW, int NCT) {
    const int H = 192, HF = 96, KT = 5, NL = 4, bm = 32 * NCT, xs = bm + KT - 1, lb_n = H + 2 * NL * 2 * H + HF;
    return {bm, 8, bm - 2 * 8, xs, lb_n, 64 * (H / 32) * NCT / NCW, (size_t)((H / 8) * xs + (H / 8) * bm) * 16 + (size_t)lb_n * 4};
}
constexpr int flow_wide_blocks(int frames) { return blocks_for(frames, flow_couple16_geom(2, 2).bo); }  // the 48-frame blocks of one utterance
constexpr bool flow_couple16_exists(int ncw, int nct) { return (nct == 1 && ncw == 1) || (nct == 2 && (ncw == 1 || ncw == 2)); }
constexpr bool wavenet16_exists(int ncw) { return ncw == 1 || ncw == 2; }
constexpr bool rbblock16_group3_exists(int C) { return C == 32 || C == 64; }

// stage one. A block may use kLdsMax of the CU's LDS; the kernels that leave room for a second block or for static arrays refuse above kLdsSoft
constexpr size_t kLdsMax = 160 * 1024, kLdsSoft = 150 * 1024;
constexpr int kAttQ = 16;     // queries per attention block
constexpr int kLnGroups = 16;  // channel groups of the LayerNorm kernels (add_layer_norm_kernel, dds_depthwise_kernel, dds_layer_kernel, dds_layer_lat_kernel)
constexpr int kLatNT = 16;    // tokens per block of dds_layer_lat_kernel
constexpr int att_lp(int len) { return (len + 63) / 64 * 64 + 4; }  // score row pitch of rel_attention_mfma_kernel: >= len + 4, = 4 (mod 64)
constexpr size_t att_mfma_lds(int head_dim, int tmax, int window) {
    return sizeof(float) * ((((size_t)kAttQ * head_dim + kAttQ * (2 * window + 1) + 3) & ~(size_t)3) + (size_t)kAttQ * att_lp(tmax));
}
constexpr size_t att_valu_lds(int head_dim, int tmax, int window, int vshift) {
    return sizeof(float) * ((size_t)kAttQ * head_dim + kAttQ * (2 * window + 1) + (size_t)kAttQ * ((tmax + 3) & ~3) + (size_t)head_dim * ((1 << vshift) + 1));
}
// rel_attention_mfma_kernel<NW, MAXS, SHORT, LAT> / rel_attention_kernel<threads>
constexpr bool att_mfma_exists(int nw, int maxs, bool sh, bool lat) {
    return lat ? nw == 8 && maxs == 24 && !sh : (nw == 4 && maxs == 24 && sh) || ((nw == 4 || nw == 8) && maxs == 32 && !sh);
}
constexpr bool att_valu_exists(int threads) { return threads == 1024 || threads == 256; }
constexpr size_t layer_norm_lds(int channels, int tw) { return sizeof(float) * ((size_t)channels * tw + 2 * tw * kLnGroups); }
constexpr size_t dds_depthwise_lds(int channels, int k, int dil) {
    return sizeof(float) * ((size_t)channels * (64 + 2 * ((k * dil - dil) / 2)) + (size_t)channels * 64 + 2 * 64 * kLnGroups);
}
constexpr size_t dds_layer_lds(int channels, int k, int dil) {
    return sizeof(float) * (((size_t)channels * (32 + (k * dil - dil)) + 3) / 4 * 4 + (size_t)channels * 32 + 2 * 32 * kLnGroups + ((size_t)channels * (6 + k) + 3) / 4 * 4) +
           (size_t)channels * 64;
}
constexpr size_t dds_lat_lds(int H, int k, int dil, bool head_conv, int h_cin) {  // (head_conv: an H -> H 1x1 conv of h_cin input channels in front)
    const int xw = kLatNT + (k * dil - dil);
    return sizeof(float) * (((size_t)H * xw + 3) / 4 * 4 + (size_t)H * kLatNT + 2 * kLnGroups * kLatNT + ((size_t)H * (6 + k) + 3) / 4 * 4 + (head_conv ? (size_t)h_cin * ((xw + 15) & ~15) : 0));
}

// dp_det_kernel<HCH, FC, K, NT> (dp_det.hip): the deterministic duration predictor. A block owns NT tokens of one utterance: the x' tile [32 HCH][xp] with 2 (K / 2)
// halo columns per side, the a1 tile [FC][ap] on NT + 2 (K / 2) columns (a2 takes its place), one wave per 16 output rows. Pitches = 16 (mod 32): the four
// channel rows a wave's B operand reads fall on different banks. The LayerNorm partial sums take the x' tile's place.
struct DpDetGeom {
    int nt, pad, w1, ct1, ct2, xp, ap, block;  // tokens, halo of one conv, a1 columns, 16-column tiles of conv_1 / conv_2, pitches (floats), threads
    size_t lds;
};
constexpr int dp_det_pitch(int need) { return (need + 15) / 32 * 32 + 16; }  // smallest pitch >= need that is 16 (mod 32)
constexpr int kDpDetWide = 64;  // the wide tile: a1 on exactly 64 columns, i.e. 64 - 2 (K / 2) tokens per block
constexpr DpDetGeom dp_det_geom(int HCH, int FC, int K, int NT) {
    const int pad = K / 2, w1 = NT + 2 * pad, ct1 = blocks_for(w1, 16), ct2 = blocks_for(NT, 16);
    const int xp = dp_det_pitch(ct1 * 16 + K - 1), need2 = ct2 * 16 + K - 1, ap = dp_det_pitch(need2 > ct1 * 16 ? need2 : ct1 * 16);
    const size_t xfloats = (size_t)32 * HCH * xp, rfloats = (size_t)(2 * kLnGroups + 2) * ct1 * 16;
    return {NT, pad, w1, ct1, ct2, xp, ap, FC / 16 * 64, sizeof(float) * ((xfloats > rfloats ? xfloats : rfloats) + (size_t)FC * ap)};
}
constexpr int dp_det_wide_nt(int K) { return kDpDetWide - 2 * (K / 2); }
constexpr bool dp_det_shape_exists(int H, int FC, int K) { return (H == 192 && FC == 256 && (K == 3 || K == 5)) || (H == 16 && FC == 32 && K == 3); }
constexpr bool dp_det_exists(int H, int FC, int K, int NT) { return dp_det_shape_exists(H, FC, K) && (NT == kLatNT || NT == dp_det_wide_nt(K)); }

// ---- one plan per launch --------------------------------------------------------------------------------------------------------------
struct LaunchGrid {
    bool ok = false;  // false: the launcher refuses
    int gx = 0, gy = 0, gz = 1, block = 0;
    size_t lds = 0;
};
struct RbPair16Plan : LaunchGrid {
    int nr = 0;
};
// force_nr (C >= 128): that many column tiles per wave whatever the grid and VITS_FUSE16_MAXC, or a refusal where no such instantiation exists; 0: the policy
RbPair16Plan plan_rbpair16(int channels, int kt, int dil, int batch, int tmax, int force_nr = 0);
struct RbBlock16Plan : LaunchGrid {
    RbBlock16Tile tile = {0, 0, 0};
    int nt = 1;  // tiles a block walks (> 1: the STREAM instantiation)
};
// in_group: as a member of the grouped launch, where C = 64, k = 11 is a whole-resblock kernel whatever VITS_RBB_C64K11 says for the single launch
// force_nt >= 1: that many tiles per block on every shape with an instantiation, whatever the grid and the knobs say (C = 64, k = 11 on one tile included); 0: the policy
RbBlock16Plan plan_rbblock16(int channels, int kt, int batch, int tmax, bool in_group = false, int force_nt = 0);
LaunchGrid plan_rbblock16_group3(int channels, const int* kts, int batch, int tmax);
LaunchGrid plan_rbpair32(int channels, int kt, int dil, int batch, int tmax);
struct RbBlock32Plan : LaunchGrid {
    int nr = 0;
};
RbBlock32Plan plan_rbblock32(int channels, int kt, int batch, int tmax);
// ConvTranspose1d streaming kernels. `supported` is the shape-and-knob part of convt16_stream_supported (the launcher adds the pointers); `tag` is what the profiler prints
struct ConvT16Plan : LaunchGrid {
    bool supported = false;
    int lines_bn = 0, nr = 0, csplit = 0, rs = 0;
    char tag[16] = "";
};
// force_split 1, 2 or 4: the lines kernels deal their units over that many blocks whatever the grid and VITS_CONVT16_SPLIT_MAX say (vits_op_upsample16), or a refusal
// (ok false) on a kernel that has no such deal; 0: the policy
ConvT16Plan plan_convt16(const PackedConv& w, int batch, int t_in, int force_split = 0);
// one WaveNet layer of the flow (fp32: ncw 0); `ok` is the shape part of wavenet32_supported / wavenet16_supported
struct WaveNetPlan : LaunchGrid {
    int ncw = 0;
};
WaveNetPlan plan_wavenet32(int hidden, int kt, int dil, int batch, int tmax);
// force_ncw: that many column tiles per wave whatever VITS_WN16_NCW says, or a refusal where no such instantiation exists; 0: the policy
WaveNetPlan plan_wavenet16(int hidden, int kt, int dil, int batch, int tmax, int force_ncw = 0);
// one whole coupling layer; `ok` is the shape part of flow_couple16_supported
struct FlowCouple16Plan : LaunchGrid {
    int ncw = 0, nct = 0;
};
// force_ncw / force_nct (either set): that tile whatever the grid, VITS_FLOW_NCW and VITS_FLOW_NARROW_MAX say, or a refusal where no such instantiation exists; 0, 0: the policy
FlowCouple16Plan plan_flow_couple16(int hidden, int half, int kt, int rate, int layers, int batch, int tmax, int force_ncw = 0, int force_nct = 0);
bool flow_couple16_narrow(int64_t wide_blocks);  // a launch of this many 48-frame blocks runs on 16-frame blocks instead (VITS_FLOW_NARROW_MAX)
// relative-position attention: the matrix-core kernel (nw waves, maxs k-steps, short / latency variant) or the VALU kernel (`block` threads, vshift)
struct AttentionPlan : LaunchGrid {
    bool mfma = false, sh = false, lat = false;
    int nw = 0, maxs = 0, vshift = 0;
};
// force (vits_op_attention): 1 / 2 = rel_attention_kernel<1024> / <256>, 3 ... 6 = rel_attention_mfma_kernel<4, 32, false, false> / <8, 32, false, false> / <4, 24, true, false> /
// <8, 24, false, true>, whatever the grid and the knobs say, or a refusal (ok false) where no instantiation can run the shape; 0: the policy
AttentionPlan plan_rel_attention(int batch, int heads, int head_dim, int tmax, int window, int force = 0);
struct LayerNormPlan : LaunchGrid {
    int tw = 0;  // time steps per block
};
// force_tw 32 or 64 (vits_op_layer_norm): that tile whatever VITS_LN_TW says, or a refusal for any other value; 0: the policy
LayerNormPlan plan_add_layer_norm(int channels, int batch, int tmax, int force_tw = 0);
LaunchGrid plan_dds_depthwise(int channels, int k, int dil, int batch, int tmax);
// one DDS layer; `ok` is the shape part of dds_layer_supported / dds_layer_lat_supported. m: the kernel's bound on 32-channel chunks
struct DdsLayerPlan : LaunchGrid {
    int m = 0;
};
DdsLayerPlan plan_dds_layer(int channels, int k, int dil, int batch, int tmax);
DdsLayerPlan plan_dds_layer_lat(int channels, int k, int dil, bool head_conv, int batch, int tmax);
bool dds_lat_grid_ok(int batch, int tmax);  // the latency kernel's grid rule (VITS_NO_DDS_LAT, VITS_DDS_LAT_MAX_BLOCKS)
// the deterministic duration predictor: `fused` = dp_det_kernel on the nt-token tile (ok: launchable), otherwise the un-fused sequence. variant 0: the planner's choice
// (VITS_NO_DP_DET_FUSE, VITS_DP_DET_LAT_MAX_BLOCKS); 1 / 2: the 16-token / the wide tile or a refusal (ok false), never the un-fused sequence; 3: un-fused
struct DpDetPlan : LaunchGrid {
    bool fused = false;
    int nt = 0;
};
DpDetPlan plan_dp_det(int hidden, int filter, int k, int batch, int tmax, int variant = 0);

}  // namespace vits
