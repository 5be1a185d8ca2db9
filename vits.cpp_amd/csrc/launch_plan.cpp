// launch_plan.cpp — see launch_plan.h: which fused vocoder kernel runs, on which tile, with what grid and how many LDS bytes. Host arithmetic only.
#include "launch_plan.h"

#include "../../include/vits.h"

#include <algorithm>
#include <cstdio>

namespace vits {

static void set_grid(LaunchGrid& p, int gx, int gy, int block, size_t lds, int gz = 1) {
    p.ok = true, p.gx = gx, p.gy = gy, p.gz = gz, p.block = block, p.lds = lds;
}

RbPair16Plan plan_rbpair16(int C, int kt, int dil, int batch, int tmax, int force_nr) {
    RbPair16Plan p;
    if (force_nr) {  // the caller names the instantiation (vits_op_resblock): no knob, no grid rule
        if (!rbpair16_exists(kt, dil, C, force_nr)) return p;
        p.nr = force_nr;
        const RbPair16Geom g = rbpair16_geom(kt, dil, C, p.nr);
        set_grid(p, blocks_for(tmax, g.bo), batch, g.block, g.lds);
        return p;
    }
    // VITS_FUSE16_MAXC=64 keeps the C = 128 pairs on two kernels
    if (!(kt == 3 || kt == 7 || kt == 11) || !(dil == 1 || dil == 3 || dil == 5) || C > kernel_knobs().fuse16_maxc || !(C == 32 || C == 64 || C == 128 || C == 256)) return p;
    // small grids (batch 1 ... 4): the row-split blocks own 128 columns (NR = 4 tiles per wave), i.e. 16 blocks for the 1,808 frames of an
    // utterance at C = 256 on 256 CUs; blocks of VITS_RB16_NARROW_NR tiles are that many times shorter chains on that many more CUs
    // (the halo costs more: they lose as soon as the chip is full). Same chains per output: bit-identical.
    p.nr = C < 128 ? 2 : (int64_t)blocks_for(tmax, rbpair16_geom(kt, dil, C, 4).bo) * batch <= kernel_knobs().rb16_narrow_max ? VITS_RB16_NARROW_NR : 4;
    const RbPair16Geom g = rbpair16_geom(kt, dil, C, p.nr);
    set_grid(p, blocks_for(tmax, g.bo), batch, g.block, g.lds);
    return p;
}

// Tiles per block for a launch of `batch` sequences of up to `tmax` columns.
// Segments of several tiles (STREAM) once the one-tile grid is many rounds of the chip: a segment's first tile pays the halo of both sides,
// and the blocks of the last round run on a partly empty chip — nt grows with the grid up to the shape's limit.
// Which shapes: measured per kernel on the benchmark batch (64 x 128 ids: 10-14 thousand tiles, i.e. 13-18 per resident block, so that long
// segments cost in balance what they save in halo — tools/rbb_micro.hip, profiles/round6_rbb_stream_micro.txt): k = 11 at C = 32
// 1.000 -> 0.892 ms with 6 tiles, k = 7 at C = 64 1.138 -> 1.040 with 3, k = 11 at C = 64 1.584 -> 1.396 with 4; k = 3 (a halo of 12
// columns) and k = 7 at C = 32 lose 0-25 %: one tile per block there.
static int rbb_stream_tiles_for(int kt, int C, int batch, int tmax) {
    const KernelKnobs& kn = kernel_knobs();
    const long blocks1 = (long)blocks_for(tmax, rbblock16_geom(kt, C).bo) * batch;
    int want = kn.rbb_stream_tiles;
    if (want < 0) want = (kt == 11 && C == 32) ? 6 : (kt == 7 && C == 64) ? 3 : (kt == 11 && C == 64) ? 4 : 0;
    if (want <= 1 || kn.rbb_stream_min_blocks <= 0 || blocks1 < 2L * kn.rbb_stream_min_blocks) return 1;
    return (int)(blocks1 / kn.rbb_stream_min_blocks < want ? blocks1 / kn.rbb_stream_min_blocks : want);
}

RbBlock16Plan plan_rbblock16(int C, int kt, int batch, int tmax, bool in_group, int force_nt) {
    RbBlock16Plan p;
    if (force_nt > 0) {  // the caller names the form (vits_op_resblock): no knob, no grid rule
        if (!rbblock16_exists(kt, C)) return p;
        p.tile = rbblock16_tile(kt, C), p.nt = force_nt;
        const RbBlock16Geom g = rbblock16_geom(kt, C);
        set_grid(p, blocks_for(tmax, g.seg_out(force_nt)), batch, g.block, g.lds(force_nt > 1));
        return p;
    }
    if (!rbblock16_exists(kt, C) || (C == 128 && !kernel_knobs().rbb_c128)) return p;
    const int nt = rbb_stream_tiles_for(kt, C, batch, tmax);
    // C = 64, k = 11: on one tile per block (1.45 x the MFMA work) the whole-resblock kernel is bound by the matrix cores (at the clock
    // the power budget leaves them) and loses to three fused pairs, 1.59 against 1.45 ms per step (batch 64 x 128 ids); on segments of four
    // tiles (1.19 x; round 6) it wins, 13.31 -> 13.19 ms per pipelined batch. VITS_RBB_C64K11=1 runs it on every grid, =0 on none.
    const int c64k11 = kernel_knobs().rbb_c64k11;
    if (C == 64 && kt == 11 && !in_group && !(c64k11 > 0 || (c64k11 < 0 && nt > 1))) return p;
    p.tile = rbblock16_tile(kt, C), p.nt = nt;
    const RbBlock16Geom g = rbblock16_geom(kt, C);
    set_grid(p, blocks_for(tmax, g.seg_out(nt)), batch, g.block, g.lds(nt > 1));
    return p;
}

LaunchGrid plan_rbblock16_group3(int C, const int* kts, int batch, int tmax) {
    const KernelKnobs& kn = kernel_knobs();
    LaunchGrid p;
    if (kn.no_rbb_group3 || !(C == 32 || (C == 64 && !kn.no_rbb_group3_c64)) || kts[0] != 3 || kts[1] != 7 || kts[2] != 11) return p;
    // (k = 11 at C = 64 is a whole-resblock kernel here whatever VITS_RBB_C64K11 says for the single launches: measured in the group)
    for (int m = 0; m < 3; ++m)
        if (!plan_rbblock16(C, kts[m], batch, tmax, true).ok) return p;
    // one tile per block, well below rbb_stream_tiles_for's threshold for segments: at most 3072 blocks of the narrowest member tile (k = 7 at C = 64)
    if ((long)blocks_for(tmax, rbblock16_geom(7, 64).bo) * batch > 3072) return p;
    // LDS of the k = 11 member (384 columns + the widest padding); grid.x of the member with the fewest outputs per tile (C = 32: k = 11; C = 64: k = 7 on 256 columns)
    const int bo_min = std::min(rbblock16_geom(7, C).bo, rbblock16_geom(11, C).bo);
    set_grid(p, blocks_for(tmax, bo_min), 3 * batch, std::max(rbblock16_geom(7, C).block, rbblock16_geom(11, C).block), rbblock16_geom(11, C).lds(false));
    return p;
}

LaunchGrid plan_rbpair32(int C, int kt, int dil, int batch, int tmax) {
    LaunchGrid p;
    // C = 128: only the k = 3 pairs — their 128-column tile with its small halo is 74 KB (two blocks per CU); k = 7 / 11 would be 84-94 KB
    if (!rbpair32_exists(kt, dil, C) || (C == 128 && !kernel_knobs().fuse32_c128)) return p;
    const RbPair32Geom g = rbpair32_geom(kt, dil, C);
    set_grid(p, blocks_for(tmax, g.bo), batch, 256, g.lds);
    return p;
}

RbBlock32Plan plan_rbblock32(int C, int kt, int batch, int tmax) {
    RbBlock32Plan p;
    if (kt != 3 || !rbblock32_nr(C)) return p;
    // (C = 32 on 384-column tiles — 1.07 x instead of 1.10 x the MFMA work, two blocks per CU instead of three — measured 1.25 against 1.22 ms)
    p.nr = rbblock32_nr(C);
    const RbBlock32Geom g = rbblock32_geom(C, p.nr);
    set_grid(p, blocks_for(tmax, g.bo), batch, 256, g.lds);
    return p;
}

// convt16_lines_kernel<BN>: four phases per wave, for row counts above 128 with a stride that is a multiple of 4; 128 positions per block,
// 64 when c_in = 512 (LDS for two blocks per CU). convt16_kernel<NR, CSPLIT, RS>: 128 positions per block; 64 when the input tile of 128
// would not leave room for two blocks per CU (c_in = 512); 256 positions with two waves per row tile when there are only two row tiles (the
// last upsampler: 64 rows); sixteen ring slots where the step count allows.
ConvT16Plan plan_convt16(const PackedConv& w, int batch, int t_in, int force_split) {
    const KernelKnobs& kn = kernel_knobs();
    ConvT16Plan p;
    // the choice and its tag, for any transposed conv (convt16_stream_tag answers whether or not the streaming kernel is taken)
    if (w.rows > 128 && w.ct_stride % 4 == 0 && !kn.convt16s_all) {
        p.lines_bn = w.cin > 256 ? 64 : 128;
        std::snprintf(p.tag, sizeof(p.tag), "SL%d", p.lines_bn);
    } else {
        p.rs = w.cin % 128 == 0 ? 16 : 8;
        if (w.rows / 32 <= 2) p.nr = 4, p.csplit = 2;
        else if (w.cin > 256) p.nr = 2, p.csplit = 1;
        else p.nr = 4, p.csplit = 1;
        if (const int ov = kn.convt16_r128; ov && w.rows == 128) {  // (developer override: same bits, another block shape)
            p.nr = ov / 100, p.csplit = ov / 10 % 10, p.rs = (ov % 10) ? 16 : 8;
            if (p.rs == 16 && w.cin % 128 != 0) p.rs = 8;
        }
        std::snprintf(p.tag, sizeof(p.tag), "S%d.%d.%d", p.nr, p.csplit, p.rs);
    }
    if (kn.no_convt16s || w.epi != EPI_CONVT || w.kt != 2 || w.cin % 64 != 0 || w.cout % 32 != 0 || w.rows % 32 != 0 || w.cin > 512) return p;
    // (VITS_CONVT16S_ALL=1: the one-row-tile-at-a-time kernel also for stride 8 — the slow first version, kept for the comparison;
    // VITS_NO_CONVT16L: no four-phase variant for strides that are multiples of 4)
    if (!(w.rows <= 128 || kn.convt16s_all || (!kn.no_convt16l && w.ct_stride % 4 == 0))) return p;
    p.supported = true;
    if (!convt16_exists(p.lines_bn, p.nr, p.csplit, p.rs)) return p;  // (an override that names no instantiation: the launch is refused)
    const int bn = p.lines_bn ? p.lines_bn : convt16_bn(p.nr, p.csplit), tiles_x = blocks_for(t_in + 1, bn);
    int zsplit = 1;
    if (force_split) {  // the caller names the deal (vits_op_upsample16): no knob, no grid rule
        if (!p.lines_bn || !(force_split == 1 || force_split == 2 || force_split == 4)) return p;
        zsplit = force_split;
    } else if (p.lines_bn && (int64_t)tiles_x * batch <= kn.convt16_split_max) {
        const int nunits = (w.cout >> 5) * (w.ct_stride / 4) * (bn / 64);
        zsplit = nunits >= 16 ? 4 : nunits >= 8 ? 2 : 1;
    }
    set_grid(p, tiles_x, batch, 256, convt16_lds(w.cin, bn), zsplit);
    return p;
}

WaveNetPlan plan_wavenet32(int hidden, int kt, int dil, int batch, int tmax) {
    WaveNetPlan p;
    if (hidden != 192 || kt != 5 || dil != 1) return p;
    set_grid(p, blocks_for(tmax, kWaveNetBM), batch, 4 * hidden, wavenet32_lds(hidden, kt));
    return p;
}
WaveNetPlan plan_wavenet16(int hidden, int kt, int dil, int batch, int tmax, int force_ncw) {
    WaveNetPlan p;
    if (hidden != 192 || kt != 5 || dil != 1) return p;
    if (force_ncw && !wavenet16_exists(force_ncw)) return p;  // the caller names the instantiation (vits_op_flow_coupling): no knob
    p.ncw = force_ncw ? force_ncw : kernel_knobs().wn16_ncw == 1 ? 1 : 2;  // (2: six waves, both column tiles each — measured 40.6 vs 38.4 us per layer)
    set_grid(p, blocks_for(tmax, kWaveNetBM), batch, 4 * hidden / p.ncw, wavenet16_lds(hidden, kt));
    return p;
}

bool flow_couple16_narrow(int64_t wide_blocks) { return wide_blocks <= kernel_knobs().flow_narrow_max; }
FlowCouple16Plan plan_flow_couple16(int hidden, int half, int kt, int rate, int layers, int batch, int tmax, int force_ncw, int force_nct) {
    FlowCouple16Plan p;
    if (hidden != 192 || half != 96 || kt != 5 || rate != 1 || layers != 4) return p;
    if (force_ncw || force_nct) {  // the caller names the instantiation (vits_op_flow_coupling): no knob, no grid rule
        if (!flow_couple16_exists(force_ncw, force_nct)) return p;
        p.ncw = force_ncw, p.nct = force_nct;
        const FlowCouple16Geom g = flow_couple16_geom(p.ncw, p.nct);
        set_grid(p, blocks_for(tmax, g.bo), batch, g.block, g.lds);
        return p;
    }
    // small grids (batch 1 ... 4 at 225 frames): 16-frame blocks on one 32-column tile (see the kernel); otherwise 48-frame blocks of six waves owning both
    // column tiles of their channel group (VITS_FLOW_NCW=1: twelve waves, one column tile each)
    if (flow_couple16_narrow((int64_t)flow_wide_blocks(tmax) * batch)) p.ncw = 1, p.nct = 1;
    else p.ncw = kernel_knobs().flow_ncw == 1 ? 1 : 2, p.nct = 2;
    const FlowCouple16Geom g = flow_couple16_geom(p.ncw, p.nct);
    set_grid(p, blocks_for(tmax, g.bo), batch, g.block, g.lds);
    return p;
}

// ---- stage one ---------------------------------------------------------------------------------------------------------------------------
AttentionPlan plan_rel_attention(int batch, int heads, int head_dim, int tmax, int window, int force) {
    const KernelKnobs& kn = kernel_knobs();
    AttentionPlan p;
    const int gx = blocks_for(tmax, kAttQ);
    const int64_t blocks = (int64_t)gx * heads * batch;
    if (force) {  // the caller names the instantiation (vits_op_attention): no knob, no grid rule. Every kernel's loops run over the utterance's own length
        // and every block works for itself: the short variant beyond VITS_ATT_SHORT tokens and the latency variant beyond 128 blocks compute the same sums
        if (force < 1 || force > 6 || head_dim < 1 || head_dim > 128) return p;
        if (force <= 2) {  // rel_attention_kernel<1024 | 256>: (d, 4-query group) items over 512 thread slots, V chunks of 2^vshift keys
            size_t lds = 0;
            for (p.vshift = 6; p.vshift >= 3; --p.vshift) {
                lds = att_valu_lds(head_dim, tmax, window, p.vshift);
                if (lds <= kLdsSoft) break;
            }
            if (lds > kLdsSoft) return p;
            set_grid(p, gx, heads, force == 1 ? 1024 : 256, lds, batch);
            return p;
        }
        p.nw = force == 3 || force == 5 ? 4 : 8, p.lat = force == 6, p.sh = force == 5, p.maxs = force >= 5 ? 24 : 32;
        const size_t lds = att_mfma_lds(head_dim, tmax, window);
        if ((head_dim & 15) || head_dim > 4 * p.maxs || lds > kLdsMax) return p;
        p.mfma = true;
        set_grid(p, gx, heads, 64 * p.nw, lds, batch);
        return p;
    }
    // matrix-core version. The number of waves (= how the key tiles and the d tiles are dealt out) does not change a single sum, so it may
    // depend on the launch: four waves while two or more blocks fit the LDS of a CU (up to ~1200 tokens: 1024 ids 0.178 ms against 0.222
    // with six waves), eight once the scores of a block leave room for one block only (2049 tokens: 0.87 against 1.29 ms with four)
    const size_t ldsm = att_mfma_lds(head_dim, tmax, window);
    if (!kn.att_valu && (head_dim & 15) == 0 && head_dim <= 128 && ldsm <= kLdsMax) {
        p.mfma = true;
        p.nw = 2 * ldsm > kLdsMax ? 8 : 4;
        // latency-bound launches (at most 128 blocks: up to eight 128-token utterances): eight waves deal the key tiles and the d tiles out one per wave
        // (per-block stamps at 128 tokens, tools/att_micro.hip: P V 5.0 -> 3.0 us, block life 15.2 -> 13.9; batch 1 / 2 / 4 / 8: -1 ... -3 % per call, round 6)
        if (blocks <= 128) p.nw = 8;
        if (kn.att_nw == 4 || kn.att_nw == 8) p.nw = kn.att_nw;
        // (the long variants keep their arrays at 32 k-steps: sized for 24 the four-wave kernel measured 0.22 against 0.18 ms at 1024 tokens)
        p.lat = !kn.no_att_lat && p.nw == 8 && head_dim <= 96 && blocks <= 128;
        p.sh = !p.lat && p.nw == 4 && head_dim <= 96 && tmax <= kn.att_short;  // (VITS_ATT_SHORT tokens; 0 disables the short variant)
        p.maxs = p.lat || p.sh ? 24 : 32;
        set_grid(p, gx, heads, 64 * p.nw, ldsm, batch);
        return p;
    }
    size_t lds = 0;
    for (p.vshift = 6; p.vshift >= 3; --p.vshift) {
        lds = att_valu_lds(head_dim, tmax, window, p.vshift);
        if (lds <= kLdsSoft) break;
    }
    if (lds > kLdsSoft || head_dim * (kAttQ / 4) > 512) return p;
    set_grid(p, gx, heads, blocks <= 512 ? 1024 : 256, lds, batch);
    return p;
}

LayerNormPlan plan_add_layer_norm(int channels, int batch, int tmax, int force_tw) {
    // tile width (time steps per block): 32 = eight waves and channels x 128 B of LDS per block (29 KB at 192 channels); VITS_LN_TW=64 = the
    // sixteen-wave, 57 KB blocks of rounds 1-3. Every token's sums are the same either way (its channels are summed by the same sixteen channel
    // groups in the same order). The small block matters when this kernel shares the chip with another batch's vocoder (vits_model_submit_batch):
    // a 57 KB block only finds room in the tail of a vocoder kernel — stage one of a pipelined f16 batch took 10.2 ms of wall with it, 8.8 with
    // the small one (alone: 1.91 -> 1.87 ms).
    LayerNormPlan p;
    if (force_tw && force_tw != 32 && force_tw != 64) return p;
    p.tw = force_tw ? force_tw : kernel_knobs().ln_tw == 64 ? 64 : 32;  // (force_tw: the caller names the tile, vits_op_layer_norm)
    const size_t lds = layer_norm_lds(channels, p.tw);
    if (lds <= kLdsSoft) set_grid(p, blocks_for(tmax, p.tw), batch, p.tw * kLnGroups, lds);
    return p;
}

LaunchGrid plan_dds_depthwise(int channels, int k, int dil, int batch, int tmax) {
    LaunchGrid p;
    const size_t lds = dds_depthwise_lds(channels, k, dil);
    if (lds <= kLdsSoft) set_grid(p, blocks_for(tmax, 64), batch, 64 * kLnGroups, lds);
    return p;
}

static bool dds_taps_ok(int k, int dil) { return k >= 1 && dil >= 1 && !((k * dil - dil) & 1); }
DdsLayerPlan plan_dds_layer(int channels, int k, int dil, int batch, int tmax) {
    DdsLayerPlan p;
    if (channels <= 0 || (channels & 31) || channels > 32 * (kLnGroups / 2) || !dds_taps_ok(k, dil)) return p;  // one wave per 32 output rows, 8 waves
    const size_t lds = dds_layer_lds(channels, k, dil);
    if (lds > kLdsSoft) return p;
    const int nchunks = channels / 32;
    p.m = nchunks <= 2 ? 2 : nchunks <= 4 ? 4 : nchunks <= 6 ? 6 : 8;
    set_grid(p, blocks_for(tmax, 32), batch, 32 * kLnGroups, lds);
    return p;
}
DdsLayerPlan plan_dds_layer_lat(int channels, int k, int dil, bool head_conv, int batch, int tmax) {
    DdsLayerPlan p;
    if (channels < 32 || (channels & 31) || channels > 256 || !dds_taps_ok(k, dil)) return p;
    if (dds_lat_lds(channels, k, dil, true, channels) > kLdsSoft) return p;  // (with the widest head: one answer per layer)
    p.m = channels <= 192 ? 6 : 8;
    set_grid(p, blocks_for(tmax, kLatNT), batch, channels / 16 * 64, dds_lat_lds(channels, k, dil, head_conv, channels));
    return p;
}
bool dds_lat_grid_ok(int batch, int tmax) {
    return !kernel_knobs().no_dds_lat && (int64_t)batch * blocks_for(tmax, kLatNT) <= kernel_knobs().dds_lat_max_blocks;
}

// One launch for the whole deterministic predictor where an instantiation exists. Small grids take the 16-token tile (many short blocks: batch 1 x 128 ids = 8 blocks
// of 16 waves), large ones the wide tile, which reads the 1.4 MB of weights once per 62 tokens instead of once per 16.
DpDetPlan plan_dp_det(int hidden, int filter, int k, int batch, int tmax, int variant) {
    const KernelKnobs& kn = kernel_knobs();
    DpDetPlan p;
    if (variant < 0 || variant > 3 || variant == 3 || (variant == 0 && kn.no_dp_det_fuse)) return p;  // un-fused (ok stays false: nothing to launch here)
    if (!dp_det_shape_exists(hidden, filter, k)) return p;
    const bool lat = variant == 1 || (variant == 0 && (int64_t)batch * blocks_for(tmax, kLatNT) <= kn.dp_det_lat_max_blocks);
    p.nt = lat ? kLatNT : dp_det_wide_nt(k);
    if (!dp_det_exists(hidden, filter, k, p.nt)) return p;
    const DpDetGeom g = dp_det_geom(blocks_for(hidden, 32), filter, k, p.nt);
    if (g.lds > kLdsMax) return p;
    p.fused = true;
    set_grid(p, blocks_for(tmax, p.nt), batch, g.block, g.lds);
    return p;
}

// ---- the engine-facing predicates: thin calls into the plans (the launchers add the checks of their pointers) -------------------------------
bool rbpair16_supported(int channels, int kt, int dil) { return plan_rbpair16(channels, kt, dil, 1, 1).ok; }
static bool dils_135(const int* dils, int ndil) { return ndil == 3 && dils[0] == 1 && dils[1] == 3 && dils[2] == 5; }
bool rbblock16_supported(int channels, int kt, const int* dils, int ndil, int batch, int tmax) { return dils_135(dils, ndil) && plan_rbblock16(channels, kt, batch, tmax).ok; }
bool rbblock16_group3_supported(int channels, const int* kts, int batch, int tmax) { return plan_rbblock16_group3(channels, kts, batch, tmax).ok; }
bool rbpair32_supported(int channels, int kt, int dil) { return plan_rbpair32(channels, kt, dil, 1, 1).ok; }
bool rbblock32_supported(int channels, int kt, const int* dils, int ndil) { return dils_135(dils, ndil) && plan_rbblock32(channels, kt, 1, 1).ok; }
bool convt16_stream_supported(const PackedConv& w) { return w.wp16 && plan_convt16(w, 1, 1).supported; }
void convt16_stream_tag(const PackedConv& w, char* buf, size_t cap) { std::snprintf(buf, cap, "%s", plan_convt16(w, 1, 1).tag); }

bool dds_layer_supported(const PackedConv& pw, int channels, int k, int dil, int arith) {
    if (!plan_dds_layer(channels, k, dil, 1, 1).ok) return false;
    if (pw.cin != channels || pw.cout != channels || pw.kt != 1 || pw.epi != EPI_STD || !pw.bias) return false;
    return arith == VITS_ARITH_F32 ? pw.wp != nullptr : pw.wp16 != nullptr;
}
bool dds_layer_lat_supported(const PackedConv& pw, int channels, int k, int dil) {
    if (!plan_dds_layer_lat(channels, k, dil, true, 1, 1).ok) return false;
    return pw.cin == channels && pw.cout == channels && pw.kt == 1 && pw.epi == EPI_STD && pw.bias && pw.wp_l16;
}

}  // namespace vits
