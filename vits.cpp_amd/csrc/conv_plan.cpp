// conv_plan.cpp — every launch decision of the convolution families (see conv_plan.h): tile, kernel family, grid, LDS ring depth, one-shot fill,
// and the predicates that route a conv to the grouped / split / latency kernels. Host arithmetic only; the measured numbers behind each rule
// travel with it. DESIGN.md section 4.1 has the measurements behind the kernels themselves.
#include "conv_plan.h"

namespace vits {

// ---- fp32 convs (conv_mfma.hip) --------------------------------------------------------------------------------------------------------
// The tile a launch runs on: the shape rule, then the small-grid steps.
static int resolve_conv_tile(const PackedConv& w, const ConvCall& c) {
    const KernelKnobs& kn = kernel_knobs();
    const int ncols_max = conv_ncols(w, c);
    if (c.tile >= 0) return c.tile;
    // rows <= 64 (few MFMAs per staged tile): 128-column tiles -> twice as many independent blocks per CU keep more
    // loads in flight (measured 120.5 -> 116.4 ms per step); VITS_NARROW_TILES=0 restores 256-column tiles
    const bool small_t = ncols_max <= 128 || (kn.narrow_tiles && w.rows <= kn.narrow_tiles);
    int tile = small_t ? TILE_32x64 : TILE_32x256;
    if (w.epi == EPI_GATE || w.rows % 64 == 0) tile = small_t ? TILE_64x64 : TILE_64x256;
    if (w.epi != EPI_GATE && w.rows % 128 == 0 && kn.tile128) tile = TILE_128x128;
    auto blocks = [&](int tl) { return tile_blocks(tile_shape(tl), ncols_max, w.mtiles_used, c.batch); };
    if (w.epi == EPI_GATE) {
        if (blocks(tile) < kSmallGridBlocks) tile = TILE_64x64;  // 64 x 128 keeps the tanh/sigmoid row pairing
    } else {
        // small grids (batch 1, short inputs): fewer than ~2 blocks per CU leaves matrix pipes idle -> step down to
        // smaller tiles until the launch has >= 512 blocks (latency case, BASELINE.json config 2)
        // (k <= 3: 1024 — a short K loop costs a small tile little, and e.g. the encoder's 192 -> 768 FFN conv at batch 64 x 128 tokens is
        // 768 blocks of 64 x 128 = 1.5 rounds of the 512 resident blocks, but 3 even rounds of 32 x 128: 82 -> 74 us)
        const int64_t min_blocks = kn.min_blocks > 0 ? kn.min_blocks : (w.kt <= 3 ? 2 * kSmallGridBlocks : kSmallGridBlocks);
        if (blocks(tile) < min_blocks && (tile == TILE_128x128 || tile == TILE_64x256)) tile = TILE_64x64;  // 64 x 128
        if (blocks(tile) < min_blocks && (tile == TILE_64x64 || tile == TILE_32x256)) tile = TILE_32x64;    // 32 x 128
    }
    if (w.epi != EPI_CONVT) {
        // tiny grids (the encoder / duration predictor / flow at batch 1: 6-18 blocks of the 128-column tiles): every block of a
        // 128-column tile streams the WHOLE input in through its one producer wave, and that stream, not the MFMA chain, is the
        // launch time (768 -> 192 FFN conv, k = 3, 128 tokens: 78 us for a 31 us chain). Blocks of four row tiles x ONE 32-column
        // strip need a quarter of the input each. Same per-output accumulation order (the tile shape never changes it).
        const int dil_eff = conv_dil(w, c);
        const bool shape_ok = dil_eff == 1 && conv_narrow_shape(w.epi, w.kt);
        const int64_t nb = blocks(tile);
        // 1x1 convs (QKV / output / projection convs of the encoder, the flow's pre / post convs): the narrow tile on large grids too —
        // 192 -> 576 at batch 64 x 128 tokens 34 -> 26 us, 192 -> 192 21 -> 13 us; at 1024 tokens (config 5) the 1x1 convs of a step 0.83 ->
        // 0.65 ms (bf16 run), 1.34 -> 1.05 ms (fp32 run). VITS_NARROW_K1 = longest sequence that takes it (0: small grids only)
        const bool k1_short = kn.narrow_k1 > 0 && w.epi == EPI_STD && w.kt == 1 && ncols_max <= kn.narrow_k1;
        if (!kn.no_narrow && shape_ok && (nb <= 128 || k1_short)) tile = TILE_NARROW;
        // ... and where the launch time is one wave's MFMA chain (a second copy of the weights exists for the layers with >= 512 products
        // per output: not the 1x1 convs, whose chain is 2.6 us of a launch that is bound by its fill), 16 x 16 tiles on
        // v_mfma_f32_16x16x4_f32 (conv_lat16_kernel): the tiny grids of the narrow tile, and any standard conv whose 32 x 32 tiles would
        // not even fill the SIMDs once (batch 1: the C = 256 stage of the vocoder, conv_pre)
        const int pitch16 = lat16_pitch((w.kt - 1) * dil_eff);
        const int64_t waves32 = (int64_t)((ncols_max + 31) / 32) * w.mtiles_used * c.batch;
        const bool tiny = tile == TILE_NARROW && nb <= 128;
        const bool unfilled = w.epi == EPI_STD && w.kt >= 3 && dil_eff >= 1 && waves32 <= kn.lat16_max_waves;
        if ((tiny || unfilled) && !kn.no_lat16 && w.wp_l16 && conv_lat16_exists(w.epi, pitch16) && ((size_t)w.nchunks + 1) * kConvCK * pitch16 * 4 <= 150 * 1024)
            tile = TILE_LAT16;
    }
    return tile;
}

ConvPlan plan_conv(const PackedConv& w, const ConvCall& c, int forced_tile) {
    const KernelKnobs& kn = kernel_knobs();
    ConvPlan p;
    const int ncols_max = conv_ncols(w, c);
    p.tile = forced_tile >= 0 ? forced_tile : resolve_conv_tile(w, c);
    const TileShape ts = tile_shape(p.tile);
    p.dil = conv_dil(w, c);
    p.dil_ct = conv_template_dil(w.epi, w.kt, p.dil);
    // producer-wave path for every compile-time-dilation conv: with dwordx4 LDS-DMA it also wins for single-chunk inputs
    // (c_in = 32: 109 -> 120 TFLOP/s on the k = 11 layers; with dword DMA it lost 8 % there). VITS_DB_MIN=2 restores the
    // register-staged kernels for them.
    p.db = p.dil_ct != 0 && p.dil_ct != kNoKernel && w.nchunks >= kn.db_min;
    const int span = (w.kt - 1) * p.dil;  // signed extent of the taps
    const int aspan = span < 0 ? -span : span;
    p.lds_off = span < 0 ? -span : 0;
    p.xw = ts.bn() + aspan;
    const int64_t nblocks = tile_blocks(ts, ncols_max, w.mtiles_used, c.batch);
    const size_t row_bytes = (size_t)kConvCK * padded_xw(p.xw) * sizeof(float);  // one chunk of the producer-wave path in LDS
    // third LDS buffer (DMA two chunks ahead) where a chunk is less MFMA work than a DMA round trip (~2.5 us = 6k cycles):
    // taps x (MFMAs per k-step) x 16 k-steps x 64 cycles
    const bool short_chunk = w.kt * ts.mr * ts.nr * 1024 < 8000 && w.nchunks >= 3 && ts.bn() == 128;
    p.nbuf = kn.nbuf == 2 || kn.nbuf == 3 ? kn.nbuf : (short_chunk ? 3 : 2);
    if (w.nchunks < 2 || p.nbuf * row_bytes > 150 * 1024) p.nbuf = 2;
    // latency-bound launch on a small tile whose whole input fits in LDS: cooperative one-shot fill (see the kernel)
    if (!kn.no_oneshot && ts.mr * ts.nr <= 2 && nblocks <= 512 && w.nchunks >= 2 && w.nchunks * row_bytes <= 150 * 1024) {
        p.oneshot = 1;
        p.nbuf = w.nchunks;
    }
    p.ok = (size_t)2 * kConvCK * p.xw * 4 <= 160 * 1024;
    p.pitch = lat16_pitch(span);
    // LayerNorm on load exists in conv_lat16_kernel only (the launches it pays for are the latency-bound ones): a standard conv without an input activation
    // whose tile choice is TILE_LAT16, with the statistics' scratch beside the input tile in LDS, and the input lengths = the output lengths (padded 'same' conv)
    const size_t ln_bytes = ((size_t)2 * 16 * 32 + 2 * (size_t)w.cin) * sizeof(float);  // partial sums of up to 32 columns; gamma, beta
    const size_t lat_bytes = ((size_t)w.nchunks + 1) * kConvCK * p.pitch * sizeof(float);  // (+ one chunk of slack rows: the look-ahead of the last tap)
    // (c_in <= kLnLoadMaxCin: the kernel stages gamma and beta as three elements per thread; a wider input takes the separate launch)
    p.ln_why = w.epi != EPI_STD                                ? "not a standard conv (epilogue)"
               : c.pre_act                                     ? "the conv has an input activation"
               : !w.wp_l16                                     ? "the layer has no conv_lat16_kernel weights"
               : c.len_in != c.len_out || c.t_in != c.t_out    ? "input and output lengths differ"
               : p.tile != TILE_LAT16                          ? "the planner's tile is not TILE_LAT16"
               : !p.pitch || span > 16                         ? "(k - 1) * dilation > 16"
               : w.cin > kLnLoadMaxCin                         ? "c_in > 768 (gamma and beta are staged as three elements per thread)"
               : lat_bytes + ln_bytes > 150 * 1024             ? "the input tile and the statistics pass 150 KB of LDS"
                                                               : nullptr;
    p.ln_ok = !p.ln_why;
    if (p.tile == TILE_LAT16) {
        p.ok = p.ok && p.pitch && w.wp_l16;
        p.xw = p.pitch;
        p.gx = (ncols_max + 15) / 16, p.gy = (w.mtiles_used + 1) / 2, p.block = 256;
        p.lds = lat_bytes + (c.ln_gamma ? ln_bytes : 0);
    } else {
        // generic kernels stage at most BN + 64 columns; and the instantiation has to exist (VITS_DB_MIN=2 has no narrow tile for single-chunk inputs)
        p.ok = p.ok && aspan <= 64 && p.dil_ct != kNoKernel && conv_tile_exists(w.epi, w.kt, p.dil_ct, p.db, p.tile);
        p.gx = (ncols_max + ts.bn() - 1) / ts.bn(), p.gy = (w.mtiles_used + ts.bm() - 1) / ts.bm(), p.block = p.db ? 320 : 256;
        p.lds = p.db ? p.nbuf * row_bytes : (size_t)kConvCK * p.xw * sizeof(float);
    }
    p.gz = c.batch;
    return p;
}

bool conv_ln_on_load_ok(const PackedConv& w, const ConvCall& c) { return plan_conv(w, c).ln_ok; }

bool conv_lat16_candidate(int epi, int kt, int cin) {
    // (>= 64 products per output: everything but the degenerate convs. The long chains — FFN, gated, vocoder — win by the chain (41 -> 17.7 us);
    // the 1x1 convs, whose chain is only 2.6 us, by the fill and the finer grid: 13-16 -> 7 us at batch 1)
    return (epi == EPI_STD || (epi == EPI_GATE && kt == 5)) && (int64_t)kt * cin >= 64;
}

bool conv_group_supported(const PackedConv& w, int dil) {
    return w.epi == EPI_STD && (w.kt == 11 || w.kt == 7 || w.kt == 3) && (dil == 1 || dil == 3 || dil == 5) && w.rows % 128 == 0 && w.cin % kConvCK == 0;
}

// (C = 64 was tried on the 64 x 256 tile (WM = 2): 92 TFLOP/s-equivalent against 124 for the fused fp32 pairs — a 60 KB chunk per buffer leaves one block per CU,
// and ONE producer wave's LDS-DMA stream, ~1 KB per 0.12 us, takes as long per chunk as the chunk's MFMAs; the narrow stages keep their fused fp32 kernels)
bool conv_split_candidate(int epi, int kt, int cin, int cout) {
    return epi == EPI_STD && (kt == 3 || kt == 7 || kt == 11) && cin >= 128 && (cin & 31) == 0 && (cout & 127) == 0;
}
bool conv_split_supported(const PackedConv& w, int dil) {
    return w.wps && conv_split_candidate(w.epi, w.kt, w.cin, w.cout) && (dil == 1 || dil == 3 || dil == 5);
}

// ---- 16-bit-operand convs (conv16.hip) ---------------------------------------------------------------------------------------------------
static int choose_conv16_tile(int rows, int epi, int ncols_max, int mtiles_used, int batch) {
    int tile;
    const bool small_t = ncols_max <= 128;
    // c_out multiple of 128: 128 x 128 tiles (default) read the input tile once per 128 rows at 3 blocks per CU. 128 x 256 tiles
    // (VITS_T16_TILE0=1) hold one block per CU (196 VGPRs: K loop and epilogue run back to back: 33.6 ms per step); 64 x 256 tiles
    // (VITS_T16_TILE0=2: 29.6 ms) overlap epilogue traffic with MFMAs but fetch the input once per 64 rows.
    const int tile0 = kernel_knobs().t16_tile0;
    if (epi == EPI_GATE) tile = small_t ? 3 : 1;
    else if (rows % 128 == 0) tile = small_t ? 3 : (tile0 == 1 ? 0 : tile0 == 2 ? 1 : tile0 == 3 ? 5 : tile0 == 4 ? 3 : 6);
    else if (rows % 64 == 0) tile = small_t ? 3 : 1;
    else tile = small_t ? 4 : 2;
    // small grids (batch 1, short inputs): step down until the launch has >= 512 blocks
    auto blocks = [&](int tl) { return tile_blocks(tile16_shape(tl), ncols_max, mtiles_used, batch); };
    if (blocks(tile) < kSmallGridBlocks && (tile == 0 || tile == 1 || tile == 5 || tile == 6)) tile = 3;
    if (epi != EPI_GATE && blocks(tile) < kSmallGridBlocks && (tile == 3 || tile == 2)) tile = 4;
    return tile;
}

Conv16Plan plan_conv16(const PackedConv& w, const Conv16Call& c) {
    Conv16Plan p;
    const bool group = c.yg || c.y16.p;
    if (w.epi == EPI_CONVT) p.epi16 = group ? C16_CONVT_GROUP : C16_CONVT;
    else if (w.epi == EPI_GATE) p.epi16 = C16_GATE;
    else p.epi16 = group ? C16_GROUP : C16_STD;
    p.dil = conv_dil(w, c);
    p.dil_ct = conv16_template_dil(p.epi16, w.kt, p.dil);
    p.part = p.epi16 != C16_GROUP ? 0 : (w.kt == 7 ? 2 : w.kt == 11 ? 3 : 1);
    p.gz = c.batch;
    if (conv16_lat_wanted(w, c)) {  // (small grids of the wide vocoder stages: conv16_lat.hip)
        // shape (VITS_LAT16H_SHAPE = 10 WM + NR): two row tiles x 32 columns per block by default (batch 1: 1.483 ms against 1.498 with 64 columns and 1.492 with four row tiles x 64)
        const int shape = kernel_knobs().lat16h_shape;
        p.lat = true;
        p.chosen = p.tile = 7;
        p.l = plan_conv16_lat(w.cin, w.cout, w.kt, c.dil, shape, c.t_out, c.batch);
        p.ok = conv16_lat_shape_exists(shape, false);
        return p;
    }
    const int ncols_max = conv_ncols(w, c);
    p.chosen = p.tile = c.tile >= 0 ? c.tile : choose_conv16_tile(w.rows, w.epi, ncols_max, w.mtiles_used, c.batch);
    // steps to an instantiation that exists: the 128-row tiles to 64 x 256, 32 x 256 to 32 x 128
    if ((p.tile == 0 || p.tile == 5 || p.tile == 6) && !conv16_tile_exists(p.epi16, p.dil_ct, p.tile)) p.tile = 1;
    if (p.tile == 2 && !conv16_tile_exists(p.epi16, p.dil_ct, 2)) p.tile = 4;
    const TileShape ts = tile16_shape(p.tile);
    const int span = (w.kt - 1) * p.dil;
    p.lds_off = span < 0 ? -span : 0;
    p.xwp = (ts.bn() + (span < 0 ? -span : span) + 7) / 8 * 8;
    // third LDS buffer where a chunk is less MFMA time than an HBM round trip (~6k cycles): taps x 2 k-halves x MR*NR MFMAs x 32 cycles
    const bool short_chunk = w.kt * 2 * ts.mr * ts.nr * 32 < 6000 && w.nchunks >= 3;
    p.nbuf = short_chunk ? 3 : 2;
    if ((size_t)p.nbuf * 4 * p.xwp * 16 > 150 * 1024) p.nbuf = 2;
    p.lds = (size_t)p.nbuf * 4 * p.xwp * 16;
    p.gx = (ncols_max + ts.bn() - 1) / ts.bn(), p.gy = (w.mtiles_used + ts.bm() - 1) / ts.bm();
    p.ok = w.wp16 && !(p.epi16 == C16_GROUP && (w.cout & 7)) && p.xwp <= 384 && p.dil_ct != kNoKernel && conv16_tile_exists(p.epi16, p.dil_ct, p.tile);
    return p;
}

// ---- conv16_lat.hip ------------------------------------------------------------------------------------------------------------------------
Conv16LatPlan plan_conv16_lat_group(int dil, int tmax, int batch) { return plan_conv16_lat(256, 256, 11, dil, kernel_knobs().lat16h_group_shape, tmax, 3 * batch); }
Conv16LatPlan plan_conv16_lat(int cin, int cout, int kt, int dil, int shape, int tmax, int nz) {
    Conv16LatPlan l;
    l.wm = shape / 10, l.nr = shape % 10;
    l.pitch = conv16_lat_pitch(l.nr, kt, dil);
    l.lds = (size_t)(cin / 8) * l.pitch * 16 + 8 * 16;  // (+ the slots the look-ahead of the last tap reads past the tile, value unused)
    l.gx = (tmax + 32 * l.nr - 1) / (32 * l.nr), l.gy = l.wm ? cout / 32 / l.wm : 0, l.gz = nz, l.block = 64 * l.wm;
    return l;
}

// Which convs: the group-layout ResBlock convs (same length in and out, bias, no activation of the stored value) of a C = 128 / 256
// stage with k = 3 / 7 / 11, while the launch has at most VITS_LAT16H_MAX_TILES (C = 256) / VITS_LAT16H_MAX_TILES_C128 32 x 32 output tiles (one to four utterances).
// Measured (f16, ms per batch of 1 / 2 / 3 / 4 x 128 ids; fused pairs -> this kernel): 1.485 -> 1.428, 1.596 -> 1.553, 1.826 -> 1.780, 1.974 -> 1.939; C = 128 at batch 1 (1792 tiles): + 6 ... 12 us.
bool conv16_lat_shape_ok(int channels, int kt, int dil, int batch, int tmax) {
    const KernelKnobs& kn = kernel_knobs();
    if (kn.no_lat16h) return false;
    if (!(channels == 128 || channels == 256) || !(kt == 3 || kt == 7 || kt == 11) || dil < 1 || (kt - 1) * dil > 50) return false;
    const int64_t tiles = (int64_t)((tmax + 31) / 32) * (channels / 32) * batch;
    return tiles <= (channels == 256 ? kn.lat16h_max_tiles : kn.lat16h_max_tiles_c128);
}
bool conv16_lat_wanted(const PackedConv& w, const Conv16Call& c) {
    if (c.tile >= 0 || w.cin != w.cout || !conv16_lat_shape_ok(w.cin, w.kt, c.dil, c.batch, c.t_out)) return false;
    if (w.epi != EPI_STD || !(c.yg || c.y16.p) || !w.wp16 || !w.bias) return false;
    if (c.len_in != c.len_out || c.t_in != c.t_out || c.post_act != 0 || c.ct_crop != 0 || c.pad_l != (w.kt - 1) * c.dil / 2) return false;
    return !(c.y.p || c.res.p || c.acc.p || c.y2);
}
// The vocoder's conv_pre (F -> up_init channels, k = 7, vits.cpp:601) on a small grid, straight from the fp32 flow output: the converter launch
// (launch_to_group16) and the throughput kernel's 14 us become one launch of conv16_lat_kernel (batch 1: - 15 us). Same rounding expression, same K order,
// same group epilogue: same bits.
bool conv16_lat_pre_wanted(const PackedConv& w, int batch, int tmax) {
    const KernelKnobs& kn = kernel_knobs();
    if (kn.no_lat16h || kn.no_lat16h_pre || !w.wp16 || !w.bias || w.epi != EPI_STD) return false;
    if (w.cin != 192 || w.kt != 7 || (w.cout % 64) != 0) return false;
    const int64_t tiles = (int64_t)((tmax + 31) / 32) * (w.cout / 32) * batch;
    return tiles <= kn.lat16h_max_tiles;
}
// the group launch: members k = 3, 7, 11 of one stage (C = 256), equal shapes; two row tiles x 32 columns per block
bool conv16_lat_group_wanted(const PackedConv* const* w, const Conv16Call* c) {
    if (kernel_knobs().no_lat16h_group) return false;
    static const int kts[3] = {3, 7, 11};
    for (int i = 0; i < 3; ++i) {
        if (!conv16_lat_wanted(*w[i], c[i]) || w[i]->kt != kts[i] || w[i]->cin != 256) return false;
        if (c[i].batch != c[0].batch || c[i].t_out != c[0].t_out || c[i].len_out != c[0].len_out || c[i].dil != c[0].dil) return false;
    }
    return true;
}

}  // namespace vits
