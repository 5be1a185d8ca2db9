// vocoder_plan.cpp — the schedule of a HiFi-GAN stage's resblocks (vocoder_plan.h). Host arithmetic over the predicates of conv_plan.cpp and launch_plan.cpp.
#include "vocoder_plan.h"

namespace vits {

namespace {

bool dils_135(const ResBlockW& R) { return R.dil.size() == 3 && R.dil[0] == 1 && R.dil[1] == 3 && R.dil[2] == 5; }

// What conv16_lat_wanted reads of the call structs the 16-bit path builds for pair d's two convs (its mk_pair): group outputs, equal lengths in and out, the
// pair's dilation and padding. The pointers are only tested for null.
float g_probe_out;
Conv16Call lat_probe(int k, int dil, int B, int t_out) {
    Conv16Call c;
    c.batch = B;
    c.t_in = c.t_out = t_out;
    c.dil = dil;
    c.pad_l = (k * dil - dil) / 2;
    c.yg = &g_probe_out;
    return c;
}
// every conv of the three resblocks goes out in a grouped launch of conv16_lat_group_kernel
bool lat_group_takes(const UpStageW& U, int B, int t_out) {
    for (size_t d = 0; d < U.rbs[0].dil.size(); ++d) {
        const PackedConv* w1[3] = {&U.rbs[0].c1[d], &U.rbs[1].c1[d], &U.rbs[2].c1[d]};
        const PackedConv* w2[3] = {&U.rbs[0].c2[d], &U.rbs[1].c2[d], &U.rbs[2].c2[d]};
        Conv16Call a[3], b[3];
        for (int j = 0; j < 3; ++j) a[j] = lat_probe(U.rbs[j].k, U.rbs[j].dil[d], B, t_out), b[j] = lat_probe(U.rbs[j].k, 1, B, t_out);
        if (!conv16_lat_group_wanted(w1, a) || !conv16_lat_group_wanted(w2, b)) return false;
    }
    return true;
}

}  // namespace

RbHas rb_has(const ResBlockW& R) {
    RbHas h;
    h.split = true;
    for (size_t d = 0; d < R.dil.size(); ++d) {
        const PackedConv &a = R.c1[d], &b = R.c2[d];
        h.bias = h.bias && a.bias && b.bias;
        h.wp = h.wp && a.wp && b.wp;
        h.wp16 = h.wp16 && a.wp16 && b.wp16;
        h.split = h.split && conv_split_supported(a, R.dil[d]) && conv_split_supported(b, 1);
    }
    return h;
}

RbKernel rb_kernel16(int C, int k, const int* dil, int nd, RbHas has, int B, int t_out, const VocPolicy& p) {
    // narrow stages: the RESBLOCK as one kernel (rbblock16.hip: the fp32 stream stays in registers across its three pairs; bit-identical to the pair path)
    if (p.fuse16 && !p.no_rbblock16 && rbblock16_supported(C, k, dil, nd, B, t_out) && has.bias && has.wp16) return RbKernel::Block;
    // each pair as ONE kernel with t in LDS (rbpair16.hip; bit-identical to the two-kernel path) — all pairs of the resblock, or none: a two-kernel pair needs
    // the second 16-bit buffer for its t, which the fused pairs use for the stream
    bool pairs = p.fuse16 && has.bias;
    for (int d = 0; d < nd && pairs; ++d) pairs = rbpair16_supported(C, k, dil[d]);
    if (!pairs) return RbKernel::Convs;
    if (C < 128) return RbKernel::Pairs;
    // one or a few utterances on a wide stage: a fused pair is 28-32 blocks that each stream both convs' weights through one CU; two launches of
    // conv16_lat_kernel deal the rows out over the chip (conv16_lat.hip; same bits)
    bool lat = true;
    for (int d = 0; d < nd && lat; ++d) lat = conv16_lat_shape_ok(C, k, dil[d], B, t_out);
    return lat ? RbKernel::Convs : RbKernel::Pairs;
}

RbKernel rb_kernel32(int C, int k, const int* dil, int nd, RbHas has, const VocPolicy& p) {
    // VITS_ARITH_F32_SPLIT: a resblock the split kernels take (conv_split.hip: C >= 128, any tap count) runs un-fused on them — the C = 128, k = 3 pairs, fused
    // in the exact mode, are 1.56 ms each there and 0.9 as two split convs
    const bool split = p.split_on && p.split_planes && C >= 128 && has.split;
    // Fused pairs (narrow stages; all pairs of a resblock or none). rbpair32 and rbblock32 are fp32 kernels that do not go through the conv wrapper: in a 16-bit
    // arithmetic mode on this (converter) path they would silently compute in fp32 — not the arithmetic that was asked for.
    bool pairs = p.arith_now == VITS_ARITH_F32 && !p.no_fuse32 && has.bias && p.aligned && !split;
    for (int d = 0; d < nd && pairs; ++d) pairs = rbpair32_supported(C, k, dil[d]);
    if (!pairs) return split ? RbKernel::Split : RbKernel::Convs;
    // 3-tap resblocks: the WHOLE resblock as one kernel (rbblock32.hip: the stream stays in registers across its three pairs; bit-identical to the fused pairs)
    return !p.no_rbblock32 && rbblock32_supported(C, k, dil, nd) && has.wp ? RbKernel::Block : RbKernel::Pairs;
}

RbKernel rb_kernel16_of(const VocStage16Plan& pl, const UpStageW& U, size_t j, int B, int t_out, const VocPolicy& p) {
    if (j < (size_t)kVocRb) return pl.rb[j];
    const ResBlockW& R = U.rbs[j];
    VocPolicy q = p;
    q.no_rbblock16 = true;
    return rb_kernel16(U.channels, R.k, R.dil.data(), (int)R.dil.size(), rb_has(R), B, t_out, q);
}

VocStage16Plan plan_voc_stage16(const UpStageW& U, int B, int t_out, int64_t frames, const VocPolicy& p) {
    const KernelKnobs& kn = kernel_knobs();
    const size_t nk = U.rbs.size();
    const int C = U.channels;
    VocStage16Plan pl;
    pl.all_block = nk <= (size_t)kVocRb;
    for (size_t j = 0; j < nk && j < (size_t)kVocRb; ++j) {
        const ResBlockW& R = U.rbs[j];
        pl.rb[j] = rb_kernel16(C, R.k, R.dil.data(), (int)R.dil.size(), rb_has(R), B, t_out, p);
        pl.all_block = pl.all_block && pl.rb[j] == RbKernel::Block;
    }
    // (small windows — up to four 128-id utterances — run the three resblocks one behind the other: a fork and a join cost ~11 us each per stage, more than the
    // overlap of these short kernels returns: f16 batch 4 2.33 -> 2.18 ms, batch 1 -1 %; from batch 8 on three streams win)
    pl.par = p.rb_streams > 1 && nk >= 2 && nk <= 3 && !p.prof_on && (frames > p.rb16_serial_max_frames || frames < p.rb16_serial_min_frames);
    // one or two utterances: the resblocks do NOT chain through the shared sum — each writes its own fp32 output side by side with the others and launch_rb_sum3
    // adds them in the reference's order (rbblock16.hip; same bits; the C = 32 stage at batch 1: three chained 15-25 us kernels + two event hand-overs = 105 us,
    // side by side + the sum ~40)
    pl.sum3 = pl.par && (pl.all_block || !kn.rb_sum3_block_only) && !kn.no_rb_sum3 && frames < p.rb16_serial_min_frames;
    // (side-by-side resblocks need no order: the LAST one, the longest chain (k = 11), is enqueued first and on the main stream, where it starts without the
    // fork's cross-queue hand-over (10-40 us later on the side streams at batch 1); the short k = 3 chain takes the last side stream)
    pl.longest_first = pl.sum3 && !kn.rb_sum3_in_order;
    if (!pl.sum3 || nk != 3 || !p.fuse16) return pl;
    bool same_dils = true, d135 = true;
    for (int m = 0; m < 3; ++m) same_dils = same_dils && U.rbs[m].dil == U.rbs[0].dil, d135 = d135 && dils_135(U.rbs[m]);
    // Side-by-side whole-resblock kernels (the C = 32 and C = 64 stages, k = 3 / 7 / 11) as ONE launch + the sum, on the main stream: no fork, no join (10-30 us
    // of queue hand-over each at batch 1). The members are the kernels' bodies on the same operands: same bits. (The k = 11 member need not pass
    // rbblock16_supported — the group has its own grid rule — but its convs need what every member's need.)
    const RbHas last = rb_has(U.rbs[2]);
    const int kts[3] = {U.rbs[0].k, U.rbs[1].k, U.rbs[2].k};
    pl.group3 = !p.no_rbblock16 && pl.block(0) && pl.block(1) && last.bias && last.wp16 && d135 && rbblock16_group3_supported(C, kts, B, t_out);
    // Side-by-side resblocks whose convs all run on conv16_lat_kernel (the C = 256 stage at one to four utterances): the same-position convs of the three
    // resblocks as ONE launch each, six launches + the sum on the main stream — no fork, no join (each was 20-45 us of queue hand-over per stage at batch 1).
    // Same kernels' bodies on the same operands: same bits.
    pl.lat3 = !pl.group3 && !pl.block(0) && !pl.block(1) && !pl.block(2) && same_dils && lat_group_takes(U, B, t_out);
    return pl;
}

VocStage32Plan plan_voc_stage32(const UpStageW& U, int B, int t_out, int64_t frames, const VocPolicy& p) {
    const KernelKnobs& kn = kernel_knobs();
    const size_t nk = U.rbs.size();
    const int C = U.channels;
    VocStage32Plan pl;
    pl.lcopy = C >= p.lrelu_copy_minc;
    for (size_t j = 0; j < nk && j < (size_t)kVocRb; ++j) {
        const ResBlockW& R = U.rbs[j];
        pl.rb[j] = rb_kernel32(C, R.k, R.dil.data(), (int)R.dil.size(), rb_has(R), p);
        pl.any_split = pl.any_split || pl.rb[j] == RbKernel::Split;
    }
    // The resblocks of a stage (vits.cpp:622-635) are independent chains of conv pairs on the same input that meet only in the sum. Only the LAST launch of each
    // chain touches the shared sum, and those run in the reference's order on the main stream. Everything before them is scheduled one of two ways:
    //   grouped  — the same-position convs of the resblocks as ONE launch (conv_group_kernel: 11-tap blocks first, 3-tap blocks last, one grid tail instead of
    //              three); resblocks that run as fused pairs keep their own chain;
    //   separate — every resblock its own chain of launches, on three streams (or serialised under the profiler).
    // Grouped: at least two un-fused resblocks with distinct tap counts of {11, 7, 3}, the same dilation list, on the 128 x 128 tile (measured, batch 64 x 128
    // ids: serialised launches 79.7 ms per step, grouped 79.1, three streams 76.8 — kernels of DIFFERENT launches share a CU, which blocks of one launch do not
    // (DESIGN.md 4.1), so the streams win where they can be used: the grouped schedule is for the single-stream case, i.e. under the per-kernel profiler;
    // VITS_RB_GROUP=1 forces it)
    pl.grouped = p.arith_now == VITS_ARITH_F32 && !pl.any_split && !p.no_rb_group && nk >= 2 && nk <= 3 && p.rb_streams > 1 && (p.prof_on || p.rb_group_always);
    int members = 0, seen = 0;
    for (size_t j = 0; j < nk && pl.grouped; ++j) {
        const ResBlockW& R = U.rbs[j];
        if (R.dil != U.rbs[0].dil) pl.grouped = false;
        if (pl.fused(j)) continue;
        const int bit = R.k == 11 ? 1 : R.k == 7 ? 2 : R.k == 3 ? 4 : 0;
        if (!bit || (seen & bit)) pl.grouped = false;
        seen |= bit;
        ConvCall shape;  // (what the tile rule looks at: small grids step down from the 128 x 128 tile and are not grouped)
        shape.batch = B;
        shape.t_in = shape.t_out = t_out;
        for (size_t d = 0; d < R.dil.size() && pl.grouped; ++d)
            pl.grouped = conv_group_supported(R.c1[d], R.dil[d]) && conv_group_supported(R.c2[d], 1) && plan_conv(R.c1[d], shape).tile == TILE_128x128;
        ++members;
    }
    pl.grouped = pl.grouped && members >= 2;
    pl.par = p.rb_streams > 1 && nk >= 2 && nk <= 3 && !p.prof_on;
    // separate schedule, up to eight 128-id utterances (small grids): every resblock writes its own output and launch_rb_sum3_std adds them in the reference's
    // order: no resblock's last launch waits for the previous resblock's; same bits. (The last pair of a fused resblock reads bt and writes by: nd is odd.)
    bool odd = true;
    for (size_t j = 0; j < nk; ++j) odd = odd && (U.rbs[j].dil.size() & 1);
    pl.sum3 = !pl.grouped && pl.par && odd && !pl.any_split && !kn.no_rb_sum3 && !kn.no_rb_sum3_f32 && frames < p.rb32_sum3_max_frames;
    return pl;
}

bool plan_voc_pre_lat(const PackedConv& pre, int F, int B, int Lw, const VocPolicy& p) { return !p.prof_on && F == pre.cin && conv16_lat_pre_wanted(pre, B, Lw); }

}  // namespace vits
