// engine_vocoder.cpp — HiFiGAN (vits.cpp:583-644) over one window of frames: the 16-bit-operand path in the group layout of
// conv16.hip and the exact fp32 path. Window-local lengths throughout (a whole-utterance run is one window).
//
// The two paths differ in layout and in which kernels exist, so they are two functions. Neither decides anything: which kernel a resblock runs on and how the
// resblocks of a stage are scheduled is the host-only planner's answer (vocoder_plan.h: plan_voc_stage16 / plan_voc_stage32 over Engine::voc_policy), the one
// Engine::plan_tile_maps and vits_op_resblock read too. What the paths share is stated once, up here: the stage context (VocStage), how a resblock chain closes
// (ChainEnd + close_chain16 / close_chain32) and the fork / chain / join of the side streams (Engine::rb_*). Inside each function a stage reads: its plan, the
// upsampler, the builders of the call structs, then the schedule the plan names. A launcher that refuses what the plan names is an error.
#include "engine_internal.h"

namespace vits {

namespace {

// One upsampling stage of one window: what both paths read of it. Stage tensors are [C][ts] per utterance in either layout.
struct VocStage {
    const UpStageW& U;
    int i, C, ts, B;                // stage, channels, time stride of the stage's buffers, utterances
    const int *len_in, *len_out;    // device [B]: lengths before / behind the upsampler
    int t_in, t_out;                // their maxima (grid extents)
    int64_t sum_in, sum_out;        // their sums (profiler accounting)
    double n_out;                   // elements of a stage tensor over the real lengths (profiler accounting)
    size_t nk;                      // resblocks per stage
    bool last, refmode;             // the stage in front of conv_post; reference semantics
    float final_slope;              // conv_post's leaky_relu (Q2)
    int64_t g_bs() const { return (int64_t)C * ts; }
    TensorRef ref(float* p) const { return make_ref(p, C, ts); }
    Ref16 ref16(float* p) const {
        Ref16 r;
        r.p = reinterpret_cast<uint16_t*>(p);
        r.ts = ts;
        r.bs = g_bs();
        return r;
    }
};
VocStage voc_stage(const UpStageW& U, int i, size_t nk, const Call& c, const WinCtx& w) {
    const double n_out = (double)U.channels * (double)w.ssum[i + 1];
    return VocStage{U, i, U.channels, c.sts[i + 1], c.B, w.d_len[i], w.d_len[i + 1], w.smax[i], w.smax[i + 1], w.ssum[i], w.ssum[i + 1], n_out, nk, i + 1 == c.n_up, c.refmode, w.final_slope};
}
RoctxRange stage_range(int i) {
    char name[32];
    std::snprintf(name, sizeof(name), "vits.hifigan.stage%d", i);
    return RoctxRange(name);
}

// How the LAST launch of resblock j's chain closes (vits.cpp:622-635). Chained (the default): it writes the shared sum, adds what the chains before
// it left there, and the last chain of the stage also applies the 1/num_kernels scale and the activation of the stage's only reader (leaky_relu in
// front of the next upsampler, vits.cpp:613; conv_post's own slope behind the last stage, Q2). Side by side (sum3): it writes its own buffer and
// nothing else — the stage-sum launch closes the stage, with chain_end(s, nk - 1, false, ...).
struct ChainEnd {
    bool own = false;           // writes the chain's own buffer, not the shared sum
    bool accumulate = false;    // adds the shared sum
    bool closes_stage = false;  // scale + activation: the stage output
    // 16-bit layout: the stage output has ONE reader, through the 16-bit copy, so the fp32 sum of the closing launch is a dead store (4 of its 10-14
    // bytes per element: 1.5 GB per batch of 64 x 128 ids over the four stages) unless VITS_KEEP_STAGE_SUM32 asks for it
    bool dead_sum32 = false;
    float scale = 1.f;  // reference: multiply by float(1 / num_kernels) (ggml_scale, vits.cpp:607); HF divides by num_kernels (modeling_vits.py:546)
    int scale_div = 0;
    bool act = false;      // fp32 layout: leaky_relu(act_slope) of the stored value (the last stage stays raw: conv_post applies its slope itself)
    float act_slope = 1.f;  // 16-bit layout: the slope of the 16-bit copy (the last stage's carries conv_post's)
};
ChainEnd chain_end(const VocStage& s, size_t j, bool sum3, bool keep_stage_sum32, float lrelu) {
    const size_t nk = s.nk;
    ChainEnd e;
    if (sum3) {
        e.own = true;
        return e;
    }
    e.accumulate = j > 0;
    if (j + 1 < nk) return e;
    // (a vocoder with a single resblock kernel has nothing to accumulate and the scale 1/1 is the identity: no special case)
    e.closes_stage = true;
    e.dead_sum32 = !keep_stage_sum32;
    e.scale = s.refmode ? (float)(1.0 / (double)nk) : (float)nk;
    e.scale_div = s.refmode ? 0 : 1;
    e.act = !s.last;
    e.act_slope = s.last ? s.final_slope : lrelu;
    return e;
}
// profiler accounting of the above, 16-bit layout: the accumulator read, the 16-bit copy, the fp32 store that is not made
double close_bytes16(const ChainEnd& e, double n_out) { return (e.accumulate ? 4.0 : 0.0) * n_out + (e.closes_stage ? 2.0 : 0.0) * n_out - (e.dead_sum32 ? 4.0 : 0.0) * n_out; }
// The appliers only copy fields. The call structs of a layout name these fields alike: Conv16Call, RbPair16Call, RbBlock16Call ...
template <class Call16>
void close_chain16(Call16& c, const ChainEnd& e, float* own, float* sum, Ref16 sum16) {
    c.yg = e.own ? own : e.dead_sum32 ? nullptr : sum;
    c.accg = e.accumulate ? sum : nullptr;
    c.scale = e.scale;
    c.scale_div = e.scale_div;
    c.y16 = e.closes_stage ? sum16 : Ref16();
    c.y16_slope = e.closes_stage ? e.act_slope : 1.f;
}
// ... and ConvCall, RbPair32Call, RbBlock32Call
template <class Call32>
void close_chain32(Call32& c, const ChainEnd& e, TensorRef own, TensorRef sum, float lrelu) {
    c.y = e.own ? own : sum;
    c.acc = e.accumulate ? sum : TensorRef();
    c.scale = e.scale;
    c.scale_div = e.scale_div;
    c.post_act = e.act ? 2 : 0;
    if (e.act) c.post_slope = lrelu;
}

}  // namespace

// ---- the side streams of a stage's resblock chains (engine.h: side_[jj - 1] carries the jj-th chain enqueued) ---------------------------------
hipError_t Engine::rb_fork(size_t n_side) {
    hipError_t e = hipEventRecord(ev_fork_, stream);
    for (size_t k = 0; k < n_side && e == hipSuccess; ++k) e = hipStreamWaitEvent(side_[k], ev_fork_, 0);
    return e;
}
// in front of the last launch of resblock j's chain: chained resblocks add into the shared sum in the reference's order, j behind j - 1
hipError_t Engine::rb_chain_wait(const RbChains& r, size_t j, hipStream_t sj) {
    return r.par && j > 0 && !r.sum3 ? hipStreamWaitEvent(sj, ev_done_[j - 1], 0) : hipSuccess;
}
hipError_t Engine::rb_chain_done(const RbChains& r, size_t j, hipStream_t sj) { return r.par ? hipEventRecord(ev_done_[j], sj) : hipSuccess; }
hipError_t Engine::rb_join(const RbChains& r) {
    hipError_t e = r.par ? hipStreamWaitEvent(stream, ev_done_[r.nk - 1], 0) : hipSuccess;
    // (side by side: every chain, not only the last — they no longer wait for each other)
    for (size_t j = 0; r.sum3 && j + 1 < r.nk && e == hipSuccess; ++j) e = hipStreamWaitEvent(stream, ev_done_[j], 0);
    return e;
}

// The handle's knobs and the call's state as the planner takes them. aligned stays true: run_vocoder_window32 tests its buffers once they are laid out.
VocPolicy Engine::voc_policy(const Call& c) const {
    VocPolicy p;
    p.rb_streams = knobs.rb_streams, p.rb16_serial_max_frames = knobs.rb16_serial_max_frames, p.rb16_serial_min_frames = knobs.rb16_serial_min_frames;
    p.rb32_sum3_max_frames = knobs.rb32_sum3_max_frames, p.lrelu_copy_minc = knobs.lrelu_copy_minc;
    p.no_rbblock16 = knobs.no_rbblock16, p.no_fuse32 = knobs.no_fuse32, p.no_rbblock32 = knobs.no_rbblock32, p.no_rb_group = knobs.no_rb_group, p.rb_group_always = knobs.rb_group_always;
    p.prof_on = prof.on, p.fuse16 = c.fuse16, p.arith_now = arith_now_, p.split_on = split_on(), p.split_planes = c.s2.sp_u != nullptr;
    return p;
}

int Engine::run_vocoder_window16(Call& c, WinCtx& w) {
    std::string& err = c.err;
    const int B = c.B, n_up = c.n_up, F = hp.flow_size, Lw = w.Lw;
    Call::S2& s2 = c.s2;
    const size_t nk = hp.rb_k.size();
    const VocPolicy pol = voc_policy(c);
    // ---- 16-bit-operand vocoder in the group layout of conv16.hip -----------------------------------------------
    // Every conv input is a 16-bit tensor WRITTEN by its producer (leaky_relu and rounding fused into the writer's
    // epilogue: what the reference's leaky_relu node + fp16 im2col compute, vits.cpp:554,567,613 + custom-ops.h:684-690);
    // the residual stream (vits.cpp:578) and the resblock sum (:622-635) stay fp32, in the same [c/8][t][8] layout.
    Ref16 z16 = x16_[0];
    z16.ts = round_up(Lw, 8);
    z16.bs = (int64_t)(F / 8) * z16.ts * 8;
    Ref16 cur16;
    cur16.p = reinterpret_cast<uint16_t*>(s2.h0);
    cur16.ts = c.lws;
    cur16.bs = (int64_t)hp.up_init * c.lws;
    // one to four utterances: conv_pre reads the fp32 flow output itself and runs on conv16_lat_kernel (conv16_lat.hip: no converter launch; same bits)
    if (plan_voc_pre_lat(dec_pre_, F, B, Lw, pol)) {
        HIP_OK(launch_conv16_lat_pre(dec_pre_, w.zwin, w.d_len[0], B, Lw, cur16, hp.lrelu, arith_now_, stream, c.spk));
    } else {
        prof.begin("to_group16", 0, 6.0 * F * (double)w.ssum[0], stream, true);
        HIP_OK(launch_to_group16(w.zwin, w.d_len[0], B, F, Lw, 1.0f, z16, arith_now_, stream));
        prof.end(stream);
        Conv16Call cv;
        cv.x = z16;
        cv.len_in = cv.len_out = w.d_len[0];
        cv.spk = c.spk;  // (multi-speaker calls: conv_pre carries the speaker term)
        cv.batch = B;
        cv.t_in = cv.t_out = Lw;
        cv.sum_in = cv.sum_out = w.ssum[0];
        cv.pad_l = (dec_pre_.kt - 1) / 2;
        cv.y16 = cur16;
        cv.y16_slope = hp.lrelu;  // only reader: the first upsampler, behind its leaky_relu (vits.cpp:613)
        HIP_OK(conv16("hifigan_conv_pre", dec_pre_, cv, stream, 2.0 * (F + hp.up_init) * (double)w.ssum[0] + (double)dec_pre_.bytes16));
    }
    for (int i = 0; i < n_up; ++i) {
        const VocStage s = voc_stage(ups_[i], i, nk, c, w);
        const UpStageW& U = s.U;
        RoctxRange rx_stage_range = stage_range(i);
        const int C = s.C;
        const double n_out = s.n_out;
        const Ref16 bul16 = s.ref16(s2.bul), bsum16 = s.ref16(s2.bs16);
        auto chain_end_of = [&](size_t j, bool side_by_side) { return chain_end(s, j, side_by_side, knobs.keep_stage_sum32, hp.lrelu); };

        // ---- the schedule of this stage, before any launch (vocoder_plan.cpp states the rules and the measurements behind them) -------------------------
        const VocStage16Plan pl = plan_voc_stage16(U, B, s.t_out, w.ssum[0], pol);
        const bool par = pl.par, sum3 = pl.sum3;
        const RbChains rb{nk, par, sum3, pl.longest_first};

        // ---- builders -----------------------------------------------------------------------------------------------------------------------
        // conv 1 / conv 2 of pair d of resblock j, on the buffers of chain q. `pingpong` (fused pairs): a fused block reads a halo of its neighbours' input
        // columns while other blocks already write their output, so a fused pair must never write the 16-bit stream it reads: the pairs of the resblock
        // alternate between the two 16-bit buffers the two-kernel path uses for the stream and for t. Returns conv 2's bytes (profiler).
        auto mk_pair = [&](size_t j, size_t d, bool pingpong, Conv16Call& c1, Conv16Call& c2) {
            const ResBlockW& R = U.rbs[j];
            const int q = par ? (int)j : 0;
            const Ref16 byl16 = s.ref16(s2.byl[q]), bt16 = s.ref16(s2.bt[q]);
            c1 = Conv16Call();
            c1.x = d == 0 ? bul16 : (pingpong && (d & 1) == 0 ? bt16 : byl16);
            c1.len_in = c1.len_out = s.len_out;
            c1.batch = B;
            c1.t_in = c1.t_out = s.t_out;
            c1.sum_in = c1.sum_out = s.sum_out;
            c1.dil = R.dil[d];
            c1.pad_l = (R.k * R.dil[d] - R.dil[d]) / 2;
            c1.y16 = bt16;  // t = leaky_relu(conv1(...)), rounded: what the second conv consumes (vits.cpp:556-567)
            c1.y16_slope = hp.lrelu;
            c2 = c1;
            c2.x = bt16;
            c2.dil = 1;
            c2.pad_l = (R.k - 1) / 2;
            c2.g_bs = s.g_bs();
            c2.g_ts = s.ts;
            c2.resg = d == 0 ? s2.bu : s2.by[q];  // residual add (vits.cpp:578), fp32
            const double bytes2 = 2.0 * n_out + 4.0 * n_out + 4.0 * n_out + (double)R.c2[d].bytes16;
            if (d + 1 < R.dil.size()) {
                c2.yg = s2.by[q];
                c2.y16 = pingpong && (d & 1) ? bt16 : byl16;  // next pair's input
                c2.y16_slope = hp.lrelu;
                return bytes2 + 2.0 * n_out;
            }
            const ChainEnd e = chain_end_of(j, sum3);
            close_chain16(c2, e, s2.by[q], s2.bs, bsum16);
            return bytes2 + close_bytes16(e, n_out);
        };
        auto mk_block = [&](size_t j) {
            RbBlock16Call f;
            f.y0 = s2.bu;
            f.lens = s.len_out;
            f.batch = B;
            f.tmax = s.t_out;
            f.slope = hp.lrelu;
            f.g_bs = s.g_bs();
            f.g_ts = s.ts;
            close_chain16(f, chain_end_of(j, sum3), s2.by[par ? j : 0], s2.bs, bsum16);
            return f;
        };
        // the stage output of side-by-side resblocks: their sum in the reference's order, the scale, the 16-bit copy
        auto stage_sum = [&](bool span) -> int {
            const ChainEnd e = chain_end_of(nk - 1, false);
            if (span) prof.begin("hifigan_resblock_sum", 0, (4.0 * nk + 2.0) * n_out, stream);
            HIP_OK(launch_rb_sum3(s2.by[0], s2.by[1], nk > 2 ? s2.by[2] : nullptr, C, s.g_bs(), s.ts, s.len_out, B, s.t_out, e.scale, e.scale_div, e.dead_sum32 ? nullptr : s2.bs, bsum16,
                                  e.act_slope, arith_now_, stream));
            if (span) prof.end(stream);
            return 0;
        };
        // the same-position convs of the three resblocks as ONE launch each (conv16_lat_group_kernel), on the main stream
        auto lat_group = [&]() -> int {
            for (size_t d = 0; d < U.rbs[0].dil.size(); ++d) {
                const PackedConv* w1[3] = {&U.rbs[0].c1[d], &U.rbs[1].c1[d], &U.rbs[2].c1[d]};
                const PackedConv* w2[3] = {&U.rbs[0].c2[d], &U.rbs[1].c2[d], &U.rbs[2].c2[d]};
                Conv16Call a[3], bb[3];
                for (size_t j = 0; j < 3; ++j) mk_pair(j, d, false, a[j], bb[j]);
                HIP_OK(launch_conv16_lat_group(w1, a, arith_now_, stream));
                HIP_OK(launch_conv16_lat_group(w2, bb, arith_now_, stream));
            }
            return 0;
        };

        // ---- the upsampler ------------------------------------------------------------------------------------------------------------------
        {
            Conv16Call cu;
            cu.x = cur16;
            cu.len_in = s.len_in;
            cu.len_out = s.len_out;
            cu.batch = B;
            cu.t_in = s.t_in;
            cu.t_out = s.t_out;
            cu.sum_in = s.sum_in;
            cu.sum_out = s.sum_out;
            cu.ct_crop = s.refmode ? 0 : (U.k - U.stride) / 2;  // Q1
            cu.yg = s2.bu;
            cu.g_bs = s.g_bs();
            cu.g_ts = s.ts;
            if (!pl.all_block) {
                cu.y16 = bul16;
                cu.y16_slope = hp.lrelu;
            }
            const double ct_bytes = 2.0 * U.up.cin * (double)s.sum_in + (pl.all_block ? 4.0 : 6.0) * n_out + (double)U.up.bytes16;
            if (convt16_stream_supported(U.up)) {
                // the upsampler as a streaming kernel (convt16.hip: every phase of a tile of input positions in one block; bit-identical)
                if (prof.on) {
                    char full[160], tag[24];
                    convt16_stream_tag(U.up, tag, sizeof(tag));
                    std::snprintf(full, sizeof(full), "hifigan_upsample_convT|k2|d-1|%s|e2g|c%dx%d", tag, U.up.cin, U.up.cout);
                    prof.begin(full, 2.0 * (double)U.up.rows * (double)U.up.cin * 2.0 * (double)s.sum_in, ct_bytes, stream, true);
                }
                HIP_OK(launch_convt16_stream(U.up, cu, arith_now_, stream));
                prof.end(stream);
            } else {
                HIP_OK(conv16("hifigan_upsample_convT", U.up, cu, stream, ct_bytes));
            }
        }
        cur16 = bsum16;

        // ---- the resblocks: the two single-stream forms of side-by-side resblocks, else one chain of launches per resblock ------------------
        if (pl.group3) {
            const PackedConv* w1[3][3];
            const PackedConv* w2[3][3];
            RbBlock16Call f[3];
            for (int m = 0; m < 3; ++m) {
                U.rbs[m].pairs3(w1[m], w2[m]);
                f[m] = mk_block(m);
            }
            HIP_OK(launch_rbblock16_group3(w1, w2, f, arith_now_, stream));
            if (stage_sum(false)) return -1;
            continue;
        }
        if (pl.lat3) {
            if (lat_group() || stage_sum(false)) return -1;
            continue;
        }
        if (par) HIP_OK(rb_fork(nk - 1));
        for (size_t jj = 0; jj < nk; ++jj) {
            const size_t j = rb.resblock(jj);
            const ResBlockW& R = U.rbs[j];
            const size_t nd = R.dil.size();
            hipStream_t sj = rb_stream(rb, jj);
            const RbKernel kernel = rb_kernel16_of(pl, U, j, B, s.t_out, pol);
            if (kernel == RbKernel::Block) {
                const PackedConv *w1[3], *w2[3];
                R.pairs3(w1, w2);
                const RbBlock16Call f = mk_block(j);
                HIP_OK(rb_chain_wait(rb, j, sj));  // (the accumulation is inside the kernel: the resblocks chain)
                if (prof.on) {
                    char full[160];
                    std::snprintf(full, sizeof(full), "hifigan_resblock_block|k%d|d135|B%d|e0g|c%dx%d", R.k, C, C, C);
                    double bytes = (4.0 + 4.0) * n_out + close_bytes16(chain_end_of(j, sum3), n_out);
                    for (size_t d = 0; d < nd; ++d) bytes += (double)R.c1[d].bytes16 + (double)R.c2[d].bytes16;
                    prof.begin(full, 3.0 * 2.0 * 2.0 * (double)C * C * R.k * (double)s.sum_out, bytes, sj, true);
                }
                HIP_OK(launch_rbblock16(w1, w2, f, arith_now_, sj));
                prof.end(sj);
                HIP_OK(rb_chain_done(rb, j, sj));
                continue;
            }
            const bool fuse = kernel == RbKernel::Pairs;
            for (size_t d = 0; d < nd; ++d) {
                const bool last = d + 1 == nd;
                Conv16Call c1, c2;
                const double bytes2 = mk_pair(j, d, fuse, c1, c2);
                if (!fuse) HIP_OK(conv16("hifigan_resblock_conv1", R.c1[d], c1, sj, 4.0 * n_out + (double)R.c1[d].bytes16));
                if (last) HIP_OK(rb_chain_wait(rb, j, sj));
                if (fuse) {
                    RbPair16Call f;
                    f.x = c1.x;
                    f.lens = s.len_out;
                    f.batch = B;
                    f.tmax = s.t_out;
                    f.dil = R.dil[d];
                    f.slope = hp.lrelu;
                    f.yg = c2.yg;
                    f.resg = c2.resg;
                    f.accg = c2.accg;
                    f.g_bs = s.g_bs();
                    f.g_ts = s.ts;
                    f.y16 = c2.y16;
                    f.y16_slope = c2.y16_slope;
                    f.scale = c2.scale;
                    f.scale_div = c2.scale_div;
                    if (prof.on) {
                        char full[160];
                        std::snprintf(full, sizeof(full), "hifigan_resblock_pair|k%d|d%d|F%d|e0g|c%dx%d", R.k, R.dil[d], C, C, C);
                        prof.begin(full, 2.0 * 2.0 * (double)C * C * R.k * (double)s.sum_out, bytes2 - 2.0 * n_out + (double)R.c1[d].bytes16 + 2.0 * n_out, sj, true);
                    }
                    HIP_OK(launch_rbpair16(R.c1[d], R.c2[d], f, arith_now_, sj));
                    prof.end(sj);
                } else {
                    HIP_OK(conv16("hifigan_resblock_conv2", R.c2[d], c2, sj, bytes2));
                }
                if (last) HIP_OK(rb_chain_done(rb, j, sj));
            }
        }
        HIP_OK(rb_join(rb));
        if (sum3 && stage_sum(true)) return -1;
    }
    prof.begin("hifigan_conv_post_tanh", 2.0 * dec_post_cin_ * dec_post_k_ * (double)w.ssum[n_up], 2.0 * (dec_post_cin_ + 2) * (double)w.ssum[n_up], stream);
    HIP_OK(launch_conv_post16(cur16, dec_post_w_, dec_post_cin_, dec_post_k_, w.pre, w.wv, w.d_len[n_up], B, w.smax[n_up], arith_now_, stream, w.emit_lo, w.emit_hi));
    prof.end(stream);
    return 0;
}

int Engine::run_vocoder_window32(Call& c, WinCtx& w) {
    std::string& err = c.err;
    const int B = c.B, n_up = c.n_up, Lw = w.Lw;
    Call::S2& s2 = c.s2;
    const size_t nk = hp.rb_k.size();
    VocPolicy pol = voc_policy(c);
    // the 16-byte loads of the fused fp32 kernels (the arena aligns every buffer and the strides are rounded up to 32: a guard)
    pol.aligned = ((reinterpret_cast<uintptr_t>(s2.bu) | reinterpret_cast<uintptr_t>(s2.by[0]) | reinterpret_cast<uintptr_t>(s2.bt[0])) & 15) == 0;
    for (int i = 0; i < n_up; ++i) pol.aligned = pol.aligned && (c.sts[i + 1] & 3) == 0;
    TensorRef h0 = make_ref(s2.h0, hp.up_init, c.lws);
    {
        ConvCall cv;
        cv.x = w.zwin;
        cv.y = h0;
        cv.len_in = w.d_len[0];
        cv.len_out = w.d_len[0];
        cv.maps = &w.maps[0];
        cv.spk = c.spk;  // (multi-speaker calls: conv_pre carries the speaker term)
        cv.batch = B;
        cv.t_in = cv.t_out = Lw;
        cv.sum_in = cv.sum_out = w.ssum[0];
        cv.pad_l = (dec_pre_.kt - 1) / 2;  // padding 3 (vits.cpp:601)
        cv.post_act = 2;  // its only reader is the first upsampler, which takes leaky_relu(h0) (vits.cpp:613): activate at the writer
        cv.post_slope = hp.lrelu;
        HIP_OK(conv("hifigan_conv_pre", dec_pre_, cv));
    }
    TensorRef cur = h0;
    for (int i = 0; i < n_up; ++i) {
        const VocStage s = voc_stage(ups_[i], i, nk, c, w);
        const UpStageW& U = s.U;
        RoctxRange rx_stage_range = stage_range(i);
        const int C = s.C;
        const double n_out = s.n_out;
        const TensorRef bu = s.ref(s2.bu), bul = s.ref(s2.bul), bsum = s.ref(s2.bs);
        auto SR = [&](uint16_t* ptr) {
            Split3Ref r;
            r.p = ptr;
            r.ts = s.ts;
            r.ps = s.g_bs();
            r.bs = 3 * r.ps;
            return r;
        };

        // ---- the schedule of this stage, before any launch (vocoder_plan.cpp states the rules and the measurements behind them) -------------------------
        const VocStage32Plan pl = plan_voc_stage32(U, B, s.t_out, w.ssum[0], pol);
        const bool lcopy = pl.lcopy, grouped = pl.grouped, par = pl.par, sum3 = pl.sum3;
        const RbChains rb{nk, par, sum3, sum3};  // (side by side: the last — longest — chain is enqueued first and on the main stream, as the 16-bit path)
        auto is = [&](size_t j, RbKernel k) { return pl.kernel_of(j) == k; };

        // ---- the upsampler ------------------------------------------------------------------------------------------------------------------
        {
            ConvCall cu;
            cu.x = cur;
            cu.y = bu;
            cu.len_in = s.len_in;
            cu.len_out = s.len_out;
            cu.maps = &w.maps_up[i];
            cu.batch = B;
            cu.t_in = s.t_in;
            cu.t_out = s.t_out;
            cu.sum_in = s.sum_in;
            cu.sum_out = s.sum_out;
            cu.pre_act = 0;  // leaky_relu before the upsampler (vits.cpp:613) was applied by whoever wrote `cur`
            cu.slope = hp.lrelu;
            cu.ct_crop = s.refmode ? 0 : (U.k - U.stride) / 2;  // Q1 (vits.cpp:187) / HF padding
            if (lcopy) {
                cu.y2 = s2.bul;
                cu.post_slope = hp.lrelu;
            }
            HIP_OK(conv("hifigan_upsample_convT", U.up, cu));
        }
        cur = bsum;
        if (pl.any_split) {
            prof.begin("split_planes", 0, 10.0 * n_out, stream);
            HIP_OK(launch_split_planes(bu, C, s.len_out, B, s.t_out, hp.lrelu, SR(s2.sp_u), stream));
            prof.end(stream);
        }

        // ---- builders: the call structs of resblock j, on the buffers of chain bufq(j) -------------------------------------------------------
        auto bufq = [&](size_t j) { return (par || grouped) ? (int)j : 0; };  // resblocks that overlap in time need their own (y, t, y') buffers
        // the last launch of resblock j's chain (whichever kernel it is): into the shared sum, or — side by side — its own buffer
        auto close = [&](auto& call, size_t j) { close_chain32(call, chain_end(s, j, sum3, knobs.keep_stage_sum32, hp.lrelu), s.ref(s2.by[bufq(j)]), bsum, hp.lrelu); };
        auto run_block = [&](size_t j, hipStream_t sj) -> int {
            const ResBlockW& R = U.rbs[j];
            const PackedConv *w1[3], *w2[3];
            R.pairs3(w1, w2);
            RbBlock32Call f;
            f.x = bu;
            f.lens = s.len_out;
            f.maps = &w.maps[i + 1];
            f.batch = B;
            f.tmax = s.t_out;
            f.slope = hp.lrelu;
            close(f, j);
            if (prof.on) {
                char full[160];
                std::snprintf(full, sizeof(full), "hifigan_resblock_block|k%d|d135|b%d|e0|c%dx%d", R.k, C, C, C);
                double bytes = 4.0 * n_out * (2 + (f.acc.p ? 1 : 0));
                for (size_t d = 0; d < R.dil.size(); ++d) bytes += (double)R.c1[d].bytes + (double)R.c2[d].bytes;
                prof.begin(full, 3.0 * 2.0 * 2.0 * (double)C * C * R.k * (double)s.sum_out, bytes, sj, true);
            }
            HIP_OK(launch_rbblock32(w1, w2, f, sj));
            prof.end(sj);
            return 0;
        };
        // conv 1 / conv 2 of pair d of resblock j (two-launch form)
        auto mk_c1 = [&](size_t j, size_t d) {
            const ResBlockW& R = U.rbs[j];
            const int q = bufq(j);
            // LeakyReLU is applied where a tensor is WRITTEN, not where it is read: the first conv of a pair stores leaky_relu(t)
            // (t has no other reader), and for wide stages the second conv stores leaky_relu(y) beside y (y itself stays the
            // residual). A reader-side LeakyReLU is VALU work next to the MFMAs — they share the issue port, measured 5 % (k = 11)
            // to 20 % (k = 3) of the K loop — a writer-side one sits in the epilogue.
            ConvCall c1;
            c1.x = lcopy ? (d > 0 ? s.ref(s2.byl[q]) : bul) : (d == 0 ? bu : s.ref(s2.by[q]));
            c1.y = s.ref(s2.bt[q]);
            c1.len_in = c1.len_out = s.len_out;
            c1.maps = &w.maps[i + 1];
            c1.batch = B;
            c1.t_in = c1.t_out = s.t_out;
            c1.sum_in = c1.sum_out = s.sum_out;
            c1.dil = R.dil[d];
            c1.pad_l = (R.k * R.dil[d] - R.dil[d]) / 2;  // vits.cpp:541-543
            c1.pre_act = lcopy ? 0 : 1;
            c1.slope = hp.lrelu;
            c1.post_act = 2;  // bt = leaky_relu(conv1(...)): what the second conv consumes (vits.cpp:556-566)
            c1.post_slope = hp.lrelu;
            if (is(j, RbKernel::Split)) {
                // split arithmetic: the input is the planes of leaky_relu(stage input / stream), the output ONLY the planes of leaky_relu(t)
                c1.x = TensorRef();
                c1.xs3 = d > 0 ? SR(s2.sp_y[q]) : SR(s2.sp_u);
                c1.y = TensorRef();
                c1.ys3 = SR(s2.sp_t[q]);
                c1.ys3_slope = hp.lrelu;
                c1.pre_act = 0;
                c1.post_act = 0;
            }
            return c1;
        };
        auto mk_c2 = [&](size_t j, size_t d) {
            const ResBlockW& R = U.rbs[j];
            const bool last = d + 1 == R.dil.size();
            const int q = bufq(j);
            const TensorRef by = s.ref(s2.by[q]);
            ConvCall c2 = mk_c1(j, d);
            c2.x = s.ref(s2.bt[q]);
            c2.pre_act = 0;
            c2.post_act = 0;
            c2.y2 = (!last && lcopy) ? s2.byl[q] : nullptr;
            c2.dil = 1;
            c2.pad_l = (R.k - 1) / 2;
            c2.res = d == 0 ? bu : by;  // residual add (vits.cpp:578)
            if (is(j, RbKernel::Split)) {
                c2.xs3 = SR(s2.sp_t[q]);
                c2.y2 = nullptr;
                c2.ys3 = Split3Ref();
                if (!last) {
                    c2.ys3 = SR(s2.sp_y[q]);  // planes of leaky_relu(y'): the next pair's first conv
                    c2.ys3_slope = hp.lrelu;
                }
            }
            if (last) close(c2, j);
            else c2.y = by;
            return c2;
        };
        // pair d of resblock j as ONE kernel, t stays in LDS (rbpair32.hip; bit-identical to the two launches). A fused block reads a
        // halo of its neighbours' input columns while other blocks store their output, so the resblock's stream ping-pongs between
        // `by` and the buffer the two-launch path uses for t.
        auto run_fused = [&](size_t j, size_t d, hipStream_t sj) -> int {
            const ResBlockW& R = U.rbs[j];
            const int q = bufq(j);
            const TensorRef by = s.ref(s2.by[q]), bt = s.ref(s2.bt[q]);
            RbPair32Call f;
            f.x = d == 0 ? bu : ((d & 1) ? by : bt);
            f.lens = s.len_out;
            f.maps = &w.maps[i + 1];
            f.batch = B;
            f.tmax = s.t_out;
            f.dil = R.dil[d];
            f.slope = hp.lrelu;
            if (d + 1 == R.dil.size()) close(f, j);
            else f.y = (d & 1) ? bt : by;
            if (prof.on) {
                char full[160];
                std::snprintf(full, sizeof(full), "hifigan_resblock_pair|k%d|d%d|f%d|e0|c%dx%d", R.k, R.dil[d], C, C, C);
                prof.begin(full, 2.0 * 2.0 * (double)C * C * R.k * (double)s.sum_out, 4.0 * n_out * (3 + (f.acc.p ? 1 : 0)) + (double)R.c1[d].bytes + (double)R.c2[d].bytes, sj, true);
            }
            HIP_OK(launch_rbpair32(R.c1[d], R.c2[d], f, sj));
            prof.end(sj);
            return 0;
        };

        if (grouped) {
            // ---- grouped schedule ---------------------------------------------------------------------------------------------------
            const size_t nd = U.rbs[0].dil.size();
            // fused resblocks: their chain up to (not including) the last pair, beside the group — on a side stream unless the profiler
            // needs kernels that do not overlap
            bool any_fused = false;
            for (size_t j = 0; j < nk; ++j) any_fused = any_fused || is(j, RbKernel::Pairs);
            hipStream_t sf = (any_fused && !prof.on) ? side_[0] : stream;
            if (sf != stream) HIP_OK(rb_fork(1));
            for (size_t j = 0; j < nk; ++j)
                if (is(j, RbKernel::Pairs))
                    for (size_t d = 0; d + 1 < nd; ++d)
                        if (run_fused(j, d, sf)) return -1;
            if (sf != stream) HIP_OK(hipEventRecord(ev_done_[0], sf));
            auto run_group = [&](size_t d, bool second) -> int {
                const PackedConv* gw[3];
                ConvCall gc[3];
                int n = 0;
                double flop = 0, bytes = 0;
                for (size_t j = 0; j < nk; ++j) {
                    if (pl.fused(j)) continue;
                    const ResBlockW& R = U.rbs[j];
                    gw[n] = second ? &R.c2[d] : &R.c1[d];
                    gc[n] = second ? mk_c2(j, d) : mk_c1(j, d);
                    const ConvCall& cc = gc[n];
                    flop += conv_flops(*gw[n], cc, s.sum_out);
                    bytes += 4.0 * ((double)C * s.sum_out * (2 + (cc.res.p ? 1 : 0) + (cc.acc.p ? 1 : 0) + (cc.y2 ? 1 : 0))) + (double)gw[n]->bytes;
                    ++n;
                }
                if (prof.on) {
                    char full[160];
                    std::snprintf(full, sizeof(full), "hifigan_resblock_group%d|kG|d%d|G0|e0|c%dx%d", n, second ? 1 : U.rbs[0].dil[d], C, C);
                    prof.begin(full, flop, bytes, stream, /*chain=*/true);
                }
                HIP_OK(launch_conv_group(gw, gc, n, stream));
                prof.end(stream);
                return 0;
            };
            for (size_t d = 0; d < nd; ++d) {
                if (run_group(d, false)) return -1;
                if (d + 1 < nd && run_group(d, true)) return -1;
            }
            // the last launch of every resblock, in the reference's order of the additions
            if (sf != stream) HIP_OK(hipStreamWaitEvent(stream, ev_done_[0], 0));
            for (size_t j = 0; j < nk; ++j) {
                if (is(j, RbKernel::Block)) {
                    if (run_block(j, stream)) return -1;
                } else if (is(j, RbKernel::Pairs)) {
                    if (run_fused(j, nd - 1, stream)) return -1;
                } else {
                    HIP_OK(conv("hifigan_resblock_conv", U.rbs[j].c2[nd - 1], mk_c2(j, nd - 1), stream));
                }
            }
            continue;
        }
        // ---- separate schedule: resblock j on its own stream (engine.h), the last launches chained j-1 -> j by events ---------------
        if (par) HIP_OK(rb_fork(nk - 1));
        for (size_t jj = 0; jj < nk; ++jj) {
            const size_t j = rb.resblock(jj);
            const ResBlockW& R = U.rbs[j];
            const size_t nd = R.dil.size();
            hipStream_t sj = rb_stream(rb, jj);
            const bool fuse_rb = is(j, RbKernel::Pairs);
            if (is(j, RbKernel::Block)) {
                // (the kernel adds into the shared sum: it takes the place of the resblock's last launch in the chain of additions)
                HIP_OK(rb_chain_wait(rb, j, sj));
                if (run_block(j, sj)) return -1;
                HIP_OK(rb_chain_done(rb, j, sj));
                continue;
            }
            for (size_t d = 0; d < nd; ++d) {
                const bool last = d + 1 == nd;
                if (!fuse_rb) HIP_OK(conv("hifigan_resblock_conv", R.c1[d], mk_c1(j, d), sj));
                if (last) HIP_OK(rb_chain_wait(rb, j, sj));
                if (fuse_rb) {
                    if (run_fused(j, d, sj)) return -1;
                } else {
                    HIP_OK(conv("hifigan_resblock_conv", R.c2[d], mk_c2(j, d), sj));
                }
                if (last) HIP_OK(rb_chain_done(rb, j, sj));
            }
        }
        HIP_OK(rb_join(rb));
        if (sum3) {
            const ChainEnd e = chain_end(s, nk - 1, false, knobs.keep_stage_sum32, hp.lrelu);  // (where the last resblock's epilogue would have closed the stage)
            prof.begin("hifigan_resblock_sum", 0, 4.0 * (nk + 1) * n_out, stream);
            HIP_OK(launch_rb_sum3_std(s.ref(s2.by[0]), s.ref(s2.by[1]), nk > 2 ? s.ref(s2.by[2]) : TensorRef(), bsum, C, s.len_out, B, s.t_out, e.scale, e.scale_div, e.act ? 2 : 0, hp.lrelu, stream));
            prof.end(stream);
        }
    }
    prof.begin("hifigan_conv_post_tanh", 2.0 * dec_post_cin_ * dec_post_k_ * (double)w.ssum[n_up], 4.0 * (dec_post_cin_ + 1) * (double)w.ssum[n_up], stream);
    HIP_OK(launch_conv_post(cur, dec_post_w_, dec_post_cin_, dec_post_k_, w.final_slope, w.pre, w.wv, w.d_len[n_up], B, w.smax[n_up], stream, w.emit_lo, w.emit_hi, arith_now_));
    prof.end(stream);
    return 0;
}

}  // namespace vits
