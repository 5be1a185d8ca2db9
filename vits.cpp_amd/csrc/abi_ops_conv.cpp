// abi_ops_conv.cpp — operator-level entry points of the convolutions and the vocoder's kernels: host arrays in, host arrays out, the engine's own launchers between
// (staging: abi_ops_common.h). vits_op_set_arith, vits_op_conv1d (with the F32_SPLIT sequence), vits_op_resblock_pair, vits_op_resblock + its plan,
// vits_op_conv_transpose1d, vits_op_upsample16 + its plan.
#include <cstdio>

#include "abi_ops_common.h"

namespace vits {
thread_local int g_op_arith = VITS_ARITH_F32;
thread_local int g_op_out_fill = 0;  // vits_op_set_output_fill: the byte the conv operators' outputs hold before the kernels run
}
using namespace vits;

namespace {
// ---- VITS_ARITH_F32_SPLIT at operator level: the engine's own sequence (pack_conv_weights_split, launch_split_planes, launch_conv_split) or a refusal
// that names its cause — never another kernel, so that a test cannot believe the split kernels ran when they did not.
// three-plane activation buffer [batch][3][channels / 8][ts][8], every byte 0xFF (bf16 NaN): a slot the writer skips (t >= len[b]) and a conv reads shows in the result
bool split3_nan(DevMem& d, int batch, int channels, int ts, Split3Ref* r) {
    if (!d.fill((size_t)batch * 3 * channels * ts * 2, 0xFF)) return false;
    r->p = d.h();
    r->ts = ts;
    r->ps = (int64_t)channels * ts;
    r->bs = 3 * r->ps;
    return true;
}
// why the split kernels do not take a conv (conv_plan.cpp conv_split_candidate / conv_split_supported), or "" if they do
std::string split_refusal(int cin, int cout, int k, int dil) {
    char m[200] = "";
    if (cin < 128 || (cin & 31)) std::snprintf(m, sizeof(m), "VITS_ARITH_F32_SPLIT: c_in = %d is not taken by the split kernels (a multiple of 32, at least 128)", cin);
    else if (cout < 128 || (cout & 127)) std::snprintf(m, sizeof(m), "VITS_ARITH_F32_SPLIT: c_out = %d is not taken by the split kernels (a multiple of 128)", cout);
    else if (k != 3 && k != 7 && k != 11) std::snprintf(m, sizeof(m), "VITS_ARITH_F32_SPLIT: k = %d taps are not taken by the split kernels (3, 7 or 11)", k);
    else if (dil != 1 && dil != 3 && dil != 5) std::snprintf(m, sizeof(m), "VITS_ARITH_F32_SPLIT: dilation %d is not taken by the split kernels (1, 3 or 5)", dil);
    return m;
}
// the split weight planes and the bias of one conv on the device; false: the error text names the cause when the split kernels do not take it
bool split_conv_upload(const float* w, const float* bias, int cout, int cin, int k, int dil, PackedConv& pc, DevMem& dw, DevMem& db) {
    const std::string why = split_refusal(cin, cout, k, dil);
    if (!why.empty()) return refuse(why);
    std::vector<uint16_t> packed;
    if (!pack_conv_weights_split(w, cout, cin, k, packed))
        return refuse("VITS_ARITH_F32_SPLIT: a weight is not the exact sum of two bf16 values (the split kernels take fp16- or bf16-valued weights)");
    if (!dw.put(packed.data(), packed.size() * 2) || (bias && !db.put(bias, (size_t)cout * 4))) return false;
    pc.cin = cin;
    pc.cout = cout;
    pc.kt = k;
    pc.epi = EPI_STD;
    pc.nchunks = (cin + 31) / 32;
    pc.wps = dw.h();
    pc.bytes_s = (int64_t)packed.size() * 2;
    pc.bias = db.f();
    if (!conv_split_supported(pc, dil)) return refuse("VITS_ARITH_F32_SPLIT: conv_split_supported refuses this conv");
    return true;
}
int op_conv1d_split(const vits_conv1d_desc* d, const float* x, const float* w, const float* bias, const float* residual, const float* accum, const int32_t* lens, float* y) {
    if (d->post_act != 0) return fail("VITS_ARITH_F32_SPLIT: post_act (relu / gate) does not exist on the split kernels");
    if (!shape_lens_ok(lens, d->batch, d->t, d->t_stride)) return fail("VITS_ARITH_F32_SPLIT: 0 <= lens[b] <= t <= t_stride is required");
    PackedConv pc;
    DevMem dw, dxs, db, dx, dy, dr, da, dl;
    if (!split_conv_upload(w, bias, d->cout, d->cin, d->k, d->dilation, pc, dw, db)) return -1;
    const size_t nx = (size_t)d->batch * d->cin * d->t_stride * 4, ny = (size_t)d->batch * d->cout * d->t_stride * 4;
    Split3Ref xs;
    if (!dx.put(x, nx) || !dy.fill(ny, 0) || !dl.put_opt(lens, (size_t)d->batch * 4) || !split3_nan(dxs, d->batch, d->cin, d->t_stride, &xs)) return -1;
    if ((residual && !dr.put(residual, ny)) || (accum && !da.put(accum, ny))) return -1;
    hipError_t e = launch_split_planes(tref(dx.f(), d->cin, d->t_stride), d->cin, dl.i(), d->batch, d->t, d->pre_act ? d->pre_slope : 1.0f, xs, nullptr);
    if (e == hipSuccess) {
        ConvCall c;
        c.xs3 = xs;
        c.y = tref(dy.f(), d->cout, d->t_stride);
        if (residual) c.res = tref(dr.f(), d->cout, d->t_stride);
        if (accum) c.acc = tref(da.f(), d->cout, d->t_stride);
        c.len_in = c.len_out = dl.i();
        c.batch = d->batch;
        c.t_in = c.t_out = d->t;
        c.dil = d->dilation;
        c.pad_l = d->pad_left;
        c.scale = d->out_scale;
        e = launch_conv_split(pc, c, nullptr);
    }
    return finish(e) && dy.get(y, ny) ? 0 : -1;
}
// conv 1 / conv 2 of a ResBlock pair as engine_vocoder.cpp builds them (mk_c1 / mk_c2), without their tensors
void pair_calls(const int* lens, int batch, int t, int k, int dil, ConvCall& c1, ConvCall& c2) {
    c1.len_in = c1.len_out = lens;
    c1.batch = batch;
    c1.t_in = c1.t_out = t;
    c1.dil = dil;
    c1.pad_l = (k * dil - dil) / 2;
    c2 = c1;
    c2.dil = 1;
    c2.pad_l = (k - 1) / 2;
}
}  // namespace

VITS_API int vits_op_set_arith(int32_t arith) {
    if (arith != VITS_ARITH_F32 && arith != VITS_ARITH_BF16 && arith != VITS_ARITH_F16 && arith != VITS_ARITH_F32_SPLIT) return fail("bad arithmetic mode");
    g_op_arith = arith;
    return 0;
}

VITS_API int vits_op_set_output_fill(int32_t byte) {
    if (byte != 0 && byte != 0xFF) return fail("vits_op_set_output_fill: 0 (zeros) or 0xFF (NaN)");
    g_op_out_fill = byte;
    return 0;
}

// The same-position convolutions of two or three ResBlocks as ONE launch (launch_conv_group), each member as the engine builds the first conv of a pair
// (mk_c1: leaky_relu on load, its result stored activated). Outputs are staged as 0xFF bytes.
VITS_API int vits_op_conv_group(const vits_conv_group_desc* d, const float* x, const float* w, const float* bias, const int32_t* lens, float* y) {
    VITS_TRY
    if (!d || !x || !w || !y) return fail("vits_op_conv_group: null argument");
    if (g_op_arith != VITS_ARITH_F32) return fail("vits_op_conv_group: VITS_ARITH_F32 only");
    if (d->n < 2 || d->n > 3) return fail("vits_op_conv_group: two or three members");
    if (!shape_lens_ok(lens, d->batch, d->t, d->t_stride)) return fail("vits_op_conv_group: 0 <= lens[b] <= t <= t_stride is required");
    OpKnobs op_knobs;
    OpTileMaps maps;
    const int B = d->batch, C = d->channels, n = d->n;
    const size_t per = (size_t)B * C * d->t_stride;
    Conv cv[3];
    ConvCall cc[3];
    const PackedConv* pw[3];
    DevMem dx, dy, dl;
    if (!dx.put(x, per * n * 4) || !dy.fill(per * n * 4, 0xFF) || !dl.put_opt(lens, (size_t)B * 4)) return -1;
    if (!maps.add(lens, lens, B, d->t, d->t, tile_shape(TILE_128x128).bn(), false)) return -1;
    size_t woff = 0;
    for (int i = 0; i < n; ++i) {
        const int k = d->k[i];
        if (k != 3 && k != 7 && k != 11) return fail("vits_op_conv_group: tap counts 11, 7 or 3");
        if (!upload_conv(cv[i], w + woff, bias ? bias + (size_t)i * C : nullptr, C, C, C, k, EPI_STD, 0, VITS_ARITH_F32)) return -1;
        woff += (size_t)C * C * k;
        if (!conv_group_supported(cv[i].pc, d->dilation)) return fail("vits_op_conv_group: conv_group_supported refuses this conv (channels a multiple of 128, dilation 1, 3 or 5)");
        ConvCall& c = cc[i];
        c.x = tref(dx.f() + per * i, C, d->t_stride);
        c.y = tref(dy.f() + per * i, C, d->t_stride);
        c.len_in = c.len_out = dl.i();
        c.maps = &maps.set;
        c.batch = B;
        c.t_in = c.t_out = d->t;
        c.dil = d->dilation;
        c.pad_l = (k * d->dilation - d->dilation) / 2;
        c.pre_act = 1, c.slope = d->slope, c.post_act = 2, c.post_slope = d->slope;
        pw[i] = &cv[i].pc;
    }
    return finish(launch_conv_group(pw, cc, n, nullptr), "vits_op_conv_group") && dy.get(y, per * n * 4) ? 0 : -1;
    VITS_CATCH(-1)
}

VITS_API uint64_t vits_op_tile_map_launches(void) { return tile_map_launches().load(std::memory_order_relaxed); }

VITS_API int vits_op_conv1d(const vits_conv1d_desc* d, const float* x, const float* w, const float* bias, const float* residual, const float* accum,
                            const int32_t* lens, float* y) {
    VITS_TRY
    if (!d || !x || !w || !y) return fail("null argument");
    const int arith = g_op_arith;
    if (arith == VITS_ARITH_F32_SPLIT) return op_conv1d_split(d, x, w, bias, residual, accum, lens, y);
    OpKnobs op_knobs;
    OpTileMaps maps;
    const int gate = d->post_act == 2;
    const int cy = gate ? d->cout / 2 : d->cout;
    Conv cv;
    DevMem dx, dy, dr, da, dl, x16;
    const size_t nx = (size_t)d->batch * d->cin * d->t_stride * 4, ny = (size_t)d->batch * cy * d->t_stride * 4;
    if (!upload_conv(cv, w, bias, d->cout, d->cout, d->cin, d->k, gate ? EPI_GATE : EPI_STD, 0, arith)) return -1;
    if (!dx.put(x, nx) || !dy.fill(ny, g_op_out_fill) || !dl.put_opt(lens, (size_t)d->batch * 4)) return -1;
    if ((residual && !dr.put(residual, ny)) || (accum && !da.put(accum, ny))) return -1;
    if (arith != VITS_ARITH_F32 && !x16.fill(group16_bytes(d->batch, d->cin, d->t), 0)) return -1;
    ConvCall c;
    c.x = tref(dx.f(), d->cin, d->t_stride);
    c.y = tref(dy.f(), cy, d->t_stride);
    if (residual) c.res = tref(dr.f(), cy, d->t_stride);
    if (accum) c.acc = tref(da.f(), cy, d->t_stride);
    c.len_in = dl.i();
    c.len_out = dl.i();
    c.batch = d->batch;
    c.t_in = c.t_out = d->t;
    c.dil = d->dilation;
    c.pad_l = d->pad_left;
    c.pre_act = d->pre_act;
    c.slope = d->pre_slope;
    c.post_act = d->post_act == 1 ? 1 : 0;
    c.scale = d->out_scale;
    if (arith == VITS_ARITH_F32) {  // (the lists are the fp32 kernels')
        if (!maps.add_conv(lens, lens, d->batch, d->t, d->t, false)) return -1;
        c.maps = &maps.set;
    }
    return finish(conv_transparent(cv.pc, c, arith, x16)) && dy.get(y, ny) ? 0 : -1;
    VITS_CATCH(-1)
}

VITS_API int vits_op_resblock_pair(const vits_resblock_pair_desc* d, const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                                   const int32_t* lens, float* y) {
    VITS_TRY
    if (!d || !x || !w1 || !w2 || !y) return fail("null argument");
    if (g_op_arith != VITS_ARITH_F32 && g_op_arith != VITS_ARITH_F32_SPLIT) return fail("vits_op_resblock_pair: VITS_ARITH_F32 or VITS_ARITH_F32_SPLIT only");
    if (!shape_lens_ok(lens, d->batch, d->t, d->t_stride)) return fail("vits_op_resblock_pair: 0 <= lens[b] <= t <= t_stride is required");
    if (d->channels < 1 || d->k < 1 || !(d->k & 1) || d->dilation < 1) return fail("vits_op_resblock_pair: an odd tap count and a dilation >= 1 are required");
    const int C = d->channels, k = d->k;
    const size_t n = (size_t)d->batch * C * d->t_stride * 4;
    DevMem dx, dy, dl;
    if (!dx.put(x, n) || !dy.fill(n, g_op_out_fill) || !dl.put_opt(lens, (size_t)d->batch * 4)) return -1;
    const TensorRef bx = tref(dx.f(), C, d->t_stride), by = tref(dy.f(), C, d->t_stride);
    ConvCall c1, c2;
    pair_calls(dl.i(), d->batch, d->t, k, d->dilation, c1, c2);
    c2.res = bx;
    c2.y = by;
    hipError_t e;
    Conv v1, v2;
    DevMem ws1, ws2, db1, db2, du, dt, bt;
    if (g_op_arith == VITS_ARITH_F32_SPLIT) {
        if (!split_conv_upload(w1, b1, C, C, k, d->dilation, v1.pc, ws1, db1) || !split_conv_upload(w2, b2, C, C, k, 1, v2.pc, ws2, db2)) return -1;
        Split3Ref su, st;
        if (!split3_nan(du, d->batch, C, d->t_stride, &su) || !split3_nan(dt, d->batch, C, d->t_stride, &st)) return -1;
        // the un-fused split resblock: planes of leaky_relu(x); conv 1 writes ONLY the planes of leaky_relu(t); conv 2 reads them, res = x
        c1.xs3 = su;
        c1.ys3 = st;
        c1.ys3_slope = d->slope;
        c2.xs3 = st;
        e = launch_split_planes(bx, C, dl.i(), d->batch, d->t, d->slope, su, nullptr);
        if (e == hipSuccess) e = launch_conv_split(v1.pc, c1, nullptr);
        if (e == hipSuccess) e = launch_conv_split(v2.pc, c2, nullptr);
    } else {
        if (!upload_conv(v1, w1, b1, C, C, C, k, EPI_STD, 0, VITS_ARITH_F32) || !upload_conv(v2, w2, b2, C, C, C, k, EPI_STD, 0, VITS_ARITH_F32) || !bt.fill(n, 0)) return -1;
        c1.x = bx;
        c1.y = tref(bt.f(), C, d->t_stride);
        c1.pre_act = 1;
        c1.slope = d->slope;
        c1.post_act = 2;  // t is stored activated: its only reader is conv 2
        c1.post_slope = d->slope;
        c2.x = c1.y;
        OpKnobs op_knobs;
        OpTileMaps maps;
        if (!maps.add_conv(lens, lens, d->batch, d->t, d->t, false)) return -1;
        c1.maps = c2.maps = &maps.set;
        e = launch_conv(v1.pc, c1, nullptr);
        if (e == hipSuccess) e = launch_conv(v2.pc, c2, nullptr);
        if (!finish(e)) return -1;  // (the lists live until the device is done)
    }
    return finish(e) && dy.get(y, n) ? 0 : -1;
    VITS_CATCH(-1)
}

// ---- vits_op_resblock: which kernel a descriptor names (host arithmetic only: launch_plan.h), then the engine's call structs on staged tensors ------------
namespace {
struct RbOpPlan {
    int variant = 0;
    std::string kernel;
    int bo = 0, adv = 0, halo = 0, seg = 0, tiles = 1, nr = 0, launches = 0;
    LaunchGrid g;
};
bool rb_fail(std::string& why, const std::string& m) {
    why = "vits_op_resblock: " + m;
    return false;
}
bool resblock_resolve(const vits_resblock_desc* d, int arith, RbOpPlan& r, std::string& why) {
    if (arith != VITS_ARITH_F32 && arith != VITS_ARITH_F16 && arith != VITS_ARITH_BF16)
        return rb_fail(why, "VITS_ARITH_F32, VITS_ARITH_F16 or VITS_ARITH_BF16 only (the split arithmetic keeps vits_op_resblock_pair)");
    const int C = d->channels, k = d->k, B = d->batch, T = d->t, nd = d->ndil;
    if (B < 1 || T < 1 || d->t_stride < T) return rb_fail(why, "batch >= 1 and 1 <= t <= t_stride are required");
    if (C < 32 || (C & 31)) return rb_fail(why, "channels = " + std::to_string(C) + ": a multiple of 32 is required");
    if (k < 1 || !(k & 1)) return rb_fail(why, "k = " + std::to_string(k) + ": an odd tap count is required");
    if (nd < 1 || nd > 3) return rb_fail(why, "ndil = " + std::to_string(nd) + ": one to three conv pairs");
    for (int p = 0; p < nd; ++p)
        if (d->dil[p] < 1) return rb_fail(why, "dilation " + std::to_string(d->dil[p]) + ": >= 1 is required");
    if (d->variant < 0 || d->variant > 4) return rb_fail(why, "variant " + std::to_string(d->variant) + ": 0 (the engine's choice), 1 (un-fused), 2 (fused pairs), 3 (whole ResBlock), 4 (segments of tiles)");
    const bool f32 = arith == VITS_ARITH_F32, bf = arith == VITS_ARITH_BF16;
    const bool d135 = nd == 3 && d->dil[0] == 1 && d->dil[1] == 3 && d->dil[2] == 5;
    const std::string shape = "C = " + std::to_string(C) + ", k = " + std::to_string(k);
    char name[96];
    int v = d->variant;
    if (v == 0) {  // the engine's per-resblock rule (vocoder_plan.h) on the operator's weights (every plane, a bias) and a handle's default knobs
        const RbKernel kernel = f32 ? rb_kernel32(C, k, d->dil, nd, RbHas(), VocPolicy()) : rb_kernel16(C, k, d->dil, nd, RbHas(), B, T, VocPolicy());
        v = kernel != RbKernel::Block ? (kernel == RbKernel::Pairs ? 2 : 1) : !f32 && plan_rbblock16(C, k, B, T).nt > 1 ? 4 : 3;
    }
    r.variant = v;
    if (v == 1) {
        r.kernel = f32 ? "launch_conv" : "launch_conv16";
        r.launches = 2 * nd;
        return true;
    }
    if (v == 2) {
        if (d->nr != 0 && (f32 || C < 128)) return rb_fail(why, "nr = " + std::to_string(d->nr) + ": only the 16-bit pairs at C >= 128 have a choice of column tiles");
        for (int p = 0; p < nd; ++p) {
            const int dil = d->dil[p];
            LaunchGrid g;
            int nr = 0;
            if (f32) {
                if (!rbpair32_exists(k, dil, C)) return rb_fail(why, "variant 2: no rbpair32_kernel for " + shape + ", dilation " + std::to_string(dil) + " (k in {3, 7, 11}, dilation in {1, 3, 5}, C = 32, 64, or 128 with k = 3)");
                g = plan_rbpair32(C, k, dil, B, T);
                if (!g.ok) return rb_fail(why, "variant 2: plan_rbpair32 refuses " + shape + " (VITS_FUSE32_C128=0)");
            } else {
                const RbPair16Plan pl = d->nr ? plan_rbpair16(C, k, dil, B, T, d->nr) : plan_rbpair16(C, k, dil, B, T);
                if (!pl.ok) return rb_fail(why, "variant 2: no rbpair16_kernel for " + shape + ", dilation " + std::to_string(dil) + ", nr = " + std::to_string(d->nr) + " (k in {3, 7, 11}, dilation in {1, 3, 5}, C in {32, 64, 128, 256}, nr 4 or " + std::to_string(VITS_RB16_NARROW_NR) + " at C >= 128)");
                g = pl, nr = pl.nr;
            }
            if (p > 0) continue;  // the plan query describes the first pair; every pair is checked
            r.g = g, r.nr = nr;
            if (f32) {
                const RbPair32Geom ge = rbpair32_geom(k, dil, C);
                r.bo = ge.bo;
                std::snprintf(name, sizeof(name), "rbpair32_kernel<%d, %d, %d>", k, dil, C);
            } else {
                const RbPair16Geom ge = rbpair16_geom(k, dil, C, nr);
                r.bo = ge.bo;
                std::snprintf(name, sizeof(name), "rbpair16_kernel<%d, %d, %d, %d, %s, %s>", k, dil, C, nr, bf ? "true" : "false", ge.rows ? "true" : "false");
            }
            r.adv = r.seg = r.bo;
            r.halo = (k - 1) / 2 * (1 + dil);
            r.kernel = name;
        }
        r.launches = nd;
        return true;
    }
    // variants 3 and 4: the whole-ResBlock kernels
    if (!d135) return rb_fail(why, "variant " + std::to_string(v) + ": the whole-ResBlock kernels take three pairs with dilations 1, 3, 5");
    if (v == 4 && f32) return rb_fail(why, "variant 4: segments of tiles exist in the 16-bit modes only (rbblock32_kernel is one tile per block)");
    if (d->variant == 4 && d->tiles < 2) return rb_fail(why, "variant 4: tiles = " + std::to_string(d->tiles) + ", at least 2 are required");
    if (f32) {
        const RbBlock32Plan pl = plan_rbblock32(C, k, B, T);
        if (!pl.ok) return rb_fail(why, "variant 3: no rbblock32_kernel for " + shape + " (k = 3, C = 32 or 64)");
        const RbBlock32Geom ge = rbblock32_geom(C, pl.nr);
        r.g = pl, r.nr = pl.nr, r.bo = r.adv = r.seg = ge.bo, r.halo = ge.h;
        std::snprintf(name, sizeof(name), "rbblock32_kernel<%d, %d>", C, pl.nr);
    } else {
        const int nt = d->variant == 0 ? plan_rbblock16(C, k, B, T).nt : v == 4 ? d->tiles : 1;
        const RbBlock16Plan pl = plan_rbblock16(C, k, B, T, false, nt);
        if (!pl.ok) return rb_fail(why, "variant " + std::to_string(v) + ": no rbblock16_kernel for " + shape + " (k in {3, 7, 11} at C = 32 or 64, k = 3 at C = 128)");
        const RbBlock16Geom ge = rbblock16_geom(k, C);
        r.g = pl, r.tiles = nt, r.bo = ge.bo, r.adv = nt > 1 ? ge.adv : ge.bo, r.seg = ge.seg_out(nt), r.halo = ge.h;
        std::snprintf(name, sizeof(name), "rbblock16_kernel<%d, %d, %d, %d, %d, 1, 3, 5, %s, %s>", k, C, pl.tile.nstrip, pl.tile.nrw, pl.tile.mrw, bf ? "true" : "false", nt > 1 ? "true" : "false");
    }
    r.kernel = name;
    r.launches = 1;
    return true;
}
}  // namespace

VITS_API int vits_op_resblock_plan(const vits_resblock_desc* d, vits_resblock_plan* out) {
    VITS_TRY
    if (!d || !out) return fail("vits_op_resblock_plan: null argument");
    RbOpPlan r;
    std::string why;
    if (!resblock_resolve(d, g_op_arith, r, why)) return fail(why);
    std::memset(out, 0, sizeof(*out));
    std::snprintf(out->kernel, sizeof(out->kernel), "%s", r.kernel.c_str());
    out->variant = r.variant, out->bo = r.bo, out->advance = r.adv, out->halo = r.halo, out->segment = r.seg, out->tiles = r.tiles, out->nr = r.nr;
    out->grid_x = r.g.gx, out->grid_y = r.g.gy, out->grid_z = r.g.ok ? r.g.gz : 0, out->block = r.g.block, out->lds = (int64_t)r.g.lds, out->launches = r.launches;
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_op_resblock(const vits_resblock_desc* d, const float* x, const float* w1, const float* b1, const float* w2, const float* b2, const float* accum,
                              const int32_t* lens, float* y) {
    VITS_TRY
    if (!d || !x || !w1 || !b1 || !w2 || !b2 || !y) return fail("vits_op_resblock: null argument (x, w1, b1, w2, b2 and y are required)");
    const int arith = g_op_arith;
    RbOpPlan r;
    std::string why;
    if (!resblock_resolve(d, arith, r, why)) return fail(why);
    const int B = d->batch, C = d->channels, T = d->t, k = d->k, nd = d->ndil, ts = round_up(T, 32);
    if (!lens_ok(lens, B, T)) return fail("vits_op_resblock: 0 <= lens[b] <= t is required");
    const bool f32 = arith == VITS_ARITH_F32;
    const size_t n = (size_t)B * C * ts, wn = (size_t)C * C * k;
    std::vector<Conv> cv(2 * nd);  // pair p: conv 1 = cv[2 p], conv 2 = cv[2 p + 1]
    for (int i = 0; i < 2 * nd; ++i)
        if (!upload_conv(cv[i], (i & 1 ? w2 : w1) + (size_t)(i / 2) * wn, (i & 1 ? b2 : b1) + (size_t)(i / 2) * C, C, C, C, k, EPI_STD, 0, arith)) return -1;
    // staged at the engine's stride with NaN behind every lens[b]; the fp32 kernels take the standard layout, the 16-bit ones the group layout
    DevMem dl, dx, dxg, dacc, dout, dp[2], dt, dx16, dn16[2], dt16;
    if (!dl.put_opt(lens, (size_t)B * 4) || !stage_rows(dx, x, B, C, d->t_stride, ts, lens, T) || !dout.fill(n * 4, g_op_out_fill) || !dp[0].fill(n * 4, 0xFF) || !dp[1].fill(n * 4, 0xFF)) return -1;
    if (accum && !(f32 ? stage_rows(dacc, accum, B, C, d->t_stride, ts, lens, T) : stage_group8(dacc, accum, B, C, d->t_stride, ts, lens, T))) return -1;
    hipError_t e = hipSuccess;
    const float scale = d->out_scale;
    OpKnobs op_knobs;
    OpTileMaps maps;
    if (f32) {
        if (r.variant == 1 && !dt.fill(n * 4, 0xFF)) return -1;
        const TensorRef bx = tref(dx.f(), C, ts), bout = tref(dout.f(), C, ts), bacc = accum ? tref(dacc.f(), C, ts) : TensorRef();
        // the lists of existing tiles of `lens`, for the widths of the variant's kernels
        bool mok = r.variant == 1 ? maps.add_conv(lens, lens, B, T, T, false) : r.variant == 3 ? maps.add(lens, lens, B, T, T, r.bo, false) : true;
        for (int p = 0; p < nd && mok && r.variant == 2; ++p) mok = maps.add(lens, lens, B, T, T, rbpair32_geom(k, d->dil[p], C).bo, false);
        if (!mok) return -1;
        if (r.variant == 3) {
            const PackedConv *c1[3] = {&cv[0].pc, &cv[2].pc, &cv[4].pc}, *c2[3] = {&cv[1].pc, &cv[3].pc, &cv[5].pc};
            RbBlock32Call f;
            f.x = bx, f.y = bout, f.acc = bacc, f.lens = dl.i(), f.batch = B, f.tmax = T, f.slope = d->slope, f.scale = scale, f.scale_div = d->scale_div;
            f.maps = &maps.set;
            e = launch_rbblock32(c1, c2, f, nullptr);
        } else {
            TensorRef in = bx;
            for (int p = 0; p < nd && e == hipSuccess; ++p) {
                const bool last = p + 1 == nd;
                const TensorRef out = last ? bout : tref(dp[p & 1].f(), C, ts);  // a pair never writes the buffer it reads
                if (r.variant == 2) {
                    RbPair32Call f;
                    f.x = in, f.y = out, f.lens = dl.i(), f.batch = B, f.tmax = T, f.dil = d->dil[p], f.slope = d->slope;
                    f.maps = &maps.set;
                    if (last) f.acc = bacc, f.scale = scale, f.scale_div = d->scale_div;
                    e = launch_rbpair32(cv[2 * p].pc, cv[2 * p + 1].pc, f, nullptr);
                } else {
                    // t is stored activated, its only reader is conv 2
                    ConvCall c1, c2;
                    pair_calls(dl.i(), B, T, k, d->dil[p], c1, c2);
                    c1.x = in, c1.y = tref(dt.f(), C, ts);
                    c1.maps = c2.maps = &maps.set;
                    c1.pre_act = 1, c1.slope = d->slope, c1.post_act = 2, c1.post_slope = d->slope;
                    c2.x = c1.y, c2.res = in, c2.y = out;
                    if (last) c2.acc = bacc, c2.scale = scale, c2.scale_div = d->scale_div;
                    e = launch_conv(cv[2 * p].pc, c1, nullptr);
                    if (e == hipSuccess) e = launch_conv(cv[2 * p + 1].pc, c2, nullptr);
                }
                in = out;
            }
        }
    } else {
        // group layout: the fp32 stream, and the 16-bit copy of leaky_relu(y_0) from the engine's converter
        const int64_t g_bs = (int64_t)C * ts;
        auto r16 = [&](const DevMem& m) {
            Ref16 q;
            q.p = m.h(), q.ts = ts, q.bs = g_bs;
            return q;
        };
        if (!stage_group8(dxg, x, B, C, d->t_stride, ts, lens, T)) return -1;
        const float* accg = accum ? dacc.f() : nullptr;
        if (r.variant >= 3) {
            const PackedConv *c1[3] = {&cv[0].pc, &cv[2].pc, &cv[4].pc}, *c2[3] = {&cv[1].pc, &cv[3].pc, &cv[5].pc};
            RbBlock16Call f;
            f.y0 = dxg.f(), f.lens = dl.i(), f.batch = B, f.tmax = T, f.slope = d->slope, f.yg = dout.f(), f.accg = accg, f.g_bs = g_bs, f.g_ts = ts;
            f.scale = scale, f.scale_div = d->scale_div, f.force_nt = r.tiles;
            e = launch_rbblock16(c1, c2, f, arith, nullptr);
        } else {
            if (!dx16.fill(n * 2, 0xFF) || !dn16[0].fill(n * 2, 0xFF) || !dn16[1].fill(n * 2, 0xFF) || (r.variant == 1 && !dt16.fill(n * 2, 0xFF))) return -1;
            e = launch_to_group16(tref(dx.f(), C, ts), dl.i(), B, C, T, d->slope, r16(dx16), arith, nullptr);
            const float* ing = dxg.f();
            Ref16 in16 = r16(dx16);
            for (int p = 0; p < nd && e == hipSuccess; ++p) {
                const bool last = p + 1 == nd;
                float* outg = last ? dout.f() : dp[p & 1].f();
                const Ref16 out16 = last ? Ref16() : r16(dn16[p & 1]);
                if (r.variant == 2) {
                    RbPair16Call f;
                    f.x = in16, f.lens = dl.i(), f.batch = B, f.tmax = T, f.dil = d->dil[p], f.slope = d->slope, f.yg = outg, f.resg = ing, f.g_bs = g_bs, f.g_ts = ts;
                    f.y16 = out16, f.y16_slope = last ? 1.f : d->slope, f.force_nr = r.nr;
                    if (last) f.accg = accg, f.scale = scale, f.scale_div = d->scale_div;
                    e = launch_rbpair16(cv[2 * p].pc, cv[2 * p + 1].pc, f, arith, nullptr);
                } else {
                    // conv 1 / conv 2 as engine_vocoder.cpp builds them (mk_pair): conv 1 writes only the 16-bit t, conv 2 the stream and its 16-bit copy
                    Conv16Call c1, c2;
                    c1.x = in16;
                    c1.len_in = c1.len_out = dl.i();
                    c1.batch = B;
                    c1.t_in = c1.t_out = T;
                    c1.dil = d->dil[p];
                    c1.pad_l = (k * d->dil[p] - d->dil[p]) / 2;
                    c1.y16 = r16(dt16);
                    c1.y16_slope = d->slope;
                    c2 = c1;
                    c2.x = c1.y16, c2.dil = 1, c2.pad_l = (k - 1) / 2, c2.g_bs = g_bs, c2.g_ts = ts, c2.resg = ing, c2.yg = outg;
                    c2.y16 = out16, c2.y16_slope = last ? 1.f : d->slope;
                    if (last) c2.accg = accg, c2.scale = scale, c2.scale_div = d->scale_div;
                    e = launch_conv16(cv[2 * p].pc, c1, arith, nullptr);
                    if (e == hipSuccess) e = launch_conv16(cv[2 * p + 1].pc, c2, arith, nullptr);
                }
                ing = outg, in16 = out16;
            }
        }
    }
    if (!finish(e, "vits_op_resblock: " + r.kernel)) return -1;
    return (f32 ? unstage_rows(dout, y, B, C, ts, d->t_stride, T) : unstage_group8(dout, y, B, C, ts, d->t_stride, T)) ? 0 : -1;
    VITS_CATCH(-1)
}

VITS_API int vits_op_conv_transpose1d(const vits_convt1d_desc* d, const float* x, const float* w, const float* bias, const int32_t* lens, float* y) {
    VITS_TRY
    if (!d || !x || !w || !y) return fail("null argument");
    if (d->k != 2 * d->stride) return fail("kernel must be 2*stride");
    const int arith = g_op_arith;
    if (arith == VITS_ARITH_F32_SPLIT) return fail("VITS_ARITH_F32_SPLIT: the transposed conv has no split kernel");
    Conv cv;
    DevMem dx, dy, dl, dlo, x16;
    const size_t nx = (size_t)d->batch * d->cin * d->t_stride * 4, ny = (size_t)d->batch * d->cout * d->t_out_stride * 4;
    std::vector<int32_t> lo;
    if (lens) {
        lo.resize(d->batch);
        for (int b = 0; b < d->batch; ++b) lo[b] = d->stride * lens[b] + d->k - d->stride - 2 * d->crop;
    }
    if (!upload_conv(cv, w, bias, d->cout, d->cout, d->cin, d->k, EPI_CONVT, d->stride, arith)) return -1;
    if (!dx.put(x, nx) || !dy.fill(ny, g_op_out_fill) || !dl.put_opt(lens, (size_t)d->batch * 4) || !dlo.put_opt(lens ? lo.data() : nullptr, (size_t)d->batch * 4)) return -1;
    if (arith != VITS_ARITH_F32 && !x16.fill(group16_bytes(d->batch, d->cin, d->t), 0)) return -1;
    ConvCall c;
    c.x = tref(dx.f(), d->cin, d->t_stride);
    c.y = tref(dy.f(), d->cout, d->t_out_stride);
    c.len_in = dl.i();
    c.len_out = dlo.i();
    c.batch = d->batch;
    c.t_in = d->t;
    c.t_out = d->stride * d->t + d->k - d->stride - 2 * d->crop;
    c.pre_act = d->pre_slope != 1.0f;
    c.slope = d->pre_slope;
    c.ct_crop = d->crop;
    OpKnobs op_knobs;
    OpTileMaps maps;
    if (arith == VITS_ARITH_F32) {  // (the lists are the fp32 kernels')
        if (!maps.add_conv(lens, lens ? lo.data() : nullptr, d->batch, c.t_in, c.t_out, true)) return -1;
        c.maps = &maps.set;
    }
    return finish(conv_transparent(cv.pc, c, arith, x16)) && dy.get(y, ny) ? 0 : -1;
    VITS_CATCH(-1)
}

// ---- vits_op_upsample16: which kernel a descriptor names (host arithmetic only: launch_plan.h, conv_plan.h), then the engine's Conv16Call on staged tensors ----------
namespace {
struct UpOpPlan {
    int variant = 0, bn = 0, t_out = 0;
    std::string kernel;
    char tag[16] = "";
    LaunchGrid g;
};
bool up_fail(std::string& why, const std::string& m) {
    why = "vits_op_upsample16: " + m;
    return false;
}
// (runs under the caller's KernelKnobsScope over the knobs' defaults: no environment variable reaches the choice)
bool upsample16_resolve(const vits_upsample16_desc* d, int arith, UpOpPlan& r, std::string& why) {
    if (arith != VITS_ARITH_F16 && arith != VITS_ARITH_BF16)
        return up_fail(why, "VITS_ARITH_F16 or VITS_ARITH_BF16 only (the fp32 upsampler is vits_op_conv_transpose1d; the split arithmetic has no transposed conv)");
    const int B = d->batch, cin = d->cin, cout = d->cout, T = d->t, s = d->stride;
    if (B < 1 || T < 1 || d->t_stride < T) return up_fail(why, "batch >= 1 and 1 <= t <= t_stride are required");
    if (s < 1) return up_fail(why, "stride = " + std::to_string(s) + ": >= 1 is required (the kernel size is 2 x stride)");
    if (d->crop < 0 || 2 * d->crop > s) return up_fail(why, "crop = " + std::to_string(d->crop) + ": 0 <= 2 crop <= stride is required");
    if (cin < 8 || (cin & 7) || cout < 8 || (cout & 7)) return up_fail(why, "c_in = " + std::to_string(cin) + ", c_out = " + std::to_string(cout) + ": the group layout takes multiples of 8");
    r.t_out = s * T + s - 2 * d->crop;
    if (d->t_out_stride < r.t_out) return up_fail(why, "t_out_stride = " + std::to_string(d->t_out_stride) + " < t_out = " + std::to_string(r.t_out));
    if (d->variant < 0 || d->variant > 2) return up_fail(why, "variant " + std::to_string(d->variant) + ": 0 (the engine's choice), 1 (GEMM tile), 2 (streaming kernel)");
    if (!(d->split == 0 || d->split == 1 || d->split == 2 || d->split == 4)) return up_fail(why, "split = " + std::to_string(d->split) + ": 0 (the planner's), 1, 2 or 4");
    PackedConv pc;  // the shape fields: all the planners read
    pc.cin = cin, pc.cout = cout, pc.kt = 2, pc.epi = EPI_CONVT, pc.ct_stride = s;
    const ConvPackDims pd = conv_pack_dims(cout, cin, 2 * s, EPI_CONVT, s);
    pc.rows = pd.rows, pc.mtiles_used = pd.mtiles_used, pc.mtiles = pd.mtiles, pc.nchunks = pd.nchunks;
    const bool bf = arith == VITS_ARITH_BF16;
    const ConvT16Plan policy = plan_convt16(pc, B, T);
    std::snprintf(r.tag, sizeof(r.tag), "%s", policy.tag);
    const int v = d->variant ? d->variant : policy.supported ? 2 : 1;  // engine_vocoder.cpp: convt16_stream_supported, else conv16
    r.variant = v;
    char name[96];
    if (v == 2) {
        const std::string shape = "c_in = " + std::to_string(cin) + ", c_out = " + std::to_string(cout) + ", stride = " + std::to_string(s);
        if (cin % 64) return up_fail(why, "variant 2: " + shape + ": c_in is not a multiple of 64");
        if (cout % 32) return up_fail(why, "variant 2: " + shape + ": c_out is not a multiple of 32");
        if (cin > 512) return up_fail(why, "variant 2: " + shape + ": c_in > 512 (the input tile of all channels does not fit LDS)");
        if (pc.rows > 128 && s % 4 != 0) return up_fail(why, "variant 2: " + shape + ": rows = stride x c_out = " + std::to_string(pc.rows) + " > 128 and stride is not a multiple of 4");
        const bool lines = policy.lines_bn != 0;
        if (d->split && !lines) return up_fail(why, "split = " + std::to_string(d->split) + ": only convt16_lines_kernel deals its units over gridDim.z, this shape runs on convt16_kernel (" + policy.tag + ")");
        const ConvT16Plan pl = plan_convt16(pc, B, T, d->split);
        if (!pl.supported || !pl.ok) return up_fail(why, "variant 2: plan_convt16 refuses " + shape);
        r.g = pl, r.bn = pl.lines_bn ? pl.lines_bn : convt16_bn(pl.nr, pl.csplit);
        if (lines) std::snprintf(name, sizeof(name), "convt16_lines_kernel<%d, %s>", pl.lines_bn, bf ? "true" : "false");
        else std::snprintf(name, sizeof(name), "convt16_kernel<%d, %d, %d, %s>", pl.nr, pl.csplit, pl.rs, bf ? "true" : "false");
        r.kernel = name;
        return true;
    }
    if (d->split) return up_fail(why, "split = " + std::to_string(d->split) + ": only convt16_lines_kernel deals its units over gridDim.z, variant 1 runs conv16_kernel");
    Conv16Call c;
    c.batch = B, c.t_in = T, c.t_out = r.t_out, c.ct_crop = d->crop;
    c.yg = reinterpret_cast<float*>(sizeof(float));  // (never dereferenced: to plan_conv16 a non-null yg means "group outputs")
    const Conv16Plan pl = plan_conv16(pc, c);
    if (pl.lat || pl.epi16 != C16_CONVT_GROUP || pl.xwp > 384 || pl.dil_ct == kNoKernel || !conv16_tile_exists(pl.epi16, pl.dil_ct, pl.tile))
        return up_fail(why, "variant 1: plan_conv16 has no conv16_kernel for this transposed conv");
    const TileShape ts = tile16_shape(pl.tile);
    r.bn = ts.bn();
    r.g.ok = true, r.g.gx = pl.gx, r.g.gy = pl.gy, r.g.gz = pl.gz, r.g.block = 320, r.g.lds = pl.lds;
    std::snprintf(name, sizeof(name), "conv16_kernel<2, -1, %d, %d, %d, %d, %d, %s>", ts.wm, ts.wn, ts.mr, ts.nr, (int)C16_CONVT_GROUP, bf ? "true" : "false");
    r.kernel = name;
    return true;
}
}  // namespace

VITS_API int vits_op_upsample16_plan(const vits_upsample16_desc* d, vits_upsample16_plan* out) {
    VITS_TRY
    if (!d || !out) return fail("vits_op_upsample16_plan: null argument");
    const KernelKnobs defaults;
    KernelKnobsScope scope(&defaults);
    UpOpPlan r;
    std::string why;
    if (!upsample16_resolve(d, g_op_arith, r, why)) return fail(why);
    std::memset(out, 0, sizeof(*out));
    std::snprintf(out->kernel, sizeof(out->kernel), "%s", r.kernel.c_str());
    std::snprintf(out->tag, sizeof(out->tag), "%s", r.tag);
    out->variant = r.variant, out->bn = r.bn;
    out->grid_x = r.g.gx, out->grid_y = r.g.gy, out->grid_z = r.g.gz, out->block = r.g.block, out->lds = (int64_t)r.g.lds;
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_op_upsample16(const vits_upsample16_desc* d, const float* x, const float* w, const float* bias, const int32_t* lens, float* y, uint16_t* y16,
                                uint16_t* x16) {
    VITS_TRY
    if (!d || !x || !w || !y) return fail("vits_op_upsample16: null argument (x, w and y are required)");
    const KernelKnobs defaults;
    KernelKnobsScope scope(&defaults);
    const int arith = g_op_arith;
    UpOpPlan r;
    std::string why;
    if (!upsample16_resolve(d, arith, r, why)) return fail(why);
    const int B = d->batch, cin = d->cin, cout = d->cout, T = d->t, s = d->stride, t_out = r.t_out;
    if (!lens_ok(lens, B, T)) return fail("vits_op_upsample16: 0 <= lens[b] <= t is required");
    Conv cv;
    if (!upload_conv(cv, w, bias, cout, cout, cin, 2 * s, EPI_CONVT, s, arith)) return -1;
    // staging, as engine_vocoder.cpp hands a stage to its upsampler
    const int x_ts = round_up(T, 32), g_ts = round_up(t_out, 32);
    const size_t nx = (size_t)B * cin * d->t_stride, nx16 = (size_t)B * cin * x_ts, ng = (size_t)B * cout * g_ts;
    std::vector<int32_t> lo;
    if (lens) {
        lo.resize(B);
        for (int b = 0; b < B; ++b) lo[b] = s * lens[b] + s - 2 * d->crop;
    }
    DevMem dl, dlo, dx, dx16, dyg, dy16;
    if (!dl.put_opt(lens, (size_t)B * 4) || !dlo.put_opt(lens ? lo.data() : nullptr, (size_t)B * 4) || !dx.put(x, nx * 4) || !dx16.fill(nx16 * 2, 0xFF) || !dyg.fill(ng * 4, 0) ||
        (y16 && !dy16.fill(ng * 2, 0)))
        return -1;
    Conv16Call cu;
    cu.x.p = dx16.h(), cu.x.ts = x_ts, cu.x.bs = (int64_t)cin * x_ts;
    cu.len_in = dl.i();
    cu.len_out = dlo.i();
    cu.batch = B;
    cu.t_in = T;
    cu.t_out = t_out;
    cu.ct_crop = d->crop;
    cu.yg = dyg.f();
    cu.g_bs = (int64_t)cout * g_ts;
    cu.g_ts = g_ts;
    if (y16) {
        cu.y16.p = dy16.h(), cu.y16.ts = g_ts, cu.y16.bs = (int64_t)cout * g_ts;
        cu.y16_slope = d->y16_slope;
    }
    cu.force_split = d->split;
    hipError_t e = launch_to_group16(tref(dx.f(), cin, d->t_stride), dl.i(), B, cin, T, d->pre_slope, cu.x, arith, nullptr);
    if (e == hipSuccess) e = r.variant == 2 ? launch_convt16_stream(cv.pc, cu, arith, nullptr) : launch_conv16(cv.pc, cu, arith, nullptr);
    if (!finish(e, "vits_op_upsample16: " + r.kernel)) return -1;
    // group layout [b][c / 8][ts][8] -> [b][c][stride]
    if (!unstage_group8(dyg, y, B, cout, g_ts, d->t_out_stride, t_out)) return -1;
    if (y16 && !unstage_group8(dy16, y16, B, cout, g_ts, d->t_out_stride, t_out)) return -1;
    if (x16 && !unstage_group8(dx16, x16, B, cin, x_ts, d->t_stride, T)) return -1;
    return 0;
    VITS_CATCH(-1)
}
