// abi_ops_stage1.cpp — operator-level entry points of the flow, the text encoder, the duration predictors and the alignment: host arrays in, host arrays out, the
// engine's own launchers between (staging: abi_ops_common.h). vits_op_flow_coupling, vits_op_rel_attention, vits_op_add_layer_norm, vits_op_attention,
// vits_op_layer_norm, vits_op_norm_conv, vits_op_duration_predictor, vits_op_dds_block, vits_op_spline, vits_op_durations, vits_op_align, and the _plan queries.
#include <cstdio>
#include <limits>

#include "abi_ops_common.h"

using namespace vits;

// ---- vits_op_flow_coupling: which kernel a descriptor names (host arithmetic only: launch_plan.h), then the engine's call structs on staged tensors ---------
namespace {
struct FlowOpPlan {
    int variant = 0;
    std::string kernel;
    int bo = 0, halo = 0, ncw = 0, nct = 0, launches = 0;
    LaunchGrid g;
};
bool fc_fail(std::string& why, const std::string& m) {
    why = "vits_op_flow_coupling: " + m;
    return false;
}
bool flow_resolve(const vits_flow_coupling_desc* d, int arith, FlowOpPlan& r, std::string& why) {
    if (arith != VITS_ARITH_F32 && arith != VITS_ARITH_F16 && arith != VITS_ARITH_BF16)
        return fc_fail(why, "VITS_ARITH_F32, VITS_ARITH_F16 or VITS_ARITH_BF16 only (the split arithmetic has no flow kernels)");
    const int H = d->hidden, HF = d->half, k = d->k, B = d->batch, T = d->t, NL = d->layers;
    if (B < 1 || T < 1 || d->t_stride < T) return fc_fail(why, "batch >= 1 and 1 <= t <= t_stride are required");
    if (H < 32 || (H & 31)) return fc_fail(why, "hidden = " + std::to_string(H) + ": a multiple of 32 is required");
    if (HF < 32 || (HF & 31)) return fc_fail(why, "half = " + std::to_string(HF) + ": a multiple of 32 is required");
    if (k < 1 || !(k & 1)) return fc_fail(why, "k = " + std::to_string(k) + ": an odd tap count is required");
    if (NL < 1 || NL > 16) return fc_fail(why, "layers = " + std::to_string(NL) + ": 1 to 16 WaveNet layers");
    if (d->rate < 1 || (d->rate > 1 && NL > 8)) return fc_fail(why, "rate = " + std::to_string(d->rate) + ": >= 1 is required (and at most 8 layers of a dilated stack)");
    if (d->flipped != 0 && d->flipped != 1) return fc_fail(why, "flipped = " + std::to_string(d->flipped) + ": 0 (x0 first) or 1 (x1 first)");
    if (d->n_bias_rows < 1) return fc_fail(why, "n_bias_rows = " + std::to_string(d->n_bias_rows) + ": the b_in table has at least one row");
    if (d->variant < 0 || d->variant > 3) return fc_fail(why, "variant " + std::to_string(d->variant) + ": 0 (the engine's choice), 1 (un-fused), 2 (fused WaveNet layers), 3 (the coupling kernel)");
    if (d->ncw < 0 || d->nct < 0) return fc_fail(why, "(ncw, nct) = (" + std::to_string(d->ncw) + ", " + std::to_string(d->nct) + "): negative");
    const bool f32 = arith == VITS_ARITH_F32, bf = arith == VITS_ARITH_BF16;
    const std::string tile = "(ncw, nct) = (" + std::to_string(d->ncw) + ", " + std::to_string(d->nct) + ")";
    char name[96];
    int v = d->variant;
    if (v == 0) {  // engine_flow.cpp's order: the coupling kernel (16-bit modes), the fused WaveNet layers on large grids, nine launches
        if (d->ncw || d->nct) return fc_fail(why, tile + ": variant 0 takes the planner's tile");
        const bool wn = f32 ? plan_wavenet32(H, k, d->rate, B, T).ok : plan_wavenet16(H, k, d->rate, B, T).ok;
        v = !f32 && plan_flow_couple16(H, HF, k, d->rate, NL, B, T).ok ? 3 : wn && (int64_t)blocks_for(T, 32) * B >= 384 ? 2 : 1;
    }
    r.variant = v;
    if (v == 1) {
        if (d->ncw || d->nct) return fc_fail(why, tile + ": variant 1 has no tile to choose");
        r.kernel = f32 ? "launch_conv" : "launch_conv16";
        r.launches = 2 * NL + 2;
        return true;
    }
    if (v == 2) {
        const char* fam = f32 ? "wavenet32_kernel" : "wavenet16_kernel";
        if (H != 192) return fc_fail(why, std::string("variant 2: no ") + fam + " for hidden = " + std::to_string(H) + " (hidden = 192, k = 5, rate = 1)");
        if (k != 5) return fc_fail(why, std::string("variant 2: no ") + fam + " for k = " + std::to_string(k) + " (hidden = 192, k = 5, rate = 1)");
        if (d->rate != 1) return fc_fail(why, std::string("variant 2: no ") + fam + " for rate = " + std::to_string(d->rate) + " (hidden = 192, k = 5, rate = 1)");
        if (d->nct) return fc_fail(why, tile + ": variant 2 has no nct (a block is two column tiles)");
        if (f32 && d->ncw) return fc_fail(why, tile + ": wavenet32_kernel has one form (ncw = 0)");
        const WaveNetPlan pl = f32 ? plan_wavenet32(H, k, 1, B, T) : plan_wavenet16(H, k, 1, B, T, d->ncw);
        if (!pl.ok) return fc_fail(why, tile + ": no such wavenet16_kernel (ncw = 1 or 2)");
        r.g = pl, r.ncw = pl.ncw, r.bo = kWaveNetBM, r.halo = (k - 1) / 2, r.launches = NL + 2;
        if (f32) std::snprintf(name, sizeof(name), "wavenet32_kernel<%d, %d>", H, k);
        else std::snprintf(name, sizeof(name), "wavenet16_kernel<%d, %d, %s, %d>", H, k, bf ? "true" : "false", pl.ncw);
        r.kernel = name;
        return true;
    }
    if (f32) return fc_fail(why, "variant 3: flow_couple16_kernel exists in the 16-bit modes only");
    const char* only = " (hidden = 192, half = 96, k = 5, rate = 1, layers = 4)";
    if (H != 192) return fc_fail(why, "variant 3: no flow_couple16_kernel for hidden = " + std::to_string(H) + only);
    if (HF != 96) return fc_fail(why, "variant 3: no flow_couple16_kernel for half = " + std::to_string(HF) + only);
    if (k != 5) return fc_fail(why, "variant 3: no flow_couple16_kernel for k = " + std::to_string(k) + only);
    if (d->rate != 1) return fc_fail(why, "variant 3: no flow_couple16_kernel for rate = " + std::to_string(d->rate) + only);
    if (NL != 4) return fc_fail(why, "variant 3: no flow_couple16_kernel for layers = " + std::to_string(NL) + only);
    const FlowCouple16Plan pl = plan_flow_couple16(H, HF, k, 1, NL, B, T, d->ncw, d->nct);
    if (!pl.ok) return fc_fail(why, tile + ": no such flow_couple16_kernel ((1, 1), (1, 2) or (2, 2))");
    const FlowCouple16Geom ge = flow_couple16_geom(pl.ncw, pl.nct);
    r.g = pl, r.ncw = pl.ncw, r.nct = pl.nct, r.bo = ge.bo, r.halo = ge.halo, r.launches = 1;
    std::snprintf(name, sizeof(name), "flow_couple16_kernel<%s, %d, %d>", bf ? "true" : "false", pl.ncw, pl.nct);
    r.kernel = name;
    return true;
}
}  // namespace

VITS_API int vits_op_flow_coupling_plan(const vits_flow_coupling_desc* d, vits_flow_coupling_plan* out) {
    VITS_TRY
    if (!d || !out) return fail("vits_op_flow_coupling_plan: null argument");
    FlowOpPlan r;
    std::string why;
    if (!flow_resolve(d, g_op_arith, r, why)) return fail(why);
    std::memset(out, 0, sizeof(*out));
    std::snprintf(out->kernel, sizeof(out->kernel), "%s", r.kernel.c_str());
    out->variant = r.variant, out->bo = r.bo, out->halo = r.halo, out->ncw = r.ncw, out->nct = r.nct;
    out->grid_x = r.g.gx, out->grid_y = r.g.gy, out->grid_z = r.g.ok ? r.g.gz : 0, out->block = r.g.block, out->lds = (int64_t)r.g.lds, out->launches = r.launches;
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_op_flow_coupling(const vits_flow_coupling_desc* d, float* z, const float* w_pre, const float* b_pre, const float* w_in, const float* b_in,
                                   const float* w_rs, const float* b_rs, const float* w_post, const float* b_post, const int32_t* bias_rows, const int32_t* lens) {
    VITS_TRY
    if (!d || !z || !w_pre || !b_pre || !w_in || !b_in || !w_rs || !b_rs || !w_post || !b_post)
        return fail("vits_op_flow_coupling: null argument (z and every weight and bias are required)");
    const int arith = g_op_arith;
    FlowOpPlan r;
    std::string why;
    if (!flow_resolve(d, arith, r, why)) return fail(why);
    const int B = d->batch, H = d->hidden, HF = d->half, T = d->t, k = d->k, NL = d->layers, ts = round_up(T, 32);
    for (int b = 0; b < B; ++b) {
        if (lens && (lens[b] < 0 || lens[b] > T)) return fail("vits_op_flow_coupling: 0 <= lens[b] <= t is required");
        if (bias_rows && (bias_rows[b] < 0 || bias_rows[b] >= d->n_bias_rows)) return fail("vits_op_flow_coupling: 0 <= bias_rows[b] < n_bias_rows is required");
    }
    // the convs on the device: pre, in[l], rs[l], post
    std::vector<Conv> cv(2 * NL + 2);
    DevMem dtab;  // the b_in table [n_bias_rows][layers][2H]: in[l] points at its segment of row 0, one row stride for all (engine_load.cpp load_speakers)
    if (!dtab.put(b_in, (size_t)d->n_bias_rows * NL * 2 * H * 4)) return -1;
    Conv &pre = cv[0], &post = cv[2 * NL + 1];
    if (!upload_conv(pre, w_pre, b_pre, H, H, HF, 1, EPI_STD, 0, arith) || !upload_conv(post, w_post, b_post, HF, HF, H, 1, EPI_STD, 0, arith)) return -1;
    std::vector<PackedConv> in(NL), rs(NL);
    for (int l = 0; l < NL; ++l) {
        const int rows = l + 1 < NL ? 2 * H : H;
        if (!upload_conv(cv[1 + 2 * l], w_in + (size_t)l * 2 * H * H * k, nullptr, 0, 2 * H, H, k, EPI_GATE, 0, arith) ||
            !upload_conv(cv[2 + 2 * l], w_rs + (size_t)l * 2 * H * H, b_rs + (size_t)l * 2 * H, rows, rows, H, 1, EPI_STD, 0, arith))
            return -1;
        in[l] = cv[1 + 2 * l].pc, rs[l] = cv[2 + 2 * l].pc;
        in[l].bias = dtab.f() + (size_t)l * 2 * H;
        in[l].bias_rs = bias_rows ? (int64_t)NL * 2 * H : 0;
    }
    DevMem dl, dspk, dz, dhout, dgate, dx16;
    if (!dl.put_opt(lens, (size_t)B * 4) || !dspk.put_opt(bias_rows, (size_t)B * 4) || !stage_rows(dz, z, B, 2 * HF, d->t_stride, ts, lens, T)) return -1;
    const TensorRef zr = tref(dz.f(), 2 * HF, ts);
    TensorRef x0 = zr, x1 = zr;
    (d->flipped ? x0 : x1).p += (size_t)HF * ts;
    hipError_t e = hipSuccess;
    if (r.variant == 3) {
        FlowCouple16Call fc;
        fc.x0 = x0, fc.x1 = x1, fc.lens = dl.i(), fc.spk = dspk.i(), fc.batch = B, fc.tmax = T, fc.hidden = H, fc.half = HF;
        fc.force_ncw = r.ncw, fc.force_nct = r.nct;
        e = launch_flow_couple16(pre.pc, in.data(), rs.data(), post.pc, fc, arith, nullptr);
    } else {
        // hout: h = rows [0, H), the skip sum `outputs` = rows [H, 2H), zero on the valid columns (launch_fill_rows of the engine); gate: the gated conv's
        // output, and the other h buffer of the fused layers
        {
            std::vector<float> hh((size_t)B * 2 * H * ts, std::numeric_limits<float>::quiet_NaN());
            for (int b = 0; b < B; ++b)
                for (int c = H; c < 2 * H; ++c) std::fill_n(&hh[((size_t)b * 2 * H + c) * ts], lens ? lens[b] : T, 0.f);
            if (!dhout.put(hh.data(), hh.size() * 4) || !dgate.fill((size_t)B * H * ts * 4, 0xFF)) return -1;
        }
        const size_t x16_bytes = arith == VITS_ARITH_F32 ? 0 : group16_bytes(B, std::max(H, HF), T);
        if (x16_bytes && !dx16.fill(x16_bytes, 0xFF)) return -1;
        auto mk = [&](TensorRef xin, TensorRef yout) {
            ConvCall c;
            c.x = xin, c.y = yout, c.len_in = c.len_out = dl.i(), c.spk = dspk.i(), c.batch = B, c.t_in = c.t_out = T;
            return c;
        };
        const TensorRef hout = tref(dhout.f(), 2 * H, ts), gate = tref(dgate.f(), H, ts);
        TensorRef outputs = hout;
        outputs.p += (size_t)H * ts;
        e = conv_transparent(pre.pc, mk(x0, hout), arith, dx16, x16_bytes);
        TensorRef hcur = hout;
        for (int l = 0, dil = 1; l < NL && e == hipSuccess; ++l, dil *= d->rate) {
            const bool last = l + 1 == NL;
            if (r.variant == 2) {
                WaveNet32Call w;
                w.h = hcur, w.h_out = last ? TensorRef() : (hcur.p == gate.p ? hout : gate), w.outputs = outputs;
                w.lens = dl.i(), w.spk = dspk.i(), w.batch = B, w.tmax = T, w.hidden = H, w.dil = dil, w.force_ncw = r.ncw;
                e = arith == VITS_ARITH_F32 ? launch_wavenet32(in[l], rs[l], w, nullptr) : launch_wavenet16(in[l], rs[l], w, arith, nullptr);
                if (w.h_out.p) hcur = w.h_out;
                continue;
            }
            ConvCall g = mk(hout, gate);
            g.dil = dil, g.pad_l = (k * dil - dil) / 2;
            e = conv_transparent(in[l], g, arith, dx16, x16_bytes);
            ConvCall q = mk(gate, last ? outputs : hout);
            q.res = q.y;
            if (e == hipSuccess) e = conv_transparent(rs[l], q, arith, dx16, x16_bytes);
        }
        if (e == hipSuccess) {
            ConvCall pc = mk(outputs, x1);
            pc.res = x1;
            e = conv_transparent(post.pc, pc, arith, dx16, x16_bytes);
        }
    }
    if (!finish(e, "vits_op_flow_coupling: " + r.kernel)) return -1;
    return unstage_rows(dz, z, B, 2 * HF, ts, d->t_stride, T) ? 0 : -1;
    VITS_CATCH(-1)
}

VITS_API int vits_op_rel_attention(int32_t batch, int32_t heads, int32_t head_dim, int32_t t, int32_t t_stride, int32_t window, const float* q, const float* k,
                                   const float* v, const float* rel_k, const float* rel_v, const int32_t* lens, float* out) {
    VITS_TRY
    const int C = heads * head_dim;
    const size_t n = (size_t)batch * C * t_stride * 4, nr = (size_t)(2 * window + 1) * head_dim * 4;
    DevMem dq, dk, dv, drk, drv, dout, dl;
    if (!dq.put(q, n) || !dk.put(k, n) || !dv.put(v, n) || !drk.put(rel_k, nr) || !drv.put(rel_v, nr) || !dout.fill(n, 0) || !dl.put_opt(lens, (size_t)batch * 4)) return -1;
    const hipError_t e = launch_rel_attention(tref(dq.f(), C, t_stride), tref(dk.f(), C, t_stride), tref(dv.f(), C, t_stride), drk.f(), drv.f(), tref(dout.f(), C, t_stride),
                                              dl.i(), batch, heads, head_dim, t, window, 1.0f, nullptr);
    return finish(e) && dout.get(out, n) ? 0 : -1;
    VITS_CATCH(-1)
}

VITS_API int vits_op_add_layer_norm(int32_t batch, int32_t channels, int32_t t, int32_t t_stride, float eps, const float* x, const float* residual,
                                    const float* gamma, const float* beta, float* y) {
    VITS_TRY
    const size_t n = (size_t)batch * channels * t_stride * 4;
    DevMem dx, dr, dg, db, dy;
    if (!dx.put(x, n) || !dg.put(gamma, (size_t)channels * 4) || !db.put(beta, (size_t)channels * 4) || !dy.fill(n, 0) || (residual && !dr.put(residual, n))) return -1;
    TensorRef none;
    const hipError_t e = launch_add_layer_norm(tref(dx.f(), channels, t_stride), residual ? tref(dr.f(), channels, t_stride) : none, dg.f(), db.f(),
                                               tref(dy.f(), channels, t_stride), nullptr, batch, channels, t, eps, 0, none, nullptr);
    return finish(e) && dy.get(y, n) ? 0 : -1;
    VITS_CATCH(-1)
}

// ---- vits_op_attention / vits_op_layer_norm / vits_op_norm_conv: which kernel a descriptor names (host arithmetic only: launch_plan.h, conv_plan.h), then the text
// encoder's launches on staged tensors. (The resolvers run under the caller's KernelKnobsScope over the knobs' defaults: no environment variable reaches the choice)
namespace {
bool op_fail(std::string& why, const char* op, const std::string& m) {
    why = std::string(op) + ": " + m;
    return false;
}
const char* tf(bool v) { return v ? "true" : "false"; }

struct AttOpPlan {
    int variant = 0;
    std::string kernel;
    AttentionPlan p;
};
bool attention_resolve(const vits_attention_desc* d, AttOpPlan& r, std::string& why) {
    const char* op = "vits_op_attention";
    const int hd = d->head_dim, v = d->variant;
    if (d->batch < 1 || d->heads < 1 || d->t < 1 || d->t_stride < d->t) return op_fail(why, op, "batch >= 1, heads >= 1 and 1 <= t <= t_stride are required");
    if (d->window < 0) return op_fail(why, op, "window = " + std::to_string(d->window) + ": at least 0");
    if (v < 0 || v > 6)
        return op_fail(why, op, "variant " + std::to_string(v) + ": 0 (the planner's choice), 1 / 2 (rel_attention_kernel<1024> / <256>), 3 ... 6 (rel_attention_mfma_kernel<4, 32, false, false>, <8, 32, false, false>, <4, 24, true, false>, <8, 24, false, true>)");
    if (hd < 1 || hd > 128) return op_fail(why, op, "head_dim = " + std::to_string(hd) + ": no attention kernel above 128 (1 to 128)");
    if (v >= 3 && (hd & 15)) return op_fail(why, op, "variant " + std::to_string(v) + ": head_dim = " + std::to_string(hd) + " is not a multiple of 16 (the matrix-core kernel's d tiles)");
    if (v >= 5 && hd > 96) return op_fail(why, op, "variant " + std::to_string(v) + ": head_dim = " + std::to_string(hd) + " is above 96 (the register arrays of the 24-step kernels)");
    if (v >= 3 && att_mfma_lds(hd, d->t, d->window) > kLdsMax)
        return op_fail(why, op, "variant " + std::to_string(v) + ": rel_attention_mfma_kernel needs " + std::to_string(att_mfma_lds(hd, d->t, d->window)) + " bytes of LDS, the limit is " + std::to_string(kLdsMax));
    if ((v == 1 || v == 2) && att_valu_lds(hd, d->t, d->window, 3) > kLdsSoft)
        return op_fail(why, op, "variant " + std::to_string(v) + ": rel_attention_kernel needs " + std::to_string(att_valu_lds(hd, d->t, d->window, 3)) + " bytes of LDS, the limit is " + std::to_string(kLdsSoft));
    r.p = plan_rel_attention(d->batch, d->heads, hd, d->t, d->window, v);
    if (!r.p.ok) return op_fail(why, op, v ? "variant " + std::to_string(v) + ": plan_rel_attention refuses the shape" : "no attention kernel takes this shape (the scores of one block pass the LDS limit)");
    char name[96];
    if (r.p.mfma) {
        r.variant = r.p.lat ? 6 : r.p.sh ? 5 : r.p.nw == 8 ? 4 : 3;
        std::snprintf(name, sizeof(name), "rel_attention_mfma_kernel<%d, %d, %s, %s>", r.p.nw, r.p.maxs, tf(r.p.sh), tf(r.p.lat));
    } else {
        r.variant = r.p.block == 1024 ? 1 : 2;
        std::snprintf(name, sizeof(name), "rel_attention_kernel<%d>", r.p.block);
    }
    r.kernel = name;
    return true;
}

bool layer_norm_resolve(const vits_layer_norm_desc* d, bool has_tab, LayerNormPlan& p, std::string& why) {
    const char* op = "vits_op_layer_norm";
    if (d->batch < 1 || d->channels < 1 || d->t < 1 || d->t_stride < d->t) return op_fail(why, op, "batch >= 1, channels >= 1 and 1 <= t <= t_stride are required");
    if (!(d->eps > 0.f)) return op_fail(why, op, "eps must be positive");
    if (d->tw != 0 && d->tw != 32 && d->tw != 64) return op_fail(why, op, "tw = " + std::to_string(d->tw) + ": 0 (the planner's choice), 32 or 64 time steps per block");
    if ((d->post_gelu != 0 && d->post_gelu != 1) || (d->add_to != 0 && d->add_to != 1)) return op_fail(why, op, "post_gelu and add_to are 0 or 1");
    if (has_tab && !d->post_gelu) return op_fail(why, op, "gelu_tab without post_gelu: the table is the GELU's");
    p = plan_add_layer_norm(d->channels, d->batch, d->t, d->tw);
    if (!p.ok) {
        const int tw = d->tw ? d->tw : 32;
        return op_fail(why, op, "add_layer_norm_kernel<" + std::to_string(tw) + "> needs " + std::to_string(layer_norm_lds(d->channels, tw)) + " bytes of LDS for channels = " +
                                    std::to_string(d->channels) + ", the limit is " + std::to_string(kLdsSoft));
    }
    return true;
}

struct NormConvOpPlan {
    int variant = 0, pitch = 0, launches = 0;
    bool ln_ok = false;
    std::string ln_why;
    ConvPlan cp;  // of the conv that runs
};
const char* conv_tile_name(int tile) {
    static const char* const names[] = {"TILE_128x128", "TILE_64x256", "TILE_32x256", "TILE_64x64", "TILE_32x64", "TILE_NARROW", "TILE_LAT16"};
    return tile >= 0 && tile <= 6 ? names[tile] : "?";
}
// the two calls of the op for the planner: `fused` with LayerNorm on load, `plain` on the normalised tensor (pointers: only whether they are set and equal matters)
void norm_conv_calls(const vits_norm_conv_desc* d, const int* lens, ConvCall& plain, ConvCall& fused) {
    plain.len_in = plain.len_out = lens;
    plain.batch = d->batch, plain.t_in = plain.t_out = d->t;
    plain.pad_l = d->pad_left, plain.post_act = d->post_act;
    fused = plain;
    fused.ln_gamma = fused.ln_beta = reinterpret_cast<const float*>(sizeof(float));  // (the op replaces them; to plan_conv non-null means "with the statistics' LDS")
    fused.ln_eps = d->eps;
}
bool norm_conv_resolve(const vits_norm_conv_desc* d, int arith, NormConvOpPlan& r, std::string& why) {
    const char* op = "vits_op_norm_conv";
    if (arith != VITS_ARITH_F32) return op_fail(why, op, "VITS_ARITH_F32 only (the engine normalises on load in fp32 alone)");
    if (d->batch < 1 || d->cin < 1 || d->cout < 1 || d->t < 1 || d->t_stride < d->t) return op_fail(why, op, "batch, cin, cout >= 1 and 1 <= t <= t_stride are required");
    r.pitch = d->pitch ? d->pitch : round_up(d->t, 32);
    if (r.pitch < d->t) return op_fail(why, op, "pitch = " + std::to_string(d->pitch) + " < t = " + std::to_string(d->t));
    if (d->k < 1 || d->k > 64) return op_fail(why, op, "k = " + std::to_string(d->k) + ": 1 to 64 taps");
    if (d->pad_left < 0 || d->pad_left > d->k - 1) return op_fail(why, op, "pad_left = " + std::to_string(d->pad_left) + ": 0 to k - 1 (every output reads its own column)");
    if (d->post_act != 0 && d->post_act != 1) return op_fail(why, op, "post_act " + std::to_string(d->post_act) + ": 0 (none) or 1 (relu)");
    if (!(d->eps > 0.f)) return op_fail(why, op, "eps must be positive");
    if (d->variant < 0 || d->variant > 2) return op_fail(why, op, "variant " + std::to_string(d->variant) + ": 0 (the engine's choice), 1 (LayerNorm launch + conv), 2 (LayerNorm on load)");
    PackedConv pc;  // the shape fields: all the planner reads, beside whether the layer has its second copy (upload_conv's rule)
    pc.cin = d->cin, pc.cout = d->cout, pc.kt = d->k, pc.epi = EPI_STD;
    const ConvPackDims pd = conv_pack_dims(d->cout, d->cin, d->k, EPI_STD, 0);
    pc.rows = pd.rows, pc.mtiles_used = pd.mtiles_used, pc.mtiles = pd.mtiles, pc.nchunks = pd.nchunks;
    if (conv_lat16_candidate(EPI_STD, d->k, d->cin)) pc.wp_l16 = reinterpret_cast<float*>(sizeof(float));  // (never dereferenced)
    ConvCall plain, fused;
    norm_conv_calls(d, nullptr, plain, fused);
    const ConvPlan pf = plan_conv(pc, fused), pp = plan_conv(pc, plain);
    r.ln_ok = pf.ln_ok, r.ln_why = pf.ln_why ? pf.ln_why : "";
    r.variant = d->variant ? d->variant : pf.ln_ok ? 2 : 1;  // Engine::run_text_encoder's conv_of_norm
    if (r.variant == 2 && !pf.ln_ok) return op_fail(why, op, "variant 2: conv_ln_on_load_ok refuses: " + r.ln_why);
    r.cp = r.variant == 2 ? pf : pp;
    if (!r.cp.ok) return op_fail(why, op, "variant " + std::to_string(r.variant) + ": plan_conv has no kernel for this conv");
    if (r.variant == 1 && !plan_add_layer_norm(d->cin, d->batch, d->t).ok) return op_fail(why, op, "variant 1: add_layer_norm_kernel has no tile for channels = " + std::to_string(d->cin));
    r.launches = r.variant == 2 ? 1 : 2;
    return true;
}
}  // namespace

VITS_API int vits_op_attention_plan(const vits_attention_desc* d, vits_attention_plan* out) {
    VITS_TRY
    if (!d || !out) return fail("vits_op_attention_plan: null argument");
    const KernelKnobs defaults;
    KernelKnobsScope scope(&defaults);
    AttOpPlan r;
    std::string why;
    if (!attention_resolve(d, r, why)) return fail(why);
    std::memset(out, 0, sizeof(*out));
    std::snprintf(out->kernel, sizeof(out->kernel), "%s", r.kernel.c_str());
    out->variant = r.variant, out->nw = r.p.nw, out->maxs = r.p.maxs, out->vshift = r.p.mfma ? 0 : r.p.vshift;
    out->grid_x = r.p.gx, out->grid_y = r.p.gy, out->grid_z = r.p.gz, out->block = r.p.block, out->lds = (int64_t)r.p.lds;
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_op_attention(const vits_attention_desc* d, const float* q, const float* k, const float* v, const float* rel_k, const float* rel_v,
                               const uint16_t* exp_tab, const int32_t* lens, float* out) {
    VITS_TRY
    if (!d || !q || !k || !v || !rel_k || !rel_v || !out) return fail("vits_op_attention: null argument");
    const KernelKnobs defaults;
    KernelKnobsScope scope(&defaults);
    AttOpPlan r;
    std::string why;
    if (!attention_resolve(d, r, why)) return fail(why);
    const int B = d->batch, C = d->heads * d->head_dim, T = d->t, ts = d->t_stride;
    if (!lens_ok(lens, B, T)) return fail("vits_op_attention: 0 <= lens[b] <= t <= t_stride is required");
    const size_t nr = (size_t)(2 * d->window + 1) * d->head_dim * 4;
    DevMem dq, dk, dv, dout, drk, drv, dtab, dl;
    if (!stage_rows(dq, q, B, C, ts, ts, lens, T) || !stage_rows(dk, k, B, C, ts, ts, lens, T) || !stage_rows(dv, v, B, C, ts, ts, lens, T) ||
        !dout.fill((size_t)B * C * ts * 4, 0xFF) || !drk.put(rel_k, nr) || !drv.put(rel_v, nr) || !dl.put_opt(lens, (size_t)B * 4) || (exp_tab && !dtab.put(exp_tab, 65536 * 2)))
        return -1;
    GgmlTables tabs;
    tabs.exp = exp_tab ? dtab.h() : nullptr;
    const hipError_t e = launch_rel_attention(tref(dq.f(), C, ts), tref(dk.f(), C, ts), tref(dv.f(), C, ts), drk.f(), drv.f(), tref(dout.f(), C, ts), dl.i(), B, d->heads,
                                              d->head_dim, T, d->window, d->q_scale, nullptr, tabs, r.variant);
    return finish(e, "vits_op_attention: " + r.kernel) && dout.get(out, (size_t)B * C * ts * 4) ? 0 : -1;
    VITS_CATCH(-1)
}

VITS_API int vits_op_layer_norm_plan(const vits_layer_norm_desc* d, vits_layer_norm_plan* out) {
    VITS_TRY
    if (!d || !out) return fail("vits_op_layer_norm_plan: null argument");
    const KernelKnobs defaults;
    KernelKnobsScope scope(&defaults);
    LayerNormPlan p;
    std::string why;
    if (!layer_norm_resolve(d, false, p, why)) return fail(why);
    std::memset(out, 0, sizeof(*out));
    std::snprintf(out->kernel, sizeof(out->kernel), "add_layer_norm_kernel<%d>", p.tw);
    out->tw = p.tw, out->grid_x = p.gx, out->grid_y = p.gy, out->block = p.block, out->lds = (int64_t)p.lds;
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_op_layer_norm(const vits_layer_norm_desc* d, const float* x, const float* residual, const float* gamma, const float* beta, const uint16_t* gelu_tab,
                                const int32_t* lens, float* y) {
    VITS_TRY
    if (!d || !x || !gamma || !beta || !y) return fail("vits_op_layer_norm: null argument");
    const KernelKnobs defaults;
    KernelKnobsScope scope(&defaults);
    LayerNormPlan p;
    std::string why;
    if (!layer_norm_resolve(d, gelu_tab != nullptr, p, why)) return fail(why);
    const int B = d->batch, C = d->channels, T = d->t, ts = d->t_stride;
    if (!lens_ok(lens, B, T)) return fail("vits_op_layer_norm: 0 <= lens[b] <= t <= t_stride is required");
    DevMem dx, dr, dy, dg, db, dtab, dl;
    if (!stage_rows(dx, x, B, C, ts, ts, lens, T) || (residual && !stage_rows(dr, residual, B, C, ts, ts, lens, T)) || !stage_rows(dy, d->add_to ? y : nullptr, B, C, ts, ts, lens, T) ||
        !dg.put(gamma, (size_t)C * 4) || !db.put(beta, (size_t)C * 4) || !dl.put_opt(lens, (size_t)B * 4) || (gelu_tab && !dtab.put(gelu_tab, 65536 * 2)))
        return -1;
    GgmlTables tabs;
    tabs.gelu = gelu_tab ? dtab.h() : nullptr;
    TensorRef none;
    const TensorRef yr = tref(dy.f(), C, ts);
    const hipError_t e = launch_add_layer_norm(tref(dx.f(), C, ts), residual ? tref(dr.f(), C, ts) : none, dg.f(), db.f(), d->add_to ? none : yr, dl.i(), B, C, T, d->eps,
                                               d->post_gelu, d->add_to ? yr : none, nullptr, tabs, p.tw);
    return finish(e, "vits_op_layer_norm") && dy.get(y, (size_t)B * C * ts * 4) ? 0 : -1;
    VITS_CATCH(-1)
}

VITS_API int vits_op_norm_conv_plan(const vits_norm_conv_desc* d, vits_norm_conv_plan* out) {
    VITS_TRY
    if (!d || !out) return fail("vits_op_norm_conv_plan: null argument");
    const KernelKnobs defaults;
    KernelKnobsScope scope(&defaults);
    NormConvOpPlan r;
    std::string why;
    if (!norm_conv_resolve(d, g_op_arith, r, why)) return fail(why);
    std::memset(out, 0, sizeof(*out));
    std::snprintf(out->tile, sizeof(out->tile), "%s", conv_tile_name(r.cp.tile));
    std::snprintf(out->ln_why, sizeof(out->ln_why), "%s", r.ln_why.c_str());
    out->variant = r.variant, out->pitch = r.pitch, out->ln_ok = r.ln_ok ? 1 : 0, out->launches = r.launches;
    out->grid_x = r.cp.gx, out->grid_y = r.cp.gy, out->grid_z = r.cp.gz, out->block = r.cp.block, out->lds = (int64_t)r.cp.lds;
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_op_norm_conv(const vits_norm_conv_desc* d, const float* x, const float* gamma, const float* beta, const float* w, const float* bias,
                               const float* residual, const int32_t* lens, float* y, float* ln_out) {
    VITS_TRY
    if (!d || !x || !gamma || !beta || !w || !y || !ln_out) return fail("vits_op_norm_conv: null argument (bias and residual alone are optional)");
    const KernelKnobs defaults;
    KernelKnobsScope scope(&defaults);
    NormConvOpPlan r;
    std::string why;
    if (!norm_conv_resolve(d, g_op_arith, r, why)) return fail(why);
    const int B = d->batch, cin = d->cin, cout = d->cout, T = d->t, ts = d->t_stride, P = r.pitch;
    if (!lens_ok(lens, B, T)) return fail("vits_op_norm_conv: 0 <= lens[b] <= t <= t_stride is required");
    Conv cv;
    DevMem dg, dbe, dx, dln, dy, dres, dl;
    if (!upload_conv(cv, w, bias, cout, cout, cin, d->k, EPI_STD, 0, VITS_ARITH_F32) || !dg.put(gamma, (size_t)cin * 4) || !dbe.put(beta, (size_t)cin * 4) ||
        !dl.put_opt(lens, (size_t)B * 4) || !stage_rows(dx, x, B, cin, ts, P, lens, T) || !dln.fill((size_t)B * cin * P * 4, 0xFF) || !dy.fill((size_t)B * cout * P * 4, 0xFF) ||
        (residual && !stage_rows(dres, residual, B, cout, ts, P, lens, T)))
        return -1;
    ConvCall plain, fused;
    norm_conv_calls(d, dl.i(), plain, fused);
    const TensorRef xr = tref(dx.f(), cin, P), lnr = tref(dln.f(), cin, P);
    plain.y = fused.y = tref(dy.f(), cout, P);
    if (residual) plain.res = fused.res = tref(dres.f(), cout, P);
    hipError_t e;
    if (r.variant == 2) {  // Engine::run_text_encoder's conv_of_norm: the un-normalised tensor in, the normalised one out of the conv's first row group
        fused.x = xr, fused.ln_gamma = dg.f(), fused.ln_beta = dbe.f(), fused.ln_out = lnr;
        e = launch_conv(cv.pc, fused, nullptr);
    } else {  // its fallback: norm_now, then the conv on the normalised tensor
        TensorRef none;
        e = launch_add_layer_norm(xr, none, dg.f(), dbe.f(), lnr, dl.i(), B, cin, T, d->eps, 0, none, nullptr);
        plain.x = lnr;
        if (e == hipSuccess) e = launch_conv(cv.pc, plain, nullptr);
    }
    if (!finish(e, "vits_op_norm_conv: variant " + std::to_string(r.variant))) return -1;
    return unstage_rows(dy, y, B, cout, P, ts, T) && unstage_rows(dln, ln_out, B, cin, P, ts, T) ? 0 : -1;
    VITS_CATCH(-1)
}

VITS_API int vits_op_duration_predictor(const vits_duration_predictor_desc* d, const float* x, const float* w1, const float* b1, const float* g1, const float* be1,
                                        const float* w2, const float* b2, const float* g2, const float* be2, const float* wp, const float* bp, const float* spk_rows,
                                        const int32_t* lens, float* logw) {
    VITS_TRY
    if (!d || !x || !w1 || !b1 || !g1 || !be1 || !w2 || !b2 || !g2 || !be2 || !wp || !bp || !logw) return fail("vits_op_duration_predictor: null argument");
    const int B = d->batch, H = d->hidden, Fc = d->filter, T = d->t, ts = d->t_stride, k = d->k;
    if (B < 1 || H < 1 || Fc < 1 || T < 1 || ts < T || k < 1 || !(k & 1)) return fail("vits_op_duration_predictor: batch, hidden, filter, t >= 1, t <= t_stride and an odd k are required");
    if (d->variant < 0 || d->variant > 3) return fail("vits_op_duration_predictor: variant 0 (planner), 1 (16-token tile), 2 (wide tile) or 3 (un-fused)");
    if (!shape_lens_ok(lens, B, T, ts)) return fail("vits_op_duration_predictor: 0 <= lens[b] <= t <= t_stride is required");
    const DpDetPlan plan = plan_dp_det(H, Fc, k, B, T, d->variant);
    if ((d->variant == 1 || d->variant == 2) && !plan.ok)
        return fail("vits_op_duration_predictor: the fused kernel has no instantiation for hidden " + std::to_string(H) + ", filter " + std::to_string(Fc) + ", k " + std::to_string(k) +
                    " (variant " + std::to_string(d->variant) + " never falls back)");
    // the predictor runs in fp32 whatever vits_op_set_arith says; its fused kernel reads the second arrangement of all three convs
    Conv cv[3];
    const size_t nx = (size_t)B * H * ts * 4, na = (size_t)B * Fc * ts * 4;
    DevMem dx, dg1, dbe1, dg2, dbe2, drows, dlogw, dxp, da, db, dl;
    if (!upload_conv(cv[0], w1, b1, Fc, Fc, H, k, EPI_STD, 0, VITS_ARITH_F32, true) || !upload_conv(cv[1], w2, b2, Fc, Fc, Fc, k, EPI_STD, 0, VITS_ARITH_F32, true) ||
        !upload_conv(cv[2], wp, bp, 1, 1, Fc, 1, EPI_STD, 0, VITS_ARITH_F32, true) || !stage_rows(dx, x, B, H, ts, ts, lens, T) || !dg1.put(g1, (size_t)Fc * 4) ||
        !dbe1.put(be1, (size_t)Fc * 4) || !dg2.put(g2, (size_t)Fc * 4) || !dbe2.put(be2, (size_t)Fc * 4) || !dlogw.put(logw, (size_t)B * ts * 4) || !dl.put_opt(lens, (size_t)B * 4) ||
        (spk_rows && !drows.put(spk_rows, (size_t)B * H * 4)))
        return -1;
    DpDetCall c;
    c.x = tref(dx.f(), H, ts);
    c.logw = tref(dlogw.f(), 1, ts);
    c.c1 = &cv[0].pc, c.c2 = &cv[1].pc, c.proj = &cv[2].pc;
    c.g1 = dg1.f(), c.be1 = dbe1.f(), c.g2 = dg2.f(), c.be2 = dbe2.f();
    if (spk_rows) c.rows = drows.f(), c.row_rs = H;  // (row b for utterance b)
    c.lens = dl.i();
    c.batch = B, c.hidden = H, c.filter = Fc, c.tmax = T, c.k = k;
    c.eps = d->eps;
    c.variant = d->variant == 3 ? 0 : d->variant;
    hipError_t e = hipSuccess;
    if (plan.ok) {
        e = launch_dp_det(c, nullptr);
    } else {
        // the un-fused sequence: the function Engine::run_duration_predictor_det calls
        if (!da.fill(na, 0) || !db.fill(na, 0) || (spk_rows && !dxp.fill(nx, 0))) return -1;
        e = launch_dp_det_unfused(c, spk_rows ? tref(dxp.f(), H, ts) : TensorRef(), tref(da.f(), Fc, ts), tref(db.f(), Fc, ts), nullptr);
    }
    return finish(e) && dlogw.get(logw, (size_t)B * ts * 4) ? 0 : -1;
    VITS_CATCH(-1)
}

// ---- vits_op_dds_block: which kernels a descriptor names (host arithmetic only: launch_plan.h), then the engine's launch sequences on staged tensors --------
namespace {
struct DdsOpPlan {
    int variant = 0, nt = 0, launches = 0;
    std::string kernel, kernel_last;
    int halo[8] = {0}, dil[8] = {0};
    size_t lds[8] = {0};
    LaunchGrid g;
};
bool dds_fail(std::string& why, const std::string& m) {
    why = "vits_op_dds_block: " + m;
    return false;
}
bool dds_resolve(const vits_dds_block_desc* d, int arith, DdsOpPlan& r, std::string& why) {
    if (arith != VITS_ARITH_F32 && arith != VITS_ARITH_F16 && arith != VITS_ARITH_BF16)
        return dds_fail(why, "VITS_ARITH_F32, VITS_ARITH_F16 or VITS_ARITH_BF16 only (the split arithmetic has no DDS kernels)");
    const int H = d->channels, k = d->k, B = d->batch, T = d->t, NL = d->layers;
    if (B < 1 || T < 1 || d->t_stride < T) return dds_fail(why, "batch >= 1 and 1 <= t <= t_stride are required");
    if (H < 1) return dds_fail(why, "channels = " + std::to_string(H) + ": at least 1");
    if (k < 1 || k > 64) return dds_fail(why, "k = " + std::to_string(k) + ": 1 to 64 taps");
    if (NL < 1 || NL > 8) return dds_fail(why, "layers = " + std::to_string(NL) + ": 1 to 8 layers");
    if (!(d->eps > 0.f)) return dds_fail(why, "eps must be positive");
    if (d->variant < 0 || d->variant > 3)
        return dds_fail(why, "variant " + std::to_string(d->variant) + ": 0 (the engine's choice), 1 (three launches per layer), 2 (dds_layer_kernel), 3 (dds_layer_lat_kernel)");
    if (d->head < 0 || d->head > 2) return dds_fail(why, "head " + std::to_string(d->head) + ": 0 (none), 1 (1 -> H conv of a latent row + conditioning), 2 (H -> H 1x1 conv)");
    if (d->tail < 0 || d->tail > 1) return dds_fail(why, "tail " + std::to_string(d->tail) + ": 0 (none) or 1 (a tail_rows x H 1x1 projection)");
    if (d->tail == 1 && d->tail_rows < 1) return dds_fail(why, "tail_rows = " + std::to_string(d->tail_rows) + ": at least 1");
    if (d->head == 1 && d->zc != 0 && d->zc != 1) return dds_fail(why, "zc = " + std::to_string(d->zc) + ": latent row 0 or 1");
    if (d->head == 2 && d->n_bias_rows < 1) return dds_fail(why, "n_bias_rows = " + std::to_string(d->n_bias_rows) + ": the head conv's bias table has at least one row");
    int64_t dl = 1;
    for (int i = 0; i < NL; ++i, dl *= k) {
        if (dl * (k - 1) > 8192) return dds_fail(why, "layer " + std::to_string(i) + ": dilation " + std::to_string(dl) + " is out of range");
        r.dil[i] = (int)dl;
        r.halo[i] = (int)((k * dl - dl) / 2);
    }
    const bool f32 = arith == VITS_ARITH_F32;
    // why dds_layer_kernel (lat false) / dds_layer_lat_kernel (lat true) has no instantiation for this block, or ""
    auto refusal = [&](bool lat) -> std::string {
        const char* fam = lat ? "dds_layer_lat_kernel" : "dds_layer_kernel";
        if (lat && !f32) return std::string("variant 3: ") + fam + " exists in fp32 only";
        if (H < 32 || (H & 31) || H > 256)
            return std::string("no ") + fam + " for channels = " + std::to_string(H) + " (32 to 256 in steps of 32)";
        for (int i = 0; i < NL; ++i) {
            const std::string at = "layer " + std::to_string(i) + " (k = " + std::to_string(k) + ", dilation " + std::to_string(r.dil[i]) + "): ";
            if ((k * r.dil[i] - r.dil[i]) & 1) return at + "(k - 1) * dilation is odd: no symmetric halo for " + fam;
            const size_t lds = lat ? dds_lat_lds(H, k, r.dil[i], true, H) : dds_layer_lds(H, k, r.dil[i]);
            if (lds > kLdsSoft) return at + fam + " needs " + std::to_string(lds) + " bytes of LDS, the limit is " + std::to_string(kLdsSoft);
            if (!(lat ? plan_dds_layer_lat(H, k, r.dil[i], true, B, T).ok : plan_dds_layer(H, k, r.dil[i], B, T).ok)) return at + "the planner refuses " + fam;
        }
        if (lat && d->tail == 1 && d->tail_rows > H) return "variant 3: tail_rows = " + std::to_string(d->tail_rows) + " exceeds channels = " + std::to_string(H);
        return "";
    };
    int v = d->variant;
    if (v == 0)  // Engine::dds_lat_ok, then Engine::run_dds
        v = f32 && NL >= 2 && dds_lat_grid_ok(B, T) && refusal(true).empty() ? 3 : NL >= 2 && refusal(false).empty() ? 2 : 1;
    r.variant = v;
    const int ends = (d->head ? 1 : 0) + (d->tail ? 1 : 0);
    char name[96];
    if (v == 1) {
        for (int i = 0; i < NL; ++i) {
            const LaunchGrid g = plan_dds_depthwise(H, k, r.dil[i], B, T);
            r.lds[i] = dds_depthwise_lds(H, k, r.dil[i]);
            if (!g.ok)
                return dds_fail(why, "variant 1: layer " + std::to_string(i) + ": dds_depthwise_kernel needs " + std::to_string(r.lds[i]) + " bytes of LDS, the limit is " +
                                         std::to_string(kLdsSoft));
            if (i == 0) r.g = g;
        }
        if (!plan_add_layer_norm(H, B, T).ok) return dds_fail(why, "variant 1: add_layer_norm_kernel has no tile for channels = " + std::to_string(H));
        r.kernel = r.kernel_last = "dds_depthwise_kernel";
        r.nt = 64, r.launches = 3 * NL + ends;
        return true;
    }
    const std::string no = refusal(v == 3);
    if (!no.empty()) return dds_fail(why, (no.rfind("variant", 0) == 0 ? "" : "variant " + std::to_string(v) + ": ") + no);
    if (v == 2) {
        const DdsLayerPlan pl = plan_dds_layer(H, k, 1, B, T);
        std::snprintf(name, sizeof(name), "dds_layer_kernel<%d, %d>", arith, pl.m);
        r.kernel = r.kernel_last = name;
        for (int i = 0; i < NL; ++i) r.lds[i] = dds_layer_lds(H, k, r.dil[i]);
        r.g = pl, r.nt = 32, r.launches = NL + ends;
        return true;
    }
    const DdsLayerPlan pl = plan_dds_layer_lat(H, k, 1, d->head == 2, B, T);
    std::snprintf(name, sizeof(name), "dds_layer_lat_kernel<%d, %d, %d>", d->head, NL == 1 ? d->tail : 0, pl.m);
    r.kernel = name;
    std::snprintf(name, sizeof(name), "dds_layer_lat_kernel<%d, %d, %d>", NL == 1 ? d->head : 0, d->tail, pl.m);
    r.kernel_last = name;
    for (int i = 0; i < NL; ++i) r.lds[i] = dds_lat_lds(H, k, r.dil[i], i == 0 && d->head == 2, H);
    r.g = pl, r.nt = kLatNT, r.launches = NL;
    return true;
}
}  // namespace

VITS_API int vits_op_dds_block_plan(const vits_dds_block_desc* d, vits_dds_block_plan* out) {
    VITS_TRY
    if (!d || !out) return fail("vits_op_dds_block_plan: null argument");
    DdsOpPlan r;
    std::string why;
    if (!dds_resolve(d, g_op_arith, r, why)) return fail(why);
    std::memset(out, 0, sizeof(*out));
    std::snprintf(out->kernel, sizeof(out->kernel), "%s", r.kernel.c_str());
    std::snprintf(out->kernel_last, sizeof(out->kernel_last), "%s", r.kernel_last.c_str());
    out->variant = r.variant, out->nt = r.nt, out->layers = d->layers, out->launches = r.launches;
    for (int i = 0; i < d->layers; ++i) out->halo[i] = r.halo[i], out->lds[i] = (int64_t)r.lds[i];
    out->grid_x = r.g.gx, out->grid_y = r.g.gy, out->block = r.g.block;
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_op_dds_block(const vits_dds_block_desc* d, const float* x, const float* z, const float* cond, const float* head_w, const float* head_b,
                               const int32_t* bias_rows, const float* dw_w, const float* dw_b, const float* g1, const float* b1, const float* pw_w,
                               const float* pw_b, const float* g2, const float* b2, const float* tail_w, const float* tail_b, const int32_t* lens, float* y,
                               float* y2) {
    VITS_TRY
    if (!d || !dw_w || !dw_b || !g1 || !b1 || !pw_w || !pw_b || !g2 || !b2) return fail("vits_op_dds_block: null argument (every per-layer parameter is required)");
    const int arith = g_op_arith;
    DdsOpPlan r;
    std::string why;
    if (!dds_resolve(d, arith, r, why)) return fail(why);
    const int B = d->batch, H = d->channels, T = d->t, ts = d->t_stride, k = d->k, NL = d->layers, TR = d->tail ? d->tail_rows : 0;
    if (d->head != 1 && !x) return fail("vits_op_dds_block: x is required with head 0 and head 2");
    if (d->head == 1 && (!z || !cond)) return fail("vits_op_dds_block: z and cond are required with head 1");
    if (d->head && (!head_w || !head_b)) return fail("vits_op_dds_block: head_w and head_b are required with a head");
    if (d->tail && (!tail_w || !tail_b || !y2)) return fail("vits_op_dds_block: tail_w, tail_b and y2 are required with a tail");
    if (!d->tail && !y) return fail("vits_op_dds_block: y is required without a tail");
    for (int b = 0; b < B; ++b) {
        if (lens && (lens[b] < 0 || lens[b] > T)) return fail("vits_op_dds_block: 0 <= lens[b] <= t is required");
        if (d->head == 2 && bias_rows && (bias_rows[b] < 0 || bias_rows[b] >= d->n_bias_rows)) return fail("vits_op_dds_block: 0 <= bias_rows[b] < n_bias_rows is required");
    }
    // the 1x1 convs: dds_layer_lat_kernel reads the second arrangement of every one, at any channel count
    std::vector<Conv> pw(NL);
    Conv hconv, tconv;
    DevMem ddw_w, ddw_b, dg1, db1, dg2, db2, dhw, dhb;
    const size_t nlh = (size_t)NL * H * 4;
    if (!ddw_w.put(dw_w, nlh * k) || !ddw_b.put(dw_b, nlh) || !dg1.put(g1, nlh) || !db1.put(b1, nlh) || !dg2.put(g2, nlh) || !db2.put(b2, nlh)) return -1;
    for (int i = 0; i < NL; ++i)
        if (!upload_conv(pw[i], pw_w + (size_t)i * H * H, pw_b + (size_t)i * H, H, H, H, 1, EPI_STD, 0, arith, true)) return -1;
    if (d->head == 1 && (!dhw.put(head_w, (size_t)H * 4) || !dhb.put(head_b, (size_t)H * 4))) return -1;
    if (d->head == 2) {
        if (!upload_conv(hconv, head_w, head_b, (size_t)d->n_bias_rows * H, H, H, 1, EPI_STD, 0, arith, true)) return -1;
        hconv.pc.bias_rs = bias_rows ? H : 0;
    }
    if (d->tail && !upload_conv(tconv, tail_w, tail_b, TR, TR, H, 1, EPI_STD, 0, arith, true)) return -1;
    // buffers nobody uploads into are NaN bytes
    DevMem dl, dspk, dx, da, dbb, dc, dz, dcond, dy2, dx16;
    if (!dl.put_opt(lens, (size_t)B * 4) || !dspk.put_opt(d->head == 2 ? bias_rows : nullptr, (size_t)B * 4)) return -1;
    const size_t nh = (size_t)B * H * ts * 4;
    if (!stage_rows(dx, d->head == 1 ? nullptr : x, B, H, ts, ts, lens, T) || !da.fill(nh, 0xFF) || !dbb.fill(nh, 0xFF) || !dc.fill(nh, 0xFF)) return -1;
    if (d->head == 1 && (!stage_rows(dz, z, B, 2, ts, ts, lens, T) || !stage_rows(dcond, cond, B, H, ts, ts, lens, T))) return -1;
    if (d->tail && !dy2.fill((size_t)B * TR * ts * 4, 0xFF)) return -1;
    const size_t x16_bytes = arith == VITS_ARITH_F32 ? 0 : group16_bytes(B, H, T);
    if (x16_bytes && !dx16.fill(x16_bytes, 0xFF)) return -1;
    auto mk = [&](TensorRef xin, TensorRef yout) {
        ConvCall c;
        c.x = xin, c.y = yout, c.len_in = c.len_out = dl.i(), c.spk = dspk.i(), c.batch = B, c.t_in = c.t_out = T;
        return c;
    };
    const TensorRef xin = tref(dx.f(), H, ts), ba = tref(da.f(), H, ts), bb = tref(dbb.f(), H, ts), bc = tref(dc.f(), H, ts);
    const TensorRef zr = tref(dz.f(), 2, ts), cr = tref(dcond.f(), H, ts), y2r = tref(dy2.f(), std::max(TR, 1), ts);
    auto lw = [&](const DevMem& p, int i, int per) { return p.f() + (size_t)i * H * per; };
    TensorRef none, out;  // out: where the block's output lies
    hipError_t e = hipSuccess;
    if (r.variant == 3) {
        // Engine::run_dds_lat: a, b ping-pong; the last layer writes the output buffer (or, with a tail, only y2)
        TensorRef src;
        out = d->tail ? none : bc;
        for (int i = 0; i < NL && e == hipSuccess; ++i) {
            DdsLatCall c;
            c.dw_w = lw(ddw_w, i, k), c.dw_b = lw(ddw_b, i, 1), c.g1 = lw(dg1, i, 1), c.b1 = lw(db1, i, 1), c.g2 = lw(dg2, i, 1), c.b2 = lw(db2, i, 1);
            c.pw = &pw[i].pc;
            c.lens = dl.i();
            c.batch = B, c.channels = H, c.tmax = T, c.k = k, c.dil = r.dil[i];
            c.eps = d->eps;
            if (i == 0) {
                if (d->head == 1) c.head_w = dhw.f(), c.head_b = dhb.f(), c.z = zr, c.cond = cr, c.zc = d->zc;
                else if (d->head == 2) c.head_conv = &hconv.pc, c.x = xin, c.spk = dspk.i();
                else c.x = xin;
            } else
                c.x = src;
            const TensorRef dst = src.p == ba.p ? bb : ba;
            if (i == NL - 1 && d->tail) c.tail_conv = &tconv.pc, c.y2 = y2r;
            else c.y = i == NL - 1 ? bc : dst;
            e = launch_dds_layer_lat(c, nullptr);
            src = dst;
        }
    } else {
        // head as its own launch, then Engine::run_dds on (x, y, p) = (cur, ba, bb), then the tail conv
        TensorRef cur = xin;
        if (d->head == 1) {
            cur = bc;
            e = launch_pointwise_from1(zr, d->zc, dhw.f(), dhb.f(), cr, cur, dl.i(), B, H, T, nullptr, arith);
        } else if (d->head == 2) {
            cur = bc;
            e = conv_transparent(hconv.pc, mk(xin, cur), arith, dx16, x16_bytes);
        }
        out = cur;
        if (r.variant == 2) {
            TensorRef src = cur;
            for (int i = 0; i < NL && e == hipSuccess; ++i) {
                // (Engine::run_dds takes this path from two layers on, so that the last layer can write x again; one layer writes y here)
                const TensorRef dst = NL == 1 ? ba : i == NL - 1 ? cur : (src.p == ba.p ? bb : ba);
                e = launch_dds_layer(src, dst, lw(ddw_w, i, k), lw(ddw_b, i, 1), lw(dg1, i, 1), lw(db1, i, 1), pw[i].pc, lw(dg2, i, 1), lw(db2, i, 1), dl.i(), B, H, T, k, r.dil[i],
                                     d->eps, arith, nullptr);
                src = dst;
            }
            if (NL == 1) out = ba;
        } else {
            for (int i = 0; i < NL && e == hipSuccess; ++i) {
                e = launch_dds_depthwise(cur, none, lw(ddw_w, i, k), lw(ddw_b, i, 1), lw(dg1, i, 1), lw(db1, i, 1), ba, dl.i(), B, H, T, k, r.dil[i], d->eps, nullptr, arith);
                if (e == hipSuccess) e = conv_transparent(pw[i].pc, mk(ba, bb), arith, dx16, x16_bytes);
                if (e == hipSuccess) e = launch_add_layer_norm(bb, none, lw(dg2, i, 1), lw(db2, i, 1), none, dl.i(), B, H, T, d->eps, 1, cur, nullptr);
            }
        }
        if (e == hipSuccess && d->tail) e = conv_transparent(tconv.pc, mk(out, y2r), arith, dx16, x16_bytes);
    }
    if (!finish(e, "vits_op_dds_block: " + r.kernel)) return -1;
    if (y) {
        if (out.p) {
            if (hipMemcpy(y, out.p, nh, hipMemcpyDeviceToHost) != hipSuccess) return fail("copy back failed");
        } else
            std::memset(y, 0xFF, nh);
    }
    if (d->tail && !dy2.get(y2, (size_t)B * TR * ts * 4)) return -1;
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_op_spline(int32_t batch, int32_t t, int32_t t_stride, int32_t bins, float tail, float inv_sqrt, int32_t mode, int32_t zc, const float* u,
                            float* z, const int32_t* lens) {
    VITS_TRY
    if (!u || !z) return fail("vits_op_spline: null argument");
    if (batch < 1 || t < 1 || t_stride < t) return fail("vits_op_spline: batch >= 1 and 1 <= t <= t_stride are required");
    if (bins < 1 || bins > 16) return fail("vits_op_spline: bins = " + std::to_string(bins) + ": spline_kernel takes 1 to 16 bins");
    if (t > 4096) return fail("vits_op_spline: t = " + std::to_string(t) + ": spline_kernel takes at most 4096 tokens");
    if (mode != VITS_MODE_HF && mode != VITS_MODE_REFERENCE) return fail("vits_op_spline: mode is VITS_MODE_HF or VITS_MODE_REFERENCE");
    if (zc != 0 && zc != 1) return fail("vits_op_spline: zc is latent row 0 or 1");
    if (!(tail > 0.f)) return fail("vits_op_spline: tail must be positive");
    if (!shape_lens_ok(lens, batch, t, t_stride)) return fail("vits_op_spline: 0 <= lens[b] <= t <= t_stride is required");
    const int rows = 3 * bins - 1;
    const size_t nz = (size_t)batch * 2 * t_stride * 4;
    DevMem du, dz, dl;
    if (!stage_rows(du, u, batch, rows, t_stride, t_stride, lens, t) || !dz.put(z, nz) || !dl.put_opt(lens, (size_t)batch * 4)) return -1;
    const hipError_t e = launch_spline(tref(du.f(), rows, t_stride), tref(dz.f(), 2, t_stride), zc, dl.i(), batch, t, bins, tail, inv_sqrt, mode, nullptr);
    return finish(e, "vits_op_spline") && dz.get(z, nz) ? 0 : -1;
    VITS_CATCH(-1)
}

VITS_API int vits_op_durations(int32_t batch, int32_t rows, int32_t row, int32_t t_stride, const float* logw, const int32_t* lens, float length_scale,
                               const float* length_scales, const int32_t* ovr, int32_t fixed, int32_t n_stage, const int32_t* stage_mul,
                               const int32_t* stage_add, float* dur, int32_t* cum, int32_t* frames, int32_t* stage_lens) {
    VITS_TRY
    if (!logw || !dur || !cum || !frames) return fail("vits_op_durations: null argument");
    if (batch < 1 || rows < 1 || row < 0 || row >= rows || t_stride < 1) return fail("vits_op_durations: batch, rows, t_stride >= 1 and 0 <= row < rows are required");
    if (n_stage < 0 || n_stage > 16 || (n_stage && (!stage_mul || !stage_add || !stage_lens))) return fail("vits_op_durations: 0 to 16 stages, each with a multiplier and an addend");
    if (!shape_lens_ok(lens, batch, t_stride, t_stride)) return fail("vits_op_durations: 0 <= lens[b] <= t_stride is required");
    const size_t nt = (size_t)batch * t_stride * 4;
    DevMem dlogw, dls, dovr, ddur, dcum, dfr, dsl, dmul, dadd, dl;
    if (!dlogw.put(logw, nt * rows) || !dl.put_opt(lens, (size_t)batch * 4) || !ddur.fill(nt, 0xFF) || !dcum.fill(nt, 0xFF) || !dfr.fill((size_t)batch * 4, 0xFF) ||
        !dsl.fill((size_t)std::max(n_stage, 1) * batch * 4, 0xFF) || !dls.put_opt(length_scales, (size_t)batch * 4) || !dovr.put_opt(ovr, nt) ||
        (n_stage && (!dmul.put(stage_mul, (size_t)n_stage * 4) || !dadd.put(stage_add, (size_t)n_stage * 4))))
        return -1;
    const hipError_t e = launch_durations(tref(dlogw.f(), rows, t_stride), row, dl.i(), batch, t_stride, length_scale, dls.f(), dovr.i(), fixed, ddur.f(), dcum.i(), dfr.i(), dsl.i(),
                                          n_stage, dmul.i(), dadd.i(), nullptr);
    if (!finish(e, "vits_op_durations")) return -1;
    return ddur.get(dur, nt) && dcum.get(cum, nt) && dfr.get(frames, (size_t)batch * 4) && (!n_stage || dsl.get(stage_lens, (size_t)n_stage * batch * 4)) ? 0 : -1;
    VITS_CATCH(-1)
}

VITS_API int vits_op_fit_durations(int32_t batch, int32_t rows, int32_t row, int32_t t_stride, const float* logw, const int32_t* lens, const int32_t* fixed,
                                   const int32_t* groups, const int64_t* target_frames, float min_rate, float max_rate, float* e_out, int32_t* dur_out,
                                   double* group_rows_out) {
    VITS_TRY
    const std::string who = "vits_op_fit_durations: ";
    if (!logw || !target_frames || !e_out || !dur_out || !group_rows_out) return fail(who + "null argument");
    if (rows < 1 || row < 0 || row >= rows) return fail(who + "rows >= 1 and 0 <= row < rows are required");
    std::string err;
    FitCall c;
    if (!fit_check_rows(batch, t_stride, fixed, lens, err) || !fit_check(batch, groups, target_frames, err) || !fit_limits(min_rate, max_rate, c.g.s_lo, c.g.s_hi, err))
        return fail(who + err);
    const size_t nt = (size_t)batch * t_stride * 4;
    const std::vector<int> tgt(target_frames, target_frames + batch);
    DevMem dlogw, dl, dfix, dgrp, dtgt, de, ddur, drows;
    // (the override rows are staged like logw: INT_MIN-like 0xFF bytes = -1 behind every length would hide a read there, so the tail holds 0x7F bytes instead)
    std::vector<int32_t> hfix;
    if (fixed) {
        hfix.assign((size_t)batch * t_stride, 0x7F7F7F7F);
        for (int b = 0; b < batch; ++b) std::memcpy(&hfix[(size_t)b * t_stride], fixed + (size_t)b * t_stride, sizeof(int32_t) * (size_t)(lens ? lens[b] : t_stride));
    }
    if (!stage_rows(dlogw, logw, batch, rows, t_stride, t_stride, lens, t_stride) || !dl.put_opt(lens, (size_t)batch * 4) || (fixed && !dfix.put(hfix.data(), nt)) ||
        !dgrp.put_opt(groups, (size_t)batch * 4) || !dtgt.put(tgt.data(), (size_t)batch * 4) || !de.fill(nt, g_op_out_fill) || !ddur.fill(nt, g_op_out_fill) ||
        !drows.fill((size_t)batch * kFitRowInts * 8, g_op_out_fill))
        return -1;
    c.logw = tref(dlogw.f(), rows, t_stride);
    c.c = row;
    c.lens = dl.i();
    c.fixed = dfix.i();
    c.g.group = dgrp.i();
    c.g.target = dtgt.i();
    c.e = de.f();
    c.dur = ddur.i();
    c.rows = static_cast<int64_t*>(drows.p);
    c.batch = batch, c.tmax = t_stride;
    if (!finish(launch_fit_durations(c, nullptr), "vits_op_fit_durations")) return -1;
    std::vector<int64_t> hrows((size_t)batch * kFitRowInts);
    if (!de.get(e_out, nt) || !ddur.get(dur_out, nt) || !drows.get(hrows.data(), hrows.size() * 8)) return -1;
    fit_rows_double(batch, hrows.data(), group_rows_out);
    return 0;
    VITS_CATCH(-1)
}

VITS_API int vits_op_align(int32_t batch, const int32_t* T, const int32_t* L, int32_t F, const float* m, const float* ls, const float* z, int32_t* durations,
                           float* scores) {
    VITS_TRY
    if (batch <= 0 || !T || !L || F <= 0 || !m || !ls || !z || !durations) return fail("null argument or empty batch");
    int tmax = 0, lmax = 0;
    for (int b = 0; b < batch; ++b) {
        if (T[b] < 1 || T[b] > L[b]) return fail("vits_op_align: 1 <= T[b] <= L[b] is required");
        tmax = std::max(tmax, T[b]);
        lmax = std::max(lmax, L[b]);
    }
    if (tmax > 4096) return fail("vits_op_align: at most 4096 tokens");
    const int ts = round_up(tmax, 32), lstr = round_up(lmax, 32);
    const size_t bit_words = align_mas_bits_in_lds(tmax, lmax) ? 0 : align_mas_bits_words(tmax, lmax);
    DevMem dm, ds, dz, da, dq, dc, dlp, dbits, dscore, dt, dl, ddur;
    if (!dm.put(m, (size_t)batch * F * tmax * 4) || !ds.put(ls, (size_t)batch * F * tmax * 4) || !dz.put(z, (size_t)batch * F * lmax * 4) ||
        !da.fill((size_t)batch * 2 * F * ts * 4, 0) || !dq.fill((size_t)batch * 2 * F * lstr * 4, 0) || !dc.fill((size_t)batch * ts * 4, 0) ||
        !dlp.fill((size_t)batch * ts * lstr * 4, 0) || !dbits.fill((size_t)batch * bit_words * 8, 0) || !dscore.fill((size_t)batch * 4, 0) || !dt.put(T, (size_t)batch * 4) ||
        !dl.put(L, (size_t)batch * 4) || !ddur.alloc((size_t)batch * tmax * 4))
        return -1;
    AlignCall c;
    c.mean = tref(dm.f(), F, tmax);
    c.logs = tref(ds.f(), F, tmax);
    c.z = tref(dz.f(), F, lmax);
    c.tlens = dt.i();
    c.frames = dl.i();
    c.channels = F;
    c.batch = batch;
    c.tmax = tmax;
    c.lmax = lmax;
    c.t_stride = ts;
    c.l_stride = lstr;
    c.plane_a = da.f();
    c.plane_z = dq.f();
    c.ct = dc.f();
    c.logp = dlp.f();
    c.bits = bit_words ? static_cast<unsigned long long*>(dbits.p) : nullptr;
    c.dur = ddur.i();
    c.dur_stride = tmax;
    c.score = dscore.f();
    hipError_t e = launch_align_logp(c, nullptr);
    if (e == hipSuccess) e = launch_align_mas(c, nullptr);
    if (!finish(e)) return -1;
    return ddur.get(durations, (size_t)batch * tmax * 4) && (!scores || dscore.get(scores, (size_t)batch * 4)) ? 0 : -1;
    VITS_CATCH(-1)
}
