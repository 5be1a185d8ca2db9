// dp_det.hip — the deterministic duration predictor (transformers VitsDurationPredictor, eval mode) as ONE launch, exact fp32.
//
//   x'[c][t] = x[c][t] + row[c]                    inside the utterance (the speaker term cond(g), added ON LOAD), 0 outside [0, len)
//   a1 = LayerNorm_channels(relu(conv_1(x') + b1))  conv_1: H -> Fc, k taps, zero padding k / 2;   0 outside [0, len)
//   a2 = LayerNorm_channels(relu(conv_2(a1) + b2))  conv_2: Fc -> Fc, k taps;                      0 outside [0, len)
//   logw[t] = proj(a2)[t] + bp                      proj: Fc -> 1, 1x1
//
// The speaker term is NOT a bias of conv_1: the conv pads x' with zeros, so the first and last k / 2 tokens of an utterance see 0, not cond(g), in the taps that
// reach outside it. That is why the row is added where the tile is staged, and only to columns inside the utterance.
//
// A block owns NT tokens of one utterance (kLatNT = 16 for small grids, 64 - 2 (k / 2) for large ones: launch_plan.h dp_det_geom, plan_dp_det). It stages x' on
// NT + 4 (k / 2) columns, computes a1 on NT + 2 (k / 2) columns and a2 on NT, all in LDS; a2 takes a1's place, the LayerNorm sums take x's.
// Every conv runs on v_mfma_f32_16x16x4_f32 from the layer's second weight copy (repack_conv_weights_l16), wave w owning output rows 16 w .. 16 w + 15 for every
// column tile of the block: the K order is (32-channel chunk, tap, channel), one ascending chain per output from 0, the bias added behind it — the chain of
// conv_mfma_kernel and conv_lat16_kernel. LayerNorm keeps add_layer_norm_kernel's order: kLnGroups channel groups, group g sums channels g, g + 16, ... in
// ascending order, the groups are combined in ascending order, the variance the same way around the mean. So every float equals the un-fused sequence
// launch_add_rows -> launch_conv(relu) -> launch_add_layer_norm -> launch_conv(relu) -> launch_add_layer_norm -> launch_conv, which is the engine's fallback
// for shapes without an instantiation (tests/test_gpu_detdp_ops.py compares them bit for bit), a row of a batch equals its batch-1 call, and both tiles agree.
// The weights (1.4 MB at H = 192, Fc = 256, k = 3) stream from L2: a wave keeps a ring of eight quads of its fragments in flight in front of the MFMAs that consume them.
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernel_common.h"
#include "kernels.h"

namespace vits {

struct DpDetParams {
    const float* x;
    int64_t x_bs;
    int x_cs;
    const float* rows;  // per-utterance rows [*][H] (row stride row_rs), or nullptr
    int64_t row_rs;
    const int* row_idx;
    const float *w1, *b1, *g1, *be1, *w2, *b2, *g2, *be2, *wp, *bp;  // w*: 16x16x4 A fragments
    float* logw;
    int64_t l_bs;
    const int* lens;
    int H, tmax;
    float eps;
};

namespace {

constexpr int G = kLnGroups;

// One wave's 16 output rows of a K-tap conv over CT column tiles of the LDS tile bt[channel][pitch] (column 0 = the first tap of output column 0):
// frag = the row tile's fragment stream, nq = 2 * chunks * K quads of 64 lanes x float4; quad q = 16 channels (half hq = q & 1 of chunk (q >> 1) / K) at tap
// (q >> 1) % K, NQ = 2 * chunks * K quads in all. Lane l: B row 4 s + (l >> 4) of the quad for MFMA s, column l & 15.
template <int K, int CT, int NQ>
__device__ __forceinline__ void conv_rows(float4v (&acc)[CT], const float* frag, const float* bt, int pitch, int lane) {
    // A ring of D quads in flight: a quad is 4 CT MFMAs (130 ... 520 cycles), an L2 round trip several times that — with one quad of look-ahead the kernel
    // waited for its weights (53 us at batch 1 x 128 ids, measured; tools/detdp_bench.py)
    constexpr int D = NQ < 8 ? NQ : 8;
    const float4v* f4 = reinterpret_cast<const float4v*>(frag) + lane;
    const int jg = lane >> 4, col = lane & 15;
    const float* b0 = bt + jg * pitch + col;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[ct] = float4v{0.f, 0.f, 0.f, 0.f};
    float4v ring[D];
#pragma unroll
    for (int j = 0; j < D; ++j) ring[j] = f4[(size_t)j * 64];
    for (int q0 = 0; q0 < NQ; q0 += D) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const int q = q0 + j;
            if (q < NQ) {
                const float4v a = ring[j];
                if (q + D < NQ) ring[j] = f4[(size_t)(q + D) * 64];
                const int g = q >> 1, chunk = g / K, tap = g - chunk * K;
                const float* bq = b0 + (chunk * 32 + 16 * (q & 1)) * pitch + tap;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], bq[4 * s * pitch + 16 * ct], acc[ct], 0, 0, 0);
                }
            }
        }
    }
}

// LayerNorm over the C channels of columns [0, ncols) of tile[channel][pitch], in place; column i is time t_first + i and becomes 0 outside [0, len).
// add_layer_norm_kernel's expressions and order of operations. red: [2 G + 2][rw] floats.
__device__ __forceinline__ void layer_norm_tile(float* tile, int pitch, int C, int ncols, float* red, int rw, const float* gamma, const float* beta, float eps, int t_first,
                                                int len, int tid, int nthr) {
    for (int idx = tid; idx < G * ncols; idx += nthr) {
        const int g = idx / ncols, i = idx - g * ncols;
        float s = 0.f;
        for (int c = g; c < C; c += G) s += tile[c * pitch + i];
        red[g * rw + i] = s;
    }
    __syncthreads();
    for (int idx = tid; idx < G * ncols; idx += nthr) {
        const int g = idx / ncols, i = idx - g * ncols;
        float msum = 0.f;
#pragma unroll
        for (int q = 0; q < G; ++q) msum += red[q * rw + i];
        const float mean = msum / (float)C;
        float vs = 0.f;
        for (int c = g; c < C; c += G) {
            const float d = tile[c * pitch + i] - mean;
            vs += d * d;
        }
        red[(G + g) * rw + i] = vs;
        if (g == 0) red[2 * G * rw + i] = mean;
    }
    __syncthreads();
    for (int i = tid; i < ncols; i += nthr) {
        float vsum = 0.f;
#pragma unroll
        for (int q = 0; q < G; ++q) vsum += red[(G + q) * rw + i];
        const float var = vsum / (float)C;
        const float inv = 1.0f / sqrtf(var + eps);
        red[(2 * G + 1) * rw + i] = inv;
    }
    __syncthreads();
    for (int idx = tid; idx < C * ncols; idx += nthr) {
        const int c = idx / ncols, i = idx - c * ncols, t = t_first + i;
        const float mean = red[2 * G * rw + i], inv = red[(2 * G + 1) * rw + i];
        const float v = (tile[c * pitch + i] - mean) * inv * gamma[c] + beta[c];
        tile[c * pitch + i] = (t >= 0 && t < len) ? v : 0.f;
    }
    __syncthreads();
}

}  // namespace

template <int HCH, int FC, int K, int NT>
__global__ __launch_bounds__(FC / 16 * 64) void dp_det_kernel(DpDetParams p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    constexpr DpDetGeom GEO = dp_det_geom(HCH, FC, K, NT);
    constexpr int PAD = GEO.pad, W1 = GEO.w1, CT1 = GEO.ct1, CT2 = GEO.ct2, XP = GEO.xp, AP = GEO.ap, NW = FC / 16, NTHR = NW * 64;
    constexpr int XF = 32 * HCH * XP, RF = (2 * G + 2) * CT1 * 16, RW = CT1 * 16;
    float* xt = sm;                           // [32 HCH][XP]: x' at times t0 - 2 PAD ..; later the LayerNorm sums
    float* red = sm;                          // [2 G + 2][RW]
    float* at = sm + (XF > RF ? XF : RF);     // [FC][AP]: a1 at times t0 - PAD .., then a2 at times t0 ..
    const int b = blockIdx.y, t0 = blockIdx.x * NT;
    const int len = p.lens ? p.lens[b] : p.tmax;
    if (t0 >= len) return;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int jg = lane >> 4, col = lane & 15;
    // ---- x' tile: masked to the utterance, the speaker row added on load inside it ----
    {
        const float* xb = p.x + (int64_t)b * p.x_bs;
        const float* row = p.rows ? p.rows + p.row_rs * (p.row_idx ? p.row_idx[b] : b) : nullptr;
        constexpr int XB = 8;
        for (int base = tid; base < XF; base += XB * NTHR) {
            float v[XB], r[XB];
            bool ok[XB];
#pragma unroll
            for (int u = 0; u < XB; ++u) {
                const int e = base + u * NTHR, c = e / XP, i = e - c * XP, t = t0 - 2 * PAD + i;
                ok[u] = e < XF && c < p.H && i < NT + 4 * PAD && t >= 0 && t < len;
                v[u] = ok[u] ? xb[(int64_t)c * p.x_cs + t] : 0.f;
                r[u] = (ok[u] && row) ? row[c] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < XB; ++u) {
                if (base + u * NTHR >= XF) continue;
                float o = v[u];
                if (row && ok[u]) o = o + r[u];
                xt[base + u * NTHR] = o;
            }
        }
    }
    __syncthreads();
    // ---- conv_1 + bias + relu on W1 columns -> at ----
    {
        float4v acc[CT1];
        conv_rows<K, CT1, 2 * HCH * K>(acc, p.w1 + (size_t)wid * (2 * HCH * K) * 256, xt, XP, lane);
#pragma unroll
        for (int ct = 0; ct < CT1; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = wid * 16 + 4 * jg + r;
                float v = acc[ct][r] + p.b1[co];
                v = v > 0.f ? v : 0.f;
                at[co * AP + 16 * ct + col] = v;
            }
    }
    __syncthreads();  // (also: every wave is done reading xt, whose place the sums take)
    layer_norm_tile(at, AP, FC, W1, red, RW, p.g1, p.be1, p.eps, t0 - PAD, len, tid, NTHR);
    // ---- conv_2 + bias + relu on NT columns, in a1's place ----
    {
        float4v acc[CT2];
        // (columns of `at` at and beyond W1 were never written — uninitialised LDS: column n of a2 reads columns n .. n + K - 1 of a1, so they reach only the
        // output columns >= NT, which nothing stores or normalises)
        conv_rows<K, CT2, 2 * (FC / 32) * K>(acc, p.w2 + (size_t)wid * (2 * (FC / 32) * K) * 256, at, AP, lane);
        __syncthreads();  // every wave is done reading a1
#pragma unroll
        for (int ct = 0; ct < CT2; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = wid * 16 + 4 * jg + r;
                float v = acc[ct][r] + p.b2[co];
                v = v > 0.f ? v : 0.f;
                at[co * AP + 16 * ct + col] = v;
            }
    }
    __syncthreads();
    layer_norm_tile(at, AP, FC, NT, red, RW, p.g2, p.be2, p.eps, t0, len, tid, NTHR);
    // ---- proj: row 0 of a 16-row tile, one wave per column tile ----
    for (int ct = wid; ct < CT2; ct += NW) {
        float4v acc[1];
        conv_rows<1, 1, 2 * (FC / 32)>(acc, p.wp, at + 16 * ct, AP, lane);
        const int t = t0 + 16 * ct + col;
        if (jg == 0 && 16 * ct + col < NT && t < len) p.logw[(int64_t)b * p.l_bs + t] = acc[0][0] + p.bp[0];
    }
}

// ---- the un-fused predictor's first step ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void add_rows_kernel(const float* x, int64_t x_bs, int x_cs, float* y, int64_t y_bs, int y_cs, const float* rows, int64_t row_rs,
                                                       const int* row_idx, const int* lens, int channels, int tmax) {
    const int b = blockIdx.z, c = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
    const int len = lens ? lens[b] : tmax;
    if (t >= len) return;
    const float r = rows[row_rs * (row_idx ? row_idx[b] : b) + c];
    y[(int64_t)b * y_bs + (int64_t)c * y_cs + t] = x[(int64_t)b * x_bs + (int64_t)c * x_cs + t] + r;
}

hipError_t launch_add_rows(TensorRef x, TensorRef y, const float* rows, int64_t row_rs, const int* row_idx, const int* lens, int batch, int channels, int tmax, hipStream_t s) {
    if (!x.p || !y.p || !rows || batch < 1 || channels < 1 || tmax < 1 || channels > 65535 || batch > 65535) return hipErrorInvalidValue;
    VITS_KLAUNCH(add_rows_kernel, dim3(blocks_for(tmax, 256), channels, batch), dim3(256), 0, s, x.p, x.bs, x.cs, y.p, y.bs, y.cs, rows, row_rs, row_idx, lens, channels, tmax);
    return hipGetLastError();
}

// The un-fused predictor: the sequence dp_det_kernel must equal bit for bit, and what runs for every shape without an instantiation. ONE definition, used by the
// engine (Engine::run_duration_predictor_det) and by the operator (vits_op_duration_predictor, variant 3). xp [B][hidden][t] (read only with rows), a, b [B][filter][t].
hipError_t launch_dp_det_unfused(const DpDetCall& c, TensorRef xp, TensorRef a, TensorRef b, hipStream_t s) {
    if (!c.x.p || !c.logw.p || !a.p || !b.p || (c.rows && !xp.p) || !c.c1 || !c.c2 || !c.proj || !c.g1 || !c.be1 || !c.g2 || !c.be2) return hipErrorInvalidValue;
    TensorRef x = c.x, none;
    if (c.rows) {
        if (hipError_t e = launch_add_rows(c.x, xp, c.rows, c.row_rs, c.row_idx, c.lens, c.batch, c.hidden, c.tmax, s)) return e;
        x = xp;
    }
    auto mk = [&](TensorRef xin, TensorRef yout, int taps) {
        ConvCall cc;
        cc.x = xin;
        cc.y = yout;
        cc.len_in = cc.len_out = c.lens;
        cc.batch = c.batch;
        cc.t_in = cc.t_out = c.tmax;
        cc.pad_l = taps / 2;
        cc.post_act = taps > 1 ? 1 : 0;  // relu behind conv_1 / conv_2, none behind proj
        return cc;
    };
    if (hipError_t e = launch_conv(*c.c1, mk(x, a, c.k), s)) return e;
    if (hipError_t e = launch_add_layer_norm(a, none, c.g1, c.be1, b, c.lens, c.batch, c.filter, c.tmax, c.eps, 0, none, s)) return e;
    if (hipError_t e = launch_conv(*c.c2, mk(b, a, c.k), s)) return e;
    if (hipError_t e = launch_add_layer_norm(a, none, c.g2, c.be2, b, c.lens, c.batch, c.filter, c.tmax, c.eps, 0, none, s)) return e;
    return launch_conv(*c.proj, mk(b, c.logw, 1), s);
}

static bool dp_det_convs_ok(const DpDetCall& c) {
    auto ok = [](const PackedConv* w, int cout, int cin, int k) { return w && w->cout == cout && w->cin == cin && w->kt == k && w->epi == EPI_STD && w->bias && w->wp_l16; };
    return ok(c.c1, c.filter, c.hidden, c.k) && ok(c.c2, c.filter, c.filter, c.k) && ok(c.proj, 1, c.filter, 1) && c.g1 && c.be1 && c.g2 && c.be2;
}
bool dp_det_supported(const DpDetCall& c) { return dp_det_shape_exists(c.hidden, c.filter, c.k) && dp_det_convs_ok(c); }

hipError_t launch_dp_det(const DpDetCall& c, hipStream_t s) {
    if (c.variant < 0 || c.variant > 2 || !c.x.p || !c.logw.p || c.batch < 1 || c.tmax < 1 || c.batch > 65535 || !dp_det_convs_ok(c)) return hipErrorInvalidValue;
    const DpDetPlan l = plan_dp_det(c.hidden, c.filter, c.k, c.batch, c.tmax, c.variant);
    if (!l.ok || !l.fused) return hipErrorInvalidValue;
    DpDetParams p{};
    p.x = c.x.p, p.x_bs = c.x.bs, p.x_cs = c.x.cs;
    p.rows = c.rows, p.row_rs = c.row_rs, p.row_idx = c.row_idx;
    p.w1 = c.c1->wp_l16, p.b1 = c.c1->bias, p.g1 = c.g1, p.be1 = c.be1;
    p.w2 = c.c2->wp_l16, p.b2 = c.c2->bias, p.g2 = c.g2, p.be2 = c.be2;
    p.wp = c.proj->wp_l16, p.bp = c.proj->bias;
    p.logw = c.logw.p, p.l_bs = c.logw.bs;
    p.lens = c.lens;
    p.H = c.hidden, p.tmax = c.tmax;
    p.eps = c.eps;
    const dim3 grid(l.gx, l.gy), block(l.block);
    const bool lat = l.nt == kLatNT;
#define VITS_DPDET(HCH, FC, K)                                                                                        \
    do {                                                                                                              \
        static_assert(dp_det_exists(HCH == 1 ? 16 : 32 * HCH, FC, K, kLatNT) && dp_det_exists(HCH == 1 ? 16 : 32 * HCH, FC, K, dp_det_wide_nt(K)), "launch_plan.h names the instantiations"); \
        if (lat) return launch_lds<&dp_det_kernel<HCH, FC, K, kLatNT>>(grid, block, l.lds, s, p);                      \
        return launch_lds<&dp_det_kernel<HCH, FC, K, dp_det_wide_nt(K)>>(grid, block, l.lds, s, p);                    \
    } while (0)
    if (c.hidden == 192 && c.filter == 256 && c.k == 3) VITS_DPDET(6, 256, 3);
    if (c.hidden == 192 && c.filter == 256 && c.k == 5) VITS_DPDET(6, 256, 5);
    if (c.hidden == 16 && c.filter == 32 && c.k == 3) VITS_DPDET(1, 32, 3);
#undef VITS_DPDET
    return hipErrorInvalidValue;
}

}  // namespace vits
