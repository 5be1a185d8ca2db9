// dds.hip — the duration predictor's dilated depth-separable convolution block (vits.cpp:651-691; depthwise_conv_with_bias :144-169): the depthwise
// half as its own kernel, one whole layer as ONE kernel, and the 1 -> channels conv_pre of a conv flow (vits.cpp:864).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/vits.h"
#include "kernel_common.h"
#include "kernels.h"
#include "phase_timing.h"

namespace vits {

// ---------------------------------------------------------------------------------------------------------
// DDS first half: y = gelu(LN_channels(depthwise_conv_k(x [+ g], dilation) + bias))
//   vits.cpp:651-673 with depthwise_conv_with_bias :144-169 (the reference runs `channels` separate 1-channel
//   convolutions = ~2,300 graph nodes per predictor, Q16). If g != null, x <- x + g is also written back
//   (vits.cpp:651-653 happens once before the layer loop; the engine passes g only for layer 0).
// Block = 64 time steps x all channels, input tile with halo in LDS.
// ---------------------------------------------------------------------------------------------------------
constexpr int LN_GROUPS = kLnGroups;  // (launch_plan.h; the channel groups of layer_norm.hip's kernel: the same partial sums in the same order)

__global__ __launch_bounds__(64 * LN_GROUPS) void dds_depthwise_kernel(float* x, int64_t x_bs, int x_cs, const float* g, int64_t g_bs, int g_cs, const float* w,
                                                            const float* bias, const float* gamma, const float* beta, float* y, int64_t y_bs, int y_cs,
                                                            const int* lens, int channels, int tmax, int k, int dil, float eps, int arith, const uint16_t* gelu_tab) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int pad = (k * dil - dil) / 2;  // vits.cpp:660
    const int xw = 64 + 2 * pad;
    float* xt = sm;                       // [channels][xw]
    float* ht = xt + channels * xw;       // [channels][64]
    float* red = ht + channels * 64;      // [2][LN_GROUPS][64]
    const int b = blockIdx.y, t0 = blockIdx.x * 64;
    const int len = lens ? lens[b] : tmax;
    if (t0 >= len) return;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    for (int c = wid; c < channels; c += LN_GROUPS) {
        for (int i = lane; i < xw; i += 64) {
            const int t = t0 - pad + i;
            float v = 0.f;
            if (t >= 0 && t < len) {
                v = x[(int64_t)b * x_bs + (int64_t)c * x_cs + t];
                if (g) {
                    v += g[(int64_t)b * g_bs + (int64_t)c * g_cs + t];
                }
            }
            xt[c * xw + i] = v;
        }
    }
    __syncthreads();
    if (g) {  // write back x + g for the centre columns (this block owns them)
        for (int c = wid; c < channels; c += LN_GROUPS) {
            const int t = t0 + lane;
            if (t < len) x[(int64_t)b * x_bs + (int64_t)c * x_cs + t] = xt[c * xw + pad + lane];
        }
    }
    const int tl = lane, gq = wid;
    float s = 0.f;
    for (int c = gq; c < channels; c += LN_GROUPS) {
        float a = bias[c];
        for (int j = 0; j < k; ++j) a += round_arith(w[c * k + j], arith) * round_arith(xt[c * xw + tl + j * dil], arith);
        ht[c * 64 + tl] = a;
        s += a;
    }
    red[gq * 64 + tl] = s;
    __syncthreads();
    float msum = 0.f;
#pragma unroll
    for (int q = 0; q < LN_GROUPS; ++q) msum += red[q * 64 + tl];
    const float mean = msum / (float)channels;
    float vs = 0.f;
    for (int c = gq; c < channels; c += LN_GROUPS) {
        const float d = ht[c * 64 + tl] - mean;
        vs += d * d;
    }
    red[(LN_GROUPS + gq) * 64 + tl] = vs;
    __syncthreads();
    float vsum = 0.f;
#pragma unroll
    for (int q = 0; q < LN_GROUPS; ++q) vsum += red[(LN_GROUPS + q) * 64 + tl];
    const float var = vsum / (float)channels;
    const float inv = 1.0f / sqrtf(var + eps);
    const int t = t0 + tl;
    if (t >= len) return;
    for (int c = gq; c < channels; c += LN_GROUPS) y[(int64_t)b * y_bs + (int64_t)c * y_cs + t] = gelu_op((ht[c * 64 + tl] - mean) * inv * gamma[c] + beta[c], gelu_tab);
}

hipError_t launch_dds_depthwise(TensorRef x, TensorRef g, const float* w, const float* bias, const float* gamma, const float* beta, TensorRef y,
                                const int* lens, int batch, int channels, int tmax, int k, int dil, float eps, hipStream_t s, int arith, GgmlTables tabs) {
    const LaunchGrid l = plan_dds_depthwise(channels, k, dil, batch, tmax);
    if (!l.ok) return hipErrorInvalidValue;
    const dim3 grid(l.gx, l.gy);
    const size_t lds = l.lds;
    return launch_lds<&dds_depthwise_kernel>(grid, dim3(l.block), lds, s, x.p, x.bs, x.cs, g.p, g.bs, g.cs, w, bias, gamma, beta, y.p, y.bs, y.cs, lens, channels, tmax, k,
                                             dil, eps, arith, tabs.gelu);
}

// ---------------------------------------------------------------------------------------------------------
// One whole DDS layer as ONE kernel (vits.cpp:655-691):
//     x_out = x + gelu(LN2(pointwise(gelu(LN1(depthwise_k,dil(x))))))
// i.e. dds_depthwise_kernel + the 1x1 conv (conv_mfma.hip / conv16.hip) + add_layer_norm_kernel(gelu, add_to) of the
// three-launch path, with the two intermediates kept in LDS. Block = 32 time steps x all channels, 16 channel groups of 32
// threads. Every sum is taken in the order of the three-launch path (the LayerNorm partial sums per channel group and
// their fixed-order combination; the MFMA chain over the packed weight fragments, chunk by chunk), so the result is
// bit-identical to it — tests/test_gpu_round2.py compares the two. At batch 1 the three launches are 45-50 us of
// latency per layer (12 layers per utterance); this one is ~10.
// The block reads a halo of its neighbours' columns: x_out must not be x (Engine::run_dds rotates three buffers).
// ---------------------------------------------------------------------------------------------------------

struct DdsLayerParams {
    const float* x;
    int64_t x_bs;
    int x_cs;
    float* y;
    int64_t y_bs;
    int y_cs;
    const float *dw_w, *dw_b, *g1, *b1, *pw_b, *g2, *b2;
    const float* wp;      // fp32 A fragments (pack_conv_weights)
    const uint16_t* wp16;  // 16-bit A fragments (pack_conv_weights16)
    const int* lens;
    int channels, tmax, k, dil, nchunks;
    float eps;
    const uint16_t* gelu_tab;  // emulated ggml GELU table (Q8) or nullptr
};
VITS_PHASE_BUF(vits_dds_phase, 16);  // developer instrumentation (tools/dds_micro.hip): per-block phase timestamps, 100 MHz clock
#define DDS_STAMP(i) VITS_PHASE_STAMP(vits_dds_phase, 16, i)

// MAXCH: upper bound of nchunks = channels / 32 — the wave's whole set of weight fragments is fetched into registers at the START
// of the kernel (at batch 1 they come from HBM: six dependent round trips inside the MFMA loop were 1/3 of the kernel), and the
// per-channel parameters go to LDS with the input tile, so that every later phase runs out of LDS and registers.
template <int ARITH, int MAXCH>
__global__ __launch_bounds__(32 * LN_GROUPS) void dds_layer_kernel(DdsLayerParams p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    constexpr int NT = 32;
    constexpr int UB = 12;  // channels a thread works on at once (192 channels / 16 groups: one step)
    const int H = p.channels;
    const int pad = (p.k * p.dil - p.dil) / 2;  // vits.cpp:660
    const int xw = NT + 2 * pad;
    float* xt = sm;                        // [H][xw]   input tile with halo (also the residual)
    float* ht = xt + ((H * xw + 3) & ~3);  // [H][NT]   depthwise output -> gelu(LN1) -> pointwise output
    float* red = ht + H * NT;              // [2][LN_GROUPS][NT]
    float* prm = red + 2 * LN_GROUPS * NT;  // [6][H] dw_b, g1, b1, pw_b, g2, b2; then [H][k] dw_w
    int4v* h16 = reinterpret_cast<int4v*>(prm + ((6 * H + H * p.k + 3) & ~3));  // [H/8][NT] 16-bit operand slots (ARITH != 0)
    const int b = blockIdx.y, t0 = blockIdx.x * NT;
    DDS_STAMP(0);
    const int len = p.lens ? p.lens[b] : p.tmax;
    if (t0 >= len) return;
    const int tid = threadIdx.x, tl = tid & 31, gq = tid >> 5;
    const int lane = tid & 63, wid = tid >> 6;
    const int nmt = H >> 5;
    DDS_STAMP(1);
    // ---- everything this block reads from memory, issued at once: parameters and the input tile first, the weight fragments behind
    // them (147 KB per block in fp32: they may still be in flight while the depthwise phase runs — memory returns in order) ----
    float pv[2][7];
    {
        constexpr int NTH = 32 * LN_GROUPS;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int c = tid + r * NTH < H ? tid + r * NTH : 0;
            pv[r][0] = p.dw_b[c];
            pv[r][1] = p.g1[c];
            pv[r][2] = p.b1[c];
            pv[r][3] = p.pw_b[c];
            pv[r][4] = p.g2[c];
            pv[r][5] = p.b2[c];
        }
    }
    float4 af[ARITH == 0 ? MAXCH * 4 : 1];
    int4v ah[ARITH != 0 ? MAXCH * 2 : 1];
    {
        // flat index over [H][xw], up to 24 loads in flight per thread (a load-then-store loop exposed one memory latency per element)
        const float* xb = p.x + (int64_t)b * p.x_bs;
        constexpr int NTH = 32 * LN_GROUPS, XB = 24;
        const int total = H * xw, dq = NTH / xw, dr = NTH % xw;
        int c = tid / xw, i = tid - c * xw;
        for (int base = tid; base < total || base == tid; base += XB * NTH) {
            float v[XB];
#pragma unroll
            for (int u = 0; u < XB; ++u) {
                const int t = t0 - pad + i;
                v[u] = (base + u * NTH < total && t >= 0 && t < len) ? xb[(int64_t)c * p.x_cs + t] : 0.f;
                c += dq;
                i += dr;
                if (i >= xw) {
                    i -= xw;
                    ++c;
                }
            }
            if (base == tid) {
                float wv[2] = {0.f, 0.f};
#pragma unroll
                for (int r = 0; r < 2; ++r)
                    if (tid + r * NTH < H * p.k) wv[r] = p.dw_w[tid + r * NTH];
                if (wid < nmt) {
                    if constexpr (ARITH == 0) {
                        const float4* wp4 = reinterpret_cast<const float4*>(p.wp) + (size_t)wid * p.nchunks * 4 * 64 + lane;
#pragma unroll
                        for (int q = 0; q < MAXCH * 4; ++q) af[q] = wp4[(q < p.nchunks * 4 ? q : 0) * 64];
                    } else {
                        const int4v* wq = reinterpret_cast<const int4v*>(p.wp16) + (size_t)wid * p.nchunks * 2 * 64 + lane;
#pragma unroll
                        for (int q = 0; q < MAXCH * 2; ++q) ah[q] = wq[(q < p.nchunks * 2 ? q : 0) * 64];
                    }
                }
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    if (tid + r * NTH < H) {
#pragma unroll
                        for (int q = 0; q < 6; ++q) prm[q * H + tid + r * NTH] = pv[r][q];
                    }
                    if (tid + r * NTH < H * p.k) prm[6 * H + tid + r * NTH] = wv[r];
                }
                for (int q = tid + 2 * NTH; q < H * p.k; q += NTH) prm[6 * H + q] = p.dw_w[q];  // (k > 5 at 192 channels)
            }
#pragma unroll
            for (int u = 0; u < XB; ++u)
                if (base + u * NTH < total) xt[base + u * NTH] = v[u];
        }
    }
    __syncthreads();
    DDS_STAMP(2);
    const float *dw_b = prm, *g1 = prm + H, *b1 = prm + 2 * H, *pw_b = prm + 3 * H, *g2 = prm + 4 * H, *b2 = prm + 5 * H, *dw_w = prm + 6 * H;
    // ---- depthwise conv + LayerNorm 1 + gelu (dds_depthwise_kernel, same expressions) ----
    {
        // (UB channels per step: the LDS reads of the chains overlap; every chain and the order of s are those of the one-channel loop)
        constexpr int CS = LN_GROUPS;
        float s = 0.f;
        for (int c0 = gq; c0 < H; c0 += UB * CS) {
            float a[UB];
            int cc[UB];
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                cc[u] = c0 + u * CS < H ? c0 + u * CS : c0;
                a[u] = dw_b[cc[u]];
            }
            for (int j = 0; j < p.k; ++j) {
#pragma unroll
                for (int u = 0; u < UB; ++u) a[u] += round_arith(dw_w[cc[u] * p.k + j], ARITH) * round_arith(xt[cc[u] * xw + tl + j * p.dil], ARITH);
            }
#pragma unroll
            for (int u = 0; u < UB; ++u)
                if (c0 + u * CS < H) {
                    ht[cc[u] * NT + tl] = a[u];
                    s += a[u];
                }
        }
        red[gq * NT + tl] = s;
        __syncthreads();
        float msum = 0.f;
#pragma unroll
        for (int q = 0; q < LN_GROUPS; ++q) msum += red[q * NT + tl];
        const float mean = msum / (float)H;
        float vs = 0.f;
        for (int c0 = gq; c0 < H; c0 += UB * LN_GROUPS) {
            float hv[UB];
#pragma unroll
            for (int u = 0; u < UB; ++u) hv[u] = ht[(c0 + u * LN_GROUPS < H ? c0 + u * LN_GROUPS : c0) * NT + tl];
#pragma unroll
            for (int u = 0; u < UB; ++u)
                if (c0 + u * LN_GROUPS < H) {
                    const float d = hv[u] - mean;
                    vs += d * d;
                }
        }
        red[(LN_GROUPS + gq) * NT + tl] = vs;
        __syncthreads();
        float vsum = 0.f;
#pragma unroll
        for (int q = 0; q < LN_GROUPS; ++q) vsum += red[(LN_GROUPS + q) * NT + tl];
        const float var = vsum / (float)H;
        const float inv = 1.0f / sqrtf(var + p.eps);
        for (int c0 = gq; c0 < H; c0 += UB * LN_GROUPS) {
            float hv[UB], gg[UB], bb[UB];
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const int c = c0 + u * LN_GROUPS < H ? c0 + u * LN_GROUPS : c0;
                hv[u] = ht[c * NT + tl];
                gg[u] = g1[c];
                bb[u] = b1[c];
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const int c = c0 + u * LN_GROUPS;
                if (c >= H) continue;
                float v = gelu_op((hv[u] - mean) * inv * gg[u] + bb[u], p.gelu_tab);
                if constexpr (ARITH == 0) {
                    ht[c * NT + tl] = v;
                } else {
                    // (the three-launch path stores the fp32 value and rounds it in another kernel; left alone, hipcc folds gelu's last
                    // product into the conversion — v_fma_mixlo_f16, ONE rounding instead of two)
                    asm volatile("" : "+v"(v));
                    uint16_t* slot = reinterpret_cast<uint16_t*>(h16 + (c >> 3) * NT + tl);
                    if constexpr (ARITH == 2) {
                        const _Float16 h = (_Float16)v;
                        slot[c & 7] = __builtin_bit_cast(uint16_t, h);
                    } else {
                        const __bf16 h = (__bf16)v;
                        slot[c & 7] = __builtin_bit_cast(uint16_t, h);
                    }
                }
            }
        }
    }
    __syncthreads();
    DDS_STAMP(3);
    // ---- pointwise conv on the matrix cores: wave w owns output rows 32w..32w+31 (the MFMA chain of conv_mfma.hip / conv16.hip) ----
    floatx16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    if (wid < nmt) {
        if constexpr (ARITH == 0) {
            const float* bcol = ht + (lane >> 5) * NT + (lane & 31);
#pragma unroll
            for (int c = 0; c < MAXCH; ++c) {
                if (c < p.nchunks) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const float* bb = bcol + (c * 32 + 8 * g) * NT;
                        const float4 a = af[c * 4 + g];
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bb[0 * NT], acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bb[2 * NT], acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bb[4 * NT], acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bb[6 * NT], acc, 0, 0, 0);
                    }
                }
            }
        } else {
            const int4v* bcol = h16 + (lane >> 5) * NT + (lane & 31);
#pragma unroll
            for (int c = 0; c < MAXCH; ++c) {
                if (c < p.nchunks) {
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk) {
                        const int4v a = ah[c * 2 + kk];
                        const int4v bq = bcol[(c * 4 + 2 * kk) * NT];
                        acc = mfma16<ARITH == 1>(a, bq, acc);
                    }
                }
            }
        }
    }
    DDS_STAMP(4);
    __syncthreads();  // (fp32: every wave is done reading ht)
    DDS_STAMP(5);
    if (wid < nmt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = wid * 32 + (r >> 2) * 8 + (lane >> 5) * 4 + (r & 3);
            ht[row * NT + (lane & 31)] = acc[r] + pw_b[row];
        }
    }
    __syncthreads();
    DDS_STAMP(6);
    // ---- LayerNorm 2 + gelu + residual (add_layer_norm_kernel with post_gelu and add_to, same expressions) ----
    {
        float s = 0.f;
        for (int c0 = gq; c0 < H; c0 += UB * LN_GROUPS) {
            float hv[UB];
#pragma unroll
            for (int u = 0; u < UB; ++u) hv[u] = ht[(c0 + u * LN_GROUPS < H ? c0 + u * LN_GROUPS : c0) * NT + tl];
#pragma unroll
            for (int u = 0; u < UB; ++u)
                if (c0 + u * LN_GROUPS < H) s += hv[u];
        }
        red[gq * NT + tl] = s;
        __syncthreads();
        float msum = 0.f;
#pragma unroll
        for (int q = 0; q < LN_GROUPS; ++q) msum += red[q * NT + tl];
        const float mean = msum / (float)H;
        float vs = 0.f;
        for (int c0 = gq; c0 < H; c0 += UB * LN_GROUPS) {
            float hv[UB];
#pragma unroll
            for (int u = 0; u < UB; ++u) hv[u] = ht[(c0 + u * LN_GROUPS < H ? c0 + u * LN_GROUPS : c0) * NT + tl];
#pragma unroll
            for (int u = 0; u < UB; ++u)
                if (c0 + u * LN_GROUPS < H) {
                    const float d = hv[u] - mean;
                    vs += d * d;
                }
        }
        red[(LN_GROUPS + gq) * NT + tl] = vs;
        __syncthreads();
        float vsum = 0.f;
#pragma unroll
        for (int q = 0; q < LN_GROUPS; ++q) vsum += red[(LN_GROUPS + q) * NT + tl];
        const float var = vsum / (float)H;
        const float inv = 1.0f / sqrtf(var + p.eps);
        const int t = t0 + tl;
        if (t >= len) return;
        float* yb = p.y + (int64_t)b * p.y_bs + t;
        for (int c0 = gq; c0 < H; c0 += UB * LN_GROUPS) {
            float hv[UB], gg[UB], bb[UB], xr[UB];
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const int c = c0 + u * LN_GROUPS < H ? c0 + u * LN_GROUPS : c0;
                hv[u] = ht[c * NT + tl];
                gg[u] = g2[c];
                bb[u] = b2[c];
                xr[u] = xt[c * xw + pad + tl];
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const int c = c0 + u * LN_GROUPS;
                if (c >= H) continue;
                float v = (hv[u] - mean) * inv * gg[u] + bb[u];
                v = gelu_op(v, p.gelu_tab);
                asm volatile("" : "+v"(v));  // (the three-launch path adds in a separate statement behind a branch: no fma of gelu's last product with this add)
                yb[(int64_t)c * p.y_cs] = xr[u] + v;
            }
        }
        DDS_STAMP(7);
    }
}

hipError_t launch_dds_layer(TensorRef x, TensorRef y, const float* dw_w, const float* dw_b, const float* g1, const float* b1, const PackedConv& pw, const float* g2,
                            const float* b2, const int* lens, int batch, int channels, int tmax, int k, int dil, float eps, int arith, hipStream_t s, GgmlTables tabs) {
    if (!dds_layer_supported(pw, channels, k, dil, arith) || x.p == y.p) return hipErrorInvalidValue;
    DdsLayerParams p;
    p.x = x.p, p.x_bs = x.bs, p.x_cs = x.cs, p.y = y.p, p.y_bs = y.bs, p.y_cs = y.cs, p.dw_w = dw_w, p.dw_b = dw_b, p.g1 = g1, p.b1 = b1;
    p.pw_b = pw.bias, p.g2 = g2, p.b2 = b2, p.wp = pw.wp, p.wp16 = pw.wp16, p.lens = lens, p.channels = channels, p.tmax = tmax, p.k = k, p.dil = dil;
    p.nchunks = pw.nchunks, p.eps = eps, p.gelu_tab = tabs.gelu;
    const DdsLayerPlan l = plan_dds_layer(channels, k, dil, batch, tmax);
    const dim3 grid(l.gx, l.gy), block(l.block);
#define VITS_DDS_LAUNCH1(A, M) return launch_lds<&dds_layer_kernel<A, M>>(grid, block, l.lds, s, p)
#define VITS_DDS_LAUNCH(A)                       \
    do {                                         \
        if (l.m == 2) VITS_DDS_LAUNCH1(A, 2);      \
        else if (l.m == 4) VITS_DDS_LAUNCH1(A, 4); \
        else if (l.m == 6) VITS_DDS_LAUNCH1(A, 6); \
        else VITS_DDS_LAUNCH1(A, 8);             \
    } while (0)
    if (arith == VITS_ARITH_F32) VITS_DDS_LAUNCH(0);
    else if (arith == VITS_ARITH_BF16) VITS_DDS_LAUNCH(1);
    else VITS_DDS_LAUNCH(2);
#undef VITS_DDS_LAUNCH1
#undef VITS_DDS_LAUNCH
}

// conv_pre of a conv flow: 1 -> channels pointwise conv of latent row zc (vits.cpp:864): y[c][t] = w[c]*z[zc][t] + b[c]
//   optionally + cond[c][t]: the DDS block's "inputs + global_conditioning" (vits.cpp:651-653), same order of additions
__global__ void pointwise_from1_kernel(const float* z, int64_t z_bs, int z_cs, int zc, const float* w, const float* bias, const float* cond, int64_t c_bs,
                                       int c_cs, float* y, int64_t y_bs, int y_cs, const int* lens, int tmax, int arith) {
    const int b = blockIdx.z, c = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
    const int len = lens ? lens[b] : tmax;
    if (t >= len) return;
    float v = round_arith(w[c], arith) * round_arith(z[(int64_t)b * z_bs + (int64_t)zc * z_cs + t], arith) + bias[c];
    if (cond) v = v + cond[(int64_t)b * c_bs + (int64_t)c * c_cs + t];
    y[(int64_t)b * y_bs + (int64_t)c * y_cs + t] = v;
}
hipError_t launch_pointwise_from1(TensorRef z, int zc, const float* w, const float* bias, TensorRef cond, TensorRef y, const int* lens, int batch, int channels,
                                  int tmax, hipStream_t s, int arith) {
    dim3 grid((tmax + 63) / 64, channels, batch);
    VITS_KLAUNCH(pointwise_from1_kernel, grid, dim3(64), 0, s, z.p, z.bs, z.cs, zc, w, bias, cond.p, cond.bs, cond.cs, y.p, y.bs, y.cs, lens, tmax, arith);
    return hipGetLastError();
}

}  // namespace vits
