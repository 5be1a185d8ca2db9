// vocoder_glue.hip — the VALU kernels around the vocoder's convolutions, fp32 path: the sum over a stage's resblocks as its own launch
// (vits.cpp:622-635), conv_post (vits.cpp:638-642), and the delivery's fp32 -> int16 PCM (test/main.cpp:31-33).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "kernel_common.h"
#include "kernels.h"

namespace vits {

// ---- ((y0 + y1) [+ y2]) * scale over fp32 [b][c][t] tensors: the sum over a stage's resblocks as its own launch (fp32 path, small grids) -------------
// The fp32 resblock kernels carry the accumulation into the stage's shared sum in their last launch, so resblock j's last launch waits for resblock
// j - 1's (vits.cpp:622-635's order of the additions). With one or two utterances the three chains are a few dozen blocks per kernel and the waits are
// idle chip: here every resblock writes its own output and this kernel adds them in that order with the epilogue's expressions (a + v; the second
// resblock's scale is 1: v * 1 = v; then the scale; then the next upsampler's leaky_relu where the last resblock's epilogue applied it): same bits.
__global__ __launch_bounds__(256) void rb_sum3_std_kernel(const float* y0, const float* y1, const float* y2, int64_t bs, int cs, const int* lens, int tmax, float scale, int scale_div,
                                                           int post_act, float post_slope, float* out, int64_t o_bs, int o_cs) {
    const int b = blockIdx.z, c = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
    const int len = lens ? lens[b] : tmax;
    if (t >= len) return;
    const int64_t go = (int64_t)b * bs + (int64_t)c * cs + t;
    float x = y0[go] + y1[go];
    if (y2) x = x + y2[go];
    x = scale_or_div(x, scale, scale_div);
    if (post_act == 2) x = fmaxf(x, x * post_slope);
    out[(int64_t)b * o_bs + (int64_t)c * o_cs + t] = x;
}
hipError_t launch_rb_sum3_std(TensorRef y0, TensorRef y1, TensorRef y2, TensorRef out, int channels, const int* lens, int batch, int tmax, float scale, int scale_div, int post_act,
                              float post_slope, hipStream_t s) {
    if (!y0.p || !y1.p || !out.p || y0.bs != y1.bs || y0.cs != y1.cs || (y2.p && (y2.bs != y0.bs || y2.cs != y0.cs))) return hipErrorInvalidValue;
    dim3 grid((tmax + 255) / 256, channels, batch);
    VITS_KLAUNCH(rb_sum3_std_kernel, grid, dim3(256), 0, s, y0.p, y1.p, y2.p, y0.bs, y0.cs, lens, tmax, scale, scale_div, post_act, post_slope, out.p, out.bs, out.cs);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// conv_post: leaky_relu -> Conv1d(C -> 1, k, no bias) -> tanh   (vits.cpp:638-642). One output row: a matrix
// tile would be 31/32 empty, so this is a VALU kernel; HBM-bound (reads C floats per output sample).
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void conv_post_kernel(const float* x, int64_t x_bs, int x_cs, const float* w, int cin, int k, float slope, float* pre,
                                                        int64_t p_bs, float* wave, int64_t w_bs, const int* lens, int tmax, int emit_lo, const int* emit_hi, int arith) {
    extern __shared__ __attribute__((aligned(16))) float sm[];  // weights [cin][k]
    const int b = blockIdx.y;
    const int len = lens ? lens[b] : tmax;
    // windowed vocoder (engine.cpp): only samples [emit_lo, emit_hi[b]) of this window are the utterance's own; the rest
    // is halo, computed from a cut edge and owned by a neighbouring window
    const int hi = emit_hi ? min(emit_hi[b], len) : len;
    const int t0 = emit_lo + blockIdx.x * 1024;
    if (t0 >= hi) return;
    for (int i = threadIdx.x; i < cin * k; i += 256) sm[i] = round_arith(w[i], arith);
    __syncthreads();
    const int pad = (k - 1) / 2;
    const float* xb = x + (int64_t)b * x_bs;
    // fast path (k = 7, 16-byte aligned rows, away from the sequence ends): one thread = 4 consecutive samples; per channel
    // three aligned float4 loads cover x[t-4 .. t+7] and feed all 28 products (the scalar path below loads every input 7x).
    // Same order of accumulation per sample (channel-major, tap-minor), so both paths give identical values.
    if (k == 7 && (x_cs & 3) == 0 && ((reinterpret_cast<uintptr_t>(xb) & 15) == 0) && (t0 & 3) == 0) {
        const int t = t0 + 4 * threadIdx.x;
        if (t >= hi) return;
        // interior threads read three aligned float4 per channel; a thread at a sequence end reads the same twelve values one by one,
        // zero outside [0, len) (what the padding contributes). The end threads used to walk a scalar loop of 4 x cin x 7 dependent
        // loads: at batch 1 that ONE thread was the whole kernel time (138 us for a 128-id utterance).
        const bool interior = t >= 4 && t + 8 <= len;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        // eight channels per step, their loads issued before the first product. Accumulation order: channel-major, tap-minor.
        constexpr int CB = 8;
        for (int c0 = 0; c0 < cin; c0 += CB) {
            float4 q[CB][3];
#pragma unroll
            for (int u = 0; u < CB; ++u) {
                const int c = c0 + u < cin ? c0 + u : cin - 1;
                const float* xc = xb + (int64_t)c * x_cs;
                if (interior) {
                    const float4* xr = reinterpret_cast<const float4*>(xc + t - 4);
                    q[u][0] = xr[0], q[u][1] = xr[1], q[u][2] = xr[2];
                } else {
                    float e[12];
#pragma unroll
                    for (int i = 0; i < 12; ++i) {
                        const int tt = t - 4 + i;
                        e[i] = (tt >= 0 && tt < len) ? xc[tt] : 0.f;
                    }
                    q[u][0] = make_float4(e[0], e[1], e[2], e[3]);
                    q[u][1] = make_float4(e[4], e[5], e[6], e[7]);
                    q[u][2] = make_float4(e[8], e[9], e[10], e[11]);
                }
            }
#pragma unroll
            for (int u = 0; u < CB; ++u) {
                if (c0 + u >= cin) break;
                float v[12] = {q[u][0].x, q[u][0].y, q[u][0].z, q[u][0].w, q[u][1].x, q[u][1].y,
                               q[u][1].z, q[u][1].w, q[u][2].x, q[u][2].y, q[u][2].z, q[u][2].w};  // v[i] = x[t - 4 + i]
#pragma unroll
                for (int i = 1; i < 11; ++i) v[i] = round_arith(v[i] > 0.f ? v[i] : v[i] * slope, arith);
                const float* wc = sm + (c0 + u) * 7;
#pragma unroll
                for (int j = 0; j < 7; ++j) {  // sample t + e reads x[t + e + j - 3] = v[e + j + 1]
                    const float wj = wc[j];
                    a0 += wj * v[j + 1];
                    a1 += wj * v[j + 2];
                    a2 += wj * v[j + 3];
                    a3 += wj * v[j + 4];
                }
            }
        }
        float* wp = wave + (int64_t)b * w_bs + t;
        if (t + 4 <= hi) {
            // (x's rows are aligned on this path; pre's row is the caller's: a pitch that is no multiple of 4 gets the four values one by one)
            float* pp = pre ? pre + (int64_t)b * p_bs + t : nullptr;
            if (pp && (reinterpret_cast<uintptr_t>(pp) & 15) == 0) *reinterpret_cast<float4*>(pp) = make_float4(a0, a1, a2, a3);
            else if (pp) pp[0] = a0, pp[1] = a1, pp[2] = a2, pp[3] = a3;
            wp[0] = tanhf(a0), wp[1] = tanhf(a1), wp[2] = tanhf(a2), wp[3] = tanhf(a3);
        } else {
            const float av[4] = {a0, a1, a2, a3};
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (t + e < hi) {
                    if (pre) pre[(int64_t)b * p_bs + t + e] = av[e];
                    wp[e] = tanhf(av[e]);
                }
        }
        return;
    }
    for (int u = 0; u < 4; ++u) {
        const int t = t0 + u * 256 + threadIdx.x;
        if (t >= hi) continue;
        float a = 0.f;
        for (int c = 0; c < cin; ++c) {
            const float* xr = xb + (int64_t)c * x_cs;
            for (int j = 0; j < k; ++j) {
                const int tt = t + j - pad;
                float v = (tt >= 0 && tt < len) ? xr[tt] : 0.f;
                v = round_arith(v > 0.f ? v : v * slope, arith);
                a += sm[c * k + j] * v;
            }
        }
        if (pre) pre[(int64_t)b * p_bs + t] = a;
        wave[(int64_t)b * w_bs + t] = tanhf(a);
    }
}

hipError_t launch_conv_post(TensorRef x, const float* w, int cin, int k, float slope, TensorRef pre_tanh, TensorRef wave, const int* lens, int batch, int tmax,
                            hipStream_t s, int emit_lo, const int* emit_hi, int arith) {
    dim3 grid((std::max(tmax - emit_lo, 1) + 1023) / 1024, batch);
    VITS_KLAUNCH(conv_post_kernel, grid, dim3(256), sizeof(float) * cin * k, s, x.p, x.bs, x.cs, w, cin, k, slope, pre_tanh.p, pre_tanh.bs, wave.p, wave.bs,
                       lens, tmax, emit_lo, emit_hi, arith);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// fp32 PCM -> int16 PCM on the device (test/main.cpp:31-33: static_cast<short>(clamp(x, -1, 1) * 32767)), so that the
// multi-GPU gather and the host copy move half the bytes. Pure streaming kernel: 8 samples per thread when both rows
// are 16-byte aligned (2 x dwordx4 in, 1 x dwordx4 out), scalar otherwise.
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ short pcm16_of(float x) { return static_cast<short>(fmaxf(-1.0f, fminf(1.0f, x)) * 32767); }

__global__ __launch_bounds__(256) void pcm16_kernel(const float* src, int64_t s_bs, short* dst, int64_t d_bs, const int64_t* lens, int64_t cols, int vec) {
    const int b = blockIdx.y;
    const int64_t n = lens ? min(lens[b], cols) : cols;
    const float* sr = src + (int64_t)b * s_bs;
    short* dr = dst + (int64_t)b * d_bs;
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i0 >= n) return;
    if (vec && i0 + 8 <= n) {
        const float4 a = *reinterpret_cast<const float4*>(sr + i0), c = *reinterpret_cast<const float4*>(sr + i0 + 4);
        union {
            short h[8];
            int4 v;
        } o;
        o.h[0] = pcm16_of(a.x), o.h[1] = pcm16_of(a.y), o.h[2] = pcm16_of(a.z), o.h[3] = pcm16_of(a.w);
        o.h[4] = pcm16_of(c.x), o.h[5] = pcm16_of(c.y), o.h[6] = pcm16_of(c.z), o.h[7] = pcm16_of(c.w);
        *reinterpret_cast<int4*>(dr + i0) = o.v;
    } else {
        for (int64_t i = i0; i < min(i0 + 8, n); ++i) dr[i] = pcm16_of(sr[i]);
    }
}

hipError_t launch_pcm16(const float* src, int64_t src_stride, int16_t* dst, int64_t dst_stride, const int64_t* lens, int rows, int64_t cols, hipStream_t s) {
    if (rows <= 0 || cols <= 0) return hipSuccess;
    const int vec = (((uintptr_t)src | (uintptr_t)dst) & 15) == 0 && (src_stride & 3) == 0 && (dst_stride & 7) == 0;
    dim3 grid((unsigned)((cols + 2047) / 2048), rows);
    VITS_KLAUNCH(pcm16_kernel, grid, dim3(256), 0, s, src, src_stride, reinterpret_cast<short*>(dst), dst_stride, lens, cols, vec);
    return hipGetLastError();
}

}  // namespace vits
