// spline.hip — the element-wise part of the duration predictor's flows: the inverse rational-quadratic spline (vits.cpp:804-852 + :695-802), the
// element-wise affine (vits.cpp:901-925), the duration latents (vits.cpp:948-949) and the per-utterance row scale.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/vits.h"
#include "../../include/vits_synth_noise.h"
#include "kernel_common.h"
#include "kernels.h"

namespace vits {

// ---------------------------------------------------------------------------------------------------------
// Inverse rational-quadratic spline on latent row zc (unconstrained_rational_quadratic_spline, vits.cpp:804-852 + :695-802;
// HF modeling_vits.py:139-163,211-302). u = conv_proj output [3*bins-1][T]. One block per utterance, one thread per token (tokens
// beyond 512 loop).
//   VITS_MODE_HF: identity outside [-B, B], the spline inside (HF:143-151).
//   VITS_MODE_REFERENCE: Q3 (:720), on the LAST token Q4 (ggml-util.h:235-236,252-253), and the masked get / set pair of :832-849
//   LITERALLY (Q6): tensor_masked_get keeps the shape (custom-ops.h:746-749) while tensor_masked_set consumes its values sequentially
//   (custom-ops.h:836-850). Every token goes through the spline — an outside token as input 0 with zeroed widths / heights / padded
//   derivatives (:834-840) —, the k-th INSIDE token receives the result of token k, and the j-th OUTSIDE token receives element j of
//   [x_t if inside_t else 0]. While every latent of the utterance lies inside (all 8,192 ids of the benchmark batch) that is the identity
//   permutation and each token keeps its own spline output: the block only pays one __syncthreads_or for it.
// ---------------------------------------------------------------------------------------------------------
constexpr int MAX_BINS = 16;

__device__ __forceinline__ float softplus_f(float x) { return x > 20.f ? x : (float)log(1.0 + exp((double)x)); }  // custom-ops.h:872-879

// rational_quadratic_spline (vits.cpp:695-802) on one token's row; masked: the row's parameters were zeroed by :837-840
// ggml_soft_max over the bins (vits.cpp:719,735), in place: fp32 by default, ggml's fp16 exp table + double sum when exp_tab is given (Q8)
template <bool TAB>
__device__ __forceinline__ void spline_softmax(float* v, int nb, const uint16_t* exp_tab) {
    float mx = -INFINITY;
    for (int i = 0; i < nb; ++i) mx = fmaxf(mx, v[i]);
    if constexpr (TAB) {
        double sum = 0.0;
        for (int i = 0; i < nb; ++i) {
            v[i] = ggml_table_lookup(exp_tab, v[i] - mx);
            sum += (double)v[i];
        }
        const float inv = (float)(1.0 / sum);
        for (int i = 0; i < nb; ++i) v[i] *= inv;
        return;
    }
    float sum = 0.f;
    for (int i = 0; i < nb; ++i) {
        v[i] = expf(v[i] - mx);
        sum += v[i];
    }
    for (int i = 0; i < nb; ++i) v[i] /= sum;
}

template <bool TAB>
__device__ __forceinline__ float spline_row(float x, const float* ub, int u_cs, int nb, float B, float inv_sqrt, int mode, bool q4, bool masked, const uint16_t* exp_tab) {
    const float min_w = 1e-3f, min_h = 1e-3f, min_d = 1e-3f;
    float W[MAX_BINS], H[MAX_BINS], cw[MAX_BINS + 1], ch[MAX_BINS + 1];
    // widths
    {
        for (int i = 0; i < nb; ++i) W[i] = masked ? 0.f : ub[(int64_t)i * u_cs] * inv_sqrt;
        spline_softmax<TAB>(W, nb, exp_tab);
        if (mode == VITS_MODE_REFERENCE) {
            const float sc = min_w + (1 - min_w * nb);  // Q3
            for (int i = 0; i < nb; ++i) W[i] = W[i] * sc;
        } else {
            for (int i = 0; i < nb; ++i) W[i] = min_w + (1 - min_w * nb) * W[i];
        }
        float cum = 0.f;
        cw[0] = 0.f;
        for (int i = 0; i < nb; ++i) {
            cum += W[i];
            cw[i + 1] = cum;
        }
        for (int i = 0; i <= nb; ++i) cw[i] = (B - (-B)) * cw[i] + (-B);
        cw[0] = -B;
        if (!q4) cw[nb] = B;
        for (int i = 0; i < nb; ++i) W[i] = cw[i + 1] - cw[i];
    }
    {
        for (int i = 0; i < nb; ++i) H[i] = masked ? 0.f : ub[(int64_t)(nb + i) * u_cs] * inv_sqrt;
        spline_softmax<TAB>(H, nb, exp_tab);
        for (int i = 0; i < nb; ++i) H[i] = min_h + (1 - min_h * nb) * H[i];
        float cum = 0.f;
        ch[0] = 0.f;
        for (int i = 0; i < nb; ++i) {
            cum += H[i];
            ch[i + 1] = cum;
        }
        for (int i = 0; i <= nb; ++i) ch[i] = (B - (-B)) * ch[i] + (-B);
        ch[0] = -B;
        if (!q4) ch[nb] = B;
        for (int i = 0; i < nb; ++i) H[i] = ch[i + 1] - ch[i];
    }
    int bin = -1;
    for (int i = 0; i <= nb; ++i) {
        float loc = ch[i];
        if (i == nb && !q4) loc += 1e-6f;
        if (x >= loc) bin++;
    }
    bin = min(max(bin, 0), nb - 1);
    const float constant = (float)log(exp(1.0 - (double)min_d) - 1.0);
    auto deriv = [&](int i) -> float {
        float ud;
        if (masked) ud = 0.f;  // (the constants of :829-830 are zeroed by the mask as well, :840)
        else if (i == 0) ud = constant;
        else if (i == nb) ud = q4 ? 0.f : constant;
        else ud = ub[(int64_t)(2 * nb + i - 1) * u_cs];
        return min_d + softplus_f(ud);
    };
    float in_cw = 0.f, in_w = 1.f, in_ch = 0.f, in_h = 1.f;
    for (int i = 0; i < nb; ++i)  // register arrays: select without dynamic indexing
        if (i == bin) {
            in_cw = cw[i];
            in_w = W[i];
            in_ch = ch[i];
            in_h = H[i];
        }
    const float d0 = deriv(bin), d1 = deriv(bin + 1);
    const float delta = in_h / in_w;
    const float i1 = d0 + d1 - 2 * delta;
    const float i2 = x - in_ch;
    const float i3 = i2 * i1;
    const float a = in_h * (delta - d0) + i3;
    const float bq = in_h * d0 - i3;
    const float cc = -delta * i2;
    const float disc = bq * bq - 4 * a * cc;
    const float root = (2 * cc) / (-bq - sqrtf(disc));
    return root * in_w + in_cw;
}

// (TAB: the emulated-ggml soft-max is a separate build, so that the default one carries no table code)
template <int NT, bool TAB>
__global__ __launch_bounds__(NT) void spline_kernel(const float* u, int64_t u_bs, int u_cs, float* z, int64_t z_bs, int z_cs, int zc, const int* lens, int tmax,
                                                      int nb, float B, float inv_sqrt, int mode, const uint16_t* exp_tab) {
    extern __shared__ float spline_lds[];  // [3][tpad]: masked input, spline result, inside flag of every token of the utterance; then [3 nb - 1][blockDim] parameters
    const int b = blockIdx.x;
    const int len = lens ? lens[b] : tmax;
    const int tpad = (tmax + 63) & ~63;
    float* s_val = spline_lds;
    float* s_res = spline_lds + tpad;
    int* s_in = reinterpret_cast<int*>(spline_lds + 2 * tpad);
    float* s_u = spline_lds + 3 * tpad;  // the parameters of the block's current chunk of tokens, [3 nb - 1][nthr]
    float* zrow = z + (int64_t)b * z_bs + (int64_t)zc * z_cs;
    const bool ref = mode == VITS_MODE_REFERENCE;
    int any_outside = 0;
    // A token's 3 nb - 1 parameters are 3 nb - 1 rows of u, one cache line each per token: read through the pointer inside spline_row they were four
    // dependent rounds of strided loads (16 us per launch at 128 tokens, most of it memory latency). The block stages them chunk by chunk with
    // coalesced loads, all rows in flight at once; the values — and every operation on them — are the same.
    const int nthr = (int)blockDim.x, nrow = 3 * nb - 1;
    for (int c0 = 0; c0 < len; c0 += nthr) {
        const int t = c0 + (int)threadIdx.x;
        {
            const float* ub = u + (int64_t)b * u_bs + (t < len ? t : len - 1);
            float v[3 * MAX_BINS - 1];
#pragma unroll
            for (int r = 0; r < 3 * MAX_BINS - 1; ++r) v[r] = r < nrow ? ub[(int64_t)r * u_cs] : 0.f;
#pragma unroll
            for (int r = 0; r < 3 * MAX_BINS - 1; ++r)
                if (r < nrow) s_u[r * nthr + threadIdx.x] = v[r];
        }
        // (each thread reads back only what it wrote: no barrier needed)
        if (t < len) {
            const float x = zrow[t];
            const bool inside = x >= -B && x <= B;
            const float* ub = s_u + threadIdx.x;
            float r = x;  // HF: identity outside the interval (HF:143-151)
            if (inside || ref) r = spline_row<TAB>(inside ? x : 0.f, ub, nthr, nb, B, inv_sqrt, mode, ref && t == len - 1, !inside, exp_tab);
            if (ref) {
                s_val[t] = inside ? x : 0.f;  // tensor_masked_get(inputs, inside_interval_mask): the shape is kept
                s_res[t] = r;
                s_in[t] = inside ? 1 : 0;
                any_outside |= inside ? 0 : 1;
            } else {
                zrow[t] = r;
            }
        }
    }
    if (!ref) return;
    if (!__syncthreads_or(any_outside)) {
        // every latent inside: both masked_set calls are the identity permutation
        for (int t = threadIdx.x; t < len; t += blockDim.x) zrow[t] = s_res[t];
        return;
    }
    // Q6: the j-th outside token takes element j of the masked input (:832), the k-th inside token the result of token k (:849).
    // nout(t) = outside tokens before t: every thread counts a contiguous chunk, one thread scans the per-thread counts (the
    // first version let every thread count from token 0: O(T^2) LDS reads per utterance)
    __shared__ int s_part[NT];
    const int per = (len + nthr - 1) / nthr;
    const int beg = min((int)threadIdx.x * per, len), end = min(beg + per, len);
    int cnt = 0;
    for (int t = beg; t < end; ++t) cnt += 1 - s_in[t];
    s_part[threadIdx.x] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int i = 0; i < nthr; ++i) {
            const int v = s_part[i];
            s_part[i] = run;
            run += v;
        }
    }
    __syncthreads();
    int nout = s_part[threadIdx.x];
    for (int t = beg; t < end; ++t) {
        zrow[t] = s_in[t] ? s_res[t - nout] : s_val[nout];
        nout += 1 - s_in[t];
    }
}

hipError_t launch_spline(TensorRef u, TensorRef z, int zc, const int* lens, int batch, int tmax, int bins, float tail, float inv_sqrt, int mode, hipStream_t s,
                         GgmlTables tabs) {
    if (bins > MAX_BINS || tmax > 4096) return hipErrorInvalidValue;
    const int tpad = (tmax + 63) & ~63;
    // 512 threads: one token per thread up to 512 tokens, two rounds for 1024-id inputs (a 1024-thread build is capped at 128 VGPRs and spills
    // the bin arrays: 74 us per launch against 32 at 8 x 1024 ids)
#define VITS_SPLINE_LAUNCH(NT, TAB)                                                                                                                 \
    do {                                                                                                                                            \
        const size_t lds_ = ((size_t)3 * tpad + (size_t)(3 * bins - 1) * (tpad < NT ? tpad : NT)) * sizeof(float);                                  \
        /* (152 KB: + the kernel's static s_part) */                                                                                                \
        return launch_lds<&spline_kernel<NT, TAB>, 152 * 1024>(dim3(batch), dim3(tpad < NT ? tpad : NT), lds_, s, u.p, u.bs, u.cs, z.p, z.bs, z.cs, zc, lens, tmax, bins, tail, \
                                                               inv_sqrt, mode, tabs.exp);                                                           \
    } while (0)
    if (tabs.exp) {
        VITS_SPLINE_LAUNCH(512, true);
    } else {
        VITS_SPLINE_LAUNCH(512, false);
    }
#undef VITS_SPLINE_LAUNCH
}

// elementwise affine, reverse (vits.cpp:901-925; Q5 sign): logical channel ch lives in physical row (c_first ? 1-ch : ch)
__global__ void affine_kernel(float* z, int64_t z_bs, int z_cs, int c_first, const float* translate, const float* log_scale, int sign, const int* lens,
                              int tmax) {
    const int b = blockIdx.z, ch = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
    const int len = lens ? lens[b] : tmax;
    if (t >= len) return;
    const int row = c_first ? 1 - ch : ch;
    float* p = z + (int64_t)b * z_bs + (int64_t)row * z_cs + t;
    *p = (*p - translate[ch]) * expf(sign > 0 ? log_scale[ch] : -log_scale[ch]);
}
hipError_t launch_affine(TensorRef z, int c_first, const float* translate, const float* log_scale, int sign, const int* lens, int batch, int tmax,
                         hipStream_t s) {
    dim3 grid((tmax + 63) / 64, 2, batch);
    VITS_KLAUNCH(affine_kernel, grid, dim3(64), 0, s, z.p, z.bs, z.cs, c_first, translate, log_scale, sign, lens, tmax);
    return hipGetLastError();
}

// duration latents: z[c][t] = N(0,1) * noise_scale_duration (vits.cpp:948-949), counter-based stream. scales (optional, device [B]): the
// scale of utterance b instead of `scale` (per-utterance prosody); the draw itself does not depend on it
__global__ void noise_dur_kernel(float* z, int64_t z_bs, int z_cs, const int* lens, int tmax, uint64_t seed, const int* seed_off, float scale, const float* scales) {
    const int b = blockIdx.z, c = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
    const int len = lens ? lens[b] : tmax;
    if (t >= len) return;
    const float sc = scales ? scales[b] : scale;  // (b = blockIdx.z: one value per block)
    z[(int64_t)b * z_bs + (int64_t)c * z_cs + t] = vits_counter_normal(seed + (uint64_t)(seed_off ? seed_off[b] : b), VITS_STREAM_NOISE_DUR, (uint64_t)c * len + t) * sc;
}
hipError_t launch_noise_dur(TensorRef z, const int* lens, int batch, int tmax, uint64_t seed, const int* seed_off, float scale, const float* scales, hipStream_t s) {
    dim3 grid((tmax + 63) / 64, 2, batch);
    VITS_KLAUNCH(noise_dur_kernel, grid, dim3(64), 0, s, z.p, z.bs, z.cs, lens, tmax, seed, seed_off, scale, scales);
    return hipGetLastError();
}

__global__ void scale_rows_kernel(float* x, int64_t bs, int cs, float scale, const float* scales, int tmax) {
    const int b = blockIdx.z, c = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= tmax) return;
    x[(int64_t)b * bs + (int64_t)c * cs + t] *= scales ? scales[b] : scale;
}
hipError_t launch_scale_rows(TensorRef x, int channels, float scale, const float* scales, int batch, int tmax, hipStream_t s) {
    dim3 grid((tmax + 63) / 64, channels, batch);
    VITS_KLAUNCH(scale_rows_kernel, grid, dim3(64), 0, s, x.p, x.bs, x.cs, scale, scales, tmax);
    return hipGetLastError();
}

}  // namespace vits
