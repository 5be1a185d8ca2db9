// layer_norm.hip — LayerNorm over the channels of x + res, optionally gelu, optionally added into another tensor: the encoder's four-node norm
// (vits.cpp:365-372, 412-418) and the second norm of a DDS layer (vits.cpp:679-688) as one kernel.
#include <hip/hip_runtime.h>

#include "kernel_common.h"
#include "kernels.h"

namespace vits {

// ---------------------------------------------------------------------------------------------------------
// y = LayerNorm_channels(x + res) [optionally gelu, optionally add_to += y]
//   encoder: vits.cpp:365-372, 412-418 (ggml_add + ggml_norm + mul + add = 4 nodes)
//   DDS:     vits.cpp:679-688 (permute, cont, norm, permute, cont, gelu, add)
// Block = 64 time steps x all channels; the tile is held in LDS so x is read from HBM once.
// ---------------------------------------------------------------------------------------------------------

// channel groups per block of the two LayerNorm kernels: 16 x 64 threads, every thread walks channels/16 rows. (4 groups
// made each thread chain 48 dependent loads: 26-58 us per launch at batch 1, where these launches have 2 blocks.) The
// partial sums are combined in a fixed order, so results do not depend on the batch.
constexpr int LN_GROUPS = kLnGroups;  // (launch_plan.h)

template <int TW>
__global__ __launch_bounds__(TW * LN_GROUPS) void add_layer_norm_kernel(const float* x, int64_t x_bs, int x_cs, const float* res, int64_t r_bs, int r_cs,
                                                             const float* gamma, const float* beta, float* y, int64_t y_bs, int y_cs, float* addto,
                                                             int64_t a_bs, int a_cs, const int* lens, int channels, int tmax, float eps, int post_gelu, const uint16_t* gelu_tab) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* tile = sm;                    // [channels][TW]
    float* red = sm + channels * TW;     // [LN_GROUPS][TW] x2
    const int b = blockIdx.y, t0 = blockIdx.x * TW;
    const int len = lens ? lens[b] : tmax;
    if (t0 >= len) return;
    const int tl = threadIdx.x % TW, g = threadIdx.x / TW;
    const int t = t0 + tl;
    const bool ok = t < len;
    float s = 0.f;
    // (twelve channels per step, their loads issued before the first LDS store: a load -> store loop exposes one memory latency per
    // channel, and at batch 1 a launch has two blocks. Same values, same order of s.)
    constexpr int UB = 12;
    for (int c0 = g; c0 < channels; c0 += UB * LN_GROUPS) {
        float xv[UB], rv[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const int c = c0 + u * LN_GROUPS;
            const bool live = ok && c < channels;
            xv[u] = live ? x[(int64_t)b * x_bs + (int64_t)c * x_cs + t] : 0.f;
            rv[u] = (live && res) ? res[(int64_t)b * r_bs + (int64_t)c * r_cs + t] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const int c = c0 + u * LN_GROUPS;
            if (c >= channels) continue;
            float v = 0.f;
            if (ok) {
                v = xv[u];
                if (res) v += rv[u];
            }
            tile[c * TW + tl] = v;
            s += v;
        }
    }
    red[g * TW + tl] = s;
    __syncthreads();
    float msum = 0.f;
#pragma unroll
    for (int q = 0; q < LN_GROUPS; ++q) msum += red[q * TW + tl];
    const float mean = msum / (float)channels;
    float vs = 0.f;
    for (int c = g; c < channels; c += LN_GROUPS) {
        const float d = tile[c * TW + tl] - mean;
        vs += d * d;
    }
    red[(LN_GROUPS + g) * TW + tl] = vs;
    __syncthreads();
    float vsum = 0.f;
#pragma unroll
    for (int q = 0; q < LN_GROUPS; ++q) vsum += red[(LN_GROUPS + q) * TW + tl];
    const float var = vsum / (float)channels;
    const float inv = 1.0f / sqrtf(var + eps);
    if (!ok) return;
    for (int c = g; c < channels; c += LN_GROUPS) {
        float v = (tile[c * TW + tl] - mean) * inv * gamma[c] + beta[c];
        if (post_gelu) v = gelu_op(v, gelu_tab);
        if (addto) {
            float* a = addto + (int64_t)b * a_bs + (int64_t)c * a_cs + t;
            *a = *a + v;
        } else
            y[(int64_t)b * y_bs + (int64_t)c * y_cs + t] = v;
    }
}

hipError_t launch_add_layer_norm(TensorRef x, TensorRef res, const float* gamma, const float* beta, TensorRef y, const int* lens, int batch, int channels,
                                 int tmax, float eps, int post_gelu, TensorRef add_to, hipStream_t s, GgmlTables tabs, int force_tw) {
    const LayerNormPlan l = plan_add_layer_norm(channels, batch, tmax, force_tw);
    if (!l.ok) return hipErrorInvalidValue;
    const dim3 grid(l.gx, l.gy), block(l.block);
#define VITS_LN_LAUNCH(TW)                                                                                                                                \
    return launch_lds<&add_layer_norm_kernel<TW>>(grid, block, l.lds, s, x.p, x.bs, x.cs, res.p, res.bs, res.cs, gamma, beta, y.p, y.bs, y.cs, add_to.p, add_to.bs, add_to.cs, lens, \
                                                  channels, tmax, eps, post_gelu, tabs.gelu)
    if (l.tw == 32) VITS_LN_LAUNCH(32);
    else VITS_LN_LAUNCH(64);
#undef VITS_LN_LAUNCH
}

}  // namespace vits
