// stage1_glue.hip — the small kernels between stage one's operators (all HBM/latency-bound; coalesced along time): the embedding gather
// (vits.cpp:262-264), fills, the speaker-bias table, durations and frame counts (vits.cpp:996-1001), prior sampling as a gather (vits.cpp:1028-1063).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/vits.h"
#include "../../include/vits_synth_noise.h"
#include "../../include/vits_exact_math.h"
#include "kernels.h"

namespace vits {

// ---------------------------------------------------------------------------------------------------------
// embedding gather * sqrt(hidden)   (vits.cpp:262-264: ggml_get_rows + ggml_scale)
// ---------------------------------------------------------------------------------------------------------
__global__ void embed_kernel(const int* ids, int id_stride, const int* lens, const float* table, int hidden, float scale, float* x, int64_t bs, int cs,
                             int tmax) {
    const int b = blockIdx.z, c = blockIdx.y;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= tmax) return;
    const int len = lens ? lens[b] : tmax;
    float v = 0.f;
    if (t < len) v = table[(size_t)ids[(size_t)b * id_stride + t] * hidden + c] * scale;
    x[(int64_t)b * bs + (int64_t)c * cs + t] = v;
}

hipError_t launch_embed(const int* ids, int id_stride, const int* lens, const float* table, int hidden, float scale, TensorRef x, int batch, int tmax,
                        hipStream_t s) {
    dim3 grid((tmax + 63) / 64, hidden, batch);
    VITS_KLAUNCH(embed_kernel, grid, dim3(64), 0, s, ids, id_stride, lens, table, hidden, scale, x.p, x.bs, x.cs, tmax);
    return hipGetLastError();
}

__global__ void fill_kernel(float* p, size_t n, float v) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) p[i] = v;
}
hipError_t launch_fill(float* p, size_t n, float v, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const int blocks = (int)std::min<size_t>((n + 255) / 256, 4096);
    VITS_KLAUNCH(fill_kernel, dim3(blocks), dim3(256), 0, s, p, n, v);
    return hipGetLastError();
}

__global__ void fill_rows_kernel(float* x, int64_t bs, int cs, float v, int tmax) {
    const int b = blockIdx.z, c = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= tmax) return;
    x[(int64_t)b * bs + (int64_t)c * cs + t] = v;
}
hipError_t launch_fill_rows(TensorRef x, int channels, float v, int batch, int tmax, hipStream_t s) {
    dim3 grid((tmax + 255) / 256, channels, batch);
    VITS_KLAUNCH(fill_rows_kernel, grid, dim3(256), 0, s, x.p, x.bs, x.cs, v, tmax);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// Effective-bias table of a multi-speaker model (built once at load; transformers modeling_vits.py: the speaker terms of
// VitsStochasticDurationPredictor.forward, VitsWaveNet.forward and VitsHifiGan.forward are per-utterance constants over time).
// Thread = (table row r, channel c) of one segment: row 0 (speaker -1) is the plain bias, row 1 + s is
// bias[c] + (sum_e cond_w[c][e] * emb[s][e] + cond_b[c]) — the 1x1 conditioning conv of g = emb[s], products summed in e order.
__global__ void speaker_bias_kernel(const float* __restrict__ bias, const float* __restrict__ cw, const float* __restrict__ cb, const float* __restrict__ emb,
                                    int n, int E, float* __restrict__ table, int64_t rs) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (c >= n) return;
    float v = bias[c];
    if (r > 0) {
        const float* g = emb + (int64_t)(r - 1) * E;
        const float* w = cw + (int64_t)c * E;
        float acc = 0.f;
        for (int e = 0; e < E; ++e) acc = fmaf(w[e], g[e], acc);
        v = v + (acc + cb[c]);
    }
    table[(int64_t)r * rs + c] = v;
}
hipError_t launch_speaker_bias(const float* bias, const float* cond_w, const float* cond_b, const float* emb, int n, int E, int n_spk, float* table,
                               int64_t row_stride, hipStream_t s) {
    if (n <= 0 || E <= 0 || n_spk < 1 || !bias || !cond_w || !cond_b || !emb || !table) return hipErrorInvalidValue;
    hipLaunchKernelGGL(speaker_bias_kernel, dim3((n + 255) / 256, n_spk + 1), dim3(256), 0, s, bias, cond_w, cond_b, emb, n, E, table, row_stride);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// durations: d = ceil(exp(logw) * length_scale) (vits.cpp:996), per-utterance inclusive cumsum (:1001),
// frames L = max(1, sum) (:999-1000,1133) and the per-stage vocoder lengths. One block per utterance.
// Per-utterance prosody (optional device arrays): length_scales[b] replaces length_scale; ovr[b][t] >= 0 replaces the token's duration
// before the sum, the cumulative sum and the dur write (ovr rows have the stride of dur, tmax).
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void durations_kernel(const float* logw, int64_t l_bs, int l_cs, int c, const int* lens, int tmax, float length_scale,
                                                        const float* length_scales, const int* ovr, int fixed, float* dur, int* cum, int* frames,
                                                        int* stage_lens, int n_stage, const int* stage_mul, const int* stage_add, int batch, int exact) {
    __shared__ int part[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int len = lens ? lens[b] : tmax;
    const int per = (tmax + 255) / 256;
    const int beg = tid * per, end = min(beg + per, len);
    const float ls = length_scales ? length_scales[b] : length_scale;
    int s = 0;
    for (int t = beg; t < end; ++t) {
        const float lw = logw[(int64_t)b * l_bs + (int64_t)c * l_cs + t];
        // exact: the emulated-ggml mode — exp as the fixed polynomial both sides share (include/vits_exact_math.h) instead of the device library's
        float d = exact ? vx_duration(lw, ls) : ceilf(expf(lw) * ls);
        if (ovr) {
            const int v = ovr[(int64_t)b * tmax + t];
            if (v >= 0) d = (float)v;
        }
        if (fixed > 0) d = (float)fixed;
        dur[(int64_t)b * tmax + t] = d;
        s += (int)d;
    }
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < 256; ++i) {
            const int v = part[i];
            part[i] = run;
            run += v;
        }
        const int L = max(1, run);
        frames[b] = L;
        for (int st = 0; st < n_stage; ++st) stage_lens[st * batch + b] = L * stage_mul[st] + stage_add[st];
    }
    __syncthreads();
    int run = part[tid];
    for (int t = beg; t < end; ++t) {
        run += (int)dur[(int64_t)b * tmax + t];
        cum[(int64_t)b * tmax + t] = run;
    }
    for (int t = max(beg, len); t < min(beg + per, tmax); ++t) {
        dur[(int64_t)b * tmax + t] = 0.f;
        cum[(int64_t)b * tmax + t] = 0x7fffffff;
    }
}

hipError_t launch_durations(TensorRef logw, int c, const int* lens, int batch, int tmax, float length_scale, const float* length_scales, const int* ovr, int fixed,
                            float* dur, int* cum, int* frames, int* stage_lens, int n_stage, const int* stage_mul, const int* stage_add, hipStream_t s, bool exact) {
    VITS_KLAUNCH(durations_kernel, dim3(batch), dim3(256), 0, s, logw.p, logw.bs, logw.cs, c, lens, tmax, length_scale, length_scales, ovr, fixed, dur, cum, frames,
                       stage_lens, n_stage, stage_mul, stage_add, batch, exact ? 1 : 0);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// prior sampling through the monotonic alignment, as a GATHER:
//   a(j) = min{ i : j < cum_i };  z_p[c][j] = mean[c][a(j)] + eps[c][j] * exp(logvar[c][a(j)]) * noise_scale
// replaces the dense [L,T] one-hot matrix + two mul_mat (vits.cpp:1028-1057) and :1059-1063.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void zp_kernel(const float* mean, int64_t m_bs, int m_cs, const float* logvar, int64_t v_bs, int v_cs, const int* cum,
                                                 int cum_stride, const int* tok_lens, const int* frames, const float* noise, int64_t n_bs, int n_cs,
                                                 int noise_kind, uint64_t seed, const int* seed_off, float noise_scale, const float* noise_scales, float* zp, int64_t z_bs,
                                                 int z_cs, int channels, int tmax_tok) {
    __shared__ int tok[256];
    const int b = blockIdx.y, j0 = blockIdx.x * 256, tid = threadIdx.x;
    const int L = frames[b];
    if (j0 >= L) return;
    const int T = tok_lens ? tok_lens[b] : tmax_tok;
    const int j = j0 + tid;
    {
        // binary search: first i with cum[i] > j
        const int* cb = cum + (int64_t)b * cum_stride;
        int lo = 0, hi = T;  // answer in [0, T]
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cb[mid] > j) hi = mid;
            else lo = mid + 1;
        }
        tok[tid] = lo < T ? lo : -1;
    }
    __syncthreads();
    if (j >= L) return;
    const int a = tok[tid];
    const float ns = noise_scales ? noise_scales[b] : noise_scale;  // (per-utterance prosody; b = blockIdx.y)
    // channels are split over blockIdx.z (every element is independent): one block per 256 frames walked all 192 channels
    // serially through the counter-based normal, 100 us at batch 1
    const int cpb = (channels + gridDim.z - 1) / gridDim.z;
    const int c_end = min(channels, (int)(blockIdx.z + 1) * cpb);
    for (int c = blockIdx.z * cpb; c < c_end; ++c) {
        const float mu = a >= 0 ? mean[(int64_t)b * m_bs + (int64_t)c * m_cs + a] : 0.f;
        const float lv = a >= 0 ? logvar[(int64_t)b * v_bs + (int64_t)c * v_cs + a] : 0.f;
        float e;
        if (noise_kind == VITS_NOISE_COUNTER) e = vits_counter_normal(seed + (uint64_t)(seed_off ? seed_off[b] : b), VITS_STREAM_NOISE_PRIOR, (uint64_t)c * L + j);
        else e = noise[(int64_t)b * n_bs + (int64_t)c * n_cs + j];
        float n = e * expf(lv);  // vits.cpp:1060
        n = n * ns;              // :1061
        zp[(int64_t)b * z_bs + (int64_t)c * z_cs + j] = mu + n;
    }
}

hipError_t launch_zp(TensorRef mean, TensorRef logvar, const int* cum, int cum_stride, const int* tok_lens, const int* frames, TensorRef noise, int noise_kind,
                     uint64_t seed, const int* seed_off, float noise_scale, const float* noise_scales, TensorRef zp, int batch, int channels, int lmax, hipStream_t s) {
    dim3 grid((lmax + 255) / 256, batch, 16);
    VITS_KLAUNCH(zp_kernel, grid, dim3(256), 0, s, mean.p, mean.bs, mean.cs, logvar.p, logvar.bs, logvar.cs, cum, cum_stride, tok_lens, frames, noise.p,
                       noise.bs, noise.cs, noise_kind, seed, seed_off, noise_scale, noise_scales, zp.p, zp.bs, zp.cs, channels, cum_stride);
    return hipGetLastError();
}

}  // namespace vits
