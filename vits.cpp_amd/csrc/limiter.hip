// limiter.hip — the loudness target under a ceiling: a 4x true-peak meter and a look-ahead limiter on a ragged batch of PCM rows (include/vits.h
// vits_model_set_limiter / vits_op_limit; DESIGN.md §8 "Under a ceiling"). The definition is stated in kernels.h (LimitCall); the constants come from
// limiter_host.cpp. Nothing in it is a recurrence, so every kernel is a tile of kLimitTile = 2048 consecutive samples of ONE row with a halo:
//   limit_meter_kernel<true>   x tile + 36 samples either side in LDS; a thread runs the four phase chains of a sample (the chain of resample.hip: acc = 0,
//                              acc = fmaf(h[k][p], x[n - R + k], acc), k ascending) and keeps c[n] = max(|x[n]|, |u[4n .. 4n+2]|) and d[n] = max(|u[4n+2]|,
//                              |u[4n+3]|); e[n] = max(c[n], d[n - 1]) goes to the scratch, the tile's maximum to tmax. u itself is never stored.
//   limit_gain_kernel          one block per row: TP = max of the tile maxima (a fixed-shape tree), g0 by the call's kind -> levels[b][2], limits[b][0]
//   limit_apply_kernel         r over [t0 - A - H, t0 + T + A) in LDS, the sliding minimum over H + A + 1 by doubling (P_2h[i] = min(P_h[i], P_h[i + h]),
//                              then min(P_h[i], P_h[i + W - h])), the mean over A + 1 in fp64 ascending, y = x (g0 s); min s and the count of s < 1 per tile
//   limit_meter_kernel<false>  the same meter over y: tile maxima only (no envelope, so no sample before the tile)
//   limit_final_kernel         one block per row: TP(y), min s, share -> limits[b][1 .. 3]
// Tiles are anchored at the row's own sample 0, only [0, len) is loaded, and only maxima, minima and integer counts cross a tile: batch position, grid and
// stream enter no bit. At a given tap the four phases' coefficients are the same for every lane: the table is read through scalar loads.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/vits.h"
#include "kernel_common.h"
#include "kernels.h"

namespace vits {

constexpr int LM_THREADS = 256, LM_TILE = kLimitTile, LM_SPT = LM_TILE / LM_THREADS;
constexpr int LM_R = 35, LM_K = 2 * LM_R + 1;
constexpr int LM_XS = LM_TILE + 1 + 2 * LM_R;                    // staged samples [t0 - 1 - R, t0 + T + R)
constexpr int LM_SPAN = LM_TILE + kLimitMaxH + 2 * kLimitMaxA;  // r over [t0 - A - H, t0 + T + A) at 48 kHz
static_assert(LM_TILE % LM_THREADS == 0 && 2 * LM_SPAN * 4 <= 64 * 1024, "two buffers of r fit the static LDS of a block");

// fixed-shape trees over the block; every thread gets the result
__device__ __forceinline__ float lm_block_max(float v, float* red, int tid) {
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int w = LM_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) red[tid] = fmaxf(red[tid], red[tid + w]);
        __syncthreads();
    }
    return red[0];
}
__device__ __forceinline__ float lm_block_min(float v, float* red, int tid) { return -lm_block_max(-v, red, tid); }
// (exact: the terms are counts of at most kLimitTile samples, and a row has fewer than 2^31 samples; summed as integers)
__device__ __forceinline__ int lm_block_sum(int v, int* red, int tid) {
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int w = LM_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    return red[0];
}

// ENV: e[n] of the tile -> env; both: the maximum of |x| and |u| over the tile -> tmax[b][t]
template <bool ENV>
__global__ __launch_bounds__(LM_THREADS) void limit_meter_kernel(const float* __restrict__ x, int64_t x_stride, const int* __restrict__ lens, int64_t n_cap,
                                                                 const float* __restrict__ taps, float* __restrict__ env, int64_t env_stride,
                                                                 float* __restrict__ tmax, int tiles) {
    __shared__ float xs[LM_XS + 3];
    __shared__ float ds[LM_TILE + 1];  // d of samples t0 - 1 .. t0 + T - 1
    __shared__ float red[LM_THREADS];
    const int b = (int)(blockIdx.x / (unsigned)tiles), t = (int)(blockIdx.x % (unsigned)tiles), tid = (int)threadIdx.x;
    const int64_t N = min((int64_t)max(lens[b], 0), n_cap);
    const int64_t t0 = (int64_t)t * LM_TILE;
    if (t0 >= N) return;  // (block-uniform)
    const float* xr = x + (int64_t)b * x_stride;
    const int64_t base = t0 - 1 - LM_R;
    for (int i = tid; i < LM_XS; i += LM_THREADS) {
        const int64_t idx = base + i;
        xs[i] = (idx >= 0 && idx < N) ? xr[idx] : 0.f;
    }
    __syncthreads();
    const int cnt = (int)min((int64_t)LM_TILE, N - t0);
    float cv[LM_SPT];
    float mx = 0.f;
#pragma unroll
    for (int it = 0; it < LM_SPT; ++it) {
        // (a thread past the row's end runs the chains of the tile's last sample: the tap loop stays free of tests)
        const int o = min(tid + it * LM_THREADS, cnt - 1);
        const float* xp = xs + o + 1;  // x[n - R], n = t0 + o
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 4
        for (int k = 0; k < LM_K; ++k) {
            const float xv = xp[k];
            a0 = fmaf(taps[k * 4 + 0], xv, a0);
            a1 = fmaf(taps[k * 4 + 1], xv, a1);
            a2 = fmaf(taps[k * 4 + 2], xv, a2);
            a3 = fmaf(taps[k * 4 + 3], xv, a3);
        }
        const float c = fmaxf(fmaxf(fabsf(xp[LM_R]), fabsf(a0)), fmaxf(fabsf(a1), fabsf(a2)));
        const float d = fmaxf(fabsf(a2), fabsf(a3));
        cv[it] = c;
        mx = fmaxf(mx, fmaxf(c, d));
        if (ENV && tid + it * LM_THREADS < cnt) ds[o + 1] = d;
    }
    if constexpr (ENV) {
        if (tid == 0) {
            // the two phases of the sample before the tile that reach into its first envelope value
            float d = 0.f;
            if (t0 > 0) {
                float a2 = 0.f, a3 = 0.f;
                for (int k = 0; k < LM_K; ++k) {
                    a2 = fmaf(taps[k * 4 + 2], xs[k], a2);
                    a3 = fmaf(taps[k * 4 + 3], xs[k], a3);
                }
                d = fmaxf(fabsf(a2), fabsf(a3));
            }
            ds[0] = d;
        }
        __syncthreads();
        float* er = env + (int64_t)b * env_stride + t0;
#pragma unroll
        for (int it = 0; it < LM_SPT; ++it) {
            const int o = tid + it * LM_THREADS;
            if (o < cnt) er[o] = fmaxf(cv[it], ds[o]);
        }
    }
    mx = lm_block_max(mx, red, tid);
    if (tid == 0) tmax[(int64_t)b * tiles + t] = mx;
}

// TP(x) and the gain before limiting of every row
__global__ __launch_bounds__(LM_THREADS) void limit_gain_kernel(const int* __restrict__ lens, int64_t n_cap, const float* __restrict__ tmax, int tiles, int kind,
                                                                float value_db, float gain, float* __restrict__ levels, float* __restrict__ limits) {
    __shared__ float red[LM_THREADS];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int64_t N = min((int64_t)max(lens[b], 0), n_cap);
    const int nt = (int)((N + LM_TILE - 1) / LM_TILE);
    float m = 0.f;
    for (int i = tid; i < nt; i += LM_THREADS) m = fmaxf(m, tmax[(int64_t)b * tiles + i]);
    m = lm_block_max(m, red, tid);
    if (tid == 0) {
        float* row = levels + (int64_t)b * 4;
        const float tp = fmaxf(m, row[1]);  // (the tile maxima contain |x| already: the sample peak cannot be larger)
        // from the values as they are reported (fp32 L and TP), as level_finish_kernel does
        float g = 1.f;
        if (kind == VITS_LEVEL_GAIN) g = gain;
        else if (kind == VITS_LEVEL_PEAK) {
            if (tp > 0.f) g = (float)(pow(10.0, (double)value_db / 20.0) / (double)tp);
        } else if (row[3] > 0.f) g = (float)pow(10.0, ((double)value_db - (double)row[0]) / 20.0);
        row[2] = g;
        float* lr = limits + (int64_t)b * 4;
        lr[0] = tp, lr[1] = 0.f, lr[2] = 1.f, lr[3] = 0.f;
    }
}

__global__ __launch_bounds__(LM_THREADS) void limit_apply_kernel(const float* __restrict__ x, int64_t x_stride, float* __restrict__ y, int64_t y_stride,
                                                                 const int* __restrict__ lens, int64_t n_cap, const float* __restrict__ env, int64_t env_stride,
                                                                 const float* __restrict__ levels, float c, int A, int H, float* __restrict__ tstat, int tiles) {
    __shared__ float buf[2][LM_SPAN];
    __shared__ float red[LM_THREADS];
    const int b = (int)(blockIdx.x / (unsigned)tiles), t = (int)(blockIdx.x % (unsigned)tiles), tid = (int)threadIdx.x;
    const int64_t N = min((int64_t)max(lens[b], 0), n_cap);
    const int64_t t0 = (int64_t)t * LM_TILE;
    if (t0 >= N) return;  // (block-uniform)
    const int cnt = (int)min((int64_t)LM_TILE, N - t0);
    const float g0 = levels[(int64_t)b * 4 + 2];
    const int span = cnt + H + 2 * A;  // <= LM_SPAN: the host checked A and H
    const int64_t lo = t0 - A - H;
    const float* er = env + (int64_t)b * env_stride;
    for (int i = tid; i < span; i += LM_THREADS) {
        const int64_t idx = lo + i;
        float r = 1.f;
        if (idx >= 0 && idx < N) {
            const float e = er[idx];
            if (e != 0.f) r = fminf(1.f, c / (g0 * e));
        }
        buf[0][i] = r;
    }
    __syncthreads();
    // sliding minimum over W = H + A + 1: buf[cur][i] = min r over [i, i + h) wherever that window lies inside the span
    const int W = H + A + 1;
    int cur = 0, h = 1;
    for (; 2 * h <= W; h *= 2) {  // (uniform)
        const float* src = buf[cur];
        float* dst = buf[cur ^ 1];
        for (int i = tid; i < span; i += LM_THREADS) {
            float v = src[i];
            if (i + h < span) v = fminf(v, src[i + h]);
            dst[i] = v;
        }
        __syncthreads();
        cur ^= 1;
    }
    // m[j], j = t0 - A + i: the window [i, i + W) as two windows of h (h <= W < 2 h); i + W - 1 <= span - 1
    const int nm = cnt + A, off = W - h;
    {
        const float* src = buf[cur];
        float* dst = buf[cur ^ 1];
        for (int i = tid; i < nm; i += LM_THREADS) dst[i] = fminf(src[i], src[i + off]);
        __syncthreads();
        cur ^= 1;
    }
    const float* m = buf[cur];
    // s[n] = mean(m[n - A .. n]) = the A + 1 values from index o on; the threads' chains are independent. (A thread past the row's end sums what lies there
    // and stores nothing; o + A < LM_SPAN.)
    double acc[LM_SPT];
#pragma unroll
    for (int it = 0; it < LM_SPT; ++it) acc[it] = 0.0;
    for (int k = 0; k <= A; ++k) {
#pragma unroll
        for (int it = 0; it < LM_SPT; ++it) acc[it] += (double)m[tid + it * LM_THREADS + k];
    }
    const double inv_n = (double)(A + 1);
    const float* xr = x + (int64_t)b * x_stride + t0;
    float* yr = y + (int64_t)b * y_stride + t0;
    float smin = 1.f;
    int below = 0;
#pragma unroll
    for (int it = 0; it < LM_SPT; ++it) {
        const int o = tid + it * LM_THREADS;
        if (o < cnt) {
            const float s = (float)(acc[it] / inv_n);
            smin = fminf(smin, s);
            below += s < 1.f;
            const float g = g0 * s;
            yr[o] = xr[o] * g;
        }
    }
    smin = lm_block_min(smin, red, tid);
    below = lm_block_sum(below, reinterpret_cast<int*>(red), tid);
    if (tid == 0) {
        float* st = tstat + ((int64_t)b * tiles + t) * 2;
        st[0] = smin, st[1] = (float)below;  // (<= 2048: exact)
    }
}

// TP(y), min s and the share of every row
__global__ __launch_bounds__(LM_THREADS) void limit_final_kernel(const int* __restrict__ lens, int64_t n_cap, const float* __restrict__ tmax, const float* __restrict__ tstat,
                                                                 int tiles, float* __restrict__ limits) {
    __shared__ float red[LM_THREADS];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int64_t N = min((int64_t)max(lens[b], 0), n_cap);
    const int nt = (int)((N + LM_TILE - 1) / LM_TILE);
    float m = 0.f, smin = 1.f;
    int below = 0;
    for (int i = tid; i < nt; i += LM_THREADS) {
        m = fmaxf(m, tmax[(int64_t)b * tiles + i]);
        if (tstat) {
            smin = fminf(smin, tstat[((int64_t)b * tiles + i) * 2]);
            below += (int)tstat[((int64_t)b * tiles + i) * 2 + 1];
        }
    }
    m = lm_block_max(m, red, tid);
    smin = lm_block_min(smin, red, tid);
    below = lm_block_sum(below, reinterpret_cast<int*>(red), tid);
    if (tid == 0) {
        float* lr = limits + (int64_t)b * 4;
        lr[1] = m, lr[2] = smin, lr[3] = N > 0 ? (float)((double)below / (double)N) : 0.f;
    }
}

hipError_t launch_limit(const LimitCall& c, hipStream_t s) {
    const LimiterPlan& p = c.plan;
    if (!c.x || !c.y || c.x == c.y || !c.lens || !c.taps || !c.scratch || !c.levels || !c.limits || c.batch < 1 || c.max_len < 0 || c.max_len > c.x_stride ||
        c.max_len > c.y_stride || c.max_len > INT32_MAX || p.up.L != 4 || p.up.M != 1 || p.up.R != LM_R || p.up.K != LM_K || p.A < 0 || p.A > kLimitMaxA || p.H < 0 ||
        p.H > kLimitMaxH || p.tile != LM_TILE || ((uintptr_t)c.scratch & 3) != 0 || c.kind < VITS_LEVEL_GAIN || c.kind > VITS_LEVEL_LOUDNESS || !(c.ceiling > 0.f))
        return hipErrorInvalidValue;
    // (the carving limit_scratch_bytes sizes)
    const int64_t tiles = std::max<int64_t>((c.max_len + LM_TILE - 1) / LM_TILE, 1), env_stride = (c.max_len + 3) / 4 * 4;
    if ((int64_t)c.batch * tiles > INT32_MAX) return hipErrorInvalidValue;
    float* env = reinterpret_cast<float*>(c.scratch);
    float* tmax_x = env + (size_t)c.batch * env_stride;
    float* tmax_y = tmax_x + (size_t)c.batch * tiles;
    float* tstat = tmax_y + (size_t)c.batch * tiles;
    const bool limit = c.kind != VITS_LEVEL_PEAK;
    const dim3 grid((unsigned)((int64_t)c.batch * tiles)), rows((unsigned)c.batch), block(LM_THREADS);
    if (c.max_len > 0) {
        if (limit) VITS_KLAUNCH((limit_meter_kernel<true>), grid, block, 0, s, c.x, c.x_stride, c.lens, c.max_len, c.taps, env, env_stride, tmax_x, (int)tiles);
        else VITS_KLAUNCH((limit_meter_kernel<false>), grid, block, 0, s, c.x, c.x_stride, c.lens, c.max_len, c.taps, env, env_stride, tmax_x, (int)tiles);
    }
    VITS_KLAUNCH(limit_gain_kernel, rows, block, 0, s, c.lens, c.max_len, tmax_x, (int)tiles, c.kind, c.value_db, c.gain, c.levels, c.limits);
    if (c.max_len > 0) {
        if (limit)
            VITS_KLAUNCH(limit_apply_kernel, grid, block, 0, s, c.x, c.x_stride, c.y, c.y_stride, c.lens, c.max_len, env, env_stride, c.levels, c.ceiling, p.A, p.H, tstat, (int)tiles);
        else {
            // true-peak normalisation: under the stated peak by construction, the plain multiply
            LevelScale sc;
            sc.x = c.x, sc.x_stride = c.x_stride, sc.y = c.y, sc.y_stride = c.y_stride, sc.lens = c.lens, sc.levels = c.levels, sc.batch = c.batch, sc.max_range = c.max_len;
            const hipError_t e = launch_level_scale(sc, s);
            if (e != hipSuccess) return e;
        }
        VITS_KLAUNCH((limit_meter_kernel<false>), grid, block, 0, s, c.y, c.y_stride, c.lens, c.max_len, c.taps, env, env_stride, tmax_y, (int)tiles);
    }
    VITS_KLAUNCH(limit_final_kernel, rows, block, 0, s, c.lens, c.max_len, tmax_y, limit ? tstat : nullptr, (int)tiles, c.limits);
    return hipGetLastError();
}

}  // namespace vits
