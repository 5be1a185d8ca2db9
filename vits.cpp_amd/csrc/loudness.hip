// loudness.hip — levelling of a ragged batch of PCM rows: ITU-R BS.1770-4 integrated loudness, sample peak, the gain of the handle's kind, and the
// multiply (include/vits.h vits_model_set_level / vits_op_level; DESIGN.md §8 "A stated level"). The state-space form of the filter and the cut of an
// utterance are stated in kernels.h; the coefficients and the matrix powers come from loudness_host.cpp.
//
// The K-weighting cascade is a linear recurrence along time, v' = A v + B x with four states. It is made parallel WITHIN an utterance in three steps:
//   level_pass_kernel<0>  every sub-segment of kLevelQ = 64 samples runs the filter from zero state and keeps its final state z_q
//   level_scan_kernel     one wave per utterance turns them into the true state at every sub-segment's start, in_(q+1) = A^Q in_q + z_q: a lane scans a
//                         group of kLevelGroup = 16 sub-segments from zero, ONE lane chains the 64 group results with A^(16 Q), every lane rescans its group
//                         from the group's true start: 16 + 64 + 16 dependent steps per 65536 samples instead of 1024
//   level_pass_kernel<1>  every sub-segment reruns from its true state and sums the squares of the weighted signal, in ascending sample order, into at
//                         most two partial sums (a sub-segment touches at most two 100 ms segments), and takes max |x|
//   level_finish_kernel   one block per utterance: a segment's mean square is the sum of its sub-segments' partials in ascending order; blocks, both
//                         gates (fixed-shape trees), L, P, and g by the call's kind -> the row [L, P, g, blocks]
//   level_scale_kernel    y = x * g, one fp32 multiply; the whole row, or the range a streaming window made final
// Sub-segments and groups are anchored at the utterance's own sample 0 and nothing is accumulated with atomics: batch position, batch size, grid and
// stream do not enter a bit. Filter, sums and gates are fp64 (the high-pass pole sits at 1 - 0.005 at 48 kHz; 78 TFLOP/s of vector fp64 make it free).
//
// Block of the two sample passes = 128 lanes = 128 consecutive sub-segments = 8192 samples of ONE row, staged in LDS with 16-byte loads (a wave reads
// 1 KiB contiguously) into rows of Q + 1 floats, so that the 64 lanes of a wave, each walking its own row, hit 64 different banks. Only samples inside
// the row's own [0, len) are loaded or walked: what lies in the gap up to x_stride cannot enter.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/vits.h"
#include "kernel_common.h"
#include "kernels.h"

namespace vits {

constexpr int LV_Q = kLevelQ, LV_G = kLevelGroup;
constexpr int LV_THREADS = 128;
constexpr int LV_TILE = LV_THREADS * LV_Q;  // samples per block
constexpr int LV_PITCH = LV_Q + 1;          // floats per LDS row
constexpr int LV_FIN_THREADS = 256;
constexpr int LV_SCALE_THREADS = 256, LV_SCALE_TILE = LV_SCALE_THREADS * 4;
static_assert(LV_Q % 4 == 0, "a 16-byte load stays inside one sub-segment");

struct LvState {
    double s1, s2, t1, t2;
};

// one sample through the cascade (transposed direct form II); returns the weighted sample
__device__ __forceinline__ double lv_step(const LevelCoef& k, LvState& v, double x) {
    const double y1 = fma(k.c[0], x, v.s1);
    v.s1 = fma(k.c[1], x, fma(-k.c[3], y1, v.s2));
    v.s2 = fma(k.c[2], x, -k.c[4] * y1);
    const double y2 = fma(k.c[5], y1, v.t1);
    v.t1 = fma(k.c[6], y1, fma(-k.c[8], y2, v.t2));
    v.t2 = fma(k.c[7], y1, -k.c[9] * y2);
    return y2;
}

// m v + z
__device__ __forceinline__ LvState lv_advance(const double* m, const LvState& v, const LvState& z) {
    LvState r;
    r.s1 = fma(m[0], v.s1, fma(m[1], v.s2, fma(m[2], v.t1, fma(m[3], v.t2, z.s1))));
    r.s2 = fma(m[4], v.s1, fma(m[5], v.s2, fma(m[6], v.t1, fma(m[7], v.t2, z.s2))));
    r.t1 = fma(m[8], v.s1, fma(m[9], v.s2, fma(m[10], v.t1, fma(m[11], v.t2, z.t1))));
    r.t2 = fma(m[12], v.s1, fma(m[13], v.s2, fma(m[14], v.t1, fma(m[15], v.t2, z.t2))));
    return r;
}

__device__ __forceinline__ LvState lv_load(const double* p) { return LvState{p[0], p[1], p[2], p[3]}; }
__device__ __forceinline__ void lv_store(double* p, const LvState& v) { p[0] = v.s1, p[1] = v.s2, p[2] = v.t1, p[3] = v.t2; }

// samples [t0, min(t0 + LV_TILE, N)) of a row -> xs[sub-segment][LV_PITCH]
template <bool VEC>
__device__ __forceinline__ void lv_stage(const float* __restrict__ xr, int64_t t0, int64_t N, float* xs, int tid) {
    const int span = (int)min((int64_t)LV_TILE, N - t0);
    for (int i = tid * 4; i < span; i += LV_THREADS * 4) {
        const int64_t idx = t0 + i;
        float4v v;
        if (VEC && idx + 3 < N) v = *reinterpret_cast<const float4v*>(xr + idx);
        else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = idx + e < N ? xr[idx + e] : 0.f;
        }
        float* d = xs + (i / LV_Q) * LV_PITCH + (i % LV_Q);
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = v[e];
    }
}

// SUM = false: the final state of every sub-segment run from zero -> state [b][q][4]
// SUM = true: state [b][q] holds the true state at the sub-segment's start; partial sums of squares -> part [b][q][2], max |x| -> pk [b][q]
template <bool SUM, bool VEC>
__global__ __launch_bounds__(LV_THREADS) void level_pass_kernel(const float* __restrict__ x, int64_t x_stride, int64_t n_cap, const int* __restrict__ lens, LevelCoef k,
                                                                int S, double* __restrict__ state, double* __restrict__ part, float* __restrict__ pk, int64_t nq_stride,
                                                                int tiles) {
    __shared__ float xs[LV_THREADS * LV_PITCH];
    const int b = (int)(blockIdx.x / (unsigned)tiles), t = (int)(blockIdx.x % (unsigned)tiles), tid = (int)threadIdx.x;
    const int64_t N = min((int64_t)max(lens[b], 0), n_cap);  // (n_cap <= x_stride is what the host sized grid and scratch for)
    const int64_t t0 = (int64_t)t * LV_TILE;
    if (t0 >= N) return;  // (block-uniform)
    lv_stage<VEC>(x + (int64_t)b * x_stride, t0, N, xs, tid);
    __syncthreads();
    const int64_t q = (int64_t)t * LV_THREADS + tid, start = q * LV_Q;
    if (start >= N) return;
    const int cnt = (int)min((int64_t)LV_Q, N - start);
    const float* xq = xs + tid * LV_PITCH;
    double* sq = state + ((int64_t)b * nq_stride + q) * 4;
    if constexpr (!SUM) {
        LvState v{0.0, 0.0, 0.0, 0.0};
        for (int i = 0; i < cnt; ++i) lv_step(k, v, (double)xq[i]);
        lv_store(sq, v);
    } else {
        LvState v = lv_load(sq);
        // samples of the sub-segment that lie in its first segment (the rest lie in the next one)
        const int64_t seg = start / S;
        const int first = (int)min((int64_t)cnt, (seg + 1) * S - start);
        double a0 = 0.0, a1 = 0.0;
        float m = 0.f;
        for (int i = 0; i < first; ++i) {
            const float xv = xq[i];
            m = fmaxf(m, fabsf(xv));
            const double y = lv_step(k, v, (double)xv);
            a0 = fma(y, y, a0);
        }
        for (int i = first; i < cnt; ++i) {
            const float xv = xq[i];
            m = fmaxf(m, fabsf(xv));
            const double y = lv_step(k, v, (double)xv);
            a1 = fma(y, y, a1);
        }
        double* pq = part + ((int64_t)b * nq_stride + q) * 2;
        pq[0] = a0, pq[1] = a1;
        pk[(int64_t)b * nq_stride + q] = m;
    }
}

// in place: state [b][q] = final state of sub-segment q run from zero -> the true state at its start. One wave per utterance.
__global__ __launch_bounds__(64) void level_scan_kernel(const int* __restrict__ lens, int64_t n_cap, LevelCoef k, double* __restrict__ state, int64_t nq_stride) {
    __shared__ double gs[64][4];
    __shared__ double carry[4];
    const int b = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int64_t N = min((int64_t)max(lens[b], 0), n_cap);
    const int64_t nq = (N + LV_Q - 1) / LV_Q, ng = (nq + LV_G - 1) / LV_G;
    double* st = state + (int64_t)b * nq_stride * 4;
    if (lane == 0) carry[0] = carry[1] = carry[2] = carry[3] = 0.0;
    for (int64_t g0 = 0; g0 < ng; g0 += 64) {  // (uniform)
        const int64_t g = g0 + lane, qa = g * LV_G;
        // the group's 16 zero-state results, loaded ONCE and at once (a load inside either dependent chain below would cost a memory round trip per step);
        // behind the utterance's last sub-segment they are zero, which leaves what is used unchanged
        LvState z[LV_G];
#pragma unroll
        for (int j = 0; j < LV_G; ++j) z[j] = qa + j < nq ? lv_load(st + (qa + j) * 4) : LvState{0.0, 0.0, 0.0, 0.0};
        LvState v{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < LV_G; ++j) v = lv_advance(k.AQ, v, z[j]);
        lv_store(gs[lane], v);
        __syncthreads();
        if (lane == 0) {
            LvState cur = lv_load(carry);
            const int n = (int)min((int64_t)64, ng - g0);
            for (int l = 0; l < n; ++l) {
                const LvState zg = lv_load(gs[l]);
                lv_store(gs[l], cur);
                cur = lv_advance(k.AG, cur, zg);
            }
            lv_store(carry, cur);
        }
        __syncthreads();
        v = lv_load(gs[lane]);
#pragma unroll
        for (int j = 0; j < LV_G; ++j) {
            if (qa + j < nq) lv_store(st + (qa + j) * 4, v);
            v = lv_advance(k.AQ, v, z[j]);
        }
        __syncthreads();
    }
}

// fixed-shape trees over the block of a sum and a count; every thread gets the results
__device__ __forceinline__ void lv_block_sum2(double& a, double& c, double (*red)[2], int tid) {
    __syncthreads();
    red[tid][0] = a, red[tid][1] = c;
    __syncthreads();
    for (int w = LV_FIN_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) red[tid][0] += red[tid + w][0], red[tid][1] += red[tid + w][1];
        __syncthreads();
    }
    a = red[0][0], c = red[0][1];
}

__global__ __launch_bounds__(LV_FIN_THREADS) void level_finish_kernel(const int* __restrict__ lens, int64_t n_cap, int S, const double* __restrict__ part,
                                                                      const float* __restrict__ pk, double* __restrict__ zseg, int64_t nq_stride, int64_t nseg_stride,
                                                                      int kind, float value_db, float ceiling_db, float gain, float* __restrict__ levels) {
    __shared__ double red[LV_FIN_THREADS][2];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int64_t N = min((int64_t)max(lens[b], 0), n_cap);
    const int64_t nq = (N + LV_Q - 1) / LV_Q, nseg = N / S, nblk = nseg >= 4 ? nseg - 3 : 0;
    const double* pr = part + (int64_t)b * nq_stride * 2;
    double* z = zseg + (int64_t)b * nseg_stride;
    for (int64_t i = tid; i < nseg; i += LV_FIN_THREADS) {
        const int64_t qa = i * S / LV_Q, qb = ((i + 1) * S - 1) / LV_Q;
        // (only the first sub-segment can have begun in the segment before: then its second partial is this segment's; Q <= S)
        double acc = pr[qa * 2 + (qa * LV_Q < i * S ? 1 : 0)];
        for (int64_t q = qa + 1; q <= qb; ++q) acc += pr[q * 2];
        z[i] = acc / (double)S;
    }
    float m = 0.f;
    for (int64_t q = tid; q < nq; q += LV_FIN_THREADS) m = fmaxf(m, pk[(int64_t)b * nq_stride + q]);
    // the peak: a maximum is exact in any order (the barriers also complete z)
    red[tid][0] = (double)m;
    __syncthreads();
    for (int w = LV_FIN_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) red[tid][0] = fmax(red[tid][0], red[tid + w][0]);
        __syncthreads();
    }
    const float peak = (float)red[0][0];
    // gate 1: blocks above -70 LUFS
    double sum = 0.0, cnt = 0.0;
    for (int64_t j = tid; j < nblk; j += LV_FIN_THREADS) {
        const double blk = ((z[j] + z[j + 1]) + (z[j + 2] + z[j + 3])) * 0.25;
        if (-0.691 + 10.0 * log10(blk) > -70.0) sum += blk, cnt += 1.0;
    }
    lv_block_sum2(sum, cnt, red, tid);
    const double s1 = sum, c1 = cnt;
    double L = -INFINITY, c2 = 0.0;
    if (c1 > 0.0) {  // (uniform)
        const double gamma = -0.691 + 10.0 * log10(s1 / c1) - 10.0;
        sum = 0.0, cnt = 0.0;
        for (int64_t j = tid; j < nblk; j += LV_FIN_THREADS) {
            const double blk = ((z[j] + z[j + 1]) + (z[j + 2] + z[j + 3])) * 0.25;
            const double l = -0.691 + 10.0 * log10(blk);
            if (l > -70.0 && l > gamma) sum += blk, cnt += 1.0;
        }
        lv_block_sum2(sum, cnt, red, tid);
        const double s2 = sum;
        c2 = cnt;
        if (c2 > 0.0) L = -0.691 + 10.0 * log10(s2 / c2);
    }
    if (tid == 0) {
        // the gain from the values as they are reported (fp32 L and P)
        const float Lf = (float)L;
        float g = 1.f;
        if (kind == VITS_LEVEL_GAIN) g = gain;
        else if (kind == VITS_LEVEL_PEAK) {
            if (peak > 0.f) g = (float)(pow(10.0, (double)value_db / 20.0) / (double)peak);
        } else if (kind == VITS_LEVEL_LOUDNESS) {
            if (peak > 0.f && c2 > 0.0) g = (float)fmin(pow(10.0, ((double)value_db - (double)Lf) / 20.0), pow(10.0, (double)ceiling_db / 20.0) / (double)peak);
        }
        float* row = levels + (int64_t)b * 4;
        row[0] = Lf, row[1] = peak, row[2] = g, row[3] = (float)c2;
    }
}

template <bool VEC>
__global__ __launch_bounds__(LV_SCALE_THREADS) void level_scale_kernel(const float* __restrict__ x, int64_t x_stride, float* __restrict__ y, int64_t y_stride,
                                                                       const int* __restrict__ lens, const int* __restrict__ j0, const int* __restrict__ j1,
                                                                       const float* __restrict__ levels, float gain, int tiles) {
    const int b = (int)(blockIdx.x / (unsigned)tiles), t = (int)(blockIdx.x % (unsigned)tiles), tid = (int)threadIdx.x;
    const int64_t N = min(min((int64_t)max(lens[b], 0), x_stride), y_stride);
    const int64_t lo = j0 ? (int64_t)max(j0[b], 0) : 0, hi = j1 ? min((int64_t)j1[b], N) : N;
    // tiles start at a multiple of four samples below the range's start: the 16-byte accesses stay aligned
    const int64_t i = (lo & ~(int64_t)3) + (int64_t)t * LV_SCALE_TILE + tid * 4;
    if (i >= hi) return;
    const float g = levels ? levels[(int64_t)b * 4 + 2] : gain;
    const float* xr = x + (int64_t)b * x_stride;
    float* yr = y + (int64_t)b * y_stride;
    if (VEC && i >= lo && i + 3 < hi) {
        float4v v = *reinterpret_cast<const float4v*>(xr + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] * g;
        *reinterpret_cast<float4v*>(yr + i) = v;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (i + e >= lo && i + e < hi) yr[i + e] = xr[i + e] * g;
    }
}

namespace {
struct LvScratch {
    double *state, *part, *zseg;
    float* pk;
    int64_t nq_stride, nseg_stride;
};
// (the carving level_scratch_bytes sizes)
LvScratch carve(void* scratch, int batch, int64_t max_len, int S) {
    LvScratch r;
    r.nq_stride = (max_len + LV_Q - 1) / LV_Q + 1;
    r.nseg_stride = max_len / S + 1;
    r.state = reinterpret_cast<double*>(scratch);
    r.part = r.state + (size_t)batch * r.nq_stride * 4;
    r.zseg = r.part + (size_t)batch * r.nq_stride * 2;
    r.pk = reinterpret_cast<float*>(r.zseg + (size_t)batch * r.nseg_stride);
    return r;
}
}  // namespace

hipError_t launch_level_measure(const LevelCall& c, hipStream_t s) {
    const int S = c.plan.S;
    if (!c.x || !c.lens || !c.levels || !c.scratch || c.batch < 1 || c.x_stride < 0 || c.max_len < 0 || c.max_len > c.x_stride || S < LV_Q ||
        ((uintptr_t)c.scratch & 7) != 0 || c.kind < VITS_LEVEL_MEASURE || c.kind > VITS_LEVEL_LOUDNESS)
        return hipErrorInvalidValue;
    const LvScratch w = carve(c.scratch, c.batch, c.max_len, S);
    const int64_t tiles = (c.max_len + LV_TILE - 1) / LV_TILE;
    if ((int64_t)c.batch * std::max<int64_t>(tiles, 1) > INT32_MAX) return hipErrorInvalidValue;
    if (tiles > 0) {
        const dim3 grid((unsigned)((int64_t)c.batch * tiles)), block(LV_THREADS);
        const bool vec = ((uintptr_t)c.x & 15) == 0 && (c.x_stride & 3) == 0;
        if (vec) VITS_KLAUNCH((level_pass_kernel<false, true>), grid, block, 0, s, c.x, c.x_stride, c.max_len, c.lens, c.plan.coef, S, w.state, w.part, w.pk, w.nq_stride, (int)tiles);
        else VITS_KLAUNCH((level_pass_kernel<false, false>), grid, block, 0, s, c.x, c.x_stride, c.max_len, c.lens, c.plan.coef, S, w.state, w.part, w.pk, w.nq_stride, (int)tiles);
        VITS_KLAUNCH(level_scan_kernel, dim3((unsigned)c.batch), dim3(64), 0, s, c.lens, c.max_len, c.plan.coef, w.state, w.nq_stride);
        if (vec) VITS_KLAUNCH((level_pass_kernel<true, true>), grid, block, 0, s, c.x, c.x_stride, c.max_len, c.lens, c.plan.coef, S, w.state, w.part, w.pk, w.nq_stride, (int)tiles);
        else VITS_KLAUNCH((level_pass_kernel<true, false>), grid, block, 0, s, c.x, c.x_stride, c.max_len, c.lens, c.plan.coef, S, w.state, w.part, w.pk, w.nq_stride, (int)tiles);
    }
    VITS_KLAUNCH(level_finish_kernel, dim3((unsigned)c.batch), dim3(LV_FIN_THREADS), 0, s, c.lens, c.max_len, S, w.part, w.pk, w.zseg, w.nq_stride, w.nseg_stride, c.kind,
                 c.value_db, c.ceiling_db, c.gain, c.levels);
    return hipGetLastError();
}

hipError_t launch_level_scale(const LevelScale& c, hipStream_t s) {
    if (!c.x || !c.y || !c.lens || c.batch < 1 || c.x_stride < 0 || c.y_stride < 0 || c.max_range < 0 || c.max_range > INT32_MAX) return hipErrorInvalidValue;
    if (c.max_range == 0) return hipSuccess;
    const int64_t tiles = (c.max_range + 3 + LV_SCALE_TILE - 1) / LV_SCALE_TILE;  // (+ 3: a range may start up to three samples behind its first tile's start)
    if ((int64_t)c.batch * tiles > INT32_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((int64_t)c.batch * tiles)), block(LV_SCALE_THREADS);
    const bool vec = ((uintptr_t)c.x & 15) == 0 && ((uintptr_t)c.y & 15) == 0 && (c.x_stride & 3) == 0 && (c.y_stride & 3) == 0;
    if (vec) VITS_KLAUNCH((level_scale_kernel<true>), grid, block, 0, s, c.x, c.x_stride, c.y, c.y_stride, c.lens, c.j0, c.j1, c.levels, c.gain, (int)tiles);
    else VITS_KLAUNCH((level_scale_kernel<false>), grid, block, 0, s, c.x, c.x_stride, c.y, c.y_stride, c.lens, c.j0, c.j1, c.levels, c.gain, (int)tiles);
    return hipGetLastError();
}

}  // namespace vits
