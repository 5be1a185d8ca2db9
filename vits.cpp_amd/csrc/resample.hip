// resample.hip — sample-rate conversion of a ragged batch of PCM rows (include/vits.h vits_model_set_rates / vits_op_resample; DESIGN.md §8 "Any sample
// rate"). The filter, its table and the index rule are stated in kernels.h (ResamplePlan); this file is the one kernel that applies them.
//
// Block = one tile of consecutive output samples [jb, je) of ONE row (kResampleTile = 1024, four per thread; 512 / 256 where a steep downsampling ratio
// would make the staged span too large). The input samples the tile needs, [floor(jb M / L) - R, floor((je - 1) M / L) + R], are staged in LDS once —
// 16-byte loads from the row, starting at a multiple of four samples, so that a wave reads 1 KiB contiguously — with ZERO wherever the index falls outside
// the row's own [0, len): the row's ends are the only place the loads branch per element, and the tap loop has no edge test at all (fmaf(h, 0, acc) is
// acc). Nothing behind len is ever read, so what lies in the gap up to x_stride (another call's data, NaN) cannot enter.
//
// Each thread then runs the chain of its outputs: acc = 0; for k ascending: acc = fmaf(h[p][k], x[n_c - R + k], acc). The four chains of a thread are
// independent, which is all the instruction-level parallelism a dependent chain of K fused multiply-adds can have. The tap table is read from global
// memory in the layout [K][L]: at a given k the threads of a wave differ only in their phase p = (j M) mod L, so their 64 loads fall into ONE row of L
// floats (one address for L = 1, three for 16 -> 48 kHz, 1.7 KiB for L = 441), which stays in L2 for the whole launch; [L][K], the layout of the public
// table, would make every one of them a gather with a stride of K floats. The LDS reads of x have the stride M / L between lanes: conflict-free when
// upsampling, two-way at 2 : 1.
//
// No matrix-core work: 2 K flops per output sample against 4 (1 + M / L) bytes, latency- and LDS-bound by construction.
#include <hip/hip_runtime.h>

#include "kernel_common.h"
#include "kernels.h"

namespace vits {

constexpr int RS_THREADS = 256;
constexpr size_t RS_LDS_BYTES = 64 * 1024;  // dynamic LDS a launch may ask for without opting in to more

// floats of LDS a tile of `tile` outputs needs: its span of at most floor((tile - 1) M / L) + 1 + 2 R samples, + 3 for the start rounded down to a
// multiple of four, + 3 for the end rounded up (resample_kernel), with slack
static int64_t span_cap(const ResamplePlan& p, int tile) { return (int64_t)tile * p.M / p.L + p.K + 8; }

template <int OPT, bool VEC>  // outputs per thread; VEC: rows start on 16-byte boundaries
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const float* __restrict__ x, int64_t x_stride, const int* __restrict__ lens, const int* __restrict__ j0,
                                                              const int* __restrict__ j1, float* __restrict__ y, int64_t y_stride, const float* __restrict__ taps,
                                                              int L, int M, int R, int K, int tiles) {
    extern __shared__ float xs[];
    constexpr int TILE = OPT * RS_THREADS;
    const int b = (int)(blockIdx.x / (unsigned)tiles), t = (int)(blockIdx.x % (unsigned)tiles), tid = (int)threadIdx.x;
    const int64_t N = min((int64_t)max(lens[b], 0), x_stride);
    const int64_t n_out = (N * L + M - 1) / M;
    const int64_t lo = j0 ? (int64_t)max(j0[b], 0) : 0, hi = j1 ? min((int64_t)j1[b], n_out) : n_out;
    const int64_t jb = lo + (int64_t)t * TILE;
    if (jb >= hi) return;  // (block-uniform)
    const int64_t je = min(hi, jb + TILE);
    const int64_t qb = jb * M, ncb = qb / L;
    const int pb = (int)(qb - ncb * L);
    const int64_t n_first = ncb - R, n_last = ((je - 1) * M) / L + R;
    const int64_t a0 = n_first & ~(int64_t)3;  // (rounds down for negative indices too)
    const int span4 = ((int)(n_last - a0 + 1) + 3) & ~3;
    const float* xr = x + (int64_t)b * x_stride;
    for (int i = tid * 4; i < span4; i += RS_THREADS * 4) {
        const int64_t idx = a0 + i;
        float4v v;
        if (VEC && idx >= 0 && idx + 3 < N) v = *reinterpret_cast<const float4v*>(xr + idx);
        else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (idx + e >= 0 && idx + e < N) ? xr[idx + e] : 0.f;
        }
        *reinterpret_cast<float4v*>(xs + i) = v;
    }
    __syncthreads();
    float acc[OPT];
    const float* xp[OPT];
    const float* hp[OPT];
    const int last = (int)(je - 1 - jb);
#pragma unroll
    for (int i = 0; i < OPT; ++i) {
        // (a thread past the range's end runs the chain of the last sample and stores nothing: the loop below stays free of tests)
        const unsigned dq = (unsigned)min(tid + i * RS_THREADS, last) * (unsigned)M + (unsigned)pb;  // < 1024 M + L: fits 32 bits for every accepted pair
        const unsigned dn = dq / (unsigned)L;
        xp[i] = xs + ((ncb + dn) - R - a0);
        hp[i] = taps + (dq - dn * (unsigned)L);
        acc[i] = 0.f;
    }
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int i = 0; i < OPT; ++i) acc[i] = fmaf(hp[i][(int64_t)k * L], xp[i][k], acc[i]);
    }
    float* yr = y + (int64_t)b * y_stride + jb;
#pragma unroll
    for (int i = 0; i < OPT; ++i)
        if (tid + i * RS_THREADS <= last) yr[tid + i * RS_THREADS] = acc[i];
}

template <int OPT>
static void launch_tile(const ResampleCall& c, int tiles, size_t lds, hipStream_t s) {
    const ResamplePlan& p = c.plan;
    const dim3 grid((unsigned)((int64_t)c.batch * tiles)), block(RS_THREADS);
    if (((uintptr_t)c.x & 15) == 0 && (c.x_stride & 3) == 0)
        VITS_KLAUNCH((resample_kernel<OPT, true>), grid, block, lds, s, c.x, c.x_stride, c.lens, c.j0, c.j1, c.y, c.y_stride, c.taps, p.L, p.M, p.R, p.K, tiles);
    else
        VITS_KLAUNCH((resample_kernel<OPT, false>), grid, block, lds, s, c.x, c.x_stride, c.lens, c.j0, c.j1, c.y, c.y_stride, c.taps, p.L, p.M, p.R, p.K, tiles);
}

hipError_t launch_resample(const ResampleCall& c, hipStream_t s) {
    const ResamplePlan& p = c.plan;
    if (!c.x || !c.lens || !c.y || !c.taps || c.batch < 1 || c.x_stride < 0 || c.y_stride < 0 || p.L < 1 || p.M < 1 || p.R < 0 || p.K != 2 * p.R + 1 ||
        (int64_t)p.L * p.K > kResampleMaxTaps || c.max_range < 0 || c.max_range > INT32_MAX)
        return hipErrorInvalidValue;
    if (c.max_range == 0) return hipSuccess;
    int tile = kResampleTile;
    while (tile > RS_THREADS && (size_t)span_cap(p, tile) * 4 > RS_LDS_BYTES) tile /= 2;
    const size_t lds = (size_t)span_cap(p, tile) * 4;
    // (the kernel's per-thread phase arithmetic is 32-bit: tile M + L must fit)
    if (lds > RS_LDS_BYTES || (int64_t)tile * p.M + p.L > (int64_t)UINT32_MAX) return hipErrorInvalidValue;
    const int64_t tiles = (c.max_range + tile - 1) / tile;
    if ((int64_t)c.batch * tiles > INT32_MAX) return hipErrorInvalidValue;
    if (tile == 1024) launch_tile<4>(c, (int)tiles, lds, s);
    else if (tile == 512) launch_tile<2>(c, (int)tiles, lds, s);
    else launch_tile<1>(c, (int)tiles, lds, s);
    return hipGetLastError();
}

}  // namespace vits
