// pitch.hip — varispeed of a ragged batch of PCM rows, a ratio per row (include/vits.h "a stated pitch" / vits_op_pitch; DESIGN.md §8 "A stated pitch").
// The integers of a row, the prototype and its two tables are stated in kernels.h (PitchPlan); this file is the one kernel that applies them.
//
// Block = one tile of kPitchTile consecutive output samples [jb, je) of ONE row, four per thread, as in resample.hip. P, S, R and K depend on the row alone, so
// they and the staged span are block-uniform. The input samples the tile needs, [n0(jb) - R, n0(je - 1) + R], are staged in LDS once — 16-byte loads from
// the row, starting at a multiple of four samples — with ZERO wherever the index falls outside the row's own [0, N): the tap loop has no edge test, and
// nothing behind N is ever read. At the largest ratio the span is 2 (tile - 1) + 1 + 2 * 70 + 6 samples: 8.6 KiB, so the tile never has to shrink
// (PT_SPAN's static_assert states the bound).
//
// A tap's weight is made where it is used: tau = |(k - R) 2^24 - f| (32 bits), u = (tau S) >> 24 (the one 64-bit product), i = u >> 16, fr = (u & 65535)
// 2^-16, h = a fmaf(fr, D[i], G[i]). The two tables are interleaved {G[i], D[i]} and read with ONE 8-byte load from global memory: 64 KiB that every block of
// the launch shares, so it lives in L2 (and its hot middle in the vector cache); as two LDS arrays it would cost every block 64 KiB for an 8.6 KiB tile. An
// index at or behind Z Q is clamped to Z Q, where G = D = 0: h = +0 there, as the definition says, without a branch. The tap still runs, fmaf(+0, x, acc):
// the same bits for every finite x, and the reason the header asks for finite rows (an Inf or NaN there would reach acc, which the host evaluation skips).
//
// No matrix-core work: K gathers and K fused multiply-adds per output sample, with about a dozen integer operations per tap in front of them; VALU- and
// latency-bound by construction. The four chains of a thread are independent.
#include <hip/hip_runtime.h>

#include "kernel_common.h"
#include "kernels.h"

namespace vits {

constexpr int PT_THREADS = 256;
constexpr int PT_OPT = kPitchTile / PT_THREADS;  // outputs per thread
// floats of LDS: the span of a tile at the largest ratio, floor((tile - 1) 2) + 1 + 2 R, + 3 for the start rounded down to a multiple of four, + 3 for the
// end rounded up, with slack
constexpr int PT_SPAN = 2 * kPitchTile + 2 * kPitchMaxR + 20;
static_assert(2 * (kPitchTile - 1) + 1 + 2 * kPitchMaxR + 6 <= PT_SPAN && PT_SPAN * 4 <= 64 * 1024, "the staged span of a tile at ratio 2 must fit the block's LDS");
constexpr int PT_ZQ = kPitchZ * kPitchQ;

template <bool VEC>  // rows start on 16-byte boundaries
__global__ __launch_bounds__(PT_THREADS) void pitch_kernel(const float* __restrict__ x, int64_t x_stride, const int* __restrict__ lens, const float* __restrict__ ratios,
                                                           float* __restrict__ y, int64_t y_stride, const float2v* __restrict__ table, int* __restrict__ lens_out,
                                                           int tiles) {
    __shared__ __attribute__((aligned(16))) float xs[PT_SPAN];  // (written and, at a0, read in 16-byte pieces)
    const int b = (int)(blockIdx.x / (unsigned)tiles), t = (int)(blockIdx.x % (unsigned)tiles), tid = (int)threadIdx.x;
    const int64_t N = min(min((int64_t)max(lens[b], 0), x_stride), kPitchMaxLen);
    // (the host has checked the ratio; the clamp keeps R, K and the span inside what this block has room for whatever the array holds)
    const float ratio = fminf(fmaxf(ratios[b], kPitchMinRatio), kPitchMaxRatio);
    const int64_t P = (int64_t)(ratio * 16777216.0f);  // (exact)
    const int64_t n_out = min((N * kPitchOne + P - 1) / P, y_stride);
    if (t == 0 && tid == 0 && lens_out) lens_out[b] = (int)n_out;
    const int64_t jb = (int64_t)t * kPitchTile;
    if (jb >= n_out) return;  // (block-uniform)
    const int64_t je = min(n_out, jb + kPitchTile);
    const int last = (int)(je - 1 - jb);
    const float* xr = x + (int64_t)b * x_stride;
    float* yr = y + (int64_t)b * y_stride + jb;
    if (P == kPitchOne) {
        // ratio 1: the row as it is (the filter at p = 1 is a 0.92-Nyquist low-pass, not an identity)
#pragma unroll
        for (int i = 0; i < PT_OPT; ++i)
            if (tid + i * PT_THREADS <= last) yr[tid + i * PT_THREADS] = xr[jb + tid + i * PT_THREADS];
        return;
    }
    const unsigned S = (unsigned)(P <= kPitchOne ? kPitchS0 : (kPitchS0 << 24) / P);
    const int R = (int)(((1u << 29) + S - 1) / S), K = 2 * R + 1;
    const float a = (float)S * (1.0f / 16777216.0f);  // (exact: S < 2^24)
    const int64_t n_first = ((jb * P) >> 24) - R, n_last = (((je - 1) * P) >> 24) + R;
    const int64_t a0 = n_first & ~(int64_t)3;  // (rounds down for negative indices too)
    const int span4 = ((int)(n_last - a0 + 1) + 3) & ~3;
    for (int i = tid * 4; i < span4; i += PT_THREADS * 4) {
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
    float acc[PT_OPT];
    const float* xp[PT_OPT];
    int f[PT_OPT];
#pragma unroll
    for (int i = 0; i < PT_OPT; ++i) {
        // (a thread past the tile's end runs the chain of the last sample and stores nothing: the loop below stays free of tests)
        const int64_t tm = (jb + min(tid + i * PT_THREADS, last)) * P;
        xp[i] = xs + ((tm >> 24) - R - a0);
        f[i] = (int)(tm & (kPitchOne - 1));
        acc[i] = 0.f;
    }
#pragma unroll 2
    for (int k = 0; k < K; ++k) {
        const int base = (k - R) * (1 << 24);  // (|k - R| <= 70: 31 bits with the sign)
#pragma unroll
        for (int i = 0; i < PT_OPT; ++i) {
            const int d = base - f[i];
            const unsigned tau = (unsigned)(d < 0 ? -d : d);
            const unsigned u = (unsigned)(((uint64_t)tau * S) >> 24);  // tau S < 2^55
            const float2v gd = table[min(u >> 16, (unsigned)PT_ZQ)];
            const float fr = (float)(u & 65535u) * (1.0f / 65536.0f);
            const float h = a * fmaf(fr, gd.y, gd.x);
            acc[i] = fmaf(h, xp[i][k], acc[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < PT_OPT; ++i)
        if (tid + i * PT_THREADS <= last) yr[tid + i * PT_THREADS] = acc[i];
}

hipError_t launch_pitch(const PitchCall& c, hipStream_t s) {
    if (!c.x || !c.lens || !c.ratios || !c.y || !c.table || c.x == c.y || c.batch < 1 || c.x_stride < 0 || c.y_stride < 0 || c.max_out < 0 || c.max_out > INT32_MAX ||
        c.max_out > c.y_stride || ((uintptr_t)c.table & 7) != 0)
        return hipErrorInvalidValue;
    // (a call whose rows are all empty still states their lengths)
    const int64_t tiles = std::max<int64_t>(1, (c.max_out + kPitchTile - 1) / kPitchTile);
    if ((int64_t)c.batch * tiles > INT32_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((int64_t)c.batch * tiles)), block(PT_THREADS);
    const float2v* table = reinterpret_cast<const float2v*>(c.table);
    if (((uintptr_t)c.x & 15) == 0 && (c.x_stride & 3) == 0)
        VITS_KLAUNCH((pitch_kernel<true>), grid, block, 0, s, c.x, c.x_stride, c.lens, c.ratios, c.y, c.y_stride, table, c.lens_out, (int)tiles);
    else
        VITS_KLAUNCH((pitch_kernel<false>), grid, block, 0, s, c.x, c.x_stride, c.lens, c.ratios, c.y, c.y_stride, table, c.lens_out, (int)tiles);
    return hipGetLastError();
}

}  // namespace vits
