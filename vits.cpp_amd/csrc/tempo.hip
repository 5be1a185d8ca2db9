// tempo.hip — pitch-preserving time stretch of a ragged batch of PCM rows, a tempo per row (include/vits.h "a stated tempo" / vits_op_tempo; DESIGN.md §8 "A stated
// tempo"). The integers of a row and the definition are stated in kernels.h (TempoPlan); this file holds the two kernels that apply them.
//
// tempo_search_kernel: segment k starts where the 16-bit row around a_k looks most like the row at s_(k-1) + H, so the segments of a row are a chain and a row is
// ONE block; the 2 D + 1 candidates of a step are ONE PER THREAD (the block has 2 D + 1 threads rounded up to whole waves: 320 at 16 kHz; with 256 the one
// candidate left over cost its wave, and so the step, a second pass). Only delta_(k-1) is carried from step to step: a_k is known for every k, the
// template of step k lies inside [a_(k-1) - D + H, a_(k-1) + D + 2 H) and its candidates inside [a_k - D, a_k + D + H), so step k reads nothing outside the
// window W_k = [min(a_(k-1) + H, a_k) - D, max(a_(k-1) + 2 H, a_k + H) + D), at most 2 D + 2 H + 2 samples, known before the chain reaches it. The block keeps two
// such windows in LDS as int16: while step k sums its differences out of one, every thread has the samples of W_(k+1) in flight from global memory, and
// quantises them into the other behind the sums. A step is then LDS reads, integer adds, one wave reduction and ONE barrier; no global round trip lies on the
// chain. A thread sums |template[i] - candidate[j + i]| in int32 (H 65535 < 2^25): the template read is the same address in every lane (a broadcast), the
// candidate reads are consecutive. The argmin is the minimum of the packed key (sum << 10 | rank in the candidate order): ties go to the smaller rank, which is
// the definition's order. Samples outside the row's own [0, N) are zero; nothing behind N is read.
//
// tempo_ola_kernel: block = one tile of kTempoTile consecutive output samples of ONE row, four per thread. H is a multiple of four, so the four samples of a
// thread share their segment: two starts, eight input samples (unaligned: s_k is any integer), two rounded products and one rounded add each, never contracted.
// VEC: rows of x and y on 16-byte boundaries: the store, and the copy of a row with Q = 2^24, go in 16-byte pieces.
#include <hip/hip_runtime.h>

#include "kernel_common.h"
#include "kernels.h"

// (the overlap-add is two rounded products and one rounded add. __fmul_rn and __fadd_rn are plain operators to the compiler, which fuses them under its
// default, so the Makefile builds this file with -ffp-contract=off; the pragma says the same for the code of this file itself)
#pragma clang fp contract(off)

namespace vits {

constexpr int TS_MAX_THREADS = (2 * kTempoMaxD + 1 + 63) / 64 * 64, TS_MAX_WAVES = TS_MAX_THREADS / 64;  // 832, 13
constexpr int TS_WIN = 2 * kTempoMaxD + 2 * kTempoMaxH + 8;  // int16 per window
constexpr int TS_PER = 3;                                    // samples of the next window per thread (launch_tempo_search checks that they cover the window)
static_assert(TS_MAX_THREADS <= 1024 && TS_PER * TS_MAX_THREADS >= TS_WIN, "one candidate per thread, and the threads cover a window in TS_PER loads each");
// the block of a launch at this rate: one thread per candidate, whole waves
static int tempo_search_threads(int rate) { return (2 * (4 * (rate / 500)) + 1 + 63) / 64 * 64; }
static_assert((int64_t)kTempoMaxH * 65535 < ((int64_t)1 << 25) && 2 * kTempoMaxD < 1024, "a sum of H differences and a rank must fit the packed key's fields");
static_assert(2 * TS_WIN * 2 <= 64 * 1024, "two windows must fit the block's LDS");

struct TempoRow {
    int64_t N, Q, n_out, F;
    int H, D;
};
__device__ __forceinline__ TempoRow tempo_row(const int* lens, const float* tempos, int b, int rate, int64_t x_stride, int64_t y_stride) {
    TempoRow r;
    r.N = min(min((int64_t)max(lens[b], 0), x_stride), kTempoMaxLen);
    // (the host has checked tempo and rate; the clamps keep every index inside what the block has room for whatever the arrays hold)
    const float q = fminf(fmaxf(tempos[b], kTempoMin), kTempoMax);
    const int sr = min(max(rate, kTempoMinRate), kTempoMaxRate);
    r.Q = (int64_t)(q * 16777216.0f);  // (exact)
    r.H = 4 * (sr / 400);
    r.D = 4 * (sr / 500);
    r.n_out = min((r.N * kTempoOne + r.Q - 1) / r.Q, y_stride);
    r.F = (r.n_out + r.H - 1) / r.H;
    return r;
}
__device__ __forceinline__ short tempo_quantise(float v) {
    if (v != v) return 0;
    const float r = fminf(fmaxf(rintf(__fmul_rn(v, 32768.0f)), -32768.0f), 32767.0f);
    return (short)(int)r;
}
// the window of step k >= 1: its first sample and its length
__device__ __forceinline__ void tempo_window(const TempoRow& r, int64_t k, int64_t& lo, int& len) {
    const int64_t a0 = ((k - 1) * r.H * r.Q) >> 24, a1 = (k * r.H * r.Q) >> 24;
    lo = min(a0 + r.H, a1) - r.D;
    len = (int)(max(a0 + 2 * r.H, a1 + r.H) + r.D - lo);
}

__global__ __launch_bounds__(TS_MAX_THREADS) void tempo_search_kernel(const float* __restrict__ x, int64_t x_stride, const int* __restrict__ lens,
                                                                  const float* __restrict__ tempos, int rate, int* __restrict__ starts, int64_t starts_stride,
                                                                  int* __restrict__ offsets, int64_t offsets_stride, int64_t y_stride, int* __restrict__ lens_out) {
    __shared__ short win[2][TS_WIN];
    __shared__ unsigned long long wave_key[2][TS_MAX_WAVES];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, nt = (int)blockDim.x, waves = nt >> 6;  // (nt <= TS_MAX_THREADS, a multiple of 64: the launcher's)
    const TempoRow r = tempo_row(lens, tempos, b, rate, x_stride, y_stride);
    const int H = r.H, D = r.D;
    // (what a short buffer cannot hold is not written: the host sizes both for the largest F of the call)
    const int64_t F = min(r.F, min(starts_stride - 1, offsets ? offsets_stride : r.F));
    if (tid == 0 && lens_out) lens_out[b] = (int)r.n_out;
    int* st = starts + (int64_t)b * starts_stride;
    int* of = offsets ? offsets + (int64_t)b * offsets_stride : nullptr;
    if (starts_stride < 1) return;
    if (r.Q == kTempoOne) {
        // tempo 1: the row is copied; its segments lie where they lay
        for (int64_t k = tid; k <= F; k += nt) {
            st[k] = (int)(k * H);
            if (of && k >= 1) of[k - 1] = 0;
        }
        return;
    }
    if (tid == 0) st[0] = 0;
    if (F < 1) return;  // (block-uniform)
    const float* xr = x + (int64_t)b * x_stride;
    float pre[TS_PER];
    // window 1, through the same registers as every later one
    int64_t lo;
    int len;
    tempo_window(r, 1, lo, len);
#pragma unroll
    for (int e = 0; e < TS_PER; ++e) {
        const int j = tid + e * nt;
        const int64_t idx = lo + j;
        if (j < len) win[1][j] = (idx >= 0 && idx < r.N) ? tempo_quantise(xr[idx]) : (short)0;
    }
    __syncthreads();
    int delta = 0;  // delta_(k-1)
    for (int64_t k = 1; k <= F; ++k) {
        const int cur = (int)(k & 1);
        const short* wc = win[cur];
        const int64_t a0 = ((k - 1) * H * r.Q) >> 24, a1 = (k * H * r.Q) >> 24;
        // the next window's samples: on their way while this step sums
        int64_t nlo = 0;
        int nlen = 0;
        if (k < F) {
            tempo_window(r, k + 1, nlo, nlen);
#pragma unroll
            for (int e = 0; e < TS_PER; ++e) {
                const int64_t idx = nlo + tid + e * nt;
                pre[e] = (tid + e * nt < nlen && idx >= 0 && idx < r.N) ? xr[idx] : 0.f;
            }
        }
        const int tpl = (int)(a0 + delta + H - lo), cand0 = (int)(a1 - D - lo);
        unsigned long long key = ~0ull;
        if (tid <= 2 * D) {
            const int j = tid;  // delta = j - D
            const short* cp = wc + cand0 + j;
            const short* tp = wc + tpl;
            int sad = 0;
#pragma unroll 8
            for (int i = 0; i < H; ++i) {
                const int d = (int)tp[i] - (int)cp[i];
                sad += d < 0 ? -d : d;
            }
            const int dl = j - D;
            const unsigned rank = dl == 0 ? 0u : dl < 0 ? (unsigned)(-2 * dl - 1) : (unsigned)(2 * dl);
            const unsigned long long kk = ((unsigned long long)(unsigned)sad << 10) | rank;
            key = kk < key ? kk : key;
        }
        // the next window into the other buffer (its readers finished before the barrier of the step before)
        if (k < F) {
#pragma unroll
            for (int e = 0; e < TS_PER; ++e) {
                const int j = tid + e * nt;
                if (j < nlen) win[cur ^ 1][j] = tempo_quantise(pre[e]);
            }
        }
        // the smallest key of the wave, then of the block
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const unsigned hi = (unsigned)__shfl_xor((int)(key >> 32), off, 64), lw = (unsigned)__shfl_xor((int)(unsigned)key, off, 64);
            const unsigned long long o = ((unsigned long long)hi << 32) | lw;
            key = o < key ? o : key;
        }
        if ((tid & 63) == 0) wave_key[cur][tid >> 6] = key;
        __syncthreads();
        key = wave_key[cur][0];
        for (int wv = 1; wv < waves; ++wv) key = wave_key[cur][wv] < key ? wave_key[cur][wv] : key;
        const int rank = (int)(key & 1023u);
        delta = rank == 0 ? 0 : (rank & 1) ? -((rank + 1) >> 1) : (rank >> 1);
        if (tid == 0) {
            st[k] = (int)(a1 + delta);
            if (of) of[k - 1] = delta;
        }
        lo = nlo;
    }
}

constexpr int TO_THREADS = 256;
static_assert(kTempoTile == 4 * TO_THREADS, "four output samples per thread");

template <bool VEC>  // rows of x and y start on 16-byte boundaries
__global__ __launch_bounds__(TO_THREADS) void tempo_ola_kernel(const float* __restrict__ x, int64_t x_stride, const int* __restrict__ lens, const float* __restrict__ tempos,
                                                               int rate, const int* __restrict__ starts, int64_t starts_stride, float* __restrict__ y, int64_t y_stride,
                                                               int tiles) {
    const int b = (int)(blockIdx.x / (unsigned)tiles), t = (int)(blockIdx.x % (unsigned)tiles), tid = (int)threadIdx.x;
    const TempoRow r = tempo_row(lens, tempos, b, rate, x_stride, y_stride);
    const int64_t m = (int64_t)t * kTempoTile + tid * 4;
    if (m >= r.n_out) return;
    const float* xr = x + (int64_t)b * x_stride;
    float* yr = y + (int64_t)b * y_stride + m;
    const int left = (int)min((int64_t)4, r.n_out - m);
    float o[4];
    if (r.Q == kTempoOne) {
        // tempo 1: the row as it is (n_out = N)
        if (VEC && left == 4) {
            *reinterpret_cast<float4v*>(yr) = *reinterpret_cast<const float4v*>(xr + m);
            return;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < left) yr[e] = xr[m + e];
        return;
    }
    const int H = r.H;
    const int64_t k = m / H;
    if (k >= starts_stride) return;  // (a segment the search had no room for: the host sizes starts for F + 1)
    const int i0 = (int)(m - k * H);
    const int* st = starts + (int64_t)b * starts_stride;
    const int64_t s0 = k == 0 ? -(int64_t)H : (int64_t)st[k - 1], s1 = st[k];
    const float h2 = (float)(2 * H);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int i = i0 + e;
        const int64_t p0 = s0 + H + i, p1 = s1 + i;
        const float x0 = (e < left && p0 >= 0 && p0 < r.N) ? xr[p0] : 0.f;
        const float x1 = (e < left && p1 >= 0 && p1 < r.N) ? xr[p1] : 0.f;
        const float w = __fdiv_rn((float)(2 * i + 1), h2), v = __fdiv_rn((float)(2 * (H - 1 - i) + 1), h2);
        o[e] = __fadd_rn(__fmul_rn(v, x0), __fmul_rn(w, x1));
    }
    if (VEC && left == 4) {
        *reinterpret_cast<float4v*>(yr) = float4v{o[0], o[1], o[2], o[3]};
        return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (e < left) yr[e] = o[e];
}

static bool tempo_call_ok(const TempoCall& c) {
    return c.x && c.lens && c.tempos && c.y && c.starts && c.x != c.y && c.batch >= 1 && c.x_stride >= 0 && c.y_stride >= 0 && c.max_out >= 0 && c.max_out <= INT32_MAX &&
           c.max_out <= c.y_stride && c.rate >= kTempoMinRate && c.rate <= kTempoMaxRate && c.starts_stride >= 1 && (!c.offsets || c.offsets_stride >= 0);
}

hipError_t launch_tempo_search(const TempoCall& c, hipStream_t s) {
    if (!tempo_call_ok(c)) return hipErrorInvalidValue;
    // the largest F of the call needs F + 1 starts and F offsets
    const int H = 4 * (c.rate / 400);
    const int64_t F = (c.max_out + H - 1) / H;
    if (c.starts_stride < F + 1 || (c.offsets && c.offsets_stride < F)) return hipErrorInvalidValue;
    const int threads = tempo_search_threads(c.rate);
    if (threads > TS_MAX_THREADS || TS_PER * threads < 2 * (4 * (c.rate / 500)) + 2 * H + 2) return hipErrorInvalidValue;  // (never at an admitted rate)
    VITS_KLAUNCH(tempo_search_kernel, dim3((unsigned)c.batch), dim3((unsigned)threads), 0, s, c.x, c.x_stride, c.lens, c.tempos, c.rate, c.starts, c.starts_stride, c.offsets,
                 c.offsets_stride, c.y_stride, c.lens_out);
    return hipGetLastError();
}

hipError_t launch_tempo_ola(const TempoCall& c, hipStream_t s) {
    if (!tempo_call_ok(c)) return hipErrorInvalidValue;
    const int H = 4 * (c.rate / 400);
    if (c.starts_stride < (c.max_out + H - 1) / H + 1) return hipErrorInvalidValue;
    const int64_t tiles = (c.max_out + kTempoTile - 1) / kTempoTile;
    if (tiles == 0) return hipSuccess;  // (every row empty: nothing to write)
    if ((int64_t)c.batch * tiles > INT32_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((int64_t)c.batch * tiles)), block(TO_THREADS);
    if ((((uintptr_t)c.x | (uintptr_t)c.y) & 15) == 0 && ((c.x_stride | c.y_stride) & 3) == 0)
        VITS_KLAUNCH((tempo_ola_kernel<true>), grid, block, 0, s, c.x, c.x_stride, c.lens, c.tempos, c.rate, c.starts, c.starts_stride, c.y, c.y_stride, (int)tiles);
    else
        VITS_KLAUNCH((tempo_ola_kernel<false>), grid, block, 0, s, c.x, c.x_stride, c.lens, c.tempos, c.rate, c.starts, c.starts_stride, c.y, c.y_stride, (int)tiles);
    return hipGetLastError();
}

}  // namespace vits
