// fit.hip — a stated duration: the length scale of a group of utterances fitted to a target frame count (include/vits.h "a stated duration"; the definition
// and the operands: kernels.h FitCall; DESIGN.md §8 "A stated duration"). One kernel, queued directly in front of durations_kernel, which then takes the rows
// this one writes as its override rows: nothing behind it knows that a fit happened.
//
// Block = one group, 256 threads. Every utterance belongs to exactly one group, so its row of e and its row of dur are written by exactly one block, and no
// block reads what another wrote: no atomics, no traffic between blocks. A thread owns the tokens t = tid, tid + 256, ... of every member: it writes
// e_t = expf(logw_t) (the expression durations_kernel evaluates) once and reads back only what it wrote itself, 4 bytes a token from L2 in each of the at most
// 26 + 4 sums of a search. A sum is the threads' int64 partials reduced inside each wave and the four wave totals added through LDS; integers, so the order
// does not matter. Every decision of the search follows from such a sum, which every thread holds: the control flow is block-uniform throughout.
//
// The remainder (R frames, non-zero only where several tokens step at the same float) goes to the free tokens in (utterance, token) order: an exclusive
// block scan of the tokens' gains c_t(next s) - c_t(s*) over 256 consecutive tokens at a time, the running total carried from one piece to the next, and
// every piece behind the one that uses up R skipped. Nothing behind lens[b] is read.
//
// No matrix-core work, and none to be had: one multiply, one ceil and one 64-bit add per token and step. Latency-bound by construction (two barriers a sum).
#include <hip/hip_runtime.h>

#include "kernel_common.h"
#include "kernels.h"

namespace vits {

constexpr int FIT_THREADS = 256;
constexpr int FIT_WAVES = FIT_THREADS / 64;

__device__ __forceinline__ long long fit_token_frames(float e, float s) {
    const float x = ceilf(e * s);
    return x < kFitMaxTokenFrames ? (long long)x : (long long)kFitMaxTokenFrames;
}

// the block's sum of v, in every thread (part: FIT_WAVES values of LDS; two barriers, so that the next call may write part again)
__device__ __forceinline__ long long fit_block_sum(long long v, long long* part) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    if (lane == 0) part[wave] = v;
    __syncthreads();
    long long sum = 0;
    for (int w = 0; w < FIT_WAVES; ++w) sum += part[w];
    __syncthreads();
    return sum;
}

// the sum of v over the threads in front of this one, and the block's total
__device__ __forceinline__ long long fit_block_scan(long long v, long long* part, long long& total) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    long long inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const long long up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    long long before = 0;
    total = 0;
    for (int w = 0; w < FIT_WAVES; ++w) {
        if (w < wave) before += part[w];
        total += part[w];
    }
    __syncthreads();
    return before + inc - v;
}

__global__ __launch_bounds__(FIT_THREADS) void fit_durations_kernel(const float* __restrict__ logw, int64_t l_bs, int l_cs, int c, const int* __restrict__ lens,
                                                                    const int* __restrict__ fixed, const int* __restrict__ group,
                                                                    const int* __restrict__ target, float s_lo, float s_hi, float* __restrict__ e,
                                                                    int* __restrict__ dur, int64_t* __restrict__ rows, int batch, int tmax) {
    __shared__ long long part[FIT_WAVES];
    const int g = (int)blockIdx.x, tid = (int)threadIdx.x;
    const long long F = target[g];
    auto member = [&](int b) { return (group ? group[b] : b) == g; };
    auto len_of = [&](int b) { return lens ? min(max(lens[b], 0), tmax) : tmax; };

    // pass 1: e of every member's tokens; -1 behind every length; the caller's rows through unchanged where the group is not fitted
    int members = 0;
    for (int b = 0; b < batch; ++b) {
        if (!member(b)) continue;
        ++members;
        const int len = len_of(b);
        const int64_t row = (int64_t)b * tmax;
        for (int t = tid; t < tmax; t += FIT_THREADS) {
            if (t < len) {
                e[row + t] = expf(logw[(int64_t)b * l_bs + (int64_t)c * l_cs + t]);
                if (F == 0) dur[row + t] = fixed ? fixed[row + t] : -1;
            } else
                dur[row + t] = -1;
        }
    }
    if (F == 0 || members == 0) {
        if (tid == 0) {
            int64_t* r = rows + (int64_t)kFitRowInts * g;
            r[0] = F, r[1] = 0, r[2] = 0, r[3] = 0, r[4] = -1;
        }
        return;
    }

    // (a thread reads the e it wrote itself: the same t of the same rows)
    auto frames_at = [&](int64_t i, float s) -> long long {
        const int v = fixed ? fixed[i] : -1;
        return v >= 0 ? (long long)v : fit_token_frames(e[i], s);
    };
    auto n_of = [&](float s) {
        long long n = 0;
        for (int b = 0; b < batch; ++b) {
            if (!member(b)) continue;
            const int len = len_of(b);
            for (int t = tid; t < len; t += FIT_THREADS) n += frames_at((int64_t)b * tmax + t, s);
        }
        return fit_block_sum(n, part);
    };

    unsigned lo = __float_as_uint(s_lo), hi = __float_as_uint(s_hi);
    long long status = 0;
    bool remainder = false;
    if (n_of(s_lo) > F) {
        status = 1;
    } else {
        const long long n_hi = n_of(s_hi);
        if (n_hi <= F) {
            lo = hi;
            status = n_hi == F ? 0 : 2;
        } else {
            // n(lo) <= F < n(hi) throughout
            while (hi - lo > 1) {
                const unsigned mid = lo + (hi - lo) / 2;
                if (n_of(__uint_as_float(mid)) <= F) lo = mid;
                else hi = mid;
            }
            remainder = true;
        }
    }
    const float s = __uint_as_float(lo), s_next = __uint_as_float(lo + 1);
    long long sum = n_of(s);
    const long long R = remainder ? F - sum : 0;

    // the result: c_t(s*), and the remainder in (utterance, token) order
    long long given = 0;  // frames of the remainder handed to the tokens in front of the piece at hand (block-uniform)
    for (int b = 0; b < batch; ++b) {
        if (!member(b)) continue;
        const int len = len_of(b);
        for (int t0 = 0; t0 < len; t0 += FIT_THREADS) {
            const int t = t0 + tid;
            const int64_t i = (int64_t)b * tmax + t;
            long long d = 0, gain = 0;
            if (t < len) {
                d = frames_at(i, s);
                if (given < R) gain = frames_at(i, s_next) - d;
            }
            if (given < R) {  // (block-uniform)
                long long total;
                const long long before = given + fit_block_scan(gain, part, total);
                if (before < R) d += min(gain, R - before);
                given = min(given + total, R);
            }
            if (t < len) dur[i] = (int)d;
        }
    }
    if (tid == 0) {
        int64_t* r = rows + (int64_t)kFitRowInts * g;
        r[0] = F, r[1] = sum + given, r[2] = (int64_t)lo, r[3] = R, r[4] = status;
    }
}

hipError_t launch_fit_durations(const FitCall& c, hipStream_t s) {
    if (c.batch < 1 || c.tmax < 1 || !c.logw.p || !c.g.target || !c.e || !c.dur || !c.rows) return hipErrorInvalidValue;
    VITS_KLAUNCH(fit_durations_kernel, dim3(c.batch), dim3(FIT_THREADS), 0, s, c.logw.p, c.logw.bs, c.logw.cs, c.c, c.lens, c.fixed, c.g.group, c.g.target, c.g.s_lo,
                 c.g.s_hi, c.e, c.dur, c.rows, c.batch, c.tmax);
    return hipGetLastError();
}

}  // namespace vits
