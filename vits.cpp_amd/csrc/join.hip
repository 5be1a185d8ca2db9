// join.hip — joined tracks: the utterances of a ragged batch laid end to end (include/vits.h "joined tracks", vits_op_join; DESIGN.md §8 "Joined
// tracks"). The definition is stated in include/vits.h; the tracks, gaps, bounds and the table come from join_host.cpp.
//   join_offsets_kernel   one block per track, one lane walks the track's utterances in order (B is small, and integer sums do not round):
//                         n_b = lens[b] clamped to [0, ubound_b], o_b, T_g -> rows[b] = {o_b, n_b}, track_lens[g] = T_g.
//   join_apply_kernel     grid (tiles of the largest bound, G). A block owns kJoinTile consecutive samples of ONE track. The ends o_b + n_b are non-decreasing
//                         along a track: a binary search (block-uniform, at most 17 steps) finds the first utterance that reaches the tile; the block then walks
//                         forward until an utterance begins behind the tile (the o_b are non-decreasing too). A thread holds its 4 samples in registers: the
//                         first utterance that covers one is copied, the second (its neighbour: the half rule allows no third) is added, one fp32 add.
//                         Every sample of [0, bound_g) is written once: +0 where nothing covers it. Lane l reads x_b[j - o_b] for consecutive j: coalesced
//                         4-byte traffic whatever o_b is; the walk is block-uniform, so only the two range tests diverge, at an utterance's edges.
// Plain vector loads and stores, no atomics, bounded loops; only a copy and one add touch a sample: batch position, track partition, tiles and streams enter no bit.
#include <hip/hip_runtime.h>

#include <climits>

#include "../../include/vits.h"
#include "kernel_common.h"
#include "kernels.h"

namespace vits {

constexpr int JN_THREADS = 256, JN_SPT = kJoinTile / JN_THREADS;
static_assert(kJoinTile % JN_THREADS == 0 && JN_SPT <= 32, "a thread's samples fit its coverage mask");

__global__ __launch_bounds__(64) void join_offsets_kernel(const int* __restrict__ lens, const int64_t* __restrict__ table, int B, int64_t* __restrict__ rows,
                                                           int* __restrict__ track_lens) {
    if (threadIdx.x != 0) return;
    const int g = (int)blockIdx.x;
    const int64_t* tr = table + (int64_t)2 * B + (int64_t)3 * g;
    const int first = (int)tr[0], end = (int)tr[1];  // 0 <= first < end <= B: join_call_ok
    int64_t o = 0, n_prev = 0;
    for (int b = first; b < end; ++b) {
        const int64_t n = min((int64_t)max(lens[b], 0), table[(int64_t)2 * b + 1]);
        if (b > first) {
            const int64_t gb = table[(int64_t)2 * b];
            o += n_prev + (gb >= 0 ? gb : -min(-gb, min(n_prev / 2, n / 2)));
        }
        rows[(int64_t)2 * b] = o, rows[(int64_t)2 * b + 1] = n;
        n_prev = n;
    }
    track_lens[g] = (int)(o + n_prev);  // T_g <= bound_g <= 2^30: the host checked the bounds
}

__global__ __launch_bounds__(JN_THREADS) void join_apply_kernel(const float* __restrict__ x, int64_t x_stride, float* __restrict__ y, int64_t y_stride,
                                                                 const int64_t* __restrict__ table, int B, const int64_t* __restrict__ rows) {
    const int g = (int)blockIdx.y, tid = (int)threadIdx.x;
    const int64_t* tr = table + (int64_t)2 * B + (int64_t)3 * g;
    const int first = (int)tr[0], end = (int)tr[1];
    const int64_t bound = tr[2];  // <= y_stride: the host checked it
    const int64_t j0 = (int64_t)blockIdx.x * kJoinTile;
    if (j0 >= bound) return;  // (block-uniform)
    const int64_t j1 = min(j0 + kJoinTile, bound);
    // the first utterance whose end lies behind j0 (ends non-decreasing); end - first <= 65535: 17 halvings at the most
    int lo = first, hi = end;
    for (int it = 0; it < 17 && lo < hi; ++it) {
        const int mid = lo + (hi - lo) / 2;
        if (rows[(int64_t)2 * mid] + rows[(int64_t)2 * mid + 1] > j0) hi = mid;
        else lo = mid + 1;
    }
    float v[JN_SPT];
#pragma unroll
    for (int it = 0; it < JN_SPT; ++it) v[it] = 0.f;
    unsigned covered = 0;
    for (int b = lo; b < end; ++b) {
        const int64_t o = rows[(int64_t)2 * b], n = rows[(int64_t)2 * b + 1];  // 0 <= n <= ubound_b <= x_stride: join_offsets_kernel
        if (o >= j1) break;                                                     // (the o_b are non-decreasing: nothing behind b begins inside the tile)
        const float* xr = x + (int64_t)b * x_stride;
#pragma unroll
        for (int it = 0; it < JN_SPT; ++it) {
            const int64_t k = j0 + it * JN_THREADS + tid - o;
            if (k >= 0 && k < n) {
                const float xv = xr[k];
                v[it] = (covered >> it) & 1u ? v[it] + xv : xv;
                covered |= 1u << it;
            }
        }
    }
    float* yr = y + (int64_t)g * y_stride;
#pragma unroll
    for (int it = 0; it < JN_SPT; ++it) {
        const int64_t j = j0 + it * JN_THREADS + tid;
        if (j < bound) yr[j] = v[it];
    }
}

namespace {
// what both launches rely on; the kernels index with the table made from this plan and check nothing again
bool join_call_ok(const JoinCall& c) {
    if (!c.plan || !c.x || !c.y || c.x == c.y || !c.lens || !c.table || ((uintptr_t)c.table & 7) || !c.rows || !c.track_lens) return false;
    const JoinPlan& p = *c.plan;
    if (p.batch < 1 || p.batch > 65535 || p.tracks < 1 || p.tracks > p.batch || (int)p.first.size() != p.tracks + 1 || (int)p.gap.size() != p.batch ||
        (int)p.ubound.size() != p.batch || (int)p.bound.size() != p.tracks || p.first[0] != 0 || p.first[(size_t)p.tracks] != p.batch)
        return false;
    int64_t mu = 0, mt = 0;
    for (int g = 0; g < p.tracks; ++g) {
        if (p.first[(size_t)g] >= p.first[(size_t)g + 1]) return false;  // (every track holds an utterance)
        int64_t sum = 0;
        for (int b = p.first[(size_t)g]; b < p.first[(size_t)g + 1]; ++b) {
            if (p.ubound[(size_t)b] < 0 || p.ubound[(size_t)b] > kEdgesMaxLen) return false;
            mu = std::max(mu, p.ubound[(size_t)b]);
            sum += p.ubound[(size_t)b] + std::max<int64_t>(p.gap[(size_t)b], 0);
        }
        if (sum != p.bound[(size_t)g] || sum > kEdgesMaxLen) return false;  // (T_g <= bound_g holds for the sum, not for a smaller number)
        mt = std::max(mt, sum);
    }
    return mu == p.max_ubound && mt == p.max_bound && mu <= c.x_stride && mt <= c.y_stride;
}
}  // namespace

hipError_t launch_join_offsets(const JoinCall& c, hipStream_t s) {
    if (!join_call_ok(c)) return hipErrorInvalidValue;
    VITS_KLAUNCH(join_offsets_kernel, dim3((unsigned)c.plan->tracks), dim3(64), 0, s, c.lens, c.table, c.plan->batch, c.rows, c.track_lens);
    return hipGetLastError();
}

hipError_t launch_join_apply(const JoinCall& c, hipStream_t s) {
    if (!join_call_ok(c)) return hipErrorInvalidValue;
    const int64_t tiles = (c.plan->max_bound + kJoinTile - 1) / kJoinTile;
    if (tiles == 0) return hipSuccess;
    if (tiles > INT32_MAX) return hipErrorInvalidValue;
    VITS_KLAUNCH(join_apply_kernel, dim3((unsigned)tiles, (unsigned)c.plan->tracks), dim3(JN_THREADS), 0, s, c.x, c.x_stride, c.y, c.y_stride, c.table, c.plan->batch,
                 c.rows);
    return hipGetLastError();
}

}  // namespace vits
