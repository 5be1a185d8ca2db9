// edges.hip — stated edges on a ragged batch of PCM rows: trimmed silence, pauses and fades (include/vits.h vits_model_set_edges / vits_op_edges;
// DESIGN.md §8 "Stated edges"). The definition is stated in include/vits.h; the counts and the fade tables come from edges_host.cpp.
//   edges_window_kernel   grid (tiles, B). A tile is plan.tile = (4096 / W) W consecutive samples of ONE row, anchored at the row's sample 0: a multiple of
//                         the window, so no window straddles two tiles. The tile's samples inside [0, len) are staged in LDS; a wave takes the tile's
//                         windows w, w + 4, ..: lane l adds the squares (exact in fp64) of the window's samples l, l + 64, .. in ascending order, the 64
//                         partial sums meet in a butterfly (xor 32 .. 1: every lane holds the same bits), q_i = sum / count goes to the scratch.
//   edges_bounds_kernel   one block per row: q_max by a fixed-shape tree (a maximum does not round; fmax drops a NaN), T, the first and the last active
//                         window as a min / max over indices, their count as an integer sum -> rows[b] = {a, b, N', n_active} and lens_out[b] = N'.
//                         VITS_EDGES_PAD reads no q: a = 0, b = len.
//   edges_apply_kernel    grid (tiles of the bound, B): y[j] for j in [0, len + Pl + Pt): +0 in the pads and behind N', (x[a + k] * wi) * wo between.
// Plain vector loads and stores, no atomics; only maxima, minima and integer counts cross a window: batch position, grid and stream enter no bit.
#include <hip/hip_runtime.h>

#include <climits>

#include "../../include/vits.h"
#include "kernel_common.h"
#include "kernels.h"

namespace vits {

constexpr int ED_THREADS = 256, ED_WAVES = ED_THREADS / 64;
constexpr int ED_APPLY_SPT = kEdgesApplyTile / ED_THREADS;
static_assert(kEdgesApplyTile % ED_THREADS == 0 && kEdgesTileTarget * 4 <= 64 * 1024, "a staged tile fits the static LDS of a block");

__global__ __launch_bounds__(ED_THREADS) void edges_window_kernel(const float* __restrict__ x, int64_t x_stride, const int* __restrict__ lens, int64_t n_cap, int W,
                                                                  int tile, double* __restrict__ q, int64_t q_stride) {
    __shared__ float xs[kEdgesTileTarget];
    const int b = (int)blockIdx.y, tid = (int)threadIdx.x;
    const int64_t N = min((int64_t)max(lens[b], 0), n_cap);
    const int64_t t0 = (int64_t)blockIdx.x * tile;
    if (t0 >= N) return;  // (block-uniform)
    const int cnt = (int)min((int64_t)tile, N - t0);  // <= tile <= kEdgesTileTarget: the host checked the plan
    const float* xr = x + (int64_t)b * x_stride + t0;
    for (int i = tid; i < cnt; i += ED_THREADS) xs[i] = xr[i];
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    const int nw = (cnt + W - 1) / W;
    double* qr = q + (int64_t)b * q_stride + t0 / W;
    for (int w = wave; w < nw; w += ED_WAVES) {  // (wave-uniform)
        const int n = min(W, cnt - w * W);
        const float* p = xs + w * W;
        double acc = 0.0;
        for (int k = lane; k < n; k += 64) {
            const double v = (double)p[k];
            acc += v * v;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == 0) qr[w] = acc / (double)n;
    }
}

__global__ __launch_bounds__(ED_THREADS) void edges_bounds_kernel(const int* __restrict__ lens, int64_t n_cap, const double* __restrict__ q, int64_t q_stride, int mode,
                                                                  int W, double f, int64_t Kh, int64_t Kt, int64_t Pl, int64_t Pt, int* __restrict__ lens_out,
                                                                  int64_t* __restrict__ rows) {
    __shared__ double redd[ED_THREADS];
    __shared__ int redi[3][ED_THREADS];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int64_t N = min((int64_t)max(lens[b], 0), n_cap);
    int64_t a = 0, e = 0, n_active = 0;
    if (mode == VITS_EDGES_PAD) e = N;
    else {
        const int n_win = (int)((N + W - 1) / W);
        const double* qr = q + (int64_t)b * q_stride;
        double m = 0.0;
        for (int i = tid; i < n_win; i += ED_THREADS) m = fmax(m, qr[i]);
        redd[tid] = m;
        __syncthreads();
        for (int w = ED_THREADS / 2; w > 0; w >>= 1) {
            if (tid < w) redd[tid] = fmax(redd[tid], redd[tid + w]);
            __syncthreads();
        }
        const double T = mode == VITS_EDGES_TRIM_RELATIVE ? redd[0] * f : f;
        int first = INT_MAX, last = -1, cnt = 0;
        for (int i = tid; i < n_win; i += ED_THREADS) {
            const double v = qr[i];
            if (v >= T && v > 0.0) {
                first = min(first, i);
                last = max(last, i);
                ++cnt;
            }
        }
        redi[0][tid] = first, redi[1][tid] = last, redi[2][tid] = cnt;
        __syncthreads();
        for (int w = ED_THREADS / 2; w > 0; w >>= 1) {
            if (tid < w) {
                redi[0][tid] = min(redi[0][tid], redi[0][tid + w]);
                redi[1][tid] = max(redi[1][tid], redi[1][tid + w]);
                redi[2][tid] += redi[2][tid + w];
            }
            __syncthreads();
        }
        n_active = redi[2][0];
        if (n_active > 0) {
            a = max((int64_t)0, (int64_t)redi[0][0] * W - Kh);
            e = min(N, ((int64_t)redi[1][0] + 1) * W + Kt);
        }
    }
    if (tid == 0) {
        const int64_t np = Pl + (e - a) + Pt;  // <= 2^30 + 2 * 384000: the host checked the lengths
        int64_t* r = rows + (int64_t)b * 4;
        r[0] = a, r[1] = e, r[2] = np, r[3] = n_active;
        lens_out[b] = (int)np;
    }
}

__global__ __launch_bounds__(ED_THREADS) void edges_apply_kernel(const float* __restrict__ x, int64_t x_stride, float* __restrict__ y, int64_t y_stride,
                                                                 const int* __restrict__ lens, int64_t n_cap, const int64_t* __restrict__ rows,
                                                                 const float* __restrict__ fades, int64_t Fi, int64_t Fo, int64_t Pl, int64_t Pt) {
    const int b = (int)blockIdx.y, tid = (int)threadIdx.x;
    const int64_t N = min((int64_t)max(lens[b], 0), n_cap);
    const int64_t bound = N + Pl + Pt;  // <= y_stride: the host checked it against the longest row
    const int64_t j0 = (int64_t)blockIdx.x * kEdgesApplyTile;
    if (j0 >= bound) return;
    const int64_t a = rows[(int64_t)b * 4], M = rows[(int64_t)b * 4 + 1] - a;  // 0 <= a, a + M <= N: edges_bounds_kernel
    const float* xr = x + (int64_t)b * x_stride + a;
    float* yr = y + (int64_t)b * y_stride;
#pragma unroll
    for (int it = 0; it < ED_APPLY_SPT; ++it) {
        const int64_t j = j0 + it * ED_THREADS + tid;
        if (j >= bound) continue;
        const int64_t k = j - Pl;
        float v = 0.f;
        if (k >= 0 && k < M) {
            const int64_t r = M - 1 - k;
            const float wi = k < Fi ? fades[k] : 1.f, wo = r < Fo ? fades[Fi + r] : 1.f;
            v = xr[k] * wi;
            v = v * wo;
        }
        yr[j] = v;
    }
}

namespace {
// what every launch below relies on; the kernels index with these and check nothing again
bool edges_call_ok(const EdgesCall& c) {
    const EdgesPlan& p = c.plan;
    const bool measures = p.mode == VITS_EDGES_TRIM_RELATIVE || p.mode == VITS_EDGES_TRIM_ABSOLUTE;
    return c.x && c.y && c.x != c.y && c.lens && c.lens_out && c.rows && c.batch >= 1 && c.batch <= 65535 && c.max_len >= 0 && c.max_len <= kEdgesMaxLen &&
           c.max_len <= c.x_stride && (measures || p.mode == VITS_EDGES_PAD) && p.W >= 1 && p.tile >= p.W && p.tile % p.W == 0 && p.tile <= kEdgesTileTarget &&
           p.Kh >= 0 && p.Kt >= 0 && p.Fi >= 0 && p.Fo >= 0 && p.Pl >= 0 && p.Pt >= 0 && p.bound(c.max_len) <= c.y_stride && (c.fades || p.Fi + p.Fo == 0) &&
           (!measures || (c.scratch && ((uintptr_t)c.scratch & 7) == 0));
}
int64_t q_stride_of(const EdgesCall& c) { return (c.max_len + c.plan.W - 1) / c.plan.W + 1; }  // (the carving edges_scratch_bytes sizes)
}  // namespace

hipError_t launch_edges_window(const EdgesCall& c, hipStream_t s) {
    if (!edges_call_ok(c)) return hipErrorInvalidValue;
    if (c.plan.mode == VITS_EDGES_PAD || c.max_len == 0) return hipSuccess;
    const int64_t tiles = (c.max_len + c.plan.tile - 1) / c.plan.tile;
    if (tiles > INT32_MAX) return hipErrorInvalidValue;
    VITS_KLAUNCH(edges_window_kernel, dim3((unsigned)tiles, (unsigned)c.batch), dim3(ED_THREADS), 0, s, c.x, c.x_stride, c.lens, c.max_len, c.plan.W, c.plan.tile,
                 reinterpret_cast<double*>(c.scratch), q_stride_of(c));
    return hipGetLastError();
}

hipError_t launch_edges_bounds(const EdgesCall& c, hipStream_t s) {
    if (!edges_call_ok(c)) return hipErrorInvalidValue;
    const EdgesPlan& p = c.plan;
    VITS_KLAUNCH(edges_bounds_kernel, dim3((unsigned)c.batch), dim3(ED_THREADS), 0, s, c.lens, c.max_len, reinterpret_cast<const double*>(c.scratch), q_stride_of(c), p.mode,
                 p.W, p.f, p.Kh, p.Kt, p.Pl, p.Pt, c.lens_out, c.rows);
    return hipGetLastError();
}

hipError_t launch_edges_apply(const EdgesCall& c, hipStream_t s) {
    if (!edges_call_ok(c)) return hipErrorInvalidValue;
    const EdgesPlan& p = c.plan;
    const int64_t tiles = (p.bound(c.max_len) + kEdgesApplyTile - 1) / kEdgesApplyTile;
    if (tiles == 0) return hipSuccess;
    if (tiles > INT32_MAX) return hipErrorInvalidValue;
    VITS_KLAUNCH(edges_apply_kernel, dim3((unsigned)tiles, (unsigned)c.batch), dim3(ED_THREADS), 0, s, c.x, c.x_stride, c.y, c.y_stride, c.lens, c.max_len, c.rows, c.fades,
                 p.Fi, p.Fo, p.Pl, p.Pt);
    return hipGetLastError();
}

}  // namespace vits
