// align.hip — forced alignment (include/vits.h vits_model_align_batch; engine_align.cpp): VITS monotonic alignment search between the text encoder's
// prior statistics per token (m, ls = logs_p) and z_p of a recording.
//
// align_planes_kernel + align_ct_kernel + align_logp_kernel: logp[t][j] = sum_c(-0.5 log 2pi - ls[c][t]) - 0.5 sum_c (z[c][j] - m[c][t])^2 exp(-2 ls[c][t]) in the expanded
// form: with s = exp(-2 ls), logp = c_t + sum_c s[c][t] (-0.5 z[c][j]^2) + sum_c (m s)[c][t] z[c][j]. align_planes_kernel writes the two operand planes
// (s | m s per token, -0.5 z^2 | z per frame, K = 2F rows each), align_ct_kernel c_t, once each; the product is one [T x 2F] . [2F x L] GEMM on v_mfma_f32_32x32x2_f32: one
// wave per 32 x 32 tile, K walked in ascending order, which is bit for bit a k-ordered fmaf chain per element, so an element does not depend on the batch or
// on the tile grid it was computed in. fp32 in every arithmetic mode (the result feeds comparisons; the operands span exp(-2 ls)).
//
// align_mas_kernel: the search (VITS maximum_path_each). Sequential in frames, parallel in tokens: one workgroup per utterance, token x = slot * nthreads + tid
// (TPL slots per lane: more than 1,024 tokens), the previous row v[y-1][.] in registers, the left neighbour by a wave shuffle and, for lane 0 of a wave,
// through a double-buffered LDS edge array written by lane 63 of the wave before: one barrier per frame. Every cell is one fp32 add and one fp32 max exactly as
// the definition writes them, so the result is independent of how tokens are spread over lanes. What is kept per (frame, token) is ONE bit, "the path came
// from the token before" (x != 0 && (x == y || v[y-1][x] < v[y-1][x-1])): a wave's ballot is 64 consecutive tokens of frame y's bitmap, in LDS when the
// bitmaps of all frames fit, in global memory otherwise. The backtrack runs in the same kernel on wave 0: per 64 frames, lane l fetches the two bitmap words
// of frame y0 - l that cover the 64 tokens the path can reach, then the walk itself reads them by lane broadcast: L dependent register steps, not L dependent
// memory reads.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernel_common.h"
#include "kernels.h"

namespace vits {

namespace {
constexpr float kAlignNeg = -1e9f;
}  // namespace

// planes: A [b][2F][t_stride] = s | m s (0 past the utterance's tokens), Z [b][2F][l_stride] = -0.5 z^2 | z (0 past its frames); blockIdx.z = a chunk of channels
__global__ __launch_bounds__(256) void align_planes_kernel(const float* __restrict__ m, int64_t m_bs, int m_cs, const float* __restrict__ ls, int64_t s_bs, int s_cs,
                                                           const float* __restrict__ z, int64_t z_bs, int z_cs, const int* __restrict__ tlens,
                                                           const int* __restrict__ frames, int F, int t_stride, int l_stride, float* __restrict__ A,
                                                           float* __restrict__ Z) {
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    const int T = tlens[b], L = frames[b];
    const int cpb = (F + gridDim.z - 1) / gridDim.z, c_lo = blockIdx.z * cpb, c_hi = min(F, c_lo + cpb);
    if (j < t_stride) {
        float* a = A + (int64_t)b * 2 * F * t_stride + j;
        for (int c = c_lo; c < c_hi; ++c) {
            float s = 0.f, ms = 0.f;
            if (j < T) {
                s = expf(-2.f * ls[(int64_t)b * s_bs + (int64_t)c * s_cs + j]);
                ms = m[(int64_t)b * m_bs + (int64_t)c * m_cs + j] * s;
            }
            a[(int64_t)c * t_stride] = s;
            a[(int64_t)(F + c) * t_stride] = ms;
        }
    }
    if (j < l_stride) {
        float* q = Z + (int64_t)b * 2 * F * l_stride + j;
        for (int c = c_lo; c < c_hi; ++c) {
            const float v = j < L ? z[(int64_t)b * z_bs + (int64_t)c * z_cs + j] : 0.f;
            q[(int64_t)c * l_stride] = -0.5f * v * v;
            q[(int64_t)(F + c) * l_stride] = v;
        }
    }
}

// ct [b][t_stride] = sum_c(-0.5 log 2pi - ls) + sum_c(-0.5 m^2 s), each sum in ascending c (one thread per token: the order is fixed), s read back from plane A
__global__ __launch_bounds__(64) void align_ct_kernel(const float* __restrict__ m, int64_t m_bs, int m_cs, const float* __restrict__ ls, int64_t s_bs, int s_cs,
                                                      const float* __restrict__ A, const int* __restrict__ tlens, int F, int t_stride, float* __restrict__ ct) {
    const int b = blockIdx.y, j = blockIdx.x * 64 + threadIdx.x;
    if (j >= t_stride) return;
    float c0 = 0.f, c1 = 0.f;
    if (j < tlens[b]) {
        const float* a = A + (int64_t)b * 2 * F * t_stride + j;
#pragma unroll 8
        for (int c = 0; c < F; ++c) {
            const float mu = m[(int64_t)b * m_bs + (int64_t)c * m_cs + j];
            c0 += -0.91893853320467274178f - ls[(int64_t)b * s_bs + (int64_t)c * s_cs + j];  // -0.5 log(2 pi)
            c1 += -0.5f * mu * mu * a[(int64_t)c * t_stride];
        }
    }
    ct[(int64_t)b * t_stride + j] = c0 + c1;
}

// one wave = one 32 (tokens) x 32 (frames) tile of logp [b][t_stride][l_stride]; K2 = 2F, ascending
__global__ __launch_bounds__(64) void align_logp_kernel(const float* __restrict__ A, const float* __restrict__ Z, const float* __restrict__ ct,
                                                        const int* __restrict__ tlens, const int* __restrict__ frames, int K2, int t_stride, int l_stride,
                                                        float* __restrict__ logp) {
    const int b = blockIdx.z, t0 = blockIdx.y * 32, j0 = blockIdx.x * 32, lane = threadIdx.x;
    const int T = tlens[b], L = frames[b];
    if (t0 >= T || j0 >= L) return;
    // operand lane maps of v_mfma_f32_32x32x2_f32: A[i = lane & 31][k = lane >> 5], B[k = lane >> 5][j = lane & 31]
    const float* ap = A + ((int64_t)b * K2 + (lane >> 5)) * t_stride + t0 + (lane & 31);
    const float* zp = Z + ((int64_t)b * K2 + (lane >> 5)) * l_stride + j0 + (lane & 31);
    floatx16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int k = 0;
    for (; k + 8 <= K2; k += 8) {  // (four steps' operands in flight; the accumulation order stays k ascending)
        float a[4], q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a[u] = ap[(int64_t)(k + 2 * u) * t_stride];
            q[u] = zp[(int64_t)(k + 2 * u) * l_stride];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], q[u], acc, 0, 0, 0);
    }
    for (; k < K2; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[(int64_t)k * t_stride], zp[(int64_t)k * l_stride], acc, 0, 0, 0);
    // C/D map: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const int j = j0 + (lane & 31);
    if (j >= L) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int t = t0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (t < T) logp[((int64_t)b * t_stride + t) * l_stride + j] = ct[(int64_t)b * t_stride + t] + acc[r];
    }
}

template <int TPL>
__global__ __launch_bounds__(1024) void align_mas_kernel(const float* __restrict__ logp, int t_stride, int l_stride, const int* __restrict__ tlens,
                                                         const int* __restrict__ frames, unsigned long long* __restrict__ gbits, int64_t gbits_bs,
                                                         int* __restrict__ dur, int dur_stride, float* __restrict__ path, int path_stride,
                                                         float* __restrict__ score) {
    extern __shared__ unsigned long long align_smem[];  // [bitmaps: L x W words, when they live in LDS] | edge [2][TPL][waves] floats
    const int b = blockIdx.x, tid = threadIdx.x, nthreads = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nthreads >> 6;
    const int T = tlens[b], L = frames[b];
    const int W = TPL * nw;  // 64-bit words of one frame's bitmap: word slot * nw + wave = tokens [64 word, 64 word + 64)
    int* d = dur + (int64_t)b * dur_stride;
    const bool bad = T <= 0 || L <= 0 || T > L;  // (refused on the host; never walked here)
    for (int t = (bad ? 0 : T) + tid; t < dur_stride; t += nthreads) d[t] = 0;
    if (bad) {
        if (tid == 0) score[b] = kAlignNeg;
        return;
    }
    unsigned long long* bits = gbits ? gbits + (int64_t)b * gbits_bs : align_smem;
    float* edge = reinterpret_cast<float*>(gbits ? align_smem : align_smem + (size_t)L * W);
    for (int i = tid; i < 2 * W; i += nthreads) edge[i] = kAlignNeg;
    float v[TPL];
    const float* row[TPL];
    float4 cur[TPL], nxt[TPL];
#pragma unroll
    for (int i = 0; i < TPL; ++i) {
        v[i] = kAlignNeg;
        const int x = i * nthreads + tid;
        row[i] = logp + ((int64_t)b * t_stride + min(x, T - 1)) * l_stride;  // (lanes past the last token read its row and never use it)
        nxt[i] = *reinterpret_cast<const float4*>(row[i]);
        cur[i] = nxt[i];
    }
    __syncthreads();
    for (int y = 0; y < L; ++y) {
        if ((y & 3) == 0) {
            // four frames of every token's row at a time, the next four in flight (rows are l_stride >= round_up(L, 4) long)
#pragma unroll
            for (int i = 0; i < TPL; ++i) {
                cur[i] = nxt[i];
                if (y + 4 < L) nxt[i] = *reinterpret_cast<const float4*>(row[i] + y + 4);
            }
        }
        const int lo = max(0, T + y - L), hi = min(T - 1, y);
        const float* e_prev = edge + ((y + 1) & 1) * W;  // v[y-1] of every wave's last lane
        float* e_cur = edge + (y & 1) * W;
        float left[TPL];
#pragma unroll
        for (int i = 0; i < TPL; ++i) {
            left[i] = __shfl_up(v[i], 1);
            if (lane == 0) left[i] = wave > 0 ? e_prev[i * nw + wave - 1] : (i > 0 ? e_prev[(i - 1) * nw + nw - 1] : kAlignNeg);
        }
#pragma unroll
        for (int i = 0; i < TPL; ++i) {
            const int x = i * nthreads + tid;
            const bool in = x >= lo && x <= hi;
            const float lp = (y & 3) == 0 ? cur[i].x : (y & 3) == 1 ? cur[i].y : (y & 3) == 2 ? cur[i].z : cur[i].w;
            const float c = x == y ? kAlignNeg : v[i];
            const float p = x == 0 ? (y == 0 ? 0.f : kAlignNeg) : left[i];
            const bool down = in && x != 0 && (x == y || c < p);
            if (in) v[i] = lp + fmaxf(p, c);
            const unsigned long long word = __ballot(down);
            if (lane == 0) bits[(int64_t)y * W + i * nw + wave] = word;
            if (lane == 63) e_cur[i * nw + wave] = v[i];
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < TPL; ++i)
        if (i * nthreads + tid == T - 1) score[b] = v[i];
    if (wave != 0) return;
    // backtrack (wave 0; every lane walks the same path, lane 0 stores): frame y belongs to token x, then x steps down iff its bit is set
    float* pth = path ? path + (int64_t)b * path_stride : nullptr;
    int x = T - 1, cnt = 0;
    for (int y0 = L - 1; y0 >= 0; y0 -= 64) {
        const int y = y0 - lane, wi = x >> 6;
        unsigned long long w_hi = 0, w_lo = 0;
        if (y >= 0) {
            w_hi = bits[(int64_t)y * W + wi];
            if (wi > 0) w_lo = bits[(int64_t)y * W + wi - 1];
        }
        const int n = min(64, y0 + 1);
        for (int s = 0; s < n; ++s) {
            // the path drops at most one token per frame: over these 64 frames it stays inside the two words fetched
            const int rel = x - ((wi - 1) << 6);  // in [1, 127]
            const unsigned long long h = __shfl(w_hi, s), l = __shfl(w_lo, s);
            const int bit = (int)((rel >= 64 ? h >> (rel - 64) : l >> rel) & 1ull);
            if (lane == 0 && pth) pth[y0 - s] = (float)x;
            ++cnt;
            if (bit) {
                if (lane == 0) d[x] = cnt;
                cnt = 0;
                --x;
            }
        }
    }
    if (lane == 0) d[x] = cnt;
}

hipError_t launch_align_logp(const AlignCall& c, hipStream_t s) {
    if (c.batch <= 0 || c.tmax <= 0 || c.lmax <= 0) return hipSuccess;
    if ((c.t_stride & 31) || (c.l_stride & 31) || c.t_stride < c.tmax || c.l_stride < c.lmax || (c.channels < 1)) return hipErrorInvalidValue;
    dim3 gp((std::max(c.t_stride, c.l_stride) + 255) / 256, c.batch, std::min(c.channels, 32));
    VITS_KLAUNCH(align_planes_kernel, gp, dim3(256), 0, s, c.mean.p, c.mean.bs, c.mean.cs, c.logs.p, c.logs.bs, c.logs.cs, c.z.p, c.z.bs, c.z.cs, c.tlens, c.frames,
                 c.channels, c.t_stride, c.l_stride, c.plane_a, c.plane_z);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    VITS_KLAUNCH(align_ct_kernel, dim3((c.t_stride + 63) / 64, c.batch), dim3(64), 0, s, c.mean.p, c.mean.bs, c.mean.cs, c.logs.p, c.logs.bs, c.logs.cs, c.plane_a,
                 c.tlens, c.channels, c.t_stride, c.ct);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    dim3 grid((c.lmax + 31) / 32, (c.tmax + 31) / 32, c.batch);
    VITS_KLAUNCH(align_logp_kernel, grid, dim3(64), 0, s, c.plane_a, c.plane_z, c.ct, c.tlens, c.frames, 2 * c.channels, c.t_stride, c.l_stride, c.logp);
    return hipGetLastError();
}

// tokens per lane, threads per block and 64-bit words per frame bitmap of a search over at most tmax tokens
static void align_mas_shape(int tmax, int& tpl, int& threads, int& words) {
    tpl = (tmax + 1023) / 1024;
    threads = ((tmax + tpl - 1) / tpl + 63) / 64 * 64;
    words = tpl * (threads / 64);
}

size_t align_mas_bits_words(int tmax, int lmax) {
    int tpl, threads, words;
    align_mas_shape(tmax, tpl, threads, words);
    return (size_t)words * (size_t)lmax;
}

bool align_mas_bits_in_lds(int tmax, int lmax) { return align_mas_bits_words(tmax, lmax) * 8 <= kAlignLdsBitBytes; }

hipError_t launch_align_mas(const AlignCall& c, hipStream_t s) {
    if (c.batch <= 0) return hipSuccess;
    if (c.tmax <= 0 || c.lmax <= 0 || c.tmax > 4096 || (c.l_stride & 3) || c.l_stride < c.lmax || c.dur_stride < c.tmax) return hipErrorInvalidValue;
    int tpl, threads, words;
    align_mas_shape(c.tmax, tpl, threads, words);
    const bool in_lds = align_mas_bits_in_lds(c.tmax, c.lmax);
    if (!in_lds && !c.bits) return hipErrorInvalidValue;
    const size_t lds = (in_lds ? (size_t)words * c.lmax * 8 : 0) + (size_t)2 * words * sizeof(float);
    unsigned long long* gb = in_lds ? nullptr : c.bits;
    const int64_t gb_bs = (int64_t)words * c.lmax;
#define VITS_ALIGN_MAS(N)                                                                                                                              \
    return launch_lds<&align_mas_kernel<N>>(dim3(c.batch), dim3(threads), lds, s, c.logp, c.t_stride, c.l_stride, c.tlens, c.frames, gb, gb_bs, c.dur, c.dur_stride, c.path, \
                                            c.l_stride, c.score)
    switch (tpl) {
        case 1: VITS_ALIGN_MAS(1);
        case 2: VITS_ALIGN_MAS(2);
        case 3: VITS_ALIGN_MAS(3);
        default: VITS_ALIGN_MAS(4);
    }
#undef VITS_ALIGN_MAS
}

}  // namespace vits
