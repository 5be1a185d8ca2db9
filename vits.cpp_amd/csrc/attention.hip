// attention.hip — the text encoder's windowed relative-position self-attention (vits.cpp:296-356; helpers :195-235): the VALU kernel, the matrix-core
// kernel with its SHORT / LAT variants, and launch_rel_attention (which of them a launch takes: plan_rel_attention, launch_plan.cpp).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernel_common.h"
#include "kernels.h"
#include "phase_timing.h"

namespace vits {

// ---------------------------------------------------------------------------------------------------------
// Relative-position self-attention core (vits.cpp:296-356; helpers :195-235).  SURVEY.md App. F1 closed form:
//   s_ij = q_i.k_j + [|j-i|<=w] q_i.Ek[j-i+w];  p = softmax_j;  o_i = sum_j p_ij v_j + sum_{|j-i|<=w} p_ij Ev[j-i+w]
// The reference materialises dense (2T-1)-row relative tables and pads/reshapes them (pure data movement);
// here the 2w+1 relative logits are 9 extra dot products per query.
// One block = (utterance, head, 16 queries); scores for the 16 queries x T keys live in LDS.
// ---------------------------------------------------------------------------------------------------------
constexpr int ATT_Q = kAttQ;  // (launch_plan.h: the planner reads the same)
// Threads per block: 1024 (16 waves) on small grids — at batch 1 a launch has ~34 blocks and every phase is a chain of LDS / memory
// latencies that only more waves hide — and 256 on large ones (16-wave blocks pack worse: 73 -> 107 us per launch at batch 64).
// Both give the same bits: scores and outputs are per-element sums in a fixed order, and the softmax always runs on 16 lanes per query.

// Which of the block's 16 queries the 16-lane group t16 = tid / 16 normalises. ds_read_b32 / ds_write_b32 are served in groups of 32 lanes
// on banks (address / 4) mod 32, and the score rows are lp = 4 (mod 64) floats apart: two ADJACENT queries in one group of 32 lanes put
// their 16 columns on overlapping bank ranges (2-way conflicts on three passes over every row: the LDS_BANK_CONFLICT / LDS_IDX_ACTIVE = 0.37
// of the round-3 PMC pass). Queries q and q + 4 sit 16 banks apart: pair those. Each query's own 16-lane sums are untouched (same bits).
__device__ __forceinline__ int softmax_query_of(int t16) { return ((t16 & 1) << 2) | ((t16 >> 1) & 3) | (t16 & 8); }

// soft-max of one score row shared by 16 lanes (lane l16 owns columns l16, l16 + 16, ...), in place. exp_tab == nullptr: expf, fp32 sum,
// multiply by 1 / sum. exp_tab: ggml's table, the sum in double (terms are fp16 values <= 1: exact in any order), multiply by (float)(1 / sum).
__device__ __forceinline__ void softmax_row16(float* row, int len, int l16, const uint16_t* exp_tab) {
    float mx = -INFINITY;
    for (int j = l16; j < len; j += 16) mx = fmaxf(mx, row[j]);
    for (int o = 8; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 16));
    if (exp_tab) {
        double sum = 0.0;
        for (int j = l16; j < len; j += 16) {
            const float e = ggml_table_lookup(exp_tab, row[j] - mx);
            row[j] = e;
            sum += (double)e;
        }
        for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 16);
        const float inv = (float)(1.0 / sum);
        for (int j = l16; j < len; j += 16) row[j] *= inv;
        return;
    }
    float sum = 0.f;
    for (int j = l16; j < len; j += 16) {
        const float e = expf(row[j] - mx);
        row[j] = e;
        sum += e;
    }
    for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 16);
    const float inv = 1.0f / sum;
    for (int j = l16; j < len; j += 16) row[j] *= inv;
}

template <int ATT_THREADS>
__global__ __launch_bounds__(ATT_THREADS) void rel_attention_kernel(const float* q, int64_t q_bs, int q_cs, const float* k, int64_t k_bs, int k_cs, const float* v,
                                                            int64_t v_bs, int v_cs, const float* rel_k, const float* rel_v, float* out, int64_t o_bs,
                                                            int o_cs, const int* lens, int head_dim, int tmax, int window, float q_scale, int vshift, const uint16_t* exp_tab) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    constexpr int ATT_PASSES = 512 / ATT_THREADS < 1 ? 1 : 512 / ATT_THREADS;  // (d, 4-query group) items per thread: head_dim <= 128 (256 threads) / 256
    const int b = blockIdx.z, h = blockIdx.y, i0 = blockIdx.x * ATT_Q;
    const int len = lens ? lens[b] : tmax;
    if (i0 >= len) return;
    const int hd = head_dim, nrel = 2 * window + 1;
    float* qs = sm;                      // [ATT_Q][hd]
    float* qe = qs + ATT_Q * hd;         // [ATT_Q][nrel]   q_i . Ek[r]
    float* sc = qe + ATT_Q * nrel;       // [ATT_Q][len_pad]
    const int lp = (len + 3) & ~3;
    const int tid = threadIdx.x;
    const float* qb = q + (int64_t)b * q_bs + (int64_t)h * hd * q_cs;
    const float* kb = k + (int64_t)b * k_bs + (int64_t)h * hd * k_cs;
    const float* vb = v + (int64_t)b * v_bs + (int64_t)h * hd * v_cs;
    for (int idx = tid; idx < ATT_Q * hd; idx += ATT_THREADS) {
        const int d = idx / ATT_Q, qi = idx % ATT_Q;
        const int i = i0 + qi;
        qs[qi * hd + d] = i < len ? qb[(int64_t)d * q_cs + i] * q_scale : 0.f;  // scaling: vits.cpp:296-297
    }
    __syncthreads();
    for (int idx = tid; idx < ATT_Q * nrel; idx += ATT_THREADS) {
        const int qi = idx / nrel, r = idx % nrel;
        float a = 0.f;
        for (int d = 0; d < hd; ++d) a += qs[qi * hd + d] * rel_k[r * hd + d];
        qe[idx] = a;
    }
    __syncthreads();
    if constexpr (ATT_THREADS == 256) {
        // large grids: thread -> key j (coalesced along time), 16 running dot products per thread (half the K loads of the split below)
        for (int j = tid; j < len; j += ATT_THREADS) {
            float a[ATT_Q];
#pragma unroll
            for (int qi = 0; qi < ATT_Q; ++qi) a[qi] = 0.f;
            for (int d = 0; d < hd; ++d) {
                const float kv = kb[(int64_t)d * k_cs + j];
#pragma unroll
                for (int qi = 0; qi < ATT_Q; ++qi) a[qi] += qs[qi * hd + d] * kv;
            }
#pragma unroll
            for (int qi = 0; qi < ATT_Q; ++qi) {
                const int r = j - (i0 + qi) + window;
                float s = a[qi];
                if (r >= 0 && r < nrel) s += qe[qi * nrel + r];
                sc[qi * lp + j] = s;
            }
        }
    } else {
        // scores: thread -> (key j, half of the 16 queries): lanes run along time (coalesced), 8 running dot products per thread. (One
        // thread per key left 255 of 256 threads idle in a second pass for T = 257 = 128 interspersed ids.)
        constexpr int QH = ATT_Q / 2;
        for (int idx = tid; idx < 2 * len; idx += ATT_THREADS) {
            const int half = idx >= len ? 1 : 0, j = idx - half * len;
            const float* qh = qs + half * QH * hd;
            float a[QH];
    #pragma unroll
            for (int qi = 0; qi < QH; ++qi) a[qi] = 0.f;
            for (int d = 0; d < hd; ++d) {
                const float kv = kb[(int64_t)d * k_cs + j];
    #pragma unroll
                for (int qi = 0; qi < QH; ++qi) a[qi] += qh[qi * hd + d] * kv;
            }
    #pragma unroll
            for (int qi = 0; qi < QH; ++qi) {
                const int qa = half * QH + qi;
                const int r = j - (i0 + qa) + window;
                float s = a[qi];
                if (r >= 0 && r < nrel) s += qe[qa * nrel + r];
                sc[qa * lp + j] = s;
            }
        }
    }
    __syncthreads();
    // softmax per query: 16 lanes per query (the first 256 threads)
    if (tid < 256) {
        const int qi = softmax_query_of(tid >> 4), l16 = tid & 15;
        softmax_row16(sc + qi * lp, len, l16, exp_tab);
    }
    __syncthreads();
    // o[qi][d] = sum_j p[qi][j] v[d][j] + windowed relative-value term; thread -> (d, 4-query group), up to ATT_PASSES items per thread.
    // V goes through LDS in 64-key chunks (rows of v are time-major: lanes that differ in d would each touch their own cache line
    // per key — 2/3 of this kernel's time at batch 1); the sums still run over j in ascending order.
    float* ob = out + (int64_t)b * o_bs + (int64_t)h * hd * o_cs;
    if constexpr (ATT_THREADS == 256) {
        // large grids: V straight from memory (rows of v are time-major, lanes differ in d: one cache line per lane and key — other
        // resident blocks hide it, and the LDS staging below costs two barriers per 64 keys: 73 vs 94 us per launch at batch 64)
        for (int idx = tid; idx < hd * (ATT_Q / 4); idx += ATT_THREADS) {
            const int d = idx % hd, qg = idx / hd;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
            const float* p0 = sc + (qg * 4 + 0) * lp;
            const float* p1 = sc + (qg * 4 + 1) * lp;
            const float* p2 = sc + (qg * 4 + 2) * lp;
            const float* p3 = sc + (qg * 4 + 3) * lp;
            const float* vr = vb + (int64_t)d * v_cs;
            for (int j = 0; j < len; ++j) {
                const float vv = vr[j];
                a0 += p0[j] * vv;
                a1 += p1[j] * vv;
                a2 += p2[j] * vv;
                a3 += p3[j] * vv;
            }
            float acc[4] = {a0, a1, a2, a3};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int qi = qg * 4 + u, i = i0 + qi;
                if (i >= len) continue;
                float rsum = 0.f;
                for (int r = 0; r < nrel; ++r) {
                    const int j = i + r - window;
                    if (j >= 0 && j < len) rsum += sc[qi * lp + j] * rel_v[r * hd + d];
                }
                ob[(int64_t)d * o_cs + i] = acc[u] + rsum;
            }
        }
        return;
    }
    const int vc = 1 << vshift, vp = vc + 1;  // keys per chunk (64 unless a long utterance's scores leave less LDS); odd pitch: lanes differ in d
    float* vt = sc + ATT_Q * lp;       // [hd][vp]
    float acc[ATT_PASSES][4];
#pragma unroll
    for (int ps = 0; ps < ATT_PASSES; ++ps)
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[ps][u] = 0.f;
    const int nitems = hd * (ATT_Q / 4);
    for (int j0 = 0; j0 < len; j0 += vc) {
        const int nj = len - j0 < vc ? len - j0 : vc;
        for (int idx = tid; idx < (hd << vshift); idx += ATT_THREADS) {
            const int d = idx >> vshift, jj = idx & (vc - 1);
            vt[d * vp + jj] = jj < nj ? vb[(int64_t)d * v_cs + j0 + jj] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int ps = 0; ps < ATT_PASSES; ++ps) {
            const int idx = tid + ps * ATT_THREADS;
            if (idx < nitems) {
                const int d = idx % hd, qg = idx / hd;
                const float* p0 = sc + (qg * 4 + 0) * lp + j0;
                const float* p1 = sc + (qg * 4 + 1) * lp + j0;
                const float* p2 = sc + (qg * 4 + 2) * lp + j0;
                const float* p3 = sc + (qg * 4 + 3) * lp + j0;
                const float* vr = vt + d * vp;
                float a0 = acc[ps][0], a1 = acc[ps][1], a2 = acc[ps][2], a3 = acc[ps][3];
                for (int j = 0; j < nj; ++j) {
                    const float vv = vr[j];
                    a0 += p0[j] * vv;
                    a1 += p1[j] * vv;
                    a2 += p2[j] * vv;
                    a3 += p3[j] * vv;
                }
                acc[ps][0] = a0;
                acc[ps][1] = a1;
                acc[ps][2] = a2;
                acc[ps][3] = a3;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int ps = 0; ps < ATT_PASSES; ++ps) {
        const int idx = tid + ps * ATT_THREADS;
        if (idx >= nitems) continue;
        const int d = idx % hd, qg = idx / hd;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int qi = qg * 4 + u, i = i0 + qi;
            if (i >= len) continue;
            float rsum = 0.f;
            for (int r = 0; r < nrel; ++r) {
                const int j = i + r - window;
                if (j >= 0 && j < len) rsum += sc[qi * lp + j] * rel_v[r * hd + d];
            }
            ob[(int64_t)d * o_cs + i] = acc[ps][u] + rsum;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// The same attention core on the matrix cores (head_dim a multiple of 16): scores S = Q K^T and O = P V as 16 x 16 x 4 fp32 MFMAs
// (v_mfma_f32_16x16x4_f32: the 16 queries of a block are M), softmax and the 2w+1 relative terms as above. The VALU kernel does
// one LDS read per FMA and, for 1024-id inputs, was the longest single entry of a 16-bit step.
//   operand layouts (lane l): A[m = l % 16][k = l / 16], B[k = l / 16][n = l % 16], D[m = 4 * (l / 16) + r][n = l % 16], r = 0..3
// Block = (utterance, head, 16 queries), NW = 4 or 8 waves (chosen by the launch, see launch_rel_attention). Scores: wave w owns key
// tiles w, w + NW, ... and fetches the K operands of its next TWO tiles while it multiplies the current one (a tile is 24 x 32 cycles of
// MFMA work, a load round trip several times that). P V: wave w owns d tiles w, w + NW and walks the keys in groups of 16: MFMA k-step 4 g + i of group g takes
// keys 16 g + 4 (l / 16) + i, so that a lane's four k-steps are ONE 16-byte load of V (its row, 4 consecutive keys) and ONE
// ds_read_b128 of P, four groups in flight. (Round 2: one K tile of look-ahead, a dword load of V per k-step consumed right behind its
// issue, V staged through LDS for short inputs; per-block stamps at 1024 ids — tools/att_micro.hip — 28 us of scores and 61 us of P V
// for 5 + 7 us of MFMA work, now 21 + 11.)
// Every sum has ONE order for every grid, so results do not depend on the batch.
// LDS: Q^T [hd][16] | q.Ek [16][nrel] | scores [16][lp], lp = 4 mod 64 (conflict-free A reads of P).
// ---------------------------------------------------------------------------------------------------------

VITS_PHASE_BUF(vits_att_phase, 8);  // developer instrumentation (tools/att_micro.hip): per-block phase stamps, 100 MHz clock
#define ATT_STAMP(k) VITS_PHASE_STAMP(vits_att_phase, 8, k)

// MAXS: k-steps of head_dim the register arrays are sized for (24: head_dim <= 96, the MMS-TTS architecture; 32: <= 128). SHORT: sequences of
// at most a few key tiles per wave (the 128-token utterances of a batch): ONE key tile of look-ahead instead of two and at most 128 VGPRs, so
// that four blocks of four waves share a CU instead of three — 1024 blocks are then one round of the chip instead of 1.33.
// LAT (latency-bound launches: at most 128 blocks, round 6): every operand that does not depend on an earlier phase is REQUESTED at the top of the phase
// before — the wave's first K tile and the relative-key embeddings beside the Q tile, the first four V groups and the relative-value embeddings before
// the softmax — so that a block pays three memory round trips instead of six (per-block stamps at 128 tokens: 13.9 -> see launch_rel_attention). The
// MFMA sequences, and with them every sum, are those of the other variants.
template <int NW, int MAXS, bool SHORT, bool LAT = false>
__global__ __launch_bounds__(64 * NW, LAT ? 2 : (SHORT ? 4 : 3)) void rel_attention_mfma_kernel(const float* q, int64_t q_bs, int q_cs, const float* k, int64_t k_bs, int k_cs, const float* v,
                                                                     int64_t v_bs, int v_cs, const float* rel_k, const float* rel_v, float* out, int64_t o_bs,
                                                                     int o_cs, const int* lens, int head_dim, int tmax, int window, float q_scale, int v16, const uint16_t* exp_tab) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    constexpr int NT = 64 * NW;
    // XCD-aware order: the dispatcher deals workgroups to the 8 XCDs round-robin by linear id and every XCD has its own L2. All query
    // tiles of one (utterance, head) read the same K and V: every XCD gets a contiguous range of the order (query tile fastest, then
    // head, then utterance), so that its L2 holds the K / V of a few (utterance, head) pairs instead of all of them (1024 ids: -10 %).
    const unsigned gx = gridDim.x, gy = gridDim.y, nblk = gx * gy * gridDim.z;
    const unsigned lin = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
    const unsigned xc = lin & 7, slot = lin >> 3, qd = nblk >> 3, rm = nblk & 7;
    const unsigned lg = xc * qd + (xc < rm ? xc : rm) + slot;
    const int b = lg / (gx * gy), h = (lg / gx) % gy, i0 = (lg % gx) * ATT_Q;
    const int len = lens ? lens[b] : tmax;
    if (i0 >= len) return;
    ATT_STAMP(0);
    const int hd = head_dim, nrel = 2 * window + 1;
    const int lp = att_lp(len);
    float* qt = sm;                 // [hd][16]  (scaled)
    float* qe = qt + hd * ATT_Q;    // [16][nrel]
    float* sc = sm + ((hd * ATT_Q + ATT_Q * nrel + 3) & ~3);  // [16][lp], 16-byte aligned rows (ds_read_b128 of P)
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int ln = lane & 15, lk = lane >> 4;
    const float* qb = q + (int64_t)b * q_bs + (int64_t)h * hd * q_cs;
    const float* kb = k + (int64_t)b * k_bs + (int64_t)h * hd * k_cs;
    const float* vb = v + (int64_t)b * v_bs + (int64_t)h * hd * v_cs;
    const int nsteps = hd >> 2;
    const int ntiles = (len + 15) >> 4;
    float k0[MAXS], k1[MAXS], k2[MAXS];  // K operands of this wave's current / next key tiles (scores phase)
    auto load_tile = [&](int n, float* dst) __attribute__((always_inline)) {
        const int nc = n < ntiles ? n : ntiles - 1;  // (past the last tile: a valid address, values unused)
        const int key = nc * 16 + ln;
        const float* kp = kb + (int64_t)lk * k_cs + (key < len ? key : len - 1);
#pragma unroll
        for (int s2 = 0; s2 < MAXS; ++s2) dst[s2] = s2 < nsteps ? kp[(int64_t)(4 * s2) * k_cs] : 0.f;
    };
    float bvp[MAXS];  // LAT: the relative-key operands of this wave's tile of relative positions
    if constexpr (LAT) {
        load_tile(wid, k0);
        const int rcol = wid * 16 + ln;
        const float* rp = rel_k + (int64_t)(rcol < nrel ? rcol : 0) * hd + lk;
#pragma unroll
        for (int s2 = 0; s2 < MAXS; ++s2) bvp[s2] = (wid * 16 < nrel && s2 < nsteps && rcol < nrel) ? rp[4 * s2] : 0.f;
    }
    {
        float tq[8];  // (head_dim <= 128: at most 8 elements per thread, all loads in flight)
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int idx = tid + u * NT;
            const int d = idx / ATT_Q, i = i0 + idx % ATT_Q;
            tq[u] = (idx < ATT_Q * hd && i < len) ? qb[(int64_t)d * q_cs + i] * q_scale : 0.f;  // scaling: vits.cpp:296-297
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (tid + u * NT < ATT_Q * hd) qt[tid + u * NT] = tq[u];  // (idx = d * 16 + qi is the Q^T index)
    }
    __syncthreads();
    // this lane's Q operands for every k-step (A[m = ln][k = 4s + lk]): the same for every key tile and for the relative-key product
    float qa[MAXS];
#pragma unroll
    for (int s2 = 0; s2 < MAXS; ++s2) qa[s2] = s2 < nsteps ? qt[(4 * s2 + lk) * ATT_Q + ln] : 0.f;
    // q_i . Ek[r] for the 2w+1 relative positions: one more 16 x 16 product per tile of 16 relative positions (one tile — wave 0 — for
    // windows up to 7, the MMS-TTS architecture has 4; wider windows take further tiles on the other waves)
    for (int ct = wid; ct * 16 < nrel; ct += NW) {
        const int rcol = ct * 16 + ln;
        float4v acc = {0.f, 0.f, 0.f, 0.f};
        const float* rp = rel_k + (int64_t)(rcol < nrel ? rcol : 0) * hd + lk;
#pragma unroll
        for (int s0 = 0; s0 < MAXS; s0 += 8) {
            float bv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (LAT && ct == wid) bv[u] = s0 + u < MAXS ? bvp[s0 + u < MAXS ? s0 + u : 0] : 0.f;
                else bv[u] = (s0 + u < nsteps && rcol < nrel) ? rp[4 * (s0 + u)] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (s0 + u < nsteps) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[s0 + u], bv[u], acc, 0, 0, 0);
        }
        if (rcol < nrel) {
#pragma unroll
            for (int r = 0; r < 4; ++r) qe[(4 * lk + r) * nrel + rcol] = acc[r];
        }
    }
    if constexpr (!LAT) __syncthreads();  // (LAT: behind the first tile's MFMA chain, below)
    ATT_STAMP(1);
    // ---- scores: S[16 q][16 keys] per key tile, K = hd; the K operands of this wave's next two tiles are in flight ----
    {
        auto tile_chain = [&](const float* kop) __attribute__((always_inline)) -> float4v {
            float4v acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s2 = 0; s2 < MAXS; ++s2)
                if (s2 < nsteps) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[s2], kop[s2], acc, 0, 0, 0);
            return acc;
        };
        auto tile_store = [&](int n, const float4v acc) __attribute__((always_inline)) {
            const int key = n * 16 + ln;
            if (key < len) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int qi = 4 * lk + r;
                    const int rr = key - (i0 + qi) + window;
                    float sv = acc[r];
                    if (rr >= 0 && rr < nrel) sv += qe[qi * nrel + rr];
                    sc[qi * lp + key] = sv;
                }
            }
        };
        auto tile = [&](int n, const float* kop) __attribute__((always_inline)) { tile_store(n, tile_chain(kop)); };
        int n = wid;
        if constexpr (LAT) {
            // the first tile's MFMA chain runs BESIDE wave 0's relative-key product: the barrier that publishes q.Ek stands behind the chain, in front of the
            // first store (the other variants have it in front of the phase)
            if (n + NW < ntiles) load_tile(n + NW, k1);
            float4v a0 = {0.f, 0.f, 0.f, 0.f};
            if (n < ntiles) a0 = tile_chain(k0);
            __syncthreads();
            if (n < ntiles) tile_store(n, a0);
            n += NW;
            // (further tiles — sequences of more than 16 NW tokens on a small grid — one tile of look-ahead, k1 / k0 in turn)
            while (n < ntiles) {
                if (n + NW < ntiles) load_tile(n + NW, k0);
                __builtin_amdgcn_sched_barrier(0);
                tile(n, k1);
                n += NW;
                if (n >= ntiles) break;
                if (n + NW < ntiles) load_tile(n + NW, k1);
                __builtin_amdgcn_sched_barrier(0);
                tile(n, k0);
                n += NW;
            }
        } else
        if constexpr (SHORT) {
            if (n < ntiles) load_tile(n, k0);
            while (n < ntiles) {
                load_tile(n + NW, k1);
                __builtin_amdgcn_sched_barrier(0);
                tile(n, k0);
                n += NW;
                if (n >= ntiles) break;
                load_tile(n + NW, k0);
                __builtin_amdgcn_sched_barrier(0);
                tile(n, k1);
                n += NW;
            }
        } else {
        if (n < ntiles) {
            load_tile(n, k0);
            load_tile(n + NW, k1);
        }
        while (n < ntiles) {
            load_tile(n + 2 * NW, k2);
            __builtin_amdgcn_sched_barrier(0);
            tile(n, k0);
            n += NW;
            if (n >= ntiles) break;
            load_tile(n + 2 * NW, k0);
            __builtin_amdgcn_sched_barrier(0);
            tile(n, k1);
            n += NW;
            if (n >= ntiles) break;
            load_tile(n + 2 * NW, k1);
            __builtin_amdgcn_sched_barrier(0);
            tile(n, k2);
            n += NW;
        }
        }
    }
    // LAT: the first four V groups of this wave's first d tile and its relative-value embeddings, requested before the softmax
    const int ndt = hd >> 4;
    const int ng = (len + 15) >> 4;
    const int klast4 = (len - 1) & ~3;  // the last 16-byte piece of a row that starts inside the sequence (rows are padded to x4)
    auto load_v = [&](int g, const float* vrow, float4v& vv) __attribute__((always_inline)) {
        const int gc = g < ng ? g : ng - 1;
        const int key0 = 16 * gc + 4 * lk;
        if (v16) {
            const float4v t = *reinterpret_cast<const float4v*>(vrow + (key0 < klast4 ? key0 : klast4));
            vv[0] = key0 < len ? t[0] : 0.f;
            vv[1] = key0 + 1 < len ? t[1] : 0.f;
            vv[2] = key0 + 2 < len ? t[2] : 0.f;
            vv[3] = key0 + 3 < len ? t[3] : 0.f;
        } else {  // rows not 16-byte aligned (never in the engine; the operator entry point takes any stride): same values, four loads
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float t = vrow[key0 + e < len ? key0 + e : len - 1];
                vv[e] = key0 + e < len ? t : 0.f;
            }
        }
    };
    float4v vpre[8];  // (eight groups = 128 keys: the whole row of a 128-token utterance)
    float evp[4];
    if constexpr (LAT) {
        if (wid < ndt) {
            const float* vrow = vb + (int64_t)(wid * 16 + ln) * v_cs;
#pragma unroll
            for (int i = 0; i < 8; ++i) load_v(i, vrow, vpre[i]);
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2) {
                const int r = 4 * s2 + lk;
                evp[s2] = r < nrel ? rel_v[(int64_t)r * hd + wid * 16 + ln] : 0.f;
            }
        }
    }
    __syncthreads();
    ATT_STAMP(2);
    // ---- softmax per query: 16 lanes per query; the padding columns of P are zeroed (the MFMA k-steps run over whole groups) ----
    if (tid < 16 * ATT_Q) {
        const int qi = softmax_query_of(tid >> 4), l16 = tid & 15;
        softmax_row16(sc + qi * lp, len, l16, exp_tab);
        for (int j = len + l16; j < lp; j += 16) sc[qi * lp + j] = 0.f;
    }
    __syncthreads();
    ATT_STAMP(3);
    // ---- O[16 q][hd] = P V: d tile dt, K = keys in groups of 16 (see the head comment), four groups in flight ----
    float4v oacc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};  // d tiles wid and wid + NW (NW >= 4, head_dim <= 128)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int dt = wid + NW * u;
        if (dt < ndt) {
            const float* prow = sc + ln * lp + 4 * lk;
            const float* vrow = vb + (int64_t)(dt * 16 + ln) * v_cs;
            float4v pr[4], vr[4];
            auto load_group = [&](int g, float4v& pa, float4v& vv) __attribute__((always_inline)) {
                const int gc = g < ng ? g : ng - 1;
                pa = *reinterpret_cast<const float4v*>(prow + 16 * gc);
                load_v(g, vrow, vv);
            };
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (LAT && u == 0) {  // (V requested before the softmax; P exists only now)
                    pr[i] = *reinterpret_cast<const float4v*>(prow + 16 * (i < ng ? i : ng - 1));
                    vr[i] = vpre[i];
                } else {
                    load_group(i, pr[i], vr[i]);
                }
            }
            float4v a4 = oacc[u];
            for (int g = 0; g < ng; g += 4) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float4v pa = pr[i], vv = vr[i];
                    if (LAT && u == 0 && g == 0) {  // (groups 4-7: V came with the first four)
                        pr[i] = *reinterpret_cast<const float4v*>(prow + 16 * (4 + i < ng ? 4 + i : ng - 1));
                        vr[i] = vpre[4 + i];
                    } else {
                        load_group(g + 4 + i, pr[i], vr[i]);
                    }
                    if (g + i < ng) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) a4 = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[e], vv[e], a4, 0, 0, 0);
                    }
                }
            }
            oacc[u] = a4;
        }
    }
    ATT_STAMP(4);
    // ---- + windowed relative-value term: O += Pwin[16 q][r] . Ev[r][d] with Pwin[q][r] = P[q][i_q + r - w] (zero outside the sequence
    // and for r >= 2w+1): (2w+1+3)/4 more k-steps per d tile ----
    {
        const int rsteps = (nrel + 3) >> 2;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int dt = wid + NW * u;
            if (dt < ndt) {
                float4v a4 = oacc[u];
                for (int s = 0; s < rsteps; ++s) {
                    const int r = 4 * s + lk;
                    const int j = i0 + ln + r - window;
                    const float pw = (r < nrel && j >= 0 && j < len && i0 + ln < len) ? sc[ln * lp + j] : 0.f;
                    const float ev = (LAT && u == 0 && s < 4) ? evp[s < 4 ? s : 0] : (r < nrel ? rel_v[(int64_t)r * hd + dt * 16 + ln] : 0.f);
                    a4 = __builtin_amdgcn_mfma_f32_16x16x4f32(pw, ev, a4, 0, 0, 0);
                }
                oacc[u] = a4;
            }
        }
    }
    // ---- store: lane holds queries 4*lk .. 4*lk+3 of channel dt*16 + ln ----
    float* ob = out + (int64_t)b * o_bs + (int64_t)h * hd * o_cs;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int dt = wid + NW * u;
        if (dt >= ndt) continue;
        const int d = dt * 16 + ln;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = i0 + 4 * lk + r;
            if (i < len) ob[(int64_t)d * o_cs + i] = oacc[u][r];
        }
    }
    ATT_STAMP(5);
}

hipError_t launch_rel_attention(TensorRef q, TensorRef k, TensorRef v, const float* rel_k, const float* rel_v, TensorRef out, const int* lens, int batch,
                                int heads, int head_dim, int tmax, int window, float q_scale, hipStream_t s, GgmlTables tabs, int force) {
    // (which kernel, how many waves, which variant, LDS: plan_rel_attention, launch_plan.cpp)
    const AttentionPlan l = plan_rel_attention(batch, heads, head_dim, tmax, window, force);
    if (!l.ok) return hipErrorInvalidValue;
    const dim3 grid(l.gx, l.gy, l.gz), block(l.block);
    if (l.mfma) {
        const bool v_aligned = (v.cs & 3) == 0 && (v.bs & 3) == 0 && (reinterpret_cast<uintptr_t>(v.p) & 15) == 0;
#define VITS_ATTM_LAUNCH(NW, MS, SH, LAT)                                                                                                                  \
    static_assert(att_mfma_exists(NW, MS, SH, LAT), "the planner's predicate");                                                                            \
    if (l.nw == NW && l.maxs == MS && l.sh == SH && l.lat == LAT)                                                                                          \
        return launch_lds<&rel_attention_mfma_kernel<NW, MS, SH, LAT>>(grid, block, l.lds, s, q.p, q.bs, q.cs, k.p, k.bs, k.cs, v.p, v.bs, v.cs, rel_k, rel_v, out.p, out.bs, \
                                                                       out.cs, lens, head_dim, tmax, window, q_scale, v_aligned ? 1 : 0, tabs.exp)
        VITS_ATTM_LAUNCH(8, 24, false, true);
        VITS_ATTM_LAUNCH(4, 24, true, false);
        VITS_ATTM_LAUNCH(4, 32, false, false);
        VITS_ATTM_LAUNCH(8, 32, false, false);
#undef VITS_ATTM_LAUNCH
        return hipErrorInvalidValue;
    }
#define VITS_ATT_LAUNCH(T)                                                                                                                           \
    static_assert(att_valu_exists(T), "the planner's predicate");                                                                                    \
    if (l.block == T)                                                                                                                                \
        return launch_lds<&rel_attention_kernel<T>>(grid, block, l.lds, s, q.p, q.bs, q.cs, k.p, k.bs, k.cs, v.p, v.bs, v.cs, rel_k, rel_v, out.p, out.bs, out.cs, lens, head_dim, \
                                                    tmax, window, q_scale, l.vshift, tabs.exp)
    VITS_ATT_LAUNCH(1024);
    VITS_ATT_LAUNCH(256);
#undef VITS_ATT_LAUNCH
    return hipErrorInvalidValue;
}

}  // namespace vits
