// rbblock16.hip — one WHOLE HiFiGAN ResBlock (three conv pairs, dilations D0 / D1 / D2) as a single kernel, 16-bit-operand modes, the
// narrow vocoder stages (C = 32 / 64; C = 128 for k = 3):
//     y_{p+1} = y_p + Conv_{k,1}( leaky_relu( Conv_{k,D_p}( leaky_relu(y_p) ) + b1_p ) ) + b2_p ,  p = 0, 1, 2     (/root/reference/src/vits.cpp:545-581)
//     out     = [sum of the previous resblocks +] y_3 [ * 1/num_kernels ]                                             (vits.cpp:622-635)
// Why: in the 16-bit modes these stages are bound by HBM bytes (and, through the power budget, by the clock those bytes leave the matrix
// cores: tools/rb16_micro.hip — a C = 64, k = 3 pair takes 0.29 ms, 0.085 ms without its epilogue's traffic). As three fused pairs
// (rbpair16.hip) a resblock moves 3 x 12 B per element: every pair reads the 16-bit input and the fp32 residual and writes the fp32 stream
// and its 16-bit copy. Here the fp32 stream lives in REGISTERS across the three pairs (the MFMA C layout: a wave owns all 32 rows of a row
// tile for its 96 columns), the 16-bit conv inputs x_p = round(leaky_relu(y_p)) and t_p live in ONE LDS tile that the phases take turns
// in, and HBM sees the stage input once (4 B, + halo) and the resblock output once (4 B, + 4 B accumulator, + 2 B 16-bit copy on the last
// resblock): 10-14 B per element and resblock instead of 36. The price is the halo: a tile of W = 384 columns yields W - 24 (k - 1) / 2
// outputs (k = 3: 360, 7: 312, 11: 264), i.e. 1.07 / 1.23 / 1.45 x the MFMA work, which these stages have to spare (C = 64 runs 256-column
// tiles on four waves, 1.10 / 1.39 x, so that two blocks share a CU: see launch_rbblock16).
// Same operands, rounding points (kernel_common.h: pack16 / group_add_scale / group_store) and k-order of accumulation (chunk, tap, k-half) as
// rbpair16_kernel / conv16_kernel: bit-identical to the pair path (GPU test), which stays for C >= 128 (MFMA-bound: the halo would cost more
// than the bytes) and behind VITS_NO_RBBLOCK16=1.
// Round 6: on grids of thousands of tiles a block walks a SEGMENT of tiles and takes the halo on its left from the tile before
// (template parameter STREAM; rbb_stream_tiles_for() says where): 1.19 x instead of 1.45 x the MFMA work at k = 11, which also brings the
// C = 64 / k = 11 resblocks to this kernel.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstdlib>

#include "../../include/vits.h"
#include "kernel_common.h"
#include "kernels.h"
#include "phase_timing.h"

namespace vits {

// Two 8-byte halves of two 16-byte slots per lane -> one whole slot per lane. In the MFMA C layout lane l < 32 holds channels 0-3 and lane
// l + 32 channels 4-7 of a channel group at one column; writing them as two ds_write_b64 at a 16-byte stride is a 4-way bank conflict
// (PMC: 0.08-0.20 of the LDS cycles of the pair kernels). v_permlane32_swap exchanges the upper half of one register with the lower half of
// another: given groups g0 (a) and g1 (b), lanes < 32 end up with the whole slot of g0 and lanes >= 32 with the whole slot of g1.
__device__ __forceinline__ int4v slot_pair(int2v a, int2v b) {
    const auto x = __builtin_amdgcn_permlane32_swap((unsigned)a.x, (unsigned)b.x, false, false);
    const auto y = __builtin_amdgcn_permlane32_swap((unsigned)a.y, (unsigned)b.y, false, false);
    return int4v{(int)x[0], (int)y[0], (int)x[1], (int)y[1]};
}

struct RbBlockParams {
    const float* y0;  // stage input (the fp32 stream), group layout [b][C/8][g_ts][8]
    const uint16_t* w1[3];
    const uint16_t* w2[3];  // A fragments of the six convs (pack_conv_weights16)
    const float* b1[3];
    const float* b2[3];
    const int* lens;
    int tmax;
    float slope;  // leaky_relu in front of every conv
    float* yg;    // output, fp32 group layout (same strides as y0)
    const float* accg;
    int64_t g_bs;
    int g_ts;
    uint16_t* y16;
    int64_t y16_bs;
    int y16_ts;
    float y16_slope;
    float scale;
    int scale_div;
    int nt;  // STREAM: tiles a block walks (its segment = W - 2 H + (nt - 1) (W - H) output columns)
};

VITS_PHASE_BUF(vits_rbb_phase, 16);  // developer instrumentation (tools/rbb_micro.hip)
#define RBB_STAMP(k) VITS_PHASE_STAMP(vits_rbb_phase, 16, k)

// Block = NSTRIP column strips x C / (32 MRW) row groups of waves; wave (strip, rg) owns the MRW row tiles [MRW rg, MRW rg + MRW) (32 rows each)
// of the NRW 32-column tiles of its strip.
// STREAM (round 6; large grids): the block WALKS a segment of p.nt tiles from left to right and the halo on the LEFT of every tile but the
// first is not recomputed: each of the six convs finds the columns in front of the tile — P2 D_p of x_p, P2 of t_p — where the previous
// tile left them (`hist`, copied out of the LDS tile while that stage was in it and into the padding in front of the tile when the stage is
// written again). A tile then yields W - H outputs instead of W - 2 H (k = 11 at W = 384: 1.19 x the algorithmic MFMA work instead of
// 1.45 x; k = 7: 1.10 / 1.23). The halo on the right stays: without it the fp32 stream in the registers would have to lag from pair to pair
// (a 32-column tile handed from wave to wave through LDS per pair: 16-28 KB, one block per CU fewer). Every element is the same chain of
// operations on the same operands whichever tile computes it, and a history column is the value its tile computed: bit-identical to the
// one-tile form (GPU test), which stays for grids too small to be cut into segments.
// (The body as a device function: rbblock16_kernel runs it for one resblock, rbblock16_group3_kernel for the three resblocks of a stage in ONE launch.)
template <int KT, int C, int NSTRIP, int NRW, int MRW, int D0, int D1, int D2, bool BF, bool STREAM>
__device__ __forceinline__ void rbblock16_body(const RbBlockParams& p, const int b) {
    constexpr RbBlock16Geom GEO = rbblock16_geom(KT, C, NSTRIP, NRW, MRW, D0, D1, D2);  // (launch_plan.h: the planner reads the same)
    constexpr int NCH = C / 32;  // (LDS tile: C / 8 channel groups x PITCH slots)
    constexpr int P2 = GEO.p2;
    constexpr int DMAX = D0 > D1 ? (D0 > D2 ? D0 : D2) : (D1 > D2 ? D1 : D2);
    constexpr int H = GEO.h;        // halo per side
    constexpr int BO = GEO.bo;      // output columns of a (first) tile
    constexpr int ADV = GEO.adv;    // STREAM: distance between the tiles of a segment = output columns of every later tile
    constexpr int PADX = GEO.padx;  // the first conv of a pair reads up to P2 * D_p columns beyond a tile column
    constexpr int PITCH = GEO.pitch;
    constexpr int STEPS = 2 * KT, TOTAL = NCH * STEPS;
    constexpr int G = C / 8;
    static_assert(BO > 0, "tile too narrow for this kernel size");
    extern __shared__ __attribute__((aligned(16))) int4v tile[];  // [G][PITCH] slots of 8 x 16 bit: x_p, then t_p, then x_{p+1}, ...
    // behind the tile: the biases of the six convs, [pair][b1 | b2][C] fp32 — read from LDS where they are added (fetched from memory
    // behind each conv they cost an exposed L2 round trip per conv: six per block, which the short k = 3 blocks notice)
    float* lbias = reinterpret_cast<float*>(tile + G * PITCH);
    // STREAM: behind the biases the histories, [x_0 | t_0 | x_1 | t_1 | x_2 | t_2], stage q as [G][h_q] slots
    int4v* hist = tile + G * PITCH + 6 * C * (int)sizeof(float) / 16;

    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (wave-uniform: strip / row group live in scalar registers)
    const int strip = wid % NSTRIP, rt0 = (wid / NSTRIP) * MRW;
    const int len = p.lens ? p.lens[b] : p.tmax;
    const int nt = STREAM ? p.nt : 1;
    const int seg0 = blockIdx.x * (BO + (nt - 1) * ADV);
    if (seg0 >= len) return;
    RBB_STAMP(0);
    typedef const __attribute__((address_space(3))) int4v* LdsV;
    typedef __attribute__((address_space(3))) int4v* LdsS;
    // (the biases: requested in front of the first stream loads, so that the two round trips overlap)
    for (int i = threadIdx.x; i < 6 * C; i += C / (32 * MRW) * NSTRIP * 64) {  // (the body's own thread count: in a group launch the block may be larger)
        const int pi = i / (2 * C), r = i - pi * 2 * C;
        lbias[i] = r < C ? p.b1[pi][r] : p.b2[pi][r - C];
    }
    constexpr int HX0 = 0, HT0 = HX0 + P2 * D0, HX1 = HT0 + P2, HT1 = HX1 + P2 * D1, HX2 = HT1 + P2, HT2 = HX2 + P2 * D2;  // column offsets of the histories
    static_assert(HT2 + P2 == H, "the histories are the halo of one side");
    static_assert(!STREAM || G * P2 * DMAX <= C / (32 * MRW) * NSTRIP * 64, "one history slot per thread");

  for (int it = 0; it < nt; ++it) {
    // (STREAM: every per-lane address below is derived from an opaque copy of the lane id — left to itself the compiler hoists the
    // invariant halves of ~50 addresses out of the tile loop and spills 120 registers to keep them)
    int lane_v = lane;
    if constexpr (STREAM) asm volatile("" : "+v"(lane_v));
    const int h = lane_v >> 5, col = lane_v & 31;
    const int tid = wid * 64 + lane_v;
    const int u0 = strip * (NRW * 32) + col;  // this lane's tile column of column tile nr: u0 + 32 nr
    const int tg0 = seg0 - H + it * ADV;  // global time of tile column 0
    // history of a stage: `hq` columns in front of the NEXT tile (tile columns [ADV - hq, ADV)) out of the LDS tile, once the stage is
    // complete in it; and back in front of the tile (slots [PADX - hq, PADX)) when the next tile writes that stage
    auto hist_save = [&](const int off, const int hq) __attribute__((always_inline)) {
        if constexpr (STREAM) {
            if (tid < G * hq) {
                const int g = tid / hq, c = tid - g * hq;
                const int4v v = *((LdsV)(tile + g * PITCH + PADX + ADV - hq + c));
                *((LdsS)(hist + G * off + tid)) = v;
            }
        }
    };
    auto hist_restore = [&](const int off, const int hq, const bool on) __attribute__((always_inline)) {
        if constexpr (STREAM) {
            if (on && tid < G * hq) {
                const int g = tid / hq, c = tid - g * hq;
                const int4v v = *((LdsV)(hist + G * off + tid));
                *((LdsS)(tile + g * PITCH + PADX - hq + c)) = v;
            }
        }
    };
    const int ulo = it == 0 ? H : 0;      // the tile's own outputs: columns [ulo, ADV)
    if (tg0 + ulo >= len) break;
    if (it > 0) __syncthreads();  // every wave is done with the previous tile's t_2

    // ---- the fp32 stream of this wave's rows x columns, in the MFMA C layout: register 4 g + e of yv[m][nr] = channel 32 (rt0 + m) + 8 g + 4 h + e ----
    floatx16 yv[MRW][NRW];
    {
        const float* yb = p.y0 + (int64_t)b * p.g_bs;
#pragma unroll
        for (int m = 0; m < MRW; ++m)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int ch0 = (rt0 + m) * 32 + 8 * g + 4 * h;
#pragma unroll
                for (int nr = 0; nr < NRW; ++nr) {
                    const int t = tg0 + u0 + 32 * nr;
                    float4v v = {0.f, 0.f, 0.f, 0.f};
                    if (t >= 0 && t < len) v = *reinterpret_cast<const float4v*>(yb + group_off(ch0, p.g_ts, t));
#pragma unroll
                    for (int e = 0; e < 4; ++e) yv[m][nr][4 * g + e] = v[e];
                }
            }
    }
    // round(leaky_relu(src + bias)) of this wave's rows x columns into the LDS tile as whole 16-byte slots, zero outside the sequence (what a
    // conv sees as padding): x_p from the stream (bias = nullptr), t_p from the first conv's accumulators
    auto write_tile = [&](const floatx16 (&src)[MRW][NRW], const float* bias_p) __attribute__((always_inline)) {
#pragma unroll
        for (int m = 0; m < MRW; ++m)
#pragma unroll
            for (int k = 0; k < 2; ++k) {  // channel groups 2k and 2k + 1 of the row tile: one slot each per lane after the half swap
                float4v bias[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
                if (bias_p) {
#pragma unroll
                    for (int q = 0; q < 2; ++q) bias[q] = *reinterpret_cast<const float4v*>(bias_p + (rt0 + m) * 32 + 8 * (2 * k + q) + 4 * h);
                }
#pragma unroll
                for (int nr = 0; nr < NRW; ++nr) {
                    const int u = u0 + 32 * nr, t = tg0 + u;
                    int2v w[2];
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        float v[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            v[e] = src[m][nr][4 * (2 * k + q) + e];
                            if (bias_p) v[e] = v[e] + bias[q][e];
                            v[e] = fmaxf(v[e], v[e] * p.slope);
                            if (t < 0 || t >= len) v[e] = 0.f;
                        }
                        w[q].x = (int)pack16<BF>(v[0], v[1]);
                        w[q].y = (int)pack16<BF>(v[2], v[3]);
                    }
                    *((LdsS)(tile + ((rt0 + m) * 4 + 2 * k + h) * PITCH + PADX + u)) = slot_pair(w[0], w[1]);
                }
            }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    };

    floatx16 acc[MRW][NRW];
    // one conv over the LDS tile: output column u reads slots u + off0 + j * dstep; acc = sum over (chunk, tap, k-half) — the order of
    // rbpair16_kernel / conv16_kernel
    auto conv = [&](const uint16_t* wp, const int off0, const int dstep) __attribute__((always_inline)) {
#pragma unroll
        for (int m = 0; m < MRW; ++m)
#pragma unroll
            for (int j = 0; j < NRW; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[m][j][r] = 0.f;
        LdsV base = (LdsV)(tile + h * PITCH + PADX + u0 + off0);
        const __amdgpu_buffer_rsrc_t wrsrc = stream_rsrc(wp);
        int wvoff[MRW];
#pragma unroll
        for (int m = 0; m < MRW; ++m) wvoff[m] = (int)(((size_t)(rt0 + m) * TOTAL * 64 + lane_v) * 16);
        auto load_a = [&](int m, int step) __attribute__((always_inline)) -> int4v { return load_frag<int4v>(wrsrc, wvoff[m], step); };
        // weight-fragment ring: a step is NRW 32-cycle MFMAs per row tile, an L2 round trip several steps (C = 32, k >= 7: six slots — eight spill at the 168-VGPR cap of three blocks per CU)
        constexpr int RS = MRW == 1 ? ((C == 32 && KT > 3) ? 6 : 8) : 4, RD = RS - 2;
        int4v ring[RS][MRW];
#pragma unroll
        for (int i = 0; i < RD; ++i)
#pragma unroll
            for (int m = 0; m < MRW; ++m) ring[i][m] = load_a(m, i < TOTAL ? i : TOTAL - 1);
        // chunk / tap / k-half nest with a per-chunk operand pointer (the loop shape of rbpair16_kernel: a flat step loop with absolute
        // offsets compiled to more VGPRs there)
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            LdsV xb = base + c * 4 * PITCH;
            int4v b_nxt[NRW];
#pragma unroll
            for (int nr = 0; nr < NRW; ++nr) b_nxt[nr] = xb[nr * 32];
#pragma unroll
            for (int j = 0; j < KT; ++j)
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    const int s = c * STEPS + j * 2 + kk;  // compile time after unrolling
#pragma unroll
                    for (int m = 0; m < MRW; ++m) ring[(s + RD) % RS][m] = load_a(m, s + RD < TOTAL ? s + RD : TOTAL - 1);
                    __builtin_amdgcn_sched_barrier(0);
                    int4v b_cur[NRW];
#pragma unroll
                    for (int nr = 0; nr < NRW; ++nr) b_cur[nr] = b_nxt[nr];
                    {
                        // next step: the other k-half of this tap, or k-half 0 of the next tap (past the last tap: a slot a little further on, unused)
                        const int noff = kk == 0 ? 2 * PITCH + j * dstep : (j + 1) * dstep;
#pragma unroll
                        for (int nr = 0; nr < NRW; ++nr) b_nxt[nr] = xb[noff + nr * 32];
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int m = 0; m < MRW; ++m)
#pragma unroll
                        for (int nr = 0; nr < NRW; ++nr) acc[m][nr] = mfma16<BF>(ring[s % RS][m], b_cur[nr], acc[m][nr]);
                }
        }
    };

    // (hx / ht: history offsets of x_p and t_p; hxn, dn: offset and dilation of the next pair's x)
    auto pair = [&](const int pi, const int dil, const bool last, const int hx, const int ht, const int hxn, const int dn) __attribute__((always_inline)) {
        hist_save(hx, P2 * dil);  // (x_p is complete in the tile: what the next tile's first conv reads in front of its columns)
        // conv 1 over x_p: t column u reads x columns u - P2 dil + j dil
        conv(p.w1[pi], -P2 * dil, dil);
        __syncthreads();  // every wave is done with x_p: t_p takes its place
        write_tile(acc, lbias + pi * 2 * C);  // t = round(leaky_relu(conv1 + b1)), zero outside the sequence (the second conv's padding)
        hist_restore(ht, P2, it > 0);
        __syncthreads();
        hist_save(ht, P2);
        // conv 2 over t_p: y column u reads t columns u - P2 + j
        conv(p.w2[pi], -P2, 1);
        // the stream: y_{p+1} = y_p + (conv2 + b2)
#pragma unroll
        for (int m = 0; m < MRW; ++m)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int ch0 = (rt0 + m) * 32 + 8 * g + 4 * h;
                const float4v bias = *reinterpret_cast<const float4v*>(lbias + pi * 2 * C + C + ch0);
#pragma unroll
                for (int nr = 0; nr < NRW; ++nr)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float v = acc[m][nr][4 * g + e] + bias[e];
                        yv[m][nr][4 * g + e] = yv[m][nr][4 * g + e] + v;
                    }
            }
        if (!last) {
            __syncthreads();  // every wave is done with t_p: x_{p+1} takes its place
            write_tile(yv, nullptr);
            hist_restore(hxn, P2 * dn, it > 0);
            __syncthreads();
        }
    };

    write_tile(yv, nullptr);
    hist_restore(HX0, P2 * D0, it > 0);
    __syncthreads();
    RBB_STAMP(1);
    pair(0, D0, false, HX0, HT0, HX1, D1);
    RBB_STAMP(2);
    pair(1, D1, false, HX1, HT1, HX2, D2);
    RBB_STAMP(3);
    pair(2, D2, true, HX2, HT2, 0, 1);
    RBB_STAMP(4);

    // ---- epilogue (as the last pair's in rbpair16_kernel): resblock sum / scale, fp32 output + 16-bit copy, the BO owned columns only ----
    // Two passes: the accumulator of the previous resblocks is read in place (accg == yg), so a load / add / store per element is a chain of
    // dependent HBM round trips — the compiler may not move a later load above an earlier store that could alias it (the WaveNet kernels
    // spent 15 of 48 us that way). All addends first (the conv accumulators are dead: their registers hold them), then every store.
    {
        // (STREAM: addresses from a second opaque copy of the lane id — shared with the loads at the top of the tile they would be kept, and spilled, across the six convs)
        int lane_e = lane;
        if constexpr (STREAM) asm volatile("" : "+v"(lane_e));
        const int h = lane_e >> 5, u0 = strip * (NRW * 32) + (lane_e & 31);
        float* yg = p.yg ? p.yg + (int64_t)b * p.g_bs : nullptr;  // (null: only the 16-bit copy is wanted — the last resblock of a stage)
        const float* ag = p.accg ? p.accg + (int64_t)b * p.g_bs : nullptr;
        uint16_t* y16 = p.y16 ? p.y16 + (int64_t)b * p.y16_bs : nullptr;
        float4v av[MRW][4][NRW];
        __builtin_amdgcn_sched_barrier(0);  // (not above the last conv: its accumulators have to be dead for these registers)
        if constexpr (STREAM) {  // (defined on every path: left undefined without an accumulator they become loop-carried values of the tile loop, 40 spilled registers)
#pragma unroll
            for (int m = 0; m < MRW; ++m)
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int nr = 0; nr < NRW; ++nr) av[m][g][nr] = float4v{0.f, 0.f, 0.f, 0.f};
        }
        if (ag) {
#pragma unroll
            for (int m = 0; m < MRW; ++m)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int ch0 = (rt0 + m) * 32 + 8 * g + 4 * h;
#pragma unroll
                    for (int nr = 0; nr < NRW; ++nr) {
                        const int u = u0 + 32 * nr, t = tg0 + u;
                        av[m][g][nr] = float4v{0.f, 0.f, 0.f, 0.f};
                        if (u >= ulo && u < ADV && t < len) av[m][g][nr] = *reinterpret_cast<const float4v*>(ag + group_off(ch0, p.g_ts, t));
                    }
                }
        }
#pragma unroll
        for (int m = 0; m < MRW; ++m)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int ch0 = (rt0 + m) * 32 + 8 * g + 4 * h;
#pragma unroll
                for (int nr = 0; nr < NRW; ++nr) {
                    const int u = u0 + 32 * nr, t = tg0 + u;
                    if (u < ulo || u >= ADV || t >= len) continue;
                    const int64_t go = group_off(ch0, p.g_ts, t);
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = yv[m][nr][4 * g + e];
                    if (ag) group_add_scale(v, av[m][g][nr], p.scale, p.scale_div);
                    group_store<BF>(v, yg, go, y16, p.y16_ts, p.y16_slope, ch0, t);
                }
            }
    }
  }  // (tiles of the segment)
    RBB_STAMP(5);
}
template <int KT, int C, int NSTRIP, int NRW, int MRW, int D0, int D1, int D2, bool BF, bool STREAM>
__global__ __launch_bounds__(C / (32 * MRW) * NSTRIP * 64, (C == 32 && NSTRIP == 4 && NRW <= 3) ? 3 : (C / (32 * MRW) * NSTRIP <= 4 ? 2 : 1)) void rbblock16_kernel(const RbBlockParams p) {
    rbblock16_body<KT, C, NSTRIP, NRW, MRW, D0, D1, D2, BF, STREAM>(p, (int)blockIdx.y);
}
// The three resblocks of a narrow stage (k = 3, 7, 11; equal block shapes) in ONE launch: blockIdx.y = 3 x utterance + member; blocks past a member's last
// tile leave at once. One or two utterances, side-by-side resblocks (launch_rb_sum3 adds their outputs): one launch on the main stream instead of three on three
// streams behind a fork and in front of a join of 10-30 us each (the C = 32 stage at batch 1: 63 -> see DESIGN 9). A member is the kernel's body.
struct RbBlockGroup3Params {
    RbBlockParams m[3];
};
// member shapes (column strips, 32-column tiles per wave): those of launch_rbblock16 — C = 32: 4 x 3 for every k; C = 64: 2 x 4 for k = 3 / 7 (four waves), 4 x 3 for
// k = 11 (eight waves: the block is eight waves and a four-wave member's upper four leave before its first barrier)
template <int C, bool BF>
__global__ __launch_bounds__(C == 32 ? 256 : 512, C == 32 ? 3 : 2) void rbblock16_group3_kernel(const RbBlockGroup3Params gp) {
    const int member = (int)blockIdx.y % 3, b = (int)blockIdx.y / 3;
    if constexpr (C == 32) {
        if (member == 0) rbblock16_body<3, C, 4, 3, 1, 1, 3, 5, BF, false>(gp.m[0], b);
        else if (member == 1) rbblock16_body<7, C, 4, 3, 1, 1, 3, 5, BF, false>(gp.m[1], b);
        else rbblock16_body<11, C, 4, 3, 1, 1, 3, 5, BF, false>(gp.m[2], b);
    } else {
        if (member == 2) {
            rbblock16_body<11, C, 4, 3, 1, 1, 3, 5, BF, false>(gp.m[2], b);
        } else {
            if (threadIdx.x >= 256) return;
            if (member == 0) rbblock16_body<3, C, 2, 4, 1, 1, 3, 5, BF, false>(gp.m[0], b);
            else rbblock16_body<7, C, 2, 4, 1, 1, 3, 5, BF, false>(gp.m[1], b);
        }
    }
}

// ---- the sum over a stage's resblocks as its own launch (small grids, round 6) ------------------------------------------------------------------------
// The whole-resblock kernel carries the accumulation into the stage's shared sum itself, so the three resblocks of a narrow stage are a CHAIN of launches in
// the reference's order of the additions (RB0, += RB1, (+= RB2) * 1/num_kernels: vits.cpp:622-635) — at batch 1 three 15-25 us kernels of 75-100 blocks and two
// event hand-overs one behind the other (105 us for the C = 32 stage) on a chip that could run them side by side. Here every resblock writes its own fp32
// output and this kernel adds them in that same order with the same expressions (a + v, then the scale, then leaky_relu and the rounding of the 16-bit copy
// the next upsampler / conv_post reads): the same bits as the chained accumulation, element for element.
template <bool BF>
__global__ __launch_bounds__(256) void rb_sum3_kernel(const float* y0, const float* y1, const float* y2, int64_t g_bs, int g_ts, const int* lens, int tmax, float scale,
                                                       int scale_div, float* yg, uint16_t* y16, int64_t y16_bs, int y16_ts, float y16_slope) {
    const int b = blockIdx.z, grp = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
    const int len = lens ? lens[b] : tmax;
    if (t >= len) return;
    const int64_t go = (int64_t)b * g_bs + ((int64_t)grp * g_ts + t) * 8;
    float v[8];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
        const float4v a = *reinterpret_cast<const float4v*>(y0 + go + 4 * hh), b1 = *reinterpret_cast<const float4v*>(y1 + go + 4 * hh);
        float4v c2 = {0.f, 0.f, 0.f, 0.f};
        if (y2) c2 = *reinterpret_cast<const float4v*>(y2 + go + 4 * hh);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float x = a[e] + b1[e];  // (the second resblock's a + v; its scale is 1: v * 1 = v)
            if (y2) x = x + c2[e];
            x = scale_or_div(x, scale, scale_div);
            v[4 * hh + e] = x;
        }
    }
    if (yg) {
        *reinterpret_cast<float4v*>(yg + go) = float4v{v[0], v[1], v[2], v[3]};
        *reinterpret_cast<float4v*>(yg + go + 4) = float4v{v[4], v[5], v[6], v[7]};
    }
    if (y16) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], v[e] * y16_slope);
        int4v w;
        w.x = (int)pack16<BF>(v[0], v[1]);
        w.y = (int)pack16<BF>(v[2], v[3]);
        w.z = (int)pack16<BF>(v[4], v[5]);
        w.w = (int)pack16<BF>(v[6], v[7]);
        *reinterpret_cast<int4v*>(y16 + (int64_t)b * y16_bs + ((int64_t)grp * y16_ts + t) * 8) = w;
    }
}

hipError_t launch_rb_sum3(const float* y0, const float* y1, const float* y2, int channels, int64_t g_bs, int g_ts, const int* lens, int batch, int tmax, float scale, int scale_div,
                          float* yg, Ref16 y16, float y16_slope, int arith, hipStream_t s) {
    if (!y0 || !y1 || (channels & 7) || (!yg && !y16.p)) return hipErrorInvalidValue;
    dim3 grid((tmax + 255) / 256, channels / 8, batch);
    if (arith == VITS_ARITH_BF16) VITS_KLAUNCH(rb_sum3_kernel<true>, grid, dim3(256), 0, s, y0, y1, y2, g_bs, g_ts, lens, tmax, scale, scale_div, yg, y16.p, y16.bs, y16.ts, y16_slope);
    else VITS_KLAUNCH(rb_sum3_kernel<false>, grid, dim3(256), 0, s, y0, y1, y2, g_bs, g_ts, lens, tmax, scale, scale_div, yg, y16.p, y16.bs, y16.ts, y16_slope);
    return hipGetLastError();
}

// ---- host side -----------------------------------------------------------------------------------------------------------
// (in_group: as a member of launch_rbblock16_group3)
static hipError_t rbb_params(const PackedConv* const* c1, const PackedConv* const* c2, const RbBlock16Call& c, RbBlockParams& p, RbBlock16Plan& l, bool in_group = false) {
    const int C = c1[0]->cin, kt = c1[0]->kt;
    for (int i = 0; i < 3; ++i) {
        if (!c1[i]->wp16 || !c2[i]->wp16 || !c1[i]->bias || !c2[i]->bias || c1[i]->cin != C || c1[i]->cout != C || c2[i]->cin != C || c2[i]->cout != C || c1[i]->kt != kt ||
            c2[i]->kt != kt)
            return hipErrorInvalidValue;
        p.w1[i] = c1[i]->wp16;
        p.w2[i] = c2[i]->wp16;
        p.b1[i] = c1[i]->bias;
        p.b2[i] = c2[i]->bias;
    }
    l = plan_rbblock16(C, kt, c.batch, c.tmax, in_group, in_group ? 0 : c.force_nt);
    if (!l.ok || !c.y0 || (!c.yg && !c.y16.p)) return hipErrorInvalidValue;
    p.y0 = c.y0, p.lens = c.lens, p.tmax = c.tmax, p.slope = c.slope, p.yg = c.yg, p.accg = c.accg, p.g_bs = c.g_bs, p.g_ts = c.g_ts, p.y16 = c.y16.p;
    p.y16_bs = c.y16.bs, p.y16_ts = c.y16.ts, p.y16_slope = c.y16_slope, p.scale = c.scale, p.scale_div = c.scale_div;
    p.nt = in_group ? 1 : l.nt;  // (the grouped launch: one tile per block)
    return hipSuccess;
}

// the three resblocks (k = 3, 7, 11) of a C = 32 stage as one launch (small grids: one tile per block); c1[m] / c2[m]: member m's three conv pairs
hipError_t launch_rbblock16_group3(const PackedConv* const (*c1)[3], const PackedConv* const (*c2)[3], const RbBlock16Call* c, int arith, hipStream_t s) {
    RbBlockGroup3Params gp;
    const int C = c1[0][0]->cin;
    const int kts[3] = {c1[0][0]->kt, c1[1][0]->kt, c1[2][0]->kt};
    const LaunchGrid l = plan_rbblock16_group3(C, kts, c[0].batch, c[0].tmax);
    if (!l.ok) return hipErrorInvalidValue;
    for (int m = 0; m < 3; ++m) {
        RbBlock16Plan member;
        if (hipError_t e = rbb_params(c1[m], c2[m], c[m], gp.m[m], member, true)) return e;
        if (c[m].batch != c[0].batch || c[m].tmax != c[0].tmax) return hipErrorInvalidValue;
    }
    static_assert(rbblock16_group3_exists(32) && rbblock16_group3_exists(64), "the planner's predicate");
    const dim3 grid(l.gx, l.gy), block(l.block);
    const bool bf = arith == VITS_ARITH_BF16;
    if (C == 32) return bf ? launch_lds<&rbblock16_group3_kernel<32, true>>(grid, block, l.lds, s, gp) : launch_lds<&rbblock16_group3_kernel<32, false>>(grid, block, l.lds, s, gp);
    return bf ? launch_lds<&rbblock16_group3_kernel<64, true>>(grid, block, l.lds, s, gp) : launch_lds<&rbblock16_group3_kernel<64, false>>(grid, block, l.lds, s, gp);
}

template <int KT, int C, bool BF>
static hipError_t launch_rbb(const RbBlockParams& p, const RbBlock16Plan& l, hipStream_t s) {
    static_assert(rbblock16_exists(KT, C), "the planner would never ask for it");
    constexpr RbBlock16Tile T = rbblock16_tile(KT, C);
    const dim3 grid(l.gx, l.gy), block(l.block);
    if (l.nt > 1) return launch_lds<&rbblock16_kernel<KT, C, T.nstrip, T.nrw, T.mrw, 1, 3, 5, BF, true>>(grid, block, l.lds, s, p);
    return launch_lds<&rbblock16_kernel<KT, C, T.nstrip, T.nrw, T.mrw, 1, 3, 5, BF, false>>(grid, block, l.lds, s, p);
}
hipError_t launch_rbblock16(const PackedConv* const* c1, const PackedConv* const* c2, const RbBlock16Call& c, int arith, hipStream_t s) {
    const int C = c1[0]->cin, kt = c1[0]->kt;
    RbBlockParams p;
    RbBlock16Plan l;
    if (hipError_t e = rbb_params(c1, c2, c, p, l)) return e;
    const bool bf = arith == VITS_ARITH_BF16;
    // tile shapes (rbblock16_tile: column strips x 32-column tiles per wave x row tiles per wave). C = 32: 4 x 3 = 384 columns, three blocks per CU. Measured
    // alternatives (batch 64 x 128 ids, f16): C = 32 with 4 x 4 = 512 columns (two blocks per CU instead of three) +5...12 %; C = 64 as 4 x 3 (eight waves, one
    // block per CU: round 3's first version), as 6 x 2 (twelve waves) +-0, as 8 x 2 = 512 columns (sixteen waves at 128 VGPRs, spills) -5 %
    // on k = 11 only, as 2 x 5 (spills) worse than 2 x 4.
    // C = 64, k = 3 / 7: four waves (two strips of four column tiles, 256 columns) instead of eight (4 x 3): at 236 VGPRs two blocks share a CU and
    // one's loads, tile writes and epilogue overlap the other's MFMA phases — with eight waves a CU ran ONE block at a time, its matrix
    // pipes 30 % busy at 1.4 TB/s: k = 3 0.70 -> 0.55 ms, k = 7 1.09 -> 1.05 (the narrower tile costs 1.39 x instead of 1.23 x the MFMA work there)
    // C = 128, k = 3: the pairs are HBM-bound (4.4 TB/s); eight waves of two row tiles x two column tiles (256-column tiles, 232 outputs).
    // (Eight waves of one row tile on 128-column tiles at 128 VGPRs — two blocks per CU —, sixteen waves on 256 columns, eight on 192: +-2 %.)
#define VITS_RBB_GO(K, CC) \
    if (kt == K && C == CC) return bf ? launch_rbb<K, CC, true>(p, l, s) : launch_rbb<K, CC, false>(p, l, s)
    VITS_RBB_GO(3, 32);
    VITS_RBB_GO(7, 32);
    VITS_RBB_GO(11, 32);
    VITS_RBB_GO(3, 64);
    VITS_RBB_GO(7, 64);
    VITS_RBB_GO(11, 64);
    VITS_RBB_GO(3, 128);
#undef VITS_RBB_GO
    return hipErrorInvalidValue;
}

}  // namespace vits
