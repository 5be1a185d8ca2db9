// phase_timing.h — the per-block phase stamp of the developer harnesses (tools/*_micro.hip), stated ONCE. Nothing in the product build defines
// VITS_PHASE_TIMING: every macro below then expands to nothing and the kernels are what they read like without their *_STAMP lines.
//   VITS_PHASE_BUF(name, W)      a stamp buffer, [65536 blocks][W slots] of unsigned 64-bit; the harness reads it with hipMemcpyFromSymbol
//   VITS_PHASE_ROW(who, block, statements)   the guard every stamp shares: thread `who` of a block, and only a block whose linear index `block` has a
//                                row in the buffers; the statements see that index as `lin`
//   VITS_PHASE_STAMP(buf, W, k)  the block's first thread writes the 100 MHz clock (s_memrealtime) into slot k of its row
//   VITS_PHASE_STAMP_EXT(buf, W, block, k, clk, id)   the same for the block `block`, and with it the shader clock (s_memtime) in slot clk + k at
//                                k = 1 and k = 2, and HW_ID / XCC_ID in slots id, id + 1 at k = 0 (where a block ran, at which clock)
// Every stamp is an ordinary vector store from plain C++.
#pragma once

#ifdef VITS_PHASE_TIMING
#define VITS_PHASE_BUF(name, W) __device__ unsigned long long name[(W) * 65536]
#define VITS_PHASE_BLOCK (blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z))
#define VITS_PHASE_ROW(who, block, ...)   \
    do {                                  \
        if (who) {                        \
            const unsigned lin = (block); \
            if (lin < 65536) {            \
                __VA_ARGS__;              \
            }                             \
        }                                 \
    } while (0)
__device__ __forceinline__ void vits_phase_stamp_ext(unsigned long long* row, int k, int clk, int id) {
    row[k] = __builtin_amdgcn_s_memrealtime();
    if (k == 1 || k == 2) row[clk + k] = __builtin_amdgcn_s_memtime();
    if (k == 0) {
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        row[id] = hw;
        row[id + 1] = xcc;
    }
}
#else
#define VITS_PHASE_BUF(name, W)
#define VITS_PHASE_ROW(who, block, ...) \
    do {                                \
    } while (0)
#endif
#define VITS_PHASE_STAMP(buf, W, k) VITS_PHASE_ROW(threadIdx.x == 0, VITS_PHASE_BLOCK, buf[(W) * lin + (k)] = __builtin_amdgcn_s_memrealtime())
#define VITS_PHASE_STAMP_EXT(buf, W, block, k, clk, id) VITS_PHASE_ROW(threadIdx.x == 0, block, vits_phase_stamp_ext(buf + (W) * lin, k, clk, id))
