// conv_mfma_ablations.inc — developer instrumentation and ablation hooks of conv_mfma.hip (included by it; nothing here is part of the product build).
//   VITS_PHASE_TIMING (tools/conv_micro.hip, tools/lat16_micro.hip): per-block / per-wave phase timestamps into device buffers;
//   VAR_* (tools/conv_micro.hip): the kernel WITHOUT one of its parts — what that part costs. DESIGN.md 4.1 quotes the measurements:
//     VAR_NOA / VAR_NOB  no weight-fragment loads / no LDS operand reads in the K loop        VAR_NOBPIN  without the sched_barrier that pins the next step's LDS reads
//     VAR_NOPS=n         n x 64 idle cycles behind every MFMA (when does the next block launch)  VAR_YIELD=n the compute waves sleep in front of their last chunk
//     VAR_SETPRIO        prologue / producer / epilogue at wave priority 3, the K loop at 0       VAR_NOEPI   no epilogue (the ceiling of any epilogue work: +6 ... +16 %)
//     VAR_NOSTAGE        register-staged kernels without their global loads                       VITS_TAP_ROLLED / VITS_ZERO_OOB_NOROT  the round-2 / round-3 forms of two loops
// Every hook expands to NOTHING unless its macro is defined: the product kernels are what conv_mfma.hip reads like without them (the object files are byte-identical
// to the ones built from the in-line #ifdef blocks this file replaced in round 6).
// Per-block phase timestamps (tools/conv_micro.hip): the buffers, the plain and the extended stamp and the block-index guard are phase_timing.h's (included
// by conv_mfma.hip); the producer, chunk, epilogue and wave stamps below are this kernel's own. A body's block is (bx, by, bz), its arguments.
#define VITS_CONV_BLOCK (bx + gridDim.x * (by + gridDim.y * bz))
VITS_PHASE_BUF(vits_phase_buf, 8);   // [block][0..3] 100 MHz stamps, [4..5] shader clock around the K loop, [6..7] HW_ID / XCC_ID
VITS_PHASE_BUF(vits_prod_buf, 4);    // [block][0..3]: producer wave, shader cycles in issue / DMA wait / post-processing / barrier
VITS_PHASE_BUF(vits_chunk_buf, 8);   // [block][2c], [2c+1]: shader clock at the end of chunk c < 4 and behind its barrier
VITS_PHASE_BUF(vits_epi_buf, 8);     // [block][0..6]: shader clock at the epilogue's entry, in front of its first sub-tile, behind each of (up to) four sub-tiles, at its end
VITS_PHASE_BUF(vits_wave_end, 8);    // [block][wave]: 100 MHz clock when wave 0..4 retires
VITS_PHASE_BUF(vits_wave_start, 8);  // [block][wave]: 100 MHz clock at the first instructions of wave 0..4; [5..7]: HW_ID of waves 0, 1, 4
#define VITS_STAMP(k) VITS_PHASE_STAMP_EXT(vits_phase_buf, 8, VITS_CONV_BLOCK, k, 3, 6)
#define VITS_ESTAMP(k) VITS_PHASE_ROW(tid == 0, VITS_CONV_BLOCK, vits_epi_buf[8 * lin + (k)] = __builtin_amdgcn_s_memtime())
#define VITS_CHUNK_STAMP(slot) VITS_PHASE_ROW(tid == 0 && c < 4, VITS_CONV_BLOCK, vits_chunk_buf[8 * lin + (slot)] = __builtin_amdgcn_s_memtime())
#define VITS_WSTAMP() VITS_PHASE_ROW(lane == 0, VITS_CONV_BLOCK, vits_wave_end[8 * lin + wid] = __builtin_amdgcn_s_memrealtime())
#define VITS_WSTART()                                                                          \
    VITS_PHASE_ROW(lane == 0, VITS_CONV_BLOCK, {                                               \
        vits_wave_start[8 * lin + wid] = __builtin_amdgcn_s_memrealtime();                     \
        if (wid == 0 || wid == 1 || wid == 4) {                                                \
            unsigned hw;                                                                       \
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));                   \
            vits_wave_start[8 * lin + (wid == 0 ? 5 : wid == 1 ? 6 : 7)] = hw;                 \
        }                                                                                      \
    })
#define VITS_PSTAMP_END() VITS_PHASE_ROW(lane == 0, VITS_CONV_BLOCK, for (int k = 0; k < 4; ++k) vits_prod_buf[4 * lin + k] = pt[k])
#ifdef VITS_PHASE_TIMING
#define VITS_PSTAMP_BEGIN()                     \
    unsigned long long pt[4] = {0, 0, 0, 0};    \
    unsigned long long pprev = __builtin_amdgcn_s_memtime()
#define PSTAMP(k)                                                    \
    do {                                                             \
        const unsigned long long now = __builtin_amdgcn_s_memtime(); \
        pt[k] += now - pprev;                                        \
        pprev = now;                                                 \
    } while (0)
#else
#define VITS_PSTAMP_BEGIN()
#define PSTAMP(k)
#endif

#ifdef VITS_ZERO_OOB_NOROT  // every row starts at outside-column 0 (the round-3 walk, 16-way LDS bank conflicts)
#define VITS_ABL_ZERO_OOB_START(rotated) 0
#else
#define VITS_ABL_ZERO_OOB_START(rotated) (rotated)
#endif
#ifdef VAR_SETPRIO  // no effect on the starvation described at the K loop (DESIGN.md 4.1 "what the remaining 20 % are")
#define VITS_ABL_SETPRIO(x) __builtin_amdgcn_s_setprio(x)
#else
#define VITS_ABL_SETPRIO(x)
#endif
#ifdef VITS_TAP_ROLLED
#define VITS_ABL_TAP_UNROLL _Pragma("unroll 1")
#else
#define VITS_ABL_TAP_UNROLL _Pragma("unroll")
#endif
#ifdef VAR_NOA
#define VITS_ABL_UNLESS_NOA(...)
#else
#define VITS_ABL_UNLESS_NOA(...) __VA_ARGS__
#endif
#ifdef VAR_NOB
#define VITS_ABL_UNLESS_NOB(...)
#else
#define VITS_ABL_UNLESS_NOB(...) __VA_ARGS__
#endif
#ifdef VAR_NOBPIN
#define VITS_ABL_UNLESS_NOBPIN(...)
#else
#define VITS_ABL_UNLESS_NOBPIN(...) __VA_ARGS__
#endif
#ifdef VAR_NOPS
#define VITS_ABL_NOPS() _Pragma("unroll") for (int z = 0; z < VAR_NOPS; ++z) asm volatile("s_nop 15")
#else
#define VITS_ABL_NOPS()
#endif
#ifdef VAR_NOSTAGE
#define VITS_ABL_NOSTAGE_RETURN() return
#else
#define VITS_ABL_NOSTAGE_RETURN()
#endif
#ifdef VAR_YIELD
#define VITS_ABL_YIELD(last) \
    if (last) __builtin_amdgcn_s_sleep(VAR_YIELD)
#else
#define VITS_ABL_YIELD(last)
#endif
#ifdef VAR_NOEPI  // keep the accumulators alive, store one value per lane
#define VITS_ABL_NOEPI_RETURN()                                              \
    {                                                                        \
        float sacc = 0.f;                                                    \
        for (int i = 0; i < MR; ++i)                                         \
            for (int j = 0; j < NR; ++j)                                     \
                for (int r = 0; r < 16; ++r) sacc += acc[i][j][r];           \
        if (sacc == 12345.678f) p.y[tid] = sacc;                             \
        return;                                                              \
    }
#else
#define VITS_ABL_NOEPI_RETURN()
#endif
