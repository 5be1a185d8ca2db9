// kernel_common.h — the arithmetic and layout helpers the MFMA kernel files share, stated ONCE: the vector types, the 16-bit rounding
// points, the weight-fragment stream, the group-layout address and the group epilogue's tail. The interchangeable kernels of the
// 16-bit-operand path (conv16 / conv16_lat / convt16 / rbpair16 / rbblock16) promise the same bits; they get them by calling the same
// functions. Everything here is a typedef or a __device__ __forceinline__ function: no object file, no launch, no option of its own.
#pragma once

#include <cstdint>

#include "tile_map.h"

#ifdef __HIPCC__
namespace vits {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float float4v __attribute__((ext_vector_type(4)));
typedef float float2v __attribute__((ext_vector_type(2)));
typedef int int4v __attribute__((ext_vector_type(4)));
typedef int int2v __attribute__((ext_vector_type(2)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef __bf16 bf2v __attribute__((ext_vector_type(2)));

// round-to-nearest-even pair conversion (v_cvt_pk_f16_f32 / v_cvt_pk_bf16_f32), low half = a
template <bool BF>
__device__ __forceinline__ unsigned pack16(float a, float b) {
    float2v f = {a, b};
    if constexpr (BF) return __builtin_bit_cast(unsigned, __builtin_convertvector(f, bf2v));
    else return __builtin_bit_cast(unsigned, __builtin_convertvector(f, half2v));
}
template <bool BF>
__device__ __forceinline__ float unpack16(unsigned short h) {
    if constexpr (BF) return __builtin_bit_cast(float, (unsigned)h << 16);
    else return (float)__builtin_bit_cast(_Float16, h);
}
// Q7 (custom-ops.h:684-690): in the 16-bit arithmetic modes every conv operand is rounded (nearest even) to fp16 / bf16; the
// products are then exact in fp32. arith: 0 fp32, 1 bf16, 2 fp16 (VITS_ARITH_*). The VALU convolutions' form (dds.hip, vocoder_glue.hip).
__device__ __forceinline__ float round_arith(float v, int arith) {
    if (arith == 2) return (float)(_Float16)v;
    if (arith == 1) return (float)(__bf16)v;
    return v;
}
// v_mfma_f32_32x32x16_{f16,bf16} on two 16-byte operands (8 x 16 bit each)
template <bool BF>
__device__ __forceinline__ floatx16 mfma16(int4v a, int4v b, floatx16 c) {
    if constexpr (BF) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8, a), __builtin_bit_cast(half8, b), c, 0, 0, 0);
}

// A block's coordinates in a ragged launch: its utterance, the first column of its tile, and its utterance's lengths. With a list of the existing tiles
// (tile_map.h; the grid's x then runs over the list) they come from entry bx in ONE 16-byte load through the scalar cache; without one (map null) it is the
// dense decode: column tile bx of `bn` columns of utterance bz, the lengths from the arrays (null: the launch's maxima). Every converted kernel calls this.
struct TileCoord {
    int b, t0, len_a, len_b;
};
__device__ __forceinline__ TileCoord tile_coord(const TileEntry* map, int bx, int bz, int bn, const int* len_a, const int* len_b, int max_a, int max_b) {
    TileCoord c;
    if (map) {
        const int4v e = *reinterpret_cast<const int4v*>(map + bx);
        c.b = e.x, c.t0 = e.y, c.len_a = e.z, c.len_b = e.w;
    } else {
        c.b = bz, c.t0 = bx * bn;
        c.len_a = len_a ? len_a[bz] : max_a;
        c.len_b = len_b ? len_b[bz] : max_b;
    }
    return c;
}

// Buffer descriptor over a whole tensor (no bounds clamp: the kernels clamp their own offsets) — the packed weights' A-fragment
// stream and the LDS-DMA source of an activation tile.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t stream_rsrc(const void* base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0x7fffffff, 0x00020000);
}
// One lane's 16 bytes of A fragment number `step` (1 KiB per fragment = 64 lanes x 16 bytes) behind the scalar byte offset `sbase`; voff =
// the lane's byte offset into fragment 0. V = int4v (8 x 16 bit) or float4v (the fp32 kernels' fragments).
template <typename V>
__device__ __forceinline__ V load_frag(__amdgpu_buffer_rsrc_t wrsrc, int voff, int step, int sbase = 0) {
    return __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, voff, sbase + step * 1024, 0));
}

// group layout [channel / 8][time][8] (ts = slots per group row): element offset of channel ch0 at time t
__device__ __forceinline__ int64_t group_off(int ch0, int ts, int t) { return ((int64_t)(ch0 >> 3) * ts + t) * 8 + (ch0 & 7); }

// the resblock sum's scaling as the reference writes it: a division where it divides, a product where it multiplies
__device__ __forceinline__ float scale_or_div(float v, float scale, int scale_div) { return scale_div ? v / scale : v * scale; }

// The tail of the group epilogue, the rounding points of the 16-bit path, in two steps. v = channels ch0 .. ch0 + 3 at time t: conv + bias
// with the kernel's own post-activation and residual applied.
// Step 1, only where the call carries the resblock sum so far (a): v = scale(a + v).
__device__ __forceinline__ void group_add_scale(float (&v)[4], float4v a, float scale, int scale_div) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[e] = a[e] + v[e];
        v[e] = scale_or_div(v[e], scale, scale_div);
    }
}
// Step 2: the fp32 stream gets v at element `go` (= group_off(ch0, its time stride, t): the callers have it from their residual / sum
// loads), the 16-bit copy round(leaky_relu(v, y16_slope)) (slope 1 = identity). Null destinations are skipped.
template <bool BF>
__device__ __forceinline__ void group_store(float (&v)[4], float* yg, int64_t go, uint16_t* y16, int y16_ts, float y16_slope, int ch0, int t) {
    if (yg) *reinterpret_cast<float4v*>(yg + go) = float4v{v[0], v[1], v[2], v[3]};
    if (y16) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], v[e] * y16_slope);
        int2v w2;
        w2.x = (int)pack16<BF>(v[0], v[1]);
        w2.y = (int)pack16<BF>(v[2], v[3]);
        *reinterpret_cast<int2v*>(y16 + group_off(ch0, y16_ts, t)) = w2;
    }
}

// EMULATED ggml lookup tables (kernels.h GgmlTables): with a table pointer, GELU / the soft-max exponential go through the 65536-entry
// fp16 table indexed by the fp16 bits of the argument, as upstream ggml's ggml_vec_gelu_f32 / ggml_compute_forward_soft_max_f32 do (the
// tables are built on the HOST with the C library's tanhf / expf, like ggml_init). Null pointers = the default arithmetic.
__device__ __forceinline__ float ggml_table_lookup(const uint16_t* tab, float x) {
    const uint16_t i = __builtin_bit_cast(uint16_t, (_Float16)x);  // GGML_FP32_TO_FP16: round to nearest even
    return (float)__builtin_bit_cast(_Float16, tab[i]);
}
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }
// vits.cpp:673,687 ggml_gelu: erf-GELU (HF) by default; with a table, ggml's tanh-GELU through its fp16 lookup table (Q8, emulated)
__device__ __forceinline__ float gelu_op(float x, const uint16_t* gelu_tab) { return gelu_tab ? ggml_table_lookup(gelu_tab, x) : gelu_erf(x); }

}  // namespace vits
#endif  // __HIPCC__
