// abi_ops_common.h — the staging layer of the operator-level entry points (vits_op_*: abi_ops_conv.cpp, abi_ops_stage1.cpp, abi_ops_pcm.cpp, abi_ops_glue.cpp). An operator takes
// host arrays, runs the engine's own launchers on device copies and hands host arrays back; what lies between is here, once: the device buffer, the conv upload,
// the fp32-layout conv of a 16-bit mode, the NaN staging of ragged batches and the end of a run.
//
// What is NaN and why: a staged tensor is allocated at the stride the engine would give it, EVERY byte 0xFF (an fp32, f16 and bf16 NaN alike), and only the
// lens[b] valid columns of each row are copied in. A kernel that reads past an utterance's end, or into the pad between t and the stride, carries the NaN into
// its result, where the operator tests find it. Buffers that only the kernels write (intermediates, 16-bit copies) are 0xFF bytes too; outputs are zeros or
// 0xFF as each operator states at its call.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/vits.h"
#include "abi_internal.h"
#include "engine.h"

namespace vits {
extern thread_local int g_op_out_fill;  // vits_op_set_output_fill (abi_ops_conv.cpp)
extern thread_local int g_op_arith;  // vits_op_set_arith (abi_ops_conv.cpp): the arithmetic of this thread's operator calls

// a helper's failure: the error text is set, the entry point returns -1
inline bool refuse(const std::string& why) {
    set_err(why);
    return false;
}

// Owning device memory, sizes in bytes. A failed call has set the error text: the caller returns -1.
struct DevMem {
    void* p = nullptr;
    DevMem() = default;
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    ~DevMem() {
        if (p) hipFree(p);
    }
    static bool ok(hipError_t e, const char* what) { return e == hipSuccess || refuse(what); }
    bool alloc(size_t bytes) { return ok(hipMalloc(&p, std::max<size_t>(bytes, 16)), "device allocation failed"); }
    bool fill(size_t bytes, int byte) { return alloc(bytes) && ok(hipMemset(p, byte, std::max<size_t>(bytes, 16)), "device allocation failed"); }
    // a null source uploads zeros
    bool put(const void* h, size_t bytes) { return h ? alloc(bytes) && ok(hipMemcpy(p, h, bytes, hipMemcpyHostToDevice), "device allocation failed") : fill(bytes, 0); }
    // an optional array (lens, bias_rows): a null source leaves the device pointer null
    bool put_opt(const void* h, size_t bytes) { return !h || put(h, bytes); }
    bool get(void* h, size_t bytes) const { return ok(hipMemcpy(h, p, bytes, hipMemcpyDeviceToHost), "copy back failed"); }
    float* f() const { return static_cast<float*>(p); }
    uint16_t* h() const { return static_cast<uint16_t*>(p); }
    int* i() const { return static_cast<int*>(p); }
};

inline TensorRef tref(float* p, int channels, int stride) {
    TensorRef t;
    t.p = p;
    t.cs = stride;
    t.bs = (int64_t)channels * stride;
    return t;
}
inline bool lens_ok(const int32_t* lens, int batch, int t) {
    for (int b = 0; lens && b < batch; ++b)
        if (lens[b] < 0 || lens[b] > t) return false;
    return true;
}
inline bool shape_lens_ok(const int32_t* lens, int batch, int t, int t_stride) { return batch >= 1 && t >= 1 && t_stride >= t && lens_ok(lens, batch, t); }

// The end of a run: wait for the device. A failure becomes the error text, behind `what` where the operator names itself or its kernel.
inline bool finish(hipError_t e, const std::string& what = "") {
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) return true;
    set_err(what.empty() ? std::string(hipGetErrorString(e)) : what + ": " + hipGetErrorString(e));
    return false;
}

// ---- ragged batches ---------------------------------------------------------------------------------------------------------------------------------------
// Standard layout [batch][rows][pitch] floats: NaN everywhere, then columns [0, lens[b]) (lens NULL: [0, t)) of src's rows, which lie at src_pitch. src NULL: NaN only.
inline bool stage_rows(DevMem& dst, const float* src, int batch, int rows, int64_t src_pitch, int64_t pitch, const int32_t* lens, int t) {
    std::vector<float> h((size_t)batch * rows * pitch);
    std::memset(h.data(), 0xFF, h.size() * 4);
    for (int b = 0; src && b < batch; ++b)
        for (int c = 0; c < rows; ++c)
            std::memcpy(&h[((size_t)b * rows + c) * pitch], src + ((size_t)b * rows + c) * src_pitch, sizeof(float) * (size_t)(lens ? lens[b] : t));
    return dst.put(h.data(), h.size() * 4);
}
// ... and columns [0, t) of every row back, as the device holds them
inline bool unstage_rows(const DevMem& src, float* dst, int batch, int rows, int64_t pitch, int64_t dst_pitch, int t) {
    return DevMem::ok(hipMemcpy2D(dst, (size_t)dst_pitch * 4, src.p, (size_t)pitch * 4, (size_t)t * 4, (size_t)batch * rows, hipMemcpyDeviceToHost), "copy back failed");
}
// Group-of-8 layout [batch][channels / 8][pitch][8] floats (the 16-bit vocoder's streams; channels a multiple of 8), staged from and handed back to [batch][channels][*_pitch]
inline bool stage_group8(DevMem& dst, const float* src, int batch, int channels, int64_t src_pitch, int64_t pitch, const int32_t* lens, int t) {
    std::vector<float> h((size_t)batch * channels * pitch);
    std::memset(h.data(), 0xFF, h.size() * 4);
    for (int b = 0; b < batch; ++b)
        for (int c = 0; c < channels; ++c) {
            const float* s = src + ((size_t)b * channels + c) * src_pitch;
            float* g = &h[((size_t)b * channels + (size_t)(c / 8) * 8) * pitch + (c & 7)];
            for (int n = 0, len = lens ? lens[b] : t; n < len; ++n) g[(size_t)n * 8] = s[n];
        }
    return dst.put(h.data(), h.size() * 4);
}
template <class T>  // float streams, uint16_t copies
inline bool unstage_group8(const DevMem& src, T* dst, int batch, int channels, int64_t pitch, int64_t dst_pitch, int t) {
    std::vector<T> h((size_t)batch * channels * pitch);
    if (!src.get(h.data(), h.size() * sizeof(T))) return false;
    for (int b = 0; b < batch; ++b)
        for (int c = 0; c < channels; ++c) {
            const T* g = &h[((size_t)b * channels + (size_t)(c / 8) * 8) * pitch + (c & 7)];
            T* d = dst + ((size_t)b * channels + c) * dst_pitch;
            for (int n = 0; n < t; ++n) d[n] = g[(size_t)n * 8];
        }
    return true;
}

// ---- ragged batches on lists of existing tiles (tile_map.h) ------------------------------------------------------------------------------------------------
// The operators' kernel knobs: the process defaults, with VITS_TILE_MAP / VITS_NO_TILE_MAP read again at EVERY call — a test runs the dense grid and the lists
// in one process and compares the bits. (Operator calls are test infrastructure; the engine reads its knobs once, at load.)
struct OpKnobs {
    KernelKnobs k;
    KernelKnobsScope scope;
    OpKnobs() : k(kernel_knobs()), scope(&k) {
        k.no_tile_map = getenv("VITS_NO_TILE_MAP") != nullptr;
        k.tile_map = getenv("VITS_TILE_MAP") != nullptr;
    }
};
// The lists of ONE length vector on the device, built by the engine's builder for the tile widths the operator names (those its launchers may plan; a width no
// launch takes is a list nobody reads). As in the engine a list exists where the dense grid would hold empty blocks, or everywhere under VITS_TILE_MAP; whether
// a launch is large enough to take it is the launcher's rule (tile_map_for). lens NULL: every utterance t_in / t_out long.
struct OpTileMaps {
    TileMapSet set;
    std::vector<std::unique_ptr<DevMem>> mem;
    bool add(const int32_t* len_in, const int32_t* len_out, int batch, int t_in, int t_out, int width, bool convt) {
        const KernelKnobs& kn = kernel_knobs();
        if (kn.no_tile_map || set.find(width, convt)) return true;
        std::vector<int> la(batch, t_in), lb(batch, t_out);
        if (len_in) la.assign(len_in, len_in + batch);
        if (len_out) lb.assign(len_out, len_out + batch);
        if (!kn.tile_map && !tile_map_needed(la.data(), lb.data(), batch, t_in, t_out, width, convt)) return true;
        std::vector<TileEntry> e((size_t)tile_map_count(la.data(), lb.data(), batch, width, convt) + 1);  // (+ 1: an empty list still has an address)
        const int64_t n = tile_map_fill(la.data(), lb.data(), batch, width, convt, e.data());
        mem.emplace_back(new DevMem);
        if (!mem.back()->put(e.data(), e.size() * sizeof(TileEntry))) return false;
        return set.add(TileMapRef{static_cast<const TileEntry*>(mem.back()->p), (int)n, width, convt}) || refuse("too many tile widths for one length vector");
    }
    // every width a conv over these lengths can run a list on (conv_tile_mapped: the throughput tiles of conv_mfma.hip, 128 and 256 columns)
    bool add_conv(const int32_t* len_in, const int32_t* len_out, int batch, int t_in, int t_out, bool convt) {
        return add(len_in, len_out, batch, t_in, t_out, tile_shape(TILE_128x128).bn(), convt) && add(len_in, len_out, batch, t_in, t_out, tile_shape(TILE_64x256).bn(), convt);
    }
};

// ---- convs ------------------------------------------------------------------------------------------------------------------------------------------------
struct Conv {
    PackedConv pc;
    DevMem w, wl, w16, b;  // the fp32 plane, its conv_lat16_kernel arrangement, the 16-bit plane, the bias (or bias table)
};
// One conv on the device as the engine's load leaves it. w: torch layout, `taps` its last extent (2 x ct_stride for EPI_CONVT); bias: bias_n floats (a whole bias
// table where the layer is speaker-conditioned) or NULL. VITS_ARITH_F32 uploads the fp32 plane and, for the layers conv_lat16_candidate names, the second
// arrangement; a 16-bit arithmetic uploads the 16-bit plane alone (launch_conv16 and its kin read nothing else).
// l16_always: the second arrangement whatever the candidate rule says. The fused stage-one kernels (dp_det.hip, stage1_lat.hip) read ONLY that arrangement and
// take layers below the rule's 64 products per output (a 32-channel 1x1 conv), where the engine builds it on demand (Engine::make_lat16).
inline bool upload_conv(Conv& c, const float* w, const float* bias, size_t bias_n, int cout, int cin, int taps, int epi, int ct_stride, int arith, bool l16_always = false) {
    PackedConv& pc = c.pc;
    const ConvPackDims pd = conv_pack_dims(cout, cin, taps, epi, ct_stride);
    pc.cin = cin, pc.cout = cout, pc.kt = pd.kt, pc.epi = epi, pc.ct_stride = ct_stride;
    pc.rows = pd.rows, pc.mtiles_used = pd.mtiles_used, pc.mtiles = pd.mtiles, pc.nchunks = pd.nchunks;
    if (bias) {
        if (!c.b.put(bias, bias_n * 4)) return false;
        pc.bias = c.b.f();
    }
    if (arith != VITS_ARITH_F32) {
        const std::vector<uint16_t> p16 = pack_conv_weights16(w, cout, cin, taps, epi, ct_stride, arith);
        if (!c.w16.put(p16.data(), p16.size() * 2)) return false;
        pc.wp16 = c.w16.h(), pc.bytes16 = (int64_t)p16.size() * 2;
        return true;
    }
    const std::vector<float> packed = pack_conv_weights(w, cout, cin, taps, epi, ct_stride, &pc.rows, &pc.mtiles_used, &pc.mtiles, &pc.nchunks);
    if (!c.w.put(packed.data(), packed.size() * 4)) return false;
    pc.wp = c.w.f(), pc.bytes = (int64_t)packed.size() * 4;
    if (l16_always || conv_lat16_candidate(epi, taps, cin)) {
        const std::vector<float> pl = repack_conv_weights_l16(packed, pc.mtiles, pc.nchunks, pc.kt);
        if (!c.wl.put(pl.data(), pl.size() * 4)) return false;
        pc.wp_l16 = c.wl.f();
    }
    return true;
}

// room for the converter's output for a conv of c_in channels over t columns, [batch][c_in / 8][round_up(t, 8)][8] 16-bit elements (and one group row per utterance to spare)
inline size_t group16_bytes(int batch, int cin, int t) { return (size_t)batch * ((cin + 7) / 8 + 1) * round_up(t, 8) * 8 * 2; }
// A conv of the fp32-layout orchestration (Engine::conv): the fp32 kernel, or in a 16-bit arithmetic the converter + the 16-bit-operand kernel
// (Engine::conv16_transparent). x16: the converter's scratch, at least group16_bytes(batch, c_in, t_in). nan_bytes: that many bytes of it are set to 0xFF
// before the converter runs, where one scratch serves the convs of a sequence and none may read what the one before left.
inline hipError_t conv_transparent(const PackedConv& w, const ConvCall& c, int arith, const DevMem& x16, size_t nan_bytes = 0) {
    if (arith == VITS_ARITH_F32) return launch_conv(w, c, nullptr);
    Ref16 r;
    r.p = x16.h(), r.ts = round_up(c.t_in, 8), r.bs = (int64_t)((w.cin + 7) / 8) * r.ts * 8;
    if (nan_bytes && hipMemsetAsync(x16.p, 0xFF, nan_bytes, nullptr) != hipSuccess) return hipErrorUnknown;
    const hipError_t e = launch_to_group16(c.x, c.len_in, c.batch, w.cin, c.t_in, c.pre_act ? c.slope : 1.0f, r, arith, nullptr);
    if (e != hipSuccess) return e;
    Conv16Call q;
    q.x = r, q.len_in = c.len_in, q.len_out = c.len_out, q.spk = c.spk, q.batch = c.batch, q.t_in = c.t_in, q.t_out = c.t_out, q.dil = c.dil, q.pad_l = c.pad_l;
    q.post_act = c.post_act, q.post_slope = c.post_slope, q.scale = c.scale, q.scale_div = c.scale_div, q.ct_crop = c.ct_crop, q.tile = c.tile;
    q.y = c.y, q.res = c.res, q.acc = c.acc;
    return launch_conv16(w, q, arith, nullptr);
}
}  // namespace vits
