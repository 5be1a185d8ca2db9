// voices.hip — rows of an effective-bias table for speaker embeddings registered at run time (include/vits.h vits_model_add_voices;
// DESIGN.md §8 "Custom voices"). speaker_bias_kernel (stage1_glue.hip) builds the file's rows at load, one launch per segment and one thread
// per (row, channel) walking its weight row with stride-E loads; registration is a serving-path call, so all segments of a table and all new
// rows go in ONE launch here, with the weights read coalesced.
//
// Block = VOICE_TC channels of one segment x VOICE_VSTEP * VPT voices (VPT = 8: 32 voices; VPT = 1 for a registration of at most four voices, which would
// otherwise spend 31 of 32 chains on padding). The embedding dimension is walked in chunks of VOICE_EC: the block stages the weight
// tile [VOICE_TC][VOICE_EC] (consecutive threads read consecutive e of a weight row) and the voices' chunk [voices][VOICE_EC] in LDS, then every thread
// runs its VPT chains. A wave = 64 channels of ONE voice: the weight read is conflict-free (row pitch VOICE_EC + 1), the embedding read a
// broadcast. The arithmetic of one output is speaker_bias_kernel's, operation for operation: acc = 0; for e ascending: acc = fmaf(w[c][e], g[e], acc);
// row[c] = bias[c] + (acc + cond_b[c]) — chunks are walked in ascending order and each chain lives in one thread, so a voice that equals a file speaker's
// embedding gets that speaker's row bit for bit (tests/test_gpu_voices.py).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"

namespace vits {

constexpr int VOICE_TC = 64, VOICE_EC = 64, VOICE_THREADS = 256;
constexpr int VOICE_VSTEP = VOICE_THREADS / VOICE_TC;  // voices a block works on side by side (one per wave)
constexpr int VOICE_MAX_GRID_Y = 65535;

template <int VPT>  // voices per thread
__global__ __launch_bounds__(VOICE_THREADS) void voice_rows_kernel(const VoiceSeg* __restrict__ segs, int nseg, const float* __restrict__ emb, int n_voices, int E,
                                                                   float* __restrict__ table, int64_t rs, int row_first) {
    __shared__ float w_s[VOICE_TC][VOICE_EC + 1];
    constexpr int VOICE_TV = VOICE_VSTEP * VPT;
    __shared__ float g_s[VOICE_TV][VOICE_EC];
    // the segment of this channel tile (segments are listed by ascending first tile)
    int si = 0;
    while (si + 1 < nseg && (int)blockIdx.x >= segs[si + 1].tile0) ++si;
    const VoiceSeg sg = segs[si];
    const int c0 = ((int)blockIdx.x - sg.tile0) * VOICE_TC;  // first channel of the tile inside its segment
    const int nc = min(VOICE_TC, sg.n - c0);
    const int v0 = (int)blockIdx.y * VOICE_TV;
    const int tid = (int)threadIdx.x, cl = tid % VOICE_TC, vl = tid / VOICE_TC;
    float acc[VPT];
#pragma unroll
    for (int j = 0; j < VPT; ++j) acc[j] = 0.f;
    for (int e0 = 0; e0 < E; e0 += VOICE_EC) {
        const int ne = min(VOICE_EC, E - e0);
        for (int i = tid; i < VOICE_TC * VOICE_EC; i += VOICE_THREADS) {
            const int r = i / VOICE_EC, e = i % VOICE_EC;
            w_s[r][e] = (r < nc && e < ne) ? sg.w[(int64_t)(c0 + r) * E + e0 + e] : 0.f;
        }
        for (int i = tid; i < VOICE_TV * VOICE_EC; i += VOICE_THREADS) {
            const int r = i / VOICE_EC, e = i % VOICE_EC;
            g_s[r][e] = (v0 + r < n_voices && e < ne) ? emb[(int64_t)(v0 + r) * E + e0 + e] : 0.f;
        }
        __syncthreads();
        for (int e = 0; e < ne; ++e) {
            const float w = w_s[cl][e];
#pragma unroll
            for (int j = 0; j < VPT; ++j) acc[j] = fmaf(w, g_s[vl + j * VOICE_VSTEP][e], acc[j]);
        }
        __syncthreads();
    }
    if (cl >= nc) return;
    const int c = c0 + cl;
    const float bias = table[sg.off + c], cb = sg.cb[c];  // row 0 of the table: the plain bias
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
        const int v = v0 + vl + j * VOICE_VSTEP;
        if (v < n_voices) table[(int64_t)(row_first + v) * rs + sg.off + c] = bias + (acc[j] + cb);
    }
}

int voice_seg_tiles(int n) { return (n + VOICE_TC - 1) / VOICE_TC; }

template <int VPT>
static void launch_slices(const VoiceSeg* segs, int nseg, int tiles, const float* emb, int n_voices, int E, float* table, int64_t rs, int row_first, hipStream_t s) {
    constexpr int TV = VOICE_VSTEP * VPT;
    for (int v0 = 0; v0 < n_voices; v0 += VOICE_MAX_GRID_Y * TV) {  // (one launch up to 2 million voices)
        const int n = std::min(n_voices - v0, VOICE_MAX_GRID_Y * TV);
        VITS_KLAUNCH(voice_rows_kernel<VPT>, dim3(tiles, (n + TV - 1) / TV), dim3(VOICE_THREADS), 0, s, segs, nseg, emb + (int64_t)v0 * E, n, E, table, rs, row_first + v0);
    }
}

hipError_t launch_voice_rows(const VoiceSeg* segs, int nseg, int tiles, const float* emb, int n_voices, int E, float* table, int64_t row_stride, int row_first,
                             hipStream_t s) {
    if (!segs || nseg < 1 || tiles < 1 || !emb || n_voices < 1 || E < 1 || !table || row_stride < 1 || row_first < 1) return hipErrorInvalidValue;
    if (n_voices <= VOICE_VSTEP) launch_slices<1>(segs, nseg, tiles, emb, n_voices, E, table, row_stride, row_first, s);
    else launch_slices<8>(segs, nseg, tiles, emb, n_voices, E, table, row_stride, row_first, s);
    return hipGetLastError();
}

}  // namespace vits
