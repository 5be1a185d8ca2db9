// tile_map.h — ragged batches: the list of the column tiles that EXIST, one entry per (utterance, tile), for the fp32 vocoder kernels whose dense
// grid is sized by the longest utterance of the batch (conv_mfma.hip, rbpair32.hip, rbblock32.hip). A launch over the list has no block that loads a
// length and returns; the block -> (utterance, tile) mapping is all that changes, so the results are bit-identical. The builder (tile_map.cpp) is plain
// host arithmetic: no kernels, no HIP calls; tests/tile_map_dump.cpp links tile_map.o alone. The device decode is tile_coord() in kernel_common.h.
#pragma once
#include <cstdint>
#include <vector>

namespace vits {

// What a block needs before it can start, in ONE 16-byte scalar load: the utterance, the first column of its tile and the length(s) the kernel would
// otherwise fetch from len_in / len_out / lens.
struct TileEntry {
    int32_t b;      // utterance
    int32_t t0;     // tile origin: tile index x tile width
    int32_t len_a;  // len_in[b] (convolutions) / lens[b] (fused ResBlock kernels)
    int32_t len_b;  // len_out[b] (convolutions; == len_a for the fused kernels)
};
static_assert(sizeof(TileEntry) == 16, "one dwordx4 load per block");

// Columns of utterance b that a launch tiles: the transposed conv's q runs over [0, len_in] (conv_plan.h conv_ncols), every other kernel's over
// [0, len_out). An utterance without input (a vocoder window it has no frames in) has none.
inline int tile_map_cols(int len_in, int len_out, bool convt) { return len_in <= 0 ? 0 : convt ? len_in + 1 : (len_out > 0 ? len_out : 0); }
inline int64_t tile_map_tiles(int cols, int width) { return ((int64_t)cols + width - 1) / width; }

// entries of the list = sum over the batch of ceil(cols / width). len_out null: len_in.
int64_t tile_map_count(const int* len_in, const int* len_out, int batch, int width, bool convt);
// blocks of the dense grid over the same utterances: batch x ceil(cols(t_in, t_out) / width), t_in / t_out the launch's maximum lengths
int64_t tile_map_dense(int batch, int t_in, int t_out, int width, bool convt);
// the dense grid holds blocks that would return at once (false: every utterance fills every tile of the grid, e.g. an equal-length batch)
bool tile_map_needed(const int* len_in, const int* len_out, int batch, int t_in, int t_out, int width, bool convt);
// the list: utterances in batch order, tiles ascending within an utterance (the order the dense grid dispatches them in, minus the empty ones).
// `out` has room for tile_map_count entries; returns how many were written
int64_t tile_map_fill(const int* len_in, const int* len_out, int batch, int width, bool convt, TileEntry* out);
// The grouped launch (conv_group_kernel): one list per member, concatenated with the longer tap counts first. counts[i] / taps[i]: member i's list and
// tap count (11, 7 or 3, each at most once). slot_of[i]: member i's slot (0: 11 taps, 1: 7, 2: 3); xend[s]: end of slot s's list in the concatenation
// (an absent slot has xend[s] == xend[s - 1]). false: a tap count outside {11, 7, 3} or twice
bool tile_map_group_layout(const int* taps, const int64_t* counts, int n, int slot_of[3], int64_t xend[3]);

// ---- what a launcher sees ---------------------------------------------------------------------------------------------------------------------
struct TileMapRef {
    const TileEntry* dev = nullptr;  // device copy of the list
    int n = 0;                       // entries
    int width = 0;
    bool convt = false;
};
// the maps of ONE length vector (one vocoder stage of one window), every tile width its kernels use
struct TileMapSet {
    static constexpr int kMax = 8;
    TileMapRef m[kMax];
    int count = 0;
    const TileMapRef* find(int width, bool convt) const {
        for (int i = 0; i < count; ++i)
            if (m[i].width == width && m[i].convt == convt) return &m[i];
        return nullptr;
    }
    bool add(const TileMapRef& r) {
        if (count >= kMax) return false;
        m[count++] = r;
        return true;
    }
};

}  // namespace vits
