// tile_map.cpp — the builder of tile_map.h: host arithmetic only (no kernels, no HIP calls), so that tests/tile_map_dump.cpp links it alone.
#include "tile_map.h"

namespace vits {

int64_t tile_map_count(const int* len_in, const int* len_out, int batch, int width, bool convt) {
    int64_t n = 0;
    for (int b = 0; b < batch; ++b) n += tile_map_tiles(tile_map_cols(len_in[b], len_out ? len_out[b] : len_in[b], convt), width);
    return n;
}

int64_t tile_map_dense(int batch, int t_in, int t_out, int width, bool convt) { return (int64_t)batch * tile_map_tiles(convt ? t_in + 1 : t_out, width); }

bool tile_map_needed(const int* len_in, const int* len_out, int batch, int t_in, int t_out, int width, bool convt) {
    return tile_map_count(len_in, len_out, batch, width, convt) < tile_map_dense(batch, t_in, t_out, width, convt);
}

int64_t tile_map_fill(const int* len_in, const int* len_out, int batch, int width, bool convt, TileEntry* out) {
    int64_t n = 0;
    for (int b = 0; b < batch; ++b) {
        const int lo = len_out ? len_out[b] : len_in[b];
        const int cols = tile_map_cols(len_in[b], lo, convt);
        for (int64_t t0 = 0; t0 < cols; t0 += width) out[n++] = TileEntry{b, (int32_t)t0, len_in[b], lo};
    }
    return n;
}

bool tile_map_group_layout(const int* taps, const int64_t* counts, int n, int slot_of[3], int64_t xend[3]) {
    if (n < 1 || n > 3) return false;
    int64_t per_slot[3] = {0, 0, 0};
    bool have[3] = {false, false, false};
    for (int i = 0; i < n; ++i) {
        const int s = taps[i] == 11 ? 0 : taps[i] == 7 ? 1 : taps[i] == 3 ? 2 : -1;
        if (s < 0 || have[s]) return false;
        have[s] = true;
        per_slot[s] = counts[i];
        slot_of[i] = s;
    }
    int64_t x = 0;
    for (int s = 0; s < 3; ++s) xend[s] = x += per_slot[s];
    return true;
}

}  // namespace vits
