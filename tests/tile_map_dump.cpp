// tile_map_dump — the builder of the lists of existing tiles (vits.cpp_amd/csrc/tile_map.cpp) from the command line, for tests/test_tile_map_host.py. Linked with
// tile_map.o ALONE: that the link succeeds is the proof that the builder needs no kernel and no device. One command per line of standard input, one line of output each:
//   W                                              -> every tile width the geometry functions give the converted kernels: "conv <bn>" / "pair <kt> <dil> <C> <bo>" / "block <C> <bo>"
//   M width convt t_in t_out B len_in[B] len_out[B] -> "M count dense needed | b:t0:len_a:len_b ..." (the list is filled into exactly `count` entries)
//   G n taps[n] counts[n]                          -> "G ok slot_of[n] xend[3]"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../vits.cpp_amd/csrc/conv_plan.h"
#include "../vits.cpp_amd/csrc/launch_plan.h"
#include "../vits.cpp_amd/csrc/tile_map.h"

using namespace vits;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "W") {
            for (int tile : {(int)TILE_128x128, (int)TILE_64x256, (int)TILE_32x256, (int)TILE_64x64, (int)TILE_32x64}) std::printf("conv %d;", tile_shape(tile).bn());
            for (int kt : {3, 7, 11})
                for (int dil : {1, 3, 5})
                    for (int C : {32, 64, 128})
                        if (rbpair32_exists(kt, dil, C)) std::printf("pair %d %d %d %d;", kt, dil, C, rbpair32_geom(kt, dil, C).bo);
            for (int C : {32, 64})
                if (rbblock32_exists(C, rbblock32_nr(C))) std::printf("block %d %d;", C, rbblock32_geom(C, rbblock32_nr(C)).bo);
            std::printf("\n");
        } else if (cmd == "M") {
            int width = 0, convt = 0, t_in = 0, t_out = 0, B = 0;
            in >> width >> convt >> t_in >> t_out >> B;
            if (!in || width < 1 || B < 1) return 2;
            std::vector<int> la(B), lb(B);
            for (int& v : la) in >> v;
            for (int& v : lb) in >> v;
            if (!in) return 2;
            const int64_t count = tile_map_count(la.data(), lb.data(), B, width, convt != 0);
            std::vector<TileEntry> e((size_t)count);  // exactly: one entry too many written is an overflow the sanitizer sees
            const int64_t n = tile_map_fill(la.data(), lb.data(), B, width, convt != 0, e.data());
            if (n != count) return 3;
            std::printf("M %lld %lld %d |", (long long)count, (long long)tile_map_dense(B, t_in, t_out, width, convt != 0),
                        (int)tile_map_needed(la.data(), lb.data(), B, t_in, t_out, width, convt != 0));
            for (const TileEntry& t : e) std::printf(" %d:%d:%d:%d", t.b, t.t0, t.len_a, t.len_b);
            std::printf("\n");
        } else if (cmd == "G") {
            int n = 0;
            in >> n;
            if (!in || n < 0 || n > 8) return 2;
            std::vector<int> taps(n);
            std::vector<int64_t> counts(n);
            for (int& v : taps) in >> v;
            for (int64_t& v : counts) in >> v;
            if (!in) return 2;
            int slot_of[3] = {-1, -1, -1};
            int64_t xend[3] = {0, 0, 0};
            const bool ok = tile_map_group_layout(taps.data(), counts.data(), n, slot_of, xend);
            std::printf("G %d", (int)ok);
            for (int i = 0; i < n && i < 3; ++i) std::printf(" %d", slot_of[i]);
            std::printf(" | %lld %lld %lld\n", (long long)xend[0], (long long)xend[1], (long long)xend[2]);
        } else {
            return 2;
        }
    }
    return 0;
}
