// window_plan_dump — the vocoder window plan (vits.cpp_amd/csrc/window_plan.cpp) from the command line, for tests/test_window_plan_host.py. Linked with
// window_plan.o ALONE: that the link succeeds is the proof that the planner needs no kernel, no device and no engine. One case per line of standard input:
//   chunk collect_taps halo n_up smul[n_up + 1] sadd[n_up + 1] B frames[B]
// and one line of output each, sections separated by '|':
//   windowed Lw_max Lmax M windows
//   per window: f0 f1 lo hi emit_lo g0 g1 (the copy span at stride = the longest utterance's samples), then stage_max stage_sum per stage
//   per window and utterance: frames_in, len per stage, emit_end, owns, chunk_begin, final_end
//   the device table (nothing when the call is not windowed)
//   the range table of final_of(b, e) = e
//   the range table of final_of(b, e) = e if e is the utterance's sample count, else floor(2 e / 3)
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../vits.cpp_amd/csrc/window_plan.h"

using namespace vits;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int chunk = 0, taps = 0, halo = 0, n_up = 0, B = 0;
        if (!(in >> chunk >> taps >> halo >> n_up) || n_up < 0 || n_up > 7) return 2;
        std::vector<int> smul(n_up + 1), sadd(n_up + 1);
        for (int& v : smul) in >> v;
        for (int& v : sadd) in >> v;
        if (!(in >> B) || B < 1) return 2;
        std::vector<int> frames(B);
        for (int& v : frames) in >> v;
        if (!in) return 2;
        WindowPlan p;
        p.plan(frames.data(), B, smul.data(), sadd.data(), n_up, halo, chunk, taps != 0);
        std::vector<int64_t> slen(B);
        int64_t stride = 0;
        for (int b = 0; b < B; ++b) stride = std::max(stride, slen[b] = (int64_t)frames[b] * smul[n_up] + sadd[n_up]);
        std::printf("%d %d %d %d %zu |", (int)p.windowed, p.Lw_max, p.Lmax, p.M, p.size());
        for (size_t w = 0; w < p.size(); ++w) {
            size_t g0 = 0, g1 = 0;
            p.copy_span(w, (size_t)stride, g0, g1);
            std::printf(" %d %d %d %d %d %zu %zu", p[w].f0, p[w].f1, p[w].lo, p[w].hi, p.emit_lo(w), g0, g1);
            for (int i = 0; i <= n_up; ++i) std::printf(" %d %lld", p.stage_max(w, i), (long long)p.stage_sum(w, i));
        }
        std::printf(" |");
        for (size_t w = 0; w < p.size(); ++w)
            for (int b = 0; b < B; ++b) {
                std::printf(" %d", p.frames_in(w, b));
                for (int i = 0; i <= n_up; ++i) std::printf(" %d", p.len(w, i, b));
                std::printf(" %d %d %lld %lld", p.emit_end(w, b), (int)p.owns(w, b), (long long)p.chunk_begin(w), (long long)p.final_end(w, b));
            }
        std::printf(" |");
        if (p.windowed) {
            const std::vector<int> t = p.device_table();
            if (t.size() != p.size() * p.table_rows() * (size_t)B) return 3;
            for (int v : t) std::printf(" %d", v);
        }
        std::vector<int> rg;
        p.range_table(rg, [](int, int64_t e) { return (int)e; });
        if (rg.size() != p.size() * 2 * (size_t)B) return 3;
        std::printf(" |");
        for (int v : rg) std::printf(" %d", v);
        p.range_table(rg, [&](int b, int64_t e) { return (int)(e == slen[b] ? e : 2 * e / 3); });
        std::printf(" |");
        for (int v : rg) std::printf(" %d", v);
        std::printf("\n");
    }
    return 0;
}
