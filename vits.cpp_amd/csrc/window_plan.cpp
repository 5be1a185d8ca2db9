// window_plan.cpp — the vocoder windows of window_plan.h: host arithmetic only (no kernels, no HIP calls), so that tests/window_plan_dump.cpp links it alone.
#include "window_plan.h"

namespace vits {

void WindowPlan::plan(const int* frames_, int B_, const int* smul_, const int* sadd_, int n_up_, int halo_frames, int chunk, bool collect_taps) {
    frames = frames_, B = B_, smul = smul_, sadd = sadd_, n_up = n_up_;
    M = smul[n_up];
    Lmax = 0;
    for (int b = 0; b < B; ++b) Lmax = std::max(Lmax, frames[b]);
    wins.clear();
    const int W = (chunk > 0 && !collect_taps && chunk < Lmax) ? chunk : 0;
    if (!W) wins.push_back({0, Lmax, 0, Lmax});
    else
        for (int f0 = 0; f0 < Lmax; f0 += W) {
            const int f1 = std::min(Lmax, f0 + W);
            wins.push_back({f0, f1, std::max(0, f0 - halo_frames), std::min(Lmax, f1 + halo_frames)});
        }
    windowed = wins.size() > 1;
    Lw_max = 0;
    for (const Win& w : wins) Lw_max = std::max(Lw_max, w.hi - w.lo);
}

int64_t WindowPlan::stage_sum(size_t w, int i) const {
    int64_t sum = 0;
    for (int b = 0; b < B; ++b) {
        const int lf = frames_in(w, b);
        if (lf > 0) sum += (int64_t)lf * smul[i] + sadd[i];
    }
    return sum;
}

std::vector<int> WindowPlan::device_table() const {
    std::vector<int> t(wins.size() * table_rows() * B, 0);
    for (size_t w = 0; w < wins.size(); ++w) {
        int* row = t.data() + w * table_rows() * B;
        for (int b = 0; b < B; ++b) {
            for (int i = 0; i <= n_up; ++i) row[(size_t)i * B + b] = len(w, i, b);
            row[(size_t)(n_up + 1) * B + b] = emit_end(w, b);
        }
    }
    return t;
}

void WindowPlan::range_table(std::vector<int>& table, const std::function<int(int, int64_t)>& final_of) const {
    table.assign(wins.size() * (size_t)2 * B, 0);
    std::vector<int> prev(B, 0);
    for (size_t w = 0; w < wins.size(); ++w)
        for (int b = 0; b < B; ++b) {
            int done = prev[b];
            if (owns(w, b)) done = std::max(done, final_of(b, final_end(w, b)));
            table[(w * 2) * B + b] = prev[b];
            table[(w * 2 + 1) * B + b] = done;
            prev[b] = done;
        }
}

}  // namespace vits
