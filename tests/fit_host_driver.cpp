// fit_host_driver — the fit's host definition (vits.cpp_amd/csrc/fit_host.cpp ALONE: no kernel, no device) as a stand-alone program, for
// tests/test_fit_host.py, which builds it under AddressSanitizer + UBSan and runs it on the cases it writes to standard input. A case is
//   batch t_stride min_rate max_rate / lens [batch] / groups [batch] / targets [batch] / the bits of e [sum lens] / fixed [sum lens]
// held here in buffers of EXACTLY batch x t_stride elements with the rows' tails NaN (e) and INT_MIN (fixed), so that a read or a write one element out of
// place is the sanitizer's to find. Prints per case one line of durations (the valid tokens, row by row) and one of group rows, and exits 0.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../vits.cpp_amd/csrc/kernels.h"

using namespace vits;

int main() {
    int cases = 0;
    if (std::scanf("%d", &cases) != 1) return 2;
    for (int k = 0; k < cases; ++k) {
        int B = 0, ts = 0;
        float lo_rate = 0, hi_rate = 0;
        if (std::scanf("%d %d %f %f", &B, &ts, &lo_rate, &hi_rate) != 4 || B < 1 || ts < 1) return 2;
        std::vector<int> lens((size_t)B), groups((size_t)B), fixed((size_t)B * ts, INT_MIN), dur((size_t)B * ts, 12345);
        std::vector<int64_t> targets((size_t)B), rows((size_t)B * kFitRowInts, 777);
        std::vector<float> e((size_t)B * ts, std::numeric_limits<float>::quiet_NaN());
        for (int& v : lens)
            if (std::scanf("%d", &v) != 1 || v < 0 || v > ts) return 2;
        for (int& v : groups)
            if (std::scanf("%d", &v) != 1) return 2;
        for (int64_t& v : targets) {
            long long t;
            if (std::scanf("%lld", &t) != 1) return 2;
            v = t;
        }
        for (int b = 0; b < B; ++b)
            for (int t = 0; t < lens[(size_t)b]; ++t) {
                unsigned u;
                if (std::scanf("%x", &u) != 1) return 2;
                const uint32_t w = u;
                std::memcpy(&e[(size_t)b * ts + t], &w, 4);
            }
        for (int b = 0; b < B; ++b)
            for (int t = 0; t < lens[(size_t)b]; ++t)
                if (std::scanf("%d", &fixed[(size_t)b * ts + t]) != 1) return 2;
        FitGroups g;
        std::string err;
        if (!fit_limits(lo_rate, hi_rate, g.s_lo, g.s_hi, err) || !fit_check(B, groups.data(), targets.data(), err)) {
            std::printf("refused %s\n", err.c_str());
            continue;
        }
        const std::vector<int> tgt(targets.begin(), targets.end());
        g.group = groups.data(), g.target = tgt.data();
        fit_host(B, ts, e.data(), fixed.data(), lens.data(), g, dur.data(), rows.data());
        for (int b = 0; b < B; ++b) {
            for (int t = 0; t < lens[(size_t)b]; ++t) std::printf("%d ", dur[(size_t)b * ts + t]);
            for (int t = lens[(size_t)b]; t < ts; ++t)
                if (dur[(size_t)b * ts + t] != -1) return 3;
        }
        std::printf("\n");
        for (const int64_t v : rows) std::printf("%lld ", (long long)v);
        std::printf("\n");
    }
    return 0;
}
