// fit_host.cpp — a stated duration on the host (include/vits.h "a stated duration"): the definition the kernel (fit.hip) and the numpy restatement
// (tests/fit_ref.py) agree with on every integer. IEEE fp32 multiply, ceilf and integer arithmetic only; nothing here touches the device.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "kernels.h"

namespace vits {

namespace {
uint32_t bits_of(float s) {
    uint32_t u;
    std::memcpy(&u, &s, sizeof(u));
    return u;
}
float float_of(uint32_t u) {
    float s;
    std::memcpy(&s, &u, sizeof(s));
    return s;
}
// c_t(s): a free token's frames at the scale s
int64_t token_frames(float e, float s) {
    const float x = std::ceil(e * s);
    return x < kFitMaxTokenFrames ? (int64_t)x : (int64_t)kFitMaxTokenFrames;
}
std::string fmt(float v) {
    char buf[48];
    std::snprintf(buf, sizeof(buf), "%.9g", (double)v);
    return buf;
}
}  // namespace

bool fit_limits(float min_rate, float max_rate, float& s_lo, float& s_hi, std::string& err) {
    if (!std::isfinite(min_rate) || !std::isfinite(max_rate) || min_rate < kFitMinRate || max_rate > kFitMaxRate || min_rate > max_rate) {
        err = "min_rate = " + fmt(min_rate) + ", max_rate = " + fmt(max_rate) + ": 0.1 <= min_rate <= max_rate <= 10 is required";
        return false;
    }
    // (the engine's own expression for a rate's length scale: a clamped fit is a speaking_rates call)
    s_lo = (float)(1.0 / (double)max_rate);
    s_hi = (float)(1.0 / (double)min_rate);
    return true;
}

bool fit_check(int batch, const int* group, const int64_t* target, std::string& err) {
    for (int b = 0; b < batch; ++b) {
        if (group && (group[b] < 0 || group[b] >= batch)) {
            err = "groups[" + std::to_string(b) + "] = " + std::to_string(group[b]) + ": outside [0, " + std::to_string(batch) + ")";
            return false;
        }
        if (target[b] != 0 && (target[b] < 1 || target[b] > kFitMaxTarget)) {
            err = "target_frames[" + std::to_string(b) + "] = " + std::to_string(target[b]) + " (group " + std::to_string(b) +
                  "): a target is 1 to 2^22 frames, or 0 for a group that is not fitted";
            return false;
        }
    }
    return true;
}

bool fit_check_rows(int batch, int t_stride, const int* fixed, const int* lens, std::string& err) {
    if (batch < 1 || t_stride < 1) {
        err = "batch >= 1 and t_stride >= 1 are required";
        return false;
    }
    for (int b = 0; b < batch; ++b) {
        const int len = lens ? lens[b] : t_stride;
        if (len < 0 || len > t_stride) {
            err = "lens[" + std::to_string(b) + "] = " + std::to_string(len) + ": outside [0, t_stride = " + std::to_string(t_stride) + "]";
            return false;
        }
        for (int t = 0; fixed && t < len; ++t) {
            const int v = fixed[(size_t)b * t_stride + t];
            if (v < -1 || v > (int)kFitMaxTokenFrames) {
                err = "fixed[" + std::to_string(b) + "][" + std::to_string(t) + "] = " + std::to_string(v) + ": -1 (a free token) or 0 to 2^24 frames";
                return false;
            }
        }
    }
    return true;
}

void fit_rows_double(int groups, const int64_t* rows, double* out) {
    for (int g = 0; g < groups; ++g) {
        const int64_t* r = rows + (size_t)kFitRowInts * g;
        double* o = out + (size_t)kFitRowInts * g;
        o[0] = (double)r[0], o[1] = (double)r[1], o[2] = r[4] < 0 ? 0.0 : (double)float_of((uint32_t)r[2]), o[3] = (double)r[3], o[4] = (double)r[4];
    }
}

void fit_host(int batch, int t_stride, const float* e, const int* fixed, const int* lens, const FitGroups& gr, int* dur, int64_t* rows) {
    auto len_of = [&](int b) { return lens ? lens[b] : t_stride; };
    auto fixed_of = [&](int b, int t) { return fixed ? fixed[(size_t)b * t_stride + t] : -1; };
    for (int b = 0; b < batch; ++b)
        for (int t = 0; t < t_stride; ++t) dur[(size_t)b * t_stride + t] = t < len_of(b) ? fixed_of(b, t) : -1;
    for (int g = 0; g < batch; ++g) {
        int64_t* row = rows + (size_t)kFitRowInts * g;
        const int64_t F = gr.target[g];
        row[0] = F, row[1] = 0, row[2] = 0, row[3] = 0, row[4] = -1;
        std::vector<int> members;
        for (int b = 0; b < batch; ++b)
            if ((gr.group ? gr.group[b] : b) == g) members.push_back(b);
        if (F == 0 || members.empty()) continue;
        auto frames_at = [&](int b, int t, float s) {
            const int v = fixed_of(b, t);
            return v >= 0 ? (int64_t)v : token_frames(e[(size_t)b * t_stride + t], s);
        };
        auto n_of = [&](float s) {
            int64_t n = 0;
            for (int b : members)
                for (int t = 0; t < len_of(b); ++t) n += frames_at(b, t, s);
            return n;
        };
        uint32_t lo = bits_of(gr.s_lo), hi = bits_of(gr.s_hi);
        int64_t status = 0, R = 0;
        bool remainder = false;
        if (n_of(gr.s_lo) > F) {
            status = 1;
        } else if (const int64_t n_hi = n_of(gr.s_hi); n_hi <= F) {
            lo = hi;
            status = n_hi == F ? 0 : 2;
        } else {
            // n(lo) <= F < n(hi) throughout
            while (hi - lo > 1) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (n_of(float_of(mid)) <= F) lo = mid;
                else hi = mid;
            }
            remainder = true;
        }
        const float s = float_of(lo), s_next = float_of(lo + 1);
        int64_t sum = 0;
        for (int b : members)
            for (int t = 0; t < len_of(b); ++t) sum += frames_at(b, t, s);
        int64_t left = R = remainder ? F - sum : 0;
        for (int b : members)
            for (int t = 0; t < len_of(b); ++t) {
                int64_t d = frames_at(b, t, s);
                if (left > 0) {
                    const int64_t take = std::min(frames_at(b, t, s_next) - d, left);
                    d += take, left -= take, sum += take;
                }
                dur[(size_t)b * t_stride + t] = (int)d;
            }
        row[1] = sum, row[2] = (int64_t)lo, row[3] = R, row[4] = status;
    }
}

}  // namespace vits
