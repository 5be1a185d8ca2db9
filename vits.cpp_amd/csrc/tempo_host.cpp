// tempo_host.cpp — the time-stretch stage's definition on the host (kernels.h TempoPlan; include/vits.h "a stated tempo"): the integers of a row, the
// integer search and the overlap-add in fp32, sequentially. No kernel, no device: it links alone.
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/vits.h"
#include "kernels.h"

// (the overlap-add is two rounded products and one rounded add: never a fused multiply-add)
#pragma STDC FP_CONTRACT OFF

namespace vits {

bool tempo_plan(int rate, float tempo, int64_t n, TempoPlan& p, std::string& err) {
    if (rate < kTempoMinRate || rate > kTempoMaxRate) {
        err = "rate " + std::to_string(rate) + " is outside [8000, 48000]";
        return false;
    }
    if (!std::isfinite(tempo) || tempo < kTempoMin || tempo > kTempoMax) {
        err = "tempo " + std::to_string(tempo) + " is not finite or outside [0.5, 2]";
        return false;
    }
    if (n < 0 || n > kTempoMaxLen) {
        err = "a row of " + std::to_string(n) + " samples is outside [0, 2^30]";
        return false;
    }
    TempoPlan q;
    q.H = 4 * (rate / 400);
    q.D = 4 * (rate / 500);
    q.Q = (int64_t)((double)tempo * (double)kTempoOne);  // (exact: a float in [0.5, 2] is a multiple of 2^-24)
    q.n_out = (n * kTempoOne + q.Q - 1) / q.Q;
    q.F = (q.n_out + q.H - 1) / q.H;
    p = q;
    return true;
}

namespace {
// the search signal: 0 for a NaN and outside the row, else the sample at 16 bits, rounded to nearest even and clamped
inline int quantise(const float* x, int64_t n, int64_t idx) {
    if (idx < 0 || idx >= n) return 0;
    const float v = x[idx];
    if (std::isnan(v)) return 0;
    const float r = std::nearbyint(v * 32768.0f);  // (the default rounding mode: to nearest even; the product is exact)
    return r <= -32768.0f ? -32768 : r >= 32767.0f ? 32767 : (int)r;
}
inline float sample(const float* x, int64_t n, int64_t idx) { return idx < 0 || idx >= n ? 0.f : x[idx]; }
}  // namespace

void tempo_host(const float* x, int64_t n, const TempoPlan& p, float* y, int32_t* offsets) {
    const int H = p.H, D = p.D;
    if (p.Q == kTempoOne) {  // (tempo 1 is a copy by definition; its search finds 0 everywhere: the template is the candidate)
        for (int64_t m = 0; m < n; ++m) y[m] = x[m];
        for (int64_t k = 0; offsets && k < p.F; ++k) offsets[k] = 0;
        return;
    }
    std::vector<float> w((size_t)H);
    for (int i = 0; i < H; ++i) w[(size_t)i] = (float)(2 * i + 1) / (float)(2 * H);
    std::vector<int> tpl((size_t)H), reg((size_t)(2 * D + H));
    int64_t s_prev2 = -H, s_prev = 0;  // s_(k-2), s_(k-1)
    for (int64_t k = 1; k <= p.F; ++k) {
        const int64_t a = (k * H * p.Q) >> 24, c = s_prev + H;
        for (int i = 0; i < H; ++i) tpl[(size_t)i] = quantise(x, n, c + i);
        for (int j = 0; j < 2 * D + H; ++j) reg[(size_t)j] = quantise(x, n, a - D + j);
        int best = 0;
        int64_t best_sad = -1;
        for (int r = 0; r <= 2 * D; ++r) {  // the order 0, -1, +1, -2, +2, ...: a later candidate wins only by a smaller sum
            const int d = r == 0 ? 0 : (r & 1) ? -((r + 1) / 2) : r / 2;
            const int* cand = reg.data() + (d + D);
            int64_t sad = 0;
            for (int i = 0; i < H; ++i) sad += std::abs(tpl[(size_t)i] - cand[i]);
            if (best_sad < 0 || sad < best_sad) best_sad = sad, best = d;
        }
        if (offsets) offsets[k - 1] = best;
        const int64_t s = a + best;
        // frame k - 1: the segment before going on, fading out, under segment k - 1 fading in
        const int64_t m0 = (k - 1) * H;
        for (int i = 0; i < H && m0 + i < p.n_out; ++i) {
            const float t0 = w[(size_t)(H - 1 - i)] * sample(x, n, s_prev2 + H + i);
            const float t1 = w[(size_t)i] * sample(x, n, s_prev + i);
            y[m0 + i] = t0 + t1;
        }
        s_prev2 = s_prev;
        s_prev = s;
    }
}

}  // namespace vits
