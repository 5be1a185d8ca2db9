// pitch_host.cpp — the varispeed stage's definition on the host (kernels.h PitchPlan; include/vits.h "a stated pitch"): the integers of a row, the two
// tables and the sequential evaluation in double. No kernel, no device: it links alone.
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/vits.h"
#include "kernels.h"

namespace vits {

namespace {
constexpr double kBeta = 9.0;
// modified Bessel function of the first kind, order 0, by its power series (the resampler's, engine_support.cpp: this file links without it)
double bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int m = 1; m < 1000; ++m) {
        term *= q / ((double)m * (double)m);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}
}  // namespace

bool pitch_plan(float ratio, int64_t n, PitchPlan& p, std::string& err) {
    if (!std::isfinite(ratio) || ratio < kPitchMinRatio || ratio > kPitchMaxRatio) {
        err = "pitch ratio " + std::to_string(ratio) + " is not finite or outside [0.5, 2]";
        return false;
    }
    if (n < 0 || n > kPitchMaxLen) {
        err = "a row of " + std::to_string(n) + " samples is outside [0, 2^30]";
        return false;
    }
    PitchPlan q;
    q.P = (int64_t)((double)ratio * (double)kPitchOne);  // (exact: a float in [0.5, 2] is a multiple of 2^-24)
    q.S = q.P <= kPitchOne ? kPitchS0 : (kPitchS0 << 24) / q.P;
    q.R = (int)((((int64_t)1 << 29) + q.S - 1) / q.S);
    q.K = 2 * q.R + 1;
    q.n_out = (n * kPitchOne + q.P - 1) / q.P;
    p = q;
    return true;
}

std::vector<float> pitch_table() {
    const double pi = 3.14159265358979323846, i0b = bessel_i0(kBeta);
    const int ZQ = kPitchZ * kPitchQ;
    std::vector<float> t((size_t)2 * kPitchTableN, 0.f);
    float* G = t.data();
    float* D = G + kPitchTableN;
    for (int i = 0; i < ZQ; ++i) {
        const double u = (double)i / kPitchQ, w = u / kPitchZ, a = pi * u;
        G[i] = (float)((a == 0.0 ? 1.0 : std::sin(a) / a) * bessel_i0(kBeta * std::sqrt(1.0 - w * w)) / i0b);
    }
    // (G[ZQ] = G[ZQ + 1] = 0 by definition)
    for (int i = 0; i <= ZQ; ++i) D[i] = G[i + 1] - G[i];
    return t;
}

std::vector<float> pitch_table_pairs() {
    const std::vector<float> t = pitch_table();
    std::vector<float> gd((size_t)2 * kPitchTableN);
    for (int i = 0; i < kPitchTableN; ++i) gd[(size_t)2 * i] = t[(size_t)i], gd[(size_t)2 * i + 1] = t[(size_t)kPitchTableN + i];
    return gd;
}

void pitch_host(const float* x, int64_t n, const PitchPlan& p, const float* table, double* y) {
    const float* G = table;
    const float* D = table + kPitchTableN;
    const double a = (double)p.S / (double)kPitchOne;
    if (p.P == kPitchOne) {  // (ratio 1 is a copy by definition: the filter there is a low-pass, not an identity)
        for (int64_t m = 0; m < n; ++m) y[m] = (double)x[m];
        return;
    }
    for (int64_t m = 0; m < p.n_out; ++m) {
        const int64_t t = m * p.P, n0 = t >> 24, f = t & (kPitchOne - 1);
        double acc = 0.0;
        for (int k = 0; k < p.K; ++k) {
            const int64_t idx = n0 - p.R + k;
            const int64_t d = (int64_t)(k - p.R) * kPitchOne - f, tau = d < 0 ? -d : d;
            const int64_t u = (tau * p.S) >> 24, i = u >> 16;
            if (i >= kPitchZ * kPitchQ || idx < 0 || idx >= n) continue;
            const double fr = (double)(u & 65535) * (1.0 / 65536.0);
            acc += a * (fr * (double)D[i] + (double)G[i]) * (double)x[idx];
        }
        y[m] = acc;
    }
}

}  // namespace vits
