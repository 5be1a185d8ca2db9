// loudness_host.cpp — the host side of levelling (include/vits.h vits_model_set_level): the K-weighting coefficients at any rate, the powers of the
// filter's state matrix that loudness.hip steps over sub-segments with, and the definition restated sequentially in double (vits_loudness_host).
// No device call in here: both public functions answer on a machine without a GPU.
#include <cmath>
#include <limits>

#include "../../include/vits.h"
#include "kernels.h"

namespace vits {

namespace {
constexpr double kPi = 3.14159265358979323846;

void matmul4(const double* a, const double* b, double* out) {
    double r[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double acc = 0.0;
            for (int k = 0; k < 4; ++k) acc += a[i * 4 + k] * b[k * 4 + j];
            r[i * 4 + j] = acc;
        }
    for (int i = 0; i < 16; ++i) out[i] = r[i];
}

// m^(2^log2n) by squaring
void matpow2(const double* m, int log2n, double* out) {
    double r[16];
    for (int i = 0; i < 16; ++i) r[i] = m[i];
    for (int i = 0; i < log2n; ++i) matmul4(r, r, r);
    for (int i = 0; i < 16; ++i) out[i] = r[i];
}

constexpr int ilog2(int v) { return v <= 1 ? 0 : 1 + ilog2(v / 2); }
static_assert((1 << ilog2(kLevelQ)) == kLevelQ && (1 << ilog2(kLevelGroup)) == kLevelGroup, "powers of two: the state matrices are built by squaring");
}  // namespace

bool loudness_plan(int rate, LoudnessPlan& p, std::string& err) {
    if (rate < kResampleMinRate || rate > kResampleMaxRate) {
        err = "rate " + std::to_string(rate) + " Hz is outside [" + std::to_string(kResampleMinRate) + ", " + std::to_string(kResampleMaxRate) + "]";
        return false;
    }
    p.rate = rate;
    p.S = (rate + 5) / 10;
    double* c = p.coef.c;
    {  // stage 1: the shelf
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(kPi * f0 / rate), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416), a0 = 1.0 + K / Q + K * K;
        c[0] = (Vh + Vb * K / Q + K * K) / a0;
        c[1] = 2.0 * (K * K - Vh) / a0;
        c[2] = (Vh - Vb * K / Q + K * K) / a0;
        c[3] = 2.0 * (K * K - 1.0) / a0;
        c[4] = (1.0 - K / Q + K * K) / a0;
    }
    {  // stage 2: the high-pass
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(kPi * f0 / rate), a0 = 1.0 + K / Q + K * K;
        c[5] = 1.0;
        c[6] = -2.0;
        c[7] = 1.0;
        c[8] = 2.0 * (K * K - 1.0) / a0;
        c[9] = (1.0 - K / Q + K * K) / a0;
    }
    // the homogeneous part of the cascade in transposed direct form II (kernels.h), v = (s1, s2, t1, t2)
    const double A[16] = {-c[3], 1.0, 0.0, 0.0,                      //
                          -c[4], 0.0, 0.0, 0.0,                      //
                          c[6] - c[8] * c[5], 0.0, -c[8], 1.0,       //
                          c[7] - c[9] * c[5], 0.0, -c[9], 0.0};
    matpow2(A, ilog2(kLevelQ), p.coef.AQ);
    matpow2(p.coef.AQ, ilog2(kLevelGroup), p.coef.AG);
    return true;
}

bool level_values_ok(int kind, float value_db, float ceiling_db, std::string& err) {
    if (kind < VITS_LEVEL_NONE || kind > VITS_LEVEL_LOUDNESS) {
        err = "unknown kind " + std::to_string(kind);
        return false;
    }
    auto inside = [&](const char* name, float v, int lo, int hi) {
        if (std::isfinite(v) && v >= (float)lo && v <= (float)hi) return true;
        err = std::string(name) + " = " + std::to_string(v) + " is outside [" + std::to_string(lo) + ", " + std::to_string(hi) + "] dB";
        return false;
    };
    if (kind == VITS_LEVEL_GAIN) return inside("value_db (a gain)", value_db, -60, 40);
    if (kind == VITS_LEVEL_PEAK) return inside("value_db (a sample peak)", value_db, -60, 0);
    if (kind == VITS_LEVEL_LOUDNESS) return inside("value_db (LUFS)", value_db, -70, 0) && inside("ceiling_db", ceiling_db, -60, 0);
    return true;
}

void loudness_host(const float* pcm, size_t n, const LoudnessPlan& p, double* lufs, double* peak, int* blocks) {
    const double* c = p.coef.c;
    const size_t S = (size_t)p.S, n_seg = n / S;
    std::vector<double> z(n_seg, 0.0);
    double s1 = 0, s2 = 0, t1 = 0, t2 = 0, pk = 0;
    for (size_t i = 0; i < n; ++i) {
        const double x = pcm[i];
        pk = std::max(pk, std::fabs(x));
        const double y1 = c[0] * x + s1;
        s1 = c[1] * x - c[3] * y1 + s2;
        s2 = c[2] * x - c[4] * y1;
        const double y2 = c[5] * y1 + t1;
        t1 = c[6] * y1 - c[8] * y2 + t2;
        t2 = c[7] * y1 - c[9] * y2;
        if (i / S < n_seg) z[i / S] += y2 * y2;
    }
    for (double& v : z) v /= (double)S;
    const double ninf = -std::numeric_limits<double>::infinity();
    if (peak) *peak = pk;
    if (lufs) *lufs = ninf;
    if (blocks) *blocks = 0;
    if (n_seg < 4) return;
    const size_t nb = n_seg - 3;
    std::vector<double> blk(nb), l(nb);
    for (size_t j = 0; j < nb; ++j) {
        blk[j] = (z[j] + z[j + 1] + z[j + 2] + z[j + 3]) / 4.0;
        l[j] = -0.691 + 10.0 * std::log10(blk[j]);
    }
    double sum = 0;
    size_t cnt = 0;
    for (size_t j = 0; j < nb; ++j)
        if (l[j] > -70.0) sum += blk[j], ++cnt;
    if (!cnt) return;
    const double gamma = -0.691 + 10.0 * std::log10(sum / (double)cnt) - 10.0;
    sum = 0, cnt = 0;
    for (size_t j = 0; j < nb; ++j)
        if (l[j] > -70.0 && l[j] > gamma) sum += blk[j], ++cnt;
    if (!cnt) return;
    if (lufs) *lufs = -0.691 + 10.0 * std::log10(sum / (double)cnt);
    if (blocks) *blocks = (int)cnt;
}

size_t level_scratch_bytes(int batch, int64_t max_len, int S) {
    const size_t nq = (size_t)((max_len + kLevelQ - 1) / kLevelQ) + 1, nseg = (size_t)(max_len / std::max(S, 1)) + 1;
    // per row: states [nq][4] double | partial sums [nq][2] double | segment means [nseg] double | peaks [nq] float (+ one float of padding to 8 bytes)
    return (size_t)batch * (nq * (4 + 2) * sizeof(double) + nseg * sizeof(double) + (nq + (nq & 1)) * sizeof(float)) + 256;
}

}  // namespace vits
