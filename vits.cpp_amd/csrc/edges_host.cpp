// edges_host.cpp — the host side of the edges stage (include/vits.h vits_model_set_edges): the sample counts of a desc at a rate, the fade tables, the
// scratch edges.hip needs, and the definition evaluated sequentially (vits_edges_host). No device call in here: both public functions answer on a machine
// without a GPU.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/vits.h"
#include "kernels.h"

namespace vits {

namespace {
constexpr double kPi = 3.14159265358979323846;

std::string fmt(float v) {
    char buf[32];
    std::snprintf(buf, sizeof(buf), "%.9g", (double)v);
    return buf;
}
}  // namespace

bool edges_plan(int rate, const ::vits_edges_desc& d, EdgesPlan& p, std::string& err) {
    if (d.struct_size != sizeof(vits_edges_desc)) {
        err = "struct_size = " + std::to_string(d.struct_size) + " is not sizeof(vits_edges_desc) = " + std::to_string(sizeof(vits_edges_desc));
        return false;
    }
    if (d.mode < VITS_EDGES_OFF || d.mode > VITS_EDGES_TRIM_ABSOLUTE) {
        err = "unknown mode " + std::to_string(d.mode);
        return false;
    }
    if (rate < kResampleMinRate || rate > kResampleMaxRate) {
        err = "rate " + std::to_string(rate) + " Hz is outside [" + std::to_string(kResampleMinRate) + ", " + std::to_string(kResampleMaxRate) + "]";
        return false;
    }
    const bool trims = d.mode == VITS_EDGES_TRIM_RELATIVE || d.mode == VITS_EDGES_TRIM_ABSOLUTE;
    if (trims && !(std::isfinite(d.threshold_db) && d.threshold_db >= -120.f && d.threshold_db <= 0.f)) {
        err = "threshold_db = " + fmt(d.threshold_db) + " must be finite and in [-120, 0] dB";
        return false;
    }
    const float ms[6] = {d.keep_head_ms, d.keep_tail_ms, d.fade_in_ms, d.fade_out_ms, d.lead_ms, d.tail_ms};
    const char* names[6] = {"keep_head_ms", "keep_tail_ms", "fade_in_ms", "fade_out_ms", "lead_ms", "tail_ms"};
    int64_t cnt[6];
    for (int i = 0; i < 6; ++i) {
        if (!(std::isfinite(ms[i]) && ms[i] >= 0.f && ms[i] <= 2000.f)) {
            err = std::string(names[i]) + " = " + fmt(ms[i]) + " must be finite and in [0, 2000] ms";
            return false;
        }
        cnt[i] = (int64_t)std::floor((double)ms[i] * rate / 1000 + 0.5);
    }
    EdgesPlan q;
    q.rate = rate;
    q.mode = d.mode;
    q.W = (rate + 50) / 100;
    q.Kh = cnt[0], q.Kt = cnt[1], q.Fi = cnt[2], q.Fo = cnt[3], q.Pl = cnt[4], q.Pt = cnt[5];
    q.tile = kEdgesTileTarget / q.W * q.W;
    q.f = trims ? std::pow(10.0, (double)d.threshold_db / 10.0) : 1.0;
    p = q;
    return true;
}

std::vector<float> edges_fades(const EdgesPlan& p) {
    std::vector<float> t((size_t)(p.Fi + p.Fo));
    for (int64_t k = 0; k < p.Fi; ++k) t[(size_t)k] = (float)(0.5 - 0.5 * std::cos(kPi * ((double)k + 0.5) / (double)p.Fi));
    for (int64_t k = 0; k < p.Fo; ++k) t[(size_t)(p.Fi + k)] = (float)(0.5 - 0.5 * std::cos(kPi * ((double)k + 0.5) / (double)p.Fo));
    return t;
}

size_t edges_scratch_bytes(int batch, int64_t max_len, int W) {
    const size_t n_win = (size_t)((max_len + W - 1) / std::max(W, 1)) + 1;
    return (size_t)batch * n_win * sizeof(double) + 256;
}

void edges_host(const float* pcm, int64_t n, const EdgesPlan& p, const float* fades, float* y, int64_t row[4]) {
    const int64_t N = n, W = p.W;
    int64_t a = 0, b = 0, n_active = 0;
    if (p.mode == VITS_EDGES_PAD) b = N;
    else {
        const int64_t n_win = (N + W - 1) / W;
        std::vector<double> q((size_t)n_win);
        double q_max = 0.0;
        for (int64_t i = 0; i < n_win; ++i) {
            const int64_t lo = i * W, hi = std::min(lo + W, N);
            double acc = 0.0;
            for (int64_t k = lo; k < hi; ++k) acc += (double)pcm[k] * (double)pcm[k];
            q[(size_t)i] = acc / (double)(hi - lo);
            if (q[(size_t)i] > q_max) q_max = q[(size_t)i];  // (a NaN compares false)
        }
        const double T = p.mode == VITS_EDGES_TRIM_RELATIVE ? q_max * p.f : p.f;
        int64_t first = -1, last = -1;
        for (int64_t i = 0; i < n_win; ++i)
            if (q[(size_t)i] >= T && q[(size_t)i] > 0.0) {
                if (first < 0) first = i;
                last = i;
                ++n_active;
            }
        if (n_active) {
            a = std::max<int64_t>(0, first * W - p.Kh);
            b = std::min(N, (last + 1) * W + p.Kt);
        }
    }
    const int64_t M = b - a, Np = p.Pl + M + p.Pt;
    if (y) {
        const float *win = fades, *wout = fades ? fades + p.Fi : nullptr;
        for (int64_t j = 0; j < p.Pl; ++j) y[j] = 0.f;
        for (int64_t k = 0; k < M; ++k) {
            const float wi = k < p.Fi ? win[k] : 1.f, wo = M - 1 - k < p.Fo ? wout[M - 1 - k] : 1.f;
            const float v = pcm[a + k] * wi;
            y[p.Pl + k] = v * wo;
        }
        for (int64_t j = p.Pl + M; j < p.bound(N); ++j) y[j] = 0.f;
    }
    if (row) row[0] = a, row[1] = b, row[2] = Np, row[3] = n_active;
}

}  // namespace vits
