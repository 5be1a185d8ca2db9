// limiter_host.cpp — the host side of the true-peak limiter (include/vits.h vits_model_set_limiter): its constants at a rate, the scratch limiter.hip
// needs, and the definition restated sequentially in double (vits_limiter_host). No device call in here: both public functions answer on a machine
// without a GPU.
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/vits.h"
#include "kernels.h"

namespace vits {

bool limiter_plan(int rate, LimiterPlan& p, std::string& err) {
    if (rate < kResampleMinRate || rate > kLimitMaxRate) {
        err = "rate " + std::to_string(rate) + " Hz is outside [" + std::to_string(kResampleMinRate) + ", " + std::to_string(kLimitMaxRate) +
              "] (the true-peak meter runs at four times the rate, and the resampler's filter ends at " + std::to_string(kResampleMaxRate) + " Hz)";
        return false;
    }
    LimiterPlan q;
    q.rate = rate;
    q.A = (rate + 100) / 200;
    q.H = (rate + 10) / 20;
    if (!resample_plan(rate, 4 * rate, q.up, err)) return false;
    p = q;
    return true;
}

size_t limit_scratch_bytes(int batch, int64_t max_len) {
    const size_t tiles = (size_t)((max_len + kLimitTile - 1) / kLimitTile) + 1;
    // per row: the envelope [max_len rounded up to four] | tile maxima of x and of y [tiles] each | tile statistics [tiles][2]
    return (size_t)batch * (((size_t)max_len + 3) / 4 * 4 + tiles * 4) * sizeof(float) + 256;
}

namespace {
// the row at four times its rate, in double: u[j] = sum_k h[j % 4][k] x[j / 4 - R + k], zero outside the row
template <class T>
std::vector<double> oversample(const T* x, size_t n, const ResamplePlan& rp, const float* taps) {
    std::vector<double> u(4 * n);
    for (size_t j = 0; j < 4 * n; ++j) {
        const int64_t nc = (int64_t)(j / 4);
        const float* h = taps + (j % 4) * (size_t)rp.K;
        double acc = 0.0;
        for (int k = 0; k < rp.K; ++k) {
            const int64_t i = nc - rp.R + k;
            if (i >= 0 && i < (int64_t)n) acc += (double)h[k] * (double)x[i];
        }
        u[j] = acc;
    }
    return u;
}
template <class T>
double true_peak(const T* x, size_t n, const std::vector<double>& u) {
    double tp = 0.0;
    for (size_t i = 0; i < n; ++i) tp = std::max(tp, std::fabs((double)x[i]));
    for (double v : u) tp = std::max(tp, std::fabs(v));
    return tp;
}
}  // namespace

void limiter_host(const float* pcm, size_t n, const LimiterPlan& p, const float* taps, double g0, double c, double* y, double limits[4]) {
    const int64_t N = (int64_t)n, A = p.A, H = p.H;
    const std::vector<double> u = oversample(pcm, n, p.up, taps);
    // r over [0, N); 1 outside
    std::vector<double> r(n);
    for (int64_t k = 0; k < N; ++k) {
        double e = std::fabs((double)pcm[k]);
        for (int64_t j = std::max<int64_t>(4 * k - 2, 0); j <= std::min<int64_t>(4 * k + 2, 4 * N - 1); ++j) e = std::max(e, std::fabs(u[(size_t)j]));
        r[(size_t)k] = e == 0.0 ? 1.0 : std::min(1.0, c / (g0 * e));
    }
    auto r_at = [&](int64_t k) { return k >= 0 && k < N ? r[(size_t)k] : 1.0; };
    // m[j] = min r[j - H .. j + A], j in [-A, N), kept at index j + A: a monotonic queue of the indices whose r can still be a window's minimum
    std::vector<double> m((size_t)(N + A));
    {
        std::vector<int64_t> q((size_t)(N + 2 * A + H + 1));
        size_t head = 0, tail = 0;
        int64_t next = -A - H;  // the next index to enter
        for (int64_t j = -A; j < N; ++j) {
            for (; next <= j + A; ++next) {
                const double v = r_at(next);
                while (tail > head && r_at(q[tail - 1]) >= v) --tail;
                q[tail++] = next;
            }
            while (q[head] < j - H) ++head;
            m[(size_t)(j + A)] = r_at(q[head]);
        }
    }
    std::vector<double> yy(n);
    double smin = 1.0;
    int64_t below = 0;
    for (int64_t i = 0; i < N; ++i) {
        double acc = 0.0;
        for (int64_t k = 0; k <= A; ++k) acc += m[(size_t)(i + k)];  // m[i - A .. i]
        const double s = acc / (double)(A + 1);
        smin = std::min(smin, s);
        below += s < 1.0;
        yy[(size_t)i] = (double)pcm[i] * (g0 * s);
    }
    if (y) std::copy(yy.begin(), yy.end(), y);
    if (limits) {
        limits[0] = true_peak(pcm, n, u);
        limits[1] = true_peak(yy.data(), n, oversample(yy.data(), n, p.up, taps));
        limits[2] = smin;
        limits[3] = N ? (double)below / (double)N : 0.0;
    }
}

}  // namespace vits
