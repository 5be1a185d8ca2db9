// tempo_host_driver — the time stretch's host definition (vits.cpp_amd/csrc/tempo_host.cpp ALONE: no kernel, no device) as a stand-alone program, for
// tests/test_tempo_host.py, which builds it under AddressSanitizer + UBSan and runs it. Rows of pseudo-random samples (NaN, Inf and over-range values among
// them) in buffers of EXACTLY n, N' and F elements, so that a read or a write one element out of place is the sanitizer's to find; every length around the hop
// and the candidate region at both rates and every tempo of the test. Prints one line per case, "rate tempo n n_out F checksum sum(offsets)", and exits 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../vits.cpp_amd/csrc/kernels.h"

using namespace vits;

int main() {
    const int rates[] = {8000, 16000, 22050, 48000};
    const float tempos[] = {0.5f, 0.890898718f, 1.0f - 5.9604645e-8f, 1.0f, 1.0f + 1.1920929e-7f, 1.122462048f, 1.5f, 2.0f};
    uint32_t lcg = 12345u;
    for (const int rate : rates)
        for (const float q : tempos) {
            TempoPlan p0;
            std::string err;
            if (!tempo_plan(rate, q, 0, p0, err)) {
                std::fprintf(stderr, "%s\n", err.c_str());
                return 1;
            }
            const int H = p0.H, D = p0.D;
            const int64_t lens[] = {0, 1, 2, H - 1, H, H + 1, 2 * H - 1, 2 * H + 1, 2 * D + H - 1, 2 * D + H + 1, 1000, 3001};
            for (const int64_t n : lens) {
                TempoPlan p;
                if (!tempo_plan(rate, q, n, p, err)) {
                    std::fprintf(stderr, "%s\n", err.c_str());
                    return 1;
                }
                std::vector<float> x((size_t)n), y((size_t)p.n_out);
                std::vector<int32_t> off((size_t)p.F);
                for (auto& v : x) {
                    lcg = lcg * 1664525u + 1013904223u;
                    v = ((float)(lcg >> 8) / 8388608.0f - 1.0f) * 1.2f;
                    if ((lcg & 255u) == 7u) v = std::numeric_limits<float>::quiet_NaN();
                    if ((lcg & 255u) == 9u) v = std::numeric_limits<float>::infinity();
                }
                tempo_host(x.data(), n, p, y.data(), off.data());
                double sum = 0;
                for (const float v : y)
                    if (std::isfinite(v)) sum += v;
                long long osum = 0;
                for (const int32_t d : off) {
                    if (d < -D || d > D) {
                        std::fprintf(stderr, "offset %d outside [-%d, %d]\n", d, D, D);
                        return 1;
                    }
                    osum += d;
                }
                std::printf("%d %.9g %lld %lld %lld %.6f %lld\n", rate, (double)q, (long long)n, (long long)p.n_out, (long long)p.F, sum, osum);
            }
        }
    // the refusals
    TempoPlan p;
    std::string err;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    if (tempo_plan(7999, 1.f, 0, p, err) || tempo_plan(48001, 1.f, 0, p, err) || tempo_plan(16000, 0.49f, 0, p, err) || tempo_plan(16000, 2.01f, 0, p, err) ||
        tempo_plan(16000, nan, 0, p, err) || tempo_plan(16000, 1.f, -1, p, err) || tempo_plan(16000, 1.f, ((int64_t)1 << 30) + 1, p, err)) {
        std::fprintf(stderr, "a plan that must be refused was accepted\n");
        return 1;
    }
    return 0;
}
