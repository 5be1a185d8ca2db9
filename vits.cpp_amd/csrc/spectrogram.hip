// spectrogram.hip — the front end of voice conversion (engine_convert.cpp): the linear magnitude spectrogram of the input PCM
// (VITS mel_processing.spectrogram_torch, center = False) and the posterior sample z_q = mean + eps * exp(log_std).
//
// spectrogram_kernel: one block = FPB consecutive frames of one utterance. Every frame is independent (no cross-frame or
// cross-utterance reduction), so the result of a frame does not depend on the batch it was computed in. A frame is loaded with
// reflection indexing at the utterance's own ends (the pad of spectrogram_torch), multiplied by the periodic Hann window, placed in
// bit-reversed order in LDS as a complex vector (imaginary part 0) and transformed by a radix-2 decimation-in-time FFT in LDS; the
// magnitudes sqrt(re^2 + im^2 + 1e-6) of bins [0, n/2] go straight to the engine's [b][bin][t] layout, zero past the utterance's frames.
// The twiddles and the window come from tables built on the host in double precision (no v_sin_f32 / v_cos_f32: too coarse for a
// 1e-5 match). fp32 in every arithmetic mode.
//
// Traffic: each frame reads n_fft samples (the frames overlap: hop < n_fft, mostly from L2) and writes bins floats. A 1024-point FFT
// is 10 stages x 512 butterflies = ~50 kFLOP per frame, far below what a DFT-as-GEMM would cost (2 n (n + 2)), and below the
// memory time of the bins written.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "../../include/vits.h"
#include "../../include/vits_synth_noise.h"
#include "kernels.h"

namespace vits {

__global__ __launch_bounds__(256) void spectrogram_kernel(const float* __restrict__ pcm, int64_t pcm_stride, const int* __restrict__ n_samples,
                                                          const int* __restrict__ frames, const float2* __restrict__ tw, const float* __restrict__ win,
                                                          int log2n, int fpb, int hop, int pad, int bins, float* __restrict__ out, int64_t o_bs, int o_cs,
                                                          int tmax) {
    extern __shared__ float2 buf[];  // [fpb][n]
    const int b = blockIdx.y, t0 = blockIdx.x * fpb, tid = threadIdx.x;
    const int n = 1 << log2n;
    const int L = frames[b], N = n_samples[b];
    const float* y = pcm + (int64_t)b * pcm_stride;
    float* ob = out + (int64_t)b * o_bs;
    if (t0 >= L) {
        // past the utterance: zeros (the tensor is read as [b][bin][t] up to the batch's longest utterance)
        for (int i = tid; i < bins * fpb; i += 256) {
            const int k = i / fpb, t = t0 + i % fpb;
            if (t < tmax) ob[(int64_t)k * o_cs + t] = 0.f;
        }
        return;
    }
    for (int j = tid; j < fpb * n; j += 256) {
        const int f = j >> log2n, m = j & (n - 1), t = t0 + f;
        float v = 0.f;
        if (t < L) {
            int s = t * hop + m - pad;  // index into the utterance; reflection at both ends (requires pad < N)
            if (s < 0) s = -s;
            else if (s >= N) s = 2 * (N - 1) - s;
            v = y[s] * win[m];
        }
        const int r = (int)(__brev((unsigned)m) >> (32 - log2n));
        buf[f * n + r] = make_float2(v, 0.f);
    }
    __syncthreads();
    const int halfn = n >> 1;
    for (int s = 1; s <= log2n; ++s) {
        const int half = 1 << (s - 1);
        for (int q = tid; q < fpb * halfn; q += 256) {
            const int f = q >> (log2n - 1), r = q & (halfn - 1);
            const int pos = r & (half - 1), grp = r >> (s - 1);
            const int i0 = f * n + grp * 2 * half + pos, i1 = i0 + half;
            const float2 w = tw[pos << (log2n - s)];
            const float2 a = buf[i0], c = buf[i1];
            const float mr = c.x * w.x - c.y * w.y, mi = c.x * w.y + c.y * w.x;
            buf[i0] = make_float2(a.x + mr, a.y + mi);
            buf[i1] = make_float2(a.x - mr, a.y - mi);
        }
        __syncthreads();
    }
    // consecutive threads: consecutive frames of one bin (fpb contiguous floats per row)
    for (int i = tid; i < bins * fpb; i += 256) {
        const int k = i / fpb, f = i % fpb, t = t0 + f;
        if (t >= tmax) continue;
        float v = 0.f;
        if (t < L) {
            const float2 z = buf[f * n + k];
            v = sqrtf(z.x * z.x + z.y * z.y + 1e-6f);
        }
        ob[(int64_t)k * o_cs + t] = v;
    }
}

std::string stft_geometry(int n_fft, int hop) {
    if (n_fft < 16 || n_fft > 2048 || (n_fft & (n_fft - 1)))
        return "n_fft = " + std::to_string(n_fft) + ": the spectrogram kernel needs a power of two in [16, 2048]";
    if (hop < 1 || hop > n_fft || ((n_fft - hop) & 1))
        return "hop " + std::to_string(hop) + " does not fit n_fft " + std::to_string(n_fft) + ": 1 <= hop <= n_fft, and (n_fft - hop) / 2 must be a whole pad";
    return std::string();
}

void stft_tables(int n_fft, std::vector<float>& tw, std::vector<float>& win) {
    tw.assign((size_t)n_fft, 0.f);
    win.assign((size_t)n_fft, 0.f);
    const double pi = 3.14159265358979323846;
    for (int m = 0; m < n_fft / 2; ++m) {
        tw[2 * m] = (float)std::cos(2.0 * pi * m / n_fft);
        tw[2 * m + 1] = (float)-std::sin(2.0 * pi * m / n_fft);
    }
    for (int m = 0; m < n_fft; ++m) win[m] = (float)(0.5 - 0.5 * std::cos(2.0 * pi * m / n_fft));
}

hipError_t launch_spectrogram(const SpectrogramCall& c, hipStream_t s) {
    int log2n = 0;
    while ((1 << log2n) < c.n_fft) ++log2n;
    if ((1 << log2n) != c.n_fft || log2n < 4 || log2n > 11 || c.bins < 1 || c.bins > c.n_fft / 2 + 1 || c.hop <= 0 || c.pad < 0 || c.batch <= 0 ||
        c.tmax <= 0)
        return hipErrorInvalidValue;
    // 64 KB of LDS per block: 8 frames of a 1024-point FFT, 16 of the tiny models' 16-point ones
    const int fpb = std::min(16, std::max(1, 8192 >> log2n));
    dim3 grid((c.tmax + fpb - 1) / fpb, c.batch);
    VITS_KLAUNCH(spectrogram_kernel, grid, dim3(256), (size_t)fpb * c.n_fft * sizeof(float2), s, c.pcm, c.pcm_stride, c.n_samples, c.frames,
                 c.tw, c.win, log2n, fpb, c.hop, c.pad, c.bins, c.out.p, c.out.bs, c.out.cs, c.tmax);
    return hipGetLastError();
}

// z_q[b][c][t] = mean + (eps * eps_scale) * exp(log_std) for t < frames[b] (VitsPosteriorEncoder.forward), eps drawn like prior sampling's (zp_kernel,
// stage1_glue.hip: the counter stream VITS_STREAM_NOISE_PRIOR, index c * L + t, or the explicit / reference tensor). flip = 1 writes
// channel c to row F - 1 - c: the physical layout of the forward flow's input when the flow has an odd number of layers (engine_flow.cpp).
__global__ __launch_bounds__(256) void posterior_sample_kernel(const float* mean, int64_t m_bs, int m_cs, const float* logstd, int64_t v_bs, int v_cs,
                                                               const int* frames, const float* noise, int64_t n_bs, int n_cs, int noise_kind, uint64_t seed,
                                                               const int* seed_off, float* zq, int64_t z_bs, int z_cs, int channels, int flip, float eps_scale) {
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    const int L = frames[b];
    if (j >= L) return;
    const int cpb = (channels + gridDim.z - 1) / gridDim.z;
    const int c_end = min(channels, (int)(blockIdx.z + 1) * cpb);
    for (int c = blockIdx.z * cpb; c < c_end; ++c) {
        const float mu = mean[(int64_t)b * m_bs + (int64_t)c * m_cs + j];
        const float ls = logstd[(int64_t)b * v_bs + (int64_t)c * v_cs + j];
        float e = 0.f;
        if (eps_scale == 0.f) {
            zq[(int64_t)b * z_bs + (int64_t)(flip ? channels - 1 - c : c) * z_cs + j] = mu;  // the posterior mean: nothing drawn, nothing read
            continue;
        }
        if (noise_kind == VITS_NOISE_COUNTER) e = vits_counter_normal(seed + (uint64_t)(seed_off ? seed_off[b] : b), VITS_STREAM_NOISE_PRIOR, (uint64_t)c * L + j);
        else e = noise[(int64_t)b * n_bs + (int64_t)c * n_cs + j];
        const int row = flip ? channels - 1 - c : c;
        zq[(int64_t)b * z_bs + (int64_t)row * z_cs + j] = mu + (e * eps_scale) * expf(ls);
    }
}

hipError_t launch_posterior_sample(TensorRef mean, TensorRef logstd, const int* frames, TensorRef noise, int noise_kind, uint64_t seed, const int* seed_off,
                                   TensorRef zq, int batch, int channels, int lmax, int flip, hipStream_t s, float eps_scale) {
    if (batch <= 0 || lmax <= 0) return hipSuccess;
    dim3 grid((lmax + 255) / 256, batch, 16);
    VITS_KLAUNCH(posterior_sample_kernel, grid, dim3(256), 0, s, mean.p, mean.bs, mean.cs, logstd.p, logstd.bs, logstd.cs, frames, noise.p, noise.bs,
                 noise.cs, noise_kind, seed, seed_off, zq.p, zq.bs, zq.cs, channels, flip, eps_scale);
    return hipGetLastError();
}

}  // namespace vits
