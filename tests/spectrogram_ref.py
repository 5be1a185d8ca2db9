"""numpy side of the spectrogram operator tests (tests/test_gpu_spectrogram_ops.py, tests/test_glue_op_host.py, tests/test_vc_host.py): the float64 reference of
vits.cpp_amd/csrc/spectrogram.hip's spectrogram_kernel, an fp32 restatement of its own arithmetic, the geometry rule of the engine and the case tables.

The operation (VITS spectrogram_torch, center = False): utterance y of N samples, reflection pad (n_fft - hop) / 2 at both ends, N // hop frames of n_fft samples
hop apart, periodic Hann window, magnitudes sqrt(re^2 + im^2 + 1e-6) of bins [0, bins).
  * spectrogram64: float64, np.fft.rfft.
  * spectrogram32: what the kernel computes, step by step in fp32: the window and the twiddles from tables built in double and rounded once, the windowed frame in
    bit-reversed order, log2(n_fft) radix-2 decimation-in-time stages (m = c w as four products and two sums, a + m, a - m), then sqrtf(re re + im im + 1e-6f).
    Every operation is rounded on its own (the device contracts some a b + c into one rounding): its error against float64 is what the 2x rule of
    tests/split_ref.py doubles.
The geometry rule (stft_geometry, stft_min_samples in the library): n_fft a power of two in [16, 2048], 1 <= hop <= n_fft, n_fft - hop even, N >= max(hop, pad + 1)."""
import numpy as np

N_FFTS = (16, 32, 64, 256, 1024, 2048)
BATCH = 4


def fpb_of(n_fft):
    """frames per block of launch_spectrogram: 16 up to n_fft 512, 8 at 1024, 4 at 2048"""
    return min(16, max(1, 8192 // n_fft))


def pad_of(n_fft, hop):
    return (n_fft - hop) // 2


def min_samples(n_fft, hop):
    return max(hop, pad_of(n_fft, hop) + 1)


def geometry_ok(n_fft, hop):
    return 16 <= n_fft <= 2048 and not (n_fft & (n_fft - 1)) and 1 <= hop <= n_fft and not ((n_fft - hop) & 1)


def hops_of(n_fft):
    return sorted({n_fft, n_fft // 2, n_fft // 4, n_fft - 2, 2})


def frame_counts(n_fft):
    f = fpb_of(n_fft)
    return (1, f - 1, f, f + 1, 2 * f + 3)


def case_lengths(n_fft, hop):
    """The utterances of the case (n_fft, hop): the shortest legal one and one sample more, then every frames * hop + r with frames on the block edges and
    r = N mod hop in {0, 1, hop - 1} that is legal (long enough for the reflection), shortest first. Where the reflection needs more frames than those (a small
    hop under a large n_fft), the first block edge above the shortest utterance's frame count stands in: m - 1, m, m + 1 frames for that multiple m of fpb."""
    mn = min_samples(n_fft, hop)
    out = {mn, mn + 1}
    m = (mn // hop // fpb_of(n_fft) + 1) * fpb_of(n_fft)
    for f in frame_counts(n_fft) + (m - 1, m, m + 1):
        for r in sorted({0, 1 % hop, hop - 1}):
            if f * hop + r >= mn:
                out.add(f * hop + r)
    return sorted(out)


def bins_of(n_fft):
    return (n_fft // 2 + 1, n_fft // 2, 1)


def signal(n_fft, hop, n, row, quiet):
    """noise (sigma 1, or 1e-4 in the quiet draw) + a tone on the centre of bin n_fft / 4 + 1 + a DC offset: the Hann window spreads a bin-centred tone and the
    offset over three bins each and no further, so in the quiet draw every other bin sits at the floor sqrt(1e-6) = 1e-3, where only the 1e-6 keeps the root finite"""
    rng = np.random.default_rng(((n_fft * 4099 + hop) * 8209 + n) * 8 + row * 2 + int(quiet))
    m = np.arange(n)
    k0 = n_fft // 4 + 1
    y = rng.standard_normal(n) * (1e-4 if quiet else 1.0) + 0.5 * np.cos(2 * np.pi * k0 * m / n_fft + 0.3) + 0.1
    return y.astype(np.float32)


def np_spectrogram(y, n_fft, hop):
    """spectrogram_torch (center=False) in numpy alone: reflection pad, periodic Hann, rfft, sqrt(|X|^2 + 1e-6)"""
    p = (n_fft - hop) // 2
    yp = np.pad(y.astype(np.float64), (p, p), mode="reflect")
    L = (yp.size - n_fft) // hop + 1
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)
    frames = np.stack([yp[t * hop:t * hop + n_fft] * win for t in range(L)])
    X = np.fft.rfft(frames, axis=1)
    return np.sqrt(X.real ** 2 + X.imag ** 2 + 1e-6).T


def spectrogram64(y, n_fft, hop, bins=None):
    """float64 [bins, N // hop]"""
    s = np_spectrogram(np.asarray(y), n_fft, hop)
    assert s.shape[1] == len(y) // hop, (s.shape, len(y), hop)
    return s[:n_fft // 2 + 1 if bins is None else bins]


def tables32(n_fft):
    """(twiddle re, twiddle im) [n_fft / 2] and the periodic Hann window [n_fft]: float64 expressions rounded once to fp32, as stft_tables builds them"""
    m = np.arange(n_fft // 2)
    tw_re = np.cos(2.0 * np.pi * m / n_fft).astype(np.float32)
    tw_im = (-np.sin(2.0 * np.pi * m / n_fft)).astype(np.float32)
    win = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)).astype(np.float32)
    return tw_re, tw_im, win


def frame_indices(n, n_fft, hop):
    """[N // hop, n_fft]: the sample every element of every frame reads, with the kernel's reflection at the utterance's own ends"""
    p = pad_of(n_fft, hop)
    s = np.arange(n // hop)[:, None] * hop + np.arange(n_fft)[None, :] - p
    s = np.where(s < 0, -s, s)
    return np.where(s >= n, 2 * (n - 1) - s, s)


def spectrogram32(y, n_fft, hop, bins=None):
    """fp32 [bins, N // hop]: the kernel's own radix-2 decimation-in-time FFT, every operation rounded to fp32"""
    y = np.asarray(y, np.float32)
    log2n = n_fft.bit_length() - 1
    tw_re, tw_im, win = tables32(n_fft)
    idx = frame_indices(len(y), n_fft, hop)
    assert idx.min() >= 0 and idx.max() < len(y), "the reflection leaves the utterance: N < max(hop, pad + 1)"
    v = y[idx] * win[None, :]
    rev = np.array([int(format(m, "0%db" % log2n)[::-1], 2) for m in range(n_fft)])
    re = np.zeros_like(v)
    re[:, rev] = v
    im = np.zeros_like(v)
    L = v.shape[0]
    for s in range(1, log2n + 1):
        half = 1 << (s - 1)
        wr, wi = tw_re[np.arange(half) << (log2n - s)], tw_im[np.arange(half) << (log2n - s)]
        re4, im4 = re.reshape(L, -1, 2, half), im.reshape(L, -1, 2, half)
        ar, ai, cr, ci = re4[:, :, 0], im4[:, :, 0], re4[:, :, 1], im4[:, :, 1]
        mr = cr * wr - ci * wi
        mi = cr * wi + ci * wr
        re = np.stack([ar + mr, ar - mr], axis=2).reshape(L, n_fft)
        im = np.stack([ai + mi, ai - mi], axis=2).reshape(L, n_fft)
        assert re.dtype == np.float32 and im.dtype == np.float32
    b = n_fft // 2 + 1 if bins is None else bins
    out = np.sqrt(re[:, :b] * re[:, :b] + im[:, :b] * im[:, :b] + np.float32(1e-6))
    assert out.dtype == np.float32
    return out.T
