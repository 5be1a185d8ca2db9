"""ITU-R BS.1770-4 integrated loudness and sample peak in numpy float64: a restatement of the definition in include/vits.h ("a stated level"), written
from that text and shared by the levelling tests. Nothing here calls the library."""
import numpy as np

LEVEL_NONE, LEVEL_MEASURE, LEVEL_GAIN, LEVEL_PEAK, LEVEL_LOUDNESS = 0, 1, 2, 3, 4

# the coefficient table of BS.1770 at 48 kHz: b0 b1 b2 a1 a2 of the shelf, then of the high-pass
BS1770_48K = np.array([[1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585],
                       [1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]])


def coefficients(fs):
    """[2, 5] float64: b0 b1 b2 a1 a2 of the two K-weighting biquads at rate fs"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = np.tan(np.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = np.tan(np.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    hp = [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return np.array([shelf, hp], np.float64)


def segment(fs):
    return (int(fs) + 5) // 10


def _biquad(c, x):
    """direct form I, zero state before sample 0"""
    b0, b1, b2, a1, a2 = (float(v) for v in c)
    y = np.zeros(x.size, np.float64)
    x1 = x2 = y1 = y2 = 0.0
    xs = x.tolist()
    for n, xn in enumerate(xs):
        yn = b0 * xn + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
        x2, x1 = x1, xn
        y2, y1 = y1, yn
        y[n] = yn
    return y


def k_weight(x, fs):
    c = coefficients(fs)
    return _biquad(c[1], _biquad(c[0], np.asarray(x, np.float64)))


def segment_means(x, fs, weighted=True):
    S = segment(fs)
    y = k_weight(x, fs) if weighted else np.asarray(x, np.float64)
    n_seg = y.size // S
    return (y[:n_seg * S].reshape(n_seg, S) ** 2).mean(axis=1) if n_seg else np.zeros(0)


def gated(z, absolute=True, relative=True, overlap=True):
    """(L, blocks) from the 100 ms segment means z; the switches drop a part of the definition (what the test signals are built to expose)"""
    if z.size < 4:
        return -np.inf, 0
    blk = np.array([z[j:j + 4].mean() for j in range(0, z.size - 3, 1 if overlap else 4)])
    with np.errstate(divide="ignore"):
        l = -0.691 + 10.0 * np.log10(blk)
    keep = l > -70.0 if absolute else np.ones(blk.size, bool)
    if not keep.any():
        return -np.inf, 0
    if relative:
        gamma = -0.691 + 10.0 * np.log10(blk[keep].mean()) - 10.0
        keep = keep & (l > gamma)
    return float(-0.691 + 10.0 * np.log10(blk[keep].mean())), int(keep.sum())


def loudness(x, fs):
    """(L in LUFS or -inf, sample peak, blocks that passed both gates) of one utterance x at rate fs"""
    x = np.asarray(x, np.float32)
    L, nb = gated(segment_means(x, fs))
    return L, (float(np.abs(x).max()) if x.size else 0.0), nb


def gain(kind, value_db, ceiling_db, L, P):
    """the linear gain of a kind from a measured L and P (float64)"""
    L, P = float(L), float(P)
    if kind == LEVEL_GAIN:
        return 10.0 ** (value_db / 20.0)
    if kind == LEVEL_PEAK:
        return 10.0 ** (value_db / 20.0) / P if P > 0 else 1.0
    if kind == LEVEL_LOUDNESS:
        if P <= 0 or not np.isfinite(L):
            return 1.0
        return min(10.0 ** ((value_db - L) / 20.0), 10.0 ** (ceiling_db / 20.0) / P)
    return 1.0


# ---- the test signals (each built so that one defect moves the result by far more than the tolerance) ----
def _t(fs, seconds):
    return np.arange(int(round(fs * seconds)), dtype=np.float64) / fs


def _noise(fs, seconds, seed):
    return 1e-5 * np.random.default_rng(seed).standard_normal(int(round(fs * seconds)))


def sig_levels(fs):
    """two levels 14 dB apart and a long quiet tail: either gate dropped moves L by more than 2.6 LU"""
    tone = 0.25 * np.sin(2 * np.pi * 500 * _t(fs, 1.0))
    return np.concatenate([tone, tone * 10.0 ** (-14 / 20.0), _noise(fs, 6.0, 1)]).astype(np.float32)


def sig_overlap(fs):
    """1 s / 1 s / 1 s at 0 dB / -25 dB / noise: blocks taken without overlap read 0.55 LU off"""
    tone = 0.25 * np.sin(2 * np.pi * 500 * _t(fs, 1.0))
    return np.concatenate([tone, tone * 10.0 ** (-25 / 20.0), _noise(fs, 1.0, 2)]).astype(np.float32)


def sig_weighting(fs):
    """a 60 Hz sine: an unweighted mean square reads +2.8 LU off"""
    return (0.5 * np.sin(2 * np.pi * 60 * _t(fs, 2.0))).astype(np.float32)


def sig_carry(fs, extra=0):
    """an offset and a small tone: the high-pass removes the offset only if its state crosses every boundary the kernels cut the utterance at"""
    t = np.arange(int(round(fs * 2.0)) + extra, dtype=np.float64) / fs
    return (0.5 + 0.01 * np.sin(2 * np.pi * 300 * t)).astype(np.float32)


def sig_silence(fs):
    """unmeasurable: every block lies below the absolute gate"""
    return _noise(fs, 2.0, 3).astype(np.float32)


def signals(fs):
    return {"levels": sig_levels(fs), "overlap": sig_overlap(fs), "weighting": sig_weighting(fs), "carry": sig_carry(fs), "carry_odd": sig_carry(fs, 37),
            "silence": sig_silence(fs)}


def ragged(rows, gap=5):
    """(x float32 [B, stride] with NaN behind every row, lens int64 [B])"""
    lens = np.array([r.size for r in rows], np.int64)
    x = np.full((len(rows), int(lens.max()) + gap), np.nan, np.float32)
    for b, r in enumerate(rows):
        x[b, :r.size] = r
    return x, lens
