"""The numpy restatement of the time-stretch stage (include/vits.h "a stated tempo"): waveform-similarity overlap-add with an integer search and a float32
overlap-add, written from the header's definition alone. The search works on int64 throughout; every product and the one add of a sample are float32
operations of numpy (two rounded products, one rounded add: numpy never contracts them)."""
import numpy as np

ONE = 1 << 24


def plan(rate, q, n):
    """(H, D, Q, F, N') of a row of n samples at `rate` and tempo q"""
    H, D = 4 * (rate // 400), 4 * (rate // 500)
    Q = int(float(np.float32(q)) * ONE)
    n_out = -((-n * ONE) // Q)
    return H, D, Q, -(-n_out // H), n_out


def quantise(x):
    """the search signal: 0 for a NaN, else the sample at 16 bits, rounded to nearest even and clamped"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.clip(np.rint(x * np.float32(32768.0)), -32768.0, 32767.0)
    return np.where(np.isnan(x), 0.0, r).astype(np.int64)


def order(D):
    """the candidate order 0, -1, +1, -2, +2, ..., -D, +D"""
    d = np.zeros(2 * D + 1, np.int64)
    d[1::2] = -np.arange(1, D + 1)
    d[2::2] = np.arange(1, D + 1)
    return d


def tempo(x, rate, q, search=True):
    """(y float32 [N'], offsets int64 [F]); search=False: every offset 0 (what a broken search would deliver)"""
    x = np.ascontiguousarray(x, np.float32).ravel()
    n = x.size
    H, D, Q, F, n_out = plan(rate, q, n)
    if Q == ONE:
        return x.copy(), np.zeros(F, np.int64)
    # the row and its search signal, zero outside [0, N): pad in front for a_1 - D and a template at s_-1 + H, behind for a_F + D + H
    front, back = D + H, 3 * H + 2 * D + 2
    xp = np.zeros(front + n + back, np.float32)
    xp[front:front + n] = x
    xq = np.zeros(front + n + back, np.int64)
    xq[front:front + n] = quantise(x)
    cand = order(D)
    w = (np.arange(H, dtype=np.float32) * np.float32(2) + np.float32(1)) / np.float32(2 * H)
    v = w[::-1]
    s = np.zeros(F + 1, np.int64)
    off = np.zeros(F, np.int64)
    for k in range(1, F + 1):
        a, c = (k * H * Q) >> 24, int(s[k - 1]) + H
        if search:
            tpl = xq[front + c:front + c + H]
            reg = xq[front + a - D:front + a + D + H]
            sad = np.abs(np.lib.stride_tricks.sliding_window_view(reg, H) - tpl).sum(axis=1)  # [2 D + 1], index d + D
            off[k - 1] = cand[int(np.argmin(sad[cand + D]))]  # (argmin: the first minimum in the candidate order)
        s[k] = a + off[k - 1]
    y = np.zeros(F * H, np.float32)
    i = np.arange(H)
    for k in range(F):
        s0 = -H if k == 0 else int(s[k - 1])
        with np.errstate(invalid="ignore"):  # (a row may hold NaN and Inf: they go through the sums as IEEE says)
            y[k * H:(k + 1) * H] = v * xp[front + s0 + H + i] + w * xp[front + int(s[k]) + i]
    return y[:n_out], off


# ---- what the host test and the operator test share: the tempos, the row lengths and the signals ---------------------------------------------------------
TEMPOS = (0.5, float(np.float32(2.0 ** (-2 / 12))), 1.0 - 2.0 ** -24, 1.0, 1.0 + 2.0 ** -23, float(np.float32(2.0 ** (2 / 12))), 1.5, 2.0)
RATES = (16000, 22050)


def lengths(rate):
    """1, 2, around the hop, around two hops, around a whole candidate region, and 1000"""
    H, D = plan(rate, 1.0, 0)[:2]
    return [1, 2, H - 1, H, H + 1, 2 * H - 1, 2 * H + 1, 2 * D + H - 1, 2 * D + H + 1, 1000]


def signal(kind, n, seed=0):
    """one row of n samples: 'noise' (white), 'silence', 'ties' (period 40, multiples of 2^-15: candidates a period apart have EQUAL sums, the order decides),
    'clamp' (amplitudes of +-1.5: the search signal saturates), 'nonfinite' (white noise holding NaN and +Inf)"""
    rng = np.random.default_rng([seed, n])
    if kind == "noise":
        return (0.3 * rng.standard_normal(n)).astype(np.float32)
    if kind == "silence":
        return np.zeros(n, np.float32)
    if kind == "ties":
        period = rng.integers(-8000, 8000, 40).astype(np.float32) / np.float32(32768.0)
        return np.tile(period, n // 40 + 1)[:n].copy()
    if kind == "clamp":
        return (1.5 * np.sign(rng.standard_normal(n)) * (0.5 + 0.5 * rng.random(n))).astype(np.float32)
    if kind == "nonfinite":
        x = (0.3 * rng.standard_normal(n)).astype(np.float32)
        x[::37] = np.nan
        x[5::53] = np.inf
        return x
    raise ValueError(kind)


KINDS = ("noise", "silence", "ties", "clamp", "nonfinite")


def harmonic_tone(f0, rate=16000, n=16000):
    """five harmonics of f0 with falling amplitudes, as float32"""
    t = np.arange(n) / rate
    return (0.15 * sum(np.sin(2 * np.pi * f0 * h * t + 0.7 * h) / h for h in range(1, 6))).astype(np.float32)


def off_harmonic_db(y, f0, rate=16000):
    """(energy outside +-8 Hz of the five harmonics in dB of the total, frequency of the largest peak in Hz): Hann window, 2^18-point FFT, without the first
    and the last 400 samples"""
    y = np.asarray(y, np.float64)[400:-400]
    nfft = 1 << 18
    m = np.abs(np.fft.rfft(y * np.hanning(y.size), nfft)) ** 2
    hz = np.arange(m.size) * rate / nfft
    near = np.zeros(m.size, bool)
    for h in range(1, 6):
        near |= np.abs(hz - h * f0) <= 8.0
    k = int(m.argmax())
    a, b, c = np.log(m[k - 1:k + 2])
    peak = (k + 0.5 * (a - c) / (a - 2 * b + c)) * rate / nfft
    return 10 * np.log10(m[~near].sum() / m.sum()), peak
