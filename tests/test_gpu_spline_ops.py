"""spline_kernel and durations_kernel at operator level (vits_op_spline, vits_op_durations) on inputs no whole model produces: other bin counts than 10, every
length at which the 512-thread block changes its rounds, latents outside the interval wherever the reference's masked get / set pair shifts tokens, and
log-durations whose integer results are known exactly.

Spline. SPLINE_CASES = (bins, parameter scale): 1, 2, 10, 16 bins, each with unit-scale parameters and with parameters x 8 (sharp bins). Every case runs at
T in SPLINE_T (one token per thread; the second and third round of a 512-thread block; the rounding of tpad to 64; 4096 tokens = the largest LDS request) as the
ragged batch lens = [T, T - 1, 0, T // 2 + 1], on latent row 0 and on row 1, in both modes. Asserted:
  * values: against dp_ref.spline in float64, pooled over the lengths of a case and mode: rms error <= 2 x and max error <= 4 x those of dp_ref.spline in
    float32 on the same data (the restatement's max is heavy-tailed; what a wrong knot, bin or derivative does is 1e-3 and more);
  * HF mode: a token outside [-tail, tail] keeps its bits; x = +-tail exactly is inside (it is part of every draw; in reference mode its classification moves
    every later token, which the permutation check sees);
  * reference mode, outside tokens nowhere / everywhere / first / last (the Q4 row) / in a run across a thread-chunk boundary at len > 512 (two and three
    tokens per thread): the k-th inside token holds the result of token k and the j-th outside token element j of the masked input — checked exactly: every
    output is nearest to the candidate value dp_ref.spline_sources names among all results and all masked inputs, and a forwarded input keeps its bits;
  * the other latent row, everything behind lens[b] and the lens = 0 row keep their bits; every row == its batch-1 call bit for bit;
  * 17 bins and t = 4097 are refused by name.

Durations. DUR_STRIDES x the combinations of DUR_COMBOS (scalar scale against the per-utterance array, overrides with -1 and >= 0 mixed and one all-zero row,
fixed > 0, two stage tables) on a ragged batch with a length of 1, logw = log((n + f) / scale) with f in [0.05, 0.95] (tests/test_dp_op_host.py checks the
distance from an integer on the float64 products): dur, cum, frames and every stage_lens entry equal dp_ref.durations exactly, 0 and INT_MAX behind lens[b].

Observed on an MI355X, on the commit that adds this file (the tests print every figure; 34000 tokens per case and mode, result RMS 2.8 to 2.9; the ranges
are over the modes and placements; one bin has no inner derivative and its one width is the interval, so both of its draws are the same spline):
  bins, scale | restatement rms | restatement max  | GPU rms        | GPU max          | GPU / restatement: rms, max
  1, both     | 2.0e-7          | 7.0e-7 .. 1.2e-6 | 2.0e-7         | 7.2e-7 .. 1.1e-6 | 1.01, 0.90 .. 1.02
  2, unit     | 3.5e-7          | 3.9e-6 .. 5.9e-6 | 3.3e-7         | 6.0e-6 .. 6.4e-6 | 0.96, 1.08 .. 1.53
  10, unit    | 5.7e-7 .. 6.1e-7 | 6.8e-6 .. 8.9e-6 | 5.3e-7 .. 5.5e-7 | 4.8e-6 .. 6.9e-6 | 0.91 .. 0.93, 0.54 .. 1.01
  16, unit    | 6.7e-7          | 7.4e-6 .. 1.1e-5 | 6.4e-7         | 6.2e-6 .. 7.5e-6 | 0.94 .. 0.95, 0.66 .. 0.84
  2, x 8      | 7.1e-7          | 2.0e-5 .. 2.2e-5 | 6.1e-7 .. 6.3e-7 | 1.7e-5 .. 2.8e-5 | 0.86 .. 0.89, 0.78 .. 1.46
  10, x 8     | 1.4e-6 .. 2.4e-6 | 8.7e-5 .. 3.8e-4 | 1.2e-6 .. 2.0e-6 | 1.0e-4 .. 2.3e-4 | 0.82 .. 0.85, 0.60 .. 1.16
  16, x 8     | 1.6e-6 .. 2.7e-6 | 1.1e-4 .. 3.9e-4 | 1.7e-6 .. 2.1e-6 | 1.6e-4 .. 2.6e-4 | 0.77 .. 1.04, 0.67 .. 1.46
Every permutation, bit-identity and exact-durations assertion holds. The whole file runs in 3 s."""
import numpy as np
import pytest

import dp_ref as D

pytestmark = pytest.mark.gpu
MODE_REFERENCE, MODE_HF = 0, 1
SPLINE_CASES = [(bins, scale) for scale in (1.0, 8.0) for bins in (1, 2, 10, 16)]
SPLINE_T = [1, 2, 63, 64, 65, 511, 512, 513, 1025, 4096]
RMS_FACTOR, MAX_FACTOR = 2.0, 4.0
INV_SQRT = float(1.0 / np.sqrt(192.0))


def spline_id(c):
    return "bins%d-x%g" % c


def spline_lens(T):
    return [T, max(1, T - 1), 0, T // 2 + 1]


def chunk(n):
    """tokens per thread of the kernel's second phase: the utterance spread over its 512 (or fewer) threads"""
    tpad = (n + 63) // 64 * 64
    return -(-n // min(tpad, 512))


def outside_of(place, n):
    """token indices outside the interval, by placement"""
    if place == "none":
        return []
    if place == "all":
        return list(range(n))
    if place == "first":
        return [0]
    if place == "last":
        return [n - 1]
    per = chunk(n)  # "run": across the boundary between thread 7's and thread 8's tokens, and two singles further on
    run = [t for t in (8 * per - 2, 8 * per - 1, 8 * per, 8 * per + 1) if 0 <= t < n]
    return sorted(set(run + [t for t in (n // 2, n - 2) if 0 <= t < n]))


def spline_batch(bins, scale, T, place, zc, seed):
    """u [B, 3 bins - 1, T], z [B, 2, T] for the ragged batch of T: row zc per utterance from dp_ref.make_spline_case with x = +-tail exactly at two inside tokens;
    the other row and everything behind lens[b] are recognisable values that must come back bit for bit"""
    lens = spline_lens(T)
    B = len(lens)
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((B, 3 * bins - 1, T)).astype(np.float32)
    z = rng.standard_normal((B, 2, T)).astype(np.float32) * 100
    tail = 5.0
    for b, n in enumerate(lens):
        if n == 0:
            continue
        ub, zr, tail = D.make_spline_case(n, bins, seed * 8 + b, scale, outside_of(place, n))
        if place != "all" and n >= 8:
            for t, v in ((2, tail), (3, -tail)):
                if t not in outside_of(place, n):
                    zr[t] = np.float32(v)
        u[b, :, :n] = ub
        z[b, zc, :n] = zr
    return u, z, lens, tail


def run_spline(pkg, u, z, zc, bins, tail, mode, lens, T):
    return pkg.op_spline(u, z, zc, bins, tail, INV_SQRT, mode, lens=lens, t=T)


def check_untouched(got, z, zc, lens):
    gb, zb = got.view(np.uint32), z.view(np.uint32)
    assert np.array_equal(gb[:, 1 - zc], zb[:, 1 - zc]), "the other latent row changed"
    for b, n in enumerate(lens):
        assert np.array_equal(gb[b, zc, n:], zb[b, zc, n:]), (b, "a token behind lens[b] changed")


class Errors:
    def __init__(self):
        self.g2 = self.c2 = self.r2 = 0.0
        self.gmax = self.cmax = 0.0
        self.n = 0

    def add(self, got, chain, ref):
        if ref.size == 0:
            return
        eg, ec = np.abs(got.astype(np.float64) - ref), np.abs(chain.astype(np.float64) - ref)
        self.g2 += float((eg ** 2).sum())
        self.c2 += float((ec ** 2).sum())
        self.r2 += float((ref ** 2).sum())
        self.gmax, self.cmax = max(self.gmax, float(eg.max())), max(self.cmax, float(ec.max()))
        self.n += ref.size

    def hold(self, label):
        rms = np.sqrt(self.r2 / self.n)
        g, c = np.sqrt(self.g2 / self.n), np.sqrt(self.c2 / self.n)
        print("%s: %d tokens, RMS of the result %.2f: gpu rms %.2e max %.2e; fp32 restatement rms %.2e max %.2e; ratios %.2f and %.2f"
              % (label, self.n, rms, g, self.gmax, c, self.cmax, g / c, self.gmax / self.cmax))
        assert g <= RMS_FACTOR * c, (label, "rms", g, c)
        assert self.gmax <= MAX_FACTOR * self.cmax, (label, "max", self.gmax, self.cmax)


@pytest.mark.parametrize("c", SPLINE_CASES, ids=spline_id)
def test_hf_mode_values_and_identity_outside(pkg, c):
    bins, scale = c
    err = Errors()
    for T in SPLINE_T:
        for zc in (0, 1):
            u, z, lens, tail = spline_batch(bins, scale, T, "run", zc, 1000 * bins + T + zc)
            got = run_spline(pkg, u, z, zc, bins, tail, MODE_HF, lens, T)
            check_untouched(got, z, zc, lens)
            for b, n in enumerate(lens):
                if n == 0:
                    continue
                x = z[b, zc, :n]
                inside = np.abs(x) <= np.float32(tail)
                assert np.array_equal(got[b, zc, :n][~inside].view(np.uint32), x[~inside].view(np.uint32)), "an outside token lost its bits"
                ref = D.spline(x, u[b, :, :n], bins, tail, INV_SQRT, MODE_HF, np.float64)
                chain = D.spline(x, u[b, :, :n], bins, tail, INV_SQRT, MODE_HF, np.float32)
                assert np.isfinite(got[b, zc, :n]).all()
                err.add(got[b, zc, :n][inside], chain[inside], ref[inside])
                if n >= 8:
                    assert x[2] == np.float32(tail) and x[3] == -np.float32(tail) and inside[2] and inside[3]  # x = +-tail: held to the reference as inside tokens
    err.hold("HF %s" % spline_id(c))


@pytest.mark.parametrize("place", ["none", "all", "first", "last", "run"])
@pytest.mark.parametrize("c", SPLINE_CASES, ids=spline_id)
def test_reference_mode_values_and_permutation(pkg, c, place):
    bins, scale = c
    err = Errors()
    for T in SPLINE_T:
        for zc in (0, 1):
            u, z, lens, tail = spline_batch(bins, scale, T, place, zc, 2000 * bins + T + zc)
            got = run_spline(pkg, u, z, zc, bins, tail, MODE_REFERENCE, lens, T)
            check_untouched(got, z, zc, lens)
            for b, n in enumerate(lens):
                if n == 0:
                    continue
                x = z[b, zc, :n]
                g = got[b, zc, :n]
                assert np.isfinite(g).all()
                ref = D.spline(x, u[b, :, :n], bins, tail, INV_SQRT, MODE_REFERENCE, np.float64)
                chain = D.spline(x, u[b, :, :n], bins, tail, INV_SQRT, MODE_REFERENCE, np.float32)
                inside, src = D.spline_sources(x, tail)
                check_sources(g, x, u[b, :, :n], bins, tail, (T, b))
                fwd = ~inside
                assert np.array_equal(g[fwd].view(np.uint32), np.where(inside, x, np.float32(0))[src[fwd]].view(np.uint32)), "a forwarded input lost its bits"
                err.add(g[inside], chain[inside], ref[inside])
    if place != "all":
        err.hold("reference %s, outside: %s" % (spline_id(c), place))


def check_sources(g, x, u, bins, tail, label):
    """The permutation of reference mode, token by token: what a token holds is nearer to the candidate the reference's pair gives it (dp_ref.spline_sources)
    than to the candidates a wrong pairing would give it — its own spline result (no shift) and the sources one before and one behind — wherever those differ
    from the right one by more than 1e-3 (two tokens' values are O(1) apart; the kernel's error is 1e-5 at the most)."""
    n = x.size
    inside, src = D.spline_sources(x, tail)
    res = _own_results(x, u, bins, tail, inside)
    vals = np.where(inside, x, np.float32(0)).astype(np.float64)
    pick = lambda k: np.where(inside, res[np.clip(k, 0, n - 1)], vals[np.clip(k, 0, n - 1)])
    want = pick(src)
    d = np.abs(g - want)
    told_apart = 0
    for alt in (res, pick(src - 1), pick(src + 1)):
        differs = np.abs(alt - want) > 1e-3
        told_apart += int(differs.sum())
        bad = np.flatnonzero(differs & (np.abs(g - alt) <= d))
        assert bad.size == 0, (label, "token %d holds %r; the reference's pair gives it %r" % (bad[0] if bad.size else -1, g[bad[:1]], want[bad[:1]]))
    assert (d <= 1e-3).all(), (label, "a token is far from its source", float(d.max()))
    return told_apart


def _own_results(x, u, bins, tail, inside):
    """float64 spline result of every token as reference mode computes it before the set pair (an outside token: input 0, zeroed parameters)"""
    T = x.size
    q4 = np.arange(T) == T - 1
    return D._spline_rows(np.where(inside, x, np.float32(0)).astype(np.float64), u, bins, tail, INV_SQRT, MODE_REFERENCE, q4, ~inside, np.float64)


@pytest.mark.parametrize("mode", [MODE_HF, MODE_REFERENCE], ids=["hf", "reference"])
def test_every_row_is_its_batch_1_call(pkg, mode):
    for bins, T in ((10, 65), (16, 513), (2, 1025)):
        u, z, lens, tail = spline_batch(bins, 1.0, T, "run", 1, 77 + T)
        got = run_spline(pkg, u, z, 1, bins, tail, mode, lens, T)
        for b, n in enumerate(lens):
            one = run_spline(pkg, u[b:b + 1], z[b:b + 1], 1, bins, tail, mode, [n], T)
            assert np.array_equal(one.view(np.uint32), got[b:b + 1].view(np.uint32)), (bins, T, b)
        # a stride beyond t: the same bits
        wide_u, wide_z = np.zeros((len(lens), 3 * bins - 1, T + 37), np.float32), np.full((len(lens), 2, T + 37), 7.0, np.float32)
        wide_u[:, :, :T], wide_z[:, :, :T] = u, z
        wide = run_spline(pkg, wide_u, wide_z, 1, bins, tail, mode, lens, T)
        assert np.array_equal(wide[:, :, :T].view(np.uint32), got.view(np.uint32)) and (wide[:, :, T:] == 7.0).all()


def test_spline_refusals(pkg):
    check_spline_refusals(pkg)


def check_spline_refusals(pkg):
    for bins, T, cause in ((17, 8, "bins = 17"), (10, 4097, "t = 4097")):
        with pytest.raises(pkg.VitsError) as e:
            pkg.op_spline(np.zeros((1, 3 * bins - 1, T), np.float32), np.zeros((1, 2, T), np.float32), 0, bins, 5.0, INV_SQRT, MODE_HF)
        assert cause in str(e.value) and "spline_kernel" in str(e.value), str(e.value)


# ---- durations -------------------------------------------------------------------------------------------------------------------------------------
DUR_STRIDES = [1, 255, 256, 257, 1000]
STAGES = (([1, 8, 64, 256], [0, 8, 72, 288]), ([1, 8, 64, 128, 256], [0, 0, 0, 0, 0]))  # reference-mode and HF-mode tables of an (8, 8, 2[, 2]) vocoder
DUR_COMBOS = [dict(), dict(per_utt=True), dict(ovr=True), dict(per_utt=True, ovr=True, stages=1), dict(fixed=3), dict(fixed=2, ovr=True, per_utt=True, stages=1)]


def dur_id(k):
    return "-".join(sorted("%s%s" % (n, "" if v is True else v) for n, v in k.items())) or "scalar"


def dur_lens(ts):
    return [ts, max(1, ts - 1), 1, max(1, ts // 2), max(1, ts - 3)]


def dur_case(ts, combo):
    """inputs of one durations call: (logw [B, 2, ts], row, lens, kwargs of op_durations / dp_ref.durations)"""
    lens = dur_lens(ts)
    B = len(lens)
    rng = np.random.default_rng(ts * 31 + len(dur_id(combo)))
    scalar = 1.25
    scales = np.array([0.8, 1.0, 1.25, 2.0, 0.5], np.float32)[:B] if combo.get("per_utt") else None
    logw = D.make_logw(lens, ts, scales if scales is not None else [scalar] * B, ts + 5)
    kw = dict(length_scale=scalar, length_scales=scales, fixed=combo.get("fixed", 0))
    kw["stage_mul"], kw["stage_add"] = STAGES[combo.get("stages", 0)]
    if combo.get("ovr"):
        o = np.where(rng.uniform(size=(B, ts)) < 0.5, -1, rng.integers(0, 9, (B, ts))).astype(np.int32)
        o[3] = 0  # an all-zero override row: frames = max(1, 0)
        kw["overrides"] = o
    return logw, 1, lens, kw


@pytest.mark.parametrize("combo", DUR_COMBOS, ids=dur_id)
@pytest.mark.parametrize("ts", DUR_STRIDES)
def test_durations_are_exact(pkg, ts, combo):
    logw, row, lens, kw = dur_case(ts, combo)
    dur, cum, frames, sl = pkg.op_durations(logw, row, lens, **kw)
    w_dur, w_cum, w_frames, w_sl, _ = D.durations(logw[:, row], lens, **kw)
    assert np.array_equal(dur.astype(np.int64), w_dur) and (dur == np.floor(dur)).all()
    assert np.array_equal(cum.astype(np.int64), w_cum)
    assert np.array_equal(frames.astype(np.int64), w_frames) and np.array_equal(sl.astype(np.int64), w_sl)
    for b, n in enumerate(lens):
        assert (dur[b, n:] == 0).all() and (cum[b, n:] == D.INT_MAX).all()
    if combo.get("ovr") and not combo.get("fixed"):
        assert frames[3] == 1 and (dur[3, :lens[3]] == 0).all()
    if combo.get("fixed"):
        assert all(frames[b] == combo["fixed"] * n for b, n in enumerate(lens))
