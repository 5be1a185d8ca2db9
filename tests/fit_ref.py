"""A stated duration (include/vits.h "a stated duration") restated in numpy: IEEE fp32 multiply, ceil and integer arithmetic, so that the product's host
definition (vits_fit_host), its kernel (fit.hip) and this file agree on every integer. Nothing here calls the product.

fit(e, fixed, lens, groups, targets, min_rate, max_rate) -> (dur int32 [B, T], rows float64 [B, 5] = (F, sum d, s*, R, status) by group), as vits_fit_host
hands them out: d_t of every token of a fitted utterance, fixed_t (or -1) of every other token, -1 behind every length; status -1 for a group that is not
fitted or that no utterance names. `defect` seeds one of two mistakes, for the tests that show the comparison can fail."""
import numpy as np

CAP = np.float32(16777216.0)


def bits(x):
    return int(np.float32(x).view(np.uint32))


def from_bits(b):
    return np.uint32(b).view(np.float32)


def limits(min_rate, max_rate):
    """(s_lo, s_hi): the engine's own expression for a rate's length scale"""
    return np.float32(1.0 / float(np.float32(max_rate))), np.float32(1.0 / float(np.float32(min_rate)))


def frames(e, s, fixed):
    """c_t(s) of a row of tokens, int64"""
    with np.errstate(over="ignore", invalid="ignore"):
        x = np.ceil(np.asarray(e, np.float32) * np.float32(s))
    c = np.where(x < CAP, x, CAP).astype(np.int64)
    return np.where(fixed >= 0, fixed, c)


def fit_group(e, fixed, F, s_lo, s_hi, defect=None):
    """one group's tokens in (utterance, token) order -> (d int64, bits of s*, R, status, bisection steps)"""
    lo, hi = bits(s_lo), bits(s_hi)
    n = lambda b: int(frames(e, from_bits(b), fixed).sum())
    steps = 0
    if n(lo) > F:
        return frames(e, from_bits(lo), fixed), lo, 0, 1, steps
    if n(hi) <= F:
        d = frames(e, from_bits(hi), fixed)
        return d, hi, 0, 0 if int(d.sum()) == F else 2, steps
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        steps += 1
        fits = n(mid) < F if defect == "strict" else n(mid) <= F
        if fits:
            lo = mid
        else:
            hi = mid
    d = frames(e, from_bits(lo), fixed)
    gain = frames(e, from_bits(lo + 1), fixed) - d
    R = left = F - int(d.sum())
    order = range(len(d) - 1, -1, -1) if defect == "wrong_end" else range(len(d))
    for t in order:
        if left <= 0:
            break
        take = min(int(gain[t]), left)
        d[t] += take
        left -= take
    return d, lo, R, 0, steps


def fit(e, targets, lens=None, fixed=None, groups=None, min_rate=0.1, max_rate=10.0, defect=None, steps_out=None):
    e = np.asarray(e, np.float32)
    B, T = e.shape
    lens = np.full(B, T, np.int64) if lens is None else np.asarray(lens, np.int64)
    fixed = np.full((B, T), -1, np.int64) if fixed is None else np.asarray(fixed, np.int64)
    groups = np.arange(B) if groups is None else np.asarray(groups, np.int64)
    targets = np.asarray(targets, np.int64)
    s_lo, s_hi = limits(min_rate, max_rate)
    dur = np.full((B, T), -1, np.int32)
    for b in range(B):
        dur[b, :lens[b]] = fixed[b, :lens[b]]
    rows = np.zeros((B, 5), np.float64)
    for g in range(B):
        F = int(targets[g])
        members = [b for b in range(B) if groups[b] == g]
        rows[g] = (F, 0, 0, 0, -1)
        if F == 0 or not members:
            continue
        ge = np.concatenate([e[b, :lens[b]] for b in members])
        gf = np.concatenate([fixed[b, :lens[b]] for b in members])
        d, sb, R, status, steps = fit_group(ge, gf, F, s_lo, s_hi, defect)
        if steps_out is not None:
            steps_out.append(steps)
        at = 0
        for b in members:
            dur[b, :lens[b]] = d[at:at + lens[b]]
            at += lens[b]
        rows[g] = (F, int(d.sum()), float(from_bits(sb)), R, status)
    return dur, rows
