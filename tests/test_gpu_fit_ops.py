"""fit_durations_kernel at operator level (vits_op_fit_durations; include/vits.h "a stated duration"): the kernel must equal the numpy restatement
(tests/fit_ref.py) applied to the kernel's OWN e_out, integer for integer and with the scale's bits equal. Nothing here has a tolerance.

Shapes: rows of 1, 2, 255, 256, 257 and 4096 tokens (a thread's first, second and seventeenth token; one block walks every member), batch 1 to 8 with ragged
lens, every utterance its own group, one group over the whole batch, groups that interleave utterances, unfitted groups among fitted ones, rows of equal logw
(remainders that cross the 256-token pieces of the scan and the utterances of a group), fixed tokens (0 among them), both clamps. logw is staged with NaN
behind every length and the fixed rows with 0x7F bytes, so a token read there would reach a sum.

Further: vits_op_durations at length_scale = s* and no override gives ceil(e_out * s*) for every token, which shows that the two kernels evaluate one expf;
and a group's result does not change with its batch position or its neighbours."""
import numpy as np
import pytest

import fit_ref as FR

pytestmark = pytest.mark.gpu

ROW_LENGTHS = (1, 2, 255, 256, 257, 4096)
GROUPINGS = ("own", "one", "interleaved")


def logw_rows(rng, B, T, equal):
    lw = rng.normal(0.5, 1.0, (B, 2, T)).astype(np.float32)
    if equal == "all":
        lw[:, 1] = np.float32(0.9)
    elif equal == "head":
        lw[:, 1, : max(1, T // 2)] = np.float32(0.9)
    lw[:, 0] = np.nan  # (the other row of the tensor is never read)
    return lw


def lens_for(rng, B, T):
    lens = rng.integers(1, T + 1, B).astype(np.int32)
    lens[0] = T
    if B > 1:
        lens[-1] = max(1, T - 1)
    return lens


def groups_for(kind, B):
    if kind == "own":
        return None
    if kind == "one":
        return np.zeros(B, np.int32)
    return (np.arange(B) % 3 + (B > 3)).astype(np.int32) % B  # members of a group lie apart; group 0 may have none


def natural(e, lens, groups, fixed):
    B = e.shape[0]
    g = np.arange(B) if groups is None else groups
    n = np.zeros(B, np.int64)
    for b in range(B):
        f = np.full(lens[b], -1) if fixed is None else fixed[b, :lens[b]]
        n[g[b]] += FR.frames(e[b, :lens[b]], 1.0, f).sum()
    return n


def check(pkg, lw, lens, groups, targets, fixed=None, lo=0.1, hi=10.0):
    e, dur, rows = pkg.op_fit_durations(lw, 1, targets, lens, fixed, groups, lo, hi)
    B, T = dur.shape
    for b in range(B):
        assert np.isfinite(e[b, :lens[b]]).all() and (e[b, lens[b]:] == 0).all()  # (the output fill behind every length)
        assert np.abs(e[b, :lens[b]] / np.exp(lw[b, 1, :lens[b]].astype(np.float64)) - 1).max() < 4e-7  # (the device library's expf: within 2 ulp, 2.4e-7)
    w_dur, w_rows = FR.fit(e, targets, lens, fixed, groups, lo, hi)
    assert np.array_equal(dur, w_dur)
    assert np.array_equal(rows.view(np.uint64), w_rows.view(np.uint64)), (rows, w_rows)
    return e, dur, rows


@pytest.mark.parametrize("grouping", GROUPINGS)
@pytest.mark.parametrize("T", ROW_LENGTHS)
def test_the_kernel_is_the_restatement_on_its_own_exp(pkg, T, grouping):
    rng = np.random.default_rng(T * 7 + len(grouping))
    seen = {-1: 0, 0: 0, 1: 0, 2: 0}
    remainders = 0
    for B in (1, 2, 3, 5, 8) if T < 4096 else (1, 3):
        for equal in (None, "all", "head"):
            lw = logw_rows(rng, B, T, equal)
            lens = lens_for(rng, B, T)
            groups = groups_for(grouping, B)
            fixed = None
            if equal == "head":
                fixed = np.where(rng.random((B, T)) < 0.1, rng.integers(0, 6, (B, T)), -1).astype(np.int32)
            e = np.exp(lw[:, 1])
            targets = np.maximum(1, (natural(e, lens, groups, fixed) * rng.uniform(0.4, 2.5, B)).astype(np.int64))
            if B >= 3:
                targets[1] = 0  # an unfitted group among fitted ones: its rows pass through
            if B >= 5:
                targets[2] = 1  # does not fit at the fastest rate
            lo, hi = (0.1, 10.0) if equal != "all" else (0.5, 2.0)
            _, dur, rows = check(pkg, lw, lens, groups, targets, fixed, lo, hi)
            for st in rows[:, 4]:
                seen[int(st)] += 1
            remainders += int((rows[:, 3] > 0).sum())
            members = np.arange(B) if groups is None else groups
            for b in range(B):
                assert (dur[b, lens[b]:] == -1).all()
                if targets[members[b]] == 0:
                    assert np.array_equal(dur[b, :lens[b]], np.full(lens[b], -1) if fixed is None else fixed[b, :lens[b]])
            fitted = rows[rows[:, 4] == 0]
            assert np.array_equal(fitted[:, 0], fitted[:, 1])  # status 0: the group lasts its target
    print(T, grouping, "status", seen, "remainders", remainders)
    # (a remainder needs several tokens that step at the same float: the rows of equal logw have them from 255 tokens on, whatever the target)
    assert seen[0] >= 3 and (T < 255 or remainders >= 1)


def test_both_clamps_and_equal_limits(pkg):
    rng = np.random.default_rng(5)
    lw = logw_rows(rng, 4, 300, None)
    lens = np.int32([300, 299, 17, 256])
    _, dur, rows = check(pkg, lw, lens, None, [1, 1 << 22, 1, 1 << 22], lo=0.5, hi=1.5)
    assert rows[:, 4].tolist() == [1, 2, 1, 2]
    e = check(pkg, lw, lens, np.int32([0, 0, 1, 1]), [700, 0, 400, 0], lo=1.25, hi=1.25)[0]
    s = np.float32(1.0 / float(np.float32(1.25)))
    d = check(pkg, lw, lens, None, [1, 1, 1, 1], lo=0.5, hi=1.25)[1]
    for b in range(4):
        assert np.array_equal(d[b, :lens[b]], np.ceil(e[b, :lens[b]] * s).astype(np.int32))  # clamped: the speaking_rates call's durations


def test_the_durations_kernel_evaluates_the_same_exp(pkg):
    rng = np.random.default_rng(6)
    B, T = 4, 257
    lw = logw_rows(rng, B, T, None)
    lens = np.int32([257, 256, 1, 100])
    e = np.exp(lw[:, 1])
    targets = (natural(e, lens, None, None) * np.array([0.7, 1.0, 3.0, 1.4])).astype(np.int64)
    e_out, dur, rows = check(pkg, lw, lens, None, targets)
    scales = rows[:, 2].astype(np.float32)
    logw = np.where(np.isnan(lw), 0, lw)
    d2 = pkg.op_durations(logw, 1, lens, length_scales=scales)[0]
    for b in range(B):
        want = np.ceil(e_out[b, :lens[b]] * scales[b])
        assert np.array_equal(d2[b, :lens[b]], want), b
        # ... and the fit's durations are those plus the remainder's shares
        extra = dur[b, :lens[b]] - want
        assert (extra >= 0).all() and extra.sum() == rows[b, 3]
    # the override rows the fit writes, given to the durations kernel, sum to the targets
    frames = pkg.op_durations(logw, 1, lens, overrides=dur)[2]
    assert np.array_equal(frames, rows[:, 1].astype(np.int32)) and np.array_equal(frames[rows[:, 4] == 0], targets[rows[:, 4] == 0])


def test_a_group_does_not_depend_on_its_position_or_its_neighbours(pkg):
    rng = np.random.default_rng(7)
    T = 300
    lw = logw_rows(rng, 6, T, "head")
    lens = np.int32([300, 41, 257, 256, 1, 299])
    groups = np.int32([0, 1, 0, 2, 1, 2])
    e = np.exp(lw[:, 1])
    targets = np.zeros(6, np.int64)
    targets[:3] = (natural(e, lens, groups, None)[:3] * np.array([1.3, 0.8, 1.1])).astype(np.int64)
    _, dur, rows = check(pkg, lw, lens, groups, targets)
    # the same groups at other batch positions, under other group numbers, beside other neighbours (the remainder follows batch order, so every group's
    # members keep their order: position i of the second call holds utterance perm2[i] of the first)
    perm2 = np.array([3, 1, 0, 5, 2, 4])
    renumber = np.int32([4, 2, 5])
    g2 = renumber[groups[perm2]]
    t2 = np.zeros(6, np.int64)
    t2[renumber] = targets[:3]
    _, dur2, rows2 = check(pkg, lw[perm2], lens[perm2], g2, t2)
    assert np.array_equal(dur2, dur[perm2])
    assert np.array_equal(rows2[renumber], rows[:3])
    # each group alone
    for g in range(3):
        m = [b for b in range(6) if groups[b] == g]
        _, d1, r1 = check(pkg, lw[m], lens[m], np.zeros(len(m), np.int32), [targets[g]] + [0] * (len(m) - 1))
        assert np.array_equal(d1, dur[m]) and np.array_equal(r1[0], rows[g])


def test_refusals_come_before_the_device(pkg):
    lw = np.zeros((2, 2, 4), np.float32)
    for kw, msg in ((dict(targets=[0, 1 << 23]), r"target_frames\[1\]"), (dict(targets=[1, 1], groups=[0, 2]), r"groups\[1\] = 2"),
                    (dict(targets=[1, 1], lens=[5, 1]), r"lens\[0\] = 5"), (dict(targets=[1, 1], min_rate=3.0, max_rate=2.0), r"min_rate <= max_rate")):
        with pytest.raises(pkg.VitsError, match=msg):
            pkg.op_fit_durations(lw, 1, **kw)
    with pytest.raises(pkg.VitsError, match="0 <= row < rows"):
        pkg.op_fit_durations(lw, 2, [1, 1])
