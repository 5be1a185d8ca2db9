"""Joined tracks, host side (include/vits.h "joined tracks"): vits_join_plan and vits_join_host against the numpy restatement
(tests/join_ref.py), exactly, on hand cases and on seeded random ones; the property the kernel relies on (ends non-decreasing, at most two neighbours
per sample), checked on the restatement itself; every refusal of the plan by message; the sentence splitter. No device."""
import numpy as np
import pytest

import join_ref as JR

FS = JR.FS


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def rows_of(rng, lens):
    """fp32 rows with both signs, some exact zeros of both signs"""
    out = []
    for n in lens:
        x = rng.standard_normal(n).astype(np.float32)
        if n:
            x[rng.integers(0, n, max(n // 16, 1))] = np.float32(-0.0)
        out.append(x)
    return out


def check(pkg, rows, fs, track, gap_ms):
    lens = np.array([len(r) for r in rows], np.int64)
    want, o, T, bounds = JR.join(rows, fs, track, gap_ms)
    G, got_bounds, tile = pkg.join_plan(fs, lens, track, gap_ms)
    assert G == len(want) and np.array_equal(got_bounds, bounds) and tile == 1024
    stride = max(int(lens.max(initial=0)), 1)
    x = np.full((len(rows), stride), np.nan, np.float32)  # (NaN behind every n_b: nothing behind it is read)
    for b, r in enumerate(rows):
        x[b, : len(r)] = r
    y, tl, got_rows = pkg.join_host(x, fs, lens, track, gap_ms)
    assert np.array_equal(tl, T) and np.array_equal(got_rows[:, 0], o) and np.array_equal(got_rows[:, 1], lens)
    for g in range(G):
        assert same(y[g, : T[g]], want[g])
        tail = y[g, T[g]:bounds[g]]
        assert not tail.any() and not np.signbit(tail).any()  # [T_g, bound_g) is +0
    return want, o, T, bounds


def test_hand_cases(pkg):
    a, b, c = np.array([1, 2, 3, 4], np.float32), np.array([10, 20, 30], np.float32), np.array([100], np.float32)
    # no gap: the concatenation
    want, o, T, _ = check(pkg, [a, b, c], FS, None, None)
    assert o.tolist() == [0, 4, 7] and T.tolist() == [8] and want[0].tolist() == [1, 2, 3, 4, 10, 20, 30, 100]
    # + 2 samples (0.125 ms) in front of b: +0 between
    want, o, T, bounds = check(pkg, [a, b], FS, None, [0.0, 0.125])
    assert o.tolist() == [0, 6] and want[0].tolist() == [1, 2, 3, 4, 0, 0, 10, 20, 30] and bounds.tolist() == [9]
    # - 1 sample: the last of a and the first of b add; - 2000 ms: the half rule gives min(4 / 2, 3 / 2) = 1 all the same
    for ms in (-0.0625, -2000.0):
        want, o, T, bounds = check(pkg, [a, b], FS, None, [0.0, ms])
        assert o.tolist() == [0, 3] and T.tolist() == [6] and want[0].tolist() == [1, 2, 3, 14, 20, 30] and bounds.tolist() == [7]
    # n = 1 gives nothing away (v = 0), n = 3 gives one sample
    want, o, T, _ = check(pkg, [a, c, b], FS, None, -2000.0)
    assert o.tolist() == [0, 4, 5] and want[0].tolist() == [1, 2, 3, 4, 100, 10, 20, 30]
    # two tracks: the gap of the utterance that opens track 1 is validated and ignored
    want, o, T, bounds = check(pkg, [a, b, c], FS, [0, 0, 1], [0.0, -0.0625, 60000.0])
    assert o.tolist() == [0, 3, 0] and T.tolist() == [6, 1] and bounds.tolist() == [7, 1] and want[1].tolist() == [100]
    # an empty row in the middle gives and takes nothing; an empty track
    empty = np.zeros(0, np.float32)
    want, o, T, _ = check(pkg, [a, empty, b], FS, None, -2000.0)
    assert o.tolist() == [0, 4, 4] and want[0].tolist() == [1, 2, 3, 4, 10, 20, 30]
    want, o, T, bounds = check(pkg, [empty, empty, a], FS, [0, 0, 1], [0.0, -5.0, 0.0])
    assert T.tolist() == [0, 4] and bounds.tolist() == [0, 4] and want[0].size == 0
    # ... and one that holds nothing but a pause
    want, o, T, bounds = check(pkg, [empty, empty], FS, None, [0.0, 0.125])
    assert T.tolist() == [2] and bounds.tolist() == [2] and want[0].tolist() == [0, 0]
    # the rounding of samples(ms): half a sample rounds away from zero on both sides
    assert JR.gap_samples(0.03125, FS) == 1 and JR.gap_samples(-0.03125, FS) == -1 and JR.gap_samples(0.03, FS) == 0
    assert pkg.join_plan(FS, [5, 5], None, [0.0, 0.03125])[1].tolist() == [11] and pkg.join_plan(FS, [5, 5], None, [0.0, 0.03])[1].tolist() == [10]
    # a copy keeps every bit, the sign of a zero included; an add of a zero does not
    z, p = np.array([-0.0, -0.0], np.float32), np.array([0.0, 0.0], np.float32)
    want, *_ = check(pkg, [z, p], FS, None, [0.0, -0.0625])
    assert np.signbit(want[0]).tolist() == [True, False, False]


def random_case(rng):
    B = int(rng.integers(1, 13))
    # lengths 0 .. 5000, a few of them tiny so that the half rule binds often
    lens = [int(rng.integers(0, 5001)) if rng.random() < 0.7 else int(rng.integers(0, 8)) for _ in range(B)]
    G = int(rng.integers(1, min(B, 4) + 1))
    cuts = sorted(rng.choice(np.arange(1, B), G - 1, replace=False).tolist()) if G > 1 else []
    track = np.zeros(B, np.int32)
    for cut in cuts:
        track[cut:] += 1
    fs = int(rng.choice([8000, 16000, 22050, 48000]))
    gaps = np.where(rng.random(B) < 0.5, rng.uniform(-400.0, 0.0, B), rng.uniform(0.0, 30.0, B)).astype(np.float32)
    gaps[rng.random(B) < 0.15] = 0.0
    return lens, track, fs, gaps


def test_random_cases_equal_the_restatement_and_keep_the_kernels_property(pkg):
    rng = np.random.default_rng(20240611)
    overlaps = clamps = 0
    for case in range(300):
        lens, track, fs, gaps = random_case(rng)
        rows = rows_of(rng, lens)
        want, o, T, bounds = check(pkg, rows, fs, track if case % 3 else (None if track.max() == 0 else track), gaps)
        # the property join_apply_kernel relies on, on the restatement itself
        for g, (first, end) in enumerate(JR.tracks_of(len(lens), track)):
            starts = o[first:end]
            ends = starts + np.asarray(lens[first:end], np.int64)
            assert (np.diff(starts) >= 0).all() and (np.diff(ends) >= 0).all()
            assert T[g] == ends[-1] <= bounds[g]
            cover, lowest, highest = JR.census(lens, o, first, end, T[g])
            assert cover.max(initial=0) <= 2
            two = cover == 2
            # (two utterances on a sample are neighbours, but for empty rows between them, which lie on no sample)
            for j in np.flatnonzero(two)[:: max(int(two.sum()) // 50, 1)]:
                assert all(lens[b] == 0 for b in range(int(lowest[j]) + 1, int(highest[j])))
            overlaps += int(two.any())
            for b in range(first + 1, end):
                gb = JR.gap_samples(gaps[b], fs)
                clamps += int(gb < 0 and -gb > min(lens[b - 1] // 2, lens[b] // 2))
    assert overlaps > 100 and clamps > 50  # the draw exercises what it is meant to


def test_refusals_of_the_plan_by_message(pkg):
    def refused(*a, **k):
        with pytest.raises(pkg.VitsError) as e:
            pkg.join_plan(*a, **k)
        return str(e.value)

    assert "rate 3999 Hz is outside [4000, 192000]" in refused(3999, [1, 2])
    assert "batch = 0 is outside [1, 65535]" in refused(FS, [])
    assert "track[0] = 1: the first utterance opens track 0" in refused(FS, [1, 2], [1, 1])
    assert "track[2] = 3 after track[1] = 1" in refused(FS, [1, 2, 3], [0, 1, 3]) and "each step is 0 or 1" in pkg.last_error()
    assert "track[2] = 0 after track[1] = 1" in refused(FS, [1, 2, 3], [0, 1, 0])
    assert "gap_ms[1] = -2000.5 (utterance 1): must be finite and in [-2000, 60000] ms" in refused(FS, [1, 2], None, [0.0, -2000.5])
    assert "gap_ms[2] = 60001 (utterance 2)" in refused(FS, [1, 2, 3], None, [0.0, 0.0, 60001.0])
    assert "gap_ms[0] = nan (utterance 0)" in refused(FS, [1, 2], None, [np.nan, 0.0])  # validated, although ignored
    assert "gap_ms[1] = inf" in refused(FS, [1, 2], None, [0.0, np.inf])
    assert "utterance 1 has a bound of -1 samples" in refused(FS, [1, -1])
    assert "utterance 0 has a bound of 1073741825 samples" in refused(FS, [(1 << 30) + 1])
    msg = refused(FS, [1 << 29, 1 << 29, 1], [0, 0, 0])
    assert "track 0 (utterances 0 .. 2) has a bound of 1073741825 samples" in msg and "split it into several tracks or calls" in msg
    assert "track 1 (utterances 1 .. 2)" in refused(48000, [5, 1 << 30, 0], [0, 1, 1], [0.0, 0.0, 1.0])  # a positive gap counts
    msg = refused(FS, [0] * 1200, None, 60000.0)  # 1199 pauses of a minute: no audio is needed to know
    assert "track 0 (utterances 0 .. 1199) has a bound of at least 1151040000 samples (its pauses alone), above the 1073741824 a track may have" in msg
    # the same cuts as two tracks are accepted
    assert pkg.join_plan(FS, [1 << 29, 1 << 29, 1], [0, 0, 1])[1].tolist() == [1 << 30, 1]
    with pytest.raises(pkg.VitsError, match="vits_join_host: lens\\[1\\] = 9 is above x_stride = 4"):
        pkg.join_host(np.zeros((2, 4), np.float32), FS, [4, 9])


def spans(pkg, text):
    raw = text.encode("utf-8")
    return [(raw[s:e].decode("utf-8"), k) for s, e, k in pkg.split_sentences(text)]


def test_the_sentence_splitter(pkg):
    assert spans(pkg, "a. b") == [("a.", 0), ("b", 0)]
    assert spans(pkg, "a.b") == [("a.b", 0)]  # no whitespace behind the stop: one span
    assert spans(pkg, "wait... what?! ok") == [("wait...", 0), ("what?!", 0), ("ok", 0)]
    assert spans(pkg, "  one.  two \t\n ") == [("one.", 0), ("two", 0)]  # leading and trailing whitespace is dropped
    assert spans(pkg, "one. two\n\nthree.\n\n\nfour\nfive") == [("one.", 0), ("two", 1), ("three.", 1), ("four\nfive", 0)]
    assert spans(pkg, "a.\n \nb") == [("a.", 1), ("b", 0)]  # the run holds two newlines, whatever lies between them
    assert spans(pkg, "\n\nfirst") == [("first", 0)]
    assert spans(pkg, "好。你好！吗？是") == [("好。", 0), ("你好！", 0), ("吗？", 0), ("是", 0)]  # U+3002, U+FF01, U+FF1F need no whitespace
    assert spans(pkg, "好。\n\n是") == [("好。", 1), ("是", 0)]
    assert spans(pkg, "") == [] and spans(pkg, " \n\n ") == []
    assert spans(pkg, "...") == [] and spans(pkg, "?! ... 。") == []  # terminators alone say nothing
    assert spans(pkg, "x. ... y") == [("x.", 0), ("y", 0)]
    # byte offsets, and a cap below the count still counts
    assert pkg.split_sentences("é. b") == [(0, 3, 0), (4, 5, 0)]
    assert pkg.lib().vits_split_sentences(b"a. b. c", None, None, None, 0) == 3
    assert pkg.lib().vits_split_sentences(None, None, None, None, 0) == -1 and "null argument" in pkg.last_error()
