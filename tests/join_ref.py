"""Joined tracks restated in numpy (include/vits.h "joined tracks", the definition): int64 offsets, fp32 rows, one fp32 add. Not a copy of
join_host.cpp: the offsets come from the recurrence as it is written in the header, the samples from a per-sample census of the utterances that cover
them. Shared by the CPU and the GPU tests of the feature."""
import math

import numpy as np

FS = 16000


def gap_samples(ms, fs):
    """g_b = sign(ms) floor(|ms| fs / 1000 + 0.5) of the fp32 value"""
    ms = float(np.float32(ms))
    mag = int(math.floor(abs(ms) * fs / 1000 + 0.5))
    return -mag if ms < 0 else mag


def tracks_of(B, track):
    """[(first, end)] of every track; track None = one track"""
    if track is None:
        return [(0, B)]
    track = [int(t) for t in track]
    assert track[0] == 0 and all(track[b] - track[b - 1] in (0, 1) for b in range(1, B))
    firsts = [b for b in range(B) if b == 0 or track[b] != track[b - 1]]
    return list(zip(firsts, firsts[1:] + [B]))


def offsets(lens, fs, track=None, gap_ms=None):
    """(o int64 [B], T int64 [G], bounds int64 [G]) for utterances of lens samples (which are their own bounds)"""
    B = len(lens)
    gaps = [0.0] * B if gap_ms is None else [float(g) for g in np.broadcast_to(np.asarray(gap_ms, np.float32), (B,))]
    o, T, bounds = np.zeros(B, np.int64), [], []
    for first, end in tracks_of(B, track):
        bound = 0
        for b in range(first, end):
            n = int(lens[b])
            bound += n
            if b > first:
                g, n_prev = gap_samples(gaps[b], fs), int(lens[b - 1])
                step = g if g >= 0 else -min(-g, n_prev // 2, n // 2)
                o[b] = o[b - 1] + n_prev + step
                bound += max(g, 0)
        T.append(int(o[end - 1]) + int(lens[end - 1]))
        bounds.append(bound)
    return o, np.asarray(T, np.int64), np.asarray(bounds, np.int64)


def join(rows, fs, track=None, gap_ms=None):
    """rows: a list of float32 arrays (utterance b is rows[b], all of it). Returns (tracks: a list of float32 arrays of T_g samples, o, T, bounds)."""
    lens = [len(r) for r in rows]
    o, T, bounds = offsets(lens, fs, track, gap_ms)
    out = []
    for g, (first, end) in enumerate(tracks_of(len(rows), track)):
        y = np.zeros(int(T[g]), np.float32)  # +0 where nothing lies
        cover = np.zeros(int(T[g]), np.int32)
        for b in range(first, end):
            x = np.asarray(rows[b], np.float32)
            seg = slice(int(o[b]), int(o[b]) + lens[b])
            once = cover[seg] == 0
            # one utterance: its sample, bit for bit; a second one: one fp32 add
            y[seg] = np.where(once, x, (y[seg] + x).astype(np.float32))
            cover[seg] += 1
        assert cover.max(initial=0) <= 2
        out.append(y)
    return out, o, T, bounds


def census(lens, o, first, end, T):
    """how many utterances of [first, end) cover each sample of a track, and whether those that do are neighbours"""
    cover = np.zeros(int(T), np.int32)
    lowest = np.full(int(T), -1, np.int64)
    highest = np.full(int(T), -1, np.int64)
    for b in range(first, end):
        seg = slice(int(o[b]), int(o[b]) + int(lens[b]))
        cover[seg] += 1
        lowest[seg] = np.where(lowest[seg] < 0, b, lowest[seg])
        highest[seg] = b
    return cover, lowest, highest
