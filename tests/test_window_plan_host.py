"""The vocoder window plan (vits.cpp_amd/csrc/window_plan.cpp: long-form / streaming calls run HiFiGAN window by window), on the CPU.

tests/window_plan_dump.cpp links window_plan.o ALONE (that the link succeeds is the proof that the planner needs no kernel, no device and no engine) and
prints everything the plan states for a case given on standard input. Here the dump is compared with a numpy restatement written from the definitions (a
window owns frames [f0, f1) and computes [lo, hi); include/vits.h: vocoder_chunk_frames, on_chunk), and the properties streaming rests on are asserted:
the owned ranges partition the frames, every utterance's chunks tile its samples, the range tables tile what is final. The same program, built with
AddressSanitizer + UBSan as a stand-alone executable, runs the same cases."""
import itertools
import os
import random
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vits.cpp_amd", "csrc")

# stage lengths as affine functions of the frame count: the tiny synthetic model (upsample rates 4, 2; kernels 8, 4; cropped), and a made-up set whose last
# stage keeps a tail (sadd[n_up] > 0: the no-crop tail of the utterance's last window)
AFFINE = [((1, 4, 8), (0, 0, 0)), ((1, 2, 6, 12), (0, 1, 5, 11))]
B = 4


def build(target):
    subprocess.check_call(["make", "-s", "-C", CSRC, target])
    return os.path.join(CSRC, target)


def run(exe, lines, env=None):
    got = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env)
    assert got.returncode == 0, got.stderr[-2000:]
    out = got.stdout.splitlines()
    assert len(out) == len(lines)
    return out


@pytest.fixture(scope="module")
def dump():
    return build("window_plan_dump")


def cases():
    """(chunk, collect_taps, halo, smul, sadd, frames): chunks 1, 3, 8; halos 0, 2, 5 (also larger than the chunk); batches of four drawn from
    {1, W - 1, W, W + 1, 2 W, 2 W + halo + 1}; a chunk at least as long as the longest utterance, and collect_taps: one window each"""
    rng = random.Random(20250309)
    for (smul, sadd), W, halo in itertools.product(AFFINE, (1, 3, 8), (0, 2, 5)):
        pool = [f for f in (1, W - 1, W, W + 1, 2 * W, 2 * W + halo + 1) if f >= 1]
        batches = [pool[:B], pool[-B:], pool[-B:][::-1]] + [[rng.choice(pool) for _ in range(B)] for _ in range(3)]
        for frames in batches:
            frames = (frames + [1] * B)[:B]
            yield W, 0, halo, smul, sadd, frames
        frames = batches[1]
        yield max(frames), 0, halo, smul, sadd, frames      # a chunk of exactly the longest utterance
        yield max(frames) + 5, 0, halo, smul, sadd, frames
        yield 0, 0, halo, smul, sadd, frames                # no chunking asked for
        yield W, 1, halo, smul, sadd, frames                # collect_taps


def case_line(c):
    W, taps, halo, smul, sadd, frames = c
    return " ".join(map(str, [W, taps, halo, len(smul) - 1, *smul, *sadd, len(frames), *frames]))


def made_up_final(e, slen):
    """a monotone final_of with final_of(slen) = slen: two thirds of what is final, everything once the utterance has ended"""
    return e if e == slen else 2 * e // 3


def restate(c):
    """the plan by its definition, as the sections of the dump"""
    W, taps, halo, smul, sadd, frames = c
    smul, sadd, frames = np.array(smul), np.array(sadd), np.array(frames)
    n_up, M, tail = len(smul) - 1, int(smul[-1]), int(sadd[-1])
    Lmax = int(frames.max())
    slen = frames * M + tail
    if W > 0 and not taps and W < Lmax:
        wins = [(f0, min(Lmax, f0 + W), max(0, f0 - halo), min(Lmax, f0 + W + halo)) for f0 in range(0, Lmax, W)]
    else:
        wins = [(0, Lmax, 0, Lmax)]
    windowed = len(wins) > 1
    head = [int(windowed), max(hi - lo for _, _, lo, hi in wins), Lmax, M, len(wins)]
    per_win, per_utt, table = [], [], []
    final = {"id": np.zeros(B, int), "made_up": np.zeros(B, int)}
    ranges = {"id": [], "made_up": []}
    for f0, f1, lo, hi in wins:
        lf = np.minimum(frames, hi) - lo                                      # frames of every utterance inside the window
        lens = np.where(lf[None, :] > 0, lf[None, :] * smul[:, None] + sadd[:, None], 0)  # [stage][utterance]
        owns, ends = frames > f0, frames <= f1
        emit_end = np.where(owns, np.where(ends, (frames - lo) * M + tail, (f1 - lo) * M), 0)
        final_end = np.where(ends, slen, f1 * M)
        per_win += [f0, f1, lo, hi, (f0 - lo) * M, f0 * M, min(int(slen.max()), f1 * M + tail)]
        for i in range(n_up + 1):
            per_win += [(hi - lo) * int(smul[i]) + int(sadd[i]), int(lens[i].sum())]
        for b in range(B):
            per_utt += [int(lf[b]), *map(int, lens[:, b]), int(emit_end[b]), int(owns[b]), f0 * M, int(final_end[b])]
        table += [*map(int, lens.ravel()), *map(int, emit_end)]
        for key, fn in (("id", lambda e, s: e), ("made_up", made_up_final)):
            after = np.array([max(int(final[key][b]), fn(int(final_end[b]), int(slen[b]))) if owns[b] else int(final[key][b]) for b in range(B)])
            ranges[key] += [*map(int, final[key]), *map(int, after)]
            final[key] = after
    return [head, per_win, per_utt, table if windowed else [], ranges["id"], ranges["made_up"]]


def parse(line):
    return [[int(v) for v in sec.split()] for sec in line.split("|")]


def test_the_dump_is_the_restatement(dump):
    cs = list(cases())
    assert {c[0] for c in cs if not c[1]} >= {1, 3, 8} and {c[2] for c in cs} == {0, 2, 5} and any(c[2] > c[0] > 0 for c in cs)
    for c, line in zip(cs, run(dump, [case_line(c) for c in cs])):
        got, want = parse(line), restate(c)
        assert len(got) == 6
        for name, g, w in zip(("head", "windows", "utterances", "device table", "ranges", "made-up ranges"), got, want):
            assert g == w, (c, name, g[:16], w[:16])


def windows_of(c, secs):
    n_up = len(c[3]) - 1
    per = 7 + 2 * (n_up + 1)
    return [secs[1][i * per:(i + 1) * per] for i in range(secs[0][4])]


def utterance(c, secs, w, b):
    n_up = len(c[3]) - 1
    per = n_up + 6
    v = secs[2][(w * B + b) * per:(w * B + b + 1) * per]
    return dict(lf=v[0], lens=v[1:n_up + 2], emit_end=v[n_up + 2], owns=v[n_up + 3], begin=v[n_up + 4], final_end=v[n_up + 5])


def test_owned_ranges_partition_the_frames_and_chunks_tile_every_utterance(dump):
    cs = list(cases())
    for c, line in zip(cs, run(dump, [case_line(c) for c in cs])):
        W, taps, halo, smul, sadd, frames = c
        secs = parse(line)
        wins = windows_of(c, secs)
        Lmax, M = max(frames), smul[-1]
        # owned ranges: [0, Lmax) with no gap or overlap; computed ranges: the owned ones widened by the halo inside [0, Lmax)
        assert wins[0][0] == 0 and wins[-1][1] == Lmax and all(a[1] == b[0] for a, b in zip(wins, wins[1:])) and all(w[0] < w[1] for w in wins)
        assert all(w[2] == max(0, w[0] - halo) and w[3] == min(Lmax, w[1] + halo) for w in wins) or len(wins) == 1
        assert len(wins) == 1 or all(w[1] - w[0] == W for w in wins[:-1])
        for b in range(B):
            slen = frames[b] * M + sadd[-1]
            at = 0
            for w, win in enumerate(wins):
                u = utterance(c, secs, w, b)
                if not u["owns"]:
                    assert u["emit_end"] == 0 and frames[b] <= win[0]
                    continue
                # the plain chunk [f0 M, E_w(b)) continues the previous one, and is what the window emits: emit_end - emit_lo samples
                assert u["begin"] == at == win[0] * M and u["final_end"] > at, (c, w, b)
                assert u["final_end"] - u["begin"] == u["emit_end"] - win[4], (c, w, b)
                # ... which lie inside what the window computed of the utterance at the last stage, and inside the copy span
                assert 0 <= win[4] and u["emit_end"] <= u["lens"][-1], (c, w, b)
                assert win[5] <= u["begin"] and u["final_end"] <= win[6], (c, w, b)
                at = u["final_end"]
            assert at == slen, (c, b)


def test_range_tables_tile_what_is_final(dump):
    cs = list(cases())
    for c, line in zip(cs, run(dump, [case_line(c) for c in cs])):
        W, taps, halo, smul, sadd, frames = c
        secs = parse(line)
        nw = secs[0][4]
        for sec in (secs[4], secs[5]):  # final_of = the identity, and the made-up one: both end at the utterance's samples
            t = np.array(sec).reshape(nw, 2, B)
            assert (t[0, 0] == 0).all() and (t[:, 1] >= t[:, 0]).all()
            assert (t[1:, 0] == t[:-1, 1]).all()
            assert (t[-1, 1] == np.array(frames) * smul[-1] + sadd[-1]).all(), (c, t[-1, 1])


def test_one_window_holds_the_whole_utterances(dump):
    cs = [c for c in cases() if c[1] or c[0] == 0 or c[0] >= max(c[5])]
    assert len(cs) >= 4 * 18  # per stage set, chunk and halo: a chunk of the longest utterance, a longer one, none, and collect_taps
    for c, line in zip(cs, run(dump, [case_line(c) for c in cs])):
        W, taps, halo, smul, sadd, frames = c
        secs = parse(line)
        assert secs[0][0] == 0 and secs[0][4] == 1 and secs[0][1] == max(frames) and secs[3] == []
        assert windows_of(c, secs)[0][:5] == [0, max(frames), 0, max(frames), 0]
        for b in range(B):
            assert utterance(c, secs, 0, b)["lens"] == [frames[b] * m + a for m, a in zip(smul, sadd)]


def test_planner_under_the_sanitizers(dump):
    """the same cases through the AddressSanitizer + UBSan build of the same two sources (a stand-alone program): same output, clean exit"""
    asan = build("_asan/window_plan_dump")
    lines = [case_line(c) for c in cases()]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")
    assert run(asan, lines, env) == run(dump, lines)
