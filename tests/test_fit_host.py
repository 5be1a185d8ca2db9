"""A stated duration on the CPU (include/vits.h "a stated duration"): the product's host definition, vits_fit_host, against the numpy restatement
(tests/fit_ref.py), integer for integer and with the scale's bits equal; the properties the definition promises (a status-0 group lasts F frames, a clamped
group is a speaking_rates call, at most 26 bisection steps); the refusals; a C99 caller; and the same definition as a stand-alone program under
AddressSanitizer + UBSan (tests/fit_host_driver.cpp links fit_host.cpp ALONE). Two seeded defects of the restatement show that the comparison can fail."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fit_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vits.cpp_amd", "csrc")
PROCESS_OPTS_SIZE = 160


def case(rng, kind):
    """a seeded batch: (e [B, T], lens, fixed or None, groups or None, targets, min_rate, max_rate)"""
    B = int(rng.integers(1, 7))
    T = int(rng.integers(1, 40))
    lens = rng.integers(1, T + 1, B)
    lw = rng.normal(0.5, 1.0, (B, T)).astype(np.float32)
    if kind % 4 == 0:
        lw[:] = lw[0, 0]  # rows of equal e: remainders up to the group size - 1
    if kind % 5 == 1:
        lw[:, : T // 2] = lw[0, 0]
    e = np.exp(lw).astype(np.float32)
    fixed = np.where(rng.random((B, T)) < 0.15, rng.integers(0, 9, (B, T)), -1).astype(np.int32) if kind % 3 == 0 else None
    groups = [None, np.zeros(B, np.int32), rng.integers(0, B, B).astype(np.int32)][kind % 3]
    g = np.arange(B) if groups is None else groups
    f = np.full((B, T), -1) if fixed is None else fixed
    natural = np.zeros(B, np.int64)
    for b in range(B):
        natural[g[b]] += FR.frames(e[b, :lens[b]], 1.0, f[b, :lens[b]]).sum()
    targets = np.maximum(1, (natural * rng.uniform(0.3, 3.0, B)).astype(np.int64))
    targets[natural == 0] = 0 if kind % 2 else 5  # (a group nobody names: fitted or not, its row says -1)
    if kind % 7 == 3:
        targets[int(rng.integers(0, B))] = 0
    lo, hi = [(0.1, 10.0), (0.5, 2.0), (0.8, 1.25), (1.0, 1.0)][(kind // 2) % 4 if kind % 2 else 0]
    return e, lens, fixed, groups, targets, lo, hi


def same(got, want):
    (gd, gr), (wd, wr) = got, want
    return np.array_equal(gd, wd) and np.array_equal(gr.view(np.uint64), wr.view(np.uint64))


def test_the_host_definition_is_the_restatement(pkg):
    rng = np.random.default_rng(11)
    steps, remainders, status = [], 0, {-1: 0, 0: 0, 1: 0, 2: 0}
    for kind in range(240):
        e, lens, fixed, groups, targets, lo, hi = case(rng, kind)
        got = pkg.fit_host(e, targets, lens, fixed, groups, lo, hi)
        want = FR.fit(e, targets, lens, fixed, groups, lo, hi, steps_out=steps)
        assert same(got, want), kind
        dur, rows = got
        for g in range(e.shape[0]):
            F, n, s, R, st = rows[g]
            status[int(st)] += 1
            remainders += R > 0
            if st == 0:
                assert n == F, (kind, g)  # a fitted group lasts its target
            if st == 1:
                assert n > F and np.float32(s) == FR.limits(lo, hi)[0]
            if st == 2:
                assert n < F and np.float32(s) == FR.limits(lo, hi)[1]
        members = np.arange(e.shape[0]) if groups is None else groups
        for b in range(e.shape[0]):
            assert (dur[b, lens[b]:] == -1).all()
            if targets[members[b]] == 0:
                assert np.array_equal(dur[b, :lens[b]], np.full(lens[b], -1) if fixed is None else fixed[b, :lens[b]])
            else:
                assert (dur[b, :lens[b]] >= 0).all()
    print("bisection steps at most", max(steps), "groups with a remainder", remainders, "status", status)
    assert max(steps) <= 26 and remainders >= 20 and min(status.values()) >= 5


def test_targets_at_and_around_a_step(pkg):
    """F exactly n(s) for a float s, one above and one below: the sum is F each time, and the scale moves to the other side of the step"""
    rng = np.random.default_rng(12)
    e = np.exp(rng.normal(0.5, 1.0, (1, 50))).astype(np.float32)
    free = np.full(50, -1)
    for s in (0.5, 0.73, 1.0, 1.9):
        n = int(FR.frames(e[0], np.float32(s), free).sum())
        scales = []
        for F in (n - 1, n, n + 1):
            got = pkg.fit_host(e, [F])
            assert same(got, FR.fit(e, [F]))
            assert got[0].sum() == F and got[1][0, 4] == 0
            scales.append(np.float32(got[1][0, 2]))
        assert scales[0] < np.float32(s) <= scales[1] <= scales[2]
    # one token: d = F whenever the limits allow it; equal tokens: the remainder goes to the first ones
    for F in (1, 2, 17, 1000):
        d, rows = pkg.fit_host(np.float32([[3.7]]), [F], min_rate=0.1, max_rate=10.0)
        want = min(max(F, int(np.ceil(np.float32(3.7) * FR.limits(0.1, 10)[0]))), int(np.ceil(np.float32(3.7) * FR.limits(0.1, 10)[1])))
        assert d[0, 0] == want and same((d, rows), FR.fit(np.float32([[3.7]]), [F]))
    e = np.full((2, 6), 2.5, np.float32)
    d, rows = pkg.fit_host(e, [40, 0], groups=[0, 0])
    assert same((d, rows), FR.fit(e, [40, 0], groups=[0, 0]))
    assert d.tolist() == [[4, 4, 4, 4, 3, 3], [3, 3, 3, 3, 3, 3]] and rows[0].tolist()[:2] == [40, 40] and rows[0, 3] == 4 and rows[0, 4] == 0 and rows[1, 4] == -1


def test_a_clamped_fit_is_a_speaking_rate(pkg):
    rng = np.random.default_rng(13)
    e = np.exp(rng.normal(0.5, 1.0, (3, 30))).astype(np.float32)
    lens = np.int32([30, 7, 19])
    for rate, F, st in ((1.5, 1, 1), (0.75, 1 << 22, 2)):
        d, rows = pkg.fit_host(e, [F, F, F], lens, min_rate=min(rate, 1.0) if st == 2 else 0.5, max_rate=rate if st == 1 else 2.0)
        s = np.float32(1.0 / float(np.float32(rate)))  # the engine's expression for the length scale of speaking_rates[b]
        for b in range(3):
            assert np.array_equal(d[b, :lens[b]], np.ceil(e[b, :lens[b]] * s).astype(np.int32))
            assert rows[b, 4] == st and np.float32(rows[b, 2]) == s and rows[b, 3] == 0
    # min_rate = max_rate: nothing to search; status says on which side of the target the frames fell
    d, rows = pkg.fit_host(e, [10, 32, 100000], lens, min_rate=1.25, max_rate=1.25)
    assert same((d, rows), FR.fit(e, [10, 32, 100000], lens, min_rate=1.25, max_rate=1.25))
    assert rows[0, 4] == 1 and rows[2, 4] == 2 and len({np.float32(r[2]) for r in rows}) == 1


def test_seeded_defects_are_found(pkg):
    """the remainder handed to the wrong end, and < for <= in the bisection: each changes some case of the first test's kind, so that test can fail"""
    rng = np.random.default_rng(11)
    found = {"wrong_end": 0, "strict": 0}
    for kind in range(120):
        e, lens, fixed, groups, targets, lo, hi = case(rng, kind)
        got = pkg.fit_host(e, targets, lens, fixed, groups, lo, hi)
        for defect in found:
            found[defect] += not same(got, FR.fit(e, targets, lens, fixed, groups, lo, hi, defect=defect))
    print(found)
    assert found["wrong_end"] >= 5 and found["strict"] >= 5


def test_refusals(pkg):
    e = np.ones((2, 4), np.float32)
    for kw, msg in (
        (dict(targets=[-1, 0]), r"target_frames\[0\] = -1 \(group 0\)"),
        (dict(targets=[1, (1 << 22) + 1]), r"target_frames\[1\] = 4194305 \(group 1\)"),
        (dict(targets=[1, 1], groups=[0, 2]), r"groups\[1\] = 2: outside \[0, 2\)"),
        (dict(targets=[1, 1], groups=[-1, 0]), r"groups\[0\] = -1"),
        (dict(targets=[1, 1], lens=[5, 1]), r"lens\[0\] = 5: outside \[0, t_stride = 4\]"),
        (dict(targets=[1, 1], fixed=np.int32([[0, -2, 0, 0], [0, 0, 0, 0]])), r"fixed\[0\]\[1\] = -2"),
        (dict(targets=[1, 1], min_rate=0.05), r"0.1 <= min_rate <= max_rate <= 10"),
        (dict(targets=[1, 1], max_rate=10.5), r"0.1 <= min_rate <= max_rate <= 10"),
        (dict(targets=[1, 1], min_rate=2.0, max_rate=1.0), r"0.1 <= min_rate <= max_rate <= 10"),
        (dict(targets=[1, 1], min_rate=float("nan")), r"0.1 <= min_rate <= max_rate <= 10"),
    ):
        with pytest.raises(pkg.VitsError, match=msg):
            pkg.fit_host(e, **kw)
    # (a fixed value behind a length is never read)
    pkg.fit_host(e, [3, 3], lens=[2, 2], fixed=np.int32([[0, 1, -7, -7], [-1, -1, -7, -7]]))
    assert pkg.lib().vits_fit_host(2, 4, None, None, None, None, None, 0.5, 2.0, None, None) == -1 and "null argument" in pkg.last_error()


def test_a_c99_caller_links_and_process_opts_keeps_its_size(pkg, tmp_path):
    for s in ("vits_fit_host", "vits_op_fit_durations", "vits_model_set_fit", "vits_model_set_fit_total", "vits_model_fit_frames", "vits_model_last_fit"):
        assert s in pkg.EXPORTED_SYMBOLS and hasattr(pkg.lib(), s)
    for name in ("set_fit", "set_fit_total", "fit_frames", "last_fit"):
        assert hasattr(pkg.Model, name), name
    src = tmp_path / "fit.c"
    src.write_text('#include <stdio.h>\n#include "vits.h"\n'
                   'int main(void) {\n'
                   '  int (*a)(vits_model*, const int64_t*, const int32_t*, int32_t, float, float) = vits_model_set_fit;\n'
                   '  int (*b)(vits_model*, int64_t, float, float) = vits_model_set_fit_total;\n'
                   '  int64_t (*c)(const vits_model*, double) = vits_model_fit_frames;\n'
                   '  int64_t (*d)(vits_model*, double*, size_t) = vits_model_last_fit;\n'
                   '  int (*op)(int32_t, int32_t, int32_t, int32_t, const float*, const int32_t*, const int32_t*, const int32_t*, const int64_t*, float, float, float*,\n'
                   '            int32_t*, double*) = vits_op_fit_durations;\n'
                   '  float e[4] = {2.5f, 2.5f, 2.5f, 2.5f}; int64_t F[1] = {13}; int32_t dur[4]; double row[5];\n'
                   '  int ok = vits_fit_host(1, 4, e, NULL, NULL, NULL, F, 0.1f, 10.f, dur, row) == 0;\n'
                   '  int refused = a(NULL, F, NULL, 1, 0.1f, 10.f) == -1 && b(NULL, 1, 0.1f, 10.f) == -1 && c(NULL, 1.0) == -1 && d(NULL, row, 5) == -1 && op != NULL;\n'
                   '  printf("%zu %d %d %d %d %d %d %d %d\\n", sizeof(vits_process_opts), ok, refused, dur[0], dur[1], dur[2], dur[3], (int)row[1], (int)row[3]); return 0; }\n')
    exe = tmp_path / "fit"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", CSRC, "-lvits_hip",
                    "-Wl,-rpath," + CSRC], check=True)
    size, ok, refused, *rest = map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert size == PROCESS_OPTS_SIZE == C.sizeof(pkg.ProcessOpts)
    assert ok == 1 and refused == 1 and rest == [4, 3, 3, 3, 13, 1]


def test_the_definition_alone_under_the_sanitizers():
    """fit_host.cpp as a stand-alone program, in buffers of exactly the stated sizes with NaN / INT_MIN behind every length"""
    rng = np.random.default_rng(14)
    cases = [case(rng, kind) for kind in range(60)]
    text = [str(len(cases))]
    for e, lens, fixed, groups, targets, lo, hi in cases:
        B, T = e.shape
        g = np.arange(B) if groups is None else groups
        f = np.full((B, T), -1) if fixed is None else fixed
        text.append("%d %d %.9g %.9g" % (B, T, lo, hi))
        text.append(" ".join(map(str, lens)))
        text.append(" ".join(map(str, g)))
        text.append(" ".join(map(str, targets)))
        text.append(" ".join("%x" % v for b in range(B) for v in e[b, :lens[b]].view(np.uint32)))
        text.append(" ".join(str(v) for b in range(B) for v in f[b, :lens[b]]))
    subprocess.check_call(["make", "-s", "-C", CSRC, "_asan/fit_host_driver"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")
    got = subprocess.run([os.path.join(CSRC, "_asan", "fit_host_driver")], input="\n".join(text) + "\n", capture_output=True, text=True, env=env)
    assert got.returncode == 0, got.stderr[-2000:]
    lines = got.stdout.splitlines()
    assert len(lines) == 2 * len(cases)
    for k, (e, lens, fixed, groups, targets, lo, hi) in enumerate(cases):
        dur, rows = FR.fit(e, targets, lens, fixed, groups, lo, hi)
        assert list(map(int, lines[2 * k].split())) == [int(v) for b in range(e.shape[0]) for v in dur[b, :lens[b]]], k
        raw = np.array(list(map(int, lines[2 * k + 1].split())), np.int64).reshape(-1, 5)
        assert np.array_equal(raw[:, [0, 1, 3, 4]], rows[:, [0, 1, 3, 4]].astype(np.int64)), k
        for g in range(e.shape[0]):
            if rows[g, 4] >= 0:
                assert raw[g, 2] == FR.bits(rows[g, 2]), (k, g)
