"""A stated level, host side (include/vits.h vits_model_set_level): the K-weighting coefficients against the table of BS.1770, the segment lengths, the
calibration statement of BS.1770 / EBU Tech 3341 (a full-scale 997 Hz sine reads -3.01 LUFS), vits_loudness_host against the float64 restatement
(tests/loudness_ref.py) on signals that each expose one defect, the refusals, and the prototypes as a C99 caller sees them. No device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import loudness_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vits_model_set_level", "vits_model_get_level", "vits_model_last_levels", "vits_loudness_plan", "vits_loudness_host", "vits_op_level")
PROCESS_OPTS_SIZE = 160  # the level is a handle-level setting, not a field (tests/test_align_host.py pins the same number)


def test_plan_is_the_table_of_bs1770_at_48k(pkg):
    coef, S = pkg.loudness_plan(48000)
    assert coef.shape == (2, 5) and S == 4800
    assert np.abs(coef - R.BS1770_48K).max() <= 1e-12
    assert np.abs(R.coefficients(48000) - R.BS1770_48K).max() <= 1e-12  # (so does the restatement)
    for fs, want in ((16000, 1600), (22050, 2205), (8000, 800), (11025, 1103)):
        c, S = pkg.loudness_plan(fs)
        assert S == want == R.segment(fs), fs
        assert np.abs(c - R.coefficients(fs)).max() <= 1e-12, fs


@pytest.mark.parametrize("seconds", [1.0, 2.5])
def test_a_full_scale_997_hz_sine_reads_minus_3_01_lufs(pkg, seconds):
    x = np.sin(2 * np.pi * 997 * np.arange(int(48000 * seconds)) / 48000.0).astype(np.float32)
    L, P, blocks = pkg.loudness_host(x, 48000)
    print(f"{seconds} s: {L:.4f} LUFS, peak {P:.6f}, {blocks} blocks")
    assert abs(L - (-3.01)) <= 0.01
    assert blocks == int(seconds * 10) - 3
    assert abs(R.loudness(x, 48000)[0] - (-3.01)) <= 0.01


@pytest.mark.parametrize("fs", [16000, 22050])
def test_host_equals_the_restatement(pkg, fs):
    """both are double: only the association of the sums differs"""
    for name, x in R.signals(fs).items():
        want_L, want_P, want_b = R.loudness(x, fs)
        L, P, b = pkg.loudness_host(x, fs)
        print(f"{fs} {name}: {L!r} against {want_L!r}, {b} blocks")
        assert b == want_b and P == want_P, name
        if np.isfinite(want_L):
            assert abs(L - want_L) <= 1e-9, name
        else:
            assert L == -np.inf and b == 0, name
    assert not np.isfinite(R.loudness(R.sig_silence(fs), fs)[0])


def test_the_signals_expose_what_they_are_built_for():
    """on the restatement: a defect moves the reading by far more than any tolerance the levelling tests use (the figures of the definition's author)"""
    fs = 16000
    z = R.segment_means(R.sig_levels(fs), fs)
    L = R.gated(z)[0]
    assert abs(L - (-16.29)) < 0.01
    assert abs(R.gated(z, relative=False)[0] - L - (-3.05)) < 0.02
    assert abs(R.gated(z, absolute=False)[0] - L - (-2.62)) < 0.02
    assert abs(R.gated(z, absolute=False, relative=False)[0] - L - (-8.70)) < 0.02
    assert abs(R.loudness(R.sig_levels(22050), 22050)[0] - (-16.33)) < 0.01
    z = R.segment_means(R.sig_overlap(fs), fs)
    assert abs(R.gated(z, relative=False)[0] - R.gated(z)[0] - (-3.00)) < 0.02
    # blocks taken without overlap: 0.09 LU off when they start at segment 0, 0.54 when they start one segment later (the alignment decides which blocks
    # straddle the steps of the signal) — either is many times the 0.01 LU the kernels are held to
    off = R.gated(z, overlap=False)[0] - R.gated(z)[0]
    print(f"overlap dropped: {off:+.3f} LU")
    assert abs(off) > 0.05
    x = R.sig_weighting(fs)
    assert abs(R.gated(R.segment_means(x, fs, weighted=False))[0] - R.loudness(x, fs)[0] - 2.8) < 0.1
    x = (0.5 * np.sin(2 * np.pi * 997 * np.arange(2 * fs) / fs)).astype(np.float32)  # (the shelf lifts 997 Hz: unweighted reads low there)
    assert abs(R.gated(R.segment_means(x, fs, weighted=False))[0] - R.loudness(x, fs)[0] - (-0.73)) < 0.01
    # carry: one restart of the filter from zero state in the middle of the offset adds a transient of the offset's size
    x = R.sig_carry(fs).astype(np.float64)
    y = np.concatenate([R.k_weight(x[:16000], fs), R.k_weight(x[16000:], fs)])
    S = R.segment(fs)
    restarted = R.gated((y[:y.size // S * S].reshape(-1, S) ** 2).mean(axis=1))[0]
    assert restarted - R.loudness(x, fs)[0] > 3.0  # (the start at sample 0 is such a transient too: a second one adds 4.5 LU)


def test_short_and_empty_utterances(pkg):
    rng = np.random.default_rng(5)
    x = (0.1 * rng.standard_normal(5 * 1600)).astype(np.float32)
    for n, blocks in ((0, 0), (1, 0), (4 * 1600 - 1, 0), (4 * 1600, 1), (4 * 1600 + 1, 1), (5 * 1600 - 1, 1), (5 * 1600, 2)):
        L, P, b = pkg.loudness_host(x[:n], 16000)
        assert b == blocks == R.loudness(x[:n], 16000)[2], n
        assert np.isfinite(L) == (blocks > 0), n
        assert P == (float(np.abs(x[:n]).max()) if n else 0.0), n


def test_refusals_name_their_cause(pkg):
    lib = pkg.lib()
    seg = C.c_int32()
    d = C.c_double()
    x = np.zeros(8, np.float32)
    for fs in (3999, 192001, 0, -5):
        assert lib.vits_loudness_plan(fs, None, C.byref(seg)) == -1 and str(fs) in pkg.last_error(), fs
        assert lib.vits_loudness_host(x.ctypes.data_as(C.c_void_p), 8, fs, C.byref(d), None, None) == -1 and str(fs) in pkg.last_error(), fs
    assert lib.vits_loudness_plan(4000, None, None) == 0 and lib.vits_loudness_plan(192000, None, C.byref(seg)) == 0 and seg.value == 19200
    assert lib.vits_loudness_host(None, 8, 16000, C.byref(d), None, None) == -1 and "null" in pkg.last_error()
    assert lib.vits_loudness_host(None, 0, 16000, C.byref(d), None, None) == 0 and d.value == -np.inf
    assert lib.vits_model_set_level(None, R.LEVEL_GAIN, 0.0, 0.0) == -1 and "null" in pkg.last_error()
    assert lib.vits_model_get_level(None, None, None, None) == -1 and "null" in pkg.last_error()
    assert lib.vits_model_last_levels(None, None, 0) == -1 and "null" in pkg.last_error()
    assert lib.vits_op_level(None, None, None, None, None) == -1 and "null" in pkg.last_error()


def test_symbols_are_declared_exported_and_typed(pkg):
    header = open(os.path.join(ROOT, "include", "vits.h")).read()
    lib = pkg.lib()
    for s in SYMBOLS:
        assert any(line.startswith("VITS_API") and s + "(" in line for line in header.splitlines()), s
        assert s in pkg.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert (pkg.LEVEL_NONE, pkg.LEVEL_MEASURE, pkg.LEVEL_GAIN, pkg.LEVEL_PEAK, pkg.LEVEL_LOUDNESS) == (0, 1, 2, 3, 4)
    for i, name in enumerate(("NONE", "MEASURE", "GAIN", "PEAK", "LOUDNESS")):
        assert f"#define VITS_LEVEL_{name} {i}\n" in header, name
    assert C.sizeof(pkg.LevelDesc) == 40
    for name in ("set_level", "level", "last_levels"):
        assert hasattr(pkg.Model, name), name
    for name in ("loudness_plan", "loudness_host", "level"):
        assert callable(getattr(pkg, name)), name


def test_a_c99_caller_links_and_process_opts_keeps_its_size(pkg, tmp_path):
    src = tmp_path / "level.c"
    src.write_text('#include <stdio.h>\n#include <math.h>\n#include "vits.h"\n'
                   'int main(void) {\n'
                   '  int (*a)(vits_model*, int32_t, float, float) = vits_model_set_level;\n'
                   '  int (*b)(const vits_model*, int32_t*, float*, float*) = vits_model_get_level;\n'
                   '  int64_t (*c)(vits_model*, float*, size_t) = vits_model_last_levels;\n'
                   '  int (*d)(int32_t, double*, int32_t*) = vits_loudness_plan;\n'
                   '  int (*e)(const float*, size_t, int32_t, double*, double*, int32_t*) = vits_loudness_host;\n'
                   '  int (*f)(const vits_level_desc*, const float*, const int64_t*, float*, float*) = vits_op_level;\n'
                   '  static float x[16000]; double coef[10], lufs = 0, peak = 0; int32_t seg = 0, blocks = -1; size_t i;\n'
                   '  for (i = 0; i < 16000; ++i) x[i] = (i & 1) ? 0.25f : -0.25f;\n'
                   '  int ok = d(48000, coef, &seg) == 0 && seg == 4800 && e(x, 16000, 16000, &lufs, &peak, &blocks) == 0 && peak == 0.25 && blocks == 7;\n'
                   '  int refused = a(NULL, VITS_LEVEL_LOUDNESS, -23.0f, -1.0f) == -1 && b(NULL, &seg, NULL, NULL) == -1 && c(NULL, NULL, 0) == -1 &&\n'
                   '                d(3999, coef, &seg) == -1 && f(NULL, x, NULL, NULL, x) == -1;\n'
                   '  printf("%zu %zu %d %d %.6f\\n", sizeof(vits_process_opts), sizeof(vits_batch_result), ok, refused, lufs); return 0; }\n')
    exe = tmp_path / "level"
    lib_dir = os.path.join(ROOT, "vits.cpp_amd", "csrc")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", lib_dir, "-lvits_hip",
                    "-Wl,-rpath," + lib_dir], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == PROCESS_OPTS_SIZE == C.sizeof(pkg.ProcessOpts)
    assert int(out[1]) == C.sizeof(pkg.BatchResult)
    assert int(out[2]) == 1 and int(out[3]) == 1
    x = np.where(np.arange(16000) & 1, 0.25, -0.25).astype(np.float32)
    assert abs(float(out[4]) - R.loudness(x, 16000)[0]) <= 1e-5  # (six printed decimals)


def test_documents_name_the_calls():
    for doc, word in (("INTEGRATION.md", "vits_model_set_level"), ("DESIGN.md", "level_scan_kernel"), ("README.md", "vits_model_set_level"),
                      ("include/vits.h", "vits_op_level")):
        assert word in open(os.path.join(ROOT, doc)).read(), doc
