"""Any sample rate, host side (include/vits.h vits_model_set_rates): the plan and the lengths, the product's tap table against the float64
restatement (tests/resample_ref.py), what the filter does to sinusoids (passband and stopband, stated on the restatement: the table test holds
the product to it), the refusals, and the prototypes as a C99 caller sees them. No device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = {(16000, 48000): (3, 1, 71), (16000, 8000): (1, 2, 141), (16000, 44100): (441, 160, 71), (44100, 16000): (160, 441, 193),
         (16000, 22050): (441, 320, 71)}
SYMBOLS = ("vits_model_set_rates", "vits_model_get_rates", "vits_resample_plan", "vits_resample_taps", "vits_resample_length", "vits_op_resample")
PROCESS_OPTS_SIZE = 160  # the rates are handle-level settings, not fields (tests/test_align_host.py pins the same number)


def test_plan_and_lengths(pkg):
    for (fi, fo), want in PLANS.items():
        assert pkg.resample_plan(fi, fo) == want, (fi, fo)
        L, M, _, K = R.plan(fi, fo)[:4]
        assert (L, M, K) == want, (fi, fo)  # (the restatement agrees with the issue's table too)
        for n in (0, 1, 2, 159, 160, 161, 2 ** 30):
            assert pkg.resample_length(fi, fo, n) == -((-n * L) // M) == R.out_len(fi, fo, n), (fi, fo, n)


@pytest.mark.parametrize("fi,fo", sorted(PLANS))
def test_taps_equal_the_restatement(pkg, fi, fo):
    """every entry within one fp32 ulp of the float64 value rounded to fp32 (the last bits of a double I0 series and of np.i0 may differ)"""
    h = pkg.resample_taps(fi, fo)
    want = R.taps(fi, fo).astype(np.float32)
    assert h.shape == want.shape == PLANS[(fi, fo)][::2]
    ulp = np.spacing(np.abs(want))
    worst = float((np.abs(h.astype(np.float64) - want.astype(np.float64)) / ulp).max())
    print(f"{fi} -> {fo}: worst table difference {worst:.2f} ulp")
    assert worst <= 1.0


def test_refusals_name_their_cause(pkg):
    lib = pkg.lib()
    v = C.c_int32()
    for fi, fo, word in ((3999, 16000, "3999"), (16000, 192001, "192001"), (16000, 44101, "L = 44101")):
        assert lib.vits_resample_plan(fi, fo, C.byref(v), C.byref(v), C.byref(v)) == -1
        assert word in pkg.last_error(), pkg.last_error()
        assert lib.vits_resample_taps(fi, fo, None, 0) == -1 and word in pkg.last_error()
        assert lib.vits_resample_length(fi, fo, 100) == -1 and word in pkg.last_error()
    assert "K = 71" in pkg.last_error()  # (the table that is too large: both of its dimensions)
    assert lib.vits_resample_taps(16000, 48000, None, 213) == -1 and "null" in pkg.last_error()
    assert lib.vits_model_set_rates(None, 0, 8000) == -1 and "null" in pkg.last_error()
    assert lib.vits_model_get_rates(None, C.byref(v), C.byref(v)) == -1 and "null" in pkg.last_error()
    x = np.zeros(8, np.float32)
    assert lib.vits_op_resample(16000, 8000, 1, None, 8, None, x.ctypes.data_as(C.c_void_p), 8) == -1 and "null" in pkg.last_error()
    # a size query writes nothing, and a buffer that is too small is left alone
    assert lib.vits_resample_taps(16000, 48000, None, 0) == 213
    small = np.full(10, 7.0, np.float32)
    assert lib.vits_resample_taps(16000, 48000, small.ctypes.data_as(C.c_void_p), 10) == 213 and (small == 7.0).all()


@pytest.mark.parametrize("fi,fo", sorted(PLANS))
def test_the_filter_does_what_a_resampler_must(fi, fo):
    """x[n] = sin(2 pi f n / fi + 0.3), 4,000 samples, the middle 60 % of the output. Passband (f = 0.25, 0.5, 0.8 of the lower Nyquist frequency): peak
    error against sin(2 pi f m / fo + 0.3) at most -90 dB. Stopband (downsampling; f = 1.1, 1.2, 1.3, 1.5 of it): amplitude at most -100 dB."""
    ny = min(fi, fo) / 2
    n = np.arange(4000, dtype=np.float64)
    h = R.taps(fi, fo)
    for rel in (0.25, 0.5, 0.8):
        f = rel * ny
        y = R.resample(np.sin(2 * np.pi * f * n / fi + 0.3), fi, fo, h)
        m = np.arange(y.size, dtype=np.float64)
        mid = slice(int(0.2 * y.size), int(0.8 * y.size))
        err = np.abs(y - np.sin(2 * np.pi * f * m / fo + 0.3))[mid].max()
        print(f"{fi} -> {fo} passband {rel}: {20 * np.log10(err):.1f} dB")
        assert 20 * np.log10(err) <= -90.0
    if fo < fi:
        for rel in (1.1, 1.2, 1.3, 1.5):
            y = R.resample(np.sin(2 * np.pi * rel * ny * n / fi + 0.3), fi, fo, h)
            amp = np.abs(y[int(0.2 * y.size):int(0.8 * y.size)]).max()
            print(f"{fi} -> {fo} stopband {rel}: {20 * np.log10(amp):.1f} dB")
            assert 20 * np.log10(amp) <= -100.0


def test_symbols_are_declared_exported_and_typed(pkg):
    header = open(os.path.join(ROOT, "include", "vits.h")).read()
    lib = pkg.lib()
    for s in SYMBOLS:
        assert any(line.startswith("VITS_API") and s + "(" in line for line in header.splitlines()), s
        assert s in pkg.EXPORTED_SYMBOLS and hasattr(lib, s), s
    i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
    assert lib.vits_model_set_rates.restype is i32 and lib.vits_model_set_rates.argtypes == [vp, i32, i32]
    assert lib.vits_model_get_rates.restype is i32 and lib.vits_model_get_rates.argtypes == [vp, C.POINTER(i32), C.POINTER(i32)]
    assert lib.vits_resample_plan.restype is i32 and lib.vits_resample_plan.argtypes == [i32, i32] + [C.POINTER(i32)] * 3
    assert lib.vits_resample_taps.restype is i64 and lib.vits_resample_taps.argtypes == [i32, i32, vp, C.c_size_t]
    assert lib.vits_resample_length.restype is i64 and lib.vits_resample_length.argtypes == [i32, i32, i64]
    assert lib.vits_op_resample.restype is i32 and lib.vits_op_resample.argtypes == [i32, i32, i32, vp, i64, vp, vp, i64]
    for name in ("set_rates", "rates"):
        assert hasattr(pkg.Model, name), name
    for name in ("resample", "resample_plan", "resample_taps", "resample_length"):
        assert callable(getattr(pkg, name)), name


def test_a_c99_caller_links_and_process_opts_keeps_its_size(pkg, tmp_path):
    src = tmp_path / "rates.c"
    src.write_text('#include <stdio.h>\n#include "vits.h"\n'
                   'int main(void) {\n'
                   '  int (*a)(vits_model*, int32_t, int32_t) = vits_model_set_rates;\n'
                   '  int (*b)(const vits_model*, int32_t*, int32_t*) = vits_model_get_rates;\n'
                   '  int (*c)(int32_t, int32_t, int32_t*, int32_t*, int32_t*) = vits_resample_plan;\n'
                   '  int64_t (*d)(int32_t, int32_t, float*, size_t) = vits_resample_taps;\n'
                   '  int64_t (*e)(int32_t, int32_t, int64_t) = vits_resample_length;\n'
                   '  int (*f)(int32_t, int32_t, int32_t, const float*, int64_t, const int64_t*, float*, int64_t) = vits_op_resample;\n'
                   '  int32_t L = 0, M = 0, K = 0; static float h[213];\n'
                   '  int ok = c(16000, 48000, &L, &M, &K) == 0 && d(16000, 48000, h, 213) == 213 && e(16000, 44100, 161) == 444;\n'
                   '  int refused = a(NULL, 0, 8000) == -1 && b(NULL, &L, &M) == -1 && c(3999, 16000, &L, &M, &K) == -1 && f(16000, 8000, 0, h, 1, NULL, h, 1) == -1;\n'
                   '  printf("%zu %d %d %d %d %d\\n", sizeof(vits_process_opts), ok, refused, (int)L, (int)M, (int)K); return 0; }\n')
    exe = tmp_path / "rates"
    lib_dir = os.path.join(ROOT, "vits.cpp_amd", "csrc")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", lib_dir, "-lvits_hip",
                    "-Wl,-rpath," + lib_dir], check=True)
    size, ok, refused, L, M, K = map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert size == PROCESS_OPTS_SIZE == C.sizeof(pkg.ProcessOpts)
    assert ok == 1 and refused == 1 and (L, M, K) == (3, 1, 71)


def test_documents_name_the_calls():
    for doc, word in (("INTEGRATION.md", "vits_model_set_rates"), ("DESIGN.md", "resample_kernel"), ("README.md", "vits_model_set_rates"),
                      ("include/vits.h", "vits_op_resample")):
        assert word in open(os.path.join(ROOT, doc)).read(), doc
