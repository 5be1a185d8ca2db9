"""Forced alignment, host side: the new symbols are declared, exported and typed; vits_process_opts did not grow; the header is C99; the fixture script's
float64 search and the GPU test's fp32 search (both restate VITS maximum_path) agree on the fixtures' own likelihood matrices."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["align_tiny_speakers_hf_export_taps.npz", "align_tiny_speakers_hf_export_refmode_taps.npz", "align_tiny_flows3_taps.npz", "align_full_synth_taps.npz"]
PROCESS_OPTS_SIZE = 160  # sizeof(vits_process_opts) before alignment existed: the call adds arguments, not fields


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def gpu_test():
    return load(os.path.join(ROOT, "tests", "test_gpu_align.py"), "gpu_align_restatement")


def test_alignment_symbols_are_declared_exported_and_typed(pkg):
    header = open(os.path.join(ROOT, "include", "vits.h")).read()
    lib = pkg.lib()
    for s in ("vits_model_align_batch", "vits_model_align", "vits_model_hop", "vits_op_align"):
        assert "VITS_API" in header and s + "(" in header, s
        assert s in pkg.EXPORTED_SYMBOLS and hasattr(lib, s), s
    f = lib.vits_model_align_batch
    assert f.restype is C.c_int32 and len(f.argtypes) == 14 and f.argtypes[9] is C.c_float and f.argtypes[10] == C.POINTER(pkg.ProcessOpts)
    f = lib.vits_model_align
    assert f.restype is C.c_int64 and len(f.argtypes) == 8 and f.argtypes[3] is C.c_char_p
    assert lib.vits_op_align.restype is C.c_int32 and len(lib.vits_op_align.argtypes) == 9
    for name in ("align_batch", "align", "hop"):
        assert hasattr(pkg.Model, name), name
    assert callable(pkg.durations_to_seconds) and callable(pkg.op_align)


def test_process_opts_keeps_its_size_and_the_header_is_c99(pkg, tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "vits.h"\n'
                   'int main(void) { int (*f)(vits_model*, const float*, const int64_t*, int32_t, int64_t, const int32_t*, const int32_t*, int32_t, const int32_t*,\n'
                   '    float, const vits_process_opts*, int32_t*, int64_t*, float*) = vits_model_align_batch;\n'
                   '  int64_t (*g)(vits_model*, const float*, size_t, const char*, int32_t, int32_t*, int32_t*, size_t) = vits_model_align;\n'
                   '  printf("%zu %d\\n", sizeof(vits_process_opts), f != 0 && g != 0); return 0; }\n')
    exe = tmp_path / "size"
    lib_dir = os.path.join(ROOT, "vits.cpp_amd", "csrc")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", lib_dir, "-lvits_hip",
                    "-Wl,-rpath," + lib_dir], check=True)
    size, linked = map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert size == PROCESS_OPTS_SIZE == C.sizeof(pkg.ProcessOpts) and linked == 1


def test_null_handles_and_arguments_are_refused(pkg):
    lib = pkg.lib()
    d = np.zeros(4, np.int32)
    assert lib.vits_model_align_batch(None, None, None, 1, 1, None, None, 1, None, 0.0, None, d.ctypes.data, None, None) == -1
    assert "null" in pkg.last_error()
    assert lib.vits_model_align(None, None, 0, b"a", -1, None, None, 0) == -1
    assert lib.vits_model_hop(None) == 0
    assert lib.vits_op_align(0, None, None, 4, None, None, None, None, None) == -1


@pytest.mark.parametrize("fixture", FIXTURES)
def test_float64_and_fp32_searches_agree_on_the_fixtures_logp(gpu_test, fixture):
    make = load(os.path.join(GOLDEN, "make_golden_align.py"), "make_golden_align_restatement") if importlib.util.find_spec("torch") else None
    g = golden(fixture)
    for k in range(len(g["cases"])):
        lp64 = g["c%d_logp64" % k]
        T, L = lp64.shape
        d64, s64 = g["c%d_durations64" % k], float(g["c%d_score64" % k][0])
        assert d64.sum() == L and d64.min() >= 1
        # the test module's vectorised search in float64 is the fixture script's loop
        d, sc, path = gpu_test.mas(lp64)
        np.testing.assert_array_equal(d, d64)
        assert sc == s64
        np.testing.assert_array_equal(path, np.repeat(np.arange(T), d64))
        if make is not None:
            dm, sm = make.mas(lp64)
            np.testing.assert_array_equal(dm, d64)
            assert float(sm) == s64
            np.testing.assert_allclose(make.logp(g["c%d_prior_mean" % k], g["c%d_prior_logvar" % k], g["c%d_z_p" % k], np.float64), lp64, rtol=0, atol=0)
        # in fp32 on the rounded matrix: a path within the proven bound of the float64 optimum (e = the rounding of the matrix itself)
        lp32 = lp64.astype(np.float32)
        d32, s32, p32 = gpu_test.mas(lp32)
        e = float(np.abs(lp32.astype(np.float64) - lp64).max())
        assert d32.sum() == L and d32.min() >= 1
        assert gpu_test.path_score64(lp64, p32) >= s64 - 2 * L * e - L * float(np.spacing(np.float32(abs(s64))))
        assert abs(float(s32) - s64) <= 2 * L * e + L * float(np.spacing(np.float32(abs(s64))))


def test_planted_durations_are_recovered_by_both_restatements(gpu_test):
    for i, (T, L) in enumerate([(17, 65), (65, 304), (33, 54), (40, 40)]):
        d, m, ls, z = gpu_test.planted(T, L, 192, 100 + i)
        for dt in (np.float32, np.float64):
            got, _, _ = gpu_test.mas(gpu_test.logp_formula(m, ls, z, dt))
            np.testing.assert_array_equal(got, d, err_msg=str((T, L, dt)))


def test_documents_name_the_call():
    for doc, word in (("INTEGRATION.md", "vits_model_align_batch"), ("DESIGN.md", "align_mas"), ("README.md", "align")):
        assert word in open(os.path.join(ROOT, doc)).read(), doc
