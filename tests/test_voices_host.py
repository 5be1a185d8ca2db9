"""Custom voices, host side: the six symbols are declared, exported and typed; a C99 caller links against them; vits_process_opts did not grow;
NULL handles and arguments are refused without a device."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vits_model_speaker_embedding_size", "vits_model_get_speaker_embedding", "vits_model_add_voices", "vits_model_set_voice",
           "vits_model_clear_voices", "vits_model_num_voices")
PROCESS_OPTS_SIZE = 160  # voices add calls, not fields (tests/test_align_host.py pins the same number)


def test_voice_symbols_are_declared_exported_and_typed(pkg):
    header = open(os.path.join(ROOT, "include", "vits.h")).read()
    lib = pkg.lib()
    for s in SYMBOLS:
        assert any(line.startswith("VITS_API") and s + "(" in line for line in header.splitlines()), s
        assert s in pkg.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert lib.vits_model_speaker_embedding_size.restype is C.c_int32 and lib.vits_model_speaker_embedding_size.argtypes == [C.c_void_p]
    assert lib.vits_model_num_voices.restype is C.c_int32 and lib.vits_model_num_voices.argtypes == [C.c_void_p]
    f = lib.vits_model_get_speaker_embedding
    assert f.restype is C.c_int32 and f.argtypes == [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t]
    f = lib.vits_model_add_voices
    assert f.restype is C.c_int32 and f.argtypes == [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    f = lib.vits_model_set_voice
    assert f.restype is C.c_int32 and f.argtypes == [C.c_void_p, C.c_int32, C.c_void_p]
    assert lib.vits_model_clear_voices.restype is C.c_int32 and lib.vits_model_clear_voices.argtypes == [C.c_void_p]
    for name in ("add_voices", "set_voice", "clear_voices", "num_voices", "speaker_embedding_size", "speaker_embedding", "add_voice_mix"):
        assert hasattr(pkg.Model, name), name


def test_a_c99_caller_links_and_process_opts_keeps_its_size(pkg, tmp_path):
    src = tmp_path / "voices.c"
    src.write_text('#include <stdio.h>\n#include "vits.h"\n'
                   'int main(void) {\n'
                   '  int32_t (*a)(const vits_model*) = vits_model_speaker_embedding_size;\n'
                   '  int (*b)(vits_model*, int32_t, float*, size_t) = vits_model_get_speaker_embedding;\n'
                   '  int (*c)(vits_model*, const float*, int32_t, int32_t*) = vits_model_add_voices;\n'
                   '  int (*d)(vits_model*, int32_t, const float*) = vits_model_set_voice;\n'
                   '  int (*e)(vits_model*) = vits_model_clear_voices;\n'
                   '  int32_t (*f)(const vits_model*) = vits_model_num_voices;\n'
                   '  float g[4] = {0.f, 0.f, 0.f, 0.f}; int32_t id = 0;\n'
                   '  int refused = c(NULL, g, 1, &id) == -1 && d(NULL, 0, g) == -1 && e(NULL) == -1 && b(NULL, 0, g, 4) == -1 && a(NULL) == 0 && f(NULL) == 0;\n'
                   '  printf("%zu %d\\n", sizeof(vits_process_opts), refused); return 0; }\n')
    exe = tmp_path / "voices"
    lib_dir = os.path.join(ROOT, "vits.cpp_amd", "csrc")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", lib_dir, "-lvits_hip",
                    "-Wl,-rpath," + lib_dir], check=True)
    size, refused = map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert size == PROCESS_OPTS_SIZE == C.sizeof(pkg.ProcessOpts) and refused == 1


def test_null_handles_and_arguments_are_refused_without_a_device(pkg):
    lib = pkg.lib()
    g = np.zeros(8, np.float32)
    ids = np.zeros(2, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.vits_model_speaker_embedding_size(None) == 0
    assert lib.vits_model_num_voices(None) == 0
    for call in (lambda: lib.vits_model_add_voices(None, p(g), 1, p(ids)), lambda: lib.vits_model_add_voices(None, p(g), 0, p(ids)),
                 lambda: lib.vits_model_add_voices(None, None, 1, None), lambda: lib.vits_model_set_voice(None, 3, p(g)),
                 lambda: lib.vits_model_set_voice(None, 3, None), lambda: lib.vits_model_clear_voices(None),
                 lambda: lib.vits_model_get_speaker_embedding(None, 0, p(g), 8), lambda: lib.vits_model_get_speaker_embedding(None, 0, None, 8)):
        assert call() == -1
        assert "null" in pkg.last_error()


def test_documents_name_the_calls():
    for doc, word in (("INTEGRATION.md", "vits_model_add_voices"), ("DESIGN.md", "voice_rows_kernel"), ("README.md", "vits_model_add_voices"),
                      ("include/vits.h", "vits_model_clear_voices")):
        assert word in open(os.path.join(ROOT, doc)).read(), doc
