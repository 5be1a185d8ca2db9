"""Per-utterance prosody, host side: the C layout of the five vits_process_opts fields, the two model-level calls (declared, exported,
mirrored), and the transformers prosody fixtures (tests/golden/make_golden_prosody.py) pinned against the CPU oracle on model files whose
config holds each setting. No GPU needed. The file-rewriting helper is shared with tests/test_gpu_prosody.py."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden, rel_err

FIELDS = ["speaking_rates", "noise_scales", "noise_scale_durations", "duration_override", "durations_out"]
FIXTURES = [("tiny_hf_export_prosody_taps.npz", 1), ("tiny_hf_export_prosody_refmode_taps.npz", 0), ("full_synth_prosody_taps.npz", 1),
            ("full_synth_prosody_refmode_taps.npz", 0)]


# ---- model files with other prosody values in their config (the on-disk format of vits.cpp_amd/csrc/model_file.h) ----------------
def _config_span(data):
    """(offset of the config count, offset behind the last config entry) of a model file"""
    off = 0

    def u32():
        nonlocal off
        v = struct.unpack_from("<I", data, off)[0]
        off += 4
        return v

    def blob():
        nonlocal off
        n = u32()
        off += n

    for _ in range(u32()):  # vocabulary: (key, id)
        blob()
        u32()
    u32(), u32(), blob(), blob()  # tokenizer head
    start = off
    for _ in range(u32()):
        blob(), blob()
    return start, off


def _config(data):
    start, end = _config_span(data)
    out, off = [], start + 4

    def blob():
        nonlocal off
        n = struct.unpack_from("<I", data, off)[0]
        off += 4 + n
        return data[off - n:off]

    for _ in range(struct.unpack_from("<I", data, start)[0]):
        out.append((blob(), blob()))
    return out


def with_prosody(data, speaking_rate, noise_scale, noise_scale_duration):
    """The model file with its config's speaking_rate / noise_scale / noise_scale_duration replaced, written as "%.9g" of the float32 value,
    so that the file parser and a ctypes float hold the same number."""
    start, end = _config_span(data)
    new = {b"speaking_rate": speaking_rate, b"noise_scale": noise_scale, b"noise_scale_duration": noise_scale_duration}
    cfg = [(k, ("%.9g" % np.float32(new[k])).encode() if k in new else v) for k, v in _config(data)]
    for k in new:
        if k not in dict(cfg):
            cfg.append((k, ("%.9g" % np.float32(new[k])).encode()))
    body = bytearray(struct.pack("<I", len(cfg)))
    for k, v in cfg:
        body += struct.pack("<I", len(k)) + k + struct.pack("<I", len(v)) + v
    return data[:start] + bytes(body) + data[end:]


def fixture_bytes(pkg, name):
    if name.startswith("tiny_hf_export"):
        with open(os.path.join(GOLDEN, "tiny_hf_export.ggml"), "rb") as f:
            return f.read()
    return pkg.synth_model_bytes(0x5EED, pkg.SYNTH_FULL)


# ---- tests -------------------------------------------------------------------------------------------------------------------------
def test_process_opts_prosody_layout_matches_the_c_header(pkg, tmp_path):
    import ctypes as C
    src = tmp_path / "off.c"
    fmt = " ".join(["%zu"] * (len(FIELDS) + 1))
    args = ", ".join(["offsetof(vits_process_opts, %s)" % f for f in FIELDS] + ["sizeof(vits_process_opts)"])
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vits.h"\nint main(void) { printf("%s\\n", %s); return 0; }\n' % (fmt, args))
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert [getattr(pkg.ProcessOpts, f).offset for f in FIELDS] == got[:-1]
    assert C.sizeof(pkg.ProcessOpts) == got[-1]
    assert got[0] > pkg.ProcessOpts.speaker_ids.offset  # appended behind speaker_ids: older callers' struct_size leaves them NULL


def test_prosody_calls_are_declared_exported_and_mirrored(pkg):
    header = open(os.path.join(ROOT, "include", "vits.h")).read()
    lib = pkg.lib()
    for s in ("vits_model_set_prosody", "vits_model_get_prosody"):
        assert re.search(r"VITS_API int %s\(" % s, header), s
        assert s in pkg.EXPORTED_SYMBOLS and hasattr(lib, s)
    for prop in ("speaking_rate", "noise_scale", "noise_scale_duration"):
        assert isinstance(getattr(pkg.Model, prop), property) and getattr(pkg.Model, prop).fset is not None
    import inspect
    for fn in (pkg.Model.process_batch, pkg.Model.submit_batch):
        params = inspect.signature(fn).parameters
        for a in ("speaking_rate", "noise_scale", "noise_scale_duration", "duration_override", "durations_out"):
            assert a in params and params[a].default is None, (fn.__name__, a)


def test_with_prosody_rewrites_only_the_three_values(pkg, oracle, tiny_hf_bytes):
    data = with_prosody(tiny_hf_bytes, 1.7, 0.25, 0.0)
    m = oracle.Model(data)
    assert float(m.config("speaking_rate")) == np.float32(1.7) and m.config("speaking_rate") == "%.9g" % np.float32(1.7)
    assert float(m.config("noise_scale")) == 0.25 and float(m.config("noise_scale_duration")) == 0.0
    assert pkg.reserialize(data) == data
    pkg.validate(data)
    keys = (b"speaking_rate", b"noise_scale", b"noise_scale_duration")
    assert [kv for kv in _config(data) if kv[0] not in keys] == [kv for kv in _config(tiny_hf_bytes) if kv[0] not in keys]
    _, end = _config_span(data)
    assert data[end:] == tiny_hf_bytes[_config_span(tiny_hf_bytes)[1]:]  # the tensors, untouched


def test_prosody_fixtures_cover_the_settings():
    for name, _ in FIXTURES:
        g = golden(name)
        s = g["settings"]
        assert s.shape == (4, 3) and s.dtype == np.float32
        assert set(s[:, 0].tolist()) == {np.float32(0.6), np.float32(1.7)} and set(s[:, 1].tolist()) == {0.0, 1.0}
        assert set(s[:, 2].tolist()) == {0.0, np.float32(1.2)}
        frames = [int(g["p%d_durations" % i].sum()) for i in range(4)]
        # the rate really stretches: each slow setting is longer than the fast setting with the same duration noise scale
        for i in range(4):
            for j in range(4):
                if s[i, 0] < s[j, 0] and s[i, 2] == s[j, 2]:
                    assert frames[i] > frames[j], (name, frames)


@pytest.mark.parametrize("fixture,mode", FIXTURES)
def test_oracle_on_rewritten_files_reproduces_the_prosody_fixtures(pkg, oracle, fixture, mode):
    """The oracle reads the three values from the model file: on a file rewritten with each setting it reproduces transformers with the
    attributes set (durations exact, floats within the speaker fixtures' 2e-4 of RMS)."""
    g = golden(fixture)
    dec = int(g["decimate"][0])
    base = fixture_bytes(pkg, fixture)
    for i, (rate, ns, nsd) in enumerate(g["settings"].tolist()):
        k = "p%d_" % i
        m = oracle.Model(with_prosody(base, rate, ns, nsd))
        r = m.process_ids(g["ids"], mode=mode, noise_kind=oracle.NOISE_EXPLICIT, noise_dur=g["noise_dur"], noise_prior=g["noise_prior"])
        np.testing.assert_array_equal(r["durations"], g[k + "durations"].ravel(), err_msg=k)
        assert rel_err(r["log_duration"], g[k + "log_duration"]) < 2e-4, k
        assert rel_err(r["z_flow"], g[k + "z_flow"]) < 2e-4, k
        assert r["waveform"].size == int(g[k + "waveform_len"][0]), k
        assert rel_err(r["waveform"][::dec], g[k + "waveform"]) < 2e-4, k
        m.close()
