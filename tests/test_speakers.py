"""Multi-speaker model files (speaker conditioning), host side: what vits_model_file_validate accepts and refuses, the byte-exact
round trip, the synthetic speaker models and the C layout of vits_process_opts.speaker_ids. No GPU needed."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

EXPORT = os.path.join(GOLDEN, "tiny_speakers_hf_export.ggml")


# ---- a minimal reader / writer of the on-disk format (vits.cpp_amd/csrc/model_file.h), payloads kept as stored ------------------
def read_file(data):
    off = 0

    def u32():
        nonlocal off
        v = struct.unpack_from("<I", data, off)[0]
        off += 4
        return v

    def blob():
        nonlocal off
        n = u32()
        b = data[off:off + n]
        off += n
        return b

    vocab = [(blob(), u32()) for _ in range(u32())]
    head = [u32(), u32(), blob(), blob()]
    cfg = [(blob(), blob()) for _ in range(u32())]
    tensors = []
    for _ in range(u32()):
        name, dtype, rank = blob(), u32(), u32()
        dims = [u32() for _ in range(rank)]
        tensors.append([name.decode(), dtype, dims, blob()])
    assert off == len(data)
    return vocab, head, cfg, tensors


def write_file(vocab, head, cfg, tensors):
    out = bytearray()
    u32 = lambda v: out.extend(struct.pack("<I", v))

    def blob(b):
        u32(len(b))
        out.extend(b)

    u32(len(vocab))
    for k, i in vocab:
        blob(k)
        u32(i)
    u32(head[0])
    u32(head[1])
    blob(head[2])
    blob(head[3])
    u32(len(cfg))
    for k, v in cfg:
        blob(k)
        blob(v)
    u32(len(tensors))
    for name, dtype, dims, payload in tensors:
        blob(name.encode())
        u32(dtype)
        u32(len(dims))
        for d in dims:
            u32(d)
        blob(payload)
    return bytes(out)


def refusal(pkg, data):
    try:
        pkg.validate(data)
    except pkg.VitsError as e:
        return str(e)
    return None


@pytest.fixture(scope="module")
def export_bytes():
    with open(EXPORT, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def synth_speakers(pkg):
    return {a: pkg.synth_model_bytes(0x5EED, a | pkg.SYNTH_SPEAKERS) for a in (pkg.SYNTH_TINY, pkg.SYNTH_FULL)}


def test_validate_accepts_the_exported_and_the_synthetic_speaker_models(pkg, export_bytes, synth_speakers):
    pkg.validate(export_bytes)
    for data in synth_speakers.values():
        pkg.validate(data)


def test_exported_file_has_the_transformers_speaker_tensors(export_bytes):
    _, _, cfg, tensors = read_file(export_bytes)
    cfg = {k.decode(): v.decode() for k, v in cfg}
    assert cfg["num_speakers"] == "3" and cfg["speaker_embedding_size"] == "8"
    shapes = {n: d for n, _, d, _ in tensors}
    assert shapes["embed_speaker.weight"] == [8, 3]
    assert shapes["duration_predictor.cond.weight"] == [1, 8, 16]
    assert shapes["decoder.cond.weight"] == [1, 8, 32]
    for i in range(2):
        assert shapes["flow.flows.%d.wavenet.cond_layer.weight" % i] == [1, 8, 2 * 16 * 2]
        assert shapes["flow.flows.%d.wavenet.cond_layer.bias" % i] == [2 * 16 * 2]


def test_synthetic_speaker_model_extends_the_single_speaker_one(pkg, synth_speakers):
    """VITS_SYNTH_SPEAKERS: the tensors of the model without the flag, byte for byte, then the speaker tensors."""
    base = read_file(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_TINY))[3]
    spk = read_file(synth_speakers[pkg.SYNTH_TINY])[3]
    assert spk[:len(base)] == base
    assert [t[0] for t in spk[len(base):]] == ["embed_speaker.weight", "duration_predictor.cond.weight", "duration_predictor.cond.bias"] + \
        ["flow.flows.%d.wavenet.cond_layer.%s" % (i, w) for i in range(2) for w in ("weight", "bias")] + ["decoder.cond.weight", "decoder.cond.bias"]
    _, _, cfg, tensors = read_file(synth_speakers[pkg.SYNTH_FULL])
    cfg = {k.decode(): v.decode() for k, v in cfg}
    assert cfg["num_speakers"] == "109" and cfg["speaker_embedding_size"] == "256"
    assert {n: d for n, _, d, _ in tensors}["embed_speaker.weight"] == [256, 109]


COND = ["embed_speaker.weight", "duration_predictor.cond.weight", "duration_predictor.cond.bias", "flow.flows.0.wavenet.cond_layer.weight",
        "flow.flows.1.wavenet.cond_layer.bias", "decoder.cond.weight", "decoder.cond.bias"]


@pytest.mark.parametrize("name", COND)
def test_missing_speaker_tensor_is_named(pkg, export_bytes, name):
    v, h, c, t = read_file(export_bytes)
    msg = refusal(pkg, write_file(v, h, c, [x for x in t if x[0] != name]))
    assert msg is not None and name in msg, msg


@pytest.mark.parametrize("name", COND)
def test_misshapen_speaker_tensor_is_named(pkg, export_bytes, name):
    v, h, c, t = read_file(export_bytes)
    t2 = []
    for n, dtype, dims, payload in t:
        if n == name:  # one row fewer in the slowest dimension
            row = len(payload) // dims[-1]
            dims, payload = dims[:-1] + [dims[-1] - 1], payload[:len(payload) - row]
        t2.append([n, dtype, dims, payload])
    msg = refusal(pkg, write_file(v, h, c, t2))
    assert msg is not None and name in msg, msg


def test_speaker_embedding_size_zero_with_several_speakers_is_refused(pkg, export_bytes):
    v, h, c, t = read_file(export_bytes)
    c = [(k, b"0" if k == b"speaker_embedding_size" else val) for k, val in c]
    msg = refusal(pkg, write_file(v, h, c, t))
    assert msg is not None and "speaker" in msg, msg


def test_one_speaker_with_an_embedding_size_loads(pkg, export_bytes):
    """transformers: num_speakers == 1 has no embed_speaker (and its cond layers are never used) — such a file loads as single-speaker."""
    v, h, c, t = read_file(export_bytes)
    c = [(k, b"1" if k == b"num_speakers" else val) for k, val in c]
    pkg.validate(write_file(v, h, c, [x for x in t if x[0] != "embed_speaker.weight"]))


def test_deterministic_duration_predictor_stays_refused(pkg, export_bytes):
    v, h, c, t = read_file(export_bytes)
    c = [(k, b"False" if k == b"use_stochastic_duration_prediction" else val) for k, val in c]
    assert refusal(pkg, write_file(v, h, c, t)) is not None


def test_reserialize_is_byte_exact(pkg, export_bytes, synth_speakers):
    assert write_file(*read_file(export_bytes)) == export_bytes
    for data in [export_bytes] + list(synth_speakers.values()):
        assert pkg.reserialize(data) == data


def test_process_opts_layout_matches_the_c_header(pkg, tmp_path):
    import ctypes as C
    src = tmp_path / "off.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vits.h"\nint main(void) { printf("%zu %zu\\n", '
                   "offsetof(vits_process_opts, speaker_ids), sizeof(vits_process_opts)); return 0; }\n")
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    off, size = map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert pkg.ProcessOpts.speaker_ids.offset == off
    assert C.sizeof(pkg.ProcessOpts) == size


def test_python_mirror(pkg):
    assert pkg.SYNTH_SPEAKERS == 0x200
    lib = pkg.lib()
    for s in ("vits_model_set_speaker", "vits_model_get_speaker", "vits_model_num_speakers"):
        assert s in pkg.EXPORTED_SYMBOLS and hasattr(lib, s)
    assert np.int32(pkg.ProcessOpts.speaker_ids.offset) > pkg.ProcessOpts.noise_seed_offsets.offset
