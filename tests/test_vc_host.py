"""Voice conversion, host side: the VITS_SYNTH_POSTERIOR synthetic files, files made without the flag unchanged, the fixtures' spectrogram
reproduced by numpy alone, and the new entry points of the C ABI and its ctypes mirror."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden
from modelfile_py import parse_model_file
from spectrogram_ref import np_spectrogram  # (the float64 reference of the spectrogram operator tests: the fixture comparison below checks it on the CPU)

# sha256 of vits_synth_model_bytes(0x5EED, arch) on the commit before voice conversion: the flag only appends
PARENT_SHA256 = {
    0x000: "20369f3f44526609265804e3a3645649f21ab08ba2ce048eb84f29ad4873891f",
    0x001: "6d18e7ba44e9e8ca4ab429bd041196e7473c6a0a158b64b9faf0680499540b25",
    0x200: "2cba771e040f8df984a817b359eb9d8fe3254471763d89bf79e758eb6ca56ac1",
    0x201: "d7fb80096020698bf60cd935735f7cad391aae2ea4b57b20cce388c8cdd3690d",
    0x101: "c150750c963eade3dab189794b48a54bc84195f99263be47cf06432e5d3fe700",
}


@pytest.mark.parametrize("arch", sorted(PARENT_SHA256))
def test_files_without_the_posterior_flag_are_unchanged(pkg, arch):
    assert hashlib.sha256(pkg.synth_model_bytes(0x5EED, arch)).hexdigest() == PARENT_SHA256[arch]


def posterior_shapes(H, F, bins, k, nl, E):
    want = {"posterior_encoder.conv_pre.weight": (H, bins, 1), "posterior_encoder.conv_pre.bias": (H,),
            "posterior_encoder.conv_proj.weight": (2 * F, H, 1), "posterior_encoder.conv_proj.bias": (2 * F,)}
    for l in range(nl):
        want["posterior_encoder.wavenet.in_layers.%d.weight" % l] = (2 * H, H, k)
        want["posterior_encoder.wavenet.in_layers.%d.bias" % l] = (2 * H,)
        co = 2 * H if l + 1 < nl else H
        want["posterior_encoder.wavenet.res_skip_layers.%d.weight" % l] = (co, H, 1)
        want["posterior_encoder.wavenet.res_skip_layers.%d.bias" % l] = (co,)
    if E:
        want["posterior_encoder.wavenet.cond_layer.weight"] = (2 * H * nl, E, 1)
        want["posterior_encoder.wavenet.cond_layer.bias"] = (2 * H * nl,)
    return want


@pytest.mark.parametrize("arch,H,F,bins,nl,E", [(1, 16, 16, 9, 2, 0), (0x201, 16, 16, 9, 2, 8), (0x200, 192, 192, 513, 16, 256)])
def test_posterior_flag_appends_the_transformers_tensors(pkg, arch, H, F, bins, nl, E):
    base = pkg.synth_model_bytes(0x5EED, arch)
    data = pkg.synth_model_bytes(0x5EED, arch | pkg.SYNTH_POSTERIOR)
    pkg.validate(data)  # raises on a rejected file
    p, q = parse_model_file(base), parse_model_file(data)
    names_b, names_p = list(p["tensors"]), list(q["tensors"])
    assert names_p[:len(names_b)] == names_b  # every existing tensor first, in order ...
    for n in names_b:
        np.testing.assert_array_equal(p["tensors"][n][0], q["tensors"][n][0])  # ... with the same values
    added = {n: tuple(q["tensors"][n][0].shape) for n in names_p[len(names_b):]}
    assert added == posterior_shapes(H, F, bins, 5, nl, E)
    assert q["config"]["spectrogram_bins"] == str(bins) and q["config"]["posterior_encoder_num_wavenet_layers"] == str(nl)


@pytest.mark.parametrize("fixture,n_fft,hop", [("vc_tiny_speakers_hf_export_taps.npz", 16, 8), ("vc_full_synth_taps.npz", 1024, 256)])
def test_numpy_spectrogram_reproduces_the_fixture(fixture, n_fft, hop):
    g = golden(fixture)
    seen = 0
    for i, s, t in g["pairs"].tolist():
        k = "p%s_%s_u%d_spec" % ("m1" if s < 0 else s, "m1" if t < 0 else t, i)
        y = g["pcm%d" % i]
        want = np_spectrogram(y, n_fft, hop)
        assert want.shape == g[k].shape == (n_fft // 2 + 1, y.size // hop)
        rms = np.sqrt((want ** 2).mean())
        assert np.abs(g[k] - want).max() / rms < 1e-5, k
        seen += 1
    assert seen >= 2


def test_fixture_inputs_cover_the_minimum_length_and_ragged_lengths():
    g = golden("vc_tiny_speakers_hf_export_taps.npz")
    lens = [g["pcm%d" % i].size for i in range(3)]
    assert min(lens) == 8  # max(hop, pad + 1) for hop 8, pad 4
    assert any(n % 8 for n in lens)
    assert all(np.abs(g["pcm%d" % i]).max() <= 0.9 + 1e-6 for i in range(3))


def test_conversion_symbols_are_declared_exported_and_typed(pkg):
    header = open(os.path.join(ROOT, "include", "vits.h")).read()
    L = pkg.lib()
    for name in ("vits_model_prepare_conversion", "vits_model_convert_batch", "vits_model_convert"):
        assert name in pkg.EXPORTED_SYMBOLS and name + "(" in header and hasattr(L, name)
    assert L.vits_model_convert_batch.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                                                   C.POINTER(pkg.ProcessOpts), C.POINTER(pkg.BatchResult)]
    assert L.vits_model_convert_batch.restype == C.c_int32
    assert L.vits_model_convert.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_int32]
    assert L.vits_model_convert.restype is pkg.VitsResult
    assert L.vits_model_prepare_conversion.argtypes == [C.c_void_p] and L.vits_model_prepare_conversion.restype == C.c_int32
    assert pkg.SYNTH_POSTERIOR == 0x400 and "#define VITS_SYNTH_POSTERIOR 0x400" in header


def test_conversion_entry_points_refuse_null_handles(pkg):
    L = pkg.lib()
    assert L.vits_model_prepare_conversion(None) == -1
    pcm = np.zeros(64, np.float32)
    lens = np.array([64], np.int64)
    assert L.vits_model_convert_batch(None, pcm.ctypes.data, lens.ctypes.data, 1, 64, None, None, None, None) == -1
    r = L.vits_model_convert(None, pcm.ctypes.data, 64, -1, -1)
    assert not r.data and r.size == 0


def test_odd_flow_fixture_file_has_three_coupling_layers():
    with open(os.path.join(GOLDEN, "vc_tiny_flows3.ggml"), "rb") as f:
        q = parse_model_file(f.read())
    assert q["config"]["prior_encoder_num_flows"] == "3" and q["config"]["posterior_encoder_num_wavenet_layers"] == "3"
    assert "posterior_encoder.wavenet.res_skip_layers.2.weight" in q["tensors"]
