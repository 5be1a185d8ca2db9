"""Full-size drill of the model-file path against the REFERENCE'S OWN exporter (CPU): what scripts/export_vits.py:5-93 of the
reference writes for a default-config transformers.VitsModel (the MMS-TTS architecture, 36.3 M parameters) is recorded in
tests/golden/fullsize_export_manifest.json (tests/golden/make_golden.py --fullsize-manifest): the bytes in front of the tensors, every
tensor's name, dtype and shape in file order with the mean / standard deviation of its values, the size of the exported file and of the
checkpoint the reference ships as an LFS pointer (scripts/vits-english.ggml: 74,551,853 B; the difference is the tokenizer's vocabulary
strings). From that record the test rebuilds a file of the same layout — header bytes verbatim, each tensor's values drawn from its
recorded mean and deviation with a fixed seed — and that file (698 tensors, within the 80 bytes of the shipped checkpoint) passes the
product's host-only load check (vits_model_file_validate == everything Engine::load checks: format, hyper-parameters, every tensor the
engine asks for with its shape and dtype), survives the product's reader / writer byte for byte, and loads and runs in the oracle. The
tiny exporter-written fixture tests/golden/tiny_hf_export.ggml covers the GPU side. VERDICT r4 next 8."""
import base64
import json
import os
import struct

import numpy as np
import pytest

MANIFEST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fullsize_export_manifest.json")


@pytest.fixture(scope="module")
def manifest():
    with open(MANIFEST) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def exported(manifest):
    rng = np.random.default_rng(3)
    parts = [base64.b64decode(manifest["header_base64"]), struct.pack("<I", len(manifest["tensors"]))]
    for name, dt, ne, mean, std in manifest["tensors"]:
        n = int(np.prod(ne))
        vals = (mean + std * rng.standard_normal(n)).astype(np.float32 if dt == 0 else np.float16)
        raw = vals.tobytes()
        parts += [struct.pack("<I", len(name)), name.encode(), struct.pack("<II", dt, len(ne)), struct.pack("<%dI" % len(ne), *ne),
                  struct.pack("<I", len(raw)), raw]
    data = b"".join(parts)
    assert len(data) == manifest["export_bytes"]
    return data


def test_default_config_export_matches_the_shipped_checkpoints_size_and_manifest(manifest, exported):
    from modelfile_py import parse_model_file
    shipped = manifest["shipped_checkpoint_bytes"]
    assert shipped == 74551853
    assert abs(len(exported) - shipped) <= 80, (len(exported), shipped)
    f = parse_model_file(exported)
    t = f["tensors"]
    assert len(t) == 698
    groups = {}
    for name in t:
        groups[name.split(".")[0]] = groups.get(name.split(".")[0], 0) + 1
    assert groups == {"duration_predictor": 284, "decoder": 155, "text_encoder": 111, "flow": 80, "posterior_encoder": 68}
    # spot checks of App. C's examples: ggml ne = reversed torch shape; conv weights fp16 (type 1), the rest fp32
    w, dt = t["flow.flows.0.wavenet.in_layers.0.weight"]
    assert w.shape == (384, 192, 5) and dt == 1
    w, dt = t["decoder.upsampler.0.weight"]
    assert w.shape == (512, 256, 16) and dt == 1
    w, dt = t["text_encoder.encoder.layers.0.attention.emb_rel_k"]
    assert w.shape == (1, 9, 96) and dt == 0
    w, dt = t["duration_predictor.flows.0.log_scale"]
    assert w.shape == (2, 1) and dt == 0
    assert f["config"]["upsample_rates"] == "[8, 8, 2, 2]" and f["config"]["use_stochastic_duration_prediction"] == "True"
    assert len(f["vocab"]) == 38 and f["add_blank"] == 1


def test_product_reader_accepts_and_round_trips_the_full_size_export(pkg, exported):
    # host-only: no device is touched (Engine::validate runs load()'s checks in dry-run mode)
    pkg.validate(exported)
    assert pkg.reserialize(exported) == exported
    # and a file with one engine-side tensor renamed is rejected by name
    bad = exported.replace(b"decoder.resblocks.11.convs2.2.weight", b"decoder.resblocks.11.convs2.2.weighx")
    assert bad != exported
    with pytest.raises(pkg.VitsError, match="decoder.resblocks.11.convs2.2.weight"):
        pkg.validate(bad)
    ids = pkg.file_tokenize(exported, "Hello world")
    assert ids.size == 2 * 11 + 1 and (ids[::2] == 0).all()  # blanks interspersed (src/vits_tokenizer.cpp:200-208)


def test_oracle_loads_and_runs_the_full_size_export(exported):
    import oracle_lib as O
    om = O.Model(exported)
    ids = np.array([0, 9, 0, 17, 0], np.int32)
    r = om.process_ids(ids, mode=O.MODE_REFERENCE, noise_kind=O.NOISE_COUNTER, noise_seed=1, threads=4, taps=["waveform", "durations"])
    assert r["durations"].size == 5 and (r["durations"] >= 1).all()
    assert r["waveform"].size == 256 * int(r["durations"].sum()) + 294 and np.isfinite(r["waveform"]).all()  # Q1: no crop in reference mode
