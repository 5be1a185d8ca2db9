"""Model files with the deterministic duration predictor (use_stochastic_duration_prediction = False), host side: what vits_model_file_validate accepts
and refuses, the synthetic VITS_SYNTH_DETERMINISTIC models, the byte-exact round trip, the Python mirror of the new ABI, and the frozen launch policy of the
fused kernel (tests/dp_det_plan_dump.cpp against tests/golden/dp_det_plan_table.txt). No GPU needed."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_speakers import read_file, refusal, write_file

CSRC = os.path.join(ROOT, "vits.cpp_amd", "csrc")
TABLE = os.path.join(GOLDEN, "dp_det_plan_table.txt")
DP = "duration_predictor."
DET_TENSORS = [DP + n for n in ("conv_1.weight", "conv_1.bias", "norm_1.weight", "norm_1.bias", "conv_2.weight", "conv_2.bias", "norm_2.weight", "norm_2.bias",
                                "proj.weight", "proj.bias")]


@pytest.fixture(scope="module")
def export_bytes():
    with open(os.path.join(GOLDEN, "tiny_detdp_hf_export.ggml"), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def tiny_det(pkg):
    return pkg.synth_model_bytes(0x5EED, pkg.SYNTH_TINY | pkg.SYNTH_SPEAKERS | pkg.SYNTH_DETERMINISTIC)


def flags(pkg):
    """every subset of {SPEAKERS, POSTERIOR, BF16} on both architectures: the sixteen models VITS_SYNTH_DETERMINISTIC combines with"""
    for arch in (pkg.SYNTH_TINY, pkg.SYNTH_FULL):
        for bits in range(8):
            yield arch | (pkg.SYNTH_SPEAKERS if bits & 1 else 0) | (pkg.SYNTH_POSTERIOR if bits & 2 else 0) | (pkg.SYNTH_BF16 if bits & 4 else 0)


def test_validate_accepts_every_flag_combination_and_the_exporter_file(pkg, export_bytes):
    pkg.validate(export_bytes)
    n = 0
    for f in flags(pkg):
        data = pkg.synth_model_bytes(0x5EED, f | pkg.SYNTH_DETERMINISTIC)
        pkg.validate(data)
        assert pkg.reserialize(data) == data
        n += 1
    assert n == 16
    assert pkg.reserialize(export_bytes) == export_bytes and write_file(*read_file(export_bytes)) == export_bytes


def test_the_flag_replaces_the_predictor_and_nothing_else(pkg):
    for f in flags(pkg):
        fc = b"32" if f & 0xFF == pkg.SYNTH_TINY else None  # (FULL: 256, and then the key is not written)
        _, head0, cfg0, t0 = read_file(pkg.synth_model_bytes(0x5EED, f))
        _, head1, cfg1, t1 = read_file(pkg.synth_model_bytes(0x5EED, f | pkg.SYNTH_DETERMINISTIC))
        keep = lambda t: [x for x in t if not x[0].startswith(DP) or x[0].startswith(DP + "cond.")]
        assert keep(t0) == keep(t1), hex(f)  # same tensors, same order, same bytes
        first = [i for i, x in enumerate(t0) if x[0].startswith(DP)][0]
        assert [x[0] for x in t1[first:first + len(DET_TENSORS)]] == DET_TENSORS  # in the stochastic predictor's place, state_dict order
        assert not any(x[0].startswith(DP + "flows.") or x[0].startswith(DP + "conv_dds.") for x in t1)
        c0, c1 = dict(cfg0), dict(cfg1)
        assert c1[b"use_stochastic_duration_prediction"] == b"False" and c1.pop(b"duration_predictor_filter_channels", None) == fc
        c1[b"use_stochastic_duration_prediction"] = b"True"
        assert c0 == c1 and head0 == head1
    # FULL: 256 filter channels, and the key is not written (the exporter writes config.to_diff_dict())
    _, _, cfg, t = read_file(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_FULL | pkg.SYNTH_DETERMINISTIC))
    assert b"duration_predictor_filter_channels" not in dict(cfg)
    assert {n: d for n, _, d, _ in t}[DP + "conv_1.weight"] == [3, 192, 256]


def test_a_file_without_the_flag_is_byte_identical_to_the_one_before_the_feature(pkg):
    """sha256 of vits_synth_model_bytes(0x5EED, VITS_SYNTH_FULL), recorded from the commit before VITS_SYNTH_DETERMINISTIC existed"""
    data = pkg.synth_model_bytes(0x5EED, pkg.SYNTH_FULL)
    assert hashlib.sha256(data).hexdigest() == "20369f3f44526609265804e3a3645649f21ab08ba2ce048eb84f29ad4873891f"


def test_synthetic_tensor_names_are_the_exporters(pkg, export_bytes, tiny_det):
    """the synthetic deterministic file names the tensors the reference's exporter writes for such a VitsConfig (sizes apart; the synthetic file leaves out what
    inference never reads: the posterior encoder of a TTS-only file)"""
    real = {n: len(d) for n, _, d, _ in read_file(export_bytes)[3] if not n.startswith("posterior_encoder.")}
    synth = {n: len(d) for n, _, d, _ in read_file(tiny_det)[3]}
    assert set(synth) == set(real), (sorted(set(synth) ^ set(real)))
    assert synth == real  # the same ranks
    cfg = dict(read_file(export_bytes)[2])
    assert cfg[b"use_stochastic_duration_prediction"] == b"False" and cfg[b"duration_predictor_filter_channels"] == b"32"


def edit(data, tensors=None, config=None):
    v, h, c, t = read_file(data)
    if config:
        c = config(c)
    if tensors:
        t = tensors(t)
    return write_file(v, h, c, t)


def test_missing_and_misshapen_tensors_are_named(pkg, export_bytes, tiny_det):
    for data in (export_bytes, tiny_det):
        for name in DET_TENSORS:
            msg = refusal(pkg, edit(data, tensors=lambda t: [x for x in t if x[0] != name]))
            assert msg is not None and name in msg, (name, msg)
        msg = refusal(pkg, edit(data, tensors=lambda t: [x for x in t if x[0] != DP + "norm_2.bias"]))
        assert DP + "norm_2.bias" in msg

        def narrower(t, name=DP + "conv_2.weight"):  # one output channel fewer
            out = []
            for n, dtype, dims, payload in t:
                if n == name:
                    row = len(payload) // dims[-1]
                    dims, payload = dims[:-1] + [dims[-1] - 1], payload[:len(payload) - row]
                out.append([n, dtype, dims, payload])
            return out
        msg = refusal(pkg, edit(data, tensors=narrower))
        assert msg is not None and DP + "conv_2.weight" in msg, msg
        for name in (DP + "norm_1.weight", DP + "conv_1.bias"):
            msg = refusal(pkg, edit(data, tensors=lambda t: narrower(t, name)))
            assert msg is not None and name in msg, (name, msg)


def test_the_filter_channels_key_must_agree_with_the_shape(pkg, export_bytes, tiny_det):
    for data in (export_bytes, tiny_det):
        # the key says 64, the tensors 32
        msg = refusal(pkg, edit(data, config=lambda c: [(k, b"64" if k == b"duration_predictor_filter_channels" else v) for k, v in c]))
        assert msg is not None and "duration_predictor_filter_channels" in msg and "conv_1.weight" in msg, msg
        # the key is absent: 256 by default, the tensors say 32
        msg = refusal(pkg, edit(data, config=lambda c: [(k, v) for k, v in c if k != b"duration_predictor_filter_channels"]))
        assert msg is not None and "256" in msg and "conv_1.weight" in msg, msg


def test_false_on_a_stochastic_file_names_the_first_missing_tensor(pkg):
    with open(os.path.join(GOLDEN, "tiny_speakers_hf_export.ggml"), "rb") as f:
        data = f.read()
    msg = refusal(pkg, edit(data, config=lambda c: [(k, b"False" if k == b"use_stochastic_duration_prediction" else v) for k, v in c]))
    assert msg is not None and DP + "conv_1.weight" in msg, msg


def test_the_stochastic_tensors_are_not_needed(pkg, tiny_det):
    """a deterministic file loads without a single stochastic-predictor tensor (the synthetic one has none), and True on it is refused"""
    assert not any(n.startswith(DP + "flows.") for n, *_ in read_file(tiny_det)[3])
    msg = refusal(pkg, edit(tiny_det, config=lambda c: [(k, b"True" if k == b"use_stochastic_duration_prediction" else v) for k, v in c]))
    assert msg is not None and DP in msg


def test_python_mirror(pkg, tmp_path):
    import ctypes as C
    assert pkg.SYNTH_DETERMINISTIC == 0x800
    lib = pkg.lib()
    for s in ("vits_model_duration_predictor_kind", "vits_op_duration_predictor"):
        assert s in pkg.EXPORTED_SYMBOLS and hasattr(lib, s)
    fields = [n for n, _ in pkg.DurationPredictorDesc._fields_]
    src = tmp_path / "off.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vits.h"\nint main(void) { printf("%d %zu", VITS_SYNTH_DETERMINISTIC, sizeof(vits_duration_predictor_desc)); '
                   + " ".join('printf(" %%zu", offsetof(vits_duration_predictor_desc, %s));' % n for n in fields) + ' printf("\\n"); return 0; }\n')
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    flag, size, *offs = map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert flag == pkg.SYNTH_DETERMINISTIC and size == C.sizeof(pkg.DurationPredictorDesc)
    assert offs == [getattr(pkg.DurationPredictorDesc, n).offset for n in fields]
    assert fields == ["batch", "hidden", "filter", "t", "t_stride", "k", "eps", "variant"]


# ---- the launch policy of dp_det_kernel, frozen ---------------------------------------------------------------------------------------------------
def test_plan_table_is_the_recorded_one():
    subprocess.check_call(["make", "-s", "-C", CSRC, "dp_det_plan_dump"])
    out = subprocess.run([os.path.join(CSRC, "dp_det_plan_dump")], check=True, capture_output=True).stdout  # (non-zero: a plan without an instantiation)
    want = open(TABLE, "rb").read()
    if out != want:
        a, b = out.decode().splitlines(), want.decode().splitlines()
        diff = [(i + 1, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y][:10]
        raise AssertionError("dp_det_plan_dump differs from the golden table (%d lines against %d); first differing lines (got, want):\n%s"
                             % (len(a), len(b), "\n".join("%d: %s\n   %s" % d for d in diff)))


def test_the_table_covers_the_policy():
    rows, knobs = [], None
    for line in open(TABLE).read().splitlines():
        if line.startswith("## "):
            knobs = line[3:]
        elif not line.startswith("#"):
            key, fields = line.split(" : ", 1)
            rows.append((knobs, tuple(int(x) for x in key.split()[1:]), fields))
    sets = sorted({kn for kn, *_ in rows})
    assert sets == sorted(["default", "no_dp_det_fuse", "dp_det_lat_max_blocks=8", "dp_det_lat_max_blocks=0"])  # every knob set moves a case
    default = {case: f for kn, case, f in rows if kn == "default"}
    kernels = set(re.findall(r"dp_det_kernel<[^>]*>", "\n".join(default.values())))
    assert kernels == {"dp_det_kernel<6, 256, 3, 16>", "dp_det_kernel<6, 256, 3, 62>", "dp_det_kernel<6, 256, 5, 16>", "dp_det_kernel<6, 256, 5, 60>",
                       "dp_det_kernel<1, 32, 3, 16>", "dp_det_kernel<1, 32, 3, 62>"}
    tile = lambda f: f.split(">")[0].split(", ")[-1]
    # the threshold from both sides: 96 / 97 blocks of 16 tokens, as one utterance and as six
    assert tile(default[(192, 256, 3, 0, 1536, 1)]) == "16" and tile(default[(192, 256, 3, 0, 1537, 1)]) == "62"
    assert tile(default[(192, 256, 3, 0, 256, 6)]) == "16" and tile(default[(192, 256, 3, 0, 257, 6)]) == "62"
    # the forced tiles, the un-fused variant, the refused shapes
    assert tile(default[(192, 256, 3, 1, 128, 64)]) == "16" and tile(default[(192, 256, 3, 2, 1, 1)]) == "62"
    assert all(f == "unfused" for case, f in default.items() if case[3] == 3)
    for shape in ((128, 256, 3), (192, 192, 3), (192, 256, 7), (16, 32, 5), (192, 256, 2)):
        assert default[shape + (0, 128, 1)] == "unfused" and default[shape + (1, 128, 1)] == "refused" and default[shape + (2, 128, 1)] == "refused"
    # the knobs
    moved = {kn: {case: f for k2, case, f in rows if k2 == kn} for kn in sets if kn != "default"}
    assert all(f == "unfused" for f in moved["no_dp_det_fuse"].values()) and all(case[3] == 0 for case in moved["no_dp_det_fuse"])
    assert tile(moved["dp_det_lat_max_blocks=8"][(192, 256, 3, 0, 129, 1)]) == "62" and (192, 256, 3, 0, 128, 1) not in moved["dp_det_lat_max_blocks=8"]
    assert tile(moved["dp_det_lat_max_blocks=0"][(192, 256, 3, 0, 1, 1)]) == "62"
    # LDS within the CU's 160 KB and the geometry's block = one wave per 16 filter channels
    for f in default.values():
        if f.startswith("fused"):
            gx, gy, gz, block, lds = map(int, f.split(" | ")[1].split())
            fc = int(f.split("<")[1].split(", ")[1])
            assert lds <= 160 * 1024 and block == fc // 16 * 64 and gz == 1
