#!/usr/bin/env python3
"""Generates the fixtures of the deterministic duration predictor (use_stochastic_duration_prediction = False; transformers VitsDurationPredictor)
in tests/golden/. Runs ONLY in the build container (needs transformers and, for the exporter-written file, the reference tree's
scripts/export_vits.py); nothing here travels to the GPU box except the data files it writes. Helpers come from make_golden.py and
make_golden_speakers.py, which are unchanged.

Fixtures (data only):
  tiny_detdp_hf_export.ggml                 the tiny 3-speaker VitsConfig of make_golden_speakers.py with use_stochastic_duration_prediction=False,
                                            duration_predictor_filter_channels=32, written by the reference's own exporter: pins the real tensor names
                                            (duration_predictor.conv_1 / norm_1 / conv_2 / norm_2 / proj / cond) and the to_diff_dict config.
  tiny_detdp_hf_export[_refmode]_taps.npz   transformers taps for the speakers None (-1), 0, 2 on 14 ids; keys "s<speaker>_<tap>" (speaker -1 = "sm1").
  full_synth_detdp[_refmode]_taps.npz       the same for vits_synth_model_bytes(0x5EED, VITS_SYNTH_FULL | VITS_SYNTH_SPEAKERS | VITS_SYNTH_DETERMINISTIC),
                                            16 ids, speakers -1, 5, 77 (waveform decimated by 4).
Every npz also holds "<key>_log_duration_f64": the predictor re-evaluated in float64 on the same (fp32) encoder output. The generator ASSERTS that every
exp(logw) * length_scale of a fixture is at least 1e-3 away from an integer in both evaluations, so that "the durations equal transformers' exactly" is a
fair demand of an fp32 implementation with another summation order; ids seeds are picked until that holds.

usage: python tests/golden/make_golden_detdp.py REFERENCE_TREE   (from the repo root, after building csrc/libvits_hip.so)
"""
import contextlib
import copy
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402
import make_golden_speakers as S  # noqa: E402

MARGIN = 1e-3


class DetAdapter(torch.nn.Module):
    """VitsDurationPredictor behind the call make_golden.hf_taps makes for the stochastic predictor (reverse / noise_scale: no such thing here); records the
    float64 evaluation of the same call."""

    def __init__(self, dp):
        super().__init__()
        self.dp = dp
        self.dp64 = copy.deepcopy(dp).double()
        self.f64 = None

    def forward(self, inputs, padding_mask, global_conditioning=None, reverse=True, noise_scale=1.0):
        g = None if global_conditioning is None else global_conditioning.double()
        self.f64 = self.dp64(inputs.double(), padding_mask.double(), g)
        return self.dp(inputs, padding_mask, global_conditioning)


def margin(logw, length_scale=1.0):
    v = np.exp(np.asarray(logw, np.float64)) * length_scale
    return float(np.abs(v - np.round(v)).min())


def det_taps(parsed, T, seed, speakers, refmode=False, decimate=1):
    """S.speaker_taps for a deterministic model; None when some duration of the fixture sits within MARGIN of an integer"""
    model = G.hf_model_from_file(parsed)
    assert not model.config.use_stochastic_duration_prediction
    model.duration_predictor = DetAdapter(model.duration_predictor)
    ids = G.make_ids(T, model.config.vocab_size, seed)
    rng = np.random.default_rng(seed)
    nd = rng.standard_normal((2, T)).astype(np.float32)  # (never read: the adapter ignores the patched torch.randn)
    npr = rng.standard_normal((model.config.flow_size, 64 * T)).astype(np.float32)
    out = {}
    for s in speakers:
        with torch.no_grad(), (G.reference_mode_patches() if refmode else contextlib.nullcontext()):
            t = S.hf_taps_speaker(model, ids, nd, lambda L: npr[:, :L].copy(), s, refmode=refmode)
        key = "sm1" if s is None else "s%d" % s
        f64 = model.duration_predictor.f64[0].numpy()
        if min(margin(t["log_duration"]), margin(f64)) < MARGIN:
            return None
        for k in ("log_duration", "durations", "z_flow", "noise_prior"):
            out[key + "_" + k] = t[k]
        out[key + "_log_duration_f64"] = f64
        out[key + "_waveform_len"] = np.array([t["waveform"].size], np.int64)
        out[key + "_waveform"] = t["waveform"][..., ::decimate].copy()
        out["ids"] = t["ids"]
    out["decimate"] = np.array([decimate], np.int64)
    out["speakers"] = np.array([-1 if s is None else s for s in speakers], np.int32)
    out["ids_seed"] = np.array([seed], np.int64)
    return out


def reference_exported_tiny_detdp(reference_root):
    sys.path.insert(0, os.path.join(reference_root, "scripts"))
    import export_vits
    from transformers import VitsConfig, VitsModel
    torch.manual_seed(21)
    cfg = VitsConfig(vocab_size=38, hidden_size=16, num_hidden_layers=2, num_attention_heads=2, window_size=2, ffn_dim=32,
                     flow_size=16, spectrogram_bins=9, upsample_initial_channel=32, upsample_rates=[4, 2],
                     upsample_kernel_sizes=[8, 4], resblock_kernel_sizes=[3, 5], resblock_dilation_sizes=[[1, 3], [1, 2]],
                     depth_separable_num_layers=2, prior_encoder_num_flows=2, prior_encoder_num_wavenet_layers=2,
                     posterior_encoder_num_wavenet_layers=1, num_speakers=3, speaker_embedding_size=8,
                     use_stochastic_duration_prediction=False, duration_predictor_filter_channels=32)
    model = VitsModel(cfg).eval()
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.startswith("decoder.") and "weight" in n and "cond" not in n:
                p.mul_(0.6)
        # default init leaves log-durations and the speaker terms near zero: one to four frames per id, and speakers that move them
        model.duration_predictor.proj.bias.fill_(0.45)
        model.embed_speaker.weight.mul_(2.0)
        model.duration_predictor.cond.weight.mul_(3.0)
    model = export_vits.remove_weight_norm_and_convert_to_fp16(model)
    path = os.path.join(HERE, "tiny_detdp_hf_export.ggml")

    class Tok:
        phonemize = False
        is_uroman = False
        add_blank = True
        normalize = True
        pad_token = "<pad>"
        unk_token = "<unk>"

        def get_vocab(self):
            v = {"<pad>": 0, " ": 1, "'": 2, "-": 3}
            for i, c in enumerate("abcdefghijklmnopqrstuvwxyz"):
                v[c] = 4 + i
            for i, c in enumerate("0123456"):
                v[c] = 30 + i
            v["<unk>"] = 37
            return v

    with contextlib.redirect_stdout(io.StringIO()):
        export_vits.serialize_model_to_binary(model.config, model.state_dict(), Tok(), path)
    return open(path, "rb").read()


def fixture(parsed, T, speakers, first_seed, decimate=1):
    """both modes on the first ids seed whose durations all keep the margin"""
    for seed in range(first_seed, first_seed + 200):
        both = [det_taps(parsed, T, seed, speakers, refmode=r, decimate=decimate) for r in (False, True)]
        if all(b is not None for b in both):
            return both
    raise SystemExit("no ids seed keeps every duration %g away from an integer" % MARGIN)


def main():
    pkg = G.load_package()
    save = lambda name, d: np.savez_compressed(os.path.join(HERE, name), **d)
    data = reference_exported_tiny_detdp(sys.argv[1])
    pkg.validate(data)
    parsed = G.parse_model_file(data)
    assert "duration_predictor_filter_channels" in parsed["config"] and parsed["config"]["use_stochastic_duration_prediction"] == "False"
    print("tiny_detdp_hf_export.ggml", len(data), "bytes,", len(parsed["tensors"]), "tensors")
    for name, p, T, spk, seed, dec in (("tiny_detdp_hf_export", parsed, 14, (None, 0, 2), 31, 1),
                                       ("full_synth_detdp", G.parse_model_file(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_FULL | pkg.SYNTH_SPEAKERS | pkg.SYNTH_DETERMINISTIC)),
                                        16, (None, 5, 77), 41, 4)):
        for t, suffix in zip(fixture(p, T, spk, seed, dec), ("", "_refmode")):
            save("%s%s_taps.npz" % (name, suffix), t)
            keys = [k for k in sorted(t) if k.endswith("_log_duration")]
            print(name + suffix, "ids seed", int(t["ids_seed"][0]), "frames", [int(t[k[:-13] + "_durations"].sum()) for k in keys], "margin",
                  min(min(margin(t[k]), margin(t[k + "_f64"])) for k in keys), "max |fp32 - f64|", max(float(np.abs(t[k] - t[k + "_f64"]).max()) for k in keys))


if __name__ == "__main__":
    main()
