#!/usr/bin/env python3
"""Generates the prosody fixtures in tests/golden/ (per-utterance speaking rate and noise scales: transformers VitsModel.speaking_rate,
noise_scale, noise_scale_duration). Runs ONLY in the build container (needs transformers); nothing here travels to the GPU box except the
data files it writes. Helpers come from make_golden.py, which is unchanged: hf_taps already reads the three attributes, this script only
sets them (to float32 values, so that the model file's "%.9g" text, the library's float and torch's scalar agree).

Fixtures (data only), for SETTINGS[i] = (speaking_rate, noise_scale, noise_scale_duration), on the same ids and injected noise:
  tiny_hf_export_prosody[_refmode]_taps.npz   tiny_hf_export.ggml (written by the reference's exporter), 14 ids.
  full_synth_prosody[_refmode]_taps.npz       vits_synth_model_bytes(0x5EED, VITS_SYNTH_FULL), 16 ids (waveform decimated by 4).
HF mode, and reference mode through reference_mode_patches(). Keys: "settings" [n][3], "ids", "noise_dur" [2][T], "noise_prior" [F][Lmax]
(setting i uses its first L_i columns), "decimate", and per setting "p<i>_log_duration", "p<i>_durations", "p<i>_z_flow",
"p<i>_waveform", "p<i>_waveform_len".

usage: python tests/golden/make_golden_prosody.py   (from the repo root, after building csrc/libvits_hip.so)
"""
import contextlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402

SETTINGS = np.array([[0.6, 0.0, 0.0], [0.6, 1.0, 1.2], [1.7, 0.0, 1.2], [1.7, 1.0, 0.0]], np.float32)


def prosody_taps(parsed, T, seed, refmode=False, decimate=1):
    model = G.hf_model_from_file(parsed)
    ids = G.make_ids(T, model.config.vocab_size, seed)
    rng = np.random.default_rng(seed)
    nd = rng.standard_normal((2, T)).astype(np.float32)
    npr = rng.standard_normal((model.config.flow_size, 256 * T)).astype(np.float32)  # prior noise: the first L columns, the same for every setting
    out, lmax = {}, 0
    for i, (rate, ns, nsd) in enumerate(SETTINGS.tolist()):
        model.speaking_rate, model.noise_scale, model.noise_scale_duration = rate, ns, nsd  # (float32 values, as doubles)
        with (G.reference_mode_patches() if refmode else contextlib.nullcontext()):
            t = G.hf_taps(model, ids, nd, lambda L: npr[:, :L].copy(), refmode=refmode)
        k = "p%d_" % i
        for name in ("log_duration", "durations", "z_flow"):
            out[k + name] = t[name]
        out[k + "waveform_len"] = np.array([t["waveform"].size], np.int64)
        out[k + "waveform"] = t["waveform"][..., ::decimate].copy()
        lmax = max(lmax, t["noise_prior"].shape[-1])
    out.update(settings=SETTINGS, ids=ids.astype(np.int32), noise_dur=nd, noise_prior=npr[:, :lmax].copy(), decimate=np.array([decimate], np.int64))
    return out


def main():
    pkg = G.load_package()
    save = lambda name, d: np.savez_compressed(os.path.join(HERE, name), **d)
    with open(os.path.join(HERE, "tiny_hf_export.ggml"), "rb") as f:
        tiny = G.parse_model_file(f.read())
    full = G.parse_model_file(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_FULL))
    for parsed, T, seed, dec, stem in ((tiny, 14, 21, 1, "tiny_hf_export_prosody"), (full, 16, 23, 4, "full_synth_prosody")):
        for refmode, suffix in ((False, ""), (True, "_refmode")):
            t = prosody_taps(parsed, T, seed, refmode=refmode, decimate=dec)
            name = "%s%s_taps.npz" % (stem, suffix)
            save(name, t)
            print(name, os.path.getsize(os.path.join(HERE, name)), "bytes, frames", [int(t["p%d_durations" % i].sum()) for i in range(len(SETTINGS))])


if __name__ == "__main__":
    main()
