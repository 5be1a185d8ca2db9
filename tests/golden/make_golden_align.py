#!/usr/bin/env python3
"""Generates the forced-alignment fixtures in tests/golden/ (VITS monotonic alignment search, SynthesizerTrn.forward: neg_cent + maximum_path,
written with transformers.VitsModel modules). Runs ONLY in the build container (needs transformers); nothing here travels to the GPU box except
the data files it writes. Helpers come from make_golden.py and make_golden_vc.py, unchanged.

Per (recording, ids, speaker) triple: m, ls = text_encoder(ids) prior means / log-deviations [F][T]; z_p = flow(posterior mean of the recording,
g_speaker) [F][L] (the posterior draw with noise scale 0); logp64 [T][L] = the float64 evaluation of
  logp[t][j] = sum_c(-0.5 log 2pi - ls[c][t]) - 0.5 sum_c (z[c][j] - m[c][t])^2 exp(-2 ls[c][t])
and the float64 optimum of the search over it: durations64 [T], score64.

Fixtures (data only; keys "<case>_<name>" with case "c<k>"; "cases" [n][3] = recording index, ids index, speaker; inputs "pcm<i>", "ids<i>"):
  align_tiny_speakers_hf_export[_refmode]_taps.npz   tiny_speakers_hf_export.ggml (3 speakers)
  align_tiny_flows3_taps.npz                         vc_tiny_flows3.ggml (odd number of coupling layers)
  align_full_synth_taps.npz                          vits_synth_model_bytes(0x5EED, FULL | SPEAKERS | POSTERIOR)

usage: python tests/golden/make_golden_align.py   (from the repo root, after building csrc/libvits_hip.so)
"""
import contextlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402
import make_golden_vc as V  # noqa: E402


def logp(m, ls, z, dt):                      # m, ls [F][T]; z [F][L]
    m, ls, z = m.astype(dt), ls.astype(dt), z.astype(dt)
    s = np.exp(-2 * ls)
    c = (-0.5 * np.log(2 * np.pi) - ls).sum(0) + (-0.5 * m * m * s).sum(0)
    return (c[:, None] + s.T @ (-0.5 * z * z) + (m * s).T @ z).astype(dt)      # [T][L]


def mas(lp):                                 # lp [T][L], T <= L
    T, L = lp.shape
    dt = lp.dtype
    NEG = dt.type(-1e9)
    v = np.full((L, T), NEG, dt)
    for y in range(L):
        for x in range(max(0, T + y - L), min(T, y + 1)):
            cur = NEG if x == y else v[y - 1, x]
            prev = (dt.type(0) if y == 0 else NEG) if x == 0 else v[y - 1, x - 1]
            v[y, x] = lp[x, y] + max(prev, cur)
    d = np.zeros(T, np.int32)
    i = T - 1
    for y in range(L - 1, -1, -1):
        d[i] += 1
        if i != 0 and (i == y or v[y - 1, i] < v[y - 1, i - 1]):
            i -= 1
    return d, v[L - 1, T - 1]


@torch.no_grad()
def align_inputs(model, y, ids, spk):
    cfg = model.config
    n_fft, hop, _ = V.stft_params(cfg)
    input_ids = torch.from_numpy(ids.astype(np.int64))[None]
    mask = torch.ones_like(input_ids).unsqueeze(-1).float()
    enc = model.text_encoder(input_ids=input_ids, padding_mask=mask, attention_mask=None, return_dict=True)
    m = enc.prior_means.transpose(1, 2)[0].numpy()
    ls = enc.prior_log_variances.transpose(1, 2)[0].numpy()
    spec = V.spectrogram_torch(y, n_fft, hop)[None]
    fm = torch.ones(1, 1, spec.shape[-1])
    g = None if spk < 0 else model.embed_speaker(torch.tensor([spk])).unsqueeze(-1)
    pe = model.posterior_encoder
    h = pe.wavenet(pe.conv_pre(spec) * fm, fm, g)
    pm, _ = torch.split(pe.conv_proj(h) * fm, pe.out_channels, dim=1)
    z_p = model.flow(pm * fm, fm, g, reverse=False)[0].numpy()
    return m.astype(np.float32), ls.astype(np.float32), z_p.astype(np.float32)


def fixture(parsed, pcm_lens, id_lens, cases, seed, refmode=False):
    model = G.hf_model_from_file(parsed)
    cfg = model.config
    ys = [V.make_signal(n, cfg.sampling_rate, seed * 100 + i) for i, n in enumerate(pcm_lens)]
    idl = [G.make_ids(t, cfg.vocab_size, seed * 10 + i) for i, t in enumerate(id_lens)]
    out = {"pcm%d" % i: y for i, y in enumerate(ys)}
    out.update({"ids%d" % i: v for i, v in enumerate(idl)})
    for k, (i, j, s) in enumerate(cases):
        with (G.reference_mode_patches() if refmode else contextlib.nullcontext()):
            m, ls, z = align_inputs(model, ys[i], idl[j], s)
        lp = logp(m, ls, z, np.float64)
        d, sc = mas(lp)
        assert d.sum() == lp.shape[1] and d.min() >= 1
        for name, v in (("prior_mean", m), ("prior_logvar", ls), ("z_p", z), ("logp64", lp), ("durations64", d), ("score64", np.array([sc], np.float64))):
            out["c%d_%s" % (k, name)] = v
    out["cases"] = np.array(cases, np.int32)
    return out


def main():
    pkg = G.load_package()
    save = lambda name, d: np.savez_compressed(os.path.join(HERE, name), **d)
    with open(os.path.join(HERE, "tiny_speakers_hf_export.ggml"), "rb") as f:
        parsed = G.parse_model_file(f.read())
    cases = [(0, 0, -1), (1, 1, -1), (2, 2, 0), (1, 0, 2), (2, 1, 1)]
    for refmode, suffix in ((False, ""), (True, "_refmode")):
        save("align_tiny_speakers_hf_export%s_taps.npz" % suffix, fixture(parsed, [203, 517, 1103], [9, 21, 40], cases, 31, refmode=refmode))
    with open(os.path.join(HERE, "vc_tiny_flows3.ggml"), "rb") as f:
        p3 = G.parse_model_file(f.read())
    save("align_tiny_flows3_taps.npz", fixture(p3, [301, 811], [11, 33], [(0, 0, -1), (1, 1, -1), (1, 0, -1)], 32))
    full = G.parse_model_file(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_FULL | pkg.SYNTH_SPEAKERS | pkg.SYNTH_POSTERIOR))
    save("align_full_synth_taps.npz", fixture(full, [5000, 9301], [7, 19], [(0, 0, 3), (1, 1, 77), (1, 0, -1)], 33))


if __name__ == "__main__":
    main()
