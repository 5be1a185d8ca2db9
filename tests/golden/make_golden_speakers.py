#!/usr/bin/env python3
"""Generates the multi-speaker fixtures in tests/golden/ (speaker conditioning, transformers VitsModel with num_speakers > 1).
Runs ONLY in the build container (needs transformers and, for the exporter-written file, the reference tree's scripts/export_vits.py);
nothing here travels to the GPU box except the data files it writes. Helpers come from make_golden.py, which is unchanged.

Fixtures (data only):
  tiny_speakers_hf_export.ggml        a tiny VitsModel(num_speakers=3, speaker_embedding_size=8) written by the reference's own exporter:
                                      pins the real names and layout of embed_speaker / *.cond / cond_layer.
  tiny_speakers_hf_export[_refmode]_taps.npz   transformers taps (HF mode; reference mode through reference_mode_patches()) for the
                                      speakers None (-1), 0, 1, 2 on the same ids and injected noise; keys "s<speaker>_<tap>" (speaker -1 = "sm1").
  full_synth_speakers[_refmode]_taps.npz  the same for vits_synth_model_bytes(0x5EED, VITS_SYNTH_FULL | VITS_SYNTH_SPEAKERS), 16 ids, speakers
                                      -1, 5, 77 (waveform decimated by 4, pre_tanh not stored).
  tiny_synth_speakers_arith_f16_taps.npz  vits_synth_model_bytes(0x5EED, VITS_SYNTH_TINY | VITS_SYNTH_SPEAKERS) — the architecture and weights of
                                      make_golden.py's tiny_synth_arith_f16_taps.npz plus the speaker tensors — in reference mode with every conv input
                                      of the flow and the vocoder rounded to fp16 (make_golden.conv_operand_rounding: the VITS_ARITH_F16 pin), 20 ids,
                                      speakers -1, 1 and 3.

usage: python tests/golden/make_golden_speakers.py REFERENCE_TREE   (from the repo root, after building csrc/libvits_hip.so)
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402


def hf_taps_speaker(model, ids, noise_dur, noise_prior_fn, speaker, refmode=False, rounding=None, keep=None):
    """make_golden.hf_taps with the speaker term (VitsModel.forward, modeling_vits.py: g = embed_speaker(speaker_id).unsqueeze(-1), passed
    to the duration predictor, the flow and the decoder); speaker None = no conditioning (hf_taps itself)."""
    if speaker is None:
        return G.hf_taps(model, ids, noise_dur, noise_prior_fn, refmode=refmode, rounding=rounding)
    cfg = model.config
    g = model.embed_speaker(torch.tensor([speaker])).unsqueeze(-1)
    input_ids = torch.from_numpy(ids.astype(np.int64))[None]
    mask = torch.ones_like(input_ids).unsqueeze(-1).float()
    enc = model.text_encoder(input_ids=input_ids, padding_mask=mask, attention_mask=None, return_dict=True)
    hidden = enc.last_hidden_state.transpose(1, 2)
    mask_t = mask.transpose(1, 2)
    prior_means, prior_logvar = enc.prior_means, enc.prior_log_variances
    real_randn = torch.randn
    try:
        torch.randn = lambda *a, **k: torch.from_numpy(noise_dur.astype(np.float32))[None]
        log_duration = model.duration_predictor(hidden, mask_t, g, reverse=True, noise_scale=model.noise_scale_duration)
    finally:
        torch.randn = real_randn
    duration = torch.ceil(torch.exp(log_duration) * mask_t * (1.0 / model.speaking_rate))
    predicted_lengths = torch.clamp_min(torch.sum(duration, [1, 2]), 1).long()
    L = int(predicted_lengths.max())
    out_mask = (torch.arange(L)[None] < predicted_lengths[:, None]).unsqueeze(1).float()
    attn_mask = torch.unsqueeze(mask_t, 2) * torch.unsqueeze(out_mask, -1)
    b, _, out_len, in_len = attn_mask.shape
    cum = torch.cumsum(duration, -1).view(b * in_len, 1)
    idx = torch.arange(out_len, dtype=duration.dtype)
    valid = (idx.unsqueeze(0) < cum).to(attn_mask.dtype).view(b, in_len, out_len)
    padded = valid - torch.nn.functional.pad(valid, [0, 0, 1, 0, 0, 0])[:, :-1]
    attn = padded.unsqueeze(1).transpose(2, 3) * attn_mask
    pm = torch.matmul(attn.squeeze(1), prior_means).transpose(1, 2)
    plv = torch.matmul(attn.squeeze(1), prior_logvar).transpose(1, 2)
    noise_prior = noise_prior_fn(L)
    z_p = pm + torch.from_numpy(noise_prior)[None] * torch.exp(plv) * model.noise_scale
    z = model.flow(z_p, out_mask, g, reverse=True)
    spec = z * out_mask
    dec = model.decoder
    h = dec.conv_pre(spec) + dec.cond(g)  # VitsHifiGan.forward
    for i in range(dec.num_upsamples):
        h = torch.nn.functional.leaky_relu(h, cfg.leaky_relu_slope)
        up = dec.upsampler[i]
        if refmode:
            hin = rounding.round(h) if rounding is not None else h
            h = torch.nn.functional.conv_transpose1d(hin, up.weight, up.bias, stride=up.stride, padding=0)  # Q1
        else:
            h = up(h)
        res = dec.resblocks[i * dec.num_kernels](h)
        for j in range(1, dec.num_kernels):
            res = res + dec.resblocks[i * dec.num_kernels + j](h)
        h = res * float(np.float32(1.0 / dec.num_kernels)) if refmode else res / dec.num_kernels
    h = torch.nn.functional.leaky_relu(h, cfg.leaky_relu_slope) if refmode else torch.nn.functional.leaky_relu(h)  # Q2
    pre = dec.conv_post(h)
    wave = torch.tanh(pre)
    if not refmode:
        assert torch.allclose(wave, dec(spec, g), atol=1e-6)  # against the unmodified decoder forward
    f = lambda t: t[0].detach().numpy().astype(np.float32)
    return dict(
        ids=ids.astype(np.int32), noise_dur=noise_dur.astype(np.float32), noise_prior=noise_prior.astype(np.float32),
        log_duration=f(log_duration), durations=f(duration), z_p=f(z_p), z_flow=f(spec), pre_tanh=f(pre), waveform=f(wave),
    )


def speaker_taps(parsed, T, seed, speakers, refmode=False, dtype=None, decimate=1):
    model = G.hf_model_from_file(parsed)
    ids = G.make_ids(T, model.config.vocab_size, seed)
    rng = np.random.default_rng(seed)
    nd = rng.standard_normal((2, T)).astype(np.float32)
    F = model.config.flow_size
    npr = rng.standard_normal((F, 64 * T)).astype(np.float32)  # prior noise: the first L columns, the same for every speaker
    out = {}
    for s in speakers:
        with torch.no_grad(), (G.reference_mode_patches() if refmode else contextlib.nullcontext()):
            with (G.conv_operand_rounding([model.flow, model.decoder], dtype) if dtype is not None else contextlib.nullcontext()) as cr:
                t = hf_taps_speaker(model, ids, nd, lambda L: npr[:, :L].copy(), s, refmode=refmode, rounding=cr)
        key = "sm1" if s is None else "s%d" % s
        for k in ("log_duration", "durations", "z_flow", "noise_prior"):
            out[key + "_" + k] = t[k]
        out[key + "_waveform_len"] = np.array([t["waveform"].size], np.int64)
        out[key + "_waveform"] = t["waveform"][..., ::decimate].copy()
        out["ids"], out["noise_dur"] = t["ids"], t["noise_dur"]
    out["decimate"] = np.array([decimate], np.int64)
    out["speakers"] = np.array([-1 if s is None else s for s in speakers], np.int32)
    return out


def reference_exported_tiny_speakers(reference_root):
    """A tiny multi-speaker HF model written by the reference's own exporter (scripts/export_vits.py), like make_golden.reference_exported_tiny."""
    sys.path.insert(0, os.path.join(reference_root, "scripts"))
    import export_vits
    from transformers import VitsConfig, VitsModel
    torch.manual_seed(9)
    cfg = VitsConfig(vocab_size=38, hidden_size=16, num_hidden_layers=2, num_attention_heads=2, window_size=2, ffn_dim=32,
                     flow_size=16, spectrogram_bins=9, upsample_initial_channel=32, upsample_rates=[4, 2],
                     upsample_kernel_sizes=[8, 4], resblock_kernel_sizes=[3, 5], resblock_dilation_sizes=[[1, 3], [1, 2]],
                     depth_separable_num_layers=2, prior_encoder_num_flows=2, prior_encoder_num_wavenet_layers=2,
                     posterior_encoder_num_wavenet_layers=1, num_speakers=3, speaker_embedding_size=8)
    model = VitsModel(cfg).eval()
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.startswith("decoder.") and "weight" in n and "cond" not in n:
                p.mul_(0.6)
        model.duration_predictor.flows[0].log_scale.copy_(torch.tensor([[0.2], [-0.1]]))
        model.duration_predictor.flows[0].translate.copy_(torch.tensor([[-0.5], [0.3]]))
        # default init leaves the speaker terms small: make them audible (durations and audio both move)
        model.embed_speaker.weight.mul_(2.0)
        model.duration_predictor.cond.weight.mul_(3.0)
    model = export_vits.remove_weight_norm_and_convert_to_fp16(model)

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

    path = os.path.join(HERE, "tiny_speakers_hf_export.ggml")
    with contextlib.redirect_stdout(io.StringIO()):
        export_vits.serialize_model_to_binary(model.config, model.state_dict(), Tok(), path)
    return open(path, "rb").read()


def main():
    pkg = G.load_package()
    save = lambda name, d: np.savez_compressed(os.path.join(HERE, name), **d)
    data = reference_exported_tiny_speakers(sys.argv[1])
    parsed = G.parse_model_file(data)
    print("tiny_speakers_hf_export.ggml", len(data), "bytes,", len(parsed["tensors"]), "tensors")
    spk = (None, 0, 1, 2)
    for refmode, suffix in ((False, ""), (True, "_refmode")):
        t = speaker_taps(parsed, 14, 11, spk, refmode=refmode)
        save("tiny_speakers_hf_export%s_taps.npz" % suffix, t)
        print(suffix or "hf", "frames", [int(t[k].sum()) for k in sorted(t) if k.endswith("_durations")])
    tiny = G.parse_model_file(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_TINY | pkg.SYNTH_SPEAKERS))
    save("tiny_synth_speakers_arith_f16_taps.npz", speaker_taps(tiny, 20, 12, (None, 1, 3), refmode=True, dtype=torch.float16))
    full = G.parse_model_file(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_FULL | pkg.SYNTH_SPEAKERS))
    for refmode, suffix in ((False, ""), (True, "_refmode")):
        t = speaker_taps(full, 16, 13, (None, 5, 77), refmode=refmode, decimate=4)
        save("full_synth_speakers%s_taps.npz" % suffix, t)
        print("full", suffix or "hf", "frames", [int(t[k].sum()) for k in sorted(t) if k.endswith("_durations")])


if __name__ == "__main__":
    main()
