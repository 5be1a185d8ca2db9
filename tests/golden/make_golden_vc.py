#!/usr/bin/env python3
"""Generates the voice-conversion fixtures in tests/golden/ (VITS SynthesizerTrn.voice_conversion written with transformers.VitsModel modules).
Runs ONLY in the build container (needs transformers and, for the exporter-written file, the reference tree's scripts/export_vits.py);
nothing here travels to the GPU box except the data files it writes. Helpers come from make_golden.py, unchanged.

Per utterance: spec = spectrogram_torch(y) (periodic Hann, n_fft = 2 (bins - 1), hop = prod(upsample_rates), reflection pad (n_fft - hop) / 2,
center = False, sqrt(|X|^2 + 1e-6)); m, log_std = posterior_encoder(spec, g_src); z_q = m + eps * exp(log_std) with an injected eps [F][L];
z_p = flow(z_q, g_src); z_flow = flow(z_p, g_tgt, reverse); waveform = decoder(z_flow, g_tgt) (reference mode: make_golden_speakers' decoder).

Fixtures (data only; keys "<pair>_<tap>" with pair "p<src>_<tgt>", -1 written "m1"; inputs "pcm<i>"; "pairs" [n][3] = input, src, tgt):
  vc_tiny_speakers_hf_export[_refmode]_taps.npz  tiny_speakers_hf_export.ggml (3 speakers, 1 posterior layer), pairs (-1,-1), (0,2), (2,1)
  vc_tiny_flows3.ggml                     a tiny VitsModel with prior_encoder_num_flows = 3 and 3 posterior layers, written by the reference's
                                          exporter: the odd channel-flip parity
  vc_tiny_flows3_taps.npz                 its taps (HF mode), pairs (-1,-1) on two inputs
  vc_full_synth_taps.npz                  vits_synth_model_bytes(0x5EED, FULL | SPEAKERS | POSTERIOR), pairs (3,50), (77,77) on ~0.3 s inputs
                                          (waveform decimated by 4)
  vc_tiny_synth_arith_f16_taps.npz        TINY | SPEAKERS | POSTERIOR, reference mode, every conv input of the flow (both directions), of the
                                          posterior WaveNet and of the vocoder rounded to fp16 (make_golden.conv_operand_rounding)

usage: python tests/golden/make_golden_vc.py REFERENCE_TREE   (from the repo root, after building csrc/libvits_hip.so)
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


def stft_params(cfg):
    n_fft = 2 * (cfg.spectrogram_bins - 1)
    hop = int(np.prod(cfg.upsample_rates))
    return n_fft, hop, (n_fft - hop) // 2


def spectrogram_torch(y, n_fft, hop):
    """VITS mel_processing.spectrogram_torch (center=False)."""
    p = (n_fft - hop) // 2
    yt = torch.nn.functional.pad(torch.from_numpy(y.astype(np.float32))[None, None], (p, p), mode="reflect")[0, 0]
    X = torch.stft(yt, n_fft, hop_length=hop, win_length=n_fft, window=torch.hann_window(n_fft), center=False, normalized=False, onesided=True,
                   return_complex=True)
    return torch.sqrt(X.real.pow(2) + X.imag.pow(2) + 1e-6)


def make_signal(n, sr, seed):
    """harmonics plus noise, |y| <= 0.9"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    f0 = rng.uniform(90, 260)
    y = np.zeros(n)
    for h in range(1, 6):
        y += rng.uniform(0.2, 1.0) / h * np.sin(2 * np.pi * f0 * h * t + rng.uniform(0, 2 * np.pi))
    y += 0.1 * rng.standard_normal(n)
    return (0.9 * y / np.abs(y).max()).astype(np.float32)


@torch.no_grad()
def vc_taps(model, y, eps, src, tgt, refmode=False, rounding=None):
    cfg = model.config
    n_fft, hop, _ = stft_params(cfg)
    spec = spectrogram_torch(y, n_fft, hop)[None]
    L = spec.shape[-1]
    mask = torch.ones(1, 1, L)
    g_s = None if src < 0 else model.embed_speaker(torch.tensor([src])).unsqueeze(-1)
    g_t = None if tgt < 0 else model.embed_speaker(torch.tensor([tgt])).unsqueeze(-1)
    pe = model.posterior_encoder
    h = pe.conv_pre(spec) * mask
    h = pe.wavenet(h, mask, g_s)
    stats = pe.conv_proj(h) * mask
    m, logs = torch.split(stats, pe.out_channels, dim=1)
    e = torch.from_numpy(eps[:, :L].astype(np.float32))[None]
    z_q = (m + e * torch.exp(logs)) * mask
    z_p = model.flow(z_q, mask, g_s, reverse=False)
    z = model.flow(z_p, mask, g_t, reverse=True)
    wave, pre = decode(model, z * mask, g_t, refmode, rounding)
    f = lambda t: t[0].detach().numpy().astype(np.float32)
    return dict(spec=f(spec), post_mean=f(m), post_logstd=f(logs), noise_prior=eps[:, :L].astype(np.float32), z_q=f(z_q), z_p=f(z_p), z_flow=f(z * mask),
                waveform=f(wave))


def decode(model, spec, g, refmode, rounding):
    """VitsHifiGan.forward with the reference's Q1 / Q2 in reference mode (as make_golden_speakers.hf_taps_speaker)."""
    cfg = model.config
    dec = model.decoder
    h = dec.conv_pre(spec)
    if g is not None:
        h = h + dec.cond(g)
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
    if not refmode and rounding is None:
        assert torch.allclose(wave, dec(spec, g), atol=1e-6)
    return wave, pre


def key(s, t):
    return "p%s_%s" % ("m1" if s < 0 else s, "m1" if t < 0 else t)


def fixture(parsed, lengths, pairs, seed, refmode=False, dtype=None, decimate=1, data=None):
    """pairs: (input index, src, tgt)"""
    model = parsed if data is None else data
    if not hasattr(model, "posterior_encoder"):
        model = G.hf_model_from_file(parsed)
        # (hf_model_from_file tolerates a missing posterior encoder: here every one of its tensors must come from the file)
        want = [k for k in model.state_dict() if k.startswith("posterior_encoder.")]
        assert want and all(k in parsed["tensors"] for k in want), [k for k in want if k not in parsed["tensors"]]
    cfg = model.config
    F = cfg.flow_size
    rng = np.random.default_rng(seed)
    ys = [make_signal(n, cfg.sampling_rate, seed * 100 + i) for i, n in enumerate(lengths)]
    eps = [rng.standard_normal((F, n // stft_params(cfg)[1])).astype(np.float32) for n in lengths]
    out = {"pcm%d" % i: y for i, y in enumerate(ys)}
    for i, s, t in pairs:
        mods = [model.flow, model.posterior_encoder.wavenet, model.decoder]
        with torch.no_grad(), (G.reference_mode_patches() if refmode else contextlib.nullcontext()):
            with (G.conv_operand_rounding(mods, dtype) if dtype is not None else contextlib.nullcontext()) as cr:
                tp = vc_taps(model, ys[i], eps[i], s, t, refmode=refmode, rounding=cr)
        k = key(s, t) + "_u%d" % i
        for name, v in tp.items():
            if name == "waveform":
                out[k + "_waveform_len"] = np.array([v.size], np.int64)
                v = v[..., ::decimate].copy()
            out[k + "_" + name] = v
    out["pairs"] = np.array(pairs, np.int32)
    out["decimate"] = np.array([decimate], np.int64)
    return out


def reference_exported_tiny_flows3(reference_root):
    """A tiny single-speaker VitsModel with an odd number of coupling layers, written by the reference's exporter."""
    sys.path.insert(0, os.path.join(reference_root, "scripts"))
    import export_vits
    from transformers import VitsConfig, VitsModel
    torch.manual_seed(17)
    cfg = VitsConfig(vocab_size=38, hidden_size=16, num_hidden_layers=2, num_attention_heads=2, window_size=2, ffn_dim=32,
                     flow_size=16, spectrogram_bins=9, upsample_initial_channel=32, upsample_rates=[4, 2],
                     upsample_kernel_sizes=[8, 4], resblock_kernel_sizes=[3, 5], resblock_dilation_sizes=[[1, 3], [1, 2]],
                     depth_separable_num_layers=2, prior_encoder_num_flows=3, prior_encoder_num_wavenet_layers=2,
                     posterior_encoder_num_wavenet_layers=3)
    model = VitsModel(cfg).eval()
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.startswith("decoder.") and "weight" in n:
                p.mul_(0.6)
            if n.startswith("flow.") and "conv_post" in n:  # (zero-initialised in transformers: give the coupling layers something to do)
                p.normal_(0.0, 0.3)
        model.duration_predictor.flows[0].log_scale.copy_(torch.tensor([[0.2], [-0.1]]))
        model.duration_predictor.flows[0].translate.copy_(torch.tensor([[-0.5], [0.3]]))
    model = export_vits.remove_weight_norm_and_convert_to_fp16(model)
    path = os.path.join(HERE, "vc_tiny_flows3.ggml")
    with contextlib.redirect_stdout(io.StringIO()):
        export_vits.serialize_model_to_binary(model.config, model.state_dict(), tok(), path)
    return open(path, "rb").read()


def tok():
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
    return Tok()


def main():
    pkg = G.load_package()
    save = lambda name, d: np.savez_compressed(os.path.join(HERE, name), **d)
    # tiny exporter file with speakers: hop 8, n_fft 16, pad 4 -> minimum input max(8, 5) = 8 samples
    with open(os.path.join(HERE, "tiny_speakers_hf_export.ggml"), "rb") as f:
        parsed = G.parse_model_file(f.read())
    lens = [8, 203, 517]
    pairs = [(0, -1, -1), (1, -1, -1), (2, -1, -1), (1, 0, 2), (2, 0, 2), (0, 2, 1), (2, 2, 1)]
    for refmode, suffix in ((False, ""), (True, "_refmode")):
        save("vc_tiny_speakers_hf_export%s_taps.npz" % suffix, fixture(parsed, lens, pairs, 21, refmode=refmode))
    data = reference_exported_tiny_flows3(sys.argv[1])
    p3 = G.parse_model_file(data)
    print("vc_tiny_flows3.ggml", len(data), "bytes")
    save("vc_tiny_flows3_taps.npz", fixture(p3, [13, 301], [(0, -1, -1), (1, -1, -1)], 22))
    full = G.parse_model_file(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_FULL | pkg.SYNTH_SPEAKERS | pkg.SYNTH_POSTERIOR))
    save("vc_full_synth_taps.npz", fixture(full, [4801, 5000], [(0, 3, 50), (1, 77, 77)], 23, decimate=4))
    tiny = G.parse_model_file(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_TINY | pkg.SYNTH_SPEAKERS | pkg.SYNTH_POSTERIOR))
    save("vc_tiny_synth_arith_f16_taps.npz", fixture(tiny, [411, 1003], [(0, -1, -1), (1, 1, 3), (0, 3, 0)], 24, refmode=True, dtype=torch.float16))


if __name__ == "__main__":
    main()
