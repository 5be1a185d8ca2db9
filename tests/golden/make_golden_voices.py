#!/usr/bin/env python3
"""Generates the custom-voice fixtures in tests/golden/ (vits_model_add_voices): transformers taps for speaker embeddings that are NOT rows of the
model file. Runs on the CPU (needs transformers); reads only tests/golden/tiny_speakers_hf_export.ggml; helpers come from make_golden.py and
make_golden_speakers.py, which are unchanged. A second run reproduces the files bit for bit (np.savez, no timestamps).

Fixtures (data only):
  tiny_speakers_hf_export_voices[_refmode]_taps.npz   make_golden_speakers.hf_taps_speaker on the model of tiny_speakers_hf_export.ggml after
        model.embed_speaker.weight[SLOT] was overwritten with
          v0  0.5 emb[0] + 0.5 emb[1]
          v1  0.25 emb[0] + 0.75 emb[2]
          v2  a random vector of the embedding's own RMS
        (fp32, the file's rows), in HF mode and, through reference_mode_patches(), in reference mode; keys "v<k>_<tap>", the vectors themselves
        under "vectors" [3][E], 14 ids.

Durations are ceil(exp(log_duration) / speaking_rate): a test can only demand that an implementation within 2e-4 of transformers reproduces them
when no token sits next to an integer. That is a property of the INPUTS, so it is checked here, on transformers' own values: seeds are tried in
order (one seed draws the ids, the injected noise and the random vector) and the first is kept for which every token of every voice in both modes
is at least MARGIN frames away from an integer; seed and margin are stored in the fixtures.

usage: python tests/golden/make_golden_voices.py   (from the repo root)
"""
import contextlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402
from make_golden_speakers import hf_taps_speaker  # noqa: E402

SLOT = 2       # the embed_speaker row that carries the vector in transformers
T = 14
MARGIN = 0.02  # frames
MAX_SEEDS = 100000


class TooLong(Exception):
    """an utterance longer than the drawn prior noise (64 frames per id): the seed is passed over"""


def vectors_for(emb, rng):
    h, q, tq = np.float32(0.5), np.float32(0.25), np.float32(0.75)
    rnd = rng.standard_normal(emb.shape[1]).astype(np.float32)
    rms = np.float32(np.sqrt((emb.astype(np.float64) ** 2).mean()))
    rnd = (rnd * (rms / np.float32(np.sqrt((rnd.astype(np.float64) ** 2).mean())))).astype(np.float32)
    return np.stack([(h * emb[0] + h * emb[1]).astype(np.float32), (q * emb[0] + tq * emb[2]).astype(np.float32), rnd])


def inputs_for(parsed, model, seed):
    emb = parsed["tensors"]["embed_speaker.weight"][0].astype(np.float32)
    ids = G.make_ids(T, model.config.vocab_size, seed)
    rng = np.random.default_rng(seed)
    nd = rng.standard_normal((2, T)).astype(np.float32)
    npr = rng.standard_normal((model.config.flow_size, 64 * T)).astype(np.float32)
    return ids, nd, npr, vectors_for(emb, rng)


def distance_to_integer(log_duration, model):
    """(frames per token before the ceil, their smallest distance to an integer) from transformers' log_duration"""
    x = np.exp(log_duration.astype(np.float32)).astype(np.float64) / float(model.speaking_rate)
    return x, float(np.abs(x - np.round(x)).min())


def screen(parsed, model, seed, refmode):
    """the margin of a seed from the duration predictor alone (the lines of hf_taps_speaker up to log_duration): cheap, so that thousands of seeds
    can be tried; the margin of record is the one voice_taps computes from the taps it stores"""
    ids, nd, _, vecs = inputs_for(parsed, model, seed)
    input_ids = torch.from_numpy(ids.astype(np.int64))[None]
    mask = torch.ones_like(input_ids).unsqueeze(-1).float()
    margin = np.inf
    with torch.no_grad(), (G.reference_mode_patches() if refmode else contextlib.nullcontext()):
        hidden = model.text_encoder(input_ids=input_ids, padding_mask=mask, attention_mask=None, return_dict=True).last_hidden_state.transpose(1, 2)
        for vec in vecs:
            model.embed_speaker.weight[SLOT] = torch.from_numpy(vec)
            g = model.embed_speaker(torch.tensor([SLOT])).unsqueeze(-1)
            real_randn = torch.randn
            try:
                torch.randn = lambda *a, **k: torch.from_numpy(nd.astype(np.float32))[None]
                logw = model.duration_predictor(hidden, mask.transpose(1, 2), g, reverse=True, noise_scale=model.noise_scale_duration)
            finally:
                torch.randn = real_randn
            margin = min(margin, distance_to_integer(logw[0].numpy(), model)[1])
    return margin


def voice_taps(parsed, model, seed, refmode):
    ids, nd, npr, vecs = inputs_for(parsed, model, seed)
    out = {"vectors": vecs, "slot": np.array([SLOT], np.int32), "seed": np.array([seed], np.int64), "decimate": np.array([1], np.int64)}
    margin = np.inf

    def prior(L):
        if L > npr.shape[1]:
            raise TooLong()
        return npr[:, :L].copy()

    for k, vec in enumerate(vecs):
        with torch.no_grad():
            model.embed_speaker.weight[SLOT] = torch.from_numpy(vec)
            with (G.reference_mode_patches() if refmode else contextlib.nullcontext()):
                t = hf_taps_speaker(model, ids, nd, prior, SLOT, refmode=refmode)
        x, dist = distance_to_integer(t["log_duration"], model)
        agree = np.array_equal(np.ceil(x).ravel(), t["durations"].ravel())  # (float64 here, fp32 in torch: they part only next to an integer)
        margin = min(margin, dist if agree else 0.0)
        key = "v%d" % k
        for name in ("log_duration", "durations", "z_flow", "noise_prior", "waveform"):
            out[key + "_" + name] = t[name]
        out[key + "_waveform_len"] = np.array([t["waveform"].size], np.int64)
        out["ids"], out["noise_dur"] = t["ids"], t["noise_dur"]
    return out, margin


def main():
    with open(os.path.join(HERE, "tiny_speakers_hf_export.ggml"), "rb") as f:
        parsed = G.parse_model_file(f.read())
    assert parsed["tensors"]["embed_speaker.weight"][1] == 0  # fp32 in the file: the vectors are combinations of exactly the rows the engine reads
    model = G.hf_model_from_file(parsed)
    for seed in range(1, MAX_SEEDS + 1):
        if min(screen(parsed, model, seed, refmode) for refmode in (False, True)) < MARGIN:
            continue
        try:
            taps = [voice_taps(parsed, model, seed, refmode) for refmode in (False, True)]
        except TooLong:
            print("seed", seed, "passed over: longer than the prior noise drawn")
            continue
        margin = min(m for _, m in taps)
        print("seed", seed, "margin %.4f" % margin, "frames", [int(taps[0][0]["v%d_durations" % k].sum()) for k in range(3)])
        if margin >= MARGIN:
            break
    else:
        raise SystemExit("no seed with a margin of %g frames" % MARGIN)
    for (t, _), suffix in zip(taps, ("", "_refmode")):
        t["margin"] = np.array([margin], np.float64)
        np.savez_compressed(os.path.join(HERE, "tiny_speakers_hf_export_voices%s_taps.npz" % suffix), **t)


if __name__ == "__main__":
    main()
