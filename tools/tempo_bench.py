"""Cost of a conversion's rate and pitch (vits_model_set_conversion_ratios, tempo.hip + pitch.hip) on the FULL synthetic multi-speaker model in fp32, PCM left on
the device: conversions of batch 64 and batch 1, recordings of --seconds each, with the stage off ("off": nothing given; "ones": rates and pitches of 1 given),
at the tempo q = 0.8 ("rate08": rate 0.8) and at the same tempo with the varispeed behind it ("rate08_pitch": pitch 2^(2/12), rate 0.8 * that pitch). ms per call
(wall clock around the call), median of interleaved rounds; a profiled pass gives the stage's own kernels per call ("tempo_search", "tempo_ola", "pitch"), the
search's time per step of its longest row's chain, and the stage's share of the call's kernel time. On a commit in front of the stage the same tool times "off"
alone. Prints one JSON line.
usage: python tools/tempo_bench.py [--rounds 5] [--steps 4] [--seconds 1.5] [--tag NAME]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from conftest import load_package  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--seconds", type=float, default=1.5)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    pkg = load_package()
    import torch
    m = pkg.Model(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_FULL | pkg.SYNTH_SPEAKERS | pkg.SYNTH_POSTERIOR))
    has_tempo = hasattr(m, "set_conversion_ratios")
    fs = m.sampling_rate
    n = int(a.seconds * fs)
    p2 = float(np.float32(2.0 ** (2 / 12)))
    cases = [("off", None, None)]
    if has_tempo:
        cases += [("ones", 1.0, 1.0), ("rate08", 0.8, None), ("rate08_pitch", float(np.float32(0.8 * p2)), p2)]
    res = {}
    for batch in (64, 1):
        rng = np.random.default_rng(3)
        t = np.arange(n) / fs
        pcm = np.stack([0.5 * np.sin(2 * np.pi * rng.uniform(90, 240) * t) + 0.02 * rng.standard_normal(n) for _ in range(batch)]).astype(np.float32)
        src, tgt = np.arange(batch) % 4, (np.arange(batch) + 1) % 4
        stride = 2 * n + 4096  # (room for the slowest rows: N' <= N / 0.8, and the varispeed gives that back)
        out_dev = torch.empty(batch * stride, dtype=torch.float32, device="cuda")

        def call(r, p):
            kw = {}
            if r is not None:
                kw["vc_rate"] = r
            if p is not None:
                kw["vc_pitch"] = p
            return m.convert_batch(pcm, src=src, tgt=tgt, noise_seed=5, out_device=out_dev.data_ptr(), out_device_stride=stride, skip_host_copy=True, keep_pcm=False, **kw)

        for _, r, p in cases:
            call(r, p)
        times = {name: [] for name, _, _ in cases}
        for _ in range(a.rounds):
            for name, r, p in cases:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    call(r, p)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
        for name, r, p in cases:
            m.prof_enable(True)
            m.prof_reset()
            _, lengths, frames = call(r, p)
            rep = m.prof_report()
            m.prof_enable(False)
            ks = rep["kernels"]
            tot = sum(x["ms"] for x in ks) or 1.0
            us = {k: round(1e3 * sum(x["ms"] for x in ks if x["name"] == k), 2) for k in ("tempo_search", "tempo_ola", "pitch")}
            row0 = None if not has_tempo or m.last_tempo() is None else [int(v) for v in m.last_tempo()[0]]
            res["b%d_%s" % (batch, name)] = {
                "ms_per_call": round(float(np.median(times[name])), 4), "samples": int(lengths.sum()), "frames": int(frames.sum()), "kernel_ms": round(tot, 4),
                "stage_us": us, "search_us_per_step": None if not row0 or not row0[3] else round(us["tempo_search"] / row0[3], 3),
                "stage_share_of_kernel_time": round(sum(us.values()) * 1e-3 / tot, 5), "launches": sorted({x["name"] for x in ks}), "tempo_row0": row0,
                "rounds_ms": [round(v, 4) for v in times[name]]}
        del out_dev
    m.close()
    print(json.dumps({"tool": "tempo_bench", "tag": a.tag, "model": "FULL synthetic, speakers + posterior", "arith": "f32", "seconds": a.seconds, "results": res}))


if __name__ == "__main__":
    main()
