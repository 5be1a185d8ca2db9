"""Cost of forced alignment (vits_model_align_batch) on the FULL synthetic model with speakers and posterior encoder: batch 64 and batch 1 at
~2.3 s per utterance (143 frames, 129 ids each), fp32 and f16, against vits_model_convert_batch on the same audio (PCM left on the device): the
alignment runs the conversion's front end plus the text encoder and the two alignment kernels, and none of the reverse flow and vocoder. ms per call
(wall clock around the call), median of interleaved rounds. A profiled pass gives the share of align_logp and align_mas in the call's kernel time,
their own times and what a frame step of the search costs (align_mas time / longest utterance's frames). One long case (batch 1, >= 60 s,
>= 1,000 ids: more than one token per lane, decision bits in the arena) is timed once per arithmetic. Prints one JSON line.
usage: python tools/align_bench.py [--rounds 5] [--steps 4] [--seconds 2.3] [--long-seconds 64] [--long-ids 1201]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from conftest import load_package  # noqa: E402
from vc_bench import signals  # noqa: E402


def align_kernels(report):
    ks = report["kernels"]
    tot = sum(k["ms"] for k in ks) or 1.0
    pick = lambda name: sum(k["ms"] for k in ks if k["name"] == name)
    return tot, pick("align_logp"), pick("align_mas")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--seconds", type=float, default=2.3)
    ap.add_argument("--long-seconds", type=float, default=64.0)
    ap.add_argument("--long-ids", type=int, default=1201)
    a = ap.parse_args()
    pkg = load_package()
    import torch
    n = int(a.seconds * 16000)
    L = n // 256
    S = L * 256 + 4096
    out_dev = torch.empty(64 * S, dtype=torch.float32, device="cuda")
    m = pkg.Model(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_FULL | pkg.SYNTH_SPEAKERS | pkg.SYNTH_POSTERIOR))
    m.prepare_conversion()
    pcm64 = signals(64, n)
    spk64 = np.arange(64, dtype=np.int32)
    T = min(L, 129)
    ids64 = pkg.synth_ids(64, T)
    cases = {"b64": (pcm64, spk64, ids64), "b1": (pcm64[:1], spk64[:1], ids64[:1])}
    n_long = int(a.long_seconds * 16000)
    pcm_long = signals(1, n_long, seed=4)
    ids_long = pkg.synth_ids(1, a.long_ids)
    res = {}
    for arith_name, arith in (("f32", pkg.ARITH_F32), ("f16", pkg.ARITH_F16)):
        m.set_arith(arith)
        for cname, (pcm, spk, ids) in cases.items():
            B = pcm.shape[0]
            steps = a.steps if B > 1 else 10 * a.steps
            al = lambda: m.align_batch(pcm, ids, speakers=spk, noise_scale=1.0, noise_seed=5)[1]
            vc = lambda: m.convert_batch(pcm, src=spk, tgt=spk, noise_seed=5, out_device=out_dev.data_ptr(), out_device_stride=S, skip_host_copy=True,
                                         keep_pcm=False)[2]
            for _ in range(2):
                al()
                vc()
            times = {"align": [], "vc": []}
            for _ in range(a.rounds):
                for label, fn in (("align", al), ("vc", vc)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(steps):
                        fr = fn()
                    torch.cuda.synchronize()
                    times[label].append((time.perf_counter() - t0) * 1e3 / steps)
            m.prof_enable(True)
            m.prof_reset()
            al()
            rep = m.prof_report()
            m.prof_enable(False)
            tot, lp, mas = align_kernels(rep)
            ams, vms = float(np.median(times["align"])), float(np.median(times["vc"]))
            res["%s_%s" % (cname, arith_name)] = {
                "frames": int(fr.sum()), "ids": int(B * T), "ms_align": round(ams, 4), "ms_convert_same_audio": round(vms, 4),
                "ratio_align_to_convert": round(ams / vms, 4), "kernel_ms_profiled": round(tot, 4), "align_logp_us": round(1e3 * lp, 2),
                "align_mas_us": round(1e3 * mas, 2), "share": {"align_logp": round(lp / tot, 4), "align_mas": round(mas / tot, 4)},
                "mas_us_per_frame_step": round(1e3 * mas / L, 4),
                "rounds_ms_align": [round(t, 4) for t in times["align"]], "rounds_ms_vc": [round(t, 4) for t in times["vc"]]}
        # the long case: once warm, once timed, once profiled
        m.align_batch(pcm_long, ids_long, speakers=3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d, fr, sc = m.align_batch(pcm_long, ids_long, speakers=3)
        ms = (time.perf_counter() - t0) * 1e3
        m.prof_enable(True)
        m.prof_reset()
        m.align_batch(pcm_long, ids_long, speakers=3)
        rep = m.prof_report()
        m.prof_enable(False)
        tot, lp, mas = align_kernels(rep)
        res["long_%s" % arith_name] = {"seconds": a.long_seconds, "frames": int(fr[0]), "ids": int(ids_long.shape[1]), "ms_align": round(ms, 3),
                                       "kernel_ms_profiled": round(tot, 3), "align_logp_us": round(1e3 * lp, 1), "align_mas_us": round(1e3 * mas, 1),
                                       "mas_us_per_frame_step": round(1e3 * mas / int(fr[0]), 4), "durations_sum": int(d.sum())}
    m.close()
    print(json.dumps({"tool": "align_bench", "model": "FULL synthetic, 109 speakers, posterior 513 bins x 16 layers", "seconds": a.seconds,
                      "frames_per_utt": L, "ids_per_utt": T, "results": res}))


if __name__ == "__main__":
    main()
