"""Cost of voice conversion (vits_model_convert_batch) on the FULL synthetic model with speakers and posterior encoder (109 speakers, 513 bins,
16 posterior WaveNet layers): batch 64 and batch 1 at ~2.3 s per utterance, 64 distinct (src, tgt) pairs, fp32 and f16, PCM in from the host
and out left on the device. ms per call (wall clock around the call), median of interleaved rounds, against a text-to-speech call of about
the same total frames (every id pinned to 2 frames: fixed_duration). A profiled pass gives each new phase's share of the kernel time (the
forward flow runs the same kernels as the reverse one: half of the flow's kernel time) and the spectrogram kernel against its byte floor.
Prints one JSON line.
usage: python tools/vc_bench.py [--rounds 5] [--steps 4] [--seconds 2.3] [--hbm-tbs 8.0]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from conftest import load_package  # noqa: E402


def signals(B, n, seed=3):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    out = np.zeros((B, n), np.float32)
    for b in range(B):
        y = sum(rng.uniform(0.2, 1.0) / h * np.sin(2 * np.pi * rng.uniform(90, 260) * h * t) for h in range(1, 6)) + 0.1 * rng.standard_normal(n)
        out[b] = 0.9 * y / np.abs(y).max()
    return out


def phase_shares(report):
    ks = report["kernels"]
    tot = sum(k["ms"] for k in ks) or 1.0
    pick = lambda f: sum(k["ms"] for k in ks if f(k["name"]))
    spec = [k for k in ks if k["name"].startswith("spectrogram")]
    flow = pick(lambda n: n.startswith("flow_"))
    post = pick(lambda n: n.startswith("post_") or n.startswith("posterior_sample"))
    return tot, {"spectrogram": pick(lambda n: n.startswith("spectrogram")) / tot, "posterior": post / tot, "flow_forward": 0.5 * flow / tot}, spec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--seconds", type=float, default=2.3)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM bandwidth of the byte floor (TB/s)")
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
    src64 = np.arange(64, dtype=np.int32)
    tgt64 = (np.arange(64, dtype=np.int32) * 7 + 13) % 109
    T = (L + 1) // 2  # TTS at equal frames: T ids x 2 frames
    ids64 = pkg.synth_ids(64, T)
    cases = {"b64": (pcm64, src64, tgt64, ids64), "b1": (pcm64[:1], src64[:1], tgt64[:1], ids64[:1])}
    res = {}
    for arith_name, arith in (("f32", pkg.ARITH_F32), ("f16", pkg.ARITH_F16)):
        m.set_arith(arith)
        for cname, (pcm, src, tgt, ids) in cases.items():
            B = pcm.shape[0]
            steps = a.steps if B > 1 else 10 * a.steps
            vc = lambda: m.convert_batch(pcm, src=src, tgt=tgt, noise_seed=5, out_device=out_dev.data_ptr(), out_device_stride=S, skip_host_copy=True,
                                         keep_pcm=False)
            tts = lambda: m.process_batch(ids, noise_seed=5, speaker_ids=tgt, fixed_duration=2, out_device=out_dev.data_ptr(), out_device_stride=S,
                                          skip_host_copy=True, keep_pcm=False)
            for _ in range(2):
                vc()
                tts()
            times = {"vc": [], "tts": []}
            frames = {}
            for _ in range(a.rounds):
                for label, fn in (("vc", vc), ("tts", tts)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(steps):
                        fr = fn()[2]
                    torch.cuda.synchronize()
                    times[label].append((time.perf_counter() - t0) * 1e3 / steps)
                    frames[label] = int(fr.sum())
            m.prof_enable(True)
            m.prof_reset()
            vc()
            rep = m.prof_report()
            m.prof_enable(False)
            tot, shares, spec = phase_shares(rep)
            vms, tms = float(np.median(times["vc"])), float(np.median(times["tts"]))
            sb = sum(k["bytes"] for k in spec)
            sms = sum(k["ms"] for k in spec)
            res["%s_%s" % (cname, arith_name)] = {
                "frames_vc": frames["vc"], "frames_tts": frames["tts"], "ms_vc": round(vms, 4), "ms_tts_equal_frames": round(tms, 4),
                "ratio_vc_to_tts": round(vms / tms, 4), "kernel_ms_profiled": round(tot, 4),
                "share": {k: round(v, 4) for k, v in shares.items()},
                "spectrogram_us": round(1e3 * sms, 2), "spectrogram_bytes": int(sb), "spectrogram_floor_us": round(sb / (a.hbm_tbs * 1e12) * 1e6, 2),
                "rounds_ms_vc": [round(t, 4) for t in times["vc"]], "rounds_ms_tts": [round(t, 4) for t in times["tts"]]}
    m.close()
    print(json.dumps({"tool": "vc_bench", "model": "FULL synthetic, 109 speakers, posterior 513 bins x 16 layers", "seconds": a.seconds,
                      "frames_per_utt": L, "results": res}))


if __name__ == "__main__":
    main()
