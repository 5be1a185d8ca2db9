"""Cost of delivering the PCM at another sample rate (vits_model_set_rates, resample.hip) on the FULL synthetic model: batch 64 x 128 ids, PCM left on the
device, at the model's own 16 kHz and at 16 -> 48 kHz, 16 -> 8 kHz and 16 -> 44.1 kHz, in fp32 and f16 arithmetic. ms per call (wall clock around the call),
median of interleaved rounds: the 16 kHz case queues no resampling kernel and is the point of comparison. A profiled pass gives the resample_out kernel's
own time per call, its share of the call's kernel time and its byte floor (the model-rate waveform read once, the delivered PCM written once).
Prints one JSON line.
usage: python tools/resample_bench.py [--rounds 5] [--steps 4] [--batch 64] [--ids 128] [--hbm-tbs 8.0]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from conftest import load_package  # noqa: E402

RATES = (0, 48000, 8000, 44100)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--ids", type=int, default=128)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM bandwidth of the byte floor (TB/s)")
    a = ap.parse_args()
    pkg = load_package()
    import torch
    m = pkg.Model(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_FULL))
    ids = pkg.synth_ids(a.batch, a.ids)
    res = {}
    for arith_name, arith in (("f32", pkg.ARITH_F32), ("f16", pkg.ARITH_F16)):
        m.set_arith(arith)
        # one buffer for every rate: sized by the longest delivery (48 kHz)
        m.set_rates(0, 48000)
        stride = int(m.process_batch(ids, noise_seed=5, frames_only=True)[1].max()) + 64
        out_dev = torch.empty(a.batch * stride, dtype=torch.float32, device="cuda")

        def call(rate):
            m.set_rates(0, rate)
            return m.process_batch(ids, noise_seed=5, out_device=out_dev.data_ptr(), out_device_stride=stride, skip_host_copy=True, keep_pcm=False)

        for r in RATES:
            call(r)
        times = {r: [] for r in RATES}
        for _ in range(a.rounds):
            for r in RATES:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    call(r)
                torch.cuda.synchronize()
                times[r].append((time.perf_counter() - t0) * 1e3 / a.steps)
        base = float(np.median(times[0]))
        for r in RATES:
            m.prof_enable(True)
            m.prof_reset()
            _, lengths, frames = call(r)
            rep = m.prof_report()
            m.prof_enable(False)
            ks = rep["kernels"]
            tot = sum(k["ms"] for k in ks) or 1.0
            rs = [k for k in ks if k["name"].startswith("resample_")]
            rms, rbytes = sum(k["ms"] for k in rs), sum(k["bytes"] for k in rs)
            ms = float(np.median(times[r]))
            res["%s_%s" % (arith_name, r or "model_rate")] = {
                "ms_per_call": round(ms, 4), "vs_model_rate": round(ms / base, 4), "frames": int(frames.sum()), "samples_out": int(lengths.sum()),
                "resample_launches": sum(k["calls"] for k in rs), "resample_us": round(1e3 * rms, 2), "resample_share_of_kernel_time": round(rms / tot, 5),
                "resample_bytes": int(rbytes), "resample_floor_us": round(rbytes / (a.hbm_tbs * 1e12) * 1e6, 2),
                "rounds_ms": [round(t, 4) for t in times[r]]}
        del out_dev
    m.close()
    print(json.dumps({"tool": "resample_bench", "model": "FULL synthetic", "batch": a.batch, "ids": a.ids, "results": res}))


if __name__ == "__main__":
    main()
