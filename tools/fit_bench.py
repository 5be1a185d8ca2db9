"""Cost of a stated duration (vits_model_set_fit, fit.hip) on the FULL synthetic model in fp32, PCM left on the device: the benchmark configuration (batch 64 x
128 ids) and batch 1 x 128 ids. "off": no fit given. "rate": every utterance at the speaking rate 0.8. "fit": every utterance its own group, fitted to the
frames the "rate" call gave it, so the two calls make the same frames and their difference is the stage: the kernel, its 40 bytes per group on the way to the
host beside the frame counts, and the call staying whole instead of being split across the front-end stream ("rate_whole" is the "rate" call with
vocoder_chunk_frames = 1 << 20, which keeps it whole too). "fit_total": the batch as one group fitted to the same total. ms per call (wall clock around the
call), median of interleaved rounds; a profiled pass gives the kernel's own time per call ("fit_durations"). Prints one JSON line.
usage: python tools/fit_bench.py [--rounds 7] [--steps 4] [--ids 128]"""
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--ids", type=int, default=128)
    a = ap.parse_args()
    pkg = load_package()
    import torch
    m = pkg.Model(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_FULL))
    has_fit = hasattr(pkg.Model, "set_fit")  # (the same tool times the commit in front of the stage: "off" and "rate" only)
    res = {}
    for batch in (64, 1):
        ids = pkg.synth_ids(batch, a.ids)
        _, lengths, frames = m.process_batch(ids, noise_seed=5, frames_only=True, speaking_rate=0.8)
        stride = int(lengths.max()) + 4096
        out_dev = torch.empty(batch * stride, dtype=torch.float32, device="cuda")
        cases = [("off", {}), ("rate", dict(speaking_rate=0.8)), ("rate_whole", dict(speaking_rate=0.8, vocoder_chunk_frames=1 << 20))]
        if has_fit:
            cases += [("fit", dict(fit=dict(targets=frames))), ("fit_total", dict(fit=int(frames.sum())))]

        def call(kw):
            return m.process_batch(ids, noise_seed=5, out_device=out_dev.data_ptr(), out_device_stride=stride, skip_host_copy=True, keep_pcm=False, **kw)

        for _, kw in cases:
            call(kw)
        times = {n: [] for n, _ in cases}
        for _ in range(a.rounds):
            for n, kw in cases:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    call(kw)
                torch.cuda.synchronize()
                times[n].append((time.perf_counter() - t0) * 1e3 / a.steps)
        for n, kw in cases:
            m.prof_enable(True)
            m.prof_reset()
            _, lens, fr = call(kw)
            rep = m.prof_report()
            m.prof_enable(False)
            ks = rep["kernels"]
            tot = sum(x["ms"] for x in ks) or 1.0
            ft = sum(x["ms"] for x in ks if x["name"] == "fit_durations")
            rows = m.last_fit() if has_fit else None
            res["b%d_%s" % (batch, n)] = {
                "ms_per_call": round(float(np.median(times[n])), 4), "samples": int(lens.sum()), "frames": int(fr.sum()), "kernel_ms": round(tot, 4),
                "fit_us": round(1e3 * ft, 2), "fit_share_of_kernel_time": round(ft / tot, 6),
                "fit_status": None if rows is None else sorted(set(int(s) for s in rows[:, 5])),
                "fit_remainders": None if rows is None else int((rows[:, 4] > 0).sum()), "rounds_ms": [round(t, 4) for t in times[n]]}
        del out_dev
    m.close()
    print(json.dumps({"tool": "fit_bench", "model": "FULL synthetic", "arith": "f32", "ids": a.ids, "results": res}))


if __name__ == "__main__":
    main()
