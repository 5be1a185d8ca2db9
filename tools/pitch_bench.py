"""Cost of a stated pitch (vits_model_set_pitch_ratios, pitch.hip) on the FULL synthetic model in fp32, PCM left on the device: the benchmark configuration (batch
64 x 128 ids) and batch 1 x 128 ids, with the stage off ("off": no ratio given) and at p = 2^(2/12) ("st2") and p = 2 ("oct"). An utterance with ratio p is
spoken p times slower first, so its call makes p times the frames: "slow_st2" and "slow_oct" are the calls at the speaking rate 1 / p WITHOUT the stage, and
the stage's own cost is the pitched call against those. ms per call (wall clock around the call), median of interleaved rounds; a profiled pass gives the
kernel's own time per call ("pitch") and its share of the call's kernel time. Prints one JSON line.
usage: python tools/pitch_bench.py [--rounds 5] [--steps 4] [--ids 128]"""
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
    ap.add_argument("--ids", type=int, default=128)
    a = ap.parse_args()
    pkg = load_package()
    import torch
    m = pkg.Model(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_FULL))
    has_pitch = hasattr(pkg, "pitch_ratio")  # (the same tool times the commit in front of the stage: "off" only)
    rate = m.speaking_rate
    st2, octave = (pkg.pitch_ratio(2), 2.0) if has_pitch else (None, None)
    cases = [("off", None, None)]
    if has_pitch:
        slow = lambda p: float(np.float32(np.float64(np.float32(rate)) / np.float64(np.float32(p))))
        cases += [("st2", st2, None), ("slow_st2", None, slow(st2)), ("oct", octave, None), ("slow_oct", None, slow(octave))]
    res = {}
    for batch in (64, 1):
        ids = pkg.synth_ids(batch, a.ids)
        # (room for the slowest call's rows: twice the frames, and N' <= N)
        stride = 2 * int(m.process_batch(ids, noise_seed=5, frames_only=True)[1].max()) + 4096
        out_dev = torch.empty(batch * stride, dtype=torch.float32, device="cuda")

        def call(p, r):
            kw = {} if p is None else dict(pitch_ratio=p)
            if r is not None:
                kw["speaking_rate"] = r
            return m.process_batch(ids, noise_seed=5, out_device=out_dev.data_ptr(), out_device_stride=stride, skip_host_copy=True, keep_pcm=False, **kw)

        for _, p, r in cases:
            call(p, r)
        times = {n: [] for n, _, _ in cases}
        for _ in range(a.rounds):
            for n, p, r in cases:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    call(p, r)
                torch.cuda.synchronize()
                times[n].append((time.perf_counter() - t0) * 1e3 / a.steps)
        for n, p, r in cases:
            m.prof_enable(True)
            m.prof_reset()
            _, lengths, frames = call(p, r)
            rep = m.prof_report()
            m.prof_enable(False)
            ks = rep["kernels"]
            tot = sum(x["ms"] for x in ks) or 1.0
            pt = sum(x["ms"] for x in ks if x["name"] == "pitch")
            res["b%d_%s" % (batch, n)] = {
                "ms_per_call": round(float(np.median(times[n])), 4), "samples": int(lengths.sum()), "frames": int(frames.sum()), "kernel_ms": round(tot, 4),
                "pitch_us": round(1e3 * pt, 2), "pitch_share_of_kernel_time": round(pt / tot, 5),
                "pitch_row0": None if not has_pitch or m.last_pitch() is None else [int(v) for v in m.last_pitch()[0]], "rounds_ms": [round(t, 4) for t in times[n]]}
        del out_dev
    m.close()
    print(json.dumps({"tool": "pitch_bench", "model": "FULL synthetic", "arith": "f32", "ids": a.ids, "results": res}))


if __name__ == "__main__":
    main()
