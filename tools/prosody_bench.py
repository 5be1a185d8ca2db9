"""Cost of the per-utterance prosody arrays on the FULL synthetic model: batch 64 x 128 ids (and batch 1) with speaking_rates,
noise_scales and noise_scale_durations holding the model's own values (so the work, the frames and the PCM are those of the call without
arrays), durations_out on or off, against the same call with NULL arrays, in fp32 and f16. ms per call (wall clock around
vits_model_process_batch, PCM left on the device), median of interleaved rounds; prints one JSON line.
usage: python tools/prosody_bench.py [--rounds 5] [--steps 4]"""
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
    a = ap.parse_args()
    pkg = load_package()
    import torch
    out_dev = torch.empty(64 * 128 * 12 * 256, dtype=torch.float32, device="cuda")
    m = pkg.Model(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_FULL))
    rate, ns, nsd = m.get_prosody()
    ids64 = pkg.synth_ids(64, 128)
    res = {}
    for arith_name, arith in (("f32", pkg.ARITH_F32), ("f16", pkg.ARITH_F16)):
        m.set_arith(arith)
        for cname, ids in (("b64", ids64), ("b1", ids64[:1])):
            B = ids.shape[0]
            steps = a.steps if B > 1 else 10 * a.steps
            dout = np.zeros(ids.shape, np.int32)
            variants = {"null": {}, "arrays": dict(speaking_rate=np.full(B, rate, np.float32), noise_scale=np.full(B, ns, np.float32),
                                                   noise_scale_duration=np.full(B, nsd, np.float32)),
                        "arrays_durations_out": dict(speaking_rate=np.full(B, rate, np.float32), noise_scale=np.full(B, ns, np.float32),
                                                     noise_scale_duration=np.full(B, nsd, np.float32), durations_out=dout)}
            call = lambda kw: m.process_batch(ids, noise_seed=5, out_device=out_dev.data_ptr(), out_device_stride=128 * 12 * 256, skip_host_copy=True,
                                              keep_pcm=False, **kw)
            for _ in range(2):  # warm-up: arenas, weight copies of the latency kernels
                for kw in variants.values():
                    call(kw)
            times, frames = {k: [] for k in variants}, {}
            for _ in range(a.rounds):
                for label, kw in variants.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(steps):
                        _, _, fr = call(kw)
                    torch.cuda.synchronize()
                    times[label].append((time.perf_counter() - t0) * 1e3 / steps)
                    frames[label] = int(fr.sum())
            assert len(set(frames.values())) == 1, frames
            med = {k: float(np.median(v)) for k, v in times.items()}
            res["%s_%s" % (cname, arith_name)] = {"frames": frames["null"], **{"ms_" + k: round(v, 4) for k, v in med.items()},
                                                  **{"overhead_pct_" + k: round(100.0 * (med[k] / med["null"] - 1.0), 2) for k in variants if k != "null"},
                                                  **{"rounds_ms_" + k: [round(t, 4) for t in v] for k, v in times.items()}}
    m.close()
    print(json.dumps({"tool": "prosody_bench", "model": "FULL synthetic", "ids": 128, "results": res}))


if __name__ == "__main__":
    main()
