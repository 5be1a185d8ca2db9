"""Cost of speaker conditioning on the FULL multi-speaker synthetic model (109 speakers, embedding 256): batch 64 x 128 ids with 64
distinct speakers against the same ids with speaker -1, and batch 1 (speaker 7 against -1), in fp32 and f16. ms per call (wall clock
around vits_model_process_batch, PCM left on the device), median of interleaved rounds; prints one JSON line. Speakers change the
predicted durations, i.e. the amount of work: the overhead of the conditioning itself is measured with every id pinned to 2 frames
(fixed_duration, equal work), the predicted-duration figures are reported beside it with their frame counts.
usage: python tools/speaker_bench.py [--rounds 5] [--steps 4] [--pinned 1]"""
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
    ap.add_argument("--pinned", type=int, default=1, help="1: every id lasts 2 frames (equal work with and without speakers); 0: predicted durations")
    a = ap.parse_args()
    pkg = load_package()
    import torch
    out_dev = torch.empty(64 * 128 * 12 * 256, dtype=torch.float32, device="cuda")
    m = pkg.Model(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_FULL | pkg.SYNTH_SPEAKERS))
    ids64 = pkg.synth_ids(64, 128)
    ids1 = ids64[:1]
    cases = {"b64": (ids64, np.arange(64, dtype=np.int32) + 3), "b1": (ids1, np.array([7], np.int32))}
    res = {}
    for arith_name, arith in (("f32", pkg.ARITH_F32), ("f16", pkg.ARITH_F16)):
        m.set_arith(arith)
        for cname, (ids, spk) in cases.items():
            B = ids.shape[0]
            steps = a.steps if B > 1 else 10 * a.steps
            times = {"none": [], "speakers": []}
            fixed = 2 if a.pinned else 0
            for _ in range(2):  # warm-up: arenas, weight copies of the latency kernels
                for s in (None, spk):
                    m.process_batch(ids, noise_seed=5, speaker_ids=s, out_device=out_dev.data_ptr(), out_device_stride=128 * 12 * 256,
                                    skip_host_copy=True, keep_pcm=False, fixed_duration=fixed)
            frames = {}
            for _ in range(a.rounds):
                for label, s in (("none", np.full(B, -1, np.int32)), ("speakers", spk)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(steps):
                        _, _, fr = m.process_batch(ids, noise_seed=5, speaker_ids=s, out_device=out_dev.data_ptr(), out_device_stride=128 * 12 * 256,
                                                   skip_host_copy=True, keep_pcm=False, fixed_duration=fixed)
                    frames[label] = int(fr.sum())
                    torch.cuda.synchronize()
                    times[label].append((time.perf_counter() - t0) * 1e3 / steps)
            none, spk_ms = float(np.median(times["none"])), float(np.median(times["speakers"]))
            res["%s_%s_%s" % (cname, arith_name, "pinned" if fixed else "predicted")] = {
                                                  "frames_no_speaker": frames["none"], "frames_speakers": frames["speakers"],
                                                  "ms_no_speaker": round(none, 4), "ms_speakers": round(spk_ms, 4),
                                                  "overhead_pct": round(100.0 * (spk_ms / none - 1.0), 2),
                                                  "rounds_ms_no_speaker": [round(t, 4) for t in times["none"]],
                                                  "rounds_ms_speakers": [round(t, 4) for t in times["speakers"]]}
    m.close()
    print(json.dumps({"tool": "speaker_bench", "model": "FULL synthetic, 109 speakers, E=256", "ids": 128, "results": res}))


if __name__ == "__main__":
    main()
