"""Cost of the deterministic duration predictor (dp_det.hip) on the FULL synthetic model against the stochastic one: stage one alone (a frames_only call: text
encoder + duration predictor + the frame-count read) and the whole call, at batch 1 x 128 ids and batch 64 x 128 ids, fp32 and f16 (the predictor itself is fp32
in both). Five handles: the stochastic model; the deterministic model as shipped (the planner's tile); with VITS_NO_DP_DET_FUSE (the un-fused sequence of six
launches); with the 16-token tile forced (VITS_DP_DET_LAT_MAX_BLOCKS huge) and with the wide tile forced (= 0). ms per call (wall clock around the call),
MEDIANS of interleaved rounds, with the rounds' own spread (max - min) beside them: a difference below the spread is no difference. A profiled pass gives the
predictor's own kernel time. The whole-call times of the two model kinds are not comparable frame for frame (other durations: `frames`). Prints one JSON line.
usage: python tools/detdp_bench.py [--rounds 7] [--steps 2] [--rotate N] [--reverse]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from conftest import load_package  # noqa: E402

DP_KERNELS = ("dp_det_fused", "dp_det_unfused")


def load(pkg, flags, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return pkg.Model(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_FULL | flags))  # (the knobs are read at load)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--rotate", type=int, default=0, help="time the handles in an order rotated by this many places (a difference that follows the position, not the handle, is the bench's)")
    ap.add_argument("--reverse", action="store_true", help="the opposite order")
    a = ap.parse_args()
    pkg = load_package()
    import torch
    det = pkg.SYNTH_DETERMINISTIC
    handles = {
        "stochastic": load(pkg, 0, {}),
        "det": load(pkg, det, {}),
        "det_unfused": load(pkg, det, {"VITS_NO_DP_DET_FUSE": "1"}),
        "det_tile16": load(pkg, det, {"VITS_DP_DET_LAT_MAX_BLOCKS": "100000000"}),
        "det_wide": load(pkg, det, {"VITS_DP_DET_LAT_MAX_BLOCKS": "0"}),
    }
    if a.reverse:
        handles = dict(reversed(list(handles.items())))
    if a.rotate:
        items = list(handles.items())
        handles = dict(items[a.rotate % len(items):] + items[:a.rotate % len(items)])
    ids64 = pkg.synth_ids(64, 128)
    res = {}
    for arith_name, arith in (("f32", pkg.ARITH_F32), ("f16", pkg.ARITH_F16)):
        for m in handles.values():
            m.set_arith(arith)
        for cname, ids in (("b1", ids64[:1]), ("b64", ids64)):
            B = ids.shape[0]
            steps = a.steps if B > 1 else 10 * a.steps
            out_dev = None
            calls = {}
            frames = {}
            for name, m in handles.items():
                _, lengths, fr = m.process_batch(ids, noise_seed=5, frames_only=True)
                frames[name] = int(fr.sum())
                S = int(lengths.max()) + 4096
                buf = torch.empty(B * S, dtype=torch.float32, device="cuda")
                calls[name] = {
                    "stage_one": (lambda m=m: m.process_batch(ids, noise_seed=5, frames_only=True)),
                    "call": (lambda m=m, buf=buf, S=S: m.process_batch(ids, noise_seed=5, out_device=buf.data_ptr(), out_device_stride=S, skip_host_copy=True, keep_pcm=False)),
                }
                for fn in calls[name].values():
                    for _ in range(2):
                        fn()
            times = {(n, w): [] for n in handles for w in ("stage_one", "call")}
            for _ in range(a.rounds):
                for what in ("stage_one", "call"):
                    for name in handles:  # interleaved: every handle once per round
                        fn = calls[name][what]
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(steps):
                            fn()
                        torch.cuda.synchronize()
                        times[(name, what)].append((time.perf_counter() - t0) * 1e3 / steps)
            entry = {}
            for name, m in handles.items():
                m.prof_enable(True)
                m.prof_reset()
                calls[name]["stage_one"]()
                rep = m.prof_report()
                m.prof_enable(False)
                ks = rep["kernels"]
                dp_ms = sum(k["ms"] for k in ks if k["name"] in DP_KERNELS) if name != "stochastic" else None
                e = {"frames": frames[name], "stage_one_kernel_ms_profiled": round(sum(k["ms"] for k in ks), 4), "launches_stage_one": int(sum(k["calls"] for k in ks))}
                if dp_ms is not None:
                    e["predictor_us_profiled"] = round(1e3 * dp_ms, 2)
                for what in ("stage_one", "call"):
                    t = times[(name, what)]
                    e["ms_" + what] = round(float(np.median(t)), 4)
                    e["spread_ms_" + what] = round(float(max(t) - min(t)), 4)
                entry[name] = e
            res["%s_%s" % (cname, arith_name)] = entry
    for m in handles.values():
        m.close()
    print(json.dumps({"tool": "detdp_bench", "model": "FULL synthetic, 128 ids per utterance", "rounds": a.rounds, "results": res}))


if __name__ == "__main__":
    main()
