"""Cost of delivering the PCM at a stated level (vits_model_set_level, loudness.hip) on the FULL synthetic model in fp32, PCM left on the device: the
benchmark configuration (batch 64 x 128 ids) and batch 1 x 128 ids, without a level and under VITS_LEVEL_LOUDNESS (-23 LUFS, ceiling -1 dB). ms per call
(wall clock around the call), median of interleaved rounds; a profiled pass gives the levelling kernels' own time per call (level_measure: the four
measuring launches as one span; level_scale: the multiply) and their share of the call's kernel time. --limit adds the same call with the true-peak
limiter on (vits_model_set_limiter, limiter.hip; "limit": its launches as one span, in place of the multiply). --edges adds the call without a level and
with the edges stage on (vits_model_set_edges, edges.hip: TRIM_RELATIVE -40 dB, 20 ms kept, 5 ms fades, 50 ms and 150 ms of silence; edges_window, edges_bounds
and edges_apply one span each). --join adds vits_model_process_joined (join.hip: join_offsets and join_apply one span each) on the same batch: every utterance
in one track (join_g1) and every utterance its own track (join_gB) without a level, against "none", and one track under VITS_LEVEL_LOUDNESS
(join_g1_loudness: the programme measured as one row), against "loudness". Prints one JSON line.
usage: python tools/level_bench.py [--rounds 5] [--steps 4] [--ids 128] [--limit] [--edges] [--join]"""
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
    ap.add_argument("--limit", action="store_true", help="also time VITS_LEVEL_LOUDNESS with VITS_LIMIT_TRUE_PEAK")
    ap.add_argument("--edges", action="store_true", help="also time VITS_LEVEL_NONE with the edges stage on (VITS_EDGES_TRIM_RELATIVE)")
    ap.add_argument("--join", action="store_true", help="also time vits_model_process_joined: one track, every utterance its own track, one track under VITS_LEVEL_LOUDNESS")
    a = ap.parse_args()
    pkg = load_package()
    import torch
    m = pkg.Model(pkg.synth_model_bytes(0x5EED, pkg.SYNTH_FULL))
    kinds = (("none", pkg.LEVEL_NONE), ("loudness", pkg.LEVEL_LOUDNESS)) + ((("limit", pkg.LEVEL_LOUDNESS),) if a.limit else ()) + ((("edges", pkg.LEVEL_NONE),) if a.edges else ())
    if a.join:
        kinds += (("join_g1", pkg.LEVEL_NONE), ("join_gB", pkg.LEVEL_NONE), ("join_g1_loudness", pkg.LEVEL_LOUDNESS))
    edges = dict(mode=pkg.EDGES_TRIM_RELATIVE, threshold_db=-40.0, keep_head_ms=20.0, keep_tail_ms=20.0, fade_in_ms=5.0, fade_out_ms=5.0, lead_ms=50.0, tail_ms=150.0) if a.edges else None
    pads = sum(pkg.edges_plan(m.sampling_rate, **edges)[5:7]) if a.edges else 0  # (the stage's rows are checked against N + Pl + Pt)
    res = {}
    for batch in (64, 1):
        ids = pkg.synth_ids(batch, a.ids)
        m.set_level(pkg.LEVEL_NONE)
        stride = int(m.process_batch(ids, noise_seed=5, frames_only=True)[1].max()) + 64 + pads
        out_dev = torch.empty(batch * stride, dtype=torch.float32, device="cuda")

        def call(kind, name):
            m.set_limiter(pkg.LIMIT_TRUE_PEAK if name == "limit" else pkg.LIMIT_OFF)
            if a.edges:
                m.set_edges(**(edges if name == "edges" else dict(mode=pkg.EDGES_OFF)))
            m.set_level(kind, -23.0, -1.0)
            if name.startswith("join"):
                # (the same buffer: one row of batch * stride samples, or batch rows)
                one = "_g1" in name
                return m.process_joined(ids, track=None if one else np.arange(batch), noise_seed=5, out_device=out_dev.data_ptr(),
                                        out_device_stride=batch * stride if one else stride, skip_host_copy=True, keep_pcm=False)
            return m.process_batch(ids, noise_seed=5, out_device=out_dev.data_ptr(), out_device_stride=stride, skip_host_copy=True, keep_pcm=False)

        for n, k in kinds:
            call(k, n)
        times = {n: [] for n, _ in kinds}
        for _ in range(a.rounds):
            for n, k in kinds:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    call(k, n)
                torch.cuda.synchronize()
                times[n].append((time.perf_counter() - t0) * 1e3 / a.steps)
        base = float(np.median(times["none"]))
        for n, k in kinds:
            m.prof_enable(True)
            m.prof_reset()
            _, lengths, _ = call(k, n)
            rep = m.prof_report()
            m.prof_enable(False)
            ks = rep["kernels"]
            tot = sum(x["ms"] for x in ks) or 1.0
            lv = {x["name"]: x for x in ks if x["name"].startswith(("level_", "edges_", "join_")) or x["name"] == "limit"}
            lms = sum(x["ms"] for x in lv.values())
            ms = float(np.median(times[n]))
            res["b%d_%s" % (batch, n)] = {
                "ms_per_call": round(ms, 4), "vs_no_level": round(ms / base, 4), "samples": int(lengths.sum()), "kernel_ms": round(tot, 4),
                "level_us": {name: round(1e3 * x["ms"], 2) for name, x in lv.items()}, "level_share_of_kernel_time": round(lms / tot, 5),
                "levels_row0": None if m.last_levels() is None else [float(v) for v in m.last_levels()[0]],
                "limits_row0": None if m.last_limits() is None else [float(v) for v in m.last_limits()[0]],
                **({"edges_row0": None if m.last_edges() is None else [int(v) for v in m.last_edges()[0]]} if a.edges else {}),
                **({"joins_last_row": None if m.last_joins() is None else [int(v) for v in m.last_joins()[-1]]} if a.join else {}), "rounds_ms": [round(t, 4) for t in times[n]]}
        del out_dev
    m.close()
    print(json.dumps({"tool": "level_bench", "model": "FULL synthetic", "arith": "f32", "ids": a.ids, "results": res}))


if __name__ == "__main__":
    main()
