"""Cost of the voice registry (vits_model_add_voices) on VITS_SYNTH_FULL | VITS_SYNTH_SPEAKERS | VITS_SYNTH_POSTERIOR with conversion prepared
(109 file speakers, embedding 256; two effective-bias tables: 6,848 + 6,144 floats per row). Needs the GPU. Prints one JSON line:

  add_voices_ms        wall clock of one add_voices(n) call for n = 1, 64, 1024 (upload + one launch per table + the synchronisation that ends
                       the call; the registry was cleared before, its capacity and the resident conditioning convs kept), median of 5
  kernel_us_per_row    from a kernel trace of a child process (rocprofv3 --kernel-trace): voice_rows_kernel, both tables, per voice, for each n
                       (median of 5), beside the load-time build it replaces — every speaker_bias_kernel launch of load + prepare_conversion
                       (18 + 16 segments) over the 110 rows they fill
  process_batch_ms     batch 64 x 128 ids, f16, 64 file speakers against the same batch with 64 voices that hold those speakers' embeddings
                       (the same work, bit for bit), interleaved rounds, medians and the spread of the rounds

Conditions (exit status 1 if one fails): the per-row kernel time at n = 64 and n = 1024 is not above the load-time build's; the two process_batch
medians agree within the larger of the two spreads (max - min of the rounds).
usage: python tools/voices_bench.py [--rounds 5] [--steps 4] [--no-trace]"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from conftest import load_package  # noqa: E402

NS = (1, 64, 1024)
REPS = 5
ARCH_FLAGS = ("SYNTH_FULL", "SYNTH_SPEAKERS", "SYNTH_POSTERIOR")


def open_model(pkg):
    arch = 0
    for f in ARCH_FLAGS:
        arch |= getattr(pkg, f)
    m = pkg.Model(pkg.synth_model_bytes(0x5EED, arch))
    m.prepare_conversion()
    return m


def registrations(m, vecs, clock=None):
    """REPS x add_voices(n) for every n, the registry cleared before each; ms per call when a clock is given"""
    out = {}
    for n in NS:
        times = []
        for _ in range(REPS):
            m.clear_voices()
            t0 = time.perf_counter()
            m.add_voices(vecs[:n])
            times.append((time.perf_counter() - t0) * 1e3)
        out[n] = times
    m.clear_voices()
    return out


def child():
    """what the kernel trace sees: the load-time builds (speaker_bias_kernel), then 3 x REPS registrations = 2 voice_rows_kernel launches each"""
    pkg = load_package()
    m = open_model(pkg)
    vecs = np.random.default_rng(1).standard_normal((max(NS), m.speaker_embedding_size)).astype(np.float32)
    registrations(m, vecs)
    m.close()


def traced_kernels():
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    with tempfile.TemporaryDirectory() as d:
        cmd = [rocprof, "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--child"]
        run = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if run.returncode != 0:
            raise RuntimeError("the traced child failed: " + run.stderr[-2000:])
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as f:
                for r in csv.DictReader(f):
                    r = {k.lower(): v for k, v in r.items()}
                    rows.append((int(r["start_timestamp"]), int(r["end_timestamp"]), r["kernel_name"]))
    rows.sort()
    load = [e - s for s, e, name in rows if "speaker_bias_kernel" in name]
    voice = [e - s for s, e, name in rows if "voice_rows_kernel" in name]
    if not load or len(voice) != 2 * REPS * len(NS):
        raise RuntimeError("kernel trace: %d speaker_bias_kernel and %d voice_rows_kernel launches (expected 34 and %d)" % (len(load), len(voice), 2 * REPS * len(NS)))
    res = {"load_build_launches": len(load), "load_build_rows": 110, "load_build_us_per_row": sum(load) / 1e3 / 110}
    for i, n in enumerate(NS):
        per_call = [voice[2 * (i * REPS + k)] + voice[2 * (i * REPS + k) + 1] for k in range(REPS)]  # main table + the posterior's
        res["voice_rows_us_per_row_n%d" % n] = float(np.median(per_call)) / 1e3 / n
        res["voice_rows_us_per_call_n%d" % n] = float(np.median(per_call)) / 1e3
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--no-trace", action="store_true", help="skip the kernel trace (and its condition)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child()
    failed = []
    kernels = None
    if not a.no_trace:
        kernels = traced_kernels()  # (before this process opens the device)
        for n in (64, 1024):
            if kernels["voice_rows_us_per_row_n%d" % n] > kernels["load_build_us_per_row"]:
                failed.append("voice_rows_kernel at n = %d costs more per row than the load-time build" % n)
    pkg = load_package()
    import torch
    m = open_model(pkg)
    vecs = np.random.default_rng(1).standard_normal((max(NS), m.speaker_embedding_size)).astype(np.float32)
    registrations(m, vecs)  # warm: resident convs, table capacity
    add_ms = {str(n): {"median": round(float(np.median(t)), 4), "rounds": [round(x, 4) for x in t]} for n, t in registrations(m, vecs, True).items()}
    # the same batch with 64 file speakers and with 64 voices that hold their embeddings
    ids = pkg.synth_ids(64, 128)
    spk = np.arange(64, dtype=np.int32) + 3
    voices = np.array(m.add_voices(np.stack([m.speaker_embedding(s) for s in spk])), np.int32)
    out_dev = torch.empty(64 * 128 * 12 * 256, dtype=torch.float32, device="cuda")
    m.set_arith(pkg.ARITH_F16)
    call = lambda s: m.process_batch(ids, noise_seed=5, speaker_ids=s, out_device=out_dev.data_ptr(), out_device_stride=128 * 12 * 256, skip_host_copy=True,
                                     keep_pcm=False)
    frames = {}
    for _ in range(2):
        for label, s in (("speakers", spk), ("voices", voices)):
            frames[label] = int(call(s)[2].sum())
    times = {"speakers": [], "voices": []}
    for _ in range(a.rounds):
        for label, s in (("speakers", spk), ("voices", voices)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                call(s)
            torch.cuda.synchronize()
            times[label].append((time.perf_counter() - t0) * 1e3 / a.steps)
    m.close()
    med = {k: float(np.median(v)) for k, v in times.items()}
    spread = {k: float(max(v) - min(v)) for k, v in times.items()}
    if frames["speakers"] != frames["voices"]:
        failed.append("the two batches differ in frames")
    if abs(med["speakers"] - med["voices"]) > max(spread.values()):
        failed.append("process_batch medians differ by more than the spread of the rounds")
    name = ctypes_device_name(pkg)
    print(json.dumps({"tool": "voices_bench", "device": name, "model": "FULL synthetic, 109 speakers, E=256, conversion prepared", "add_voices_ms": add_ms,
                      "kernel_us_per_row": kernels,
                      "process_batch_ms": {"batch": 64, "ids": 128, "arith": "f16", "frames": frames["speakers"],
                                           "median_speakers": round(med["speakers"], 4), "median_voices": round(med["voices"], 4),
                                           "spread_speakers": round(spread["speakers"], 4), "spread_voices": round(spread["voices"], 4),
                                           "rounds_speakers": [round(t, 4) for t in times["speakers"]], "rounds_voices": [round(t, 4) for t in times["voices"]]},
                      "conditions_failed": failed}))
    return 1 if failed else 0


def ctypes_device_name(pkg):
    import ctypes as C
    buf = C.create_string_buffer(256)
    cu, mhz, hbm = C.c_int32(), C.c_int32(), C.c_int64()
    return buf.value.decode() if pkg.lib().vits_device_info(buf, 256, C.byref(cu), C.byref(mhz), C.byref(hbm)) == 0 else "unknown"


if __name__ == "__main__":
    sys.exit(main())
