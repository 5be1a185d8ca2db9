#!/usr/bin/env python3
"""What a ragged batch pays over an equal-length one, per kernel instantiation of the fp32 vocoder (profiles/ragged_attribution_*.json).

Inputs: two rocprofv3 --kernel-trace CSVs of the same bench command, one with predicted durations (ragged) and one with --pinned N (every utterance N frames
per id), and the frame counts of the ragged run (bench.py --dump-outputs: frames.npy). For every vocoder launch geometry (kernel instantiation x stage) the
script reports the summed duration per real output column (sum over the batch of the stage length), the ratio ragged / pinned of that figure, and — from
the frame counts and the kernel's tile width — how many blocks the launch dispatched and how many of them were past their utterance's end.

    python tools/ragged_attribution.py OUT.json --ragged trace_ragged.csv --pinned trace_pinned.csv --frames frames.npy --pinned-frames 256 --steps-in-trace 7
"""
import argparse
import collections
import csv
import json
import re

import numpy as np


def stage_affine(strides, kernels):
    """stage lengths as len_i = L * mul[i] + add[i] (reference semantics: no crop), as Engine::set_stage_affine"""
    mul, add = [1], [0]
    for s, k in zip(strides, kernels):
        mul.append(mul[-1] * s)
        add.append(add[-1] * s + (k - s))
    return mul, add


def geometry(name):
    """(family, channels or None, tile width, transposed) of a converted kernel instantiation, or None"""
    m = re.search(r"conv_mfma_kernel<(-?\d+), (-?\d+), (\w+), (\d+), (\d+), (\d+), (\d+), (\d+)>", name)
    if m:
        kt, dil, db, wm, wn, mr, nr, epi = m.groups()
        if int(wm) == 4 and int(wn) == 1:
            return None  # the narrow tile: stage one / flow
        return "conv k%s d%s %dx%d%s" % (kt, dil, 32 * int(wm) * int(mr), 32 * int(wn) * int(nr), " convT" if epi == "2" else ""), None, 32 * int(wn) * int(nr), epi == "2"
    m = re.search(r"conv_group(?:_list)?_kernel<(\d+)>", name)
    if m:
        return "group d%s 128x128" % m.group(1), None, 128, False
    m = re.search(r"rbpair32_kernel<(\d+), (\d+), (\d+)>", name)
    if m:
        kt, dil, c = map(int, m.groups())
        bm = (4 // (c // 32)) * (4 if c >= 128 else 2) * 32
        return "rbpair32 k%d d%d" % (kt, dil), c, bm - (kt - 1), False
    m = re.search(r"rbblock32_kernel<(\d+), (\d+)>", name)
    if m:
        c, nr = map(int, m.groups())
        return "rbblock32", c, 4 // (c // 32) * nr * 32 - 24, False
    return None


def launches(trace):
    """{(kernel name, blocks x, y, z): [calls, ns]} of a kernel trace"""
    out = collections.OrderedDict()
    for r in csv.DictReader(open(trace)):
        g = tuple(int(r["Grid_Size_" + a]) // int(r["Workgroup_Size_" + a]) for a in "XYZ")
        e = out.setdefault((r["Kernel_Name"], g), [0, 0])
        e[0] += 1
        e[1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    return out


def reduce(trace, frames, mul, add, channels, steps):
    """per (family, stage): calls per step, us per step, ns per real column, blocks dispatched / empty per launch"""
    rows = {}
    for (name, g), (calls, ns) in launches(trace).items():
        geo = geometry(name)
        if not geo:
            continue
        fam, c, width, convt = geo
        # the stage whose lengths this launch tiles: by channel count for the fused kernels; for the convolutions the one whose dense or compact grid it has
        cand = []
        for i in range(len(mul) - (1 if convt else 0)):
            if c is not None and (i == 0 or channels[i - 1] != c):
                continue
            cols = frames * mul[i] + add[i] + (1 if convt else 0)
            tiles = -(-cols // width)
            B, gx, exist = len(frames), int(tiles.max()), int(tiles.sum())
            # dense grids: conv (tiles, row blocks, utterances [x members of a grouped launch]), fused kernels (tiles, utterances, 1);
            # lists: conv (entries [x members], row blocks, 1), fused kernels (entries, 1, 1)
            if c is None and g[0] == gx and g[2] % B == 0 and g[2] // B in (1, 2, 3):
                cand.append((i, gx * g[2], exist * (g[2] // B), False))
            elif c is not None and g[0] == gx and g[1] == B and g[2] == 1:
                cand.append((i, gx * B, exist, False))
            elif g[2] == 1 and (c is None or g[1] == 1) and g[0] % exist == 0 and g[0] // exist in (1, 2, 3) and (g[0] == exist or "group" in fam):
                cand.append((i, g[0], g[0], True))
        if len(cand) != 1:
            continue  # (a launch of stage one or the flow on a vocoder tile shape)
        i, dispatched, exist, mapped = cand[0]
        out_stage = i + 1 if convt else i
        cols_out = int((frames * mul[out_stage] + add[out_stage]).sum())
        key = "%s | stage %d%s" % (fam, i, "" if c is None else " C%d" % c)
        rows[key] = {"kernel": name.replace("void vits::", "").split("(")[0], "stage": i, "tile_width": width, "launches_per_step": calls / steps, "us_per_step": ns / steps / 1e3,
                     "ns_per_column": ns / steps / cols_out, "row_blocks": g[1], "blocks_dispatched_per_launch": dispatched * g[1] if c is None else dispatched,
                     "blocks_empty_per_launch": (dispatched - exist) * (g[1] if c is None else 1), "empty_fraction": (dispatched - exist) / dispatched, "list": mapped}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--ragged", required=True)
    ap.add_argument("--pinned", required=True)
    ap.add_argument("--frames", required=True, help="frames.npy of the ragged run")
    ap.add_argument("--pinned-frames", type=int, required=True, help="frames per utterance of the pinned run (ids x --pinned)")
    ap.add_argument("--steps-in-trace", type=int, required=True, help="warm-up + timed steps of each traced command")
    ap.add_argument("--strides", default="8,8,2,2")
    ap.add_argument("--kernels", default="16,16,4,4")
    ap.add_argument("--channels", default="256,128,64,32")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    mul, add = stage_affine([int(x) for x in a.strides.split(",")], [int(x) for x in a.kernels.split(",")])
    channels = [int(x) for x in a.channels.split(",")]
    fr = np.load(a.frames).astype(np.int64)
    fp = np.full(len(fr), a.pinned_frames, np.int64)
    R, P = reduce(a.ragged, fr, mul, add, channels, a.steps_in_trace), reduce(a.pinned, fp, mul, add, channels, a.steps_in_trace)
    table = {}
    for k, r in R.items():
        p = P.get(k)
        table[k] = dict(r, pinned_ns_per_column=p["ns_per_column"] if p else None, ragged_over_pinned=r["ns_per_column"] / p["ns_per_column"] if p else None,
                        quantisation_ragged=None, pinned_us_per_step=p["us_per_step"] if p else None)
        # tile quantisation alone: columns the existing tiles span over the real columns, ragged against pinned
        convt = "convT" in k
        i, w = r["stage"], r["tile_width"]
        span = lambda f: float(((-(-(f * mul[i] + add[i] + convt) // w)) * w).sum()) / float((f * mul[i] + add[i] + convt).sum())
        table[k]["quantisation_ragged"] = span(fr) / span(fp)
    by_stage = collections.OrderedDict()
    for k, r in table.items():
        if r["ragged_over_pinned"] is None:
            continue
        s = by_stage.setdefault("stage %d" % r["stage"], {"ragged_us": 0.0, "pinned_us_scaled": 0.0, "quantisation_us": 0.0})
        s["ragged_us"] += r["us_per_step"]
        s["pinned_us_scaled"] += r["us_per_step"] / r["ragged_over_pinned"]
        s["quantisation_us"] += r["us_per_step"] / r["ragged_over_pinned"] * (r["quantisation_ragged"] - 1.0)
    for s in by_stage.values():
        s["ragged_over_pinned"] = s["ragged_us"] / s["pinned_us_scaled"]
        s["penalty_us_per_step"] = s["ragged_us"] - s["pinned_us_scaled"]
        s["of_which_other_than_quantisation_us"] = s["penalty_us_per_step"] - s["quantisation_us"]
    json.dump({"label": a.label, "frames_mean": float(fr.mean()), "frames_min": int(fr.min()), "frames_max": int(fr.max()), "pinned_frames": a.pinned_frames,
               "steps_in_trace": a.steps_in_trace, "note": "ns_per_column = summed kernel time per step / sum over the batch of the stage's output length; ragged_over_pinned compares that "
               "figure between the two runs; quantisation_ragged = (columns spanned by existing tiles / real columns), ragged over pinned: the part of the ratio that partial tiles explain",
               "by_stage": by_stage, "launches": table}, open(a.out, "w"), indent=1)
    for k, s in by_stage.items():
        print(k, {x: round(y, 4) for x, y in s.items()})


if __name__ == "__main__":
    main()
