"""p3_hisup_polygons on one GPU at B = 4 and 16, 224 x 224, on the outputs of p3_hisup_junctions + p3_hisup_regions for the planted inputs of
tools/bench_hisup_predict.py (120 junctions per class and image, a dozen building blobs):
  polygons                    the call as forward_val(polygons=True) makes it (default capacity)
  polygons_workspace_form     the same with force_fallback (every region through the workspace slabs)
  until_walk / after_walk     the call cut short right before / right after the single-lane border walk (P3_HISUP_POLY_STOP, a measurement switch of the
                              library): their difference over `polygons` is the share of the walk
  all_foreground              one region per image that fills it: the longest ring of a 224 x 224 image (896 points), workspace form
  junctions_600               the same blobs with 300 junctions per class

    python tools/bench_hisup_polygons.py [--batches 4,16] [--iters 50] [--warmup 10] [--out profiles/hisup_polygons_bench.json]

Eager launches, every timed call between its own pair of HIP events after warm-up calls; medians (min, max beside them).  Prints one JSON line and writes it."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_hisup_predict import DEV, S, planted, timed  # noqa: E402
from pixelspointspolygons_amd import hip  # noqa: E402


def region_args(jloc, joff, remask):
    juncs, _, _, counts = hip.hisup_junctions(jloc, joff)
    reg = hip.hisup_regions(remask)
    return (reg["labels"], reg["n_regions"], reg["bbox"], juncs, counts), reg["n_regions"].tolist()


def stopped(fn, stop, iters, warmup):
    os.environ["P3_HISUP_POLY_STOP"] = str(stop)
    try:
        return timed(fn, iters, warmup)
    finally:
        del os.environ["P3_HISUP_POLY_STOP"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4,16")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hisup_polygons_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hisup_polygons.py measures on the GPU: none visible (no CPU fall-back)")
    res = {"tool": "bench_hisup_polygons", "gpu": torch.cuda.get_device_name(0), "size": S, "iters": args.iters, "warmup": args.warmup, "results": {}}
    for B in [int(b) for b in args.batches.split(",")]:
        r = {}
        jloc, joff, remask = planted(B, 120, 4, seed=B)
        a, r["n_regions"] = region_args(jloc, joff, remask)
        call = lambda: hip.hisup_polygons_device(*a)
        out = hip.hisup_polygons(*a)
        flags = out["poly_flags"]
        r["vertices"], r["longest_polygon"] = out["counts"]
        r["junction_polygons"], r["regions_with_holes"], r["no_polygon"] = [int(((flags & bit) != 0).sum()) for bit in (1, 2, 4)]
        r["polygons"] = timed(call, args.iters, args.warmup)
        r["polygons_workspace_form"] = timed(lambda: hip.hisup_polygons_device(*a, force_fallback=True), args.iters, args.warmup)
        r["until_walk"] = stopped(call, 1, args.iters, args.warmup)
        r["after_walk"] = stopped(call, 2, args.iters, args.warmup)
        r["walk_share"] = round(max(r["after_walk"]["median_us"] - r["until_walk"]["median_us"], 0.0) / r["polygons"]["median_us"], 4)
        all_fg = torch.stack([torch.full((B, S, S), -3.0), torch.full((B, S, S), 3.0)], 1).to(DEV)
        f, _ = region_args(jloc, joff, all_fg)
        r["all_foreground"] = timed(lambda: hip.hisup_polygons_device(*f), args.iters, args.warmup)
        r["all_foreground_until_walk"] = stopped(lambda: hip.hisup_polygons_device(*f), 1, args.iters, args.warmup)
        r["all_foreground_after_walk"] = stopped(lambda: hip.hisup_polygons_device(*f), 2, args.iters, args.warmup)
        jl6, jo6, _ = planted(B, 300, 4, seed=100 + B)
        j6, n6 = region_args(jl6, jo6, remask)
        r["junctions_600_counts"] = j6[4].sum(1).tolist()
        r["junctions_600"] = timed(lambda: hip.hisup_polygons_device(*j6), args.iters, args.warmup)
        res["results"][f"B{B}"] = r
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
