"""p3_hisup_polygons_rings on one GPU at B = 4 and 16, 224 x 224, next to p3_hisup_polygons on the same inputs in the same run:
  blobs                       the inputs of tools/bench_hisup_polygons.py (a dozen building blobs, 120 junctions per class and image; next to no courtyard)
  courtyards                  four 100 x 100 blocks per image with three 20 x 20 holes each: every hole gives a ring
  small_holes                 the same blocks with 6 x 6 holes: every hole is found, flooded and walked (steps G and H), none gives a ring
For each input: `outer` (hip.hisup_polygons_device), `rings` (hip.hisup_polygon_rings_device), `rings_workspace_form` (force_fallback) and the ratio
rings / outer.  rings - outer on `small_holes` is what finding and measuring a hole costs, the rest of rings - outer on `courtyards` is step I with E and F.

    python tools/bench_hisup_rings.py [--batches 4,16] [--iters 50] [--warmup 10] [--out profiles/hisup_rings_bench.json]

Eager launches, every timed call between its own pair of HIP events after warm-up calls; medians (min, max beside them).  Prints one JSON line and writes it."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_hisup_polygons import region_args  # noqa: E402
from bench_hisup_predict import DEV, S, planted, timed  # noqa: E402
from pixelspointspolygons_amd import hip  # noqa: E402


def courtyards(B, hole, seed):
    """remask logits [B, 2, S, S]: four 100 x 100 blocks per image, three hole x hole courtyards in each, the noise of `planted` on top"""
    g = torch.Generator().manual_seed(seed)
    d = torch.full((B, S, S), -3.0)
    for b in range(B):
        for y0 in (6, 118):
            for x0 in (6, 118):
                d[b, y0:y0 + 100, x0:x0 + 100] = 3.0
                for k in range(3):
                    dy, dx = [int(v) for v in torch.randint(0, 8, (2,), generator=g)]
                    y, x = y0 + 8 + dy + 30 * k, x0 + 8 + dx + 30 * (k % 2) + 20 * (k // 2)
                    d[b, y:y + hole, x:x + hole] = -3.0
    d += 0.3 * torch.randn(B, S, S, generator=g)
    return torch.stack([-d / 2, d / 2], 1).to(DEV)


def measure(a, iters, warmup):
    out = hip.hisup_polygon_rings(*a)
    r = {"vertices": out["counts"][0], "rings": out["ring_counts"][0], "ring_vertices": out["ring_counts"][1], "holes": int(out["n_holes"].sum()),
         "regions_with_holes": int(((out["poly_flags"] & 2) != 0).sum())}
    r["outer"] = timed(lambda: hip.hisup_polygons_device(*a), iters, warmup)
    r["rings"] = timed(lambda: hip.hisup_polygon_rings_device(*a), iters, warmup)
    r["rings_workspace_form"] = timed(lambda: hip.hisup_polygon_rings_device(*a, force_fallback=True), iters, warmup)
    r["ratio"] = round(r["rings"]["median_us"] / r["outer"]["median_us"], 3)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4,16")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hisup_rings_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hisup_rings.py measures on the GPU: none visible (no CPU fall-back)")
    res = {"tool": "bench_hisup_rings", "gpu": torch.cuda.get_device_name(0), "size": S, "iters": args.iters, "warmup": args.warmup, "results": {}}
    for B in [int(b) for b in args.batches.split(",")]:
        jloc, joff, remask = planted(B, 120, 4, seed=B)
        r = {}
        for name, logits in (("blobs", remask), ("courtyards", courtyards(B, 20, seed=200 + B)), ("small_holes", courtyards(B, 6, seed=200 + B))):
            a, n_regions = region_args(jloc, joff, logits)
            r[name] = dict(n_regions=n_regions, **measure(a, args.iters, args.warmup))
        res["results"][f"B{B}"] = r
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
