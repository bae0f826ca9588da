"""Polygon metrics (IoU / C-IoU / NR, POLIS, chamfer, Hausdorff) on one GPU: 64 images of 224 x 224 with 20 ground-truth buildings and
20 predictions each (18 jittered copies, 2 spurious small rings).
  (a) hip.polygon_metrics_device: p3_polygon_metrics (csrc/poly_metrics.hip) without a read-back, between HIP events: all modes, and each mode alone,
  (b) eval_metrics.polygon_metrics on the host clock: the call with its one read-back,
  (c) the float64 restatement tests/poly_metrics_ref.py on the same input on the host clock, once (numpy on one core: no reference implementation, and no
      speed-up over pycocotools / shapely is claimed - neither is installed), and whether the device equals it.

    python tools/bench_poly_metrics.py [--batch 64] [--buildings 20] [--repeats 20] [--out profiles/poly_metrics_bench.json]

(a) is timed between HIP events, (b) and (c) with the host clock; medians (min, max beside them) after warm-up runs, all in this one process.  The kernels'
own shares come from a kernel trace of this tool (rocprofv3 --kernel-trace --stats -- python tools/bench_poly_metrics.py).  Prints one JSON line and writes
it to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_acm import timed  # noqa: E402
from bench_init_contours import wall  # noqa: E402
from pixelspointspolygons_amd import eval_metrics as E  # noqa: E402
from pixelspointspolygons_amd import hip  # noqa: E402
from tests import poly_metrics_cases as C  # noqa: E402
from tests import poly_metrics_ref as R  # noqa: E402

DEV = "cuda"
S = 224


def scene(batch, buildings, seed):
    """per image `buildings` star-shaped gt rings of 4-8 vertices on a grid of cells, all but two with a prediction jittered by sigma 0.8, and two small
    spurious predictions"""
    rng = np.random.default_rng(seed)
    cols = int(np.ceil(np.sqrt(buildings)))
    rows = -(-buildings // cols)
    cw, ch = S / cols, S / rows
    gt, dt = [], []
    for _ in range(batch):
        g = [C.star(rng, (k % cols + 0.5) * cw + rng.uniform(-2, 2), (k // cols + 0.5) * ch + rng.uniform(-2, 2), int(rng.integers(4, 9)),
                    0.2 * min(cw, ch), 0.42 * min(cw, ch)) for k in range(buildings)]
        d = [C.f32(r + rng.normal(0, 0.8, r.shape)) for r in g[:-2]] + [C.star(rng, rng.uniform(10, S - 10), rng.uniform(10, S - 10), 4, 1.0, 2.5) for _ in range(2)]
        gt.append(g)
        dt.append(d)
    return gt, dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--buildings", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poly_metrics_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_poly_metrics.py measures on the GPU: none visible (no CPU fall-back)")
    gt, dt = scene(args.batch, args.buildings, args.seed)
    g, d = E.pack_rings(gt, DEV), E.pack_rings(dt, DEV)
    found = E.polygon_metrics(d, g, S, S)          # also sizes the workspace
    match = found["pairs"]["match"].cpu().numpy()
    res = {"tool": "bench_poly_metrics", "gpu": torch.cuda.get_device_name(0), "batch": args.batch, "size": S, "repeats": args.repeats, "warmup": args.warmup,
           "gt_rings": int(g["ring_slice"].shape[0]), "dt_rings": int(d["ring_slice"].shape[0]), "gt_vertices": int(g["pos"].shape[0]),
           "dt_vertices": int(d["pos"].shape[0]), "counted_pairs": int((match >= 0).sum()), "status": found["status"],
           "metrics": {k: found[k] for k in E.KEYS}, "launches": {"kernels": 5, "memsets": 1},
           "workspace_bytes": hip.polygon_metrics_workspace_bytes(g["ring_slice"].shape[0], d["ring_slice"].shape[0], args.batch)}

    def device(modes):
        return hip.polygon_metrics_device(g["pos"], g["ring_slice"], g["ring_image"], d["pos"], d["ring_slice"], d["ring_image"], args.batch, S, S, modes)

    res["a_device_all_modes"] = timed(lambda _: device(hip.PM_IOU | hip.PM_POLIS | hip.PM_SAMPLES), args.repeats, args.warmup)
    res["a_device_iou"] = timed(lambda _: device(hip.PM_IOU), args.repeats, args.warmup)
    res["a_device_polis"] = timed(lambda _: device(hip.PM_POLIS), args.repeats, args.warmup)
    res["a_device_chamfer_hausdorff"] = timed(lambda _: device(hip.PM_SAMPLES), args.repeats, args.warmup)
    res["b_polygon_metrics"] = wall(lambda: E.polygon_metrics(d, g, S, S), args.repeats, args.warmup)

    t0 = time.perf_counter()
    want = R.run(gt, dt, S, S)
    res["c_restatement_host_s"] = round(time.perf_counter() - t0, 3)
    samples = [len(R.samples(gt[0][k])) for k in range(len(gt[0]))]
    res["samples_per_gt_ring_image_0"] = {"min": min(samples), "max": max(samples)}
    res["device_equals_the_restatement"] = bool(
        np.array_equal(match, want["match"]) and np.array_equal(found["per_image"]["counts"].cpu().numpy(), want["image_counts"])
        and np.array_equal(found["per_image"]["valid"].cpu().numpy(), want["image_valid"])
        and all(abs(found[k] - want["means"][k]) <= 1e-9 for k in E.KEYS)
        and bool(np.nanmax(np.abs(found["pairs"]["hausdorff"].cpu().numpy() - want["pair_hausdorff"])) <= 1e-9))
    res["restatement_over_device"] = round(res["c_restatement_host_s"] * 1e6 / res["a_device_all_modes"]["median_us"], 1)
    res["not_measured"] = ["pycocotools rleFrPoly / maskUtils.iou and shapely distances (none of them is installed: no speed-up over them is claimed)",
                           "the share of fp64 VALU issue in pm_pair_kernel"]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
