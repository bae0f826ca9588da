"""Mask / topology metrics, subset IoU and annotation counts on one GPU: the scene of tools/bench_poly_metrics.py - 64 images of
224 x 224 with 20 ground-truth buildings and 20 predictions each (18 jittered copies, 2 spurious small rings).
  (a) hip.mask_metrics_device: p3_mask_metrics (csrc/mask_metrics.hip) without a read-back, between HIP events: all modes, and each mode alone,
  (b) hip.polygon_metrics_device with PM_IOU alone on the same input, between HIP events: the one comparison that means anything, since the filled pass
      repeats that work.  --parent-pm-iou names a JSON file with the same measurement made by the parent commit on the same machine in the same session
      ({"median_us", "min_us", "max_us"}); it is recorded beside this build's,
  (c) eval_metrics.mask_metrics on the host clock: the call with its one read-back,
  (d) the restatement tests/mask_metrics_ref.py on the same input on the host clock, once (numpy on one core: no reference implementation, and no speed-up
      over OpenCV, pycocotools or torchmetrics is claimed - none is installed), and whether the device equals it bit for bit.

    python tools/bench_mask_metrics.py [--batch 64] [--buildings 20] [--repeats 20] [--parent-pm-iou FILE] [--out profiles/mask_metrics_bench.json]

Medians (min, max beside them) after warm-up runs, all in this one process.  Prints one JSON line and writes it to --out."""
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
from bench_poly_metrics import S, scene  # noqa: E402
from pixelspointspolygons_amd import eval_metrics as E  # noqa: E402
from pixelspointspolygons_amd import hip  # noqa: E402
from tests import mask_metrics_ref as R  # noqa: E402

DEV = "cuda"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--buildings", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--thickness", type=int, default=5)
    ap.add_argument("--parent-pm-iou", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_metrics_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mask_metrics.py measures on the GPU: none visible (no CPU fall-back)")
    gt, dt = scene(args.batch, args.buildings, args.seed)
    g, d = E.pack_rings(gt, DEV), E.pack_rings(dt, DEV)
    found = E.mask_metrics(d, g, S, S, buffer_thickness=args.thickness)          # also sizes the workspace
    res = {"tool": "bench_mask_metrics", "gpu": torch.cuda.get_device_name(0), "batch": args.batch, "size": S, "buffer_thickness": args.thickness,
           "repeats": args.repeats, "warmup": args.warmup, "gt_rings": int(g["ring_slice"].shape[0]), "dt_rings": int(d["ring_slice"].shape[0]),
           "gt_vertices": int(g["pos"].shape[0]), "dt_vertices": int(d["pos"].shape[0]), "status": found["status"],
           "metrics": {k: found[k] for k in E.MASK_KEYS}, "stats": {k: found[k] for k in E.STATS_KEYS}, "launches": {"kernels": 3, "memsets": 1},
           "workspace_bytes": hip.mask_metrics_workspace_bytes(g["ring_slice"].shape[0], d["ring_slice"].shape[0], args.batch)}

    def device(modes):
        return hip.mask_metrics_device(g["pos"], g["ring_slice"], g["ring_image"], d["pos"], d["ring_slice"], d["ring_image"], args.batch, S, S,
                                       args.thickness, modes)

    def pm_iou():
        return hip.polygon_metrics_device(g["pos"], g["ring_slice"], g["ring_image"], d["pos"], d["ring_slice"], d["ring_image"], args.batch, S, S, hip.PM_IOU)

    res["a_device_all_modes"] = timed(lambda _: device(hip.MM_TOPDIG | hip.MM_SUBSET | hip.MM_STATS), args.repeats, args.warmup)
    res["a_device_topdig"] = timed(lambda _: device(hip.MM_TOPDIG), args.repeats, args.warmup)
    res["a_device_subset_iou"] = timed(lambda _: device(hip.MM_SUBSET), args.repeats, args.warmup)
    res["a_device_stats"] = timed(lambda _: device(hip.MM_STATS), args.repeats, args.warmup)
    res["b_polygon_metrics_pm_iou"] = timed(lambda _: pm_iou(), args.repeats, args.warmup)
    res["b_polygon_metrics_pm_iou_parent_commit"] = json.load(open(args.parent_pm_iou)) if args.parent_pm_iou else None
    res["c_mask_metrics"] = wall(lambda: E.mask_metrics(d, g, S, S, buffer_thickness=args.thickness), args.repeats, args.warmup)

    t0 = time.perf_counter()
    want = R.run(gt, dt, S, S, args.thickness)
    res["d_restatement_host_s"] = round(time.perf_counter() - t0, 3)
    got = {k: v.cpu().numpy() for k, v in device(7).items()}
    bits = lambda a: a.view(np.int64) if a.dtype == np.float64 else a
    res["device_equals_the_restatement"] = bool(all(np.array_equal(bits(got[k]), bits(want[k])) for k in got))
    conf = want["image_conf"].astype(np.int64).sum(axis=0)
    res["pixels_set"] = {"filled_gt": int(conf[0, 0] + conf[0, 2]), "filled_dt": int(conf[0, 0] + conf[0, 1]), "stroked_gt": int(conf[1, 0] + conf[1, 2]),
                         "stroked_dt": int(conf[1, 0] + conf[1, 1])}
    res["not_measured"] = ["cv2.fillPoly / cv2.polylines, pycocotools and torchmetrics (none is installed: no speed-up over them is claimed)",
                           "which phase of mm_mask_kernel bounds it: the filled pass, the stroke, the popcounts or its barriers (no kernel trace, no counter run)",
                           "the deviations of DESIGN.md section 24 from the reference"]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
