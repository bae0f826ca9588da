"""COCO AP / AR on instance masks and on their boundaries on one GPU: the scene of tools/bench_poly_metrics.py - 64 images of 224 x 224
with 20 ground-truth buildings and 20 predictions each (18 jittered copies, 2 spurious small rings) - with a score per prediction (multiples of 1/64).
  (a) hip.coco_metrics_device: p3_coco_metrics (csrc/coco_metrics.hip) without a read-back, between HIP events: segm alone, and both types,
  (b) eval_metrics.coco_metrics on the host clock: the call with its one read-back,
  (c) the restatement tests/coco_metrics_ref.py on the same input on the host clock, once (numpy on one core: no reference implementation, and no speed-up
      over pycocotools / boundary-iou-api is claimed - neither is installed), and whether the device equals it.

    python tools/bench_coco_metrics.py [--batch 64] [--buildings 20] [--repeats 20] [--out profiles/coco_metrics_bench.json]

(a) is timed between HIP events, (b) and (c) with the host clock; medians (min, max beside them) after warm-up runs, all in this one process.  Prints one
JSON line and writes it to --out."""
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
from tests import coco_metrics_ref as R  # noqa: E402

DEV = "cuda"
EXACT = ("gt_area_px", "dt_area_px", "gt_boundary_px", "dt_boundary_px", "dt_rank", "pair_inter", "dt_match", "dt_ignore", "gt_match")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--buildings", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coco_metrics_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_coco_metrics.py measures on the GPU: none visible (no CPU fall-back)")
    gt, dt = scene(args.batch, args.buildings, args.seed)
    rng = np.random.default_rng(args.seed + 1)
    scores = [[float(v) / 64.0 for v in rng.integers(1, 65, len(d))] for d in dt]
    g, d = E.pack_rings(gt, DEV), E.pack_rings(dt, DEV, scores=scores)
    found = E.coco_metrics(d, g, S, S)          # also sizes the workspace
    Rg, Rd = int(g["ring_slice"].shape[0]), int(d["ring_slice"].shape[0])
    res = {"tool": "bench_coco_metrics", "gpu": torch.cuda.get_device_name(0), "batch": args.batch, "size": S, "repeats": args.repeats, "warmup": args.warmup,
           "gt_rings": Rg, "dt_rings": Rd, "gt_vertices": int(g["pos"].shape[0]), "dt_vertices": int(d["pos"].shape[0]), "dilation": R.dilation(S, S),
           "status": found["status"], "segm": {k: found[k] for k in E.COCO_KEYS}, "boundary": found["boundary"],
           "launches": {"kernels": 7, "memsets": 7},
           "workspace_bytes": {"both": hip.coco_metrics_workspace_bytes(Rg, Rd, args.batch, S, S), "segm": hip.coco_metrics_workspace_bytes(Rg, Rd, args.batch, S, S, hip.COCO_SEGM)}}

    def device(types):
        return hip.coco_metrics_device(g["pos"], g["ring_slice"], g["ring_image"], d["pos"], d["ring_slice"], d["ring_image"], args.batch, S, S, types,
                                       dt_score=d["score"])

    res["a_device_segm"] = timed(lambda _: device(hip.COCO_SEGM), args.repeats, args.warmup)
    res["a_device_segm_and_boundary"] = timed(lambda _: device(hip.COCO_SEGM | hip.COCO_BOUNDARY), args.repeats, args.warmup)
    res["b_coco_metrics"] = wall(lambda: E.coco_metrics(d, g, S, S), args.repeats, args.warmup)

    t0 = time.perf_counter()
    want = R.run(gt, dt, S, S, scores)
    res["c_restatement_host_s"] = round(time.perf_counter() - t0, 3)
    got = {k: v.cpu().numpy() for k, v in {**found["tables"], **found["pairs"]}.items()}
    res["matched_at_0.5"] = int((want["dt_match"][0, 0, 0] >= 0).sum())
    res["device_equals_the_restatement"] = bool(all(np.array_equal(got[k], want[k]) for k in EXACT)
                                                and all(np.array_equal(got[k], want[k]) for k in ("precision", "recall", "stats")))
    res["restatement_over_device"] = round(res["c_restatement_host_s"] * 1e6 / res["a_device_segm_and_boundary"]["median_us"], 1)
    res["not_measured"] = ["pycocotools COCOeval and boundary-iou-api mask_to_boundary (neither is installed: no speed-up over them is claimed)",
                           "the kernels' own shares (no trace was taken)", "the rleFrPoly deviation"]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
