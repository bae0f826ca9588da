"""Max tangent angle error (MTA) on one GPU: the scene of tools/bench_poly_metrics.py - 64 images of 224 x 224 with 20 ground-truth
buildings and 20 predictions each (18 jittered copies, 2 spurious small rings).
  (a) hip.max_tangent_angle_device: p3_max_tangent_angle (csrc/mta_metrics.hip) without a read-back, between HIP events: at the reference's
      sampling_spacing 2.0, and at 0.5 and 0.125 (4 and 16 times the samples, where the projection kernel has more to do than to start),
  (b) eval_metrics.max_tangent_angle on the host clock: the call with its one read-back,
  (c) the float64 restatement tests/mta_ref.py on the same input on the host clock, once (numpy on one core: no reference implementation, and no speed-up
      over shapely is claimed - it is not installed), and whether the device agrees with it.

    python tools/bench_mta.py [--batch 64] [--buildings 20] [--repeats 20] [--out profiles/mta_bench.json]

(a) is timed between HIP events, (b) and (c) with the host clock; medians (min, max beside them) after warm-up runs, all in this one process.  The kernels'
own shares come from a kernel trace of this tool (rocprofv3 --kernel-trace --stats -- python tools/bench_mta.py).  Prints one JSON line and writes it to
--out."""
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
from tests import mta_ref as R  # noqa: E402

DEV = "cuda"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--buildings", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mta_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mta.py measures on the GPU: none visible (no CPU fall-back)")
    gt, dt = scene(args.batch, args.buildings, args.seed)
    g, d = E.pack_rings(gt, DEV), E.pack_rings(dt, DEV)
    found = E.max_tangent_angle(d, g, S, S)          # also sizes the workspace
    state = found["per_ring"]["state"].cpu().numpy()
    res = {"tool": "bench_mta", "gpu": torch.cuda.get_device_name(0), "batch": args.batch, "size": S, "repeats": args.repeats, "warmup": args.warmup,
           "gt_rings": int(g["ring_slice"].shape[0]), "dt_rings": int(d["ring_slice"].shape[0]), "gt_vertices": int(g["pos"].shape[0]),
           "dt_vertices": int(d["pos"].shape[0]), "MTA": found["MTA"], "counted": found["counted"], "status": found["status"],
           "ring_states": np.bincount(state, minlength=5).tolist(), "launches": {"kernels": 4, "memsets": 1},
           "workspace_bytes": hip.max_tangent_angle_workspace_bytes(g["ring_slice"].shape[0], d["ring_slice"].shape[0], args.batch)}

    def device(spacing):
        return hip.max_tangent_angle_device(g["pos"], g["ring_slice"], g["ring_image"], d["pos"], d["ring_slice"], d["ring_image"], args.batch, S, S, spacing)

    res["a_device_spacing_2"] = timed(lambda _: device(2.0), args.repeats, args.warmup)
    res["a_device_spacing_0.5"] = timed(lambda _: device(0.5), args.repeats, args.warmup)
    res["a_device_spacing_0.125"] = timed(lambda _: device(0.125), args.repeats, args.warmup)
    res["b_max_tangent_angle"] = wall(lambda: E.max_tangent_angle(d, g, S, S), args.repeats, args.warmup)

    t0 = time.perf_counter()
    want = R.run(gt, dt, S, S)
    res["c_restatement_host_s"] = round(time.perf_counter() - t0, 3)
    counted = want["ring_state"] == R.COUNTED
    res["samples_per_counted_ring"] = {"min": int(want["ring_samples"][counted].min()), "max": int(want["ring_samples"][counted].max()),
                                       "total": int(want["ring_samples"][counted].sum())}
    res["gt_edges_per_image"] = round(g["pos"].shape[0] / args.batch, 1)
    cos = found["per_ring"]["cos"].cpu().numpy()
    res["device_agrees_with_the_restatement"] = bool(
        np.array_equal(state, want["ring_state"]) and np.array_equal(found["per_ring"]["px"].cpu().numpy(), want["ring_px"])
        and np.array_equal(found["per_image"]["overlap_px"].cpu().numpy(), want["image_overlap_px"]) and found["counted"] == int(want["counted"][0])
        and bool(np.abs(cos[counted] - want["ring_cos"][counted]).max() <= 1e-11) and abs(found["MTA"] - want["MTA"]) <= 1e-6)
    res["restatement_over_device"] = round(res["c_restatement_host_s"] * 1e6 / res["a_device_spacing_2"]["median_us"], 1)
    res["not_measured"] = ["shapely's unary_union, buffer(0), intersection areas and project / interpolate (not installed: no speed-up over them is claimed)",
                           "the shares of fp64 VALU issue, LDS broadcast reads and barrier phases in mta_project_kernel (no counter run)",
                           "the deviations of DESIGN.md section 23 from angle_eval.py"]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
