"""FFL polygons (planar faces, area and probability filters) on one GPU: the 224 x 224 scene of tools/bench_acm.py at B = 64, on the
pieces of polygonize_post.polygonize_acm_pieces.
  (a) hip.ffl_polygons_device: p3_ffl_polygons (csrc/ffl_polygons.hip) without a read-back, between HIP events: the LDS form and the forced fallback (the
      same device function over the global workspace),
  (b) the phases of the whole polygonize_acm_polygons on the host clock: polygonize_device (marching squares + ACM), corner_split_tensorpoly,
      polygons_from_pieces, polygons_to_host, and the whole call,
  (c) the stage against the float64 restatement tests/ffl_polygons_ref.py on the first --check images (equal or not; the restatement is no speed reference).

    python tools/bench_ffl_polygons.py [--batch 64] [--steps 500] [--repeats 20] [--tolerance 1] [--out profiles/ffl_polygons_bench.json]

(a) is timed between HIP events, (b) with the host clock around work that ends on the host; medians (min, max beside them) after warm-up runs, all in this
one process.  Neither shapely nor OpenCV is at hand: no speed-up over them is claimed.  The kernels' own shares come from a kernel trace of this tool
(rocprofv3 --kernel-trace --stats -- python tools/bench_ffl_polygons.py).  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_acm import synthetic, timed  # noqa: E402
from bench_init_contours import wall  # noqa: E402
from pixelspointspolygons_amd import hip  # noqa: E402
from pixelspointspolygons_amd import polygonize_acm as A  # noqa: E402
from pixelspointspolygons_amd import polygonize_post as Q  # noqa: E402
from tests import ffl_polygons_ref as R  # noqa: E402

DEV = "cuda"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tolerance", type=float, default=1.0)
    ap.add_argument("--check", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ffl_polygons_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ffl_polygons.py measures on the GPU: none visible (no CPU fall-back)")
    cfg = dict(A.ACM_DEFAULTS, steps=args.steps, tolerance=args.tolerance)
    seg, cf, _ = synthetic(args.batch, seed=7)
    seg, cf = seg.to(DEV), cf.to(DEV)
    ind = seg[:, 0].contiguous()
    tp = A.polygonize_device(seg, cf, cfg)
    pieces = Q.corner_split_tensorpoly(tp, cf, args.tolerance)
    pos, sl, pb = pieces["out_pos"], pieces["piece_slice"], pieces["piece_batch"]
    area, thr = cfg["min_area"], cfg["seg_threshold"]
    found = hip.ffl_polygons(pos, sl, pb, ind, area, thr)          # also sizes the workspace
    P, Rn, V = found["counts"]
    per_image = torch.bincount(pb.long(), minlength=args.batch)
    res = {"tool": "bench_ffl_polygons", "gpu": torch.cuda.get_device_name(0), "batch": args.batch, "size": int(seg.shape[-1]), "steps": args.steps,
           "tolerance": args.tolerance, "repeats": args.repeats, "warmup": args.warmup, "piece_vertices": int(pos.shape[0]), "pieces": int(sl.shape[0]),
           "most_pieces_in_an_image": int(per_image.max()), "polygons": P, "rings": Rn, "ring_vertices": V,
           "polygons_kept": int((found["poly_flags"] == 0).sum()), "images_flagged": int((found["image_status"] != 0).sum()),
           "launches": {"kernels": 7, "memsets": 1},
           "workspace_MB": round(int(hip.lib().p3_ffl_polygons_workspace_bytes(int(pos.shape[0]), args.batch)) / 2 ** 20, 2)}

    def device(fallback):
        return hip.ffl_polygons_device(pos, sl, pb, ind, area, thr, force_fallback=fallback)

    res["a_device_lds"] = timed(lambda _: device(False), args.repeats, args.warmup)
    res["a_device_fallback"] = timed(lambda _: device(True), args.repeats, args.warmup)
    slow = device(True)
    res["fallback_bits_equal"] = all(torch.equal(slow[k][:n].view(torch.uint8), found[k].view(torch.uint8)) for k, n in (
        ("ring_pos", V), ("ring_slice", Rn), ("poly_rings", P), ("poly_area", P), ("poly_prob", P), ("poly_flags", P)))

    res["b_polygonize_device"] = wall(lambda: A.polygonize_device(seg, cf, cfg), args.repeats, args.warmup)
    res["b_corner_split_tensorpoly"] = wall(lambda: Q.corner_split_tensorpoly(tp, cf, args.tolerance), args.repeats, args.warmup)
    res["b_polygons_from_pieces"] = wall(lambda: Q.polygons_from_pieces(pieces, seg, cfg), args.repeats, args.warmup)
    whole = Q.polygons_from_pieces(pieces, seg, cfg)
    res["b_polygons_to_host"] = wall(lambda: Q.polygons_to_host(whole), args.repeats, args.warmup)
    res["b_polygonize_acm_polygons"] = wall(lambda: Q.polygonize_acm_polygons(seg, cf, cfg), args.repeats, args.warmup)
    total = res["b_polygonize_acm_polygons"]["median_us"]
    res["share_of_the_whole"] = {k[2:]: round(res[k]["median_us"] / total, 4) for k in ("b_polygonize_device", "b_corner_split_tensorpoly", "b_polygons_from_pieces")}

    n = min(args.check, args.batch)
    host_pieces = Q.pieces_to_host(pieces)[:n]
    want = R.run([[p.astype(np.float32) for p in image] for image in host_pieces], ind[:n].cpu().numpy(), area, thr)
    keep = found["poly_batch"].cpu().numpy() < n
    np_, nr = int(keep.sum()), int(found["poly_rings"].cpu().numpy()[keep][-1, 1]) if keep.any() else 0
    nv = int(found["ring_slice"][nr - 1, 1]) if nr else 0
    res["device_equals_the_restatement"] = bool(
        (np_, nr, nv) == tuple(want["counts"]) and np.array_equal(found["ring_pos"][:nv].cpu().numpy(), want["ring_pos"])
        and np.array_equal(found["ring_slice"][:nr].cpu().numpy(), want["ring_slice"]) and np.array_equal(found["poly_rings"][:np_].cpu().numpy(), want["poly_rings"])
        and np.array_equal(found["poly_flags"][:np_].cpu().numpy(), want["poly_flags"])
        and np.array_equal(found["image_status"][:n].cpu().numpy(), want["image_status"])
        and bool(np.all(np.abs(found["poly_prob"][:np_].cpu().numpy() - want["poly_prob"]) <= 1e-6))
        and bool(np.all(np.abs(found["poly_area"][:np_].cpu().numpy() - want["poly_area"]) <= 1e-6 * np.abs(want["poly_area"]))))
    res["images_checked"] = n
    res["not_measured"] = ["shapely.ops.unary_union", "shapely.ops.polygonize_full", "cv2.fillPoly (none of them is installed: no speed-up over them is claimed)"]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
