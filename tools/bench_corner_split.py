"""FFL corner-aware contour simplification on one GPU: the 224 x 224, B = 16 scene of tools/bench_init_contours.py / bench_acm.py, on the optimised contours of
polygonize_acm.polygonize_device.
  (a) hip.corner_split_device: p3_corner_split (csrc/corner_split.hip) without a read-back, between HIP events: the LDS form and the forced fallback (the
      same device functions over the global workspace),
  (b) end to end with the change: polygonize_post.polygonize_acm_pieces + pieces_to_host (seg -> pieces on the host),
  (c) end to end without it: polygonize_device + tensorpoly_to_contours_batch + the numpy restatement of the same stages per contour
      (tests/corner_split_ref.py): the host path as it would be; skimage's and shapely's own time cannot be measured here, no speed-up over them is claimed,
  (d) the two tails alone, from the optimised TensorPoly on: corner_split_tensorpoly + pieces_to_host against the download + the restatement.

    python tools/bench_corner_split.py [--batch 16] [--steps 500] [--repeats 20] [--tolerance 1] [--out profiles/corner_split_bench.json]

(a) is timed between HIP events, (b)-(d) with the host clock around work that ends on the host; medians (min, max beside them) after warm-up runs; both legs in
this one process.  Prints one JSON line and writes it to --out."""
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
from tests import corner_split_ref as R  # noqa: E402

DEV = "cuda"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tolerance", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corner_split_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_corner_split.py measures on the GPU: none visible (no CPU fall-back)")
    cfg = dict(A.ACM_DEFAULTS, steps=args.steps, tolerance=args.tolerance)
    tol, tol_pre = args.tolerance, min(1.0, args.tolerance)
    seg, cf, _ = synthetic(args.batch, seed=7)
    seg, cf = seg.to(DEV), cf.to(DEV)
    cf_host = cf.cpu().numpy()
    tp = A.polygonize_device(seg, cf, cfg)
    sl = tp.poly_slice
    closed = ~tp.is_endpoint.index_select(0, sl[:, 0])
    pb = tp.batch.index_select(0, sl[:, 0])
    pos = tp.pos.detach()
    found = hip.corner_split(pos, None, sl, closed, pb, cf, tol_pre, tol, max_len=tp.max_len)          # also sizes the workspace
    V, NP, longest = found["counts"]
    res = {"tool": "bench_corner_split", "gpu": torch.cuda.get_device_name(0), "batch": args.batch, "size": int(seg.shape[-1]), "steps": args.steps,
           "tolerance": tol, "repeats": args.repeats, "warmup": args.warmup, "contours": int(sl.shape[0]), "longest_contour": int(tp.max_len),
           "vertices_in": int(pos.shape[0]), "vertices_out": V, "pieces": NP, "longest_piece": longest,
           "download_bytes_in": int(pos.shape[0]) * 8, "download_bytes_out": V * 8 + NP * 20,
           "launches": {"kernels": 4, "memsets": 2},
           "workspace_MB": round(int(hip.lib().p3_corner_split_workspace_bytes(int(pos.shape[0]) + int(sl.shape[0]), int(sl.shape[0]))) / 2 ** 20, 2)}

    def device(fallback):
        return hip.corner_split_device(pos, None, sl, closed, pb, cf, tol_pre, tol, max_len=tp.max_len, force_fallback=fallback)

    res["a_device_lds"] = timed(lambda _: device(False), args.repeats, args.warmup)
    res["a_device_fallback"] = timed(lambda _: device(True), args.repeats, args.warmup)
    slow = device(True)
    res["fallback_bits_equal"] = all(torch.equal(slow[k][:n], found[k]) for k, n in (("out_pos", V), ("out_src", V), ("piece_slice", NP), ("piece_poly", NP)))

    def host_tail(tensorpoly):
        contours = A.tensorpoly_to_contours_batch(tensorpoly)
        return [[p for c in cs for p in R.pieces_of_contour(c, cf_host[b], tol_pre, tol)] for b, cs in enumerate(contours)]

    res["b_polygonize_acm_pieces_to_host"] = wall(lambda: Q.pieces_to_host(Q.polygonize_acm_pieces(seg, cf, cfg)), args.repeats, args.warmup)
    res["c_polygonize_device_download_numpy"] = wall(lambda: host_tail(A.polygonize_device(seg, cf, cfg)), args.repeats, args.warmup)
    res["d_device_tail"] = wall(lambda: Q.pieces_to_host(Q.corner_split_tensorpoly(tp, cf, tol)), args.repeats, args.warmup)
    res["d_host_tail"] = wall(lambda: host_tail(tp), args.repeats, args.warmup)
    res["d_download_alone"] = wall(lambda: A.tensorpoly_to_contours_batch(tp), args.repeats, args.warmup)
    got, want = Q.pieces_to_host(Q.corner_split_tensorpoly(tp, cf, tol)), host_tail(tp)
    res["device_equals_the_restatement"] = bool(len(got) == len(want) and all(
        len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b)) for a, b in zip(got, want)))
    res["end_to_end_host_over_device"] = round(res["c_polygonize_device_download_numpy"]["median_us"] / res["b_polygonize_acm_pieces_to_host"]["median_us"], 2)
    res["tail_host_over_device"] = round(res["d_host_tail"]["median_us"] / res["d_device_tail"]["median_us"], 2)
    res["not_measured"] = ["skimage.measure.approximate_polygon", "shapely LineString.simplify", "unary_union / polygonize_full (host code of the caller, unchanged)"]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
