"""FFL initial contours on one GPU: the 224 x 224, B = 16 scene of tools/bench_acm.py (a dozen building outlines and noise per image), marching squares at
level 0.5 on the segmentation map itself.
  (a) hip.init_contours_device: p3_init_contours (csrc/contours.hip) without a read-back - as a captured hipGraph replayed (the device time of its launches and
      the boundaries between them) and called eagerly (what the host needs to enqueue them, when that is longer); both forms of the two pointer-doubling passes,
      forced with P3_IC_DOUBLING: `image` (one launch per pass, one workgroup per image) and `rounds` (one launch per round), and what the library picks itself,
  (b) polygonize_acm.init_contours: (a) + the read-back of the three counts + the TensorPoly,
  (c) polygonize_acm.polygonize_device: seg -> optimised contours, steps of the shipped acm_method config, ending in a device synchronise,
  (d) the path of before with the host contours ALREADY computed: contours_batch_to_tensorpoly(host contours) + .to(device) + optimize(), and its first two parts
      alone (the upload every host contour method pays, whatever it costs to find the contours: skimage is not installed here, its own time is not measured).

    python tools/bench_init_contours.py [--batch 16] [--size 224] [--tile 1] [--steps 500] [--repeats 20] [--kernel-only] [--out profiles/init_contours_bench.json]

(a) is timed between HIP events, (b)-(d) with the host clock around work that ends in a synchronise; medians (min, max beside them) after warm-up runs.
--kernel-only times (a) alone.  --size draws the same dozen buildings on a larger map (an emptier one); --tile T repeats the drawn map T x T times instead, which
keeps the share of crossed edges: the shapes on which the choice between the two forms of the doubling passes was measured.
Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_acm  # noqa: E402
from bench_acm import synthetic, timed  # noqa: E402
from pixelspointspolygons_amd import hip  # noqa: E402
from pixelspointspolygons_amd import polygonize_acm as A  # noqa: E402
from pixelspointspolygons_amd._lib import LIB_PATH  # noqa: E402

DEV = "cuda"


def wall(fn, n, warmup):
    """fn() + a device synchronise, n times on the host clock after `warmup` untimed ones"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6)
    return {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=bench_acm.S)
    ap.add_argument("--tile", type=int, default=1)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "init_contours_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_init_contours.py measures on the GPU: none visible (no CPU fall-back)")
    cfg = dict(A.ACM_DEFAULTS, steps=args.steps)
    S = bench_acm.S = args.size          # synthetic() draws its maps at the module's size
    os.environ.pop("P3_IC_DOUBLING", None)
    seg, cf, _ = synthetic(args.batch, seed=7)
    seg, cf = seg.repeat(1, 1, args.tile, args.tile).to(DEV), cf.repeat(1, 1, args.tile, args.tile).to(DEV)
    S *= args.tile
    level = cfg["data_level"]
    E = S * (S - 1) * 2
    rounds = max((E - 1).bit_length(), 1)
    found = hip.init_contours(seg, level)          # also the warm-up that sizes the workspace before the capture
    N, P, longest = found["counts"]
    res = {"tool": "bench_init_contours", "gpu": torch.cuda.get_device_name(0), "size": S, "tile": args.tile, "batch": args.batch, "level": level, "vertices": N, "contours": P,
           "longest": longest, "open_contours": int(found["is_endpoint"].sum()) // 2, "repeats": args.repeats, "warmup": args.warmup,
           "library": os.path.basename(LIB_PATH),
           # what csrc/contours.hip enqueues for this shape, whatever the data
           "launches": {"doubling_rounds_per_pass": rounds, "image": {"kernels": 11, "memsets": 1}, "rounds": {"kernels": 10 + 2 * rounds, "memsets": 1}},
           "workspace_MB": round(int(hip.lib().p3_init_contours_workspace_bytes(args.batch, S, S)) / 2 ** 20, 1)}

    def finish():
        line = json.dumps(res)
        print(line)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")

    def device_form(mode):
        """(a) with the doubling passes forced to `mode` (None: the library's own choice)"""
        if mode:
            os.environ["P3_IC_DOUBLING"] = mode
        hip.init_contours_device(seg, level)
        res["picked" if not mode else "forced_" + mode] = hip.lib().p3_last_kernel().decode()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = hip.init_contours_device(seg, level)
        r = {"graph_replay": timed(lambda _: graph.replay(), args.repeats, args.warmup)}
        r["bits_equal"] = all(torch.equal(out[k][:n], found[k]) for k, n in (("pos", N), ("batch", N), ("is_endpoint", N), ("poly_slice", P), ("poly_batch", P)))
        del graph
        r["eager"] = timed(lambda _: hip.init_contours_device(seg, level), args.repeats, args.warmup)
        os.environ.pop("P3_IC_DOUBLING", None)
        return r

    hip.lib().p3_trace_kernels(1)
    res["a_device_image"] = device_form("image")
    res["a_device_rounds"] = device_form("rounds")
    res["a_device"] = device_form(None)
    hip.lib().p3_trace_kernels(0)
    if args.kernel_only:
        return finish()
    res["b_init_contours_with_read_back"] = wall(lambda: A.init_contours(seg, level), args.repeats, args.warmup)
    res["c_polygonize_device"] = wall(lambda: A.polygonize_device(seg, cf, cfg), args.repeats, args.warmup)
    host = A.tensorpoly_to_contours_batch(A.init_contours(seg, level))          # the same contours, on the host, before any timed run
    ind = seg[:, 0]

    def before():
        tp = A.contours_batch_to_tensorpoly(host).to(DEV)
        return A.TensorPolyOptimizer(cfg, tp, ind, cf, cfg["data_coef"], cfg["length_coef"], cfg["crossfield_coef"]).optimize()

    res["d_host_contours_given_upload_and_optimize"] = wall(before, args.repeats, args.warmup)
    res["d_upload_alone"] = wall(lambda: A.contours_batch_to_tensorpoly(host).to(DEV), args.repeats, args.warmup)
    res["d_host_container_alone"] = wall(lambda: A.contours_batch_to_tensorpoly(host), args.repeats, args.warmup)
    tp = A.init_contours(seg, level)
    pos0 = tp.pos.clone()

    def optimize_alone():
        tp.pos = pos0.clone()
        A.TensorPolyOptimizer(cfg, tp, ind, cf, cfg["data_coef"], cfg["length_coef"], cfg["crossfield_coef"]).optimize()

    res["acm_optimize_alone"] = wall(optimize_alone, args.repeats, args.warmup)
    got, want = A.polygonize_device(seg, cf, cfg), before()
    res["polygonize_device_equals_the_path_of_before"] = bool(torch.equal(got.pos, want.pos) and torch.equal(got.poly_slice, want.poly_slice))
    res["init_with_read_back_over_upload_alone"] = round(res["b_init_contours_with_read_back"]["median_us"] / res["d_upload_alone"]["median_us"], 2)
    finish()


if __name__ == "__main__":
    main()
