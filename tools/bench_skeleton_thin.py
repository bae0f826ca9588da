"""FFL active-skeleton initialisation from the segmentation map (init_method "skeleton_device") on one GPU: the 224 x 224, B = 16 scene of
tools/bench_asm_init.py (a dozen building outlines per image), level 0.5.
  (a) hip.skeleton_from_seg_device: p3_skeleton_from_seg (csrc/skeleton_thin.hip) alone, no read-back,
  (b) polygonize_asm.init_skeletons(method="skeleton_device"): (a), its read-back, the plan and its read-back,
  (c) polygonize_asm.polygonize_device with init_method "skeleton_device": (b) + the optimiser at the shipped asm_method schedule, ending in a synchronise,
  (d) the marching-squares figures beside them, in the same run: p3_init_contours + p3_skeleton_from_contours alone, init_skeletons and polygonize_device.
The thinning round count of every image comes from the host restatement of the definition (tests/skeleton_thin_ref.py), which is also compared with the
device result, field by field.

    python tools/bench_skeleton_thin.py [--batch 16] [--repeats 20] [--warmup 3] [--out profiles/skeleton_thin_bench.json]

(a) and the marching-squares kernels are timed between HIP events around the eager call (the host clock around the same call plus a synchronise is given
beside them), the rest with the host clock around work that ends in a synchronise; medians (min, max beside them) after warm-up runs.  Prints one JSON
line and writes it to --out."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_acm import synthetic, timed  # noqa: E402
from bench_init_contours import wall  # noqa: E402
from pixelspointspolygons_amd import hip  # noqa: E402
from pixelspointspolygons_amd import polygonize_asm as A  # noqa: E402
from pixelspointspolygons_amd._lib import LIB_PATH  # noqa: E402

DEV = "cuda"
CONTAINER = ("pos", "degrees", "path_index", "path_delim", "batch", "batch_delim")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skeleton_thin_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_skeleton_thin.py measures on the GPU: none visible (no CPU fall-back)")
    # deliberate: this tool, unlike the package, reads the tests' host restatement - for the thinning round counts, which the device does not report, and
    # for the equality check of the result it times.  Nothing under pixelspointspolygons_amd imports it.
    from tests import skeleton_thin_ref as R
    thin = {**A.ASM_DEFAULTS, "init_method": "skeleton_device"}
    squares = {**A.ASM_DEFAULTS, "init_method": "marching_squares"}
    level, min_area, B = thin["data_level"], thin["min_area"], args.batch
    seg_host, cf, _ = synthetic(B, seed=7)
    seg, cf = seg_host.float().to(DEV), cf.to(DEV)
    sk = hip.skeleton_from_seg(seg, level)
    plan = hip.asm_plan(sk["path_index"], sk["path_delim"], sk["pos"].shape[0])
    ref = R.container(seg_host.float(), level)
    same = sk["counts"] == ref.counts and all(torch.equal(sk[k].cpu(), getattr(ref, k)) for k in CONTAINER)
    N, M, P, longest = sk["counts"]
    degrees = torch.bincount(sk["degrees"], minlength=5).tolist()
    c = hip.init_contours(seg, level)
    ms = hip.skeleton_from_contours(c["pos"], c["poly_slice"], c["poly_batch"], c["is_endpoint"], B, min_area)
    res = {"tool": "bench_skeleton_thin", "gpu": torch.cuda.get_device_name(0), "size": seg.shape[-1], "batch": B, "channels": seg.shape[1], "level": level,
           "nodes": N, "slots": M, "paths": P, "longest_path_nodes": longest, "nodes_by_degree": degrees, "components": plan["counts"][0],
           "max_comp": plan["counts"][1], "thinning_rounds_per_image": [st.rounds for st in ref.stages], "equals_the_host_restatement": bool(same),
           "marching_squares": {"nodes": ms["counts"][0], "slots": ms["counts"][1], "paths": ms["counts"][2]},
           "workspace_bytes": int(hip.lib().p3_skeleton_from_seg_workspace_bytes(B, seg.shape[2], seg.shape[3])),
           "launches": {"skeleton_from_seg": {"kernels": 3, "memsets": 0}}, "repeats": args.repeats, "warmup": args.warmup, "library": os.path.basename(LIB_PATH)}

    def both(fn):
        return {"events": timed(lambda _: fn(), args.repeats, args.warmup), "host_clock_with_synchronise": wall(fn, args.repeats, args.warmup)}

    res["a_skeleton_from_seg_device"] = both(lambda: hip.skeleton_from_seg_device(seg, level))
    res["b_init_skeletons_skeleton_device"] = wall(lambda: A.init_skeletons(seg, level, min_area, method="skeleton_device"), args.repeats, args.warmup)
    res["c_polygonize_device_skeleton_device"] = wall(lambda: A.polygonize_device(seg, cf, thin), args.repeats, args.warmup)
    res["d_init_contours_device"] = both(lambda: hip.init_contours_device(seg, level))
    res["d_skeleton_from_contours_device"] = both(lambda: hip.skeleton_from_contours_device(c["pos"], c["poly_slice"], c["poly_batch"], c["is_endpoint"], B, min_area))
    res["d_init_skeletons_marching_squares"] = wall(lambda: A.init_skeletons(seg, level, min_area), args.repeats, args.warmup)
    res["d_polygonize_device_marching_squares"] = wall(lambda: A.polygonize_device(seg, cf, squares), args.repeats, args.warmup)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
