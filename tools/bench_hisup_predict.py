"""HiSup inference after the encoder on one GPU, at B = 4 (the reference's per-GPU batch) and 16, 224 x 224, bf16 and fp32:
  (a) the head set (hisup.HiSupHeads on an NCHW feature map),
  (b) p3_hisup_junctions + p3_hisup_regions on planted head outputs (120 junctions per class and image, a dozen building blobs),
  (c) the same junction work written with the reference's own torch operators on the same GPU, per image, with its two .item() calls
      (model_hisup.py:251-253,266-268, polygon.py:8-38); regions are left out of (c): torch has no labelling,
plus the junction kernel's design worst case (every fourth pixel a candidate) and the validation-loss kernel.

    python tools/bench_hisup_predict.py [--batches 4,16] [--precisions bf16,fp32] [--iters 50] [--warmup 10]

Eager launches, every timed call between its own pair of HIP events after warm-up calls; medians (min, max beside them).  (b), (c) and the
worst case do not depend on the precision (the predictors write fp32) and are measured once per batch size.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pixelspointspolygons_amd import hip, ops  # noqa: E402
from pixelspointspolygons_amd.hisup import HiSupHeads  # noqa: E402

DEV = "cuda"
S = 224


def timed(fn, n, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1)}


def planted(B, K, stride, seed):
    """jloc / joff / remask logits [B, *, S, S]: 2K junction peaks per image on a grid of the given stride, rectangular building blobs"""
    g = torch.Generator().manual_seed(seed)
    jloc = torch.empty(B, 3, S, S)
    jloc[:, 0] = 6.0
    jloc[:, 1:] = 0.25 * torch.randn(B, 2, S, S, generator=g)
    n = len(range(1, S, stride))
    for b in range(B):
        cells = torch.randperm(n * n, generator=g)[:2 * K]
        jloc[b, 1 + (torch.arange(2 * K) % 2), 1 + stride * (cells // n), 1 + stride * (cells % n)] = 3 + 6 * torch.rand(2 * K, generator=g)
    joff = torch.randn(B, 2, S, S, generator=g)
    d = torch.full((B, S, S), -3.0)
    for b in range(B):
        for _ in range(12):
            y, x, h, w = [int(v) for v in torch.randint(0, 180, (4,), generator=g)]
            d[b, y:y + 8 + h % 40, x:x + 8 + w % 40] = 3.0
    d += 0.3 * torch.randn(B, S, S, generator=g)
    remask = torch.stack([-d / 2, d / 2], 1)
    return jloc.to(DEV), joff.to(DEV), remask.to(DEV)


def torch_junctions(jloc_pred, joff_pred):
    """forward_val's junction part with the reference's operators: per image softmax slices, max_pool2d NMS, two .item(), two topk, four gathers"""
    joff_pred = joff_pred.sigmoid() - 0.5
    convex = jloc_pred.softmax(1)[:, 2:3]
    concave = jloc_pred.softmax(1)[:, 1:2]
    out = []
    for b in range(jloc_pred.size(0)):
        parts = []
        for a in (convex[b], concave[b]):
            ap = F.max_pool2d(a, 3, stride=1, padding=1)
            nms = a * (a == ap).float().clamp(min=0.0)
            k = min(300, int((nms > 0.008).float().sum().item()))
            width = nms.size(2)
            jo = joff_pred[b].reshape(2, -1)
            scores, index = torch.topk(nms.reshape(-1), k=k)
            y = (index // width).float() + torch.gather(jo[1], 0, index) + 0.5
            x = (index % width).float() + torch.gather(jo[0], 0, index) + 0.5
            parts.append(torch.stack((x, y)).t()[scores > 0])
        out.append(torch.cat(parts, 0).detach().cpu().numpy())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4,16")
    ap.add_argument("--precisions", default="bf16,fp32")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hisup_predict.py measures on the GPU: none visible (no CPU fall-back)")
    res = {"tool": "bench_hisup_predict", "gpu": torch.cuda.get_device_name(0), "size": S, "iters": args.iters, "warmup": args.warmup, "results": {}}
    for B in [int(b) for b in args.batches.split(",")]:
        r = {}
        jloc, joff, remask = planted(B, 120, 4, seed=B)
        r["b_junctions"] = timed(lambda: hip.hisup_junctions(jloc, joff), args.iters, args.warmup)
        r["b_regions"] = timed(lambda: hip.hisup_regions_device(remask), args.iters, args.warmup)
        r["b_junctions_plus_regions"] = timed(lambda: (hip.hisup_junctions(jloc, joff), hip.hisup_regions_device(remask)), args.iters, args.warmup)
        r["n_regions"] = hip.hisup_regions(remask)["n_regions"].tolist()
        r["c_torch_junctions_per_image"] = timed(lambda: torch_junctions(jloc, joff), args.iters, args.warmup)
        mine = hip.hisup_junctions(jloc, joff)
        theirs = torch_junctions(jloc, joff)
        r["junction_counts_equal"] = all(int(mine[3][b].sum()) == len(theirs[b]) for b in range(B))
        wj, wo = jloc.clone(), joff                                # the design worst case: every fourth pixel a candidate, in both classes
        wj[:, 1:, 1::2, 1::2] = 3 + 6 * torch.rand(B, 2, S // 2, S // 2, device=DEV)
        r["junctions_worst_case"] = timed(lambda: hip.hisup_junctions(wj, wo), args.iters, args.warmup)
        all_fg = torch.stack([torch.full((B, S, S), -3.0), torch.full((B, S, S), 3.0)], 1).to(DEV)
        r["regions_all_foreground"] = timed(lambda: hip.hisup_regions_device(all_fg), args.iters, args.warmup)
        g = torch.Generator().manual_seed(3)
        pred = [torch.randn(B, n, S, S, generator=g).to(DEV) for n in (3, 2, 2, 2, 2)]
        tgt = [torch.randint(0, 3, (B, 1, S, S), generator=g).to(DEV), torch.rand(B, 2, S, S, generator=g).to(DEV) - 0.5,
               (torch.rand(B, 1, S, S, generator=g) < 0.3).float().to(DEV), torch.randn(B, 2, S, S, generator=g).to(DEV)]
        r["val_loss"] = timed(lambda: hip.hisup_val_loss(*pred, *tgt), args.iters, args.warmup)
        for prec in args.precisions.split(","):
            ops.reset_process_state()
            torch.manual_seed(0)
            heads = HiSupHeads(dim_in=256, precision=prec).to(DEV).eval()
            feats = torch.randn(B, 256, S, S, device=DEV)
            a = timed(lambda: heads(feats), max(args.iters // 5, 10), 3)
            a["b_share_of_a"] = round(r["b_junctions_plus_regions"]["median_us"] / a["median_us"], 5)
            r["a_head_set_" + prec] = a
            del heads, feats
            torch.cuda.empty_cache()
        r["b_over_c"] = round(r["b_junctions"]["median_us"] / r["c_torch_junctions_per_image"]["median_us"], 4)
        res["results"][f"B{B}"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
