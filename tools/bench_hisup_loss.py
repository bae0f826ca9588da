"""p3_hisup_train_loss on one GPU at B = 4 and 16, 224 x 224, on seeded random maps (randn logits, 1 % junction pixels, mask density 0.3):
  fused_grad          hip.hisup_train_loss, values + the five gradients, all maps NCHW
  fused_values        the same call with need_grad=False
  fused_grad_rows     jloc / joff / mask / afm as the predictors' token-major rows [B*H*W, 8] (gradients in the same layout), remask NCHW
  val_loss            p3_hisup_val_loss on the same inputs (values only, the kernel forward_val uses)
  torch_fwd_bwd       the yardstick: the reference's five lines (models/hisup/model_hisup.py:302-306, sigmoid_l1_loss :27-37) and the weighted sum
                      of train/trainer_hisup.py:31-39 written in torch, forward + backward, same GPU, same process, same inputs
  torch_fwd           their forward alone

    python tools/bench_hisup_loss.py [--batches 4,16] [--iters 200] [--warmup 20] [--out profiles/hisup_loss_bench.json]

Eager launches; the variants ALTERNATE inside one loop, every timed call between its own pair of HIP events after warm-up calls of every variant; medians
(min, max beside them).  gb_per_s = the bytes the algorithm needs (every logit and target read once, every gradient written once: 72 B read and 44 B
written per pixel with gradients, 72 B read without) over the median time of the whole call, launches included - an end-to-end figure, not a kernel's
share of peak.  Prints one JSON line and writes it."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pixelspointspolygons_amd import hip  # noqa: E402

DEV, S = "cuda", 224
WEIGHTS = (8.0, 0.25, 1.0, 0.1, 1.0)              # config/model/hisup.yaml, LOSS_KEYS order
READ_B, WRITE_B = 11 * 4 + 8 + 5 * 4, 11 * 4      # per pixel: 11 logits + int64 t_jloc + 5 fp32 targets; 11 gradients


def inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    pred = [torch.randn(B, n, S, S, generator=g) * s for n, s in ((3, 2.0), (2, 1.0), (2, 2.0), (2, 1.0), (2, 3.0))]
    t_jloc = torch.zeros(B, 1, S, S, dtype=torch.long)
    hit = torch.rand(B, 1, S, S, generator=g) < 0.01
    t_jloc[hit] = torch.randint(1, 3, (int(hit.sum()),), generator=g)
    t_joff = (torch.rand(B, 2, S, S, generator=g) - 0.5) * (t_jloc > 0)
    t_mask = (torch.rand(B, 1, S, S, generator=g) < 0.3).float()
    t_afm = torch.randn(B, 2, S, S, generator=g)
    return [p.to(DEV) for p in pred], [t.to(DEV) for t in (t_jloc, t_joff, t_mask, t_afm)]


def sigmoid_l1_loss(logits, targets, offset=0.0, mask=None):          # model_hisup.py:27-37
    logp = torch.sigmoid(logits) + offset
    loss = torch.abs(logp - targets)
    if mask is not None:
        t = ((mask == 1) | (mask == 2)).float()
        w = t.mean(3, True).mean(2, True)
        w[w == 0] = 1
        loss = loss * (t / w)
    return loss.mean()


def torch_losses(pred, tgt):
    jloc, joff, mask, afm, remask = pred
    t_jloc, t_joff, t_mask, t_afm = tgt
    losses = [F.cross_entropy(jloc, t_jloc.squeeze(dim=1)), sigmoid_l1_loss(joff[:, :], t_joff, -0.5, t_jloc),
              F.cross_entropy(mask, t_mask.squeeze(dim=1).long()), F.l1_loss(afm, t_afm), F.cross_entropy(remask, t_mask.squeeze(dim=1).long())]
    return sum(w * v for w, v in zip(WEIGHTS, losses)), losses


def alternating(fns, iters, warmup):
    """{name: fn} -> {name: stats}; one timed call of each variant per round, so that clock and neighbours' load hit all of them alike"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            us[k].append(a.elapsed_time(b) * 1e3)
    return {k: {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)} for k, v in us.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4,16")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hisup_loss_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hisup_loss.py measures on the GPU: none visible (no CPU fall-back)")
    res = {"tool": "bench_hisup_loss", "gpu": torch.cuda.get_device_name(0), "size": S, "iters": args.iters, "warmup": args.warmup,
           "bytes_per_pixel": {"read": READ_B, "written_with_gradients": WRITE_B}, "results": {}}
    for B in [int(b) for b in args.batches.split(",")]:
        pred, tgt = inputs(B, seed=B)
        shape = (B, S, S)
        rows = []
        for p in pred[:4]:
            r = torch.zeros(B * S * S, 8, device=DEV)
            r[:, :p.shape[1]] = p.permute(0, 2, 3, 1).reshape(-1, p.shape[1])
            rows.append(r[:, :p.shape[1]])
        rows.append(pred[4])
        leaves = [p.clone().requires_grad_(True) for p in pred]

        def torch_fwd_bwd():
            for p in leaves:
                p.grad = None
            torch_losses(leaves, tgt)[0].backward()

        def torch_fwd():
            with torch.no_grad():
                torch_losses(pred, tgt)

        fns = {"fused_grad": lambda: hip.hisup_train_loss(*pred, *tgt, WEIGHTS),
               "fused_values": lambda: hip.hisup_train_loss(*pred, *tgt, WEIGHTS, need_grad=False),
               "fused_grad_rows": lambda: hip.hisup_train_loss(*rows, *tgt, WEIGHTS, shape=shape),
               "val_loss": lambda: hip.hisup_val_loss(*pred, *tgt),
               "torch_fwd_bwd": torch_fwd_bwd, "torch_fwd": torch_fwd}
        # the two sides compute the same thing on these inputs (fp32 against fp32: reordered sums and another expf)
        losses, grads = fns["fused_grad"]()
        torch_fwd_bwd()
        total, parts = torch_losses(pred, tgt)
        r = {"loss_rel_diff_vs_torch": round(float(((losses[:5] - torch.stack(parts)).abs() / torch.stack(parts).abs()).max()), 9),
             "grad_rel_diff_vs_torch": round(max(float((g - p.grad).abs().max() / p.grad.abs().max()) for g, p in zip(grads, leaves)), 9)}
        r.update(alternating(fns, args.iters, args.warmup))
        n = B * S * S
        for k, nbytes in (("fused_grad", READ_B + WRITE_B), ("fused_grad_rows", READ_B + WRITE_B), ("fused_values", READ_B), ("val_loss", READ_B),
                          ("torch_fwd_bwd", READ_B + WRITE_B), ("torch_fwd", READ_B)):
            r[k]["algorithm_mb"] = round(n * nbytes / 1e6, 2)
            r[k]["gb_per_s"] = round(n * nbytes / (r[k]["median_us"] * 1e-6) / 1e9, 1)
        r["torch_over_fused_grad"] = round(r["torch_fwd_bwd"]["median_us"] / r["fused_grad"]["median_us"], 2)
        res["results"][f"B{B}"] = r
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
