"""The FFL active-skeleton optimiser on one GPU: 224 x 224, B = 16, seeded synthetic skeletons (per image the dozen building outlines and two open
border-to-border polylines of tools/bench_acm.py as paths, four "shared wall" theta graphs - two degree-3 junctions joined by three paths - and two
degree-4 stars whose arms end in tips), 300 steps of the shipped asm_method config.
  (a) hip.asm_optimize: one launch for all steps (csrc/asm.hip, the LDS path),
  (b) the same call through the one-launch-per-step fallback (what a component over the LDS cap costs),
  (c) the same three-term algorithm written with stock torch operators on the same GPU the way the reference runs its own
      (predict/ffl/polygonize_asm.py:177-235, 353, 361-421): fp32, autograd, torch.optim.RMSprop(alpha=0.9) + ExponentialLR, the tips put back after
      every step, three .item() reads per step (the reference reads six, and computes three more terms that never reach its total_loss).

    python tools/bench_asm.py [--batch 16] [--steps 300] [--repeats 20] [--torch-repeats 3] [--kernel-only] [--no-junctions]\
                               [--out profiles/asm_bench.json]

Every timed run starts from the same initial skeleton and a zero RMSprop state, between its own pair of HIP events after warm-up runs; medians (min, max
beside them).  What a run needs first (the copies of the initial positions and state for (a) and (b); the index build, the optimizer and the scheduler of
(c)) is done before its first event.  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_acm import S, synthetic, timed  # noqa: E402
from pixelspointspolygons_amd import hip  # noqa: E402
from pixelspointspolygons_amd import polygonize_asm as A  # noqa: E402
from pixelspointspolygons_amd._lib import LIB_PATH  # noqa: E402

DEV = "cuda"


def skeletons(contours_batch, seed, junctions=True):
    """the contours of every image as a Skeleton, plus junction graphs (junctions=False: the contours alone, every node of degree <= 2): -> [Skeleton]"""
    rng = np.random.default_rng(seed)
    out = []
    for contours in contours_batch:
        sk = A.contours_to_skeleton(contours)
        coords, degrees, indices, indptr = [sk.coordinates], [sk.degrees], list(sk.paths.indices), list(sk.paths.indptr)
        n = sk.coordinates.shape[0]

        def nodes(pts, degree):
            nonlocal n
            coords.append(np.asarray(pts, dtype=np.float64).reshape(-1, 2)); degrees.append(np.full(len(coords[-1]), degree, dtype=np.int64))
            n += len(coords[-1])
            return list(range(n - len(coords[-1]), n))

        def path(ids):
            indices.extend(ids); indptr.append(len(indices))

        for _ in range(4 if junctions else 0):          # theta graph: a wall shared by two buildings and their two outer outlines
            c, half, ang = rng.uniform(50, S - 50, 2), rng.uniform(12, 25), rng.uniform(0, np.pi)
            d = np.array([np.sin(ang), np.cos(ang)])
            j1, j2 = nodes([c - half * d], 3)[0], nodes([c + half * d], 3)[0]
            for bow in (0.0, rng.uniform(10, 20), -rng.uniform(10, 20)):
                k = int(round(np.hypot(2 * half, 2 * bow))) if bow else int(round(2 * half))
                t = (np.arange(1, k) / k)[:, None]
                mid = (c - half * d) * (1 - t) + (c + half * d) * t + bow * np.sin(np.pi * t) * np.array([d[1], -d[0]]) + rng.normal(0, 0.3, (k - 1, 2))
                path([j1] + nodes(mid, 2) + [j2])
        for _ in range(2 if junctions else 0):          # a degree-4 star: four arms of ~20 nodes to tips
            c = rng.uniform(40, S - 40, 2)
            x = nodes([c], 4)[0]
            for a in range(4):
                ang = a * np.pi / 2 + rng.uniform(-0.3, 0.3)
                k = int(rng.integers(15, 25))
                pts = c + np.arange(1, k + 1)[:, None] * np.array([np.sin(ang), np.cos(ang)]) + rng.normal(0, 0.3, (k, 2))
                arm = nodes(pts[:-1], 2) + nodes(pts[-1:], 1)
                path([x] + arm)
        out.append(A.Skeleton(np.concatenate(coords), A.Paths(np.array(indices, dtype=np.int64), np.array(indptr, dtype=np.int64)), np.concatenate(degrees)))
    return out


class TorchAsm:
    """The three terms of AlignLoss that reach total_loss + TensorSkeletonOptimizer with stock torch operators, as the reference runs them on the GPU"""

    def __init__(self, cfg, ts, indicator, c0c2):
        self.cfg, self.ts, self.ind, self.cf = cfg, ts, indicator, c0c2
        M = ts.path_index.shape[0]
        cuts = ts.path_delim[1:-1]
        self.edge_mask = torch.ones(M - 1, device=DEV)
        self.edge_mask[cuts - 1] = 0
        self.len_mask = torch.ones(M - 2, device=DEV)
        self.len_mask[cuts - 1] = 0
        self.len_mask[cuts - 2] = 0
        self.mid_batch = ts.batch[ts.path_index[:-1]]
        self.pos = ts.pos.clone().requires_grad_(True)
        self.is_tip = ts.degrees == 1
        self.tip_pos = self.pos.detach()[self.is_tip].clone()
        self.opt = torch.optim.RMSprop([self.pos], lr=cfg["lr"], alpha=0.9)
        self.sched = torch.optim.lr_scheduler.ExponentialLR(self.opt, cfg["gamma"])

    def loss(self, it):
        pos, batch = self.pos, self.ts.batch
        pp = pos[self.ts.path_index]
        dp = pp.detach()
        t = pp[1:] - pp[:-1]
        mid = ((pp[1:] + pp[:-1]) / 2).round().long()
        H, W = self.ind.shape[-2:]
        r, col = torch.clamp(mid[:, 0], 0, H - 1), torch.clamp(mid[:, 1], 0, W - 1)
        c0, c2 = self.cf[self.mid_batch, :2, r, col], self.cf[self.mid_batch, 2:, r, col]
        norms = torch.norm(t, dim=-1)
        mask = self.edge_mask.clone()
        mask[norms < 0.1] = 0
        z = t / (norms[:, None] + 1e-6)
        mul = lambda u, v: torch.stack([u[:, 0] * v[:, 0] - u[:, 1] * v[:, 1], u[:, 0] * v[:, 1] + u[:, 1] * v[:, 0]], dim=1)
        z2 = mul(z, z)
        f = mul(z2, z2) + mul(c2, z2) + c0
        align = torch.sum((f[:, 0] ** 2 + f[:, 1] ** 2) * mask)
        y, x = pos[:, 0], pos[:, 1]
        x0, y0 = torch.floor(x).long(), torch.floor(y).long()
        x1, y1 = x0 + 1, y0 + 1
        cx0, cx1, cy0, cy1 = torch.clamp(x0, 0, W - 1), torch.clamp(x1, 0, W - 1), torch.clamp(y0, 0, H - 1), torch.clamp(y1, 0, H - 1)
        val = ((x1.float() - x) * (y1.float() - y) * self.ind[batch, cy0, cx0] + (x1.float() - x) * (y - y0.float()) * self.ind[batch, cy1, cx0]
               + (x - x0.float()) * (y1.float() - y) * self.ind[batch, cy0, cx1] + (x - x0.float()) * (y - y0.float()) * self.ind[batch, cy1, cx1])
        level = torch.sum(torch.pow(val - self.cfg["data_level"], 2))
        prev_n, next_n = torch.norm(pp[1:-1] - dp[:-2], dim=-1), torch.norm(dp[2:] - pp[1:-1], dim=-1)
        length = torch.sum((torch.pow(prev_n, 2) + torch.pow(next_n, 2)) * self.len_mask)
        losses = {"align": align.item(), "level": level.item(), "length": length.item()}
        data_coef, length_coef, crossfield_coef, _ = A.asm_schedule(it, self.cfg)
        return data_coef * level + length_coef * length + crossfield_coef * align, losses

    def optimize(self, steps):
        for it in range(steps):
            self.opt.zero_grad()
            total, _ = self.loss(it)
            total.backward()
            self.opt.step()
            with torch.no_grad():
                self.pos[self.is_tip] = self.tip_pos
            self.sched.step()
        return self.pos.detach()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--torch-repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-only", action="store_true", help="time (a) alone")
    ap.add_argument("--no-junctions", action="store_true", help="the contours alone: what a step costs when no node has more than one occurrence but the closing ones")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "asm_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_asm.py measures on the GPU: none visible (no CPU fall-back)")
    import warnings
    warnings.filterwarnings("ignore")
    cfg = A.ASM_DEFAULTS
    knots = A._knots(cfg)
    seg, cf, contours = synthetic(args.batch, seed=7)
    seg, cf = seg.to(DEV), cf.to(DEV)
    sks = skeletons(contours, seed=8, junctions=not args.no_junctions)
    ts = A.skeletons_to_tensorskeleton(sks, device=DEV)
    ind = seg[:, 0].contiguous()
    plan = ts.plan
    sizes = np.diff(plan.comp_ptr.cpu().numpy())
    res = {"tool": "bench_asm", "gpu": torch.cuda.get_device_name(0), "size": S, "batch": args.batch, "steps": args.steps, "nodes": int(ts.num_nodes),
           "path_entries": int(ts.path_index.shape[0]), "paths": int(ts.num_paths), "components": int(plan.num_comps), "largest_component": int(plan.max_comp),
           "median_component": int(np.median(sizes)), "junctions": int((ts.degrees > 2).sum()), "tips": int((ts.degrees == 1).sum()), "repeats": args.repeats,
           "torch_repeats": args.torch_repeats, "warmup": args.warmup, "library": os.path.basename(LIB_PATH)}
    pos0 = ts.pos.clone()
    work, sq = torch.empty_like(pos0), torch.empty_like(pos0)
    is_tip, batch = (ts.degrees == 1).to(torch.uint8), ts.batch.to(torch.int32)

    def kernel(_=None, **kw):
        hip.asm_optimize(work, sq, plan, is_tip, batch, ind, cf, knots, data_level=cfg["data_level"], lr=cfg["lr"], gamma=cfg["gamma"], steps=args.steps, **kw)

    def reset():
        work.copy_(pos0)
        sq.zero_()

    res["a_kernel"] = timed(kernel, args.repeats, args.warmup, reset)
    mine = work.clone()
    res["a_kernel"]["us_per_step"] = round(res["a_kernel"]["median_us"] / args.steps, 3)
    if args.kernel_only:
        line = json.dumps(res)
        print(line)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
        return
    res["b_fallback"] = timed(lambda _: kernel(force_fallback=True), max(args.repeats // 4, 3), 1, reset)
    res["b_fallback"]["us_per_step"] = round(res["b_fallback"]["median_us"] / args.steps, 3)
    res["fallback_bits_equal"] = bool(torch.equal(work, mine))
    res["a_public_interface_with_host_conversion"] = timed(lambda _: A.optimize_skeletons(seg, cf, sks, cfg), 3, 1)
    theirs = []
    res["c_torch"] = timed(lambda t: theirs.append(t.optimize(args.steps)), args.torch_repeats, 1, lambda: TorchAsm(cfg, ts, ind, cf))
    res["c_torch"]["us_per_step"] = round(res["c_torch"]["median_us"] / args.steps, 3)
    dev = (mine - theirs[-1]).abs()
    # free-running fp32 trajectories drift apart (the reference's own fp32 and float64 runs do): reported, not a parity check
    res["kernel_vs_torch_after_all_steps"] = {"median_px": float(dev.median()), "share_over_0.05_px": float((dev > 0.05).float().mean()),
                                              "moved_median_px": float((mine - pos0).abs().median())}
    res["torch_over_kernel"] = round(res["c_torch"]["median_us"] / res["a_kernel"]["median_us"], 1)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
