"""The FFL active-contour optimiser on one GPU: 224 x 224, B = 16, seeded synthetic contours (a dozen building outlines of 60 - 250 vertices at ~1 px
spacing and two open border-to-border polylines per image), 500 steps of the shipped acm_method config.
  (a) hip.acm_optimize: one launch for all steps (csrc/acm.hip, the LDS path),
  (b) the same call through the one-launch-per-step fallback (what a polygon over the LDS cap costs),
  (c) the same algorithm written with stock torch operators on the same GPU the way the reference runs its own (predict/ffl/polygonize_acm.py:77-220):
      fp32, autograd, torch.optim.SGD + LambdaLR, three .item() reads per step.

    python tools/bench_acm.py [--batch 16] [--steps 500] [--repeats 20] [--torch-repeats 3] [--kernel-only] [--out profiles/acm_bench.json]

Every timed run starts from the same initial contours, between its own pair of HIP events after warm-up runs; medians (min, max beside them).  What a run
needs first (the copy of the initial positions for (a) and (b); the index build, the SGD optimizer and the LambdaLR of (c)) is done before its first event.
--kernel-only times (a) alone: for a second build of the library chosen with P3HIP_LIB (tools/build_variant.sh), e.g. another workgroup size.
Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pixelspointspolygons_amd import hip  # noqa: E402
from pixelspointspolygons_amd import polygonize_acm as A  # noqa: E402
from pixelspointspolygons_amd._lib import LIB_PATH  # noqa: E402

DEV = "cuda"
S = 224


def synthetic(B, seed):
    """-> seg [B,1,S,S], c0c2 [B,4,S,S] (fp32, host) and the initial contours per image"""
    rng = np.random.default_rng(seed)
    rr, cc = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    seg, cf, contours = [], [], []
    for _ in range(B):
        sd = np.full((S, S), -50.0)
        theta = np.zeros((S, S))
        cs = []
        for _ in range(12):
            a, b = rng.uniform(8, 34), rng.uniform(7, 28)
            cr, cx, ang = rng.uniform(40, S - 40), rng.uniform(40, S - 40), rng.uniform(0, np.pi / 2)
            u = (cc - cx) * np.cos(ang) + (rr - cr) * np.sin(ang)
            v = -(cc - cx) * np.sin(ang) + (rr - cr) * np.cos(ang)
            qx, qy = np.abs(u) - a, np.abs(v) - b
            d = -(np.hypot(np.maximum(qx, 0), np.maximum(qy, 0)) + np.minimum(np.maximum(qx, qy), 0))
            theta = np.where(d > sd, ang, theta)
            sd = np.maximum(sd, d)
            corners = np.array([(-a, -b), (a, -b), (a, b), (-a, b), (-a, -b)])
            ring = []
            for p0, p1 in zip(corners[:-1], corners[1:]):
                k = max(int(round(np.linalg.norm(p1 - p0))), 1)
                ring += [p0 + (p1 - p0) * t / k for t in range(k)]
            ring = np.array(ring)
            ring = np.stack([cr + ring[:, 0] * np.sin(ang) + ring[:, 1] * np.cos(ang), cx + ring[:, 0] * np.cos(ang) - ring[:, 1] * np.sin(ang)], 1)
            ring += rng.normal(0, 0.3, ring.shape)
            cs.append(np.concatenate([ring, ring[:1]]))
        for _ in range(2):
            t = np.linspace(0, 1, 80)[:, None]
            p0, p1 = np.array([0.0, rng.uniform(5, S - 5)]), np.array([rng.uniform(5, S - 5), S - 1.0])
            line = p0 * (1 - t) + p1 * t + rng.normal(0, 0.3, (80, 2))
            line[0], line[-1] = p0, p1
            cs.append(line)
        seg.append(1 / (1 + np.exp(-sd / 1.5)) + rng.normal(0, 0.02, (S, S)))
        th = theta + rng.normal(0, 0.05, (S, S))
        c0 = -np.exp(4j * th)
        c2 = rng.normal(0, 0.05, (S, S)) + 1j * rng.normal(0, 0.05, (S, S))
        cf.append(np.stack([c0.real, c0.imag, c2.real, c2.imag]))
        contours.append(cs)
    return torch.tensor(np.stack(seg), dtype=torch.float32)[:, None], torch.tensor(np.stack(cf), dtype=torch.float32), contours


class TorchAcm:
    """PolygonAlignLoss + TensorPolyOptimizer with stock torch operators, as the reference runs them on the GPU"""

    def __init__(self, cfg, tp, indicator, c0c2):
        self.cfg, self.tp, self.ind, self.cf = cfg, tp, indicator, c0c2
        n = tp.pos.shape[0]
        nxt = torch.arange(n, device=DEV) + 1
        nxt[tp.poly_slice[:, 1] - 1] = tp.poly_slice[:, 0]
        self.nxt = nxt
        self.pos = tp.pos.clone().requires_grad_(True)
        self.keep = self.pos.detach()[tp.is_endpoint].clone()
        self.opt = torch.optim.SGD([self.pos], lr=cfg["poly_lr"])
        wi, wf = cfg["warmup_iters"], cfg["warmup_factor"]
        self.sched = torch.optim.lr_scheduler.LambdaLR(self.opt, lr_lambda=lambda i: A.lr_coef(i, wi, wf))

    def loss(self):
        c, pos, batch = self.cfg, self.pos, self.tp.batch
        a, b = pos, pos[self.nxt]
        e = b - a
        mid = ((b + a) / 2).round().long()
        H, W = self.ind.shape[-2:]
        r, col = torch.clamp(mid[:, 0], 0, H - 1), torch.clamp(mid[:, 1], 0, W - 1)
        c0, c2 = self.cf[batch, :2, r, col], self.cf[batch, 2:, r, col]
        norms = torch.norm(e, dim=-1)
        mask = torch.ones_like(norms)
        mask[norms < 0.1] = 0
        z = e / (norms[:, None] + 1e-3)
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
        level = torch.sum(torch.pow(val - c["data_level"], 2))
        length = torch.sum(torch.pow(norms * mask, 2))
        losses = {"align": align.item(), "level": level.item(), "length": length.item()}          # the reference reads all three every step
        total = (c["data_coef"] * level + c["length_coef"] * length + c["crossfield_coef"] * align) / (c["data_coef"] + c["length_coef"] + c["crossfield_coef"])
        return total, losses

    def optimize(self, steps):
        for _ in range(steps):
            self.opt.zero_grad()
            total, _ = self.loss()
            total.backward()
            self.opt.step()
            self.sched.step()
            with torch.no_grad():
                self.pos[self.tp.is_endpoint] = self.keep
        return self.pos.detach()


def timed(fn, n, warmup, setup=lambda: None):
    """fn(setup()) n times after `warmup` untimed ones; setup runs before the first event of its run"""
    for _ in range(warmup):
        fn(setup())
    torch.cuda.synchronize()
    us = []
    for _ in range(n):
        arg = setup()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(arg)
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--torch-repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "acm_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_acm.py measures on the GPU: none visible (no CPU fall-back)")
    import warnings
    warnings.filterwarnings("ignore")
    cfg = dict(A.ACM_DEFAULTS, steps=args.steps)
    seg, cf, contours = synthetic(args.batch, seed=7)
    seg, cf = seg.to(DEV), cf.to(DEV)
    tp = A.contours_batch_to_tensorpoly(contours).to(DEV)
    ind = seg[:, 0].contiguous()
    lens = (tp.poly_slice[:, 1] - tp.poly_slice[:, 0]).cpu()
    res = {"tool": "bench_acm", "gpu": torch.cuda.get_device_name(0), "size": S, "batch": args.batch, "steps": args.steps, "polygons": int(lens.numel()),
           "vertices": int(tp.num_nodes), "longest": int(lens.max()), "median_length": int(lens.median()), "repeats": args.repeats,
           "torch_repeats": args.torch_repeats, "warmup": args.warmup}
    pos0 = tp.pos.clone()
    work = torch.empty_like(pos0)

    def kernel(_=None, **kw):
        hip.acm_optimize(work, tp.poly_slice, tp.batch, tp.is_endpoint, ind, cf, cfg["data_coef"], cfg["length_coef"], cfg["crossfield_coef"],
                         data_level=cfg["data_level"], poly_lr=cfg["poly_lr"], warmup_iters=cfg["warmup_iters"], warmup_factor=cfg["warmup_factor"],
                         steps=args.steps, max_len=tp.max_len, **kw)

    def reset():
        work.copy_(pos0)

    def finish():
        line = json.dumps(res)
        print(line)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")

    res["library"] = os.path.basename(LIB_PATH)
    res["a_kernel"] = timed(kernel, args.repeats, args.warmup, reset)
    mine = work.clone()
    res["a_kernel"]["us_per_step"] = round(res["a_kernel"]["median_us"] / args.steps, 3)
    if args.kernel_only:
        return finish()
    res["b_fallback"] = timed(lambda _: kernel(force_fallback=True), max(args.repeats // 4, 3), 1, reset)
    res["b_fallback"]["us_per_step"] = round(res["b_fallback"]["median_us"] / args.steps, 3)
    res["fallback_bits_equal"] = bool(torch.equal(work, mine))
    res["a_public_interface_with_host_conversion"] = timed(lambda _: A.optimize_contours(seg, cf, contours, cfg), 3, 1)
    theirs = []
    res["c_torch"] = timed(lambda t: theirs.append(t.optimize(args.steps)), args.torch_repeats, 1, lambda: TorchAcm(cfg, tp, ind, cf))
    res["c_torch"]["us_per_step"] = round(res["c_torch"]["median_us"] / args.steps, 3)
    dev = (mine - theirs[-1]).abs()
    # free-running fp32 trajectories drift apart (the reference's own fp32 and float64 runs do): reported, not a parity check
    res["kernel_vs_torch_after_all_steps"] = {"median_px": float(dev.median()), "share_over_0.05_px": float((dev > 0.05).float().mean()),
                                              "moved_median_px": float((mine - pos0).abs().median())}
    res["torch_over_kernel"] = round(res["c_torch"]["median_us"] / res["a_kernel"]["median_us"], 1)
    finish()


if __name__ == "__main__":
    main()
