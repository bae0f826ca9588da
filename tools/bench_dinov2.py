"""DINOv2 ViT-S/14 Pix2Poly (vit_dinov2) on one GPU: train-step tiles/s and encoder-forward ms, beside the ViT-S/8 image model (bench.py --workload image_s8)
measured in the same process, plus the patch-embed A/B of the two legal leading dimensions of the padded K = 588 rows (608 / 640).

    python tools/bench_dinov2.py [--batch 64] [--steps 30] [--warmup 5] [--precisions bf16,fp32x3]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_dinov2.py --profile 10 --precisions bf16       (kernel shares; no timing)

Timing discipline of bench.py: two eager steps, the step (forward + CE + 10 * BCE + backward + AdamW) captured in one hipGraph, warm-up replays, then every
timed replay between its own pair of HIP events; the median of >= 20 is reported.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pixelspointspolygons_amd import ops, synthetic as S, vision_transformer as VT  # noqa: E402
from pixelspointspolygons_amd.config import make_config  # noqa: E402
from pixelspointspolygons_amd.pix2poly import Pix2PolyModel, Tokenizer  # noqa: E402
from pixelspointspolygons_amd.training import FlatAdamW, pix2poly_loss  # noqa: E402

DEV = "cuda"


def timed(fn, n, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def measure(encoder, precision, args, profile=0):
    ops.reset_process_state()
    cfg = make_config(encoder, precision=precision, device=DEV, batch_size=args.batch)
    torch.manual_seed(0)
    m = Pix2PolyModel(cfg, Tokenizer(cfg).vocab_size, 0).train()
    opt = FlatAdamW(m, compute_dtype=VT.compute_dtype(cfg))
    inp = {k: v.to(DEV) for k, v in S.make_inputs(args.batch, seed=1).items()}
    ops.manual_seed(7, DEV)

    def fwd_bwd():
        opt.zero_grad()
        ops.advance_rng(DEV)
        logits, perm = m(inp["image"], None, inp["y"][:, :-1])
        loss = pix2poly_loss(logits, perm, inp["y"][:, 1:], inp["y_perm"])[0]
        loss.backward()
        return loss.detach()

    for _ in range(2):
        opt.prepare_step()
        loss = fwd_bwd()
        opt.apply(1.0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    opt.prepare_step()
    with torch.cuda.graph(graph):
        loss = fwd_bwd()
        opt.apply(1.0)

    def step():
        opt.prepare_step()
        graph.replay()

    if profile:
        for _ in range(profile):
            step()
        torch.cuda.synchronize()
        out = {"profiled_steps": profile, "loss": float(loss)}
    else:
        med, lo, hi = timed(step, max(args.steps, 20), args.warmup)
        out = {"step_ms": round(med, 3), "step_ms_min": round(lo, 3), "step_ms_max": round(hi, 3), "tiles_per_s": round(args.batch / med * 1e3, 1),
               "loss": float(loss)}
        assert out["loss"] == out["loss"]
        with torch.no_grad():                                    # encoder forward alone (train mode, no autograd), its own hipGraph
            for _ in range(2):
                feats = m.encoder(inp["image"])
            torch.cuda.synchronize()
            g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g2):
                feats = m.encoder(inp["image"])
            med, lo, hi = timed(g2.replay, max(args.steps, 20), args.warmup)
            out.update(encoder_fwd_ms=round(med, 3), encoder_fwd_ms_min=round(lo, 3), encoder_fwd_ms_max=round(hi, 3))
            del g2
    del graph
    opt.close()
    ops.reset_process_state()
    return out


def patch_embed_ab(precision, args):
    """patchify + patch-embed GEMM of the DINOv2 model (forward), rows padded to 608 and to 640, alternating, eager launches"""
    cfg = make_config("vit_dinov2", precision=precision, device=DEV)
    enc = VT.ViTDINOv2(cfg, bottleneck=True).to(DEV)
    img = torch.rand(args.batch, 3, 224, 224, device=DEV)
    res = {}
    was = VT.PATCH_LDK_ALIGN[0]
    try:
        with torch.no_grad():
            for rnd in range(3):
                for align in (32, 64):
                    VT.PATCH_LDK_ALIGN[0] = align
                    ldk = enc.vit.patch_embed.ldk()
                    med, lo, hi = timed(lambda: enc.vit.patch_embed.tokens(img, enc.cd), 50, 10)
                    res.setdefault(str(ldk), []).append(round(med * 1e3, 1))
    finally:
        VT.PATCH_LDK_ALIGN[0] = was
    return {"patch_embed_fwd_us_by_ldk": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precisions", default="bf16,fp32x3")
    ap.add_argument("--profile", type=int, default=0, help="run this many captured DINOv2 steps and nothing else (for rocprofv3 --kernel-trace --stats)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dinov2.py measures on the GPU: none visible (no CPU fall-back)")
    res = {"tool": "bench_dinov2", "gpu": torch.cuda.get_device_name(0), "batch": args.batch, "ldk": None, "results": {}}
    for prec in args.precisions.split(","):
        if args.profile:
            res["results"][prec] = {"vit_dinov2": measure("vit_dinov2", prec, args, profile=args.profile)}
            continue
        r = {}
        for rnd in range(2):                                     # the two models alternate: same box, same call, drift visible
            for name in ("vit_dinov2", "vit"):
                r.setdefault(name if name != "vit" else "image_s8", []).append(measure(name, prec, args))
        r.update(patch_embed_ab(prec, args))
        res["results"][prec] = r
    res["ldk"] = VT.PatchEmbed(224, 14, 3, 384).ldk()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
