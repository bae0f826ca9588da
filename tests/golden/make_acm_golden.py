"""Golden vectors for the FFL active-contour optimiser: the reference's own `contours_batch_to_tensorpoly`, `TensorPolyOptimizer` and `PolygonAlignLoss`
(predict/ffl/polygonize_acm.py:77-229) with its `tensorpoly.py` and `bilinear_interpolate`, run on the CPU.  Build-container only (imports the reference);
emits tests/golden/acm.npz (arrays only).  skimage / shapely / cv2 / omegaconf / lydorn_utils are stubs: nothing of them runs in these classes.
tensorpoly.py, functionnal.py and complex.py are loaded by file path because their package's __init__ imports torchvision.

Besides the inputs and the reference's outputs after 1 and 5 steps the file holds what the reference's fp32 run differs from ITS OWN float64 run by:
the tolerances of tests/test_acm_gpu.py are multiples of those numbers, not of anything the kernel produced."""
import importlib.machinery
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import acm_ref as R  # noqa: E402

REF = "/root/reference"
LYDORN = REF + "/ffl_submodules/pytorch_lydorn/torch_lydorn"
B, H, W = 2, 32, 40
CFG = dict(R.DEFAULTS)


def _stub(name, pkg=False):
    m = types.ModuleType(name)
    m.__spec__ = importlib.machinery.ModuleSpec(name, None, is_package=pkg)          # torch.optim's dynamo hooks look at __spec__
    if pkg:
        m.__path__ = []
    sys.modules[name] = m
    parent, _, leaf = name.rpartition(".")
    if parent:
        setattr(sys.modules[parent], leaf, m)
    return m


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    parent, _, leaf = name.rpartition(".")
    if parent:
        setattr(sys.modules[parent], leaf, m)
    spec.loader.exec_module(m)
    return m


def load_reference():
    for name in ("skimage", "shapely", "lydorn_utils", "torch_lydorn", "torch_lydorn.torch", "torch_lydorn.torch.nn", "torch_lydorn.torch.utils",
                 "torch_lydorn.torchvision", "pixelspointspolygons", "pixelspointspolygons.predict", "pixelspointspolygons.predict.ffl",
                 "pixelspointspolygons.models", "pixelspointspolygons.models.ffl"):
        _stub(name, pkg=True)
    for name in ("skimage.measure", "skimage.io", "shapely.geometry", "shapely.ops", "shapely.prepared", "cv2", "omegaconf", "lydorn_utils.math_utils",
                 "lydorn_utils.python_utils", "lydorn_utils.print_utils", "pixelspointspolygons.predict.ffl.polygonize_utils"):
        _stub(name)
    if "tqdm" not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:
            _stub("tqdm").tqdm = lambda it, **k: it
    _load("torch_lydorn.torch.utils.complex", LYDORN + "/torch/utils/complex.py")
    _load("torch_lydorn.torch.nn.functionnal", LYDORN + "/torch/nn/functionnal.py")
    tr = _stub("torch_lydorn.torchvision.transforms", pkg=True)
    tp = _load("torch_lydorn.torchvision.transforms.tensorpoly", LYDORN + "/torchvision/transforms/tensorpoly.py")
    tr.polygons_to_tensorpoly, tr.tensorpoly_pad, tr.tensorpoly = tp.polygons_to_tensorpoly, tp.tensorpoly_pad, tp
    _load("pixelspointspolygons.models.ffl.frame_field_utils", REF + "/pixelspointspolygons/models/ffl/frame_field_utils.py")
    return _load("pixelspointspolygons.predict.ffl.polygonize_acm", REF + "/pixelspointspolygons/predict/ffl/polygonize_acm.py")


def scene(seed):
    """-> indicator [B,H,W], c0c2 [B,4,H,W] (fp32) and the initial contours per image (float64 [n,2] (row, col); closed ones repeat their first point)"""
    rng = np.random.default_rng(seed)
    rr, cc = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ind, cf, contours = [], [], []
    for (cr, cx, a, b, ang) in ((16.0, 20.0, 12.0, 8.0, 0.3), (15.0, 21.0, 11.0, 7.0, -0.5)):
        u = (cc - cx) * np.cos(ang) + (rr - cr) * np.sin(ang)           # along the rectangle's long side (x = col, y = row)
        v = -(cc - cx) * np.sin(ang) + (rr - cr) * np.cos(ang)
        qx, qy = np.abs(u) - a, np.abs(v) - b
        sd = -(np.hypot(np.maximum(qx, 0), np.maximum(qy, 0)) + np.minimum(np.maximum(qx, qy), 0))          # > 0 inside
        ind.append(1 / (1 + np.exp(-sd / 1.5)) + rng.normal(0, 0.02, (H, W)))
        theta = ang + 0.1 * np.sin(cc / 7) + rng.normal(0, 0.05, (H, W))
        c0 = -np.exp(4j * theta)
        c2 = rng.normal(0, 0.05, (H, W)) + 1j * rng.normal(0, 0.05, (H, W))
        cf.append(np.stack([c0.real, c0.imag, c2.real, c2.imag]))
        # closed ring: ~1 px steps along the rectangle's outline, jittered
        corners = np.array([(-a, -b), (a, -b), (a, b), (-a, b), (-a, -b)])
        ring = []
        for p0, p1 in zip(corners[:-1], corners[1:]):
            k = int(round(np.linalg.norm(p1 - p0)))
            ring += [p0 + (p1 - p0) * t / k for t in range(k)]
        ring = np.array(ring)
        ring = np.stack([cr + ring[:, 0] * np.sin(ang) + ring[:, 1] * np.cos(ang), cx + ring[:, 0] * np.cos(ang) - ring[:, 1] * np.sin(ang)], 1)
        ring += rng.normal(0, 0.3, ring.shape)
        ring = np.concatenate([ring, ring[:1]])
        t = np.linspace(0, 1, 40)[:, None]
        ends = np.array([0.0, 6.3]), np.array([24.4, W - 1.0])             # top border to right border; the closing edge's midpoint is no rounding tie
        line = ends[0] * (1 - t) + ends[1] * t + rng.normal(0, 0.3, (40, 2))
        line[0], line[-1] = ends                                           # the endpoints stay where they are
        w = np.arange(5) * 2 * np.pi / 5
        small = np.stack([6.0 + 3 * np.sin(w), 33.0 + 3 * np.cos(w)], 1) + rng.normal(0, 0.3, (5, 2))
        small = np.concatenate([small, small[:1]])
        contours.append([ring, line, small])
    return torch.tensor(np.stack(ind), dtype=torch.float32), torch.tensor(np.stack(cf), dtype=torch.float32), contours


def make_optimizer(acm, contours, ind, cf, cfg, dtype, pos=None, first_iter=0):
    tp = acm.contours_batch_to_tensorpoly(contours)
    if pos is not None:
        tp.pos = pos.clone()
    tp.pos = tp.pos.to(dtype)
    opt = acm.TensorPolyOptimizer(cfg, tp, ind.to(dtype), cf.to(dtype), cfg["data_coef"], cfg["length_coef"], cfg["crossfield_coef"])
    if first_iter:
        opt.lr_scheduler.last_epoch = first_iter - 1
        opt.lr_scheduler.step()
    return opt


def main():
    import warnings
    warnings.filterwarnings("ignore")
    acm = load_reference()
    for seed in range(20, 60):
        ind, cf, contours = scene(seed)
        tp = acm.contours_batch_to_tensorpoly(contours)
        margin = R.decision_margin(tp.pos, tp.poly_slice)
        if margin > 1e-4:
            break
    else:
        raise SystemExit("no seed with a decision margin over 1e-4")
    print("seed", seed, "decision margin at step 0:", margin, "vertices:", tp.pos.shape[0])
    out = {"seed": np.array(seed), "margin0": np.array(margin), "indicator": ind.numpy(), "c0c2": cf.numpy(),
           "contours.flat": np.concatenate([c for cs in contours for c in cs]), "contours.len": np.array([len(c) for cs in contours for c in cs]),
           "contours.image": np.array([b for b, cs in enumerate(contours) for _ in cs]),
           "tp.pos": tp.pos.numpy().copy(), "tp.poly_slice": tp.poly_slice.numpy(), "tp.batch": tp.batch.numpy(), "tp.is_endpoint": tp.is_endpoint.numpy(),
           "tp.batch_size": np.array(tp.batch_size), "tp.to_padded_index": tp.to_padded_index.numpy()}
    pos0 = tp.pos.clone()

    # ---- the reference's fp32 run: learning rates, positions and losses after 1 and 5 steps, positions every 5 steps (the re-synchronised comparison)
    opt = make_optimizer(acm, contours, ind, cf, CFG, torch.float32)
    lrs, every5 = [], [pos0.clone()]
    for i in range(CFG["steps"]):
        lrs.append(opt.optimizer.param_groups[0]["lr"])
        loss, parts = opt.step(i)
        if i + 1 in (1, 5):
            out[f"ref32.pos{i + 1}"] = opt.tensorpoly.pos.detach().numpy().copy()
            out[f"ref32.loss{i + 1}"] = np.array([loss, parts["align"], parts["level"], parts["length"]], dtype=np.float64)
        if (i + 1) % 5 == 0:
            every5.append(opt.tensorpoly.pos.detach().clone())
    out["lrs"] = np.array(lrs, dtype=np.float64)

    # ---- reference alone, re-synchronised: its float64 run of the same 5 iterations from the fp32 run's positions at the start of each chunk
    devs = []
    for k in range(CFG["steps"] // 5):
        o64 = make_optimizer(acm, contours, ind, cf, CFG, torch.float64, pos=every5[k], first_iter=5 * k)
        assert abs(o64.optimizer.param_groups[0]["lr"] - lrs[5 * k]) < 1e-15
        for i in range(5 * k, 5 * k + 5):
            o64.step(i)
        devs.append((every5[k + 1].double() - o64.tensorpoly.pos.detach()).abs())
    devs = torch.cat(devs).reshape(-1)
    out["alone.traj"] = np.array([float((devs > 1e-4).double().mean()), float(devs.max()), float(devs.median())])
    print("reference alone, 100 x 5 steps: share over 1e-4 = %.3g, worst = %.3g, median = %.3g" % tuple(out["alone.traj"]))

    # ---- reference alone, one step at poly_lr = 1 without warm-up (delta pos = -grad): fp32 against float64 from the same fp32 inputs
    g = dict(CFG, poly_lr=1.0, warmup_iters=0)
    o32, o64 = make_optimizer(acm, contours, ind, cf, g, torch.float32), make_optimizer(acm, contours, ind, cf, g, torch.float64)
    o32.step(0); o64.step(0)
    dev = (o32.tensorpoly.pos.detach().double() - o64.tensorpoly.pos.detach()).abs()
    out["alone.grad"] = np.array([float(dev.max())])
    out["ref64.grad_pos1"] = o64.tensorpoly.pos.detach().numpy().copy()
    print("reference alone, one step at lr 1: max |fp32 - float64| = %.3g (largest move %.3g)" % (float(dev.max()), float((o64.tensorpoly.pos.detach() - pos0.double()).abs().max())))

    # ---- the restatement the GPU tests use reproduces the reference (asserted again by tests/test_acm_cpu.py)
    pos, sl, batch, ep = R.container(contours)
    assert torch.equal(pos.float(), pos0) and torch.equal(sl, tp.poly_slice) and torch.equal(batch, tp.batch) and torch.equal(ep, tp.is_endpoint)
    for n in (1, 5):
        mine, last = R.optimize(pos0, sl, batch, ep, ind, cf, CFG, steps=n, dtype=torch.float32)
        print(f"restatement fp32 after {n} steps: max |pos - reference| = %.3g, losses rel %.3g" % (
            float((mine - torch.from_numpy(out[f'ref32.pos{n}'])).abs().max()), float(np.max(np.abs(np.array(last) / out[f'ref32.loss{n}'] - 1)))))
    np.savez_compressed(os.path.join(HERE, "acm.npz"), **out)
    print("wrote acm.npz", os.path.getsize(os.path.join(HERE, "acm.npz")), "bytes")


if __name__ == "__main__":
    main()
