"""The FFL active-skeleton optimiser (predict/ffl/polygonize_asm.py:177-235, 342-353, 361-421) restated with torch operators and autograd on the CPU, in
float32 or float64, for the tests of p3_asm_optimize: the three terms of the reference's total_loss (level, length, align), scipy's linear interp1d,
ExponentialLR and RMSprop(alpha=0.9).  tests/test_asm_cpu.py pins it to the reference's own classes through tests/golden/asm.npz.  Test infrastructure
only: the product never imports it."""
import numpy as np
import torch

KNOTS = dict(step_thresholds=[0, 100, 200, 300], data=[1.0, 0.1, 0.0, 0.0], crossfield=[0.0, 0.05, 0.0, 0.0], length=[0.1, 0.01, 0.0, 0.0])
DEFAULTS = dict(data_level=0.5, lr=0.1, gamma=0.995, coefs=KNOTS)
ALIGN_ONLY = dict(DEFAULTS, coefs=dict(step_thresholds=[0, 100, 200, 300], data=[0.0] * 4, crossfield=[1.0] * 4, length=[0.0] * 4))
ALL_ZERO = dict(DEFAULTS, coefs=dict(step_thresholds=[0, 100, 200, 300], data=[0.0] * 4, crossfield=[0.0] * 4, length=[0.0] * 4))


def config_of(cfg):
    """the reference-shaped config dict (what TensorSkeletonOptimizer takes) of a restatement config"""
    z = [0.0] * len(cfg["coefs"]["step_thresholds"])
    return {"data_level": cfg["data_level"], "lr": cfg["lr"], "gamma": cfg["gamma"],
            "loss_params": {"coefs": dict(cfg["coefs"], curvature=z, corner=z, junction=z), "curvature_dissimilarity_threshold": 2, "corner_angles": [45, 90, 135],
                            "corner_angle_threshold": 22.5, "junction_angles": [0, 45, 90, 135], "junction_angle_weights": [1, 0.01, 0.1, 0.01],
                            "junction_angle_threshold": 22.5}}


def interp(x, y, i):
    """scipy.interpolate.interp1d(x, y)(i), linear.  scipy hands 1-d float tables to numpy.interp: the segment with x_lo <= i < x_hi, so a knot gives its
    own value exactly (interp1d's own searchsorted form takes the segment below a knot and can land one ulp beside it)"""
    lo = int(np.clip(np.searchsorted(np.asarray(x, dtype=np.float64), i, side="right") - 1, 0, len(x) - 2))
    hi = lo + 1
    if i == x[hi]:
        return y[hi]
    slope = (y[hi] - y[lo]) / (x[hi] - x[lo])
    return slope * (i - x[lo]) + y[lo]


def schedule(i, cfg):
    """-> (data, length, crossfield, lr) at iteration i as Python floats"""
    c = cfg["coefs"]
    lr = cfg["lr"]
    for _ in range(i):
        lr = lr * cfg["gamma"]
    return interp(c["step_thresholds"], c["data"], i), interp(c["step_thresholds"], c["length"], i), interp(c["step_thresholds"], c["crossfield"], i), lr


def path_ends(path_delim, M):
    """-> (is_start [M], is_end [M]) bool: the interior delimiters split path_index, as AlignLoss reads them"""
    start, end = torch.zeros(M, dtype=torch.bool), torch.zeros(M, dtype=torch.bool)
    if M:
        cuts = path_delim[1:-1]
        cuts = cuts[(cuts >= 1) & (cuts <= M - 1)]
        start[0] = end[M - 1] = True
        start[cuts] = True
        end[cuts - 1] = True
    return start, end


def _bilinear(im, pos, batch):
    y, x = pos[:, 0], pos[:, 1]
    x0, y0 = torch.floor(x).long(), torch.floor(y).long()
    x1, y1 = x0 + 1, y0 + 1
    H, W = im.shape[-2:]
    cx0, cx1, cy0, cy1 = x0.clamp(0, W - 1), x1.clamp(0, W - 1), y0.clamp(0, H - 1), y1.clamp(0, H - 1)
    t = pos.dtype
    return ((x1.to(t) - x) * (y1.to(t) - y) * im[batch, cy0, cx0] + (x1.to(t) - x) * (y - y0.to(t)) * im[batch, cy1, cx0]
            + (x - x0.to(t)) * (y1.to(t) - y) * im[batch, cy0, cx1] + (x - x0.to(t)) * (y - y0.to(t)) * im[batch, cy1, cx1])


def losses(pos, path_index, path_delim, batch, indicator, c0c2, level):
    """-> (align, level, length) sums; pos [N,2] in any float dtype, maps in the same"""
    M = path_index.shape[0]
    start, end = path_ends(path_delim, M)
    lv = ((_bilinear(indicator, pos, batch) - level) ** 2).sum() if pos.shape[0] else pos.sum()
    if M < 2:
        return pos.sum() * 0, lv, pos.sum() * 0
    pp = pos[path_index]
    dp = pp.detach()
    k = torch.nonzero(~end[:-1])[:, 0]                      # edges (k, k + 1) inside a path
    a, b = pp[k], pp[k + 1]
    t = b - a
    mid = ((b + a) / 2).round().long()
    H, W = indicator.shape[-2:]
    r, c = mid[:, 0].clamp(0, H - 1), mid[:, 1].clamp(0, W - 1)
    bi = batch[path_index[k]]
    c0, c2 = c0c2[bi, :2, r, c], c0c2[bi, 2:, r, c]
    norm = torch.norm(t, dim=-1)
    mask = (~(norm.detach() < 0.1)).to(pos.dtype)
    z = t / (norm[:, None] + 1e-6)
    mul = lambda u, v: torch.stack([u[:, 0] * v[:, 0] - u[:, 1] * v[:, 1], u[:, 0] * v[:, 1] + u[:, 1] * v[:, 0]], dim=1)
    z2 = mul(z, z)
    f = mul(z2, z2) + mul(c2, z2) + c0
    al = ((f[:, 0] ** 2 + f[:, 1] ** 2) * mask).sum()
    j = torch.nonzero(~start & ~end)[:, 0]                  # interior occurrences
    ln = (torch.norm(pp[j] - dp[j - 1], dim=-1) ** 2 + torch.norm(dp[j + 1] - pp[j], dim=-1) ** 2).sum()
    return al, lv, ln


def gradient(pos, ts, indicator, c0c2, cfg, i, dtype=torch.float64):
    """-> (grad [N,2] in `dtype`, (total, align, level, length) floats) of iteration i's loss at pos"""
    p = pos.detach().to(dtype).clone().requires_grad_(True)
    al, lv, ln = losses(p, ts["path_index"], ts["path_delim"], ts["batch"], indicator.to(dtype), c0c2.to(dtype), cfg["data_level"])
    wd, wl, wc, _ = schedule(i, cfg)
    total = wd * lv + wl * ln + wc * al
    g, = torch.autograd.grad(total, p, allow_unused=True)
    g = torch.zeros_like(p) if g is None else g
    return g, tuple(float(v.detach()) for v in (total, al, lv, ln))


def rmsprop(pos, sq, g, lr, is_tip):
    """one torch.optim.RMSprop(alpha=0.9, eps=1e-8) step in the tensors' dtype, tips put back: -> (pos, sq)"""
    sq = 0.9 * sq + 0.1 * g * g
    new = pos - lr * (g / (sq.sqrt() + 1e-8))
    return torch.where(is_tip[:, None], pos, new), sq


def optimize(pos, sq, ts, indicator, c0c2, cfg, first_iter=0, steps=1, dtype=torch.float64):
    """`steps` iterations from (pos, sq) computed in `dtype`: -> (pos, sq, (total, align, level, length) of the last step)"""
    p, s = pos.detach().to(dtype).clone(), sq.detach().to(dtype).clone()
    tip, last = ts["degrees"] == 1, None
    for i in range(first_iter, first_iter + steps):
        g, last = gradient(p, ts, indicator, c0c2, cfg, i, dtype)
        p, s = rmsprop(p, s, g, schedule(i, cfg)[3], tip)
    return p, s, last


def decision_margin(pos, ts):
    """smallest distance of a quantity of one step from `pos` to a floor / round / 0.1 decision (float64): below it fp32 and float64 may decide differently.
    A coordinate that IS an integer is no floor decision (both precisions hold it exactly); an edge of length exactly 0 (a node beside itself) is no
    0.1 decision."""
    p = pos.detach().double()
    fl = torch.minimum(p - p.floor(), p.ceil() - p)
    fl = torch.where(p == p.floor(), torch.ones_like(fl), fl)
    M = ts["path_index"].shape[0]
    out = [fl.min()] if p.numel() else []
    if M >= 2:
        _, end = path_ends(ts["path_delim"], M)
        k = torch.nonzero(~end[:-1])[:, 0]
        a, b = p[ts["path_index"][k]], p[ts["path_index"][k + 1]]
        mid = (a + b) / 2
        out.append(((mid - mid.floor()) - 0.5).abs().min())
        nm = (b - a).norm(dim=-1)
        out.append(torch.where(nm == 0, torch.ones_like(nm), (nm - 0.1).abs()).min())
    return float(min(out)) if out else 1.0


def tensors_of(d, prefix="ts."):
    """the fixture's container as a dict of tensors"""
    return {k: d[prefix + k] for k in ("pos", "degrees", "path_index", "path_delim", "batch", "batch_delim")}


def skeleton_arrays_of(d):
    """the fixture's skeletons per image: [(coordinates float64 [n,2], indices, indptr, degrees)]"""
    out = []
    for b in range(int(d["ts.batch_size"])):
        out.append(tuple(d[f"sk{b}.{k}"].numpy() for k in ("coordinates", "indices", "indptr", "degrees")))
    return out
