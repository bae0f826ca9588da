"""The FFL active-contour optimiser (predict/ffl/polygonize_acm.py:77-220) restated with torch operators and autograd on the CPU, in float32 or
float64, for the tests of p3_acm_optimize.  tests/test_acm_cpu.py pins it to the reference's own classes through tests/golden/acm.npz.  Test
infrastructure only: the product never imports it."""
import numpy as np
import torch

DEFAULTS = dict(steps=500, data_level=0.5, data_coef=0.1, length_coef=0.4, crossfield_coef=0.5, poly_lr=0.01, warmup_iters=100, warmup_factor=0.1)


def lr_coef(i, warmup_iters, warmup_factor):
    if i < warmup_iters:
        return 1 + (warmup_factor - 1) * (warmup_iters - i) / warmup_iters
    return 1


def container(contours_batch):
    """contours per image -> (pos float64 [N,2], poly_slice int64 [P,2], batch int64 [N], is_endpoint bool [N]); a closed contour loses its repeated point"""
    pos, sl, batch, ep, at = [], [], [], [], 0
    for b, contours in enumerate(contours_batch):
        for c in contours:
            c = np.asarray(c, dtype=np.float64)
            opened = not np.max(np.abs(c[0] - c[-1])) < 1e-6
            if not opened:
                c = c[:-1]
            e = np.zeros(len(c), dtype=bool)
            if opened:
                e[0] = e[-1] = True
            pos.append(c); ep.append(e); batch.append(np.full(len(c), b)); sl.append((at, at + len(c)))
            at += len(c)
    return (torch.from_numpy(np.concatenate(pos)), torch.tensor(sl, dtype=torch.long), torch.from_numpy(np.concatenate(batch)).long(),
            torch.from_numpy(np.concatenate(ep)))


def _bilinear(im, pos, batch):
    y, x = pos[:, 0], pos[:, 1]
    x0, y0 = torch.floor(x).long(), torch.floor(y).long()
    x1, y1 = x0 + 1, y0 + 1
    H, W = im.shape[-2:]
    cx0, cx1, cy0, cy1 = x0.clamp(0, W - 1), x1.clamp(0, W - 1), y0.clamp(0, H - 1), y1.clamp(0, H - 1)
    t = pos.dtype
    return ((x1.to(t) - x) * (y1.to(t) - y) * im[batch, cy0, cx0] + (x1.to(t) - x) * (y - y0.to(t)) * im[batch, cy1, cx0]
            + (x - x0.to(t)) * (y1.to(t) - y) * im[batch, cy0, cx1] + (x - x0.to(t)) * (y - y0.to(t)) * im[batch, cy1, cx1])


def losses(pos, poly_slice, batch, indicator, c0c2, cfg, per_polygon=False):
    """-> (total, (align, level, length)); every polygon has n edges, the closing one of an open polyline included.  per_polygon: the three terms as [P] tensors"""
    nxt = torch.arange(pos.shape[0]) + 1
    nxt[poly_slice[:, 1] - 1] = poly_slice[:, 0]
    a, b = pos, pos[nxt]
    e = b - a
    mid = ((b + a) / 2).round().long()
    H, W = indicator.shape[-2:]
    r, c = mid[:, 0].clamp(0, H - 1), mid[:, 1].clamp(0, W - 1)
    c0, c2 = c0c2[batch, :2, r, c], c0c2[batch, 2:, r, c]
    norm = torch.norm(e, dim=-1)
    mask = (~(norm.detach() < 0.1)).to(pos.dtype)
    z = e / (norm[:, None] + 1e-3)
    mul = lambda u, v: torch.stack([u[:, 0] * v[:, 0] - u[:, 1] * v[:, 1], u[:, 0] * v[:, 1] + u[:, 1] * v[:, 0]], dim=1)
    z2 = mul(z, z)
    f = mul(z2, z2) + mul(c2, z2) + c0
    align = (f[:, 0] ** 2 + f[:, 1] ** 2) * mask
    length = (norm * mask) ** 2
    level = (_bilinear(indicator, pos, batch) - cfg["data_level"]) ** 2
    if per_polygon:
        seg = lambda t: torch.stack([t[s:e_].sum() for s, e_ in poly_slice.tolist()]) if len(poly_slice) else t.new_zeros(0)
        return seg(align), seg(level), seg(length)
    A, Lv, Ln = align.sum(), level.sum(), length.sum()
    total = cfg["data_coef"] * Lv + cfg["length_coef"] * Ln + cfg["crossfield_coef"] * A
    total = total / (cfg["data_coef"] + cfg["length_coef"] + cfg["crossfield_coef"])
    return total, (A, Lv, Ln)


def optimize(pos, poly_slice, batch, is_endpoint, indicator, c0c2, cfg, first_iter=0, steps=None, dtype=torch.float64):
    """`steps` iterations from `pos` (any float dtype) computed in `dtype`: -> (new pos in `dtype`, (total, align, level, length) of the last step as floats)"""
    steps = cfg["steps"] if steps is None else steps
    p = pos.detach().to(dtype).clone()
    ind, cf = indicator.to(dtype), c0c2.to(dtype)
    keep = p[is_endpoint].clone()
    last = None
    for i in range(first_iter, first_iter + steps):
        p.requires_grad_(True)
        total, parts = losses(p, poly_slice, batch, ind, cf, cfg)
        g, = torch.autograd.grad(total, p)
        lr = cfg["poly_lr"] * lr_coef(i, cfg["warmup_iters"], cfg["warmup_factor"])
        p = p.detach().add(g, alpha=-lr)
        p[is_endpoint] = keep
        last = (float(total.detach()),) + tuple(float(t.detach()) for t in parts)
    return p.detach(), last


def decision_margin(pos, poly_slice):
    """smallest distance of a quantity of one step from `pos` to a floor / round / 0.1 decision (float64): below it fp32 and float64 may decide differently.
    A coordinate that IS an integer is no floor decision (both precisions hold it exactly)."""
    p = pos.detach().double()
    nxt = torch.arange(p.shape[0]) + 1
    nxt[poly_slice[:, 1] - 1] = poly_slice[:, 0]
    fl = torch.minimum(p - p.floor(), p.ceil() - p)
    fl = torch.where(p == p.floor(), torch.ones_like(fl), fl)
    mid = (p + p[nxt]) / 2
    rd = ((mid - mid.floor()) - 0.5).abs()
    nm = ((p[nxt] - p).norm(dim=-1) - 0.1).abs()
    return float(min(fl.min(), rd.min(), nm.min()))


def contours_of(d):
    """the fixture's initial contours per image, float64 [n, 2] arrays (closed ones repeat their first point)"""
    flat, lens, image = d["contours.flat"].numpy(), d["contours.len"].tolist(), d["contours.image"].tolist()
    out, at = [[] for _ in range(int(d["tp.batch_size"]))], 0
    for n, b in zip(lens, image):
        out[b].append(flat[at:at + n])
        at += n
    return out
