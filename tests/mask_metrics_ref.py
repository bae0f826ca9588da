"""Restatement of the mask metrics (include/p3hip.h p3_mask_metrics) in numpy and Python integers: what csrc/mask_metrics.hip is held
to.  The filled masks are those of tests/poly_metrics_ref.py.  The stroked masks are decided per edge over the pixels of the edge's box widened by the
thickness, vectorised; the one product that can leave int64, the squared cross product, is taken on Python integers, so nothing here depends on a guard.
Every figure is one division of integers (the iou one addition before it), and every sum runs sequentially in image order on Python floats.
Input: per image a list of float32 [n, 2] (x, y) arrays, open rings, for the ground truth and for the predictions."""
import numpy as np

from tests import poly_metrics_ref as PR

TOPDIG, SUBSET, STATS = 1, 2, 4
KEYS = ("IoU_", "P-Acc", "F1-Score", "IoU-Topo", "P-Acc-Topo", "F1-Score-Topo", "sIoU", "sC-IoU", "sNR")
NAN = float("nan")


def ring_points(ring):
    """the integer points of a valid ring: half to even, as np.round(...).astype(np.int32) in the reference"""
    return np.round(np.asarray(ring, dtype=np.float32).astype(np.float64)).astype(np.int32)


def stroke_edge(mask, a, b, T):
    """the pixels within T / 2 of the segment (a, b) into bool mask [H, W]; pixel (r, c) is the point (c, r)"""
    H, W = mask.shape
    ax, ay, bx, by = (int(v) for v in (a[0], a[1], b[0], b[1]))
    h = (T + 1) // 2
    c0, c1 = max(min(ax, bx) - h, 0), min(max(ax, bx) + h, W - 1)
    r0, r1 = max(min(ay, by) - h, 0), min(max(ay, by) + h, H - 1)
    if c0 > c1 or r0 > r1:
        return
    px = np.arange(c0, c1 + 1, dtype=np.int64)[None, :]
    py = np.arange(r0, r1 + 1, dtype=np.int64)[:, None]
    dx, dy = bx - ax, by - ay
    ux, uy = px - ax, py - ay          # below 2^19; d below 2^17: every product but the last square stays far inside int64
    L2 = dx * dx + dy * dy
    t = ux * dx + uy * dy
    TT = T * T
    at_a = 4 * (ux * ux + uy * uy) <= TT
    at_b = 4 * ((px - bx) ** 2 + (py - by) ** 2) <= TT
    cross = (ux * dy - uy * dx).astype(object)          # Python integers: the square can pass 2^64
    inside = np.asarray(4 * cross * cross <= TT * L2, dtype=bool)
    first = np.full(t.shape, L2 == 0) | (t <= 0)
    mask[r0:r1 + 1, c0:c1 + 1] |= np.where(first, at_a, np.where(t >= L2, at_b, inside))


def stroke_mask(rings, H, W, T):
    m = np.zeros((H, W), dtype=bool)
    for ring in rings:
        if not PR.ring_valid(ring):
            continue
        q = ring_points(ring)
        for a, b in zip(q, np.roll(q, -1, axis=0)):
            stroke_edge(m, a, b, T)
    return m


def confusion(p, g):
    tp, fp, fn = int((p & g).sum()), int((p & ~g).sum()), int((~p & g).sum())
    return tp, fp, fn, p.size - tp - fp - fn


def scores(conf, HW):
    """(iou, acc, f1) of (TP, FP, FN, TN)"""
    tp, fp, fn, tn = (int(v) for v in conf)
    if tp + fp + fn == 0:
        return 1.0, 1.0, 1.0
    return tp / ((tp + fp + fn) + 1e-9), (tp + tn) / HW, (2 * tp) / (2 * tp + fp + fn)


def run(gt_batch, dt_batch, H, W, T=5, modes=TOPDIG | SUBSET | STATS):
    """-> dict with the outputs of p3_mask_metrics as numpy arrays and "means": the nine figures by key"""
    B = len(gt_batch)
    assert len(dt_batch) == B and B >= 1
    conf = np.zeros((B, 2, 4), np.int32)
    image_scores = np.full((B, 6), NAN)
    image_nr = np.full(B, NAN)
    image_subset = np.zeros(B, np.int32)
    invalid = np.zeros((B, 2), np.int32)
    stats = [B, 0, 0, 0, 0, 0, 0]
    status = 0
    sums = [0.0] * 6
    s_iou = s_ciou = s_nr = 0.0
    in_subset = 0
    for b, (gts, dts) in enumerate(zip(gt_batch, dt_batch)):
        gv, dv = [PR.ring_valid(r) for r in gts], [PR.ring_valid(r) for r in dts]
        invalid[b] = (len(gv) - sum(gv), len(dv) - sum(dv))
        status |= int(not all(gv) or not all(dv))
        stats[1] += len(gts) > 0; stats[2] += len(dts) > 0
        stats[3] += len(gts); stats[4] += len(dts)
        stats[5] += sum(len(r) for r in gts); stats[6] += sum(len(r) for r in dts)
        if modes & (TOPDIG | SUBSET):
            conf[b, 0] = confusion(PR.set_mask(dts, H, W), PR.set_mask(gts, H, W))
        if modes & TOPDIG:
            conf[b, 1] = confusion(stroke_mask(dts, H, W, T), stroke_mask(gts, H, W, T))
            image_scores[b] = scores(conf[b, 0], H * W) + scores(conf[b, 1], H * W)
            for k in range(6):
                sums[k] += float(image_scores[b, k])
        if modes & SUBSET:
            ng, nd = sum(len(r) for r, v in zip(gts, gv) if v), sum(len(r) for r, v in zip(dts, dv) if v)
            nr = 1.0 - abs(nd - ng) / (nd + ng + 1e-9)
            image_nr[b] = nr
            image_subset[b] = len(dts) > 0
            if len(dts) > 0:
                iou = scores(conf[b, 0], H * W)[0]
                in_subset += 1
                s_iou += iou
                s_ciou += iou * nr
                s_nr += nr
    metrics = [s / B if modes & TOPDIG else NAN for s in sums] + [s / in_subset if in_subset else NAN for s in (s_iou, s_ciou, s_nr)]
    out = {"metrics": np.array(metrics, np.float64), "stats": np.array(stats if modes & STATS else [0] * 7, np.int64), "image_conf": conf,
           "image_scores": image_scores, "image_nr": image_nr, "image_subset": image_subset, "invalid_rings": invalid,
           "status": np.array([status], np.int32)}
    out["means"] = dict(zip(KEYS, out["metrics"].tolist()))
    return out
