"""Float64 restatement of the polygon metrics (include/p3hip.h p3_polygon_metrics) in plain numpy: what csrc/poly_metrics.hip is
held to.  Every step is written as the header states it, each product and sum rounded on its own, so that under the margins `margins()` reports - no pixel
centre near an edge, no edge length near a multiple of 0.1, no box IoU near 0.5 - masks, sample counts and matches are equal and the figures differ only by
the order of their sums.  Input: per image a list of float32 [n, 2] (x, y) arrays, open rings, for the ground truth and for the predictions."""
import numpy as np

STEP = 0.1
MAX_COORD = 32768.0
KEYS = ("IoU", "C-IoU", "NR", "POLIS", "chamfer", "hausdorff")


def ring_valid(ring):
    r = np.asarray(ring, dtype=np.float64).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        return len(r) >= 3 and bool(np.all(np.abs(r) <= MAX_COORD))


def ring_mask(ring, H, W):
    """even-odd parity of the pixel centres: bool [H, W]"""
    r = np.asarray(ring, dtype=np.float64)
    px = (np.arange(W, dtype=np.float64) + 0.5)[None, :]
    py = (np.arange(H, dtype=np.float64) + 0.5)[:, None]
    inside = np.zeros((H, W), dtype=bool)
    for a, b in zip(r, np.roll(r, -1, axis=0)):
        crossed = (a[1] <= py) != (b[1] <= py)
        t1 = (b[0] - a[0]) * (py - a[1])
        t2 = (px - a[0]) * (b[1] - a[1])
        cross = t1 - t2
        right = np.sign(cross) == np.sign(b[1] - a[1])
        inside ^= crossed & right
    return inside


def set_mask(rings, H, W):
    m = np.zeros((H, W), dtype=bool)
    for r in rings:
        if ring_valid(r):
            m |= ring_mask(r, H, W)
    return m


def box(ring):
    r = np.asarray(ring, dtype=np.float64)
    x0, y0, x1, y1 = r[:, 0].min(), r[:, 1].min(), r[:, 0].max(), r[:, 1].max()
    return np.array([x0, y0, x1 - x0, y1 - y0])


def box_iou(g, d):
    iw = min(g[0] + g[2], d[0] + d[2]) - max(g[0], d[0])
    ih = min(g[1] + g[3], d[1] + d[3]) - max(g[1], d[1])
    if iw <= 0 or ih <= 0:
        return 0.0
    i = iw * ih
    return float(i / (g[2] * g[3] + d[2] * d[3] - i))


def point_ring_distance(a, ring):
    """least distance of point a to the edges of the ring, the closing one included"""
    p, q = ring, np.roll(ring, -1, axis=0)
    v, w = q - p, a[None, :] - p
    den = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]
    num = w[:, 0] * v[:, 0] + w[:, 1] * v[:, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(den > 0, num / den, 0.0)
    t = np.clip(t, 0.0, 1.0)
    dx, dy = a[0] - (p[:, 0] + t * v[:, 0]), a[1] - (p[:, 1] + t * v[:, 1])
    return float(np.sqrt((dx * dx + dy * dy).min()))


def polis(A, B):
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    side = lambda P, Q: sum(point_ring_distance(a, Q) for a in P) / (2 * (len(P) + 1))
    return side(A, B) + side(B, A)


def samples(ring):
    """segmentize(0.1) restated: [S, 2], the first vertex once more at the end"""
    r = np.asarray(ring, dtype=np.float64)
    out = []
    for p, q in zip(r, np.roll(r, -1, axis=0)):
        dx, dy = q[0] - p[0], q[1] - p[1]
        L = np.sqrt(dx * dx + dy * dy)
        m = max(1, int(np.ceil(L / STEP)))
        if L == 0:
            out.append(p[None, :])
            continue
        t = (np.arange(m, dtype=np.float64) * (L / m)) / L
        out.append(np.stack([p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])], axis=1))
    out.append(r[:1])
    return np.concatenate(out)


def chamfer_hausdorff(A, B):
    sa, sb = samples(A), samples(B)
    d1 = np.empty(len(sa))
    d2 = np.full(len(sb), np.inf)
    for i0 in range(0, len(sa), 512):          # blocks keep the distance matrix small
        dx = sa[i0:i0 + 512, None, 0] - sb[None, :, 0]
        dy = sa[i0:i0 + 512, None, 1] - sb[None, :, 1]
        d = np.sqrt(dx * dx + dy * dy)
        d1[i0:i0 + 512] = d.min(axis=1)
        d2 = np.minimum(d2, d.min(axis=0))
    return float((d1.mean() + d2.mean()) / 2), float(max(d1.max(), d2.max()))


def run(gt_batch, dt_batch, H, W):
    """-> dict with the outputs of p3_polygon_metrics as numpy arrays (match indexes the predictions in packed order) and "means": the six figures by key"""
    B = len(gt_batch)
    assert len(dt_batch) == B and B >= 1
    nan = float("nan")
    out = {k: np.full(B, nan) for k in ("image_iou", "image_nr", "image_polis", "image_chamfer", "image_hausdorff")}
    out["image_valid"] = np.zeros(B, np.int32)
    out["image_counts"] = np.zeros((B, 2), np.int32)
    out["invalid_rings"] = np.zeros((B, 2), np.int32)
    match, pp, pc, ph = [], [], [], []
    dt_at, status = 0, 0
    for b, (gts, dts) in enumerate(zip(gt_batch, dt_batch)):
        gv, dv = [ring_valid(r) for r in gts], [ring_valid(r) for r in dts]
        out["invalid_rings"][b] = (len(gv) - sum(gv), len(dv) - sum(dv))
        status |= int(not all(gv) or not all(dv))
        mg, md = set_mask(gts, H, W), set_mask(dts, H, W)
        I, U = int((mg & md).sum()), int((mg | md).sum())
        out["image_counts"][b] = (I, U)
        out["image_iou"][b] = 1.0 if U == 0 else I / (U + 1e-9)
        ng, nd = sum(len(r) for r, v in zip(gts, gv) if v), sum(len(r) for r, v in zip(dts, dv) if v)
        out["image_nr"][b] = 1 - abs(nd - ng) / (nd + ng + 1e-9)
        dboxes = [box(r) if v else None for r, v in zip(dts, dv)]
        figures = []
        for g, v in zip(gts, gv):
            best, best_iou = -1, -1.0
            if v:
                gb = box(g)
                for j, db in enumerate(dboxes):
                    if db is None:
                        continue
                    u = box_iou(gb, db)
                    if u > best_iou:
                        best, best_iou = j, u
            if best >= 0 and best_iou > 0.5:
                c, h = chamfer_hausdorff(g, dts[best])
                figures.append((polis(g, dts[best]), c, h))
                match.append(dt_at + best)
                pp.append(figures[-1][0]); pc.append(c); ph.append(h)
            else:
                match.append(-1)
                pp.append(nan); pc.append(nan); ph.append(nan)
        if figures:          # the means over the counted pairs in gt order, summed in that order
            out["image_valid"][b] = 1
            for k, name in enumerate(("image_polis", "image_chamfer", "image_hausdorff")):
                s = 0.0
                for f in figures:
                    s += f[k]
                out[name][b] = s / len(figures)
        dt_at += len(dts)
    out["match"] = np.array(match, np.int32).reshape(-1)
    out["pair_polis"], out["pair_chamfer"], out["pair_hausdorff"] = (np.array(x, np.float64).reshape(-1) for x in (pp, pc, ph))
    out["status"] = np.array([status], np.int32)
    out["metrics"] = set_means(out)
    out["means"] = dict(zip(KEYS, out["metrics"].tolist()))
    return out


def set_means(out):
    """the six figures from the per-image ones, summed in image order"""
    B = len(out["image_iou"])
    s = [0.0] * 6
    valid = 0
    for b in range(B):
        s[0] += out["image_iou"][b]
        s[1] += out["image_iou"][b] * out["image_nr"][b]
        s[2] += out["image_nr"][b]
        if out["image_valid"][b]:
            valid += 1
            s[3] += out["image_polis"][b]; s[4] += out["image_chamfer"][b]; s[5] += out["image_hausdorff"][b]
    nan = float("nan")
    return np.array([s[0] / B, s[1] / B, s[2] / B] + [x / valid if valid else nan for x in s[3:]], np.float64)


def margins(gt_batch, dt_batch, H, W):
    """the three margins a comparison of exact outputs relies on: (a) pixel centres whose cross product lies within 1e-4 |edge| of zero on a crossed edge,
    (b) the least distance of any L / 0.1 from an integer over the edges that are not axis-aligned (inf without one), (c) the least |box IoU - 0.5| over
    the gt rings' argmax (inf without one)"""
    near, frac, thr = 0, np.inf, np.inf
    px = (np.arange(W, dtype=np.float64) + 0.5)[None, :]
    py = (np.arange(H, dtype=np.float64) + 0.5)[:, None]
    for gts, dts in zip(gt_batch, dt_batch):
        for ring in list(gts) + list(dts):
            if not ring_valid(ring):
                continue
            r = np.asarray(ring, dtype=np.float64)
            for a, b in zip(r, np.roll(r, -1, axis=0)):
                L = float(np.hypot(b[0] - a[0], b[1] - a[1]))
                crossed = (a[1] <= py) != (b[1] <= py)
                cross = (b[0] - a[0]) * (py - a[1]) - (px - a[0]) * (b[1] - a[1])
                near += int((crossed & (np.abs(cross) <= 1e-4 * L)).sum())
                if a[0] != b[0] and a[1] != b[1]:
                    q = L / STEP
                    frac = min(frac, abs(q - round(q)))
        dboxes = [box(r) for r in dts if ring_valid(r)]
        for g in gts:
            if ring_valid(g) and dboxes:
                thr = min(thr, abs(max(box_iou(box(g), d) for d in dboxes) - 0.5))
    return near, frac, thr
