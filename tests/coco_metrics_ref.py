"""Float64 / integer restatement of the COCO metrics (include/p3hip.h p3_coco_metrics) in plain numpy: what csrc/coco_metrics.hip is
held to.  Masks are boolean arrays, the matching and the accumulation are the plain loops of steps 5 to 7, the means are summed in index order.  Input: per
image a list of float32 [n, 2] (x, y) open rings for the ground truth and for the predictions; optionally per image a list of scores (predictions) and of
areas (ground truth).  Ring validity and the pixel-centre mask are those of tests/poly_metrics_ref.py."""
import numpy as np

from tests.poly_metrics_ref import ring_mask, ring_valid

KEEP = 100
IOU_THRS = np.linspace(0.5, 0.95, 10)
REC_THRS = np.linspace(0, 1, 101)
AREA_RANGES = ((0.0, 1e10), (0.0, 1024.0), (1024.0, 9216.0), (9216.0, 1e10))
MAX_DETS = (1, 10, 100)
TYPES = ("segm", "boundary")
KEYS = ("AP", "AP50", "AP75", "AP_small", "AP_medium", "AP_large", "AR1", "AR10", "AR100", "AR_small", "AR_medium", "AR_large")
# summarize: (precision?, threshold index or None, area range, maxDets index) in pycocotools' order
STATS = ((1, None, 0, 2), (1, 0, 0, 2), (1, 5, 0, 2), (1, None, 1, 2), (1, None, 2, 2), (1, None, 3, 2),
         (0, None, 0, 0), (0, None, 0, 1), (0, None, 0, 2), (0, None, 1, 2), (0, None, 2, 2), (0, None, 3, 2))


def dilation(H, W):
    return max(1, int(round(0.02 * float(np.sqrt(float(H * H + W * W))))))          # Python's round is half-even


def boundary_mask(mask, d):
    """the mask minus its erosion by the (2d+1) x (2d+1) square; outside the image nothing is in the mask"""
    H, W = mask.shape
    padded = np.zeros((H + 2 * d, W + 2 * d), dtype=bool)
    padded[d:d + H, d:d + W] = mask
    eroded = np.ones((H, W), dtype=bool)
    for dy in range(2 * d + 1):
        for dx in range(2 * d + 1):
            eroded &= padded[dy:dy + H, dx:dx + W]
    return mask & ~eroded


def pair_iou(a, b):
    inter = int((a & b).sum())
    union = int(a.sum()) + int(b.sum()) - inter
    return inter, (0.0 if union == 0 else float(np.float64(inter) / np.float64(union)))


def mean_in_order(values):
    """the mean of the entries > -1, summed one after the other in index order; -1 without one"""
    s, n = 0.0, 0
    for v in values:
        if v > -1:
            s += float(v)
            n += 1
    return s / n if n else -1.0


def run(gt_batch, dt_batch, H, W, scores=None, areas=None, iou_types=TYPES):
    """-> dict with the outputs of p3_coco_metrics as numpy arrays, and "named": per type the twelve figures by key"""
    B = len(gt_batch)
    assert len(dt_batch) == B and B >= 1 and all(t in TYPES for t in iou_types) and len(iou_types) > 0
    on = [t in iou_types for t in TYPES]
    d = dilation(H, W)
    Rg, Rd = sum(len(g) for g in gt_batch), sum(len(x) for x in dt_batch)
    out = {"gt_area_px": np.zeros(Rg, np.int32), "dt_area_px": np.zeros(Rd, np.int32), "gt_boundary_px": np.zeros(Rg, np.int32),
           "dt_boundary_px": np.zeros(Rd, np.int32), "dt_rank": np.full(Rd, -1, np.int32), "pair_inter": np.zeros((2, KEEP * Rg), np.int32),
           "dt_match": np.full((2, 4, 10, Rd), -1, np.int32), "dt_ignore": np.zeros((2, 4, 10, Rd), np.uint8), "gt_match": np.full((2, 4, 10, Rg), -1, np.int32)}
    status = 0
    images = []          # per image: the kept predictions (ring index, score) in order
    gt_ignored = np.zeros((4, Rg), dtype=bool)
    gt_valid = np.zeros(Rg, dtype=bool)
    g_at = d_at = 0
    for b in range(B):
        gts, dts = gt_batch[b], dt_batch[b]
        sc = [np.float32(1.0)] * len(dts) if scores is None else [np.float32(s) for s in scores[b]]
        gmask, garea = {}, {}
        for i, ring in enumerate(gts):
            if not ring_valid(ring):
                status |= 1
                continue
            g = g_at + i
            gt_valid[g] = True
            gmask[g] = ring_mask(ring, H, W)
            out["gt_area_px"][g] = int(gmask[g].sum())
            garea[g] = float(out["gt_area_px"][g]) if areas is None else float(np.float32(areas[b][i]))
            for a, (lo, hi) in enumerate(AREA_RANGES):
                gt_ignored[a, g] = garea[g] < lo or garea[g] > hi
        valid = []
        for j, ring in enumerate(dts):
            if not ring_valid(ring) or np.isnan(sc[j]):
                status |= 1
                continue
            valid.append(j)
        order = sorted(valid, key=lambda j: -float(sc[j]))          # sorted is stable
        kept = [d_at + j for j in order[:KEEP]]
        dmask = {}
        for j in valid:
            dmask[d_at + j] = ring_mask(dts[j], H, W)
            out["dt_area_px"][d_at + j] = int(dmask[d_at + j].sum())
        for k, x in enumerate(kept):
            out["dt_rank"][x] = k
        gb, db = {}, {}
        if on[1]:
            gb = {g: boundary_mask(m, d) for g, m in gmask.items()}
            db = {x: boundary_mask(m, d) for x, m in dmask.items()}
            for g, m in gb.items():
                out["gt_boundary_px"][g] = int(m.sum())
            for x, m in db.items():
                out["dt_boundary_px"][x] = int(m.sum())
        glist = sorted(gmask)
        iou = np.zeros((2, len(glist), len(kept)))
        for gi, g in enumerate(glist):
            for k, x in enumerate(kept):
                inter, v = pair_iou(gmask[g], dmask[x])
                out["pair_inter"][0, KEEP * g + k] = inter
                iou[0, gi, k] = v
                if on[1]:
                    inter_b, vb = pair_iou(gb[g], db[x])
                    out["pair_inter"][1, KEEP * g + k] = inter_b
                    iou[1, gi, k] = min(v, vb)
        for ty in range(2):
            if not on[ty]:
                continue
            for a, (lo, hi) in enumerate(AREA_RANGES):
                walk = sorted(range(len(glist)), key=lambda gi: bool(gt_ignored[a, glist[gi]]))          # not-ignored first, stable
                for t, thr in enumerate(IOU_THRS):
                    gtm = out["gt_match"][ty, a, t]
                    for k, x in enumerate(kept):
                        best, m = min(float(thr), 1 - 1e-10), -1
                        for gi in walk:
                            g = glist[gi]
                            if gtm[g] >= 0:
                                continue
                            if m >= 0 and not gt_ignored[a, m] and gt_ignored[a, g]:
                                break
                            if iou[ty, gi, k] < best:
                                continue
                            best, m = iou[ty, gi, k], g
                        if m >= 0:
                            out["dt_match"][ty, a, t, x] = m
                            gtm[m] = x
                            out["dt_ignore"][ty, a, t, x] = gt_ignored[a, m]
                        else:
                            area = float(out["dt_area_px"][x])
                            out["dt_ignore"][ty, a, t, x] = area < lo or area > hi
        images.append([(x, float(sc[x - d_at])) for x in kept])
        g_at += len(gts)
        d_at += len(dts)
    # accumulate
    precision = np.full((2, 10, 101, 4, 3), np.nan)
    recall = np.full((2, 10, 4, 3), np.nan)
    for ty in range(2):
        if not on[ty]:
            continue
        precision[ty], recall[ty] = -1.0, -1.0
        for a in range(4):
            npig = int((gt_valid & ~gt_ignored[a]).sum())
            if npig == 0:
                continue
            for mi, m in enumerate(MAX_DETS):
                dets = [p for kept in images for p in kept[:m]]
                dets = sorted(dets, key=lambda p: -p[1])          # stable
                nd = len(dets)
                for t in range(10):
                    tp = fp = 0
                    rc, pr = np.zeros(nd), np.zeros(nd)
                    for i, (x, _) in enumerate(dets):
                        if not out["dt_ignore"][ty, a, t, x]:
                            if out["dt_match"][ty, a, t, x] >= 0:
                                tp += 1
                            else:
                                fp += 1
                        rc[i] = np.float64(tp) / np.float64(npig)
                        pr[i] = np.float64(tp) / (np.float64(fp) + np.float64(tp) + np.float64(2.0 ** -52))
                    recall[ty, t, a, mi] = rc[-1] if nd else 0.0
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    at = 0          # the first i with rc[i] >= recThrs[r]: both ascend, so the search goes on where the last one ended
                    for r, want in enumerate(REC_THRS):
                        while at < nd and rc[at] < want:
                            at += 1
                        precision[ty, t, r, a, mi] = pr[at] if at < nd else 0.0
    stats = np.full((2, 12), np.nan)
    for ty in range(2):
        if not on[ty]:
            continue
        for k, (ap, tsel, a, mi) in enumerate(STATS):
            ts = range(10) if tsel is None else [tsel]
            if ap:
                stats[ty, k] = mean_in_order(precision[ty, t, r, a, mi] for t in ts for r in range(101))
            else:
                stats[ty, k] = mean_in_order(recall[ty, t, a, mi] for t in ts)
    out.update(precision=precision, recall=recall, stats=stats, status=np.array([status], np.int32))
    out["named"] = {TYPES[ty]: dict(zip(KEYS, stats[ty].tolist())) for ty in range(2)}
    return out


def margins(gt_batch, dt_batch, H, W):
    """pixel centres whose cross product lies within 1e-4 |edge| of zero on a crossed edge, over the valid rings of both sets: with none, the device and this
    file rasterise the same masks and every count is equal"""
    near = 0
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
    return near
