"""Float64 restatement of the max tangent angle error (include/p3hip.h p3_max_tangent_angle) in plain numpy: what
csrc/mta_metrics.hip is held to.  Every step is written as the header states it, each product and sum rounded on its own, so that under the margins
`margins()` reports - no pixel centre near an edge, no L / spacing near a half-integer, no near tie between two nearest points, no stretch near a bound -
masks, sample counts, nearest edges and states are equal and the figures differ by a few roundings.  Input: per image a list of float32 [n, 2] (x, y)
arrays, open rings, for the ground truth and for the predictions."""
import math

import numpy as np

from tests import poly_metrics_ref as P

COUNTED, INVALID, EMPTY, BELOW_PRECISION, NO_EDGE = 0, 1, 2, 3, 4


def edge_count(L, spacing):
    """m = max(1, (int)rint(L / spacing)): Python's round is half to even"""
    return max(1, int(round(float(L) / spacing)))


def samples(ring, spacing):
    """the sample line [1 + sum m, 2]: vertex 0, then per edge the points j = 1 .. m-1 of p + j ((q - p) / m) and the end point q itself"""
    r = np.asarray(ring, dtype=np.float64)
    out = [r[:1]]
    for p, q in zip(r, np.roll(r, -1, axis=0)):
        dx, dy = q[0] - p[0], q[1] - p[1]
        m = edge_count(np.sqrt(dx * dx + dy * dy), spacing)
        step = (q - p) / m
        j = np.arange(1, m, dtype=np.float64)[:, None]
        out += [p[None, :] + j * step[None, :], q[None, :]]
    return np.concatenate(out)


def gt_edges(rings):
    """the edges of the valid rings, rings in set order, edges in ring order, closing edges included: (p [E, 2], q [E, 2])"""
    valid = [np.asarray(r, dtype=np.float64) for r in rings if P.ring_valid(r)]
    if not valid:
        return np.zeros((0, 2)), np.zeros((0, 2))
    return np.concatenate(valid), np.concatenate([np.roll(r, -1, axis=0) for r in valid])


def project(s, p, q):
    """per sample and edge the candidate point and its squared distance: (cx, cy, e), each [S, E]"""
    ex, ey = (q[:, 0] - p[:, 0])[None, :], (q[:, 1] - p[:, 1])[None, :]
    wx, wy = s[:, 0, None] - p[None, :, 0], s[:, 1, None] - p[None, :, 1]
    den = ex * ex + ey * ey
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (wx * ex + wy * ey) / den
        at_p = ~(den > 0) | (t <= 0)
        at_q = ~at_p & (t >= 1)
        cx = np.where(at_p, p[None, :, 0], np.where(at_q, q[None, :, 0], p[None, :, 0] + t * ex))
        cy = np.where(at_p, p[None, :, 1], np.where(at_q, q[None, :, 1], p[None, :, 1] + t * ey))
    dx, dy = s[:, 0, None] - cx, s[:, 1, None] - cy
    return cx, cy, dx * dx + dy * dy


def nearest(s, p, q):
    """[S, 2]: the candidate of the first edge with the strictly smallest squared distance (argmin takes the first of equals)"""
    cx, cy, e = project(s, p, q)
    k = np.argmin(e, axis=1)
    i = np.arange(len(s))
    return np.stack([cx[i, k], cy[i, k]], axis=1)


def line_edges(s, pr):
    """per pair of consecutive samples: (|u|, |v|, u.v)"""
    u, v = s[1:] - s[:-1], pr[1:] - pr[:-1]
    nu = np.sqrt(u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1])
    nv = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1])
    return nu, nv, u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]


def ring_cos(s, pr, max_stretch):
    """the least |cos| over the valid edges of the sample line, None without one"""
    nu, nv, dot = line_edges(s, pr)
    nn = nu * nv
    with np.errstate(invalid="ignore", divide="ignore"):
        stretch = nu / nv
        c = np.abs(dot / nn)
    ok = (nn > 0) & (1.0 / max_stretch < stretch) & (stretch < max_stretch)
    return float(c[ok].min()) if ok.any() else None


def run(gt_batch, dt_batch, H, W, spacing=2.0, min_precision=0.5, max_stretch=2.0):
    """-> dict with the outputs of p3_max_tangent_angle as numpy arrays (predictions in packed order), "MTA" as a float and "ring_samples": the sample
    count of every counted or edgeless ring, 0 for the others"""
    B = len(gt_batch)
    assert len(dt_batch) == B and B >= 1
    nan = float("nan")
    angle, cos, state, px, nsamp = [], [], [], [], []
    overlap, invalid = np.zeros(B, np.int32), np.zeros((B, 2), np.int32)
    status = 0
    for b, (gts, dts) in enumerate(zip(gt_batch, dt_batch)):
        gv, dv = [P.ring_valid(r) for r in gts], [P.ring_valid(r) for r in dts]
        invalid[b] = (len(gv) - sum(gv), len(dv) - sum(dv))
        status |= int(not all(gv) or not all(dv))
        mg = P.set_mask(gts, H, W)
        p, q = gt_edges(gts)
        union, sum_a = np.zeros((H, W), bool), 0
        for ring, v in zip(dts, dv):
            angle.append(nan); cos.append(nan); nsamp.append(0)
            if not v:
                state.append(INVALID); px.append((0, 0))
                continue
            m = P.ring_mask(ring, H, W)
            A, I = int(m.sum()), int((m & mg).sum())
            union |= m
            sum_a += A
            px.append((A, I))
            if A == 0:
                state.append(EMPTY)
            elif not I / A > min_precision:
                state.append(BELOW_PRECISION)
            else:
                s = samples(ring, spacing)
                nsamp[-1] = len(s)
                c = ring_cos(s, nearest(s, p, q), max_stretch)
                if c is None:
                    state.append(NO_EDGE)
                else:
                    state.append(COUNTED)
                    cos[-1], angle[-1] = c, math.acos(min(1.0, c))
        overlap[b] = sum_a - int(union.sum())
        status |= 4 * int(overlap[b] != 0)
    out = {"ring_angle": np.array(angle, np.float64).reshape(-1), "ring_cos": np.array(cos, np.float64).reshape(-1),
           "ring_state": np.array(state, np.int32).reshape(-1), "ring_px": np.array(px, np.int32).reshape(-1, 2), "image_overlap_px": overlap,
           "invalid_rings": invalid, "status": np.array([status], np.int32), "ring_samples": np.array(nsamp, np.int64).reshape(-1)}
    mean, n = set_mean(out["ring_angle"], out["ring_state"])
    out["mta"], out["counted"], out["MTA"] = np.array([mean], np.float64), np.array([n], np.int32), mean
    return out


def set_mean(ring_angle, ring_state):
    """(the mean of (angle 180) / pi over the counted rings, summed in ring order; their number)"""
    s, n = 0.0, 0
    for a, st in zip(ring_angle.tolist(), ring_state.tolist()):
        if st == COUNTED:
            s += a * 180.0 / math.pi
            n += 1
    return (s / n if n else float("nan")), n


def margins(gt_batch, dt_batch, H, W, spacing=2.0, min_precision=0.5, max_stretch=2.0):
    """what a comparison of exact outputs relies on, as a dict:
    "pixels"   pixel centres within 1e-4 |edge| of a crossed edge, over both sets (poly_metrics_ref.margins)
    "count"    the least distance of L / spacing from a half-integer over the oblique edges of the valid predictions (inf without one)
    "ties"     samples whose runner-up edge gives another point at a squared distance not more than 1e-9 (relative) above the winner's, unless the two
               squared distances are equal and the sample and every gt edge end of the image are multiples of 1 / 64 below 2^15 (dyadic operands of
               at most 21 bits: differences, products, the sums of two of them and so both squared distances of a point that is an edge end or has an
               exact t are computed without a rounding, and the order of the edges decides the tie on either side)
    "stretch"  edges of a sample line whose stretch lies within 1e-9 of a bound while a norm is not an exact integer"""
    out = {"pixels": P.margins(gt_batch, dt_batch, H, W)[0], "count": np.inf, "ties": 0, "stretch": 0}
    for gts, dts in zip(gt_batch, dt_batch):
        mg = P.set_mask(gts, H, W)
        p, q = gt_edges(gts)
        for ring in dts:
            if not P.ring_valid(ring):
                continue
            r = np.asarray(ring, dtype=np.float64)
            for a, b in zip(r, np.roll(r, -1, axis=0)):
                if a[0] != b[0] and a[1] != b[1]:
                    x = float(np.hypot(b[0] - a[0], b[1] - a[1])) / spacing
                    out["count"] = min(out["count"], abs(x - math.floor(x) - 0.5))
            m = P.ring_mask(ring, H, W)
            A, I = int(m.sum()), int((m & mg).sum())
            if A == 0:
                continue
            if not I / A > min_precision:
                continue
            s = samples(ring, spacing)
            cx, cy, e = project(s, p, q)
            k = np.argmin(e, axis=1)
            i = np.arange(len(s))
            other = (cx != cx[i, k][:, None]) | (cy != cy[i, k][:, None])
            dyadic = lambda a: bool(np.all((a * 64.0 == np.rint(a * 64.0)) & (np.abs(a) < 32768.0)))
            exact = (dyadic(s) & np.ones(len(s), bool)) if dyadic(p) and dyadic(q) else np.zeros(len(s), bool)
            exact = exact & dyadic(cx[i, k]) & dyadic(cy[i, k])
            close = (e - e[i, k][:, None] <= 1e-9 * e) & ~((e == e[i, k][:, None]) & exact[:, None] & (cx * 64.0 == np.rint(cx * 64.0)) & (cy * 64.0 == np.rint(cy * 64.0)))
            out["ties"] += int((other & close).any(axis=1).sum())
            nu, nv, _ = line_edges(s, np.stack([cx[i, k], cy[i, k]], axis=1))
            with np.errstate(invalid="ignore", divide="ignore"):
                stretch = nu / nv
            near = (nu * nv > 0) & ((np.abs(stretch - max_stretch) <= 1e-9) | (np.abs(stretch - 1.0 / max_stretch) <= 1e-9))
            whole = (nu == np.rint(nu)) & (nv == np.rint(nv))
            out["stretch"] += int((near & ~whole).sum())
    return out
