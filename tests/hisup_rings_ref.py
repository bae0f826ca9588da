"""Sequential numpy / scipy restatement of the inner rings of the HiSup polygon step (models/hisup/polygon.py:95-109,138-169 of the reference:
`inn_c_to_poly_coco` and the hole branch of `get_poly_crowdai`), on top of tests/hisup_polygon_ref.py, and the inputs the ring tests share.

Steps G to I of include/p3hip.h.  As for the outer polygons the OpenCV calls are restated, not pinned: `hole_border` is Suzuki and Abe's hole border for
8-connected foreground (the follower of step C, started at the region pixel left of the hole's first cell with s = 0), `fill` stands for
drawContours(thickness=-1) and `area2` is twice the shoelace area.  Everything else - the area threshold, the row / column cut, the reversal, squaring,
junction match, simplification and the concatenation of a region's parts - is pinned to the reference's own code by tests/golden/hisup_rings.npz
(make_hisup_rings_golden.py).  One deviation is left: holes are numbered in raster order of their first cell, OpenCV orders sibling contours its own way.

Coordinates are (x, y) = (column, row)."""
import os

import numpy as np
from scipy import ndimage

from tests import hisup_polygon_ref as R

AREA2_MIN = 100          # a hole gives a ring iff its contour area is >= 50
EIGHT = np.ones((3, 3), bool)


def follow(T, p0, s0):
    """the border follower of step C on the bool image T from the set pixel p0 = (x, y) with start direction s0 -> list of (x, y)"""
    T = np.asarray(T, bool)
    H, W = T.shape

    def on(x, y):
        return 0 <= x < W and 0 <= y < H and bool(T[y, x])

    s, p1 = s0, None
    for _ in range(8):
        s = (s - 1) % 8
        if on(p0[0] + R.DXY[s][0], p0[1] + R.DXY[s][1]):
            p1 = (p0[0] + R.DXY[s][0], p0[1] + R.DXY[s][1])
            break
    if p1 is None:
        return [p0]
    out, p = [], p0
    while True:
        while True:
            s = (s + 1) % 8
            q = (p[0] + R.DXY[s][0], p[1] + R.DXY[s][1])
            if on(*q):
                break
        out.append(p)
        if q == p0 and p == p1:
            return out
        p, s = q, (s + 4) % 8


def holes_of(M):
    """step G -> (int label image of the holes of M, their number): 4-connected components of the background that the flood of step A does not reach,
    numbered in raster order of their first cell"""
    M = np.asarray(M, bool)
    return ndimage.label(R.fill(M) & ~M)


def hole_border(M, hole):
    """step H -> the hole border of the bool mask `hole` in M as a list of (x, y)"""
    ys, xs = np.nonzero(hole)
    xh, yh = int(xs[0]), int(ys[0])
    assert M[yh, xh - 1]
    return follow(M, (xh - 1, yh), 0)


def area2(pts):
    p = np.asarray(pts, dtype=np.int64).reshape(-1, 2)
    return abs(int(np.sum(p[:, 0] * np.roll(p[:, 1], -1) - np.roll(p[:, 0], -1) * p[:, 1])))


def hole_ring(shape, contour):
    """step I -> the ring int64 [m, 2] of a kept hole from its border; asserts that K' is one 8-connected component"""
    m = np.zeros(shape, bool)
    c = np.asarray(contour).reshape(-1, 2)
    m[c[:, 1], c[:, 0]] = True
    K = R.fill(m)
    ys, xs = np.nonzero(K)
    K[ys.min(), :] = False
    K[:, xs.min()] = False
    assert ndimage.label(K, structure=EIGHT)[1] == 1, "K' is not one component"
    return R.square(R.outer_border(K)[::-1])


def region_rings(M, juncs, x0=0, y0=0):
    """one region -> (n_holes, list of dict(pos fp32 [nv, 2], src int32 [nv], flags, area2, ring, margin_t, margin_d) per kept hole)"""
    M = np.asarray(M, bool)
    lab, n = holes_of(M)
    out = []
    for h in range(1, n + 1):
        contour = hole_border(M, lab == h)
        a2 = area2(contour)
        if a2 < AREA2_MIN:
            continue
        ring = hole_ring(M.shape, contour) + np.asarray([x0, y0])
        order, margin_d = R.match(ring, juncs)
        flags = 0
        if order is not None:
            flags = 1
            seq32, src = np.asarray(juncs, dtype=np.float32)[order], order.astype(np.int32)
        else:
            seq32, src = ring.astype(np.float32), np.arange(len(ring), dtype=np.int32)
        keep, margin_t = R.simplify(seq32.astype(np.float64))
        if len(keep) == 0:
            out.append(dict(pos=np.zeros((0, 2), np.float32), src=np.zeros(0, np.int32), flags=flags | 4, area2=a2, ring=ring, margin_t=margin_t,
                            margin_d=margin_d))
            continue
        keep = np.concatenate([keep, keep[:1]])
        out.append(dict(pos=seq32[keep], src=src[keep], flags=flags, area2=a2, ring=ring, margin_t=margin_t, margin_d=margin_d))
    return n, out


def rings(labels, n_regions, juncs, junc_counts, max_regions):
    """the whole batch in the kernel's layout, rings in (image, label, hole) order -> dict(ring_pos fp32 [V, 2], ring_src int32 [V], ring_slice int64 [Q, 2],
    ring_region int32 [Q], ring_flags int32 [Q], ring_area2 int32 [Q], region_rings int32 [B, R, 2], n_holes int32 [B, R],
    ring_counts (rings, ring vertices, longest ring), margin_t, margin_d)"""
    labels = np.asarray(labels)
    B, Rr = labels.shape[0], int(max_regions)
    pos, src, sl, reg, flags, areas = [], [], [], [], [], []
    rr, nh = np.zeros((B, Rr, 2), np.int32), np.zeros((B, Rr), np.int32)
    at, longest, margin_t, margin_d = 0, 0, np.inf, np.inf
    for b in range(B):
        n = min(R.MAXJ, int(max(junc_counts[b][0], 0)) + int(max(junc_counts[b][1], 0)))
        jb = np.asarray(juncs[b], dtype=np.float32)[:n]
        boxes = ndimage.find_objects(labels[b], max_label=Rr)
        for l in range(1, Rr + 1):
            first = len(sl)
            s = boxes[l - 1] if l <= min(int(n_regions[b]), Rr) else None
            if s is not None:
                nh[b, l - 1], found = region_rings(labels[b][s] == l, jb, s[1].start, s[0].start)
                for p in found:
                    nv = len(p["src"])
                    pos.append(p["pos"]); src.append(p["src"])
                    sl.append((at, at + nv)); reg.append(b * Rr + l - 1); flags.append(p["flags"]); areas.append(p["area2"])
                    at += nv
                    longest = max(longest, nv)
                    margin_t, margin_d = min(margin_t, p["margin_t"]), min(margin_d, p["margin_d"])
            rr[b, l - 1] = (first, len(sl))
    return dict(ring_pos=np.concatenate(pos).reshape(-1, 2).astype(np.float32) if pos else np.zeros((0, 2), np.float32),
                ring_src=np.concatenate(src).astype(np.int32) if src else np.zeros(0, np.int32), ring_slice=np.asarray(sl, np.int64).reshape(-1, 2),
                ring_region=np.asarray(reg, np.int32), ring_flags=np.asarray(flags, np.int32), ring_area2=np.asarray(areas, np.int32), region_rings=rr,
                n_holes=nh, ring_counts=(len(sl), at, longest), margin_t=margin_t, margin_d=margin_d)


def concatenated(outer, inner, b, i):
    """what `get_poly_crowdai` returns for region i (label i + 1) of image b from R.polygons' and rings' outputs -> (float64 [k, 2], part lengths), or None
    for a region without outer polygon; a ring in which nothing is kept is left out"""
    s = outer["poly_slice"][b, i]
    if outer["poly_flags"][b, i] & 4:
        return None
    parts = [outer["pos"][s[0]:s[1]]]
    for q in range(*inner["region_rings"][b, i]):
        if not inner["ring_flags"][q] & 4:
            parts.append(inner["ring_pos"][inner["ring_slice"][q, 0]:inner["ring_slice"][q, 1]])
    return np.concatenate(parts).astype(np.float64), [len(p) for p in parts]


# ------------------------------------------------------------------------------------------------ inputs
def courtyard_regions(rs, size=48):
    """a seeded foreground mask: blocks with rectangular and L-shaped cut-outs, 2 % pixel noise"""
    fg = np.zeros((size, size), bool)
    half = size // 2
    for k in range(2):
        y0 = k * half + int(rs.randint(0, 2))
        h = half - 2 - int(rs.randint(0, 2))
        x0 = int(rs.randint(0, 4))
        w = size - x0 - int(rs.randint(0, 4))
        if rs.rand() < 0.35:                                       # two blocks side by side
            cut = x0 + w // 2 + int(rs.randint(-3, 4))
            spans = [(x0, cut - 1), (cut + 1, x0 + w)]
        else:
            spans = [(x0, x0 + w)]
        for xa, xb in spans:
            fg[y0:y0 + h, xa:xb] = True
            x = xa + 2 + int(rs.randint(0, 3))
            while True:
                ch, cw = int(rs.randint(3, 12)), int(rs.randint(3, 12))
                if x + cw + 2 > xb:
                    break
                y = y0 + 2 + int(rs.randint(0, max(1, h - ch - 3)))
                ch = min(ch, y0 + h - 2 - y)
                fg[y:y + ch, x:x + cw] = False
                if rs.rand() < 0.5 and ch > 4 and cw > 4:          # L-shaped: put one corner back
                    ay, ax = int(rs.randint(2, ch - 1)), int(rs.randint(2, cw - 1))
                    fg[y:y + ay, x + ax:x + cw] = True
                x += cw + 1 + int(rs.randint(0, 4))
    return fg ^ (rs.rand(size, size) < 0.02)


def ring_junctions(rs, fg, share=0.5, jitter=0.8):
    """junctions near the turning points of some inner rings and of some outer rings, plus a few stray ones"""
    lab, n = ndimage.label(fg, structure=EIGHT)
    out = []
    for l in range(1, n + 1):
        M = lab == l
        seqs = [q["ring"] for q in region_rings(M, np.zeros((0, 2), np.float32))[1]]
        if rs.rand() < 0.3:
            seqs.append(R.ring_of(M)[0])
        for ring in seqs:
            if rs.rand() > share or len(ring) == 0:
                continue
            keep, _ = R.simplify(ring)
            for v in keep[::max(1, len(keep) // 8)]:
                out.append(ring[v] + rs.uniform(-jitter, jitter, 2))
    for _ in range(int(rs.randint(0, 6))):
        out.append(rs.uniform(0, fg.shape[0], 2))
    out = np.asarray(out, dtype=np.float32).reshape(-1, 2)
    return out[rs.permutation(len(out))]


def block_with_holes(n, block, holes):
    """(y, x, h, w) of the block and of each rectangular hole -> bool [n, n]"""
    m = R.rect(n, *block)
    for (y, x, h, w) in holes:
        m[y:y + h, x:x + w] = False
    return m


def hand_first():
    """the first hand value of include/p3hip.h: a 15 x 14 block at rows 2..15, cols 3..17 with a 6 x 7 hole at rows 4..9, cols 5..11"""
    return block_with_holes(24, (2, 3, 14, 15), [(4, 5, 6, 7)])


def hand_wall():
    """the second: two 8-row holes at cols 4..11 and 13..21 that share the one-pixel wall at col 12"""
    return block_with_holes(24, (2, 2, 12, 22), [(4, 4, 8, 8), (4, 13, 8, 9)])


def hand_set():
    """two 48 x 48 images:
    0: 6 x 7, 6 x 6 and 3 x 3 holes in three blocks; the two-hole wall case; a block at rows and cols 0..11 with its hole at 1..8
    1: a hole with a one-pixel spur reaching into it; a hole that holds an island of another region; a staircase-sided hole (all four diagonal steps)"""
    n = 48
    a = np.zeros((n, n), bool)
    a |= block_with_holes(n, (0, 0, 12, 12), [(1, 1, 8, 8)])                         # one pixel from the image corner
    a |= block_with_holes(n, (0, 14, 10, 11), [(2, 16, 6, 7)])                       # 6 x 7: kept
    a |= block_with_holes(n, (0, 27, 10, 10), [(2, 29, 6, 6)])                       # 6 x 6: dropped
    a |= block_with_holes(n, (0, 39, 7, 7), [(2, 41, 3, 3)])                         # 3 x 3: dropped
    a |= block_with_holes(n, (14, 2, 12, 22), [(16, 4, 8, 8), (16, 13, 8, 9)])       # the wall
    b = np.zeros((n, n), bool)
    b |= block_with_holes(n, (1, 1, 14, 16), [(3, 3, 10, 12)])
    b[8, 3:9] = True                                                                 # the spur
    b |= block_with_holes(n, (1, 20, 16, 18), [(3, 22, 12, 14)])
    b[7:10, 27:31] = True                                                            # the island: another region
    b[20:44, 4:40] = True                                                            # the staircase-sided hole: a diamond
    yy, xx = np.mgrid[:n, :n]
    b[(np.abs(yy - 32) + np.abs(xx - 22) <= 8)] = False
    return np.stack([a, b])


def disc_cases():
    """three 48 x 48 images, each a 40 x 40 block with a disc hole of radius 12: 60 junctions on its rim (every turn is 6 degrees: nothing is kept, ring flag
    bits 0 and 2), 24 junctions (15 degrees: a junction ring), exactly two junctions near it (the ring stays)"""
    n = 48
    yy, xx = np.mgrid[:n, :n]
    m = R.rect(n, 4, 4, 40, 40) & ~((yy + 0.5 - 24) ** 2 + (xx + 0.5 - 24) ** 2 <= 12 ** 2)
    rim = lambda k: np.stack([24 + 12 * np.cos(2 * np.pi * (np.arange(k) + 0.5) / k), 24 + 12 * np.sin(2 * np.pi * (np.arange(k) + 0.5) / k)], 1)
    return np.stack([m, m, m]), [rim(60), rim(24), rim(24)[[0, 12]]]


def comb_hole(n, y, x, h, w):
    """a block of h x w whose hole is a comb: one-pixel slots four pixels apart, joined along the bottom.  The teeth between the slots are three pixels
    wide, so their middle column is not enclosed by the hole border and K' is a comb too: its ring is far longer than its box is wide"""
    m = R.rect(n, y, x, h, w)
    m[y + 2:y + h - 2, x + 2:x + w - 2:4] = False
    m[y + h - 3, x + 2:x + w - 3] = False
    return m


def big_ring_set():
    """three 224 x 224 images: big_set's first image with a 20 x 20 and a 5 x 5 hole in its 150 x 110 block (box past the LDS form); the full image; a 40 x 40
    block with a 30 x 30 hole and a 120 x 120 block whose box fits the LDS form but whose comb hole's ring does not"""
    fg, juncs = R.big_set()
    a = fg[0].copy()
    a[150:170, 20:40] = False
    a[190:195, 70:75] = False
    c = np.zeros_like(a)
    c |= block_with_holes(224, (5, 5, 40, 40), [(10, 10, 30, 30)])
    c |= comb_hole(224, 60, 60, 120, 120)
    jc = np.asarray([(10.3, 9.8), (40.2, 10.1), (39.9, 40.3), (9.7, 39.8), (150.2, 30.1)])
    ja = np.concatenate([juncs[0], np.asarray([(20.2, 149.8), (40.1, 150.3), (39.8, 170.2), (19.7, 169.9)])])
    return np.stack([a, fg[1], c]), [ja, juncs[1], jc]


def load_fixture():
    """tests/golden/hisup_rings.npz -> (foreground bool [6, 48, 48], junctions per image, {(image, label): (the reference's polygon float64 [k, 2],
    the lengths of its parts)})"""
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hisup_rings.npz"), allow_pickle=False)
    shape = tuple(int(x) for x in d["shape"])
    fg = np.unpackbits(d["fg"])[:int(np.prod(shape))].reshape(shape).astype(bool)
    ends = np.cumsum(d["junc_n"])
    juncs = [d["juncs"][e - n:e] for e, n in zip(ends, d["junc_n"])]
    pends, qends = np.cumsum(d["rows"][:, 2]), np.cumsum(d["rows"][:, 3])
    polys = {(int(b), int(l)): (d["polys"][e - n:e], [int(v) for v in d["parts"][f - k:f]]) for (b, l, n, k), e, f in zip(d["rows"], pends, qends)}
    return fg, juncs, polys
