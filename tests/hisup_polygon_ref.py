"""Sequential numpy / scipy restatement of the HiSup polygon step (models/hisup/polygon.py:56-93,111-169 of the reference: `ext_c_to_poly_coco`,
`diagonal_to_square`, `simple_polygon`, `get_poly_crowdai` with test_inria = False), outer polygons only, and the inputs the polygon tests share.

OpenCV is not a dependency of this repository and is not installed where the fixtures are made, so the three OpenCV calls of those functions are restated,
not pinned: `outer_border` (8-connected border following of the outer border, the published algorithm of Suzuki and Abe), `fill` (scipy's
binary_fill_holes, 4-connected background) and `shoelace`.  Everything else - squaring, junction match, simplification, control flow - is pinned to the
reference's own code by tests/golden/hisup_polygon.npz (make_hisup_polygon_golden.py runs the reference over these three).

Coordinates are (x, y) = (column, row).  The kernel (csrc/hisup_polygon.hip) is structured differently: bitmaps per bounding box, a flood by sweeps, votes by
an integer atomic minimum, flags and a scan instead of boolean indexing."""
import os

import numpy as np
from scipy import ndimage
from scipy.spatial.distance import cdist

MAXJ = 600
# direction s: 0 E, 1 NE, 2 N, 3 NW, 4 W, 5 SW, 6 S, 7 SE; y grows downwards
DXY = ((1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1))


def fill(M):
    """step A: M plus the background that no 4-connected background path joins to the outside"""
    return ndimage.binary_fill_holes(np.asarray(M, bool))


def corner_grid(F):
    """step B: T [(H+1), (W+1)], T[y, x] = F[y, x] | F[y-1, x] | F[y, x-1] | F[y-1, x-1]"""
    H, W = F.shape
    T = np.zeros((H + 1, W + 1), bool)
    T[:H, :W] |= F
    T[1:, :W] |= F
    T[:H, 1:] |= F
    T[1:, 1:] |= F
    return T


def outer_border(T):
    """step C: the outer border of the component of T that holds its first set pixel in raster order -> list of (x, y); a pixel may come more than once.
    A single pixel gives itself."""
    T = np.asarray(T, bool)
    H, W = T.shape

    def on(x, y):
        return 0 <= x < W and 0 <= y < H and bool(T[y, x])

    ys, xs = np.nonzero(T)
    if len(ys) == 0:
        return []
    p0 = (int(xs[0]), int(ys[0]))
    s, p1 = 4, None
    for _ in range(8):
        s = (s - 1) % 8
        if on(p0[0] + DXY[s][0], p0[1] + DXY[s][1]):
            p1 = (p0[0] + DXY[s][0], p0[1] + DXY[s][1])
            break
    if p1 is None:
        return [p0]
    out, p = [], p0
    while True:
        while True:
            s = (s + 1) % 8
            q = (p[0] + DXY[s][0], p[1] + DXY[s][1])
            if on(*q):
                break
        out.append(p)
        if q == p0 and p == p1:
            return out
        p, s = q, (s + 4) % 8


def square(pts):
    """step D: one point after every diagonal step of the cyclic sequence -> int64 [m, 2]"""
    out = []
    n = len(pts)
    for i, p in enumerate(pts):
        q = pts[(i + 1) % n]
        out.append(p)
        d = (q[0] - p[0], q[1] - p[1])
        if d == (1, 1):
            out.append((p[0] + 1, p[1]))
        elif d == (-1, -1):
            out.append((p[0] - 1, p[1]))
        elif d == (1, -1):
            out.append((p[0], p[1] - 1))
        elif d == (-1, 1):
            out.append((p[0], p[1] + 1))
    return np.asarray(out, dtype=np.int64).reshape(-1, 2)


def shoelace(pts):
    p = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    return 0.5 * abs(float(np.sum(p[:, 0] * np.roll(p[:, 1], -1) - np.roll(p[:, 0], -1) * p[:, 1])))


def ring_of(M):
    """steps A to D -> (ring int64 [m, 2], hole_pixels)"""
    M = np.asarray(M, bool)
    F = fill(M)
    return square(outer_border(corner_grid(F))), int(F.sum() - M.sum())


def match(ring, juncs):
    """step E -> (junction indices in ascending `first`, or None when the polygon is the ring; min |d - 5| over the ring points)"""
    if len(juncs) == 0:
        return None, np.inf
    d = cdist(ring.astype(np.float64), np.asarray(juncs).astype(np.float64))
    j = np.argmin(d, axis=1)
    dj = d[np.arange(len(j)), j]
    u, first = np.unique(j[dj < 5], return_index=True)
    margin = float(np.abs(dj - 5).min())
    return (u[np.argsort(first)] if len(u) > 2 else None), margin


def simplify(q):
    """step F on the open sequence q float64 [k, 2] -> (kept vertex indices ascending, min distance of a t_i to 10 and to 350)"""
    q = np.asarray(q, dtype=np.float64)
    e = np.roll(q, -1, axis=0) - q
    a = np.arctan2(e[:, 1], e[:, 0]) * 180 / np.pi
    t = np.abs(a - np.roll(a, -1))
    keep = np.roll((t > 10) & (t < 350), 1)              # t_i decides vertex (i + 1) mod k
    return np.nonzero(keep)[0], float(np.minimum(np.abs(t - 10), np.abs(t - 350)).min())


def region_polygon(M, juncs, x0=0, y0=0):
    """one region, M the whole image or its bounding box with the box's corner at (x0, y0) -> dict(pos fp32 [nv, 2], src int32 [nv], flags, hole_pixels,
    ring, margin_t, margin_d); nv = 0 with flag bit 2.  A label without pixels (inconsistent inputs) gives no polygon."""
    ring, holes = ring_of(M)
    if len(ring) == 0:
        return dict(pos=np.zeros((0, 2), np.float32), src=np.zeros(0, np.int32), flags=4, hole_pixels=0, ring=ring, margin_t=np.inf, margin_d=np.inf)
    ring = ring + np.asarray([x0, y0])
    order, margin_d = match(ring, juncs)
    flags = 2 if holes > 0 else 0
    if order is not None:
        flags |= 1
        seq32, src = np.asarray(juncs, dtype=np.float32)[order], order.astype(np.int32)
    else:
        seq32, src = ring.astype(np.float32), np.arange(len(ring), dtype=np.int32)
    keep, margin_t = simplify(seq32.astype(np.float64))
    if len(keep) == 0:
        return dict(pos=np.zeros((0, 2), np.float32), src=np.zeros(0, np.int32), flags=flags | 4, hole_pixels=holes, ring=ring, margin_t=margin_t,
                    margin_d=margin_d)
    keep = np.concatenate([keep, keep[:1]])
    return dict(pos=seq32[keep], src=src[keep], flags=flags, hole_pixels=holes, ring=ring, margin_t=margin_t, margin_d=margin_d)


def polygons(labels, n_regions, juncs, junc_counts, max_regions):
    """the whole batch with the kernel's output layout: labels int32 [B, H, W], n_regions [B], juncs fp32 [B, 600, 2], junc_counts [B, 2] ->
    dict(pos, src, poly_slice [B, R, 2], poly_flags [B, R], hole_pixels [B, R], n_vertices [B], counts (vertices, longest), margin_t, margin_d)"""
    labels = np.asarray(labels)
    B = labels.shape[0]
    R = int(max_regions)
    pos, src = [], []
    sl = np.zeros((B, R, 2), np.int64)
    flags, holes, nvert = np.zeros((B, R), np.int32), np.zeros((B, R), np.int32), np.zeros(B, np.int32)
    at, longest, margin_t, margin_d = 0, 0, np.inf, np.inf
    for b in range(B):
        n = min(MAXJ, int(max(junc_counts[b][0], 0)) + int(max(junc_counts[b][1], 0)))
        jb = np.asarray(juncs[b], dtype=np.float32)[:n]
        boxes = ndimage.find_objects(labels[b], max_label=R)
        for l in range(1, R + 1):
            if l <= min(int(n_regions[b]), R):
                s = boxes[l - 1]
                p = region_polygon(labels[b][s] == l, jb, s[1].start, s[0].start) if s is not None else region_polygon(np.zeros((1, 1), bool), jb)
                pos.append(p["pos"]); src.append(p["src"])
                flags[b, l - 1], holes[b, l - 1] = p["flags"], p["hole_pixels"]
                nv = len(p["src"])
                margin_t, margin_d = min(margin_t, p["margin_t"]), min(margin_d, p["margin_d"])
            else:
                nv = 0
            sl[b, l - 1] = (at, at + nv)
            at += nv
            nvert[b] += nv
            longest = max(longest, nv)
    return dict(pos=np.concatenate(pos).reshape(-1, 2).astype(np.float32) if pos else np.zeros((0, 2), np.float32),
                src=np.concatenate(src).astype(np.int32) if src else np.zeros(0, np.int32), poly_slice=sl, poly_flags=flags, hole_pixels=holes,
                n_vertices=nvert, counts=(at, longest), margin_t=margin_t, margin_d=margin_d)


def region_inputs(fg):
    """foreground masks bool [B, H, W] -> (labels int32 [B, H, W], n_regions int32 [B], bbox int32 [B, R, 4], R) as p3_hisup_regions writes them:
    8-connected components numbered in raster order of their first pixel, bbox = (min_row, min_col, max_row + 1, max_col + 1)"""
    fg = np.asarray(fg, bool)
    B = fg.shape[0]
    labs, ns = [], []
    for b in range(B):
        lab, n = ndimage.label(fg[b], structure=np.ones((3, 3)))
        labs.append(lab.astype(np.int32)); ns.append(n)
    R = max(max(ns), 1)
    bbox = np.zeros((B, R, 4), np.int32)
    for b in range(B):
        for i, s in enumerate(ndimage.find_objects(labs[b])):
            bbox[b, i] = (s[0].start, s[1].start, s[0].stop, s[1].stop)
    return np.stack(labs), np.asarray(ns, np.int32), bbox, R


def junction_inputs(per_image):
    """list of [n, 2] (x, y) arrays -> (juncs fp32 [B, 600, 2], counts int32 [B, 2]); the first half of an image's junctions counts as class 2"""
    B = len(per_image)
    juncs, counts = np.zeros((B, MAXJ, 2), np.float32), np.zeros((B, 2), np.int32)
    for b, j in enumerate(per_image):
        j = np.asarray(j, dtype=np.float32).reshape(-1, 2)
        assert len(j) <= MAXJ
        juncs[b, :len(j)] = j
        counts[b] = (len(j) // 2, len(j) - len(j) // 2)
    return juncs, counts


def random_regions(rs, size=48):
    """a seeded foreground mask: unions of 1 to 4 rectangles per blob, a cut-out, 2 % pixel noise"""
    fg = np.zeros((size, size), bool)
    for _ in range(int(rs.randint(2, 5))):
        cy, cx = rs.randint(4, size - 4, 2)
        for _ in range(int(rs.randint(1, 5))):
            h, w = rs.randint(2, 12, 2)
            y, x = cy + rs.randint(-5, 6), cx + rs.randint(-5, 6)
            fg[max(y, 0):y + h, max(x, 0):x + w] = True
        if rs.rand() < 0.5:
            fg[cy:cy + 2, cx:cx + 3] = False
    return fg ^ (rs.rand(size, size) < 0.02)


def corner_junctions(rs, fg, share=0.6, jitter=0.8):
    """junctions near the turning points of some regions' rings (so that about half of the regions become junction polygons) plus a few stray ones"""
    lab, n = ndimage.label(fg, structure=np.ones((3, 3)))
    out = []
    for l in range(1, n + 1):
        if rs.rand() > share:
            continue
        ring, _ = ring_of(lab == l)
        keep, _ = simplify(ring)
        for v in keep[::max(1, len(keep) // 8)]:
            out.append(ring[v] + rs.uniform(-jitter, jitter, 2))
    for _ in range(int(rs.randint(0, 6))):
        out.append(rs.uniform(0, fg.shape[0], 2))
    out = np.asarray(out, dtype=np.float32).reshape(-1, 2)
    return out[rs.permutation(len(out))]


# ------------------------------------------------------------------------------------------------ the shapes the CPU and GPU tests share
def rect(n, y, x, h, w):
    m = np.zeros((n, n), bool)
    m[y:y + h, x:x + w] = True
    return m


def shape_l(n=12):
    m = rect(n, 2, 2, 6, 2)
    m[6:8, 2:7] = True
    return m


def shape_diagonal(n=12, k=5):
    m = np.zeros((n, n), bool)
    m[np.arange(2, 2 + k), np.arange(2, 2 + k)] = True
    return m


def shape_u(n=12, arm=1, height=7):
    """two arms `arm` pixels wide, one pixel apart, joined at the bottom: step B closes the gap"""
    m = np.zeros((n, n), bool)
    m[1:1 + height, 1:1 + arm] = True
    m[1:1 + height, 2 + arm:2 + 2 * arm] = True
    m[height, 1:2 + 2 * arm] = True
    return m


def shape_set():
    """three 48 x 48 images: (rectangle, L, 5-pixel diagonal, single pixel, two blobs with one diagonal contact, U with a one-pixel gap), (a ring with a
    3 x 3 hole, a comb, a cross that touches all four image borders), the full image"""
    n = 48
    a = np.zeros((n, n), bool)
    a[2:5, 3:8] = True                                                          # rectangle
    a[8:14, 2:4] = True; a[12:14, 2:7] = True                                   # L
    a[np.arange(5), np.arange(20, 25)] = True                                   # diagonal
    a[10, 30] = True                                                            # single pixel
    a[20:24, 20:24] = True; a[24:27, 24:29] = True                              # one diagonal contact
    a[30:37, 5] = True; a[30:37, 7] = True; a[36, 6] = True                     # U, 3 wide and 7 tall
    b = np.zeros((n, n), bool)
    b[:, 24] = True; b[24, :] = True                                            # cross
    b[4:11, 4:11] = True; b[6:9, 6:9] = False                                   # ring with a 3 x 3 hole
    b[30:40, 30:46:3] = True; b[39, 30:46] = True                               # comb: teeth two pixels apart stay apart in T
    return np.stack([a, b, np.ones((n, n), bool)])


def junction_cases():
    """three 48 x 48 images and their junctions: (no junction), (a square with exactly two matched junctions -> ring; a square with three; a square whose
    three junctions share their coordinates, of which only the lowest index can ever be the nearest), (600 junctions)"""
    n = 48
    fg = np.zeros((3, n, n), bool)
    fg[0, 5:15, 5:20] = True; fg[0, 30:40, 10:14] = True
    fg[1, 4:14, 4:14] = True; fg[1, 4:14, 30:40] = True; fg[1, 30:40, 4:14] = True
    fg[2] = random_regions(np.random.RandomState(77), n)
    j1 = [(4.3, 4.2), (14.1, 13.8),                                # two corners of the first square
          (30.2, 4.4), (40.3, 4.1), (39.8, 14.2),                  # three corners of the second
          (4.25, 30.5), (4.25, 30.5), (4.25, 30.5)]                # one point three times
    j2 = np.random.RandomState(78).uniform(0, n, (MAXJ, 2))
    return fg, [np.zeros((0, 2)), np.asarray(j1), j2]


def smooth_cases():
    """three 48 x 48 images with a disc of radius 20 each: 45 junctions on its rim (every turn of the junction polygon is 8 degrees: nothing is kept, the
    case in which the reference raises), 24 junctions (15 degrees: all kept), no junction"""
    n = 48
    yy, xx = np.mgrid[:n, :n]
    disc = (yy + 0.5 - 24) ** 2 + (xx + 0.5 - 24) ** 2 <= 20 ** 2
    rim = lambda k: np.stack([24 + 20 * np.cos(2 * np.pi * (np.arange(k) + 0.5) / k), 24 + 20 * np.sin(2 * np.pi * (np.arange(k) + 0.5) / k)], 1)
    return np.stack([disc, disc, disc]), [rim(45), rim(24), np.zeros((0, 2))]


def big_set():
    """two 224 x 224 images: (small shapes, a 150 x 110 block with a notch (its box is past what runs in LDS), a 118 x 106 comb whose box fits but whose ring
    does not and that no junction is near), the full image (the longest ring of one region)"""
    n = 224
    a = np.zeros((n, n), bool)
    a[10:20, 10:20] = True; a[20:30, 20:30] = True
    a[40:80, 160:200] = True; a[50:70, 170:190] = False
    a[3, 100] = True
    a[70:220, 2:112] = True; a[70:110, 50:60] = False
    a[100:218, 116:222:3] = True; a[217, 116:222] = True
    rs = np.random.RandomState(5)
    ja = np.concatenate([np.asarray([(2.2, 70.1), (2.4, 219.8), (111.7, 220.2), (112.1, 69.9), (50.2, 70.3), (59.8, 109.7)]), rs.uniform(0, 108, (40, 2))])
    jb = np.concatenate([np.asarray([(0.4, 0.3), (0.2, 223.9), (223.8, 223.7), (223.6, 0.4)]), rs.uniform(20, 200, (30, 2))])
    return np.stack([a, np.ones((n, n), bool)]), [ja, jb]


def load_fixture():
    """tests/golden/hisup_polygon.npz -> (foreground bool [6, 48, 48], junctions per image, {(image, label): the reference's polygon float64 [k, 2]})"""
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hisup_polygon.npz"), allow_pickle=False)
    shape = tuple(int(x) for x in d["shape"])
    fg = np.unpackbits(d["fg"])[:int(np.prod(shape))].reshape(shape).astype(bool)
    ends = np.cumsum(d["junc_n"])
    juncs = [d["juncs"][e - n:e] for e, n in zip(ends, d["junc_n"])]
    pends = np.cumsum(d["rows"][:, 2])
    polys = {(int(b), int(l)): d["polys"][e - n:e] for (b, l, n), e in zip(d["rows"], pends)}
    return fg, juncs, polys
