"""float64 restatement of DESIGN.md section 19 (FFL polygons: planar faces, area and probability filters), written from the definition and not from
csrc/ffl_polygons.hip: plain numpy, dictionaries and networkx (components and bridges, so that step 5 does not rest on the traced-ring rule).

faces(pieces, H, W)           -> (status bits, [polygon]) with polygon = [shell, hole, ...], a ring = closed list of (x, y) tuples of Python floats
geom_prob(polygon, indicator) -> float64 probability of compute_geom_prob as section 19 states it
run(pieces_batch, indicator, min_area, seg_threshold) -> the device's outputs as numpy arrays (ring_pos is (row, col))."""
import functools
import math

import networkx as nx
import numpy as np


def _pt(v):
    """a (row, col) vertex holding float32 values -> (x, y) Python floats, -0 as +0"""
    return (float(np.float32(v[1])) + 0.0, float(np.float32(v[0])) + 0.0)


def _orient(a, b, c):
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def border_sides(H, W):
    xm, ym = float(W - 1), float(H - 1)
    return [(lambda p: p[0] == 0.0 and 0.0 <= p[1] <= ym, 1), (lambda p: p[1] == ym and 0.0 <= p[0] <= xm, 0),
            (lambda p: p[0] == xm and 0.0 <= p[1] <= ym, 1), (lambda p: p[1] == 0.0 and 0.0 <= p[0] <= xm, 0)]


def graph(pieces, H, W):
    """steps 1 - 3 -> (nodes sorted by (x, y), set of edges as sorted node pairs), or None when a coordinate is not finite"""
    segs = []
    for piece in pieces:
        pts = [_pt(v) for v in np.asarray(piece).reshape(-1, 2)]
        for a, b in zip(pts[:-1], pts[1:]):
            if not all(map(math.isfinite, a + b)):
                return None
            if a != b:
                segs.append((a, b))
    xm, ym = float(W - 1), float(H - 1)
    nodes = {p for s in segs for p in s} | {(0.0, 0.0), (0.0, ym), (xm, ym), (xm, 0.0)}
    edges = {tuple(sorted(s)) for s in segs}
    for on, axis in border_sides(H, W):
        side = sorted((p for p in nodes if on(p)), key=lambda p: p[axis])
        edges |= {tuple(sorted(e)) for e in zip(side[:-1], side[1:])}
    return sorted(nodes), edges


def planar_as_given(edges):
    """step 4, every pair of edges at once"""
    E = np.array(sorted(edges), dtype=np.float64).reshape(-1, 2, 2)
    if len(E) < 2:
        return True
    A, B = E[:, None, 0], E[:, None, 1]          # edge i = (A, B) against edge j = (C, D)
    C, D = E[None, :, 0], E[None, :, 1]
    o = lambda a, b, c: (b[..., 0] - a[..., 0]) * (c[..., 1] - a[..., 1]) - (b[..., 1] - a[..., 1]) * (c[..., 0] - a[..., 0])
    box = lambda a, b, c: ((c[..., 0] >= np.minimum(a[..., 0], b[..., 0])) & (c[..., 0] <= np.maximum(a[..., 0], b[..., 0])) &
                           (c[..., 1] >= np.minimum(a[..., 1], b[..., 1])) & (c[..., 1] <= np.maximum(a[..., 1], b[..., 1])))
    same = lambda a, b: (a[..., 0] == b[..., 0]) & (a[..., 1] == b[..., 1])
    o1, o2, o3, o4 = o(A, B, C), o(A, B, D), o(C, D, A), o(C, D, B)
    proper = (o1 * o2 < 0) & (o3 * o4 < 0)
    touch = ((o1 == 0) & box(A, B, C)) | ((o2 == 0) & box(A, B, D)) | ((o3 == 0) & box(C, D, A)) | ((o4 == 0) & box(C, D, B))
    common = same(A, C).astype(int) + same(A, D) + same(B, C) + same(B, D)
    bad0 = (common == 0) & (proper | touch)
    # one common node O: the other ends P, Q are collinear with it and on the same side
    O = np.where((same(A, C) | same(A, D))[..., None], A, B)
    P = np.where((same(A, C) | same(A, D))[..., None], B, A)
    Q = np.where((same(C, A) | same(C, B))[..., None], D, C)
    dot = (P[..., 0] - O[..., 0]) * (Q[..., 0] - O[..., 0]) + (P[..., 1] - O[..., 1]) * (Q[..., 1] - O[..., 1])
    bad1 = (common == 1) & (o(O, P, Q) == 0) & (dot > 0)
    return not bool((bad0 | bad1).any())


def _angle_cmp(o):
    def half(d):
        return 0 if (d[1] > 0 or (d[1] == 0 and d[0] > 0)) else 1

    def cmp(g, h):
        dg, dh = (g[0] - o[0], g[1] - o[1]), (h[0] - o[0], h[1] - o[1])
        if half(dg) != half(dh):
            return half(dg) - half(dh)
        c = dg[0] * dh[1] - dg[1] * dh[0]
        return -1 if c > 0 else (1 if c < 0 else 0)
    return cmp


def shoelace(ring):
    S = 0.0
    for a, b in zip(ring[:-1], ring[1:]):
        S += a[0] * b[1] - b[0] * a[1]
    return S


def crossing_inside(ring, p):
    """crossing number of the ray from p towards +x with the closed ring, by orientation signs"""
    par = False
    for a, b in zip(ring[:-1], ring[1:]):
        if (a[1] <= p[1]) != (b[1] <= p[1]):
            o = _orient(a, b, p)
            if (o > 0) if b[1] > a[1] else (o < 0):
                par = not par
    return par


def faces(pieces, H, W):
    g = graph(pieces, H, W)
    if g is None:
        return 2, []
    nodes, edges = g
    if not planar_as_given(edges):
        return 1, []
    G = nx.Graph(list(edges))
    while True:          # step 5: dangles, then cuts
        leaves = [n for n in G if G.degree(n) <= 1]
        if not leaves:
            break
        G.remove_nodes_from(leaves)
    G.remove_edges_from(list(nx.bridges(G)))
    G.remove_nodes_from([n for n in G if G.degree(n) == 0])
    assert all(G.degree(n) >= 2 for n in G), "one pass of cuts after the dangles leaves no dangle"
    # step 6
    order = {v: sorted(G[v], key=functools.cmp_to_key(_angle_cmp(v))) for v in G}
    nxt = {}
    for u, v in list(G.edges) + [(v, u) for u, v in G.edges]:
        ring = order[v]
        nxt[(u, v)] = (v, ring[ring.index(u) - 1])
    rings, ring_of = [], {}
    for h in sorted(nxt):          # key order: the first half-edge met of a ring is its start
        if h in ring_of:
            continue
        walk, x = [], h
        while x not in ring_of:
            ring_of[x] = len(rings)
            walk.append(x)
            x = nxt[x]
        rings.append(walk)
    assert all(ring_of[(u, v)] != ring_of[(v, u)] for u, v in G.edges), "no cut is left: the traced-ring rule agrees with networkx's bridges"
    # step 7
    comp = {n: i for i, c in enumerate(nx.connected_components(G)) for n in c}
    closed = [[h[0] for h in walk] + [walk[0][0]] for walk in rings]
    S = [shoelace(r) for r in closed]
    if any(s == 0 or s != s for s in S):
        return 4, []
    shells = [i for i in range(len(rings)) if S[i] > 0]          # in key order already
    holes = {i: [] for i in shells}
    for i in range(len(rings)):
        if S[i] > 0:
            continue
        p = closed[i][0]
        inside = [j for j in shells if comp[closed[j][0]] != comp[p] and crossing_inside(closed[j], p)]
        if inside:
            holes[min(inside, key=lambda j: S[j])].append(i)
    return 0, [[closed[i]] + [closed[k] for k in holes[i]] for i in shells]


def polygon_area(poly):
    area = shoelace(poly[0]) * 0.5
    for hole in poly[1:]:
        area -= abs(shoelace(hole) * 0.5)
    return area


def covered(rings, xs, ys):
    """rings: integer [n, 2] (x, y) arrays, closed.  -> bool map over the pixel grids xs, ys"""
    on = np.zeros(xs.shape, dtype=bool)
    par = np.zeros(xs.shape, dtype=bool)
    for r in rings:
        for (ax, ay), (bx, by) in zip(r[:-1].tolist(), r[1:].tolist()):
            cr = (bx - ax) * (ys - ay) - (by - ay) * (xs - ax)
            on |= (cr == 0) & (xs >= min(ax, bx)) & (xs <= max(ax, bx)) & (ys >= min(ay, by)) & (ys <= max(ay, by))
            par ^= ((ay <= ys) != (by <= ys)) & ((cr > 0) if by > ay else (cr < 0))
    return on | par


def raster(poly, H, W):
    """-> (bool [H, W] raster of the polygon in image coordinates, or None when the bounds rule gives probability 0)"""
    shell = np.array(poly[0], dtype=np.float64)
    minx, miny = int(shell[:, 0].min()), int(shell[:, 1].min())          # int() truncates towards zero, as in the reference
    maxx, maxy = int(shell[:, 0].max()) + 1, int(shell[:, 1].max()) + 1
    if minx < 0 or miny < 0 or maxx > W or maxy > H:
        return None
    rounded = [np.round(np.array(r, dtype=np.float64) - (minx, miny)).astype(np.int64) + (minx, miny) for r in poly]
    ys, xs = np.mgrid[0:H, 0:W].astype(np.int64)
    window = (xs >= minx) & (xs < maxx) & (ys >= miny) & (ys < maxy)
    m = covered(rounded[:1], xs, ys)
    if len(rounded) > 1:
        m &= ~covered(rounded[1:], xs, ys)
    return m & window


def geom_prob(poly, indicator):
    ind = np.asarray(indicator, dtype=np.float64)
    m = raster(poly, *ind.shape)
    if m is None or not m.any():
        return 0.0
    total = 0.0
    for v in ind[m]:          # row-major
        total += v
    return total / int(m.sum())


def run(pieces_batch, indicator, min_area, seg_threshold):
    """pieces_batch: per image a list of (row, col) arrays; indicator [B, H, W]"""
    indicator = np.asarray(indicator)
    B, H, W = indicator.shape
    pos, rsl, prs, pb, area, prob, flags, status = [], [], [], [], [], [], [], []
    for b in range(B):
        st, polys = faces(pieces_batch[b], H, W)
        status.append(st)
        for poly in polys:
            r0 = len(rsl)
            for ring in poly:
                rsl.append((len(pos), len(pos) + len(ring)))
                pos += [(y, x) for x, y in ring]
            prs.append((r0, len(rsl)))
            pb.append(b)
            a, p = polygon_area(poly), geom_prob(poly, indicator[b])
            area.append(a)
            prob.append(p)
            flags.append((0 if min_area < a else 1) | (0 if seg_threshold < p else 2))
    return dict(ring_pos=np.array(pos, dtype=np.float32).reshape(-1, 2), ring_slice=np.array(rsl, dtype=np.int64).reshape(-1, 2),
                poly_rings=np.array(prs, dtype=np.int64).reshape(-1, 2), poly_batch=np.array(pb, dtype=np.int32), poly_area=np.array(area, dtype=np.float64),
                poly_prob=np.array(prob, dtype=np.float64), poly_flags=np.array(flags, dtype=np.int32), image_status=np.array(status, dtype=np.int32),
                counts=(len(prs), len(rsl), len(pos)))


def point_in_polygon(poly, p):
    """p strictly inside the shell and in none of the holes (for sample points away from every edge)"""
    return crossing_inside(poly[0], p) and not any(crossing_inside(h, p) for h in poly[1:])
