"""The corner-aware contour simplification of FFL's post_process restated in float64 numpy, sequential and literal, for the tests of
p3_corner_split: Douglas-Peucker as skimage.measure.approximate_polygon publishes it (a stack of sections, `dists > tolerance`, argmax, perpendicular or
end-point distance), detect_corners (models/ffl/frame_field_utils.py:71-114) over compute_crossfield_uv evaluated at the vertices,
split_polylines_corner (predict/ffl/polygonize_utils.py:47-61) and Douglas-Peucker again per piece.  tests/test_corner_split_cpu.py pins stages B and C to the
reference's own functions through tests/golden/corner_split.npz; Douglas-Peucker has no other pin than hand-checkable cases (neither skimage nor shapely is
installed).

Every function also reports the MARGINS of its own decisions into a `Margins` object, so that the fixtures can be shown to hold no decision that rounding
could turn: for a Douglas-Peucker section |largest distance - tol| and, where it splits, the gap between its two largest distances (an exact tie is
counted apart); for a corner decision ||e.u| - |e.v|| / (|e| max(|u|, |v|)) of each of the two edges."""
import numpy as np


class Margins:
    def __init__(self):
        self.dp_tol, self.dp_gap, self.dp_ties, self.corner = [], [], 0, []

    def smallest(self):
        """(smallest |distance - tol|, smallest gap between the two largest distances of a splitting section, exact ties, smallest corner margin)"""
        return (min(self.dp_tol, default=np.inf), min(self.dp_gap, default=np.inf), self.dp_ties, min(self.corner, default=np.inf))


def section_distances(pts, s, e):
    """point-to-segment distances of pts[s+1 .. e-1] to the section (s, e), float64, in the operation order of the kernel"""
    q = np.asarray(pts, dtype=np.float64)
    k = q[s + 1:e]
    dr, dc = q[e, 0] - q[s, 0], q[e, 1] - q[s, 1]
    ar, ac = k[:, 0] - q[s, 0], k[:, 1] - q[s, 1]
    br, bc = q[e, 0] - k[:, 0], q[e, 1] - k[:, 1]
    inside = (ar * dr + ac * dc > 0.0) & (br * dr + bc * dc > 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        perp = np.abs(ar * dc - ac * dr) / np.sqrt(dr * dr + dc * dc)
    ends = np.minimum(np.sqrt(ar * ar + ac * ac), np.sqrt(br * br + bc * bc))
    return np.where(inside, perp, ends)


def dp(pts, tol, margins=None):
    """Douglas-Peucker -> bool [n], True = kept.  tol <= 0 keeps every point."""
    n = len(pts)
    keep = np.zeros(n, dtype=bool)
    if n == 0:
        return keep
    if not tol > 0:
        keep[:] = True
        return keep
    keep[0] = keep[n - 1] = True
    stack = [(0, n - 1)]
    while stack:
        s, e = stack.pop()
        if e - s < 2:
            continue
        d = section_distances(pts, s, e)
        i = int(np.argmax(d))          # the first of equal maxima
        if margins is not None:
            margins.dp_tol.append(abs(float(d[i]) - tol))
        if d[i] > tol:
            if margins is not None and len(d) > 1:
                gap = float(d[i] - np.max(np.delete(d, i)))
                if gap == 0.0:
                    margins.dp_ties += 1
                else:
                    margins.dp_gap.append(gap)
            m = s + 1 + i
            keep[m] = True
            stack.append((m, e))
            stack.append((s, m))
    return keep


def crossfield_uv_at(c0c2, rc):
    """compute_crossfield_uv at the pixels rc [k,2] of one image's c0c2 [4,H,W] -> complex u [k], v [k]"""
    f = np.asarray(c0c2, dtype=np.float64)[:, rc[:, 0], rc[:, 1]]
    c0, c2 = f[0] + 1j * f[1], f[2] + 1j * f[3]
    s = np.sqrt(np.power(c2, 2) - 4 * c0)
    return np.sqrt((c2 + s) / 2), np.sqrt((c2 - s) / 2)


def _is_corner(points, left, right, c0c2, margins):
    if points.shape[0] == 0:
        return np.empty(0, dtype=bool)
    H, W = c0c2.shape[1:]
    rc = np.round(points).astype(np.int64)
    rc[:, 0] = np.clip(rc[:, 0], 0, H - 1)
    rc[:, 1] = np.clip(rc[:, 1], 0, W - 1)
    u, v = crossfield_uv_at(c0c2, rc)
    score = lambda e, w: np.abs(e[:, 0] * w.real + e[:, 1] * w.imag)
    lu, lv, ru, rv = score(left, u), score(left, v), score(right, u), score(right, v)
    if margins is not None:
        big = np.maximum(np.abs(u), np.abs(v))
        for e, a, b in ((left, lu, lv), (right, ru, rv)):
            norm = np.hypot(e[:, 0], e[:, 1]) * big
            margins.corner += [float(x) for x in (np.abs(a - b)[norm > 0] / norm[norm > 0])]          # an edge of length 0 scores 0 < 0: exact
    return np.logical_xor(lv < lu, rv < ru)


def detect_corners(polyline, c0c2, margins=None):
    """corner mask of one polyline float64 [m,2] (m >= 1) in the frame field c0c2 [4,H,W] of its image"""
    p = np.asarray(polyline, dtype=np.float64)
    mask = np.zeros(p.shape[0], dtype=bool)
    if np.max(np.abs(p[0] - p[-1])) < 1e-6:
        left = np.concatenate([p[-2:-1] - p[-1:], p[:-2] - p[1:-1]], axis=0)
        right = p[1:] - p[:-1]
        mask[:-1] = _is_corner(p[:-1], left, right, c0c2, margins)
        mask[-1] = mask[0]
    else:
        mask[0] = mask[-1] = True
        mask[1:-1] = _is_corner(p[1:-1], p[:-2] - p[1:-1], p[2:] - p[1:-1], c0c2, margins)
    return mask


def split_indices(mask):
    """split_polylines_corner on vertex numbers: -> list of int arrays, the vertices of every piece in order"""
    m = len(mask)
    splits, = np.where(mask)
    if len(splits) == 0:
        return [np.arange(m)]
    out = [np.arange(splits[i], splits[i + 1] + 1) for i in range(len(splits) - 1)]
    if not mask[0] and not mask[-1]:
        out.append(np.concatenate([np.arange(splits[-1], m), np.arange(0, splits[0] + 1)]))
    return out


def explicit_points(pos, index, sl, closed):
    """the explicit point sequence of one polyline -> float32 [n,2], with every index clamped as the device clamps it"""
    N = pos.shape[0]
    L = N if index is None else len(index)
    a = min(max(int(sl[0]), 0), L)
    b = min(max(int(sl[1]), a), L)
    ids = np.arange(a, b)
    if index is not None:
        ids = np.clip(np.asarray(index)[ids], 0, N - 1)
    if closed and len(ids):
        ids = np.concatenate([ids, ids[:1]])
    return pos[ids]


def corner_split(pos, index, slices, closed, poly_batch, c0c2, tol_pre, tol, margins=None):
    """stages A - D of every polyline -> dict with the device's outputs: out_pos f32 [V,2], out_src i32 [V], piece_slice i64 [Q,2], piece_poly i32 [Q],
    piece_batch i32 [Q], stage_flags u8 [E] (bit 0 kept by A, bit 1 corner, bit 2 kept by D in some piece), counts (V, Q, longest piece), offsets i64 [P+1]
    (where each polyline's explicit points start in stage_flags)"""
    pos = np.asarray(pos, dtype=np.float32)
    c0c2 = np.asarray(c0c2)
    B = c0c2.shape[0]
    out_pos, out_src, piece_slice, piece_poly, piece_batch, flags, offsets = [], [], [], [], [], [], [0]
    at, longest = 0, 0
    for i in range(len(slices)):
        q = explicit_points(pos, index, slices[i], bool(closed[i]))
        n = len(q)
        fl = np.zeros(n, dtype=np.uint8)
        offsets.append(offsets[-1] + n)
        if n >= 2:
            b = min(max(int(poly_batch[i]), 0), B - 1)
            q64 = q.astype(np.float64)
            keep_a = dp(q64, tol_pre, margins)
            ia = np.flatnonzero(keep_a)
            fl[ia] |= 1
            mask = detect_corners(q64[ia], c0c2[b], margins)
            fl[ia[mask]] |= 2
            for piece in split_indices(mask):
                src = ia[piece]
                src = src[dp(q64[src], tol, margins)]
                fl[src] |= 4
                out_pos.append(q[src])
                out_src.append(src)
                piece_slice.append((at, at + len(src)))
                piece_poly.append(i)
                piece_batch.append(b)
                at += len(src)
                longest = max(longest, len(src))
        flags.append(fl)
    cat = lambda xs, dt, shape: np.concatenate(xs).astype(dt) if xs else np.zeros(shape, dtype=dt)
    return {"out_pos": cat(out_pos, np.float32, (0, 2)), "out_src": cat(out_src, np.int32, (0,)),
            "piece_slice": np.array(piece_slice, dtype=np.int64).reshape(-1, 2), "piece_poly": np.array(piece_poly, dtype=np.int32),
            "piece_batch": np.array(piece_batch, dtype=np.int32), "stage_flags": cat(flags, np.uint8, (0,)), "counts": (at, len(piece_slice), longest),
            "offsets": np.array(offsets, dtype=np.int64)}


def pieces_of_contour(contour, c0c2, tol_pre, tol):
    """the host path per contour: one explicit polyline float [n,2] -> list of float64 [k,2] pieces"""
    q = np.asarray(contour, dtype=np.float64)
    if len(q) < 2:
        return []
    q = q[dp(q, tol_pre)]
    return [q[p][dp(q[p], tol)] for p in split_indices(detect_corners(q, c0c2))]
