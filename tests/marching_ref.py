"""Two sequential float64 restatements of skimage.measure.find_contours(image, level, fully_connected='low', positive_orientation='high') - what
predict/ffl/polygonize_utils.py:15-44 of the reference calls per image - and the seeded inputs the contour tests share.

skimage is not a dependency of this repository and the reference tree does not carry it, so neither function is pinned to skimage itself: both restate the
published marching-squares algorithm, and the documentation example of find_contours (test_init_contours_cpu.py) is the one value taken from there.

find_contours_ref    the published assembly: the segments of all cells in raster order are joined BY COORDINATE through two dictionaries (fragment starts and
                     fragment ends); of two fragments that meet, the one created first keeps its number; the result is reversed ('high').  Structurally
                     unlike the kernel (csrc/contours.hip), which links by edge identity and ranks lists in parallel.
link_by_edges_ref    the definition DESIGN.md section 13 gives, walked sequentially: a vertex is a crossed grid edge, succ[to] = from, contours start at the
                     vertex that is the `from` of no segment (open) or at the `to` of their largest-key segment (closed), ordered by smallest segment key.
The two agree wherever no pixel equals the level exactly (has_level_pixels); where one does, several edges share one point and coordinate joining links
differently - those inputs are held to link_by_edges_ref alone.

Both return a list of (n, 2) float64 arrays of (row, col); a closed contour repeats its first point at the end."""
from collections import deque

import numpy as np

T, R, B, L = 0, 1, 2, 3
# segments (from side, to side) of a cell per case = (ul > level) + 2 (ur > level) + 4 (ll > level) + 8 (lr > level), in slot order; 6 and 9 in their
# fully_connected='low' form
SEGMENTS = {1: [(T, L)], 2: [(R, T)], 3: [(R, L)], 4: [(L, B)], 5: [(T, B)], 6: [(R, T), (L, B)], 7: [(R, B)], 8: [(B, R)], 9: [(T, L), (B, R)],
            10: [(B, T)], 11: [(B, L)], 12: [(L, R)], 13: [(T, R)], 14: [(L, T)]}


def _frac(a, b, level):
    return 0.0 if a == b else (level - a) / (b - a)


def _cells(image, level):
    """every emitting cell in raster order: (r, c, case, the four crossing points by side)"""
    image = np.asarray(image, dtype=np.float64)
    H, W = image.shape
    level = float(level)
    for r in range(H - 1):
        for c in range(W - 1):
            ul, ur, ll, lr = float(image[r, c]), float(image[r, c + 1]), float(image[r + 1, c]), float(image[r + 1, c + 1])
            if np.isnan(ul) or np.isnan(ur) or np.isnan(ll) or np.isnan(lr):
                continue
            case = int(ul > level) + 2 * int(ur > level) + 4 * int(ll > level) + 8 * int(lr > level)
            if case in (0, 15):
                continue
            pts = {T: (float(r), c + _frac(ul, ur, level)), B: (float(r + 1), c + _frac(ll, lr, level)),
                   L: (r + _frac(ul, ll, level), float(c)), R: (r + _frac(ur, lr, level), float(c + 1))}
            yield r, c, case, pts


def find_contours_ref(image, level=0.5, positive_orientation="high"):
    image = np.asarray(image, dtype=np.float64)
    if image.ndim != 2:
        raise ValueError("find_contours_ref: a 2-d map")
    fragments, starts, ends, made = {}, {}, {}, 0          # number -> deque of points; first point -> (deque, number); last point -> (deque, number)
    for _, _, case, pts in _cells(image, level):
        for side_from, side_to in SEGMENTS[case]:
            p, q = pts[side_from], pts[side_to]
            if p == q:
                continue          # a degenerate segment (a corner pixel equal to the level)
            behind, behind_no = starts.pop(q, (None, None))          # the fragment that begins where this segment ends
            front, front_no = ends.pop(p, (None, None))              # the fragment that ends where this segment begins
            if behind is not None and front is not None:
                if behind is front:
                    front.append(q)          # the contour closes
                elif behind_no > front_no:          # the one created first keeps its number
                    front.extend(behind)
                    fragments.pop(behind_no, None)
                    starts[front[0]] = (front, front_no)
                    ends[front[-1]] = (front, front_no)
                else:
                    behind.extendleft(reversed(front))
                    starts.pop(front[0], None)
                    fragments.pop(front_no, None)
                    starts[behind[0]] = (behind, behind_no)
                    ends[behind[-1]] = (behind, behind_no)
            elif behind is None and front is None:
                new = deque((p, q))
                fragments[made] = new
                starts[p] = (new, made)
                ends[q] = (new, made)
                made += 1
            elif front is None:
                behind.appendleft(p)
                starts[p] = (behind, behind_no)
            else:
                front.append(q)
                ends[q] = (front, front_no)
    step = -1 if positive_orientation == "high" else 1          # 'high' reverses every contour
    return [np.array(fragments[k], dtype=np.float64)[::step] for k in sorted(fragments)]


def link_by_edges_ref(image, level=0.5):
    image = np.asarray(image, dtype=np.float64)
    H, W = image.shape

    def edge(r, c, side):          # identity of the grid edge a cell's side lies on
        return {T: ("h", r, c), B: ("h", r + 1, c), L: ("v", r, c), R: ("v", r, c + 1)}[side]

    pos, succ, key_of, is_from, seg_to = {}, {}, {}, set(), {}
    for r, c, case, pts in _cells(image, level):
        for slot, (side_from, side_to) in enumerate(SEGMENTS[case]):
            e_from, e_to = edge(r, c, side_from), edge(r, c, side_to)
            pos[e_from], pos[e_to] = pts[side_from], pts[side_to]
            key = 2 * (r * (W - 1) + c) + slot
            assert e_to not in succ and e_from not in is_from          # one writer per crossed edge
            succ[e_to] = e_from          # 'high' walks every segment backwards
            key_of[e_to] = key
            seg_to[key] = e_to
            is_from.add(e_from)
    contours, seen = [], set()

    def walk(start):
        chain, keys, v = [start], [], start
        while v in succ:
            keys.append(key_of[v])
            v = succ[v]
            if v == start:
                break
            chain.append(v)
        return chain, keys, v == start and len(keys) > 0

    for v in pos:          # open contours: from the vertex that is the `from` of no segment
        if v not in is_from:
            chain, keys, _ = walk(v)
            seen.update(chain)
            contours.append((min(keys), np.array([pos[e] for e in chain], dtype=np.float64)))
    for v in pos:          # closed ones: from the `to` vertex of their largest-key segment
        if v in seen:
            continue
        chain, keys, closed = walk(v)
        assert closed
        seen.update(chain)
        chain, _, _ = walk(seg_to[max(keys)])
        contours.append((min(keys), np.array([pos[e] for e in chain + chain[:1]], dtype=np.float64)))
    return [c for _, c in sorted(contours, key=lambda kc: kc[0])]


def has_level_pixels(image, level=0.5):
    return bool(np.any(np.asarray(image, dtype=np.float64) == float(level)))


def same_contours(a, b):
    """same count, order, start vertex, closedness and bits"""
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def as_float32(contours):
    return [np.asarray(c, dtype=np.float64).astype(np.float32).reshape(-1, 2) for c in contours]


# ---------------------------------------------------------------------------------------------------------------- inputs (seeded numpy, float32)
def smooth(H, W, seed, bumps=6):
    """a sigmoid of a sum of Gaussian bumps: blobs that close inside the map and some that leave it"""
    rng = np.random.default_rng(seed)
    rr, cc = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    z = np.full((H, W), -1.0)
    for _ in range(bumps):
        r0, c0, s = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.04, 0.14) * min(H, W) + 0.7
        z += rng.uniform(1.5, 3.0) * np.exp(-((rr - r0) ** 2 + (cc - c0) ** 2) / (2 * s * s))
    return (1.0 / (1.0 + np.exp(-4.0 * z))).astype(np.float32)


def doc_example():
    a = np.zeros((3, 3), dtype=np.float32)
    a[0, 0] = a[2, 2] = 1
    return a


def checkerboard(n=12, seed=3):
    """a soft n x n checkerboard: every interior cell is a saddle (cases 6 and 9)"""
    rng = np.random.default_rng(seed)
    rr, cc = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return np.where((rr + cc) % 2 == 0, 0.9, 0.1).astype(np.float32) + rng.uniform(-0.05, 0.05, (n, n)).astype(np.float32)


def cross(H=10, W=13):
    """a cross whose four arms leave the map: open contours at all four borders"""
    a = np.full((H, W), 0.1, dtype=np.float32)
    a[H // 2 - 1:H // 2 + 1, :] = 0.8
    a[:, W // 2 - 1:W // 2 + 2] = 0.9
    return a


def with_nan(H=9, W=11, seed=11):
    a = smooth(H, W, seed, bumps=3)
    a[4, 5] = np.nan
    return a


def serpentine(n=96):
    """2-pixel stripes at period 4, joined at alternate ends: one long closed contour"""
    a = np.zeros((n, n), dtype=np.float32)
    rows = list(range(2, n - 3, 4))
    for k, r in enumerate(rows):
        a[r:r + 2, 2:n - 2] = 1
        if k + 1 < len(rows):
            cols = slice(n - 4, n - 2) if k % 2 == 0 else slice(2, 4)
            a[r + 2:r + 4, cols] = 1
    return a


def level_valued(n=8, seed=5):
    """values in {0, 1/2, 1}: pixels that equal the level 0.5 exactly"""
    return np.random.default_rng(seed).integers(0, 3, (n, n)).astype(np.float32) / 2


def tiny_maps():
    rng = np.random.default_rng(17)
    return {"2x2": rng.uniform(0, 1, (2, 2)).astype(np.float32), "1x5": rng.uniform(0, 1, (1, 5)).astype(np.float32),
            "5x1": rng.uniform(0, 1, (5, 1)).astype(np.float32), "2x9": rng.uniform(0, 1, (2, 9)).astype(np.float32)}


def cases():
    """name -> (map, level): the inputs of the equality tests"""
    out = {"doc": (doc_example(), 0.5)}
    for k, v in tiny_maps().items():
        out[k] = (v, 0.5)
    out.update({"smooth5x7": (smooth(5, 7, 1, bumps=2), 0.5), "smooth33x20": (smooth(33, 20, 7), 0.5), "smooth64_l045": (smooth(64, 64, 7, bumps=9), 0.45),
                "checkerboard12": (checkerboard(), 0.5), "cross10x13": (cross(), 0.5), "nan9x11": (with_nan(), 0.5), "serpentine96": (serpentine(), 0.5)})
    return out
