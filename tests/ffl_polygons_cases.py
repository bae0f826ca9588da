"""Inputs shared by test_ffl_polygons_cpu.py and test_ffl_polygons_gpu.py: the hand cases of DESIGN.md section 19 on a 16 x 16 map with their expected
polygons written out by hand, and seeded random planar graphs.  Everything here is in (x, y); piece() turns a vertex list into the (row, col) float32 array
the device takes.  Coordinates are integers or half-integers: every predicate is exact."""
import numpy as np

H = W = 16
BORDER = [(0, 0), (15, 0), (15, 15), (0, 15), (0, 0)]          # the border shell: positive shoelace sum, start at the smallest node


def piece(*xy):
    return np.array([(y, x) for x, y in xy], dtype=np.float32).reshape(-1, 2)


def ring(*xy):
    return [(float(x), float(y)) for x, y in xy]


def square(x0, y0, x1, y1):
    """the shell of an axis-parallel square as this stage puts it out, and the same boundary as a hole (seen from outside)"""
    return ring((x0, y0), (x1, y0), (x1, y1), (x0, y1), (x0, y0)), ring((x0, y0), (x0, y1), (x1, y1), (x1, y0), (x0, y0))


_A, _A_HOLE = square(2, 2, 5, 5)
_B, _B_HOLE = square(9, 5, 12, 8)
_TWO_SQUARES = [[ring(*BORDER), _A_HOLE, _B_HOLE], [_A], [_B]]

# name -> (pieces, expected status, expected polygons [[shell, hole, ...], ...], expected areas)
HAND = {
    "one_square": ([piece((4, 4), (8, 4), (8, 8), (4, 8), (4, 4))], 0,
                   [[ring(*BORDER), square(4, 4, 8, 8)[1]], [square(4, 4, 8, 8)[0]]], [225 - 16, 16]),
    "ring_in_ring": ([piece((2, 2), (12, 2), (12, 12), (2, 12), (2, 2)), piece((5, 5), (9, 5), (9, 9), (5, 9), (5, 5))], 0,
                     [[ring(*BORDER), square(2, 2, 12, 12)[1]], [square(2, 2, 12, 12)[0], square(5, 5, 9, 9)[1]], [square(5, 5, 9, 9)[0]]],
                     [225 - 100, 100 - 16, 16]),
    # the outside ring passes (6, 6) twice: from (2, 6) it goes on to (6, 10), from (10, 6) to (6, 2)
    "touching_squares": ([piece((2, 2), (6, 2), (6, 6), (2, 6), (2, 2)), piece((6, 6), (10, 6), (10, 10), (6, 10), (6, 6))], 0,
                         [[ring(*BORDER), ring((2, 2), (2, 6), (6, 6), (6, 10), (10, 10), (10, 6), (6, 6), (6, 2), (2, 2))],
                          [square(2, 2, 6, 6)[0]], [square(6, 6, 10, 10)[0]]], [225 - 32, 16, 16]),
    # stage C's wrapped last piece (4, 8) -> (4, 4) -> (8, 4), and the edge (8, 4) - (8, 8) twice
    "square_in_pieces": ([piece((8, 4), (8, 8)), piece((8, 8), (4, 8)), piece((4, 8), (4, 4), (8, 4)), piece((8, 8), (8, 4))], 0,
                         [[ring(*BORDER), square(4, 4, 8, 8)[1]], [square(4, 4, 8, 8)[0]]], [225 - 16, 16]),
    "open_polyline": ([piece((0, 5), (5, 5), (10, 9), (15, 9))], 0,
                      [[ring((0, 0), (15, 0), (15, 9), (10, 9), (5, 5), (0, 5), (0, 0))], [ring((0, 5), (5, 5), (10, 9), (15, 9), (15, 15), (0, 15), (0, 5))]],
                      [105, 120]),
    "dangle": ([piece((3, 3), (7, 3), (7, 7))], 0, [[ring(*BORDER)]], [225]),
    "theta": ([piece((4, 8), (8, 4), (12, 8)), piece((4, 8), (12, 8)), piece((4, 8), (8, 12), (12, 8))], 0,
              [[ring(*BORDER), ring((4, 8), (8, 12), (12, 8), (8, 4), (4, 8))], [ring((4, 8), (8, 4), (12, 8), (4, 8))], [ring((4, 8), (12, 8), (8, 12), (4, 8))]],
              [225 - 32, 16, 16]),
    "bridge": ([piece((2, 2), (5, 2), (5, 5), (2, 5), (2, 2)), piece((9, 5), (12, 5), (12, 8), (9, 8), (9, 5)), piece((5, 5), (9, 5))], 0,
               _TWO_SQUARES, [225 - 18, 9, 9]),
    "bridge_with_tail": ([piece((2, 2), (5, 2), (5, 5), (2, 5), (2, 2)), piece((9, 5), (12, 5), (12, 8), (9, 8), (9, 5)), piece((5, 5), (7, 5), (9, 5)),
                          piece((7, 5), (7, 9), (8, 10))], 0, _TWO_SQUARES, [225 - 18, 9, 9]),
    "x_crossing": ([piece((3, 3), (9, 9)), piece((3, 9), (9, 3))], 1, [], []),
    "vertex_in_edge": ([piece((3, 3), (9, 3)), piece((6, 3), (6, 8))], 1, [], []),
    "no_pieces": ([], 0, [[ring(*BORDER)]], [225]),
}


def graded_indicator(h=H, w=W, seed=0):
    """a map whose every window has another mean: values in [0, 1) on a 1 / 1024 grid, exact in fp32"""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 1024, size=(h, w)) / 1024.0).astype(np.float32)


def random_graph(seed, n_points=30):
    """Delaunay edges over distinct half-integer points strictly inside the border, a random third deleted, each edge a 2-point piece: dangles, bridges
    and large faces in every seed"""
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(1000 + seed)
    grid = rng.permutation(28 * 28)[:n_points]
    pts = np.stack([grid % 28, grid // 28], 1) * 0.5 + 0.5          # 0.5 .. 14
    tri = Delaunay(pts)
    edges = sorted({tuple(sorted((int(s[i]), int(s[j])))) for s in tri.simplices for i, j in ((0, 1), (1, 2), (0, 2))})
    keep = rng.permutation(len(edges))[: (2 * len(edges)) // 3]
    return [piece(tuple(pts[edges[k][0]]), tuple(pts[edges[k][1]])) for k in sorted(keep)]
