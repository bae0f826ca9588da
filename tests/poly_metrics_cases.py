"""Inputs shared by test_poly_metrics_cpu.py and test_poly_metrics_gpu.py: the hand cases of DESIGN.md section 21, the seeded generator and the shapes at
which csrc/poly_metrics.hip takes another path.  A case is (name, gt_batch, dt_batch, H, W): per image a list of float32 [n, 2] (x, y) open rings."""
import numpy as np

f32 = lambda pts: np.asarray(pts, dtype=np.float32).reshape(-1, 2)

SQUARE_A = f32([(8, 8), (24, 8), (24, 24), (8, 24)])
SQUARE_B = SQUARE_A + np.float32([3, 0])
FAR = f32([(40, 40), (46, 40), (46, 46), (40, 46)])
TWO = f32([(10, 10), (20, 20)])
SEEDS = (0, 1, 2, 3, 4, 5)


def star(rng, cx, cy, n, r_lo, r_hi):
    """a star-shaped ring of n vertices around (cx, cy): sorted angles with a minimum gap, radii in [r_lo, r_hi]"""
    ang = (np.arange(n) + rng.uniform(0.15, 0.85, n)) * (2 * np.pi / n) + rng.uniform(0, 2 * np.pi)
    rad = rng.uniform(r_lo, r_hi, n)
    return f32(np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1))


def seeded_image(seed):
    """four star-shaped gt rings of 4-8 vertices and radius <= 9 on a 48 x 48 image; two predictions jittered by sigma 0.6 (one with an extra mid-edge
    vertex), one by sigma 4, none for the fourth gt ring, and a small prediction near no gt ring; the predictions are not in gt order"""
    rng = np.random.default_rng(1000 + seed)
    centres = [(12, 12), (36, 12), (12, 36), (36, 36)]
    gts = [star(rng, cx + rng.uniform(-1, 1), cy + rng.uniform(-1, 1), int(rng.integers(4, 9)), 5.0, 9.0) for cx, cy in centres]
    p0 = f32(gts[0] + rng.normal(0, 0.6, gts[0].shape))
    p1 = gts[1] + rng.normal(0, 0.6, gts[1].shape)
    k = int(rng.integers(0, len(p1)))
    mid = 0.5 * (p1[k] + p1[(k + 1) % len(p1)]) + rng.normal(0, 0.2, 2)
    p1 = f32(np.insert(p1, k + 1, mid, axis=0))
    p2 = f32(gts[2] + rng.normal(0, 4.0, gts[2].shape))
    small = star(rng, 24.3, 23.8, 4, 1.0, 1.8)
    return gts, [small, p1, p0, p2]


def seeded_cases():
    """two calls of three images"""
    out = []
    for name, seeds in (("seeded_012", SEEDS[:3]), ("seeded_345", SEEDS[3:])):
        images = [seeded_image(s) for s in seeds]
        out.append((name, [g for g, _ in images], [d for _, d in images], 48, 48))
    return out


def hand_cases():
    """two calls of three images at 48 x 48: A on itself, A against B, nothing at all; a far-away prediction, a 2-vertex ring beside A and B, A on itself"""
    return [("hand_1", [[SQUARE_A], [SQUARE_A], []], [[SQUARE_A], [SQUARE_B], []], 48, 48),
            ("hand_2", [[SQUARE_A], [TWO, SQUARE_A], [SQUARE_A]], [[FAR], [SQUARE_B, TWO], [SQUARE_A]], 48, 48)]


def circle(cx, cy, r, n, phase):
    a = phase + np.arange(n) * (2 * np.pi / n)
    return f32(np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], axis=1))


def shape_cases():
    tri = f32([(2.3, 3.1), (17.2, 5.4), (9.7, 28.6)])
    tri_p = f32([(2.87, 3.64), (16.63, 5.12), (10.41, 27.93)])
    outside = f32([(-4.2, 10.3), (6.1, 9.7), (5.8, 20.4), (-3.9, 21.2)])          # partly left of the image: the mask clips, the distances do not
    outside_p = f32([(-3.6, 10.9), (6.7, 10.2), (6.3, 21.1), (-3.1, 20.6)])
    repeated = f32([(20.2, 40.3), (28.7, 41.1), (28.7, 41.1), (29.3, 52.6), (19.8, 51.9)])          # an edge of length 0
    repeated_p = f32([(20.9, 40.8), (28.1, 40.6), (29.9, 52.1), (20.3, 52.4)])
    below = f32([(10.3, 55.2), (25.6, 56.1), (24.9, 70.4), (9.8, 69.7)])          # crosses the bottom row of a 64-row image
    below_p = f32([(10.9, 55.8), (25.1, 55.6), (25.4, 69.9), (10.2, 70.3)])
    big = circle(32.2, 31.7, 20.0, 40, 0.13)          # 40 edges: more than one staged chunk; perimeter 125 px: more than one tile of samples
    big_p = circle(32.9, 32.1, 19.4, 37, 0.41)
    g0, d0 = seeded_image(SEEDS[0])
    g1, d1 = seeded_image(SEEDS[1])
    rng = np.random.default_rng(77)
    corner = star(rng, 441.3, 452.6, 7, 40.0, 58.0)          # the last rows of the largest image: both masks fill 64 KB of LDS
    corner_p = f32(corner + rng.normal(0, 0.7, corner.shape))
    small = f32([(1.3, 1.2), (7.6, 2.1), (6.8, 7.7), (2.2, 6.9)])
    small_p = f32([(1.8, 1.7), (7.1, 1.6), (7.4, 7.2), (1.6, 7.3)])
    return [("33x21_one_image", [[tri, outside]], [[outside_p, tri_p]], 33, 21),
            ("odd_word_counts_9x9", [[small]], [[small_p]], 9, 9),          # 81 pixels: 3 mask words, the staged edges lie behind an odd word count
            ("odd_word_counts_30x35", [[tri, f32(small + 20.0)], [tri_p]], [[f32(small_p + 20.0), tri_p], [tri]], 30, 35),          # 1050 pixels: 33 words, two images
            ("odd_word_counts_17x19", [[f32(small + 8.0), small]], [[small_p, f32(small_p + 8.0)]], 17, 19),          # 323 pixels: 11 words
            ("512x512_largest_image", [[tri, corner]], [[corner_p, tri_p]], 512, 512),
            ("64x31", [[tri, repeated, below], [tri]], [[repeated_p, tri_p, below_p], [tri_p]], 64, 31),
            ("long_ring_64x64", [[big, f32(tri + 0.25)], [big_p]], [[big_p], [big]], 64, 64),
            ("gt_only_empty_pred_only", [g0, g1, [], [], g1], [d0, [], [], d0, d1], 48, 48)]


def many_rings_case(seed=304):          # a seed whose margins hold (test_poly_metrics_cpu.py)
    """more rings than one workgroup has threads, in one image and in one call, and more images than the finish kernel has threads: 300 small gt rings on a
    20 x 15 grid of a 90 x 120 image with their predictions in reverse order, 256 empty images, then a seeded image"""
    rng = np.random.default_rng(seed)
    gts, dts = [], []
    for k in range(300):
        cx, cy = 6.0 * (k % 20) + 3.0 + rng.uniform(-0.3, 0.3), 6.0 * (k // 20) + 3.0 + rng.uniform(-0.3, 0.3)
        g = star(rng, cx, cy, int(rng.integers(3, 6)), 1.6, 2.4)
        gts.append(g)
        dts.append(f32(g + rng.normal(0, 0.25 if k % 7 else 1.5, g.shape)))
    g1, d1 = seeded_image(SEEDS[2])
    empty = [[] for _ in range(256)]
    return ("many_rings_many_images", [gts] + empty + [g1], [dts[::-1]] + empty + [d1], 90, 120)


def all_cases():
    return hand_cases() + seeded_cases() + shape_cases() + [many_rings_case()]


def case(name):
    return next(c for c in all_cases() if c[0] == name)
