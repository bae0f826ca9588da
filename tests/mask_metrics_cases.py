"""Inputs shared by test_mask_metrics_cpu.py and test_mask_metrics_gpu.py: the hand cases of DESIGN.md section 24, the seeded images of the polygon metrics
and the shapes at which csrc/mask_metrics.hip takes another path.  A case is (name, gt_batch, dt_batch, H, W, T): per image a list of float32 [n, 2] (x, y)
open rings, T the buffer thickness.  Every coordinate that is not an integer is kept 2e-3 away from the half-integers (`off_half`), but for the case that
is about them."""
import numpy as np

from tests import mta_cases as MC
from tests import poly_metrics_cases as PC

f32 = PC.f32
SQUARE_A, SQUARE_B, FAR, TWO = PC.SQUARE_A, PC.SQUARE_B, PC.FAR, PC.TWO
TRIANGLE = f32([(5, 5), (30, 17), (11, 40)])
POINT = f32([(10, 10)] * 3)                       # three equal vertices: a disc
POINT_AT_ORIGIN = f32([(0, 0)] * 3)               # the disc clipped to a quarter
HALVES = f32([(8.5, 8.5), (9.5, 8.5), (9.5, 9.5)])          # exact in fp32; half to even: (8, 8), (10, 8), (10, 10)
EVENS = f32([(8, 8), (10, 8), (10, 10)])
HUGE = f32([(-30000, -29987), (30000, 30021), (29000, -30000)])          # one edge crosses a 48 x 48 image from far outside
REPEATED = f32([(20, 12), (31, 14), (31, 14), (29, 27), (18, 25)])        # an edge of length 0 between two others
THICKNESSES = (1, 2, 5, 6, 64)
HALF_EVEN_CASE = "half_to_even"


def off_half(ring):
    """the ring with every coordinate within 2e-3 of a half-integer moved up by 0.01"""
    r = np.asarray(ring, dtype=np.float32).copy()
    frac = np.abs(r.astype(np.float64) - np.floor(r.astype(np.float64)) - 0.5)
    with np.errstate(invalid="ignore"):
        r[frac <= 2e-3] += np.float32(0.01)
    return r


def clean(case, T=5):
    name, gt, dt, H, W = case[:5]
    return (name, [[off_half(r) for r in rings] for rings in gt], [[off_half(r) for r in rings] for rings in dt], H, W, T)


def hand_cases():
    return [("hand_shift", [[SQUARE_A]], [[SQUARE_B]], 48, 48, 5),
            ("hand_1", [[SQUARE_A], [SQUARE_A], []], [[SQUARE_A], [SQUARE_B], []], 48, 48, 5),          # the third image is void: all six figures 1.0
            ("points", [[POINT], [POINT_AT_ORIGIN]], [[POINT_AT_ORIGIN], [POINT]], 48, 48, 5),
            (HALF_EVEN_CASE, [[HALVES]], [[EVENS]], 48, 48, 5),
            ("triangle", [[TRIANGLE]], [[f32(TRIANGLE + np.float32([2, -1]))]], 48, 48, 5),
            ("both_empty", [[]], [[]], 48, 48, 5),
            ("gt_empty", [[], []], [[SQUARE_A], [TRIANGLE, FAR]], 48, 48, 5),
            ("dt_empty", [[SQUARE_A], [TRIANGLE, FAR]], [[], []], 48, 48, 5),
            ("prediction_outside", [[SQUARE_A]], [[MC.OUTSIDE]], 48, 48, 5),
            ("huge_ring", [[HUGE, SQUARE_A]], [[SQUARE_B, f32(HUGE + np.float32([3, 0]))]], 48, 48, 5),
            ("repeated_vertex", [[REPEATED]], [[f32(REPEATED + np.float32([1, 2]))]], 48, 48, 5),
            ("invalid_rings", [[SQUARE_A, TWO], [SQUARE_A], []], [[TWO, MC.NAN_RING, SQUARE_B, MC.INF_RING], [SQUARE_A, SQUARE_A], []], 48, 48, 5)]


def seeded_cases(T=5):
    """six seeded images, three per call; image 1 of the first call has no prediction: a subset of 2 of 3"""
    (n0, g0, d0, H, W), second = PC.seeded_cases()
    suffix = "" if T == 5 else f"_T{T}"
    return [clean((n0 + suffix, g0, [d0[0], [], d0[2]], H, W), T), clean((second[0] + suffix,) + second[1:], T)]


def thickness_cases():
    return [("hand_shift_T%d" % T, [[SQUARE_A]], [[SQUARE_B]], 48, 48, T) for T in THICKNESSES if T != 5] + \
           [("triangle_T%d" % T, [[TRIANGLE]], [[f32(TRIANGLE + np.float32([2, -1]))]], 48, 48, T) for T in THICKNESSES if T != 5] + \
           [seeded_cases(T)[0] for T in THICKNESSES if T != 5]


def largest_case():
    """512 x 512: H W = 2^18 exactly, both masks fill 64 KB of LDS; one ring with an edge from corner to corner, one small ring"""
    diag = f32([(0.326, 0.414), (511.226, 510.714), (3.126, 508.814)])          # coordinates at which the pixel-centre margin holds (test_mask_metrics_cpu.py)
    diag_p = f32([(1.413, 0.207), (510.613, 511.307), (2.213, 507.107)])
    small = f32([(400.3, 100.2), (440.6, 104.1), (436.8, 141.7), (402.2, 138.9)])
    small_p = f32([(401.8, 101.7), (439.1, 102.6), (438.4, 140.2), (400.6, 139.3)])
    return clean(("512x512_largest_image", [[diag, small]], [[small_p, diag_p]], 512, 512))


def shape_cases():
    by_name = {c[0]: c for c in PC.shape_cases()}
    return [clean(by_name["33x21_one_image"]), clean(by_name["64x31"]), clean(by_name["odd_word_counts_9x9"]), largest_case(),
            clean(by_name["long_ring_64x64"]),          # 40 edges: more than one staged chunk
            clean(by_name["gt_only_empty_pred_only"]), clean(PC.many_rings_case())]          # 258 images: more than the finish kernel has threads


def all_cases():
    return hand_cases() + seeded_cases() + thickness_cases() + shape_cases()


def case(name):
    return next(c for c in all_cases() if c[0] == name)


def has_fractions(case):
    with np.errstate(invalid="ignore"):
        return any((np.isfinite(r) & (r != np.round(r))).any() for rings in case[1] + case[2] for r in rings)
