"""Inputs shared by test_mta_cpu.py and test_mta_gpu.py: the hand cases of DESIGN.md section 23, the seeded images of the polygon metrics and the shapes at
which csrc/mta_metrics.hip takes another path.  A case is (name, gt_batch, dt_batch, H, W, params): per image a list of float32 [n, 2] (x, y) open rings;
params holds the keywords that differ from the reference's (sampling_spacing 2.0, min_precision 0.5, max_stretch 2.0)."""
import numpy as np

from tests import poly_metrics_cases as PC

f32 = PC.f32
SQUARE_A, SQUARE_B, FAR, TWO = PC.SQUARE_A, PC.SQUARE_B, PC.FAR, PC.TWO
SLANTED = f32([(8, 8), (24, 10), (24, 24), (8, 24)])          # A with one corner moved: the top edge turns by atan(1 / 8)
OUTSIDE = f32([(60, 60), (70, 60), (70, 70), (60, 70)])       # no pixel of a 48 x 48 image
NAN_RING = f32([(10, 10), (20, np.nan), (20, 20)])
INF_RING = f32([(10, 10), (np.inf, 10), (20, 20)])
DIAMOND = f32([(24.3, 4.1), (44.2, 24.4), (23.8, 43.9), (4.4, 23.7)])
IN_DIAMOND = f32([(18.2, 17.4), (29.9, 17.1), (30.4, 30.2), (17.7, 30.8)])          # every edge projects onto the diamond at a stretch near sqrt(2) or across a corner


def hand_cases():
    """calls of three images at 48 x 48"""
    return [("hand_1", [[SQUARE_A], [SQUARE_A], [SQUARE_A]], [[SQUARE_A], [SQUARE_B], [SLANTED]], 48, 48, {}),
            ("hand_2", [[SQUARE_A], [], [SQUARE_A]], [[FAR], [SQUARE_A], [OUTSIDE]], 48, 48, {}),          # far away, no gt, outside the image
            ("hand_3", [[SQUARE_A, TWO], [SQUARE_A], []], [[TWO, NAN_RING, SQUARE_B, INF_RING], [SQUARE_A, SQUARE_A], []], 48, 48, {}),
            ("hand_empty", [[]], [[]], 48, 48, {}),
            ("hand_1_precision_0.9", [[SQUARE_A], [SQUARE_A], [SQUARE_A]], [[SQUARE_A], [SQUARE_B], [SLANTED]], 48, 48, {"min_precision": 0.9}),
            ("hand_1_spacing_0.5", [[SQUARE_A], [SQUARE_A], [SQUARE_A]], [[SQUARE_A], [SQUARE_B], [SLANTED]], 48, 48, {"sampling_spacing": 0.5}),
            ("no_valid_edge_stretch_1.2", [[DIAMOND], [SQUARE_A]], [[IN_DIAMOND], [SLANTED]], 48, 48, {"max_stretch": 1.2}),
            ("hand_1_stretch_4", [[SQUARE_A], [SQUARE_A], [SQUARE_A]], [[SQUARE_A], [SQUARE_B], [SLANTED]], 48, 48, {"max_stretch": 4.0})]


def seeded_cases():
    """six seeded images, three per call"""
    return [c + ({},) for c in PC.seeded_cases()]


def chunk_case():
    """224 x 224: 40 + 24 + 3 gt edges, so that the first boundary between two staged chunks of 32 falls inside the first ring and the second between
    the second and the third ring; the prediction of 37 vertices (two chunks of its own edges) has more than 300 samples: two tiles"""
    big = PC.circle(112.3, 111.6, 100.0, 40, 0.13)
    inner = PC.circle(110.7, 113.2, 40.0, 24, 0.29)
    tri = f32([(3.3, 3.1), (17.2, 5.4), (9.7, 18.6)])
    big_p = PC.circle(112.9, 112.2, 99.1, 37, 0.43)
    inner_p = PC.circle(111.2, 112.6, 39.2, 9, 0.07)
    return ("chunks_224x224", [[big, inner, tri]], [[inner_p, big_p]], 224, 224, {})


def shape_cases():
    by_name = {c[0]: c for c in PC.shape_cases()}
    take = lambda name, **params: by_name[name] + (params,)
    name, gt, dt, H, W = by_name["long_ring_64x64"]
    repeated = f32([(20.2, 40.3), (28.7, 41.1), (28.7, 41.1), (29.3, 52.6), (19.8, 51.9)])          # a prediction with an edge of length 0: m = 1, a doubled sample, |u| = 0
    repeated_g = f32([(20.9, 40.8), (28.1, 40.6), (29.9, 52.1), (20.3, 52.4)])
    return [("repeated_vertex_in_a_prediction_64x31", [[repeated_g]], [[repeated]], 64, 31, {}), take("33x21_one_image"), take("odd_word_counts_9x9"), take("512x512_largest_image"), take("64x31"),          # 64x31: a repeated vertex, rings partly outside
            take("long_ring_64x64"), (name + "_spacing_0.25", gt, dt, H, W, {"sampling_spacing": 0.25}), chunk_case(),
            take("gt_only_empty_pred_only")]


def many_rings_case():
    return PC.many_rings_case() + ({},)


# images that hold no counted ring on purpose, by case
EMPTY_IMAGES = {"hand_2": {0, 1, 2}, "hand_3": {2}, "hand_empty": {0}, "hand_1_precision_0.9": {1}, "no_valid_edge_stretch_1.2": {0}, "gt_only_empty_pred_only": {1, 2, 3},
                "many_rings_many_images": set(range(1, 257))}


def ref_params(params):
    """the keywords of a case as mta_ref.run and mta_ref.margins name them"""
    return {{"sampling_spacing": "spacing"}.get(k, k): v for k, v in params.items()}


def all_cases():
    return hand_cases() + seeded_cases() + shape_cases() + [many_rings_case()]


def case(name):
    return next(c for c in all_cases() if c[0] == name)
