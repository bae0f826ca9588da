"""Inputs shared by test_coco_metrics_cpu.py and test_coco_metrics_gpu.py: the hand cases of DESIGN.md section 22, the seeded images and the shapes at which
csrc/coco_metrics.hip takes another path.  A case is (name, gt_batch, dt_batch, H, W, scores, areas): per image a list of float32 [n, 2] (x, y) open rings;
scores (per image a list, one per prediction) and areas (per image a list, one per gt ring) may be None."""
import numpy as np

from tests.poly_metrics_cases import FAR, SEEDS, SQUARE_A, SQUARE_B, TWO, f32, seeded_image, shape_cases, star


def rect(x0, y0, x1, y1):
    return f32([(x0, y0), (x1, y0), (x1, y1), (x0, y1)])


HALF = rect(8, 8, 24, 16)            # on SQUARE_A: I = 128, U = 256
THREE_QUARTERS = rect(8, 8, 24, 20)  # on SQUARE_A: I = 192, U = 256


def hand_cases():
    """48 x 48, d = 1"""
    return [("square_on_itself", [[SQUARE_A]], [[SQUARE_A]], 48, 48, None, None),
            ("square_shifted", [[SQUARE_A]], [[SQUARE_B]], 48, 48, None, None),
            ("iou_exactly_half", [[SQUARE_A]], [[HALF]], 48, 48, None, None),
            ("iou_exactly_three_quarters", [[SQUARE_A]], [[THREE_QUARTERS]], 48, 48, None, None),
            ("two_predictions_one_gt", [[SQUARE_A]], [[SQUARE_A, SQUARE_A]], 48, 48, [[1.0, 1.0]], None),
            ("greedy_keeps_the_earlier", [[SQUARE_A]], [[SQUARE_B, SQUARE_A]], 48, 48, None, None)]


def scores_for(seed, dts):
    """one score per prediction, a multiple of 1/8 in [1/8, 1]: ties are likely"""
    rng = np.random.default_rng(5000 + seed)
    return [float(v) / 8.0 for v in rng.integers(1, 9, len(dts))]


def seeded_cases():
    """six seeded images in two calls of three; the first image of the first call is empty on both sides, the middle one of the second has gt rings only and
    its last one predictions only"""
    images = [seeded_image(s) for s in SEEDS]
    sc = [scores_for(s, d) for s, (_, d) in zip(SEEDS, images)]
    first = ("seeded_empty_01", [[], images[0][0], images[1][0]], [[], images[0][1], images[1][1]], 48, 48, [[], sc[0], sc[1]], None)
    second = ("seeded_2_gt_only_pred_only", [images[2][0], images[3][0], []], [images[2][1], [], images[4][1]], 48, 48, [sc[2], [], sc[4]], None)
    return [first, second]


def edge_cases():
    by_name = {c[0]: c for c in shape_cases()}
    _, g33, d33, H33, W33 = by_name["33x21_one_image"]          # a triangle and a ring partly left of the image; words straddle nothing here: one word per row
    _, g64, d64, H64, W64 = by_name["64x31"]                    # a repeated vertex, a ring that crosses the bottom row
    rng = np.random.default_rng(91)
    wide = rect(20, 5, 81, 30)                # columns 20 .. 80: words 0, 1 and 2
    wide_p = rect(22, 6, 83, 29)
    inside = rect(34, 32, 44, 38)             # columns 34 .. 43: word 1 alone
    inside_p = rect(35, 32, 45, 39)
    thin = rect(88, 4, 91, 36)                # 3 wide with d = 2: nothing survives the erosion, the boundary is the mask
    thin_p = rect(89, 5, 92, 35)
    corner = rect(0, 0, 12, 9)                # touches two image edges: the boundary stays on them
    corner_p = rect(0, 0, 11, 10)
    outside = rect(-5, 20, 8, 33)             # partly left of the image
    outside_p = rect(-4, 21, 9, 34)
    slanted = star(rng, 60.4, 20.7, 7, 6.0, 11.0)          # crosses the word boundary at column 64 with oblique edges
    slanted_p = f32(slanted + rng.normal(0, 0.5, slanted.shape))
    gt96 = [wide, inside, thin, corner, outside, slanted]
    dt96 = [corner_p, slanted_p, wide_p, outside_p, thin_p, inside_p]
    return [("33x21_one_image", g33, d33, H33, W33, [[0.5, 0.9]], None),
            ("64x31", g64, d64, H64, W64, [[0.9, 0.9, 0.3], [0.7]], None),
            ("words_40x96", [gt96], [dt96], 40, 96, [[0.9, 0.8, 0.7, 0.6, 0.5, 0.4]], None)]


def five_rings_224():
    """224 x 224, d = 6: five rings per side, one above 9 216 pixels, one below 1 024, three between: all four buckets are live"""
    rng = np.random.default_rng(224)
    gts = [rect(10, 10, 112, 112), rect(130, 20, 150, 40), rect(130, 60, 180, 100), rect(20, 130, 70, 180)]
    gts.append(star(rng, 160.3, 160.8, 8, 30.0, 44.0))
    dts = [rect(12, 13, 115, 110), rect(131, 22, 152, 41), rect(150, 70, 200, 110), star(rng, 40.2, 150.3, 6, 20.0, 30.0),
           f32(gts[4] + rng.normal(0, 1.5, gts[4].shape))]
    return ("five_rings_224", [gts], [[dts[3], dts[0], dts[4], dts[2], dts[1]]], 224, 224, [[0.9, 0.8, 0.8, 0.4, 0.95]], None)


def many_predictions(n_gt):
    """103 predictions of 3 x 3 pixels on a grid of a 48 x 48 image with scores that are multiples of 1/16 (many ties) and a few distinct ones, on n_gt gt rings:
    the cut behind the first 100, dt_rank = -1; with 11 gt rings the image's pair IoUs no longer fit the match kernel's LDS stage"""
    rng = np.random.default_rng(103)
    dts = [rect(1 + 4 * (k % 11) + 0.25, 1 + 4 * (k // 11) + 0.25, 4 + 4 * (k % 11) + 0.25, 4 + 4 * (k // 11) + 0.25) for k in range(103)]
    scores = [float(v) / 16.0 for v in rng.integers(1, 17, 103)]
    for k in (5, 40, 77):
        scores[k] = 0.03 * (k + 1) / 3.0
    gts = [f32(dts[9 * i + 3] + np.float32([i % 2, 0])) for i in range(n_gt)]          # on a prediction (IoU 1), or one pixel beside it (IoU 6 / 12)
    return (f"predictions_103_gt_{n_gt}", [gts], [dts], 48, 48, [scores], None)


def many_images():
    """40 images of 24 x 24 with 4 gt rings and 8 predictions each: 160 + 320 rings, so the ring and order kernels run a second workgroup, and 320 predictions
    in one precision series, more than the 256 the series kernel's scans take at a time"""
    rng = np.random.default_rng(4045)          # a seed whose margins hold (test_coco_metrics_cpu.py)
    gts, dts, scores = [], [], []
    for _ in range(40):
        g = [star(rng, cx + rng.uniform(-1, 1), cy + rng.uniform(-1, 1), int(rng.integers(4, 7)), 2.5, 4.5) for cx, cy in ((6, 6), (18, 6), (6, 18), (18, 18))]
        d = [f32(r + rng.normal(0, 0.15 + 0.35 * k, r.shape)) for k, r in enumerate(g)] + [star(rng, rng.uniform(4, 20), rng.uniform(4, 20), 4, 1.0, 2.0) for _ in range(4)]
        perm = rng.permutation(8)
        gts.append(g)
        dts.append([d[i] for i in perm])
        scores.append([float(v) / 32.0 for v in rng.integers(1, 33, 8)])
    return ("images_40_of_24x24", gts, dts, 24, 24, scores, None)


def largest_image():
    """512 x 512, d = 14: 16 words per row, a ring that crosses seven of them beside the last rows and columns of the image"""
    rng = np.random.default_rng(512)
    corner = star(rng, 441.3, 452.6, 7, 40.0, 58.0)
    corner_p = f32(corner + rng.normal(0, 3.0, corner.shape))
    small = star(rng, 100.4, 90.2, 5, 9.0, 13.0)          # thinner than 2 d + 1 = 29 nearly everywhere
    small_p = f32(small + rng.normal(0, 0.8, small.shape))
    return ("largest_image_512", [[small, corner]], [[corner_p, small_p]], 512, 512, [[0.5, 0.75]], None)


def area_case():
    """the gt ring of 256 pixels is pushed into the medium bucket by its annotation area alone; the second one stays small"""
    return ("area_given", [[SQUARE_A, FAR]], [[SQUARE_B, FAR]], 48, 48, [[0.6, 0.9]], [[2000.0, 36.0]])


def invalid_case():
    """an invalid ring on each side and a prediction whose score is NaN"""
    return ("invalid_rings", [[TWO, SQUARE_A]], [[SQUARE_B, TWO, SQUARE_A, FAR]], 48, 48, [[0.9, 0.8, float("nan"), 0.2]], None)


def all_cases():
    return hand_cases() + seeded_cases() + edge_cases() + [five_rings_224(), many_predictions(3), many_predictions(11), many_images(), largest_image(), area_case(),
                                                         invalid_case()]


def case(name):
    return next(c for c in all_cases() if c[0] == name)
