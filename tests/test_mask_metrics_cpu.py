"""Mask metrics without a device: the surface of p3_mask_metrics and its argument checks, the workspace layout, the host side of
pixelspointspolygons_amd.eval_metrics.mask_metrics and evaluate, the hand values of the restatement tests/mask_metrics_ref.py, and the margins that make
the bit-for-bit comparisons of test_mask_metrics_gpu.py legitimate: no pixel centre near a crossed edge (the filled masks), no coordinate near a
half-integer (the rounding of the stroke is exact anyway; the margin keeps the inputs from being about it by accident).  The pixel-centre margin is read
with one written exception: the half-to-even case has its vertices on pixel centres by construction, so centres do lie on its crossed edges; all its
coordinates are multiples of 0.5 below 2^10, every product and sum of the crossing rule is then a multiple of 0.25 below 2^22 and exact on either side,
and the sign of an exact zero is read the same way by both."""
import ctypes

import numpy as np
import pytest
import torch

from tests import mask_metrics_cases as C
from tests import mask_metrics_ref as R
from tests import poly_metrics_ref as PR

NAMES = ("metrics", "stats", "image_conf", "image_scores", "image_nr", "image_subset", "invalid_rings", "status")


def _lib():
    from pixelspointspolygons_amd._lib import load
    from pixelspointspolygons_amd.build import build_library
    return load(build_library(verbose=False))


def stroke_px(ring, T=5, H=48, W=48):
    return int(R.stroke_mask([C.f32(ring)], H, W, T).sum())


# ------------------------------------------------------------------------------------------ surface
def test_header_declares_and_library_exports_the_entries():
    from pixelspointspolygons_amd import hip
    from pixelspointspolygons_amd._lib import HEADER, prototypes
    protos = prototypes()
    ret, args = protos["p3_mask_metrics"]
    assert ret is ctypes.c_int and len(args) == 25 and args[10:15] == [ctypes.c_int] * 5 and args[1] is ctypes.c_int64 and args[6] is ctypes.c_int64
    assert protos["p3_mask_metrics_workspace_bytes"] == (ctypes.c_int64, [ctypes.c_int] * 3)
    lib = _lib()
    assert lib.p3_mask_metrics and lib.p3_mask_metrics_workspace_bytes
    header = open(HEADER).read()
    for name, value in (("TOPDIG", 1), ("SUBSET", 2), ("STATS", 4)):
        assert f"#define P3_MM_{name} {value}\n" in header and getattr(hip, "MM_" + name) == value == getattr(R, name)
    assert hip.MM_MAX_THICKNESS == 64 and "buffer_thickness outside [1, 64]" in header


def test_workspace_sizes_are_the_layout():
    from pixelspointspolygons_amd import hip
    lib = _lib()
    up = lambda n: (n + 255) & ~255
    per_set = lambda r: 2 * up(4 * r) + up(8 * r) + up(32 * r)          # state, vertex count, first vertex, box
    for args in ((1, 1, 1), (37, 29, 3), (0, 5, 2), (5, 0, 2), (1280, 1280, 64), (604, 604, 258), (0, 0, 1)):
        want = per_set(args[0]) + per_set(args[1]) + up(32 * args[2])          # and four int64 counts per image
        assert lib.p3_mask_metrics_workspace_bytes(*args) == want == hip.mask_metrics_workspace_bytes(*args), args
    assert lib.p3_mask_metrics_workspace_bytes(1280, 1280, 64) == 124928          # the bench scene: 2 x (5120 + 5120 + 10240 + 40960) + 2048
    assert lib.p3_mask_metrics_workspace_bytes(1, 1, 1) == 2304 and lib.p3_mask_metrics_workspace_bytes(0, 0, 1) == 256
    assert lib.p3_mask_metrics_workspace_bytes(37, 29, 3) == 4352 and lib.p3_mask_metrics_workspace_bytes(604, 604, 258) == 67328
    for args in ((-1, 1, 1), (1, -1, 1), (1, 1, 0), (1, 1, -3)):
        assert lib.p3_mask_metrics_workspace_bytes(*args) == 0, args


def test_entry_validates_before_any_device_work():
    lib = _lib()
    one = ctypes.c_void_p(8)          # a non-null pointer that is never followed: every call below fails its checks first
    sl = np.array([[0, 4]], dtype=np.int64).ctypes.data_as(ctypes.c_void_p)
    im = np.array([0], dtype=np.int32).ctypes.data_as(ctypes.c_void_p)

    def call(Vg=4, Rg=1, Vd=4, Rd=1, B=1, H=8, W=8, T=5, modes=7, gt=(one, sl, im), dt=(one, sl, im), ws=one, **null):
        outs = [None if k in null else one for k in NAMES]
        return lib.p3_mask_metrics(gt[0], Vg, gt[1], gt[2], Rg, dt[0], Vd, dt[1], dt[2], Rd, B, H, W, T, modes, *outs, ws, None)

    err = lambda: lib.p3_last_error_string()
    assert call(Vg=-1) == -1 and b"p3_mask_metrics" in err() and b"negative" in err()
    assert call(Rg=-1) == -1 and call(Vd=-1) == -1 and call(Rd=-1) == -1
    for kw in (dict(B=0), dict(H=0), dict(W=0), dict(B=-2)):
        assert call(**kw) == -1 and b"p3_mask_metrics" in err() and b"bad sizes" in err(), kw
    assert call(H=513, W=512) == -1 and b"p3_mask_metrics" in err() and b"2^18" in err()
    for T in (0, 65, -1, 1 << 20):
        assert call(T=T) == -1 and b"p3_mask_metrics" in err() and b"buffer_thickness" in err(), T
    for modes in (0, 8, 15, -1):
        assert call(modes=modes) == -1 and b"p3_mask_metrics" in err() and b"modes" in err(), modes
    for k in NAMES:
        assert call(**{k: True}) == -1 and b"p3_mask_metrics" in err() and b"null pointer" in err() and k.encode() in err(), k
    for kw in (dict(gt=(None, sl, im)), dict(gt=(one, None, im)), dict(gt=(one, sl, None)), dict(dt=(None, sl, im)), dict(dt=(one, None, im)),
               dict(dt=(one, sl, None))):
        assert call(**kw) == -1 and b"p3_mask_metrics" in err() and b"null pointer" in err(), kw
    assert call() == -1 and b"p3_mask_metrics" in err() and b"device memory" in err()          # well-formed, but host index arrays
    for kw in (dict(T=1), dict(T=64), dict(modes=1), dict(modes=2), dict(modes=4), dict(H=512, W=512)):          # the ends of the ranges pass the parameter checks
        assert call(**kw) == -1 and b"device memory" in err(), kw
    assert call(Rg=0, gt=(None, None, None)) == -1 and b"device memory" in err()          # an empty set needs none of its pointers
    assert call(Rg=0, gt=(None, None, None), Rd=0, dt=(None, None, None), ws=None) == -1 and b"null workspace" in err()          # the workspace is looked at last
    assert call(ws=None) == -1 and b"device memory" in err()


def test_host_tensors_are_refused():
    from pixelspointspolygons_amd import eval_metrics as E, hip
    rings = E.pack_rings([[C.SQUARE_A]], "cpu", scores=[[0.5]], areas=[[256.0]])
    with pytest.raises(hip.P3Error, match="device tensors"):
        E.mask_metrics(rings, rings, 48, 48)
    with pytest.raises(hip.P3Error, match="device tensors"):
        hip.mask_metrics_device(rings["pos"], rings["ring_slice"], rings["ring_image"], rings["pos"], rings["ring_slice"], rings["ring_image"], 1, 48, 48)
    with pytest.raises(hip.P3Error, match="device tensors"):
        E.evaluate(rings, rings, 48, 48, ["topdig"])
    with pytest.raises(hip.P3Error, match="device tensors"):
        E.evaluate(rings, rings, 48, 48, ["iou", "stats", "mta", "coco"])
    with pytest.raises(hip.P3Error, match="mask_metrics.*ring set"):
        E.mask_metrics({"pos": rings["pos"]}, rings, 48, 48)


def test_wrappers_refuse_wrong_shapes_types_parameters_and_modes_before_any_launch(monkeypatch):
    from pixelspointspolygons_amd import eval_metrics as E, hip
    monkeypatch.setattr(hip, "_dev", lambda t: None)          # the shape checks come right behind the device check
    r = E.pack_rings([[C.SQUARE_A]], "cpu")
    pos, sl, im = r["pos"], r["ring_slice"], r["ring_image"]
    for bad in ((pos.double(), sl, im), (torch.zeros(4, 3), sl, im), (pos, sl.float(), im), (pos, sl[:, :1], im), (pos, sl, im.float()), (pos, sl, im[:0])):
        with pytest.raises(hip.P3Error, match="mask_metrics"):
            hip.mask_metrics_device(*bad, pos, sl, im, 1, 48, 48)
        with pytest.raises(hip.P3Error, match="mask_metrics"):
            hip.mask_metrics_device(pos, sl, im, *bad, 1, 48, 48)
    for B, H, W in ((0, 48, 48), (1, 0, 48), (1, 48, 0), (1, 513, 512)):
        with pytest.raises(hip.P3Error, match="height"):
            hip.mask_metrics_device(pos, sl, im, pos, sl, im, B, H, W)
    for T in (0, 65, -3):
        with pytest.raises(hip.P3Error, match="buffer_thickness"):
            hip.mask_metrics_device(pos, sl, im, pos, sl, im, 1, 48, 48, buffer_thickness=T)
        with pytest.raises(hip.P3Error, match="buffer_thickness"):
            E.mask_metrics(r, r, 48, 48, buffer_thickness=T)
    for modes in (0, 8, 9, -1):
        with pytest.raises(hip.P3Error, match="modes"):
            hip.mask_metrics_device(pos, sl, im, pos, sl, im, 1, 48, 48, modes=modes)
    for modes in (("topdig", "iou"), ("mta",), ("ldof",), ()):
        with pytest.raises(hip.P3Error, match="mask_metrics.*modes are"):
            E.mask_metrics(r, r, 48, 48, modes=modes)
    with pytest.raises(hip.P3Error, match="images"):
        E.mask_metrics(r, E.pack_rings([[], []], "cpu"), 48, 48)
    with pytest.raises(hip.P3Error, match="ldof.*external executable"):
        E.evaluate(r, r, 48, 48, modes=["ldof"])
    with pytest.raises(hip.P3Error, match="ldof.*external executable"):
        E.evaluate(r, r, 48, 48, modes=["iou", "ldof", "topdig"])
    for modes in (["iou", "lidar"], ["segm"], ["IoU"]):
        with pytest.raises(hip.P3Error, match="evaluate: unknown mode.*'iou'.*'boundary-coco'"):
            E.evaluate(r, r, 48, 48, modes=modes)
    with pytest.raises(hip.P3Error, match="evaluate: modes is empty"):
        E.evaluate(r, r, 48, 48, modes=[])
    assert set(E.EVALUATE_MODES) == set(E.MODES) | set(E.MASK_MODES) | {"mta", "coco", "boundary-coco", "ldof"}


# ------------------------------------------------------------------------------------------ hand values of the restatement
def test_the_stroke_of_a_square_by_thickness():
    assert stroke_px(C.SQUARE_A) == 316          # the square band of 320 (21 x 21 minus 11 x 11) without one pixel at each outer corner
    assert [stroke_px(C.SQUARE_A, T) for T in (1, 2, 3, 4)] == [64, 188, 192, 308]
    m = R.stroke_mask([C.SQUARE_A], 48, 48, 5)
    band = np.zeros((48, 48), bool)
    band[6:27, 6:27] = True
    band[11:22, 11:22] = False
    band[[6, 6, 26, 26], [6, 26, 6, 26]] = False
    assert np.array_equal(m, band)


def test_a_shifted_square_filled_and_stroked():
    o = R.run([[C.SQUARE_A]], [[C.SQUARE_B]], 48, 48)
    assert o["image_conf"].tolist() == [[[208, 48, 48, 2000], [220, 96, 96, 1892]]]
    iou, acc, f1, iou_t, acc_t, f1_t = o["image_scores"][0].tolist()
    assert acc == 2208 / 2304 and abs(acc - 0.958333333333) < 1e-11 and f1 == 0.8125 and iou == 208 / (304 + 1e-9)
    assert acc_t == 2112 / 2304 and abs(acc_t - 0.916666666667) < 1e-11 and f1_t == 440 / 632 and iou_t == 220 / (412 + 1e-9)
    assert o["metrics"][:6].tolist() == o["image_scores"][0].tolist()          # B = 1: the means are the figures
    assert o["metrics"][6:].tolist() == [iou, iou, 1.0] and o["image_subset"].tolist() == [1] and o["image_nr"].tolist() == [1.0]
    assert o["stats"].tolist() == [1, 1, 1, 1, 1, 4, 4] and o["status"].tolist() == [0]


def test_points_clipping_rounding_and_a_triangle():
    assert stroke_px(C.POINT) == 21 and stroke_px(C.POINT_AT_ORIGIN) == 8
    assert stroke_px(C.HALVES) == stroke_px(C.EVENS) == 40
    assert np.array_equal(R.stroke_mask([C.HALVES], 48, 48, 5), R.stroke_mask([C.EVENS], 48, 48, 5))
    assert R.ring_points(C.HALVES).tolist() == [[8, 8], [10, 8], [10, 10]] and R.ring_points(C.f32([(0.5, 1.5), (2.5, -0.5), (-1.5, 3.5)])).tolist() == [[0, 2], [2, 0], [-2, 4]]
    assert stroke_px(C.TRIANGLE) == 452


def test_the_stroke_against_distances_in_floating_point():
    """an independent statement of the band: the distance of the pixel to the segment, in doubles, compared with T / 2 - away from the boundary"""
    rng = np.random.default_rng(5)
    for T in (1, 2, 5, 6):
        for _ in range(6):
            a, b = rng.integers(-10, 58, 2), rng.integers(-10, 58, 2)
            m = np.zeros((48, 48), bool)
            R.stroke_edge(m, a, b, T)
            py, px = np.mgrid[0:48, 0:48].astype(np.float64)
            d = (b - a).astype(np.float64)
            L2 = float(d @ d)
            t = np.clip(((px - a[0]) * d[0] + (py - a[1]) * d[1]) / L2, 0.0, 1.0) if L2 > 0 else np.zeros_like(px)
            dist = np.hypot(px - (a[0] + t * d[0]), py - (a[1] + t * d[1]))
            assert m[dist < T / 2 - 1e-9].all() and not m[dist > T / 2 + 1e-9].any(), (T, a, b)


def test_void_images_empty_sets_and_the_subset():
    o = R.run([[]], [[]], 48, 48)
    assert o["metrics"][:6].tolist() == [1.0] * 6 and np.isnan(o["metrics"][6:]).all() and o["stats"].tolist() == [1, 0, 0, 0, 0, 0, 0]
    assert o["image_conf"].tolist() == [[[0, 0, 0, 2304]] * 2] and o["image_subset"].tolist() == [0]
    _, gt, dt, H, W, T = C.case("gt_empty")
    o = R.run(gt, dt, H, W, T)
    assert (o["image_conf"][:, :, [0, 2]] == 0).all() and (o["image_conf"][:, :, 1] > 0).all() and o["metrics"][[0, 2, 3, 5]].tolist() == [0.0] * 4
    assert o["image_subset"].tolist() == [1, 1] and o["metrics"][6:8].tolist() == [0.0, 0.0] and 0.0 < o["metrics"][8] < 1e-9 and o["stats"].tolist() == [2, 0, 2, 0, 3, 0, 11]
    _, gt, dt, H, W, T = C.case("dt_empty")
    o = R.run(gt, dt, H, W, T)
    assert (o["image_conf"][:, :, [0, 1]] == 0).all() and (o["image_conf"][:, :, 2] > 0).all() and np.isnan(o["metrics"][6:]).all()
    _, gt, dt, H, W, T = C.case("seeded_012")
    o = R.run(gt, dt, H, W, T)
    assert o["image_subset"].tolist() == [1, 0, 1]
    iou = [R.scores(o["image_conf"][b, 0], H * W)[0] for b in range(3)]
    assert o["metrics"][6] == (iou[0] + iou[2]) / 2 and o["metrics"][8] == (o["image_nr"][0] + o["image_nr"][2]) / 2
    assert o["metrics"][0] == (iou[0] + iou[1] + iou[2]) / 3
    _, gt, dt, H, W, T = C.case("invalid_rings")
    o = R.run(gt, dt, H, W, T)
    assert o["status"].tolist() == [1] and o["invalid_rings"].tolist() == [[1, 3], [0, 0], [0, 0]] and o["stats"].tolist() == [3, 2, 2, 3, 6, 10, 20]


def test_a_mode_that_is_off_leaves_nan_and_zero():
    _, gt, dt, H, W, T = C.case("hand_1")
    full = R.run(gt, dt, H, W, T)
    o = R.run(gt, dt, H, W, T, modes=R.SUBSET)
    assert np.isnan(o["metrics"][:6]).all() and np.isnan(o["image_scores"]).all() and not o["image_conf"][:, 1].any() and not o["stats"].any()
    assert np.array_equal(o["image_conf"][:, 0], full["image_conf"][:, 0]) and np.array_equal(o["metrics"][6:], full["metrics"][6:])
    o = R.run(gt, dt, H, W, T, modes=R.STATS)
    assert np.isnan(o["metrics"]).all() and np.isnan(o["image_nr"]).all() and not o["image_conf"].any() and not o["image_subset"].any()
    assert np.array_equal(o["stats"], full["stats"]) and o["stats"].tolist() == [3, 2, 2, 2, 2, 8, 8]
    o = R.run(gt, dt, H, W, T, modes=R.TOPDIG)
    assert np.isnan(o["metrics"][6:]).all() and np.array_equal(o["image_conf"], full["image_conf"]) and np.array_equal(o["metrics"][:6], full["metrics"][:6])


# ------------------------------------------------------------------------------------------ the inputs of the GPU test are unambiguous
@pytest.mark.parametrize("case", [c for c in C.all_cases() if C.has_fractions(c)], ids=lambda c: c[0])
def test_gpu_inputs_with_fractions_keep_their_margins(case):
    name, gt, dt, H, W, T = case
    if name == C.HALF_EVEN_CASE:          # the written exception: exact operands in place of the margin, and half-integers on purpose
        for r in gt[0] + dt[0]:
            assert np.array_equal(r * 2, np.round(r * 2)) and np.abs(r).max() < 1024 and r.dtype == np.float32
        assert any((r != np.round(r)).any() for r in gt[0] + dt[0])
        return
    near, _, _ = PR.margins(gt, dt, H, W)
    assert near == 0, near          # no pixel centre within 1e-4 |edge| of a crossed edge: the filled counts are equal
    for rings in gt + dt:
        for r in rings:
            v = r.astype(np.float64)
            v = v[np.isfinite(v)]
            assert (np.abs(v - np.floor(v) - 0.5) > 1e-3).all(), (name, r.tolist())


def test_the_cases_reach_what_they_are_named_for():
    from pixelspointspolygons_amd import hip
    assert C.has_fractions(C.case(C.HALF_EVEN_CASE)) and not C.has_fractions(C.case("hand_shift")) and not C.has_fractions(C.case("invalid_rings"))
    _, gt, dt, H, W, T = C.case("512x512_largest_image")
    assert H * W == hip.PM_MAX_HW and max(np.ptp(r, axis=0).min() for r in gt[0]) > 500          # an edge from corner to corner
    _, gt, dt, H, W, T = C.case("huge_ring")
    o = R.run(gt, dt, H, W, T)
    assert o["status"].tolist() == [0] and 0 < o["image_conf"][0, 1, 0] < H * W and np.abs(gt[0][0]).min() >= 29000
    _, gt, dt, H, W, T = C.case("many_rings_many_images")
    assert len(gt) > 256 and len(gt[0]) > 256
    _, gt, dt, H, W, T = C.case("long_ring_64x64")
    assert len(gt[0][0]) > hip.PM_EDGE_CHUNK
    for name in ("33x21_one_image", "64x31"):
        assert C.case(name)[4] % 32 != 0
    assert sorted({c[5] for c in C.all_cases()}) == sorted(C.THICKNESSES)
