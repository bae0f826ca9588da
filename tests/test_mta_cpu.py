"""Max tangent angle error without a device: the surface of p3_max_tangent_angle and its argument checks, the workspace layout, the
host side of pixelspointspolygons_amd.eval_metrics.max_tangent_angle, the hand values of the restatement tests/mta_ref.py, and the margins that make the
exact comparisons of test_mta_gpu.py legitimate.  One margin is read with a written exception: a tie between two nearest points whose squared distances
are equal is accepted when the sample, the gt edge ends and both points are multiples of 1 / 64: the arithmetic is then exact on either side (the shifted
square sampled at 0.5 has two such samples: (11, 11) and (11, 21) lie 3 from two edges of A), so the order of the edges decides it, not a rounding."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import mta_cases as C
from tests import mta_ref as R


def _lib():
    from pixelspointspolygons_amd._lib import load
    from pixelspointspolygons_amd.build import build_library
    return load(build_library(verbose=False))


def ref(name):
    _, gt, dt, H, W, params = C.case(name)
    return R.run(gt, dt, H, W, **C.ref_params(params))


# ------------------------------------------------------------------------------------------ surface
def test_header_declares_and_library_exports_the_entries():
    from pixelspointspolygons_amd._lib import prototypes
    protos = prototypes()
    ret, args = protos["p3_max_tangent_angle"]
    assert ret is ctypes.c_int and len(args) == 27 and args[13:16] == [ctypes.c_double] * 3 and args[1] is ctypes.c_int64 and args[10:13] == [ctypes.c_int] * 3
    assert protos["p3_max_tangent_angle_workspace_bytes"] == (ctypes.c_int64, [ctypes.c_int] * 3)
    lib = _lib()
    assert lib.p3_max_tangent_angle and lib.p3_max_tangent_angle_workspace_bytes
    header = open(__import__("pixelspointspolygons_amd._lib", fromlist=["HEADER"]).HEADER).read()
    from pixelspointspolygons_amd import hip
    for name, value in (("COUNTED", 0), ("INVALID", 1), ("EMPTY", 2), ("BELOW_PRECISION", 3), ("NO_EDGE", 4)):
        assert f"#define P3_MTA_{name} {value}\n" in header and getattr(hip, "MTA_" + name) == value == getattr(R, name)


def test_workspace_sizes_are_the_layout():
    from pixelspointspolygons_amd import hip
    lib = _lib()
    up = lambda n: (n + 255) & ~255
    per_set = lambda r: 2 * up(4 * r) + up(8 * r) + up(32 * r)          # state, vertex count, first vertex, box
    for args in ((1, 1, 1), (37, 29, 3), (0, 5, 2), (5, 0, 2), (1280, 1280, 64), (604, 604, 258)):
        assert lib.p3_max_tangent_angle_workspace_bytes(*args) == per_set(args[0]) + per_set(args[1]) == hip.max_tangent_angle_workspace_bytes(*args), args
    assert lib.p3_max_tangent_angle_workspace_bytes(1280, 1280, 64) == 122880          # the bench scene: 2 x (5120 + 5120 + 10240 + 40960)
    assert lib.p3_max_tangent_angle_workspace_bytes(1, 1, 1) == 2048 and lib.p3_max_tangent_angle_workspace_bytes(0, 0, 1) == 0
    for args in ((-1, 1, 1), (1, -1, 1), (1, 1, 0), (1, 1, -3)):
        assert lib.p3_max_tangent_angle_workspace_bytes(*args) == 0, args


def test_entry_validates_before_any_device_work():
    lib = _lib()
    one = ctypes.c_void_p(8)          # a non-null pointer that is never followed: every call below fails its checks first
    sl = np.array([[0, 4]], dtype=np.int64).ctypes.data_as(ctypes.c_void_p)
    im = np.array([0], dtype=np.int32).ctypes.data_as(ctypes.c_void_p)
    names = ("mta", "counted", "ring_angle", "ring_cos", "ring_state", "ring_px", "image_overlap_px", "invalid_rings", "status")

    def call(Vg=4, Rg=1, Vd=4, Rd=1, B=1, H=8, W=8, spacing=2.0, precision=0.5, stretch=2.0, gt=(one, sl, im), dt=(one, sl, im), ws=one, **null):
        outs = [None if k in null else one for k in names]
        return lib.p3_max_tangent_angle(gt[0], Vg, gt[1], gt[2], Rg, dt[0], Vd, dt[1], dt[2], Rd, B, H, W, spacing, precision, stretch, *outs, ws, None)

    err = lambda: lib.p3_last_error_string()
    assert call(Vg=-1) == -1 and b"p3_max_tangent_angle" in err() and b"negative" in err()
    assert call(Rg=-1) == -1 and call(Vd=-1) == -1 and call(Rd=-1) == -1
    for kw in (dict(B=0), dict(H=0), dict(W=0)):
        assert call(**kw) == -1 and b"p3_max_tangent_angle" in err() and b"bad sizes" in err(), kw
    assert call(H=513, W=512) == -1 and b"p3_max_tangent_angle" in err() and b"2^18" in err()
    for v in (0.0, -1.0, math.inf, -math.inf, math.nan, 1.0 / 128, 1e-6):          # below 1 / 64 a ring's samples would not be bounded
        assert call(spacing=v) == -1 and b"p3_max_tangent_angle" in err() and b"sampling_spacing" in err(), v
    for v in (-0.1, 1.0, 1.5, math.inf, math.nan):
        assert call(precision=v) == -1 and b"p3_max_tangent_angle" in err() and b"min_precision" in err(), v
    for v in (1.0, 0.5, -2.0, math.inf, math.nan):
        assert call(stretch=v) == -1 and b"p3_max_tangent_angle" in err() and b"max_stretch" in err(), v
    for k in names:
        assert call(**{k: True}) == -1 and b"p3_max_tangent_angle" in err() and b"null pointer" in err() and k.encode() in err(), k
    for kw in (dict(gt=(None, sl, im)), dict(gt=(one, None, im)), dict(gt=(one, sl, None)), dict(dt=(None, sl, im)), dict(dt=(one, None, im)),
               dict(dt=(one, sl, None))):
        assert call(**kw) == -1 and b"p3_max_tangent_angle" in err() and b"null pointer" in err(), kw
    assert call() == -1 and b"p3_max_tangent_angle" in err() and b"device memory" in err()          # well-formed, but host index arrays
    assert call(precision=0.0, spacing=1.0 / 64, stretch=1.0000001) == -1 and b"device memory" in err()          # the ends of the ranges pass the parameter checks
    assert call(Rg=0, gt=(None, None, None)) == -1 and b"device memory" in err()          # an empty gt set needs none of its pointers
    per_ring = dict(ring_angle=True, ring_cos=True, ring_state=True, ring_px=True)          # nor does an empty prediction set need its per-ring outputs
    assert call(Rd=0, dt=(None, None, None), **per_ring) == -1 and b"device memory" in err()
    assert call(ws=None) == -1 and b"device memory" in err()          # the workspace is looked at last


def test_host_tensors_are_refused():
    from pixelspointspolygons_amd import eval_metrics as E, hip
    rings = E.pack_rings([[C.SQUARE_A]], "cpu", scores=[[0.5]], areas=[[256.0]])
    with pytest.raises(hip.P3Error):
        E.max_tangent_angle(rings, rings, 48, 48)
    with pytest.raises(hip.P3Error):
        hip.max_tangent_angle_device(rings["pos"], rings["ring_slice"], rings["ring_image"], rings["pos"], rings["ring_slice"], rings["ring_image"], 1, 48, 48)
    with pytest.raises(hip.P3Error, match="max_tangent_angle.*ring set"):
        E.max_tangent_angle({"pos": rings["pos"]}, rings, 48, 48)


def test_wrapper_refuses_wrong_shapes_types_and_parameters_before_any_launch(monkeypatch):
    from pixelspointspolygons_amd import eval_metrics as E, hip
    monkeypatch.setattr(hip, "_dev", lambda t: None)          # the shape checks come right behind the device check
    r = E.pack_rings([[C.SQUARE_A]], "cpu")
    pos, sl, im = r["pos"], r["ring_slice"], r["ring_image"]
    for bad in ((pos.double(), sl, im), (torch.zeros(4, 3), sl, im), (pos, sl.float(), im), (pos, sl[:, :1], im), (pos, sl, im.float()), (pos, sl, im[:0])):
        with pytest.raises(hip.P3Error, match="max_tangent_angle"):
            hip.max_tangent_angle_device(*bad, pos, sl, im, 1, 48, 48)
        with pytest.raises(hip.P3Error, match="max_tangent_angle"):
            hip.max_tangent_angle_device(pos, sl, im, *bad, 1, 48, 48)
    for B, H, W in ((0, 48, 48), (1, 0, 48), (1, 48, 0), (1, 513, 512)):
        with pytest.raises(hip.P3Error, match="height"):
            hip.max_tangent_angle_device(pos, sl, im, pos, sl, im, B, H, W)
    for kw in (dict(sampling_spacing=0.0), dict(sampling_spacing=0.01), dict(sampling_spacing=math.inf), dict(sampling_spacing=math.nan), dict(min_precision=1.0), dict(min_precision=-0.5),
               dict(min_precision=math.nan), dict(max_stretch=1.0), dict(max_stretch=math.inf), dict(max_stretch=math.nan)):
        with pytest.raises(hip.P3Error, match="sampling_spacing"):
            hip.max_tangent_angle_device(pos, sl, im, pos, sl, im, 1, 48, 48, **kw)
        with pytest.raises(hip.P3Error, match="sampling_spacing"):
            E.max_tangent_angle(r, r, 48, 48, **kw)
    with pytest.raises(hip.P3Error, match="images"):
        E.max_tangent_angle(r, E.pack_rings([[], []], "cpu"), 48, 48)
    with pytest.raises(hip.P3Error, match="mta"):          # polygon_metrics keeps refusing it as a mode
        E.polygon_metrics(r, r, 48, 48, modes=("iou", "mta"))


# ------------------------------------------------------------------------------------------ hand values of the restatement
def test_a_square_on_itself_its_shift_and_a_moved_corner():
    o = ref("hand_1")
    assert o["ring_px"].tolist() == [[256, 256], [256, 208], [240, 240]] and o["ring_state"].tolist() == [0, 0, 0] and o["status"].tolist() == [0]
    assert o["ring_cos"][0] == 1.0 and o["ring_angle"][0] == 0.0
    # the shift by (3, 0): the edges across A's right side are stretched by exactly 2 (|u| = 2 onto |v| = 1) and by 0.4 (2 onto 5), the samples beyond
    # x = 24 fall onto the corners (|v| = 0): all excluded, and every other edge is parallel to its projection
    assert o["ring_cos"][1] == 1.0 and o["ring_angle"][1] == 0.0
    want = 45.0 - math.degrees(math.atan(1.0 / 8.0))
    assert abs(math.degrees(o["ring_angle"][2]) - want) <= 1e-12 and abs(want - 37.87498365) <= 1e-8
    assert abs(o["MTA"] - want / 3.0) <= 1e-12 and o["counted"].tolist() == [3]
    alone = R.run([[C.SQUARE_A]], [[C.SLANTED]], 48, 48)
    assert abs(alone["MTA"] - want) <= 1e-12
    assert R.run([[C.SQUARE_A]], [[C.SQUARE_B]], 48, 48)["MTA"] == 0.0 and R.run([[C.SQUARE_A]], [[C.SQUARE_A]], 48, 48)["MTA"] == 0.0


def test_the_stretch_bounds_are_strict():
    s = R.samples(C.SQUARE_B, 2.0)
    p, q = R.gt_edges([C.SQUARE_A])
    nu, nv, _ = R.line_edges(s, R.nearest(s, p, q))
    with np.errstate(divide="ignore"):
        stretch = nu / nv
    assert (stretch == 2.0).sum() == 2 and (stretch == 0.4).sum() == 2 and (nv == 0).sum() == 4 and ((stretch == 1.0) | (stretch == 2.0) | (stretch == 0.4) | (nv == 0)).all()
    wide = ref("hand_1_stretch_4")          # max_stretch = 4 admits the edges at 2 and at 0.4: (0, -2) onto (-3, -4) has |cos| 0.8, the stretch-2 edges are parallel
    assert abs(wide["ring_cos"][1] - 0.8) <= 1e-15 and wide["ring_state"].tolist() == [0, 0, 0]


def test_states_of_rings_that_are_not_counted():
    o = ref("hand_2")
    assert o["ring_state"].tolist() == [R.BELOW_PRECISION, R.BELOW_PRECISION, R.EMPTY] and o["ring_px"].tolist() == [[36, 0], [256, 0], [0, 0]]
    assert math.isnan(o["MTA"]) and o["counted"].tolist() == [0] and o["status"].tolist() == [0] and np.isnan(o["ring_angle"]).all() and np.isnan(o["ring_cos"]).all()
    o = ref("hand_3")
    assert o["ring_state"].tolist() == [1, 1, 0, 1, 0, 0] and o["status"].tolist() == [1 | 4] and o["invalid_rings"].tolist() == [[1, 3], [0, 0], [0, 0]]
    assert o["ring_px"].tolist() == [[0, 0], [0, 0], [256, 208], [0, 0], [256, 256], [256, 256]]
    assert o["image_overlap_px"].tolist() == [0, 256, 0] and o["counted"].tolist() == [3] and o["MTA"] == 0.0          # both copies are still measured
    assert np.array_equal(o["ring_cos"][[2, 4, 5]], ref("hand_1")["ring_cos"][[1, 0, 0]])          # the invalid rings change nothing else
    o = ref("hand_empty")
    assert math.isnan(o["MTA"]) and o["counted"].tolist() == [0] and o["ring_state"].shape == (0,) and o["image_overlap_px"].tolist() == [0]
    o = ref("no_valid_edge_stretch_1.2")
    assert o["ring_state"].tolist() == [R.NO_EDGE, R.COUNTED] and math.isnan(o["ring_cos"][0]) and o["ring_px"][0].tolist() == [162, 162] and o["counted"].tolist() == [1]


def test_the_parameters_change_what_they_should():
    base, tight, fine = ref("hand_1"), ref("hand_1_precision_0.9"), ref("hand_1_spacing_0.5")
    assert tight["ring_state"].tolist() == [0, R.BELOW_PRECISION, 0] and np.array_equal(tight["ring_px"], base["ring_px"])          # 208 / 256 = 0.8125
    assert (fine["ring_samples"][1] - 1) == 4 * (base["ring_samples"][1] - 1) == 128 and fine["ring_cos"][1] == 1.0


def test_a_repeated_vertex_in_a_prediction_doubles_a_sample():
    _, gt, dt, H, W, _ = C.case("repeated_vertex_in_a_prediction_64x31")
    s = R.samples(dt[0][0], 2.0)
    p, q = R.gt_edges(gt[0])
    nu, nv, _ = R.line_edges(s, R.nearest(s, p, q))
    assert (nu == 0).sum() == 1 and np.array_equal(s[np.nonzero(nu == 0)[0][0]], dt[0][0][1].astype(np.float64))          # the doubled sample is the repeated vertex
    o = R.run(gt, dt, H, W)
    assert o["ring_state"].tolist() == [R.COUNTED] and o["ring_samples"].tolist() == [len(s)]


def test_the_tie_exception_needs_dyadic_operands():
    shifted = [[C.SQUARE_A]], [[C.SQUARE_B]]
    assert R.margins(*shifted, 48, 48, spacing=0.5)["ties"] == 0          # (11, 11) and (11, 21): equal squared distances 9 of exact operands
    off = np.float32(0.1)          # the same figure moved by 0.1: the ties are still exact in value but the operands are not dyadic
    moved = [[C.SQUARE_A + off]], [[C.SQUARE_B + off]]
    assert R.margins(*moved, 48, 48, spacing=0.5)["ties"] == 2


def test_the_sampling_rule():
    assert [R.edge_count(L, 2.0) for L in (3.0, 5.0, 7.0, 1.0, 0.9, 0.0, 2.0, 9.0, 11.0)] == [2, 2, 4, 1, 1, 1, 1, 4, 6]          # 1.5 -> 2, 2.5 -> 2, 3.5 -> 4, 0.5 -> 0 -> 1
    assert [R.edge_count(L, 0.5) for L in (1.25, 1.75, 0.2)] == [2, 4, 1]
    ring = C.f32([(0, 0), (3, 0), (3, 5), (0, 5)])
    s = R.samples(ring, 2.0)
    assert s.tolist() == [[0, 0], [1.5, 0], [3, 0], [3, 2.5], [3, 5], [1.5, 5], [0, 5], [0, 2.5], [0, 0]]
    oblique = C.f32([(0.1, 0.2), (7.3, 3.4), (2.2, 9.1)])
    s = R.samples(oblique, 2.0)
    r = oblique.astype(np.float64)
    assert len(s) == 1 + 4 + 4 + 5 and np.array_equal(s[[0, 4, 8, 13]], r[[0, 1, 2, 0]])          # the end points are the vertices themselves
    step = (r[1] - r[0]) / 4
    assert np.array_equal(s[3], r[0] + 3.0 * step)


# ------------------------------------------------------------------------------------------ the inputs of the GPU test are unambiguous and not degenerate
@pytest.mark.parametrize("case", C.all_cases(), ids=lambda c: c[0])
def test_gpu_inputs_are_unambiguous(case):
    name, gt, dt, H, W, params = case
    m = R.margins(gt, dt, H, W, **C.ref_params(params))
    assert m["pixels"] == 0 and m["count"] > 1e-6 and m["ties"] == 0 and m["stretch"] == 0, m
    o = R.run(gt, dt, H, W, **C.ref_params(params))
    at = 0
    for b, rings in enumerate(dt):
        counted = int((o["ring_state"][at:at + len(rings)] == R.COUNTED).sum())
        assert (counted == 0) == (b in C.EMPTY_IMAGES.get(name, ())), (name, b, counted)
        at += len(rings)


def test_the_shape_cases_reach_the_paths_they_are_named_for():
    from pixelspointspolygons_amd import hip
    _, gt, dt, H, W, _ = C.chunk_case()
    n = [len(r) for r in gt[0]]
    assert n[0] > hip.PM_EDGE_CHUNK and n[0] + n[1] == 2 * hip.PM_EDGE_CHUNK and len(n) == 3          # a chunk boundary inside a ring, the next one between two rings
    o = R.run(gt, dt, H, W)
    assert o["ring_samples"].max() > 256 and max(len(r) for r in dt[0]) > hip.PM_EDGE_CHUNK and o["ring_state"].tolist() == [0, 0]
    o = ref("long_ring_64x64_spacing_0.25")
    assert o["ring_samples"].min() > 256 and o["ring_samples"].max() > 2 * 255 + 1          # two tiles and three tiles
    o = ref("many_rings_many_images")
    assert len(C.many_rings_case()[1]) > 256 and len(C.many_rings_case()[2][0]) > 256 and set(o["ring_state"].tolist()) == {0, 2, 3}
    assert ref("33x21_one_image")["status"].tolist() == [4]          # two predictions of the image overlap by 7 pixels
