"""Polygon metrics without a device: the surface of p3_polygon_metrics and its argument checks, the host side of
pixelspointspolygons_amd.eval_metrics, the hand values of the float64 restatement tests/poly_metrics_ref.py, and the margins that make the exact comparisons
of test_poly_metrics_gpu.py legitimate."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import poly_metrics_cases as C
from tests import poly_metrics_ref as R

# (R_gt, R_dt, B): degenerate, the smallest valid one, an odd-sized one, the long-ring case of the GPU test, the bench shape (64 images of 20 + 20 rings)
RECORDED = [((0, 0, 0), 0), ((-1, 2, 2), 0), ((2, -1, 2), 0), ((0, 0, 4), 0), ((1, 1, 1), 2048), ((37, 29, 3), 4096), ((3, 2, 2), 2048),
            ((1280, 1280, 64), 122880)]


def _lib():
    from pixelspointspolygons_amd._lib import load
    from pixelspointspolygons_amd.build import build_library
    return load(build_library(verbose=False))


# ------------------------------------------------------------------------------------------ surface
def test_header_declares_and_library_exports_the_entries():
    from pixelspointspolygons_amd._lib import prototypes
    protos = prototypes()
    assert len(protos["p3_polygon_metrics"][1]) == 30 and protos["p3_polygon_metrics"][0] is ctypes.c_int
    assert protos["p3_polygon_metrics_workspace_bytes"] == (ctypes.c_int64, [ctypes.c_int] * 3)
    lib = _lib()
    assert lib.p3_polygon_metrics and lib.p3_polygon_metrics_workspace_bytes


def test_workspace_sizes_are_the_layouts():
    lib = _lib()
    up = lambda n: (n + 255) & ~255
    per_set = lambda r: 2 * up(4 * r) + up(8 * r) + up(32 * r)          # state, vertex count, first vertex, box
    for (rg, rd, b), nbytes in RECORDED:
        assert lib.p3_polygon_metrics_workspace_bytes(rg, rd, b) == nbytes, (rg, rd, b)
        if min(rg, rd) >= 0 and b >= 1:
            assert nbytes == per_set(rg) + per_set(rd)


def test_entry_validates_before_any_device_work():
    lib = _lib()
    one = ctypes.c_void_p(8)          # a non-null pointer that is never followed: every call below fails its checks first
    sl = np.array([[0, 4]], dtype=np.int64).ctypes.data_as(ctypes.c_void_p)
    im = np.array([0], dtype=np.int32).ctypes.data_as(ctypes.c_void_p)

    def call(Vg=4, Rg=1, Vd=4, Rd=1, B=1, H=8, W=8, modes=7, gt=(one, sl, im), dt=(one, sl, im), metrics=one, per_image=one, pairs=one, status=one, ws=one):
        return lib.p3_polygon_metrics(gt[0], Vg, gt[1], gt[2], Rg, dt[0], Vd, dt[1], dt[2], Rd, B, H, W, modes, metrics, per_image, per_image, per_image,
                                      per_image, per_image, per_image, per_image, pairs, pairs, pairs, pairs, per_image, status, ws, None)

    err = lambda: lib.p3_last_error_string()
    assert call(Vg=-1) == -1 and b"p3_polygon_metrics" in err() and b"negative" in err()
    assert call(Rg=-1) == -1 and call(Vd=-1) == -1 and call(Rd=-1) == -1
    assert call(B=0) == -1 and call(H=0) == -1 and call(W=0) == -1 and b"p3_polygon_metrics" in err()
    assert call(H=513, W=512) == -1 and b"2^18" in err()
    assert call(modes=0) == -1 and call(modes=8) == -1 and b"modes" in err()
    for kw in (dict(metrics=None), dict(per_image=None), dict(status=None), dict(pairs=None), dict(gt=(None, sl, im)), dict(gt=(one, None, im)),
               dict(gt=(one, sl, None)), dict(dt=(None, sl, im)), dict(dt=(one, None, im)), dict(dt=(one, sl, None))):
        assert call(**kw) == -1 and b"p3_polygon_metrics" in err() and b"null pointer" in err(), kw
    assert call() == -1 and b"device memory" in err()          # well-formed, but host arrays: nothing is launched on them
    assert call(Rg=0, gt=(None, None, None), pairs=None) == -1 and b"device memory" in err()          # an empty gt set needs none of its pointers


def test_host_tensors_are_refused():
    from pixelspointspolygons_amd import eval_metrics as E, hip
    rings = E.pack_rings([[C.SQUARE_A]], "cpu")
    with pytest.raises(hip.P3Error):
        E.polygon_metrics(rings, rings, 48, 48)
    with pytest.raises(hip.P3Error):
        hip.polygon_metrics_device(rings["pos"], rings["ring_slice"], rings["ring_image"], rings["pos"], rings["ring_slice"], rings["ring_image"], 1, 48, 48)
    ffl = {"ring_pos": torch.zeros(5, 2), "ring_slice": torch.tensor([[0, 5]]), "poly_rings": torch.tensor([[0, 1]]), "poly_batch": torch.tensor([0]),
           "poly_flags": torch.tensor([0]), "batch_size": 1}
    with pytest.raises(hip.P3Error):
        E.rings_from_ffl(ffl)
    with pytest.raises(hip.P3Error):
        E.rings_from_ffl({"tol_1": ffl})
    hisup = {"polygons": {"pos": torch.zeros(5, 2), "poly_slice": torch.tensor([[[0, 5]]]), "poly_flags": torch.tensor([[0]])},
             "regions": {"n_regions": torch.tensor([1])}}
    with pytest.raises(hip.P3Error):
        E.rings_from_hisup(hisup)
    with pytest.raises(hip.P3Error):
        E.rings_from_hisup({"polys_pred": [[C.SQUARE_A]]})          # host lists without a device to pack them onto
    with pytest.raises(hip.P3Error):
        E.rings_from_hisup({})
    with pytest.raises(hip.P3Error, match="ring set"):
        E.polygon_metrics({"pos": rings["pos"]}, rings, 48, 48)


def test_wrapper_refuses_wrong_shapes_and_modes_before_any_launch(monkeypatch):
    from pixelspointspolygons_amd import eval_metrics as E, hip
    monkeypatch.setattr(hip, "_dev", lambda t: None)          # the shape checks come right behind the device check
    r = E.pack_rings([[C.SQUARE_A]], "cpu")
    pos, sl, im = r["pos"], r["ring_slice"], r["ring_image"]
    for bad in ((pos.double(), sl, im), (torch.zeros(4, 3), sl, im), (pos, sl.float(), im), (pos, sl[:, :1], im), (pos, sl, im.float()), (pos, sl, im[:0])):
        with pytest.raises(hip.P3Error, match="polygon_metrics"):
            hip.polygon_metrics_device(*bad, pos, sl, im, 1, 48, 48)
        with pytest.raises(hip.P3Error, match="polygon_metrics"):
            hip.polygon_metrics_device(pos, sl, im, *bad, 1, 48, 48)
    for B, H, W in ((0, 48, 48), (1, 0, 48), (1, 48, 0), (1, 513, 512)):
        with pytest.raises(hip.P3Error, match="height"):
            hip.polygon_metrics_device(pos, sl, im, pos, sl, im, B, H, W)
    for modes in (0, 8, -1):
        with pytest.raises(hip.P3Error, match="modes"):
            hip.polygon_metrics_device(pos, sl, im, pos, sl, im, 1, 48, 48, modes)
    with pytest.raises(hip.P3Error, match="unknown mode"):
        E.polygon_metrics(r, r, 48, 48, modes=("iou", "mta"))
    with pytest.raises(hip.P3Error, match="images"):
        E.polygon_metrics(r, E.pack_rings([[], []], "cpu"), 48, 48)
    assert (hip.PM_IOU, hip.PM_POLIS, hip.PM_SAMPLES, hip.PM_MAX_HW, hip.PM_EDGE_CHUNK, hip.PM_TILE) == (1, 2, 4, 1 << 18, 32, 1024)


# ------------------------------------------------------------------------------------------ pack_rings
def test_pack_rings_drops_a_closing_duplicate_and_keeps_image_order():
    from pixelspointspolygons_amd import eval_metrics as E
    closed = np.concatenate([C.SQUARE_B, C.SQUARE_B[:1]])
    r = E.pack_rings([[C.SQUARE_A, closed], [], [torch.from_numpy(C.FAR), C.TWO.tolist()]], "cpu")
    assert r["batch_size"] == 3
    assert r["ring_slice"].tolist() == [[0, 4], [4, 8], [8, 12], [12, 14]] and r["ring_slice"].dtype == torch.int64
    assert r["ring_image"].tolist() == [0, 0, 2, 2] and r["ring_image"].dtype == torch.int32
    assert r["pos"].dtype == torch.float32 and np.array_equal(r["pos"].numpy(), np.concatenate([C.SQUARE_A, C.SQUARE_B, C.FAR, C.TWO]))
    e = E.pack_rings([[], []], "cpu")
    assert tuple(e["pos"].shape) == (0, 2) and tuple(e["ring_slice"].shape) == (0, 2) and tuple(e["ring_image"].shape) == (0,) and e["batch_size"] == 2


# ------------------------------------------------------------------------------------------ hand values of the restatement
def test_a_square_on_itself():
    o = R.run([[C.SQUARE_A]], [[C.SQUARE_A]], 48, 48)
    assert o["image_counts"].tolist() == [[256, 256]] and o["match"].tolist() == [0] and o["image_valid"].tolist() == [1]
    assert abs(o["means"]["IoU"] - 1) < 1e-10 and o["means"]["NR"] == 1.0
    assert o["means"]["POLIS"] == 0.0 and o["means"]["chamfer"] == 0.0 and o["means"]["hausdorff"] == 0.0


def test_a_square_against_its_shift():
    o = R.run([[C.SQUARE_A]], [[C.SQUARE_B]], 48, 48)
    assert o["image_counts"].tolist() == [[208, 304]]
    assert R.box_iou(R.box(C.SQUARE_A), R.box(C.SQUARE_B)) == 208 / 304
    assert o["match"].tolist() == [0] and o["image_valid"].tolist() == [1]
    assert abs(o["means"]["IoU"] - 208 / 304) < 1e-10
    assert abs(o["means"]["POLIS"] - 1.2) <= 1e-12
    assert 3.0 <= o["means"]["hausdorff"] <= math.sqrt(9 + 0.05 ** 2)
    assert 0.0 < o["means"]["chamfer"] < o["means"]["hausdorff"]


def test_two_empty_sets():
    o = R.run([[]], [[]], 48, 48)
    assert o["means"]["IoU"] == 1.0 and o["means"]["C-IoU"] == 1.0 and o["image_valid"].tolist() == [0]
    assert all(math.isnan(o["means"][k]) for k in ("POLIS", "chamfer", "hausdorff"))


def test_a_far_away_prediction():
    o = R.run([[C.SQUARE_A]], [[C.FAR]], 48, 48)
    assert o["means"]["IoU"] == 0.0 and o["image_counts"].tolist() == [[0, 256 + 36]]
    assert o["match"].tolist() == [-1] and o["image_valid"].tolist() == [0] and math.isnan(o["means"]["POLIS"]) and math.isnan(o["pair_chamfer"][0])


def test_a_two_vertex_ring_is_counted_and_changes_nothing_else():
    plain = R.run([[C.SQUARE_A]], [[C.SQUARE_B]], 48, 48)
    o = R.run([[C.TWO, C.SQUARE_A]], [[C.SQUARE_B, C.TWO]], 48, 48)
    assert o["invalid_rings"].tolist() == [[1, 1]] and o["status"].tolist() == [1] and plain["status"].tolist() == [0]
    assert o["match"].tolist() == [-1, 0]
    assert np.array_equal(o["metrics"], plain["metrics"]) and np.array_equal(o["image_counts"], plain["image_counts"])
    nan_ring = np.array([(8, 8), (24, 8), (float("nan"), 24)], np.float32)
    inf_ring = np.array([(8, 8), (24, 8), (float("inf"), 24)], np.float32)
    o = R.run([[nan_ring, C.SQUARE_A, inf_ring]], [[C.SQUARE_B]], 48, 48)
    assert o["invalid_rings"].tolist() == [[2, 0]] and np.array_equal(o["metrics"], plain["metrics"])


def test_samples_follow_the_written_rule():
    s = R.samples(C.SQUARE_A)
    assert len(s) == 4 * 160 + 1 and np.array_equal(s[0], s[-1]) and np.array_equal(s[160], [24, 8])
    assert np.abs(np.diff(s[:161, 0]) - 0.1).max() < 1e-12
    rep = np.array([(0, 0), (1, 0), (1, 0), (0, 1)], np.float32)          # a zero-length edge gives its point once
    assert len(R.samples(rep)) == 10 + 1 + 15 + 10 + 1


# ------------------------------------------------------------------------------------------ the inputs of the GPU test are unambiguous
@pytest.mark.parametrize("case", C.all_cases(), ids=lambda c: c[0])
def test_gpu_inputs_are_unambiguous(case):
    _, gt, dt, H, W = case
    near, frac, thr = R.margins(gt, dt, H, W)
    assert near == 0 and frac > 1e-6 and thr > 1e-3, (near, frac, thr)


def test_seeded_images_have_counted_and_uncounted_rings():
    for seed in C.SEEDS:
        gt, dt = C.seeded_image(seed)
        assert len(gt) == 4 and len(dt) == 4 and all(4 <= len(g) <= 8 for g in gt)
        match = R.run([gt], [dt], 48, 48)["match"]
        assert 2 <= int((match >= 0).sum()) <= 3 and match[3] == -1
