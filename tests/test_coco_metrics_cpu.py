"""COCO metrics without a device: the surface of p3_coco_metrics and its argument checks, the threshold tables, the workspace layout,
the host side of pixelspointspolygons_amd.eval_metrics, the hand values of the restatement tests/coco_metrics_ref.py, and the margins that make the exact
comparisons of test_coco_metrics_gpu.py legitimate."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import coco_metrics_cases as C
from tests import coco_metrics_ref as R

P = 1.0 / (1.0 + 2.0 ** -52)          # the precision of one true positive and nothing else: tp / (fp + tp + 2^-52)


def _lib():
    from pixelspointspolygons_amd._lib import load
    from pixelspointspolygons_amd.build import build_library
    return load(build_library(verbose=False))


def ref(name, **kw):
    _, gt, dt, H, W, scores, areas = C.case(name)
    return R.run(gt, dt, H, W, scores, areas, **kw)


# ------------------------------------------------------------------------------------------ surface
def test_header_declares_and_library_exports_the_entries():
    from pixelspointspolygons_amd._lib import prototypes
    protos = prototypes()
    assert len(protos["p3_coco_metrics"][1]) == 31 and protos["p3_coco_metrics"][0] is ctypes.c_int
    assert protos["p3_coco_metrics_workspace_bytes"] == (ctypes.c_int64, [ctypes.c_int] * 6)
    assert protos["p3_coco_thresholds"] == (None, [ctypes.c_void_p] * 2)
    lib = _lib()
    assert lib.p3_coco_metrics and lib.p3_coco_metrics_workspace_bytes and lib.p3_coco_thresholds


def test_threshold_tables_are_numpys_bit_for_bit():
    lib = _lib()
    iou, rec = np.zeros(10), np.zeros(101)
    lib.p3_coco_thresholds(iou.ctypes.data_as(ctypes.c_void_p), rec.ctypes.data_as(ctypes.c_void_p))
    assert np.array_equal(iou.view(np.int64), np.linspace(0.5, 0.95, 10).view(np.int64))
    assert np.array_equal(rec.view(np.int64), np.linspace(0, 1, 101).view(np.int64))
    lib.p3_coco_thresholds(None, None)          # either pointer may be null
    assert np.array_equal(R.IOU_THRS, iou) and np.array_equal(R.REC_THRS, rec)


def test_workspace_sizes_are_the_layouts():
    from pixelspointspolygons_amd import hip
    lib = _lib()
    up = lambda n: (n + 255) & ~255

    def want(rg, rd, b, h, w, types):
        slab = 4 * h * ((w + 31) // 32)
        slabs = 3 if types & 2 else 1
        per_set = lambda r: 2 * up(4 * r) + up(8 * r) + up(32 * r) + up(16 * r) + up(r) + slabs * up(slab * r)
        return per_set(rg) + per_set(rd) + up(400 * b) + up(1600 * rg) + up(12 * rd) + up(240 * rd) + up(960 * rd) + up(1920 * rd)

    for args in ((1, 1, 1, 48, 48, 3), (1, 1, 1, 48, 48, 1), (37, 29, 3, 33, 21, 2), (0, 5, 2, 64, 31, 3), (1280, 1280, 64, 224, 224, 3), (3, 103, 1, 512, 512, 1)):
        assert lib.p3_coco_metrics_workspace_bytes(*args) == want(*args) == hip.coco_metrics_workspace_bytes(*args), args
    assert lib.p3_coco_metrics_workspace_bytes(1280, 1280, 64, 224, 224, 3) == 54417920          # the bench scene: 6 x 8.0 MB of slabs, 4.0 MB of series, 2.0 MB of pair IoUs
    for args in ((-1, 1, 1, 8, 8, 3), (1, -1, 1, 8, 8, 3), (1, 1, 0, 8, 8, 3), (1, 1, 1, 0, 8, 3), (1, 1, 1, 8, 0, 3), (1, 1, 1, 513, 512, 3), (1, 1, 1, 8, 8, 0),
                 (1, 1, 1, 8, 8, 4)):
        assert lib.p3_coco_metrics_workspace_bytes(*args) == 0, args


def test_entry_validates_before_any_device_work():
    lib = _lib()
    one = ctypes.c_void_p(8)          # a non-null pointer that is never followed: every call below fails its checks first
    sl = np.array([[0, 4]], dtype=np.int64).ctypes.data_as(ctypes.c_void_p)
    im = np.array([0], dtype=np.int32).ctypes.data_as(ctypes.c_void_p)

    def call(Vg=4, Rg=1, Vd=4, Rd=1, B=1, H=8, W=8, types=3, gt=(one, sl, im), dt=(one, sl, im), area=None, score=None, tables=one, per_gt=one, per_dt=one,
             status=one, ws=one):
        return lib.p3_coco_metrics(gt[0], Vg, gt[1], gt[2], area, Rg, dt[0], Vd, dt[1], dt[2], score, Rd, B, H, W, types, tables, tables, tables, per_gt, per_dt,
                                   per_gt, per_dt, per_dt, per_gt, per_dt, per_dt, per_gt, status, ws, None)

    err = lambda: lib.p3_last_error_string()
    assert call(Vg=-1) == -1 and b"p3_coco_metrics" in err() and b"negative" in err()
    assert call(Rg=-1) == -1 and call(Vd=-1) == -1 and call(Rd=-1) == -1
    assert call(B=0) == -1 and call(H=0) == -1 and call(W=0) == -1 and b"p3_coco_metrics" in err()
    assert call(H=513, W=512) == -1 and b"p3_coco_metrics" in err() and b"2^18" in err()
    for types in (0, 4, 7, -1):
        assert call(types=types) == -1 and b"p3_coco_metrics" in err() and b"iou_types" in err(), types
    for kw in (dict(tables=None), dict(status=None), dict(per_gt=None), dict(per_dt=None), dict(gt=(None, sl, im)), dict(gt=(one, None, im)),
               dict(gt=(one, sl, None)), dict(dt=(None, sl, im)), dict(dt=(one, None, im)), dict(dt=(one, sl, None))):
        assert call(**kw) == -1 and b"p3_coco_metrics" in err() and b"null pointer" in err(), kw
    assert call() == -1 and b"p3_coco_metrics" in err() and b"device memory" in err()          # well-formed, but host index arrays
    assert call(Rg=0, gt=(None, None, None), per_gt=None) == -1 and b"ring_slice" in err()          # an empty gt set needs none of its pointers
    empty = (None, None, None)          # score / area in host memory: test_coco_metrics_gpu.py, where the index arrays can be device memory
    assert call(Rg=0, gt=empty, per_gt=None, Rd=0, dt=empty, per_dt=None, ws=None) == -1 and b"null workspace" in err()          # the checks are passed up to there


def test_host_tensors_are_refused():
    from pixelspointspolygons_amd import eval_metrics as E, hip
    rings = E.pack_rings([[C.SQUARE_A]], "cpu", scores=[[0.5]], areas=[[256.0]])
    with pytest.raises(hip.P3Error):
        E.coco_metrics(rings, rings, 48, 48)
    with pytest.raises(hip.P3Error):
        hip.coco_metrics_device(rings["pos"], rings["ring_slice"], rings["ring_image"], rings["pos"], rings["ring_slice"], rings["ring_image"], 1, 48, 48)
    with pytest.raises(hip.P3Error, match="coco_metrics.*ring set"):
        E.coco_metrics({"pos": rings["pos"]}, rings, 48, 48)


def test_wrapper_refuses_wrong_shapes_and_types_before_any_launch(monkeypatch):
    from pixelspointspolygons_amd import eval_metrics as E, hip
    monkeypatch.setattr(hip, "_dev", lambda t: None)          # the shape checks come right behind the device check
    r = E.pack_rings([[C.SQUARE_A]], "cpu")
    pos, sl, im = r["pos"], r["ring_slice"], r["ring_image"]
    for bad in ((pos.double(), sl, im), (torch.zeros(4, 3), sl, im), (pos, sl.float(), im), (pos, sl[:, :1], im), (pos, sl, im.float()), (pos, sl, im[:0])):
        with pytest.raises(hip.P3Error, match="coco_metrics"):
            hip.coco_metrics_device(*bad, pos, sl, im, 1, 48, 48)
        with pytest.raises(hip.P3Error, match="coco_metrics"):
            hip.coco_metrics_device(pos, sl, im, *bad, 1, 48, 48)
    for B, H, W in ((0, 48, 48), (1, 0, 48), (1, 48, 0), (1, 513, 512)):
        with pytest.raises(hip.P3Error, match="height"):
            hip.coco_metrics_device(pos, sl, im, pos, sl, im, B, H, W)
    for types in (0, 4, -1):
        with pytest.raises(hip.P3Error, match="iou_types"):
            hip.coco_metrics_device(pos, sl, im, pos, sl, im, 1, 48, 48, types)
    for field in (torch.zeros(2), torch.zeros(1, dtype=torch.float64), torch.zeros(1, 1)):
        with pytest.raises(hip.P3Error, match="dt_score"):
            hip.coco_metrics_device(pos, sl, im, pos, sl, im, 1, 48, 48, dt_score=field)
        with pytest.raises(hip.P3Error, match="gt_area"):
            hip.coco_metrics_device(pos, sl, im, pos, sl, im, 1, 48, 48, gt_area=field)
    with pytest.raises(hip.P3Error, match="unknown iou type"):
        E.coco_metrics(r, r, 48, 48, iou_types=("segm", "bbox"))
    with pytest.raises(hip.P3Error, match="empty"):
        E.coco_metrics(r, r, 48, 48, iou_types=())
    with pytest.raises(hip.P3Error, match="images"):
        E.coco_metrics(r, E.pack_rings([[], []], "cpu"), 48, 48)
    assert (hip.COCO_SEGM, hip.COCO_BOUNDARY, hip.COCO_KEEP, hip.COCO_IOU_LDS) == (1, 2, 100, 2048)
    assert E.COCO_KEYS == R.KEYS


# ------------------------------------------------------------------------------------------ pack_rings and the converters
def test_pack_rings_takes_scores_and_areas():
    from pixelspointspolygons_amd import eval_metrics as E, hip
    r = E.pack_rings([[C.SQUARE_A, C.SQUARE_B], [], [C.FAR]], "cpu", scores=[[0.25, 0.5], [], [1.0]], areas=[[256, 255.5], [], [36]])
    assert r["score"].tolist() == [0.25, 0.5, 1.0] and r["score"].dtype == torch.float32
    assert r["area"].tolist() == [256.0, 255.5, 36.0] and r["area"].dtype == torch.float32 and r["ring_image"].tolist() == [0, 0, 2]
    plain = E.pack_rings([[C.SQUARE_A]], "cpu")
    assert "score" not in plain and "area" not in plain
    for bad in ([[0.25], [], [1.0]], [[0.25, 0.5], [1.0]], [[0.25, 0.5], [1.0], []]):
        with pytest.raises(hip.P3Error, match="scores"):
            E.pack_rings([[C.SQUARE_A, C.SQUARE_B], [], [C.FAR]], "cpu", scores=bad)
    assert "score" not in E.rings_from_pix2poly([[torch.from_numpy(C.SQUARE_A)]], "cpu", unit_scores=True)


# ------------------------------------------------------------------------------------------ hand values of the restatement
def test_a_square_on_itself():
    o = ref("square_on_itself")
    assert o["gt_area_px"].tolist() == [256] and o["dt_area_px"].tolist() == [256] and o["gt_boundary_px"].tolist() == [60] and o["dt_rank"].tolist() == [0]
    assert o["pair_inter"][:, 0].tolist() == [256, 60] and (o["dt_match"][:, 0] == 0).all() and (o["dt_match"][:, 1] == 0).all()
    for ty in range(2):          # every stat 1 up to the 2^-52 of pycocotools' precision; the buckets without a gt ring are -1
        s = o["stats"][ty]
        assert np.abs(s[[0, 1, 2, 3]] - 1).max() <= 1e-15 and (s[[6, 7, 8, 9]] == 1.0).all() and (s[[4, 5, 10, 11]] == -1.0).all(), s
    assert (o["precision"][:, :, :, 0, :] == P).all() and (o["precision"][:, :, :, 2:, :] == -1).all() and (o["recall"][:, :, :2, :] == 1).all()


def test_a_square_against_its_shift():
    o = ref("square_shifted")
    assert o["pair_inter"][0, 0] == 208 and o["gt_area_px"][0] + o["dt_area_px"][0] - 208 == 304
    assert (o["dt_match"][0, 0, :4, 0] == 0).all() and (o["dt_match"][0, 0, 4:, 0] == -1).all()          # 0.684: matched at 0.5 .. 0.65 and not above
    want = 0.0
    for _ in range(4 * 101):
        want += P
    want /= 1010          # four thresholds of 101 entries P, six of 101 zeros
    assert o["stats"][0, 0] == want and abs(want - 0.4) <= 1e-12 and o["stats"][0, 1] == mean_p(101) and o["stats"][0, 2] == 0.0
    assert abs(o["stats"][0, 8] - 0.4) <= 1e-15 and o["stats"][0, 3] == want and o["stats"][0, 4] == -1.0
    # the boundaries (one pixel wide frames three columns apart) share 2 rows of 13 pixels: far below 0.5
    assert o["pair_inter"][1, 0] == 26 and o["stats"][1, 0] == 0.0


def mean_p(n):
    s = 0.0
    for _ in range(n):
        s += P
    return s / n


def test_equality_with_a_threshold_matches():
    o = ref("iou_exactly_half")
    assert o["pair_inter"][0, 0] == 128 and o["dt_area_px"][0] == 128
    assert o["dt_match"][0, 0, :, 0].tolist() == [0] + [-1] * 9
    o = ref("iou_exactly_three_quarters")
    assert o["pair_inter"][0, 0] == 192 and o["dt_area_px"][0] == 192
    assert o["dt_match"][0, 0, :, 0].tolist() == [0] * 6 + [-1] * 4          # 0.75 is iouThrs[5]


def test_the_earlier_of_two_equal_predictions_wins():
    o = ref("two_predictions_one_gt")
    assert o["dt_rank"].tolist() == [0, 1] and (o["dt_match"][0, 0, :, 0] == 0).all() and (o["dt_match"][0, 0, :, 1] == -1).all()
    assert (o["gt_match"][0, 0, :, 0] == 0).all()
    assert (o["precision"][0, :, :, 0, 2] == P).all()          # the false positive lies behind full recall
    assert o["dt_ignore"][0, 0].sum() == 0 and (o["dt_ignore"][0, 2] == 1).all()          # outside the medium bucket: ignored, matched or not


def test_the_walk_is_greedy():
    o = ref("greedy_keeps_the_earlier")
    assert o["dt_match"][0, 0, :4, 0].tolist() == [0] * 4 and o["dt_match"][0, 0, :4, 1].tolist() == [-1] * 4          # the shifted square came first
    assert o["dt_match"][0, 0, 4:, 0].tolist() == [-1] * 6 and o["dt_match"][0, 0, 4:, 1].tolist() == [0] * 6
    assert o["gt_match"][0, 0, :, 0].tolist() == [0] * 4 + [1] * 6


def test_scores_order_the_predictions_and_cut_at_100():
    name, gt, dt, H, W, scores, _ = C.many_predictions(3)
    o = R.run(gt, dt, H, W, scores, None, iou_types=("segm",))
    rank = o["dt_rank"]
    assert sorted(rank[rank >= 0].tolist()) == list(range(100)) and int((rank < 0).sum()) == 3
    s = np.float32(scores[0])
    order = np.argsort(rank[rank >= 0])
    kept = np.nonzero(rank >= 0)[0][order]
    assert (np.diff(s[kept]) <= 0).all() and all(a < b for a, b in zip(kept[:-1], kept[1:]) if s[a] == s[b])          # descending, ties in input order
    assert s[rank < 0].max() <= s[kept].min() and len(set(scores[0])) < 103
    assert np.isnan(o["stats"][1]).all() and int(o["dt_boundary_px"].sum()) == 0 and int(o["pair_inter"][1].sum()) == 0
    assert (o["dt_match"][0, 0, 0] >= 0).sum() == 3 and (o["dt_match"][0, 0, 1] >= 0).sum() == 2          # IoU 6 / 12 matches at 0.5 alone
    unit = R.run(gt, dt, H, W, None, None, iou_types=("segm",))
    assert unit["dt_rank"].tolist() == list(range(100)) + [-1] * 3


def test_area_moves_a_gt_ring_across_a_bucket_edge():
    name, gt, dt, H, W, scores, areas = C.area_case()
    given, own = R.run(gt, dt, H, W, scores, areas), R.run(gt, dt, H, W, scores, None)
    assert own["stats"][0, 4] == -1.0 and given["stats"][0, 4] > 0          # medium: no gt ring by pixel count, one by annotation
    assert np.array_equal(given["gt_area_px"], own["gt_area_px"]) and np.array_equal(given["pair_inter"], own["pair_inter"])
    assert given["dt_ignore"][0, 1, 0].tolist() == [1, 0] and own["dt_ignore"][0, 1, 0].tolist() == [0, 0]          # the small bucket


def test_invalid_rings_take_part_in_nothing():
    o = ref("invalid_rings")
    assert o["status"].tolist() == [1] and o["dt_rank"].tolist() == [0, -1, -1, 1]
    assert o["gt_area_px"].tolist() == [0, 256] and o["dt_area_px"].tolist() == [256, 0, 0, 36]
    assert np.array_equal(o["stats"], ref("square_shifted")["stats"])          # the far false positive lies behind full recall


def test_boundary_rules():
    m = np.zeros((9, 12), bool)
    m[0:5, 0:6] = True          # touches the top and the left edge: the boundary stays on them
    b = R.boundary_mask(m, 1)
    assert b.sum() == 30 - 12 and not b[1:4, 1:5].any() and b[0].sum() == 6 and b[:5, 0].all()
    thin = np.zeros((9, 12), bool)
    thin[2:8, 4:6] = True
    assert np.array_equal(R.boundary_mask(thin, 1), thin)          # thinner than 2 d + 1: nothing survives the erosion
    assert [R.dilation(*hw) for hw in ((48, 48), (33, 21), (64, 31), (40, 96), (224, 224), (512, 512), (4, 4))] == [1, 1, 1, 2, 6, 14, 1]
    assert R.dilation(75, 100) == 2 and R.dilation(105, 140) == 4          # 2.5 and 3.5: half goes to the even neighbour


# ------------------------------------------------------------------------------------------ the inputs of the GPU test are unambiguous and not degenerate
@pytest.mark.parametrize("case", C.all_cases(), ids=lambda c: c[0])
def test_gpu_inputs_are_unambiguous(case):
    _, gt, dt, H, W, _, _ = case
    assert R.margins(gt, dt, H, W) == 0


@pytest.mark.parametrize("case", C.seeded_cases() + [C.five_rings_224(), C.case("words_40x96")], ids=lambda c: c[0])
def test_seeded_scenes_are_not_degenerate(case):
    _, gt, dt, H, W, scores, areas = case
    o = R.run(gt, dt, H, W, scores, areas)
    for ty in range(2):
        m = o["dt_match"][ty, 0, 0][o["dt_rank"] >= 0]
        assert (m >= 0).any() and (m < 0).any(), ty
        p = o["precision"][ty, :, :, 0, 2]
        assert len(np.unique(p[p > -1])) >= 2, ty
    assert not math.isnan(o["stats"].sum())


def test_all_four_buckets_are_live_at_224():
    _, gt, dt, H, W, scores, areas = C.five_rings_224()
    o = R.run(gt, dt, H, W, scores, areas)
    assert (o["stats"] > -1).all() and o["gt_area_px"].max() > 9216 and o["gt_area_px"].min() < 1024 and R.dilation(H, W) == 6


def test_the_match_kernel_stage_is_exceeded_by_one_case():
    from pixelspointspolygons_amd import hip
    assert 2 * 3 * hip.COCO_KEEP <= hip.COCO_IOU_LDS < 2 * 11 * hip.COCO_KEEP
