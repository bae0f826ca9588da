"""COCO metrics on the device against the restatement tests/coco_metrics_ref.py.  Every output is compared for equality: the counts
are integers, precision and recall are IEEE quotients of equal integers, and the restatement sums the means in the kernel's index order.  Under the margin
test_coco_metrics_cpu.py asserts for these inputs no pixel can legitimately differ."""
import ctypes

import numpy as np
import pytest
import torch

from tests import coco_metrics_cases as C
from tests import coco_metrics_ref as R
from tests import guard

pytestmark = pytest.mark.gpu
DEV = "cuda"
INTS = ("gt_area_px", "dt_area_px", "gt_boundary_px", "dt_boundary_px", "dt_rank", "pair_inter", "dt_match", "dt_ignore", "gt_match", "status")
FLOATS = ("precision", "recall", "stats")
PER_GT = ("gt_area_px", "gt_boundary_px")
PER_DT = ("dt_area_px", "dt_boundary_px", "dt_rank")
_REF = {}


def ref(case, iou_types=R.TYPES):
    """the restatement of a case, computed once and shared"""
    name, gt, dt, H, W, scores, areas = case
    key = (name, tuple(iou_types))
    if key not in _REF:
        _REF[key] = R.run(gt, dt, H, W, scores, areas, iou_types)
    return _REF[key]


def pack(case):
    from pixelspointspolygons_amd import eval_metrics as E
    _, gt, dt, H, W, scores, areas = case
    return E.pack_rings(gt, DEV, areas=areas), E.pack_rings(dt, DEV, scores=scores)


def device(case, types=3, out=None):
    from pixelspointspolygons_amd import hip
    _, gt, _, H, W, _, _ = case
    g, d = pack(case)
    return hip.coco_metrics_device(g["pos"], g["ring_slice"], g["ring_image"], d["pos"], d["ring_slice"], d["ring_image"], len(gt), H, W, types,
                                   dt_score=d.get("score"), gt_area=g.get("area"), out=out)


def to_host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def bits(a):
    return a.view(np.int64) if a.dtype == np.float64 else a


def compare(got, want, keys=INTS + FLOATS):
    for k in keys:
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        if k in FLOATS:
            assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k
            bad = np.nonzero(np.nan_to_num(got[k]) != np.nan_to_num(want[k]))
            assert not len(bad[0]), (k, [tuple(int(i[0]) for i in bad)], got[k][bad][:4].tolist(), want[k][bad][:4].tolist())
        else:
            assert np.array_equal(got[k], want[k]), (k, got[k].tolist()[:40], want[k].tolist()[:40])


@pytest.mark.parametrize("case", C.all_cases(), ids=lambda c: c[0])
def test_cases_equal_the_restatement(case):
    compare(to_host(device(case)), ref(case))


def test_hand_values_on_the_device():
    o = to_host(device(C.case("square_shifted")))
    assert o["pair_inter"][:, 0].tolist() == [208, 26] and o["gt_area_px"].tolist() == [256] and o["dt_area_px"].tolist() == [256]
    assert o["dt_match"][0, 0, :, 0].tolist() == [0] * 4 + [-1] * 6 and abs(o["stats"][0, 0] - 0.4) <= 1e-12 and o["stats"][0, 4] == -1.0
    o = to_host(device(C.case("square_on_itself")))
    assert np.abs(o["stats"][:, [0, 1, 2, 3]] - 1).max() <= 1e-15 and (o["stats"][:, 6:10] == 1).all() and (o["stats"][:, [4, 5, 10, 11]] == -1).all()
    o = to_host(device(C.case("iou_exactly_three_quarters")))
    assert o["dt_match"][0, 0, :, 0].tolist() == [0] * 6 + [-1] * 4


@pytest.mark.parametrize("name", ["seeded_empty_01", "words_40x96", "predictions_103_gt_11"])
def test_one_type_alone(name):
    case = C.case(name)
    both = to_host(device(case))
    segm = to_host(device(case, 1))
    compare(segm, ref(case, ("segm",)))
    assert np.isnan(segm["stats"][1]).all() and np.isnan(segm["precision"][1]).all() and np.isnan(segm["recall"][1]).all()
    assert not segm["gt_boundary_px"].any() and not segm["dt_boundary_px"].any() and not segm["pair_inter"][1].any()          # no boundary work, by the outputs
    assert (segm["dt_match"][1] == -1).all() and (segm["gt_match"][1] == -1).all() and not segm["dt_ignore"][1].any()
    for k in ("pair_inter", "dt_match", "dt_ignore", "gt_match", "precision", "recall", "stats"):          # the segm rows do not depend on the other type
        assert np.array_equal(bits(segm[k][0]), bits(both[k][0])), k
    boundary = to_host(device(case, 2))
    compare(boundary, ref(case, ("boundary",)))
    assert np.isnan(boundary["stats"][0]).all() and np.array_equal(bits(boundary["stats"][1]), bits(both["stats"][1]))
    assert np.array_equal(boundary["pair_inter"], both["pair_inter"]) and np.array_equal(boundary["dt_match"][1], both["dt_match"][1])


def test_scores_and_areas_given_or_absent():
    name, gt, dt, H, W, scores, areas = C.case("seeded_2_gt_only_pred_only")
    unit = (name + "_unit", gt, dt, H, W, None, None)
    a, b = to_host(device(C.case(name))), to_host(device(unit))
    compare(b, ref(unit))
    assert not np.array_equal(a["dt_rank"], b["dt_rank"]) and np.array_equal(a["dt_area_px"], b["dt_area_px"])
    ones = (name + "_ones", gt, dt, H, W, [[1.0] * len(x) for x in dt], None)          # a null score pointer is every score 1.0
    c = to_host(device(ones))
    for k in INTS + FLOATS:
        assert np.array_equal(bits(b[k]), bits(c[k])), k
    name, gt, dt, H, W, scores, areas = C.area_case()
    own = (name + "_own", gt, dt, H, W, scores, None)
    a, b = to_host(device(C.area_case())), to_host(device(own))
    compare(b, ref(own))
    assert a["stats"][0, 4] > 0 and b["stats"][0, 4] == -1.0 and np.array_equal(a["pair_inter"], b["pair_inter"])


def test_two_runs_and_an_image_alone_give_the_same_bits():
    for case in (C.case("seeded_empty_01"), C.case("seeded_2_gt_only_pred_only"), C.case("64x31")):
        name, gt, dt, H, W, scores, areas = case
        a, b = to_host(device(case)), to_host(device(case))
        for k in a:
            assert np.array_equal(bits(a[k]), bits(b[k])), k
        g_at = d_at = 0
        for i in range(len(gt)):
            alone = (f"{name}_{i}", [gt[i]], [dt[i]], H, W, None if scores is None else [scores[i]], None if areas is None else [areas[i]])
            o = to_host(device(alone))
            ng, nd = len(gt[i]), len(dt[i])
            for k in PER_GT:
                assert np.array_equal(o[k], a[k][g_at:g_at + ng]), (k, i)
            for k in PER_DT:
                assert np.array_equal(o[k], a[k][d_at:d_at + nd]), (k, i)
            assert np.array_equal(o["pair_inter"], a["pair_inter"][:, 100 * g_at:100 * (g_at + ng)]), i
            assert np.array_equal(o["dt_ignore"], a["dt_ignore"][..., d_at:d_at + nd]), i
            m = a["dt_match"][..., d_at:d_at + nd]
            assert np.array_equal(o["dt_match"], np.where(m >= 0, m - g_at, -1)), i
            m = a["gt_match"][..., g_at:g_at + ng]
            assert np.array_equal(o["gt_match"], np.where(m >= 0, m - d_at, -1)), i
            g_at, d_at = g_at + ng, d_at + nd


def test_outputs_in_guard_bands():
    from pixelspointspolygons_amd import hip
    for name, types in (("seeded_empty_01", 3), ("predictions_103_gt_3", 3), ("words_40x96", 1)):
        case = C.case(name)
        got = to_host(guard.guarded_run(lambda out=None: device(case, types, out=out)))
        compare(got, ref(case, R.TYPES if types == 3 else ("segm",)))
    fn = lambda out=None: device(C.case("square_shifted"), out=out)
    with pytest.raises(hip.P3Error, match="stats"):
        fn(out={"stats": torch.zeros(12, dtype=torch.float64, device=DEV)})
    with pytest.raises(hip.P3Error, match="no"):
        fn(out={"metrics": torch.zeros(24, dtype=torch.float64, device=DEV)})


def test_rings_that_are_left_out_are_flagged():
    from pixelspointspolygons_amd import eval_metrics as E
    case = C.case("seeded_empty_01")
    _, gt, dt, H, W, scores, _ = case
    want = ref(case)
    g, d = pack(case)
    n = d["ring_slice"].shape[0]
    extra = dict(d, ring_slice=torch.cat([d["ring_slice"], torch.tensor([[0, 4], [6, 9]], device=DEV)]),
                 ring_image=torch.cat([d["ring_image"], torch.tensor([3, 3], dtype=torch.int32, device=DEV)]),          # image 3 of 3
                 score=torch.cat([d["score"], torch.tensor([2.0, 2.0], device=DEV)]))
    res = E.coco_metrics(extra, g, H, W)
    assert res["status"] == 2
    got = to_host(dict(res["tables"], **res["pairs"]))
    compare(got, want, FLOATS + PER_GT + ("pair_inter", "gt_match"))
    for k in PER_DT + ("dt_match", "dt_ignore"):
        assert np.array_equal(got[k][..., :n], want[k]), k
    assert got["dt_rank"][n:].tolist() == [-1, -1] and (got["dt_match"][..., n:] == -1).all() and not got["dt_area_px"][n:].any()


def test_score_and_area_in_host_memory_are_refused():
    from pixelspointspolygons_amd import hip
    g, d = pack(C.case("square_shifted"))
    one = torch.zeros(4096, dtype=torch.float64, device=DEV)          # every output and the workspace: nothing is launched
    host = np.ones(1, np.float32)
    lib = hip.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for area, score in ((host.ctypes.data_as(ctypes.c_void_p), None), (None, host.ctypes.data_as(ctypes.c_void_p))):
        rc = lib.p3_coco_metrics(p(g["pos"]), 4, p(g["ring_slice"]), p(g["ring_image"]), area, 1, p(d["pos"]), 4, p(d["ring_slice"]), p(d["ring_image"]), score,
                                 1, 1, 48, 48, 3, *([p(one)] * 13), p(one), None)
        assert rc == -1 and b"p3_coco_metrics: score and area must be device memory" in lib.p3_last_error_string()
    with pytest.raises(hip.P3Error):
        hip.coco_metrics_device(g["pos"], g["ring_slice"], g["ring_image"], d["pos"], d["ring_slice"], d["ring_image"], 1, 48, 48, dt_score=torch.ones(1))


def test_the_public_function_on_converted_ring_sets():
    from pixelspointspolygons_amd import eval_metrics as E, hip
    close = lambda r: np.concatenate([r, r[:1]])
    case = C.case("seeded_empty_01")
    _, gt, dt, H, W, scores, _ = case
    gt, dt, scores = gt[1:], dt[1:], scores[1:]          # the two images with rings
    sub = ("seeded_01", gt, dt, H, W, scores, None)
    want, unit = ref(sub), ref(("seeded_01_unit", gt, dt, H, W, None, None))
    g = E.pack_rings(gt, DEV)
    d0, d1 = dt

    def check(res, w):
        assert res["status"] == 0 and all(isinstance(res[k], float) for k in R.KEYS) and set(res["boundary"]) == set(R.KEYS)
        assert [res[k] for k in R.KEYS] == [w["named"]["segm"][k] for k in R.KEYS]
        assert [res["boundary"][k] for k in R.KEYS] == [w["named"]["boundary"][k] for k in R.KEYS]
        assert res["tables"]["precision"].is_cuda and np.array_equal(res["pairs"]["dt_match"].cpu().numpy(), w["dt_match"])

    check(E.coco_metrics(E.pack_rings(dt, DEV, scores=scores), g, H, W), want)

    # FFL: closed rings in (row, col); polygon 1 has a hole ring, polygon 2 was flagged by a filter; poly_prob is the score
    hole = C.f32([(11, 11), (13, 11), (13, 13)])
    rings = [d0[0], d0[1], hole, C.FAR, d0[2], d0[3], d1[0], d1[1], d1[2], d1[3]]
    ring_pos = np.concatenate([close(r)[:, ::-1] for r in rings]).astype(np.float32)
    ends = np.cumsum([len(r) + 1 for r in rings])
    prob = [scores[0][0], scores[0][1], 0.99, scores[0][2], scores[0][3]] + scores[1]
    ffl = {"ring_pos": torch.from_numpy(ring_pos).to(DEV), "ring_slice": torch.from_numpy(np.stack([ends - [len(r) + 1 for r in rings], ends], 1)).to(DEV),
           "poly_rings": torch.tensor([[0, 1], [1, 3], [3, 4], [4, 5], [5, 6], [6, 7], [7, 8], [8, 9], [9, 10]], device=DEV),
           "poly_batch": torch.tensor([0, 0, 0, 0, 0, 1, 1, 1, 1], dtype=torch.int32, device=DEV),
           "poly_flags": torch.tensor([0, 0, 2, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=DEV),
           "poly_prob": torch.tensor(prob, dtype=torch.float32, device=DEV), "batch_size": 2}
    got = E.rings_from_ffl(ffl)
    assert got["score"].tolist() == [float(np.float32(s)) for s in scores[0] + scores[1]]
    check(E.coco_metrics(got, g, H, W), want)
    assert "score" not in E.rings_from_ffl(ffl, unit_scores=True)
    check(E.coco_metrics(E.rings_from_ffl(ffl, unit_scores=True), g, H, W), unit)

    # HiSup: closed polygons in (x, y), poly_slice [B, R, 2]; region 1 of image 0 has no polygon (bit 2); the region score is the score
    polys = d0 + d1
    pos = np.concatenate([close(r) for r in polys]).astype(np.float32)
    ends = np.cumsum([len(r) + 1 for r in polys])
    sl = np.stack([ends - [len(r) + 1 for r in polys], ends], 1)
    poly_slice = np.zeros((2, 6, 2), np.int64)
    poly_slice[0, [0, 2, 3, 4]] = sl[:4]
    poly_slice[1, :4] = sl[4:]
    poly_slice[1, 4:] = [[0, 5]] * 2          # stale slots behind n_regions
    score = np.full((2, 6), 0.99, np.float32)
    score[0, [0, 2, 3, 4]] = scores[0]
    score[1, :4] = scores[1]
    hisup = {"polygons": {"pos": torch.from_numpy(pos).to(DEV), "poly_slice": torch.from_numpy(poly_slice).to(DEV),
                          "poly_flags": torch.tensor([[1, 4, 0, 2, 1, 0], [0, 1, 0, 0, 0, 0]], dtype=torch.int32, device=DEV)},
             "regions": {"n_regions": torch.tensor([5, 4], dtype=torch.int32, device=DEV), "score": torch.from_numpy(score).to(DEV)}}
    got = E.rings_from_hisup(hisup)
    assert got["score"].tolist() == [float(np.float32(s)) for s in scores[0] + scores[1]] and got["pos"].data_ptr() == hisup["polygons"]["pos"].data_ptr()
    check(E.coco_metrics(got, g, H, W), want)
    check(E.coco_metrics(E.rings_from_hisup(hisup, unit_scores=True), g, H, W), unit)
    segm = E.coco_metrics(got, g, H, W, iou_types=["segm"])
    assert segm["AP"] == want["named"]["segm"]["AP"] and all(np.isnan(v) for v in segm["boundary"].values())
    assert hip.coco_metrics_workspace_bytes(8, 8, 2, H, W) > hip.coco_metrics_workspace_bytes(8, 8, 2, H, W, hip.COCO_SEGM) > 0
