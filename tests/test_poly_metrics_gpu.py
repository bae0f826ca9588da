"""Polygon metrics on the device against the float64 restatement tests/poly_metrics_ref.py: matches, flags and pixel counts equal, the
figures to 1e-9 absolute.  The bound follows from double rounding: eps = 1.1e-16 times coordinates below 2^10 times sums of a few thousand terms stays under
1e-9; under the margins test_poly_metrics_cpu.py asserts for these inputs no sample count, argmax or pixel can legitimately differ."""
import numpy as np
import pytest
import torch

from tests import guard
from tests import poly_metrics_cases as C
from tests import poly_metrics_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
EXACT = ("match", "image_valid", "invalid_rings", "status", "image_counts")
CLOSE = ("pair_polis", "pair_chamfer", "pair_hausdorff", "image_iou", "image_nr", "image_polis", "image_chamfer", "image_hausdorff", "metrics")
PER_IMAGE = ("image_iou", "image_nr", "image_polis", "image_chamfer", "image_hausdorff", "image_valid", "image_counts", "invalid_rings")
PER_PAIR = ("pair_polis", "pair_chamfer", "pair_hausdorff")
_REF = {}


def ref(case):
    """the restatement of a case, computed once and shared"""
    name, gt, dt, H, W = case
    if name not in _REF:
        _REF[name] = R.run(gt, dt, H, W)
    return _REF[name]


def device(gt, dt, H, W, **kw):
    from pixelspointspolygons_amd import eval_metrics as E, hip
    g, d = E.pack_rings(gt, DEV), E.pack_rings(dt, DEV)
    return hip.polygon_metrics_device(g["pos"], g["ring_slice"], g["ring_image"], d["pos"], d["ring_slice"], d["ring_image"], len(gt), H, W, **kw)


def to_host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def compare(got, want):
    for k in EXACT:
        assert np.array_equal(got[k], want[k]), (k, got[k].tolist(), want[k].tolist())
    for k in CLOSE:
        assert got[k].shape == want[k].shape and np.array_equal(np.isnan(got[k]), np.isnan(want[k])), (k, got[k].tolist(), want[k].tolist())
        err = np.nan_to_num(np.abs(got[k] - want[k]))
        assert err.max(initial=0.0) <= 1e-9, (k, float(err.max()), got[k].tolist(), want[k].tolist())


def bits(a):
    return a.view(np.uint8) if a.dtype != np.int32 else a


@pytest.mark.parametrize("case", C.hand_cases() + C.seeded_cases(), ids=lambda c: c[0])
def test_hand_and_seeded_images_equal_the_restatement(case):
    _, gt, dt, H, W = case
    assert len(gt) == 3
    compare(to_host(device(gt, dt, H, W)), ref(case))


@pytest.mark.parametrize("case", C.shape_cases(), ids=lambda c: c[0])
def test_shapes_at_which_the_kernels_take_another_path(case):
    from pixelspointspolygons_amd import hip
    name, gt, dt, H, W = case
    if name == "long_ring_64x64":
        assert len(gt[0][0]) > hip.PM_EDGE_CHUNK and len(R.samples(gt[0][0])) > hip.PM_TILE
    compare(to_host(device(gt, dt, H, W)), ref(case))


def test_more_rings_and_images_than_a_workgroup_has_threads():
    from pixelspointspolygons_amd import hip
    case = C.many_rings_case()
    _, gt, dt, H, W = case
    assert len(gt[0]) > 256 and len(gt) > 256          # the second workgroup of the ring kernel, the strided loops of the match and finish kernels
    want = ref(case)
    assert int((want["match"] >= 0).sum()) > 256
    compare(to_host(device(gt, dt, H, W)), want)
    part = to_host(device(gt, dt, H, W, modes=hip.PM_IOU | hip.PM_POLIS))
    assert np.array_equal(part["match"], want["match"]) and np.array_equal(part["image_counts"], want["image_counts"])
    for k in ("pair_polis", "image_polis", "image_iou", "image_nr"):
        assert np.array_equal(np.isnan(part[k]), np.isnan(want[k])) and np.nan_to_num(np.abs(part[k] - want[k])).max() <= 1e-9, k
    assert np.isnan(part["pair_chamfer"]).all() and np.isnan(part["metrics"][4:]).all() and abs(part["metrics"][3] - want["metrics"][3]) <= 1e-9


def test_hand_values_on_the_device():
    o = to_host(device([[C.SQUARE_A], [C.SQUARE_A]], [[C.SQUARE_A], [C.SQUARE_B]], 48, 48))
    assert o["image_counts"].tolist() == [[256, 256], [208, 304]] and o["match"].tolist() == [0, 1]
    assert o["pair_polis"][0] == 0 and o["pair_chamfer"][0] == 0 and o["pair_hausdorff"][0] == 0
    assert abs(o["pair_polis"][1] - 1.2) <= 1e-12 and 3.0 <= o["pair_hausdorff"][1] <= np.sqrt(9 + 0.05 ** 2)


def test_rings_with_unusable_coordinates_are_invalid():
    bad = [np.array([(8, 8), (24, 8), (v, 24)], np.float32) for v in (float("nan"), float("inf"), -float("inf"), 1e30, 32769.0)]
    edge = np.array([(8, 8), (32768, 8), (24, 24)], np.float32)          # the bound itself is valid; far outside the image, and matched by nothing
    gt, dt = [[bad[0], C.SQUARE_A, bad[3]], [edge]], [[bad[1], C.SQUARE_B, bad[2], bad[4]], []]
    want = R.run(gt, dt, 48, 48)
    assert want["invalid_rings"].tolist() == [[2, 3], [0, 0]] and want["match"].tolist() == [-1, 1, -1, -1] and want["status"].tolist() == [1]
    compare(to_host(device(gt, dt, 48, 48)), want)


def test_two_runs_and_an_image_alone_give_the_same_bits():
    for case in (C.case("seeded_012"), C.case("long_ring_64x64"), C.case("gt_only_empty_pred_only")):
        _, gt, dt, H, W = case
        a, b = to_host(device(gt, dt, H, W)), to_host(device(gt, dt, H, W))
        for k in a:
            assert np.array_equal(bits(a[k]), bits(b[k])), k
        g_at = d_at = 0
        alone = []
        for i in range(len(gt)):
            o = to_host(device([gt[i]], [dt[i]], H, W))
            alone.append(o)
            for k in PER_IMAGE:
                assert np.array_equal(bits(o[k][:1]), bits(a[k][i:i + 1])), (k, i)
            n = len(gt[i])
            for k in PER_PAIR:
                assert np.array_equal(bits(o[k]), bits(a[k][g_at:g_at + n])), (k, i)
            m = a["match"][g_at:g_at + n]
            assert np.array_equal(o["match"], np.where(m >= 0, m - d_at, -1)), i
            g_at, d_at = g_at + n, d_at + len(dt[i])
        merged = {k: np.concatenate([o[k] for o in alone]) for k in PER_IMAGE}          # the per-set means, recomputed from the images alone
        assert np.array_equal(bits(R.set_means(merged)), bits(a["metrics"]))


def test_outputs_in_guard_bands():
    from pixelspointspolygons_amd import eval_metrics as E, hip
    for case in (C.case("hand_2"), C.case("64x31")):
        _, gt, dt, H, W = case
        g, d = E.pack_rings(gt, DEV), E.pack_rings(dt, DEV)
        fn = lambda out=None: hip.polygon_metrics_device(g["pos"], g["ring_slice"], g["ring_image"], d["pos"], d["ring_slice"], d["ring_image"], len(gt), H, W,
                                                          out=out)
        got = to_host(guard.guarded_run(fn))
        compare(got, ref(case))
        off = got["match"] < 0          # uncounted rings hold exactly -1 / NaN
        assert np.array_equal(got["match"][off], np.full(int(off.sum()), -1))
        for k in PER_PAIR:
            assert np.isnan(got[k][off]).all() and not np.isnan(got[k][~off]).any()
    with pytest.raises(hip.P3Error, match="metrics"):
        fn(out={"metrics": torch.zeros(5, dtype=torch.float64, device=DEV)})
    with pytest.raises(hip.P3Error, match="no"):
        fn(out={"means": torch.zeros(6, dtype=torch.float64, device=DEV)})


def test_modes_and_the_public_function():
    from pixelspointspolygons_amd import eval_metrics as E, hip
    case = C.case("seeded_345")
    _, gt, dt, H, W = case
    want = ref(case)
    g, d = E.pack_rings(gt, DEV), E.pack_rings(dt, DEV)
    full = E.polygon_metrics(d, g, H, W)
    assert set(R.KEYS) <= set(full) and all(isinstance(full[k], float) for k in R.KEYS) and full["status"] == 0
    for k in R.KEYS:
        assert abs(full[k] - want["means"][k]) <= 1e-9, k
    assert np.array_equal(full["pairs"]["match"].cpu().numpy(), want["match"]) and full["per_image"]["iou"].is_cuda
    iou = E.polygon_metrics(d, g, H, W, modes=("iou",))
    assert all(iou[k] == full[k] for k in ("IoU", "C-IoU", "NR")) and all(np.isnan(iou[k]) for k in ("POLIS", "chamfer", "hausdorff"))
    assert np.array_equal(iou["pairs"]["match"].cpu().numpy(), want["match"]) and torch.isnan(iou["pairs"]["polis"]).all()
    points = E.polygon_metrics(d, g, H, W, modes=("polis", "hausdorff"))
    assert all(points[k] == full[k] for k in ("POLIS", "chamfer", "hausdorff")) and all(np.isnan(points[k]) for k in ("IoU", "C-IoU", "NR"))
    assert int(points["per_image"]["counts"].abs().sum()) == 0 and torch.isnan(points["per_image"]["nr"]).all() and torch.isnan(points["per_image"]["iou"]).all()
    assert torch.equal(points["per_image"]["valid"], full["per_image"]["valid"]) and torch.equal(points["pairs"]["match"], full["pairs"]["match"])
    polis = E.polygon_metrics(d, g, H, W, modes=["polis"])
    assert polis["POLIS"] == full["POLIS"] and np.isnan(polis["chamfer"]) and np.isnan(polis["hausdorff"])
    assert hip.polygon_metrics_workspace_bytes(len(want["match"]), d["ring_slice"].shape[0], 3) > 0


def test_rings_that_are_left_out_are_flagged():
    from pixelspointspolygons_amd import eval_metrics as E
    case = C.case("hand_1")
    _, gt, dt, H, W = case
    want = ref(case)
    g, d = E.pack_rings(gt, DEV), E.pack_rings(dt, DEV)
    extra = dict(d, ring_slice=torch.cat([d["ring_slice"], torch.tensor([[0, 4], [6, 9]], device=DEV)]),
                 ring_image=torch.cat([d["ring_image"], torch.tensor([3, 3], dtype=torch.int32, device=DEV)]))          # image 3 of 3; and a slice past pos too
    res = E.polygon_metrics(extra, g, H, W)
    assert res["status"] == 2 and int(res["per_image"]["invalid_rings"].sum()) == 0
    for k in ("IoU", "C-IoU", "NR", "POLIS", "chamfer", "hausdorff"):
        assert abs(res[k] - want["means"][k]) <= 1e-9
    past = dict(d, ring_slice=torch.tensor([[0, 4], [4, 9]], device=DEV))          # the second ring ends behind pos [8, 2]
    res = E.polygon_metrics(past, g, H, W)
    assert res["status"] == 2 and res["pairs"]["match"].tolist() == [0, -1]


def test_converters_give_the_ring_set_of_pack_rings():
    from pixelspointspolygons_amd import eval_metrics as E
    close = lambda r: np.concatenate([r, r[:1]])
    g0, d0 = C.seeded_image(C.SEEDS[0])
    g1, d1 = C.seeded_image(C.SEEDS[1])
    gt = E.pack_rings([g0, g1], DEV)
    want = E.pack_rings([d0, d1[:2]], DEV)
    same = lambda got: (got["batch_size"] == 2 and torch.equal(got["ring_image"], want["ring_image"]) and got["ring_image"].dtype == torch.int32
                        and [got["pos"][a:b].tolist() for a, b in got["ring_slice"].tolist()] == [want["pos"][a:b].tolist() for a, b in want["ring_slice"].tolist()])
    base = E.polygon_metrics(want, gt, 48, 48)

    # FFL: closed rings in (row, col); polygon 1 has a hole ring, polygon 2 was flagged by a filter
    hole = C.f32([(11, 11), (13, 11), (13, 13)])
    rings = [d0[0], d0[1], hole, C.FAR, d0[2], d0[3], d1[0], d1[1]]
    ring_pos = np.concatenate([close(r)[:, ::-1] for r in rings]).astype(np.float32)
    ends = np.cumsum([len(r) + 1 for r in rings])
    ffl = {"ring_pos": torch.from_numpy(ring_pos).to(DEV), "ring_slice": torch.from_numpy(np.stack([ends - [len(r) + 1 for r in rings], ends], 1)).to(DEV),
           "poly_rings": torch.tensor([[0, 1], [1, 3], [3, 4], [4, 5], [5, 6], [6, 7], [7, 8]], device=DEV),
           "poly_batch": torch.tensor([0, 0, 0, 0, 0, 1, 1], dtype=torch.int32, device=DEV),
           "poly_flags": torch.tensor([0, 0, 2, 0, 0, 0, 0], dtype=torch.int32, device=DEV), "batch_size": 2}
    got = E.rings_from_ffl(ffl)
    assert same(got) and got["pos"].is_cuda
    res = E.polygon_metrics(got, gt, 48, 48)
    assert all(res[k] == base[k] for k in R.KEYS)

    # HiSup: closed polygons in (x, y), poly_slice [B, R, 2]; region 1 of image 0 has no polygon (bit 2), image 1 has two regions of four slots
    polys = [d0[0], d0[1], d0[2], d0[3], d1[0], d1[1]]
    pos = np.concatenate([close(r) for r in polys]).astype(np.float32)
    ends = np.cumsum([len(r) + 1 for r in polys])
    sl = np.stack([ends - [len(r) + 1 for r in polys], ends], 1)
    poly_slice = np.zeros((2, 5, 2), np.int64)
    poly_slice[0, [0, 2, 3, 4]] = sl[:4]
    poly_slice[1, :2] = sl[4:]
    poly_slice[1, 2:] = [[0, 5]] * 3          # stale slots behind n_regions
    hisup = {"polygons": {"pos": torch.from_numpy(pos).to(DEV), "poly_slice": torch.from_numpy(poly_slice).to(DEV),
                          "poly_flags": torch.tensor([[1, 4, 0, 2, 1], [0, 1, 0, 0, 0]], dtype=torch.int32, device=DEV)},
             "regions": {"n_regions": torch.tensor([5, 2], dtype=torch.int32, device=DEV)}}
    got = E.rings_from_hisup(hisup)
    assert same(got) and got["pos"].data_ptr() == hisup["polygons"]["pos"].data_ptr()
    res = E.polygon_metrics(got, gt, 48, 48)
    assert all(res[k] == base[k] for k in R.KEYS)
    host = E.rings_from_hisup({"polys_pred": [[close(r).astype(np.float64) for r in d0], [close(r).astype(np.float64) for r in d1[:2]]]}, DEV)
    assert same(host) and torch.equal(host["ring_slice"], want["ring_slice"])

    # Pix2Poly: per tile a list of [n, 2] (x, y) host tensors
    got = E.rings_from_pix2poly([[torch.from_numpy(r) for r in d0], [torch.from_numpy(r) for r in d1[:2]]], DEV)
    assert same(got) and torch.equal(got["pos"], want["pos"])
