"""Max tangent angle error on the device against the restatement tests/mta_ref.py.  States, pixel counts, the overlap report and
the counts are compared for equality: under the margins test_mta_cpu.py asserts for these inputs no mask pixel, sample count, nearest edge or stretch test
can legitimately differ.  The bounds of the figures:
  ring_cos    1e-11: with coordinates below 2^8 and about 16 roundings of 1.1e-16 relative, against edge lengths of at least 1, the error stays under
              5e-13; the bound leaves a factor of 20 over that
  ring_angle  the cos bound carried through acos: 2e-11 / sqrt(1 - c^2) where 1 - c^2 >= 1e-6, else 2 sqrt(2e-11) (near c = 1 acos is only Hoelder-1/2);
              and within 1e-12 of acos(min(1, ring_cos)) of the device's own cos
  MTA         the mean of the per-ring angle bounds, in degrees"""
import math

import numpy as np
import pytest
import torch

from tests import guard
from tests import mta_cases as C
from tests import mta_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
EXACT = ("ring_state", "ring_px", "image_overlap_px", "invalid_rings", "status", "counted")
PER_RING = ("ring_angle", "ring_cos", "ring_state", "ring_px")
PER_IMAGE = ("image_overlap_px", "invalid_rings")
_REF = {}


def ref(case):
    """the restatement of a case, computed once and shared"""
    name, gt, dt, H, W, params = case
    if name not in _REF:
        _REF[name] = R.run(gt, dt, H, W, **C.ref_params(params))
    return _REF[name]


def pack(case):
    from pixelspointspolygons_amd import eval_metrics as E
    return E.pack_rings(case[1], DEV), E.pack_rings(case[2], DEV)


def device(case, out=None, **override):
    from pixelspointspolygons_amd import hip
    _, gt, _, H, W, params = case
    g, d = pack(case)
    return hip.max_tangent_angle_device(g["pos"], g["ring_slice"], g["ring_image"], d["pos"], d["ring_slice"], d["ring_image"], len(gt), H, W,
                                        **dict(params, **override), out=out)


def to_host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def bits(a):
    return a.view(np.int64) if a.dtype == np.float64 else a


def angle_bounds(c):
    s2 = 1.0 - c * c
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(s2 >= 1e-6, 2e-11 / np.sqrt(np.maximum(s2, 1e-6)), 2.0 * math.sqrt(2e-11))


def compare(got, want):
    for k in EXACT:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (k, got[k].tolist()[:40], want[k].tolist()[:40])
    on = want["ring_state"] == R.COUNTED
    for k in ("ring_cos", "ring_angle"):
        assert got[k].shape == on.shape and np.isnan(got[k][~on]).all() and not np.isnan(got[k][on]).any(), k
    c, a = got["ring_cos"][on], got["ring_angle"][on]
    err = np.abs(c - want["ring_cos"][on])
    print("ring_cos: max error", err.max(initial=0.0))
    assert (err <= 1e-11).all(), (err.max(), int(err.argmax()))
    bound = angle_bounds(want["ring_cos"][on])
    err = np.abs(a - want["ring_angle"][on])
    print("ring_angle: max error", err.max(initial=0.0), "max error / bound", (err / bound).max(initial=0.0))
    assert (err <= bound).all(), (err.max(), int((err / bound).argmax()))
    own = np.abs(a - np.arccos(np.minimum(1.0, c)))
    print("ring_angle against acos of the device's cos: max", own.max(initial=0.0))
    assert (own <= 1e-12).all(), own.max()
    if on.any():
        tol = math.degrees(float(bound.mean()))
        print("MTA", got["mta"][0], "restatement", want["mta"][0], "bound", tol)
        assert abs(got["mta"][0] - want["mta"][0]) <= tol
    else:
        assert np.isnan(got["mta"]).all() and np.isnan(want["mta"]).all()
    mean, n = R.set_mean(got["ring_angle"], got["ring_state"])          # the set mean from the device's own angles in ring order, bit for bit
    assert n == got["counted"][0] and np.array_equal(bits(np.array([mean])), bits(got["mta"]))


@pytest.mark.parametrize("case", C.all_cases(), ids=lambda c: c[0])
def test_cases_against_the_restatement(case):
    compare(to_host(device(case)), ref(case))


def test_hand_values_on_the_device():
    o = to_host(device(C.case("hand_1")))
    want = 45.0 - math.degrees(math.atan(1.0 / 8.0))
    assert o["ring_px"].tolist() == [[256, 256], [256, 208], [240, 240]] and o["ring_cos"][:2].tolist() == [1.0, 1.0] and np.abs(o["ring_angle"][:2]).max() <= 1e-12
    assert abs(math.degrees(o["ring_angle"][2]) - want) <= 1e-9 and abs(o["mta"][0] - want / 3.0) <= 1e-9 and o["counted"].tolist() == [3]
    o = to_host(device(C.case("hand_3")))
    assert o["status"].tolist() == [5] and o["image_overlap_px"].tolist() == [0, 256, 0] and o["ring_state"].tolist() == [1, 1, 0, 1, 0, 0] and abs(o["mta"][0]) <= 1e-10
    o = to_host(device(C.case("hand_empty")))
    assert np.isnan(o["mta"][0]) and o["counted"].tolist() == [0] and o["status"].tolist() == [0] and o["ring_state"].shape == (0,)


def test_the_three_parameters_arrive():
    from pixelspointspolygons_amd import hip
    base = C.case("hand_1")
    o = to_host(device(base, min_precision=0.9))
    assert o["ring_state"].tolist() == [0, hip.MTA_BELOW_PRECISION, 0] and o["counted"].tolist() == [2]
    compare(o, ref(C.case("hand_1_precision_0.9")))
    compare(to_host(device(base, sampling_spacing=0.5)), ref(C.case("hand_1_spacing_0.5")))
    assert ref(C.case("hand_1_spacing_0.5"))["mta"][0] != ref(base)["mta"][0]          # the finer line sees the moved corner at another angle
    o = to_host(device(base, max_stretch=4.0))
    assert abs(o["ring_cos"][1] - 0.8) <= 1e-15 and to_host(device(base))["ring_cos"][1] == 1.0
    compare(o, ref(C.case("hand_1_stretch_4")))
    o = to_host(device(C.case("no_valid_edge_stretch_1.2")))
    assert o["ring_state"].tolist() == [hip.MTA_NO_EDGE, hip.MTA_COUNTED]
    assert to_host(device(C.case("no_valid_edge_stretch_1.2"), max_stretch=2.0))["ring_state"].tolist() == [0, 0]


def test_two_runs_and_an_image_alone_give_the_same_bits():
    for case in (C.case("seeded_012"), C.case("hand_3"), C.case("64x31"), C.case("gt_only_empty_pred_only")):
        name, gt, dt, H, W, params = case
        a, b = to_host(device(case)), to_host(device(case))
        for k in a:
            assert np.array_equal(bits(a[k]), bits(b[k])), (name, k)
        at = 0
        for i in range(len(gt)):
            o = to_host(device((f"{name}_{i}", [gt[i]], [dt[i]], H, W, params)))
            n = len(dt[i])
            for k in PER_RING:
                assert np.array_equal(bits(o[k]), bits(a[k][at:at + n])), (name, k, i)
            for k in PER_IMAGE:
                assert np.array_equal(o[k][0], a[k][i]), (name, k, i)
            at += n


def test_outputs_in_guard_bands():
    from pixelspointspolygons_amd import hip
    for name in ("seeded_345", "hand_3", "chunks_224x224", "no_valid_edge_stretch_1.2"):
        case = C.case(name)
        got = to_host(guard.guarded_run(lambda out=None: device(case, out=out)))
        compare(got, ref(case))
    fn = lambda out=None: device(C.case("hand_1"), out=out)
    with pytest.raises(hip.P3Error, match="ring_cos"):
        fn(out={"ring_cos": torch.zeros(4, dtype=torch.float64, device=DEV)})
    with pytest.raises(hip.P3Error, match="no"):
        fn(out={"metrics": torch.zeros(1, dtype=torch.float64, device=DEV)})


def test_rings_that_are_left_out_are_flagged():
    from pixelspointspolygons_amd import eval_metrics as E
    case = C.case("seeded_012")
    _, gt, dt, H, W, _ = case
    want = ref(case)
    g, d = pack(case)
    n = d["ring_slice"].shape[0]
    V = d["pos"].shape[0]
    extra = dict(d, ring_slice=torch.cat([d["ring_slice"], torch.tensor([[0, 4], [V - 2, V + 2]], device=DEV)]),          # image 3 of 3; a slice past pos
                 ring_image=torch.cat([d["ring_image"], torch.tensor([3, 3], dtype=torch.int32, device=DEV)]))
    res = E.max_tangent_angle(extra, g, H, W)
    assert res["status"] == 2 and res["counted"] == want["counted"][0]
    assert np.array_equal(bits(np.array([res["MTA"]])), bits(to_host(device(case))["mta"]))
    got = to_host(dict(res["per_ring"], **res["per_image"]))
    assert np.array_equal(got["state"][:n], want["ring_state"]) and got["state"][n:].tolist() == [1, 1] and np.array_equal(got["px"][:n], want["ring_px"])
    assert not got["px"][n:].any() and np.isnan(got["angle"][n:]).all() and np.isnan(got["cos"][n:]).all()
    assert np.array_equal(got["overlap_px"], want["image_overlap_px"]) and np.array_equal(got["invalid_rings"], want["invalid_rings"])
    last = dict(d, ring_slice=torch.cat([d["ring_slice"], torch.tensor([[V - 2, V + 2]], device=DEV)]),
                ring_image=torch.cat([d["ring_image"], torch.tensor([2], dtype=torch.int32, device=DEV)]))          # image 2 of 3, but the slice ends behind pos
    res = E.max_tangent_angle(last, g, H, W)
    assert res["status"] == 2 and res["per_ring"]["state"].tolist()[n:] == [1] and res["per_image"]["invalid_rings"].tolist() == want["invalid_rings"].tolist()
    gt_extra = dict(g, ring_slice=torch.cat([g["ring_slice"], torch.tensor([[0, 4]], device=DEV)]),
                    ring_image=torch.cat([g["ring_image"], torch.tensor([3], dtype=torch.int32, device=DEV)]))
    res = E.max_tangent_angle(d, gt_extra, H, W)
    assert res["status"] == 2 and np.array_equal(bits(res["per_ring"]["cos"].cpu().numpy()), bits(to_host(device(case))["ring_cos"]))


def test_the_public_function_on_converted_ring_sets():
    from pixelspointspolygons_amd import eval_metrics as E
    close = lambda r: np.concatenate([r, r[:1]])
    name, gt, dt, H, W, _ = C.case("seeded_012")
    gt, dt = gt[:2], dt[:2]
    want = ref(("seeded_01", gt, dt, H, W, {}))
    g = E.pack_rings(gt, DEV, areas=[[1.0] * len(x) for x in gt])          # a score or area field is ignored
    d0, d1 = dt
    base = E.max_tangent_angle(E.pack_rings(dt, DEV, scores=[[0.5] * len(x) for x in dt]), g, H, W)
    compare(to_host({"mta": torch.tensor([base["MTA"]], dtype=torch.float64), "counted": torch.tensor([base["counted"]], dtype=torch.int32),
                     "status": torch.tensor([base["status"]], dtype=torch.int32), "ring_angle": base["per_ring"]["angle"], "ring_cos": base["per_ring"]["cos"],
                     "ring_state": base["per_ring"]["state"], "ring_px": base["per_ring"]["px"], "image_overlap_px": base["per_image"]["overlap_px"],
                     "invalid_rings": base["per_image"]["invalid_rings"]}), want)
    assert isinstance(base["MTA"], float) and isinstance(base["counted"], int) and isinstance(base["status"], int)
    assert all(t.is_cuda for t in list(base["per_ring"].values()) + list(base["per_image"].values()))

    def check(res):
        assert res["MTA"] == base["MTA"] and res["counted"] == base["counted"] and res["status"] == base["status"] and isinstance(res["MTA"], float)
        for k in base["per_ring"]:
            assert res["per_ring"][k].is_cuda and np.array_equal(bits(res["per_ring"][k].cpu().numpy()), bits(base["per_ring"][k].cpu().numpy())), k
        for k in base["per_image"]:
            assert res["per_image"][k].is_cuda and np.array_equal(res["per_image"][k].cpu().numpy(), base["per_image"][k].cpu().numpy()), k

    # FFL: closed rings in (row, col); polygon 1 has a hole ring, polygon 2 was flagged by a filter
    hole = C.f32([(11, 11), (13, 11), (13, 13)])
    rings = [d0[0], d0[1], hole, C.FAR, d0[2], d0[3], d1[0], d1[1], d1[2], d1[3]]
    ring_pos = np.concatenate([close(r)[:, ::-1] for r in rings]).astype(np.float32)
    ends = np.cumsum([len(r) + 1 for r in rings])
    ffl = {"ring_pos": torch.from_numpy(ring_pos).to(DEV), "ring_slice": torch.from_numpy(np.stack([ends - [len(r) + 1 for r in rings], ends], 1)).to(DEV),
           "poly_rings": torch.tensor([[0, 1], [1, 3], [3, 4], [4, 5], [5, 6], [6, 7], [7, 8], [8, 9], [9, 10]], device=DEV),
           "poly_batch": torch.tensor([0, 0, 0, 0, 0, 1, 1, 1, 1], dtype=torch.int32, device=DEV),
           "poly_flags": torch.tensor([0, 0, 2, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=DEV),
           "poly_prob": torch.full((9,), 0.7, dtype=torch.float32, device=DEV), "batch_size": 2}
    check(E.max_tangent_angle(E.rings_from_ffl(ffl), g, H, W))
    check(E.max_tangent_angle(E.rings_from_ffl(ffl, unit_scores=True), g, H, W))

    # HiSup: closed polygons in (x, y), poly_slice [B, R, 2]; region 1 of image 0 has no polygon (bit 2)
    polys = d0 + d1
    pos = np.concatenate([close(r) for r in polys]).astype(np.float32)
    ends = np.cumsum([len(r) + 1 for r in polys])
    sl = np.stack([ends - [len(r) + 1 for r in polys], ends], 1)
    poly_slice = np.zeros((2, 6, 2), np.int64)
    poly_slice[0, [0, 2, 3, 4]] = sl[:4]
    poly_slice[1, :4] = sl[4:]
    poly_slice[1, 4:] = [[0, 5]] * 2          # stale slots behind n_regions
    hisup = {"polygons": {"pos": torch.from_numpy(pos).to(DEV), "poly_slice": torch.from_numpy(poly_slice).to(DEV),
                          "poly_flags": torch.tensor([[1, 4, 0, 2, 1, 0], [0, 1, 0, 0, 0, 0]], dtype=torch.int32, device=DEV)},
             "regions": {"n_regions": torch.tensor([5, 4], dtype=torch.int32, device=DEV), "score": torch.full((2, 6), 0.9, device=DEV)}}
    check(E.max_tangent_angle(E.rings_from_hisup(hisup), g, H, W))

    # Pix2Poly: per tile a list of host tensors
    check(E.max_tangent_angle(E.rings_from_pix2poly([[torch.from_numpy(r) for r in rs] for rs in dt], DEV), g, H, W))
