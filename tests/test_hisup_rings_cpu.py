"""The inner rings of the HiSup polygon step without a GPU: the restatement (tests/hisup_rings_ref.py) against the reference's own `get_poly_crowdai`
output (tests/golden/hisup_rings.npz), the hand values of include/p3hip.h, and the argument checks of the wrapper and of the C entry."""
import numpy as np
import pytest
import torch

from tests import hisup_polygon_ref as R
from tests import hisup_rings_ref as Q

NOJ = np.zeros((0, 2), np.float32)


def test_restatement_equals_the_reference_on_the_fixture():
    fg, juncs, polys = Q.load_fixture()
    labels, n_regions, _, Rr = R.region_inputs(fg)
    ju, cn = R.junction_inputs(juncs)
    outer, inner = R.polygons(labels, n_regions, ju, cn, Rr), Q.rings(labels, n_regions, ju, cn, Rr)
    assert sum(int(n) for n in n_regions) == len(polys)
    assert min(outer["margin_t"], inner["margin_t"]) >= 0.01 and min(outer["margin_d"], inner["margin_d"]) >= 1e-6      # the fixture conditions
    for (b, l), (want, parts) in polys.items():
        got, got_parts = Q.concatenated(outer, inner, b, l - 1)
        assert got.tobytes() == want.tobytes() and got_parts == parts, (b, l)
    per_region = inner["region_rings"][..., 1] - inner["region_rings"][..., 0]
    kept = inner["ring_counts"][0]
    assert kept >= 20 and int(inner["n_holes"].sum()) - kept >= 10 and int((per_region >= 2).sum()) >= 3 and int((inner["ring_flags"] & 1).sum()) >= 5
    assert not (inner["ring_flags"] & 4).any() and (inner["ring_area2"] >= 100).all()


def test_follower_with_s4_is_the_outer_border_of_the_polygon_restatement():
    for M in R.shape_set():
        ys, xs = np.nonzero(M)
        assert Q.follow(M, (int(xs[0]), int(ys[0])), 4) == R.outer_border(M)


@pytest.mark.parametrize("hw,area2,kept", [((6, 6), 94, 0), ((6, 7), 108, 1), ((3, 3), 28, 0)])
def test_hole_areas_and_the_threshold(hw, area2, kept):
    M = Q.block_with_holes(24, (2, 2, 14, 14), [(4, 4) + hw])
    holes, n = Q.holes_of(M)
    assert n == 1 and Q.area2(Q.hole_border(M, holes == 1)) == area2              # areas 47, 54 and 14
    n_holes, found = Q.region_rings(M, NOJ)
    assert n_holes == 1 and len(found) == kept


def test_hand_values_of_the_header():
    n, found = Q.region_rings(Q.hand_first(), NOJ)
    assert n == 1 and found[0]["area2"] == 108 and len(found[0]["ring"]) == 26 and found[0]["flags"] == 0
    assert found[0]["pos"].tolist() == [[12, 4], [12, 10], [5, 10], [5, 4], [12, 4]]
    n, found = Q.region_rings(Q.hand_wall(), NOJ)
    assert n == 2 and [f["area2"] for f in found] == [158, 176]                   # areas 79 and 88
    assert found[0]["pos"].tolist() == [[12, 4], [12, 12], [4, 12], [4, 4], [12, 4]]
    assert found[1]["pos"].tolist() == [[22, 4], [22, 12], [13, 12], [13, 4], [22, 4]]


def test_rings_have_unit_steps_and_stay_below_the_bound():
    fg = np.concatenate([Q.hand_set(), Q.disc_cases()[0]])
    labels, n_regions, _, _ = R.region_inputs(fg)
    seen = 0
    for b in range(len(fg)):
        for l in range(1, int(n_regions[b]) + 1):
            M = labels[b] == l
            holes, n = Q.holes_of(M)
            for f, h in zip(Q.region_rings(M, NOJ)[1], [h for h in range(1, n + 1) if Q.area2(Q.hole_border(M, holes == h)) >= 100]):
                ring = f["ring"]
                assert (np.abs(np.roll(ring, -1, axis=0) - ring).sum(axis=1) == 1).all()
                hole = np.pad(holes == h, 1)
                sides = sum(int((hole & ~np.roll(hole, s, axis=a)).sum()) for a in (0, 1) for s in (1, -1))
                assert len(ring) <= 2 * sides + 16                                    # the ring bound the capacities rest on (include/p3hip.h)
                seen += 1
    assert seen >= 10


def test_disc_cases_nothing_kept_junction_ring_and_two_matched():
    fg, juncs = Q.disc_cases()
    got = [Q.region_rings(fg[b], np.asarray(juncs[b], dtype=np.float32))[1][0] for b in range(3)]
    assert got[0]["flags"] == 5 and len(got[0]["src"]) == 0 and got[0]["margin_t"] >= 1.0
    assert got[1]["flags"] == 1 and len(got[1]["src"]) == 25 and sorted(got[1]["src"][:-1].tolist()) == list(range(24))
    assert got[2]["flags"] == 0 and len(got[2]["src"]) > 25


def test_wrapper_refuses_malformed_arguments_before_touching_a_device():
    from pixelspointspolygons_amd import hip
    lab = torch.zeros((2, 8, 8), dtype=torch.int32)
    n, bbox = torch.zeros(2, dtype=torch.int32), torch.zeros((2, 4, 4), dtype=torch.int32)
    ju, cn = torch.zeros((2, 600, 2)), torch.zeros((2, 2), dtype=torch.int32)
    with pytest.raises(hip.P3Error, match="no CPU path"):
        hip.hisup_polygon_rings_device(lab, n, bbox, ju, cn)                      # well-formed host tensors: there is no fallback
    for bad, what in (((lab.long(), n, bbox, ju, cn), "labels"), ((lab[0], n, bbox, ju, cn), "labels"), ((lab, n[:1], bbox, ju, cn), "n_regions"),
                      ((lab, n, bbox[:, :, :3], ju, cn), "bbox"), ((lab, n, bbox, ju[:, :300], cn), "juncs"), ((lab, n, bbox, ju, cn.long()), "junc_counts")):
        with pytest.raises(hip.P3Error, match=what):
            hip.hisup_polygon_rings_device(*bad)
    for k in ("max_vertices", "max_rings", "max_ring_vertices"):
        with pytest.raises(hip.P3Error, match=k):
            hip.hisup_polygon_rings_device(lab, n, bbox, ju, cn, **{k: 0})


def test_default_capacities_are_the_documented_bounds():
    from pixelspointspolygons_amd import hip
    assert hip.hisup_polygon_rings_capacity(2, 8, 8, 4) == (hip.hisup_polygons_capacity(2, 8, 8, 4), 2, 2 * (2 * (8 * 7 + 8 * 7) + 17))
    assert hip.hisup_polygon_rings_capacity(16, 224, 224, 64) == (hip.hisup_polygons_capacity(16, 224, 224, 64), 16 * 1003,
                                                                   16 * (2 * (224 * 223 + 224 * 223) + 17 * 1003))
    assert hip.hisup_polygon_rings_capacity(1, 5, 5, 1)[1:] == (1, 2 * (5 * 4 + 5 * 4))                       # no hole of area 50 fits: one slot each way


def test_c_entry_checks_arguments_without_a_device():
    from pixelspointspolygons_amd._lib import lib
    L = lib()
    args = [None] * 5 + [1, 8, 8, 4, 16, 2, 16, 0] + [None] * 19
    assert L.p3_hisup_polygons_rings(*args) == -1 and b"p3_hisup_polygons_rings" in L.p3_last_error_string()
    args[5] = 0
    assert L.p3_hisup_polygons_rings(*args) == 0                                  # B == 0: nothing to do, no launch
    assert L.p3_hisup_polygons_rings_workspace_bytes(2, 48, 48, 8, 1000, 10, 500) > L.p3_hisup_polygons_workspace_bytes(2, 48, 48, 8, 1000)
