"""The HiSup polygon step without a GPU: the restatement (tests/hisup_polygon_ref.py) against the reference's own `get_poly_crowdai` output
(tests/golden/hisup_polygon.npz), closed-form cases of the ring, and the wrapper's argument checks."""
import numpy as np
import pytest
import torch

from tests import hisup_polygon_ref as R

NOJ = np.zeros((0, 2), np.float32)


def test_restatement_equals_the_reference_on_the_fixture():
    fg, juncs, polys = R.load_fixture()
    labels, n_regions, _, _ = R.region_inputs(fg)
    assert sum(int(n) for n in n_regions) == len(polys) >= 200
    n_junc = 0
    for (b, l), want in polys.items():
        got = R.region_polygon(labels[b] == l, juncs[b])
        assert got["margin_t"] >= 0.01 and got["margin_d"] >= 1e-6                # the fixture conditions
        assert got["pos"].astype(np.float64).tobytes() == want.tobytes(), (b, l)
        assert (len(want) == 0) == bool(got["flags"] & 4)
        n_junc += got["flags"] & 1
    assert n_junc >= 100                                                          # both kinds of polygon are in the fixture


def test_rectangle_starts_at_its_top_left_corner_and_goes_down():
    for (y, x, h, w) in ((2, 3, 3, 5), (0, 0, 1, 7), (5, 1, 6, 1)):
        p = R.region_polygon(R.rect(12, y, x, h, w), NOJ)
        assert p["pos"].tolist() == [[x, y], [x, y + h], [x + w, y + h], [x + w, y], [x, y]] and p["flags"] == 0
        assert len(p["ring"]) == 2 * (h + w) and p["src"].tolist() == [0, h, h + w, 2 * h + w, 0]


@pytest.mark.parametrize("mask,vertices,area", [(R.rect(12, 4, 4, 1, 1), 4, 1), (R.shape_l(), 6, 18), (R.shape_diagonal(k=5), 20, 5)])
def test_vertex_counts_of_pixel_l_and_diagonal(mask, vertices, area):
    p = R.region_polygon(mask, NOJ)
    assert len(p["src"]) == vertices + 1 and np.array_equal(p["pos"][0], p["pos"][-1])
    assert R.shoelace(p["ring"]) == area == int(mask.sum())


def test_every_ring_has_unit_steps_and_encloses_the_filled_region():
    fg = np.concatenate([R.shape_set(), R.junction_cases()[0]])
    labels, n_regions, _, _ = R.region_inputs(fg)
    seen = plain = 0
    for b in range(len(fg)):
        for l in range(1, int(n_regions[b]) + 1):
            M = labels[b] == l
            ring, holes = R.ring_of(M)
            assert (np.abs(np.roll(ring, -1, axis=0) - ring).sum(axis=1) == 1).all()
            F = R.fill(M)
            T = R.corner_grid(F)
            if np.array_equal(T[:-1, :-1] & T[1:, :-1] & T[:-1, 1:] & T[1:, 1:], F):      # no pixel outside F has all four corners in T: step B closed no gap
                assert R.shoelace(ring) == int(F.sum()) == int(M.sum()) + holes
                plain += 1
            sides = sum(int((M & ~np.roll(np.pad(M, 1), s, axis=a)[1:-1, 1:-1]).sum()) for a in (0, 1) for s in (1, -1))
            assert len(ring) <= 2 * (sides + 4)                                   # the ring bound the capacities rest on (include/p3hip.h)
            seen += 1
    assert seen >= 50 and plain >= 20


def test_u_with_a_one_pixel_gap_is_closed_by_the_corner_grid():
    """the gap between the arms is filled by step B, so the ring is the box: 15 pixels (3 wide, 7 tall) enclose 21, 21 pixels (5 x 5, arms 2 wide) enclose 25"""
    for arm, height, pixels, area in ((1, 7, 15, 21), (2, 5, 21, 25)):
        m = R.shape_u(arm=arm, height=height)
        p = R.region_polygon(m, NOJ)
        assert int(m.sum()) == pixels and R.shoelace(p["ring"]) == area and len(p["src"]) == 5 and p["hole_pixels"] == 0


def test_ring_with_a_hole_is_flagged_and_keeps_its_outer_polygon():
    m = R.rect(12, 2, 2, 7, 7)
    m[4:7, 4:7] = False
    p = R.region_polygon(m, NOJ)
    assert p["flags"] == 2 and p["hole_pixels"] == 9 and p["pos"].tolist() == [[2, 2], [2, 9], [9, 9], [9, 2], [2, 2]]


def test_junction_cases_two_three_and_equal_coordinates():
    fg, juncs = R.junction_cases()
    labels, n_regions, _, Rr = R.region_inputs(fg)
    ju, counts = R.junction_inputs(juncs)
    out = R.polygons(labels, n_regions, ju, counts, Rr)
    assert out["poly_flags"][0, :2].tolist() == [0, 0]                            # no junctions
    # two matched junctions: the ring; three: the junctions; three junctions at one point: the lowest index takes every vote, so the ring again
    assert out["poly_flags"][1, :3].tolist() == [0, 1, 0]
    s = out["poly_slice"][1, 1]
    assert out["src"][s[0]:s[1]].tolist() == [2, 4, 3, 2] and np.array_equal(out["pos"][s[0]:s[1] - 1], ju[1, [2, 4, 3]])
    assert counts[2].sum() == 600 and (out["poly_flags"][2, :n_regions[2]] & 1).sum() >= 10


def test_smooth_junction_polygon_keeps_no_vertex():
    """45 junctions on the rim of a disc: every turn is 8 degrees and the wrap from 180 to -180 gives 352, so `simple_polygon` keeps nothing - the
    reference raises there, here the region has no polygon (flag bits 0 and 2); with 24 junctions (15 degrees) every junction is kept"""
    fg, juncs = R.smooth_cases()
    got = [R.region_polygon(fg[b], np.asarray(juncs[b], dtype=np.float32)) for b in range(3)]
    assert got[0]["flags"] == 5 and len(got[0]["src"]) == 0 and got[0]["margin_t"] >= 1.0
    assert got[1]["flags"] == 1 and len(got[1]["src"]) == 25 and sorted(got[1]["src"][:-1].tolist()) == list(range(24))
    assert got[2]["flags"] == 0 and len(got[2]["src"]) > 25


def test_wrapper_refuses_malformed_arguments_before_touching_a_device():
    from pixelspointspolygons_amd import hip
    lab = torch.zeros((2, 8, 8), dtype=torch.int32)
    n, bbox = torch.zeros(2, dtype=torch.int32), torch.zeros((2, 4, 4), dtype=torch.int32)
    ju, cn = torch.zeros((2, 600, 2)), torch.zeros((2, 2), dtype=torch.int32)
    with pytest.raises(hip.P3Error, match="no CPU path"):
        hip.hisup_polygons_device(lab, n, bbox, ju, cn)                           # well-formed host tensors: there is no fallback
    for bad, what in (((lab.long(), n, bbox, ju, cn), "labels"), ((lab[0], n, bbox, ju, cn), "labels"), ((lab, n[:1], bbox, ju, cn), "n_regions"),
                      ((lab, n, bbox[:, :, :3], ju, cn), "bbox"), ((lab, n, bbox, ju[:, :300], cn), "juncs"), ((lab, n, bbox, ju, cn.long()), "junc_counts")):
        with pytest.raises(hip.P3Error, match=what):
            hip.hisup_polygons_device(*bad)
    with pytest.raises(hip.P3Error, match="max_vertices"):
        hip.hisup_polygons_device(lab, n, bbox, ju, cn, max_vertices=0)
    assert hip.hisup_polygons_capacity(2, 8, 8, 4) == 2 * (2 * (8 * 9 + 8 * 9) + 9 * 4)


def test_c_entry_checks_arguments_without_a_device():
    from pixelspointspolygons_amd._lib import lib
    L = lib()
    args = [None] * 5 + [1, 8, 8, 4, 16, 0] + [None] * 10
    assert L.p3_hisup_polygons(*args) == -1 and b"p3_hisup_polygons" in L.p3_last_error_string()
    args[5] = 0
    assert L.p3_hisup_polygons(*args) == 0                                        # B == 0: nothing to do, no launch
    assert L.p3_hisup_polygons_workspace_bytes(2, 48, 48, 8, 1000) > 2 * 51 * 51
