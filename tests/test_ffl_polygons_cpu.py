"""FFL polygons without a device: the float64 restatement tests/ffl_polygons_ref.py on hand cases with their expected rings written
out, on properties every planar subdivision has, and on the probability rule; the argument checks of the bindings and of p3_ffl_polygons."""
import ctypes

import networkx as nx
import numpy as np
import pytest
import torch

from tests import ffl_polygons_cases as C
from tests import ffl_polygons_ref as R


@pytest.mark.parametrize("name", sorted(C.HAND))
def test_restatement_on_hand_cases(name):
    pieces, status, polygons, areas = C.HAND[name]
    st, got = R.faces(pieces, C.H, C.W)
    assert st == status
    assert got == polygons
    assert [R.polygon_area(p) for p in got] == [float(a) for a in areas]


def test_dangle_equals_the_empty_image_and_pieces_equal_the_whole_square():
    assert R.faces(C.HAND["dangle"][0], C.H, C.W) == R.faces([], C.H, C.W)
    assert R.faces(C.HAND["square_in_pieces"][0], C.H, C.W) == R.faces(C.HAND["one_square"][0], C.H, C.W)
    assert R.faces(C.HAND["bridge_with_tail"][0], C.H, C.W) == R.faces(C.HAND["bridge"][0], C.H, C.W)


def test_negative_zero_and_non_finite_coordinates():
    a = C.piece((0, 5), (5, 5), (10, 9), (15, 9))
    b = a.copy()
    b[0, 1] = -0.0          # x = -0: the same node as the border's (0, 5)
    assert R.faces([b], C.H, C.W) == R.faces([a], C.H, C.W)
    b[1, 0] = np.nan
    assert R.faces([b], C.H, C.W) == (2, [])


def _left_by_step_5(pieces):
    """nodes, edges and components of what dangles and cuts leave, by networkx alone"""
    _, edges = R.graph(pieces, C.H, C.W)
    G = nx.Graph(list(edges))
    while True:
        leaves = [n for n in G if G.degree(n) <= 1]
        if not leaves:
            break
        G.remove_nodes_from(leaves)
    G.remove_edges_from(list(nx.bridges(G)))
    G.remove_nodes_from([n for n in G if G.degree(n) == 0])
    return G.number_of_nodes(), G.number_of_edges(), nx.number_connected_components(G)


@pytest.mark.parametrize("seed", range(8))
def test_properties_on_random_planar_graphs(seed):
    pieces = C.random_graph(seed)
    st, polygons = R.faces(pieces, C.H, C.W)
    assert st == 0
    # Euler: V - E + F = 1 + C with the unbounded face among the F, so the bounded faces number E - V + C
    V, E, comps = _left_by_step_5(pieces)
    assert len(polygons) == E - V + comps
    # dangles, bridges and more than one component are really there
    _, edges = R.graph(pieces, C.H, C.W)
    assert len(edges) > E and comps >= 1
    total = 0.0
    for p in polygons:
        total += R.polygon_area(p)
    assert total == (C.W - 1) * (C.H - 1)          # quarter-integer sums: exact
    rng = np.random.default_rng(seed)
    E2 = np.array(sorted(edges), dtype=np.float64)
    a, d = E2[:, 0], E2[:, 1] - E2[:, 0]
    samples = []
    while len(samples) < 2000:
        p = rng.uniform(0.0, 15.0, size=2)
        t = np.clip(((p - a) * d).sum(1) / (d * d).sum(1), 0.0, 1.0)
        if p.min() > 1e-6 and p.max() < 15 - 1e-6 and np.sqrt((((a + t[:, None] * d) - p) ** 2).sum(1)).min() > 1e-6:
            samples.append((float(p[0]), float(p[1])))
    for p in samples:
        assert sum(R.point_in_polygon(poly, p) for poly in polygons) == 1


def test_random_graphs_hold_dangles_bridges_and_several_components():
    seen = [0, 0, 0]
    for seed in range(8):
        _, edges = R.graph(C.random_graph(seed), C.H, C.W)
        G = nx.Graph(list(edges))
        seen[0] += any(G.degree(n) == 1 for n in G)
        seen[1] += len(list(nx.bridges(G))) > 0
        seen[2] += nx.number_connected_components(G) > 1
    assert all(s >= 4 for s in seen), seen


# ------------------------------------------------------------------------------------------ the probability rule
def _count(poly):
    return int(R.raster(poly, 16, 16).sum())


def test_probability_rule():
    rect = [C.ring((2, 2), (6, 2), (6, 5), (2, 5), (2, 2))]
    assert _count(rect) == 20          # a 4 x 3 rectangle: 5 x 4 lattice points, edges included
    assert _count([C.ring((0, 0), (4, 0), (0, 4), (0, 0))]) == 15
    shell, hole = C.square(1, 1, 9, 9)[0], C.square(3, 3, 6, 6)[1]
    m = R.raster([shell, hole], 16, 16)
    assert int(m.sum()) == 81 - 16 and not m[3:7, 3:7].any() and m[2, 2:8].all()          # the hole's own edge pixels are cleared
    ind = C.graded_indicator()
    assert R.geom_prob(rect, ind) == float(ind[2:6, 2:7].astype(np.float64).sum() / 20)
    assert R.geom_prob(rect, np.ones((16, 16), np.float32)) == 1.0


def test_bounds_rule_truncates_like_int():
    """compute_geom_prob takes int() of the bounds, which truncates towards zero: a shell that reaches to -0.25 has minx = 0 and is rastered (its vertex
    rounds to pixel 0), one that reaches to -1.25 has minx = -1 and gets probability 0; so does one that reaches past the last pixel."""
    ind = np.ones((16, 16), np.float32)
    assert R.geom_prob([C.ring((-0.25, 2), (4, 2), (4, 5), (-0.25, 5), (-0.25, 2))], ind) == 1.0
    assert R.raster([C.ring((-0.25, 2), (4, 2), (4, 5), (-0.25, 5), (-0.25, 2))], 16, 16).sum() == 20
    assert R.geom_prob([C.ring((-1.25, 2), (4, 2), (4, 5), (-1.25, 5), (-1.25, 2))], ind) == 0.0
    assert R.geom_prob([C.ring((2, -1.0), (4, -1.0), (4, 5), (2, 5), (2, -1.0))], ind) == 0.0
    assert R.geom_prob([C.ring((2, 2), (16, 2), (16, 5), (2, 5), (2, 2))], ind) == 0.0
    assert R.geom_prob([C.ring((2, 2), (15.5, 2), (15.5, 5), (2, 5), (2, 2))], ind) == 1.0


def test_half_to_even_rounding_in_the_cropped_window():
    """np.round acts on the coordinates moved by (-minx, -miny): 2.5 - 2 = 0.5 -> 0 and 6.5 - 2 = 4.5 -> 4 give columns 2 .. 6; 3.5 - 3 = 0.5 -> 0 and
    7.5 - 3 = 4.5 -> 4 give rows 3 .. 7 (rounding 3.5 and 7.5 themselves would give rows 4 .. 8)"""
    m = R.raster([C.ring((2.5, 3.5), (6.5, 3.5), (6.5, 7.5), (2.5, 7.5), (2.5, 3.5))], 16, 16)
    assert m[3:8, 2:7].all() and int(m.sum()) == 25


def test_raster_without_pixels_gives_zero():
    tri = [C.ring((4.6, 4.6), (4.9, 4.6), (4.9, 4.9), (4.6, 4.6))]          # every vertex rounds to 5, the window is column 4, row 4
    assert int(R.raster(tri, 16, 16).sum()) == 0
    assert R.geom_prob(tri, np.ones((16, 16), np.float32)) == 0.0


def test_filter_flags_of_the_restatement():
    ind = np.zeros((1, 16, 16), np.float32)
    ind[0, 4:9, 4:9] = 1.0
    out = R.run([C.HAND["one_square"][0]], ind, min_area=20, seg_threshold=0.5)
    assert out["counts"] == (2, 3, 15)
    assert out["poly_prob"].tolist() == [0.0, 1.0] and out["poly_area"].tolist() == [209.0, 16.0]
    assert out["poly_flags"].tolist() == [2, 1]
    assert out["ring_pos"][5:10].tolist() == [[4, 4], [8, 4], [8, 8], [4, 8], [4, 4]]          # (row, col): the hole (x, y) = (4, 4), (4, 8), ...


# ------------------------------------------------------------------------------------------ argument checks
def test_wrappers_refuse_host_tensors_and_wrong_shapes():
    from pixelspointspolygons_amd import hip, polygonize_post as Q
    pos, sl, pb, ind = torch.zeros(4, 2), torch.tensor([[0, 4]]), torch.tensor([0]), torch.zeros(1, 8, 8)
    with pytest.raises(hip.P3Error):
        hip.ffl_polygons_device(pos, sl, pb, ind, 10, 0.5)
    with pytest.raises(hip.P3Error):
        hip.ffl_polygons(pos, sl, pb, ind, 10, 0.5)
    res = {"out_pos": pos, "piece_slice": sl, "piece_batch": pb, "batch_size": 1}
    seg = torch.zeros(1, 1, 8, 8)
    cfg = {"min_area": 10, "seg_threshold": 0.5}
    for call in (lambda: Q.polygons_from_pieces(res, seg, cfg), lambda: Q.polygons_from_pieces({"tol_1": res}, seg, cfg),
                 lambda: Q.polygonize_acm_polygons(seg, torch.zeros(1, 4, 8, 8)),
                 lambda: Q.polygonize_asm_polygons(seg, torch.zeros(1, 4, 8, 8), {"init_method": "marching_squares"})):
        with pytest.raises(hip.P3Error):
            call()


def test_wrapper_refuses_wrong_shapes_and_dtypes_before_any_launch(monkeypatch):
    from pixelspointspolygons_amd import hip
    monkeypatch.setattr(hip, "_dev", lambda t: None)          # the shape checks come right behind the device check
    pos, sl, pb, ind = torch.zeros(4, 2), torch.tensor([[0, 4]]), torch.tensor([0]), torch.zeros(1, 8, 8)
    bad = [(pos.double(), sl, pb, ind), (torch.zeros(4, 3), sl, pb, ind), (torch.zeros(8), sl, pb, ind), (pos, torch.tensor([0, 4]), pb, ind),
           (pos, sl.float(), pb, ind), (pos, sl, torch.tensor([0, 0]), ind), (pos, sl, pb.float(), ind), (pos, sl, pb, torch.zeros(8, 8)),
           (pos, sl, pb, torch.zeros(1, 1, 8)), (pos, sl, pb, torch.zeros(1, 8, 8, dtype=torch.int32))]
    for args in bad:
        with pytest.raises(hip.P3Error, match="ffl_polygons"):
            hip.ffl_polygons_device(*args, 10, 0.5)
    for caps in (dict(max_polygons=0), dict(max_rings=-1), dict(max_vertices=0)):
        with pytest.raises(hip.P3Error, match="max_"):
            hip.ffl_polygons_device(pos, sl, pb, ind, 10, 0.5, **caps)
    assert hip.ffl_polygons_capacity(10, 2) == (28, 28, 84)
    assert hip.FFL_POLY_LDS_CAP == 1024


def test_entry_validates_before_any_device_work():
    from pixelspointspolygons_amd._lib import load
    from pixelspointspolygons_amd.build import build_library
    lib = load(build_library(verbose=False))
    n64, dbl = ctypes.c_int64, ctypes.c_double
    one = ctypes.c_void_p(8)          # a non-null pointer that is never followed: every call below fails its checks first
    sl_ok = np.array([[0, 4], [4, 8]], dtype=np.int64)
    pb_ok = np.array([0, 1], dtype=np.int32)

    def call(V=8, Q=2, B=2, H=8, W=8, area=10.0, thr=0.5, caps=(4, 4, 16), sl=sl_ok, pb=pb_ok, st=one):
        s = sl.ctypes.data_as(ctypes.c_void_p) if sl is not None else None
        p = pb.ctypes.data_as(ctypes.c_void_p) if pb is not None else None
        return lib.p3_ffl_polygons(one, n64(V), s, p, Q, one, B, H, W, dbl(area), dbl(thr), 0, caps[0], caps[1], caps[2], one, one, one, one, one, one, one,
                                   st, st, st, one, None)

    err = lambda: lib.p3_last_error_string()
    assert call(V=-1) == -1 and b"p3_ffl_polygons" in err() and b"negative" in err()
    assert call(Q=-1) == -1 and call(caps=(-1, 4, 16)) == -1 and call(caps=(4, -1, 16)) == -1 and call(caps=(4, 4, -1)) == -1
    assert call(B=0) == -1 and call(H=1) == -1 and call(W=1) == -1
    assert call(area=float("nan")) == -1 and b"NaN" in err()
    assert call(thr=float("nan")) == -1 and b"NaN" in err()
    assert call(st=None) == -1 and call(sl=None) == -1 and call(pb=None) == -1
    assert call(pb=np.array([0, 2], dtype=np.int32)) == -1 and b"piece_batch out of [0, B)" in err()
    assert call(pb=np.array([-1, 0], dtype=np.int32)) == -1 and b"piece_batch out of [0, B)" in err()
    assert call(sl=np.array([[0, 4], [4, 9]], dtype=np.int64)) == -1 and b"piece_slice" in err() and b"outside out_pos" in err()
    assert call(sl=np.array([[-1, 4], [4, 8]], dtype=np.int64)) == -1 and b"outside out_pos" in err()
    assert call(sl=np.array([[5, 4], [4, 8]], dtype=np.int64)) == -1 and b"outside out_pos" in err()
    assert call() == -1 and b"device memory" in err()          # well-formed, but host arrays: nothing is launched on them
    assert lib.p3_ffl_polygons_workspace_bytes(n64(-1), 2) == 0 and lib.p3_ffl_polygons_workspace_bytes(n64(10), 0) == 0
    a, b = lib.p3_ffl_polygons_workspace_bytes(n64(1000), 4), lib.p3_ffl_polygons_workspace_bytes(n64(2000), 4)
    assert 0 < a < b <= 2 * a
    assert lib.p3_ffl_polygons_workspace_bytes(n64(0), 1) > 0          # the border alone


def test_existing_entries_are_unchanged_names():
    from pixelspointspolygons_amd import polygonize_post as Q
    for name in ("corner_split_tensorpoly", "corner_split_skeleton", "pieces_to_host", "polygonize_acm_pieces", "polygonize_asm_pieces",
                 "polygons_from_pieces", "polygonize_acm_polygons", "polygonize_asm_polygons", "polygons_to_host"):
        assert callable(getattr(Q, name))
