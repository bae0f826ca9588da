"""FFL corner-aware contour simplification (csrc/corner_split.hip, p3_corner_split), the parts that need no GPU: the float64 restatement the GPU tests compare
with (tests/corner_split_ref.py) against the reference's own detect_corners / split_polylines_corner through tests/golden/corner_split.npz and against
hand-checkable Douglas-Peucker cases, the fixture's decision margins, and the argument checks of the C-ABI entry and the wrappers."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import corner_split_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "p3hip.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "corner_split.npz")
DP_MARGIN, CORNER_MARGIN = 1e-4, 1e-3          # what the issue sets for the fixture


def golden():
    return np.load(GOLDEN)


def config(g, name):
    """-> pos, index, slices, closed, poly_batch, c0c2, tol_pre, tol of a stored configuration"""
    tol_pre, tol = g["config.tols"][list(g["config.names"]).index(name)]
    if name.startswith("asm"):
        return g["asm.pos"], g["asm.index"], g["asm.slices"], g["asm.closed"], g["asm.poly_batch"], g["asm.c0c2"], float(tol_pre), float(tol)
    return g["pos"], None, g["slices"], g["closed"], g["poly_batch"], g["c0c2"], float(tol_pre), float(tol)


CONFIGS = ("acm_0.125", "acm_0.3", "acm_1", "acm_pre1_tol0", "asm_1")


@pytest.mark.parametrize("name", CONFIGS)
def test_stages_b_and_c_equal_the_reference(name):
    g = golden()
    pos, index, slices, closed, poly_batch, c0c2, tol_pre, tol = config(g, name)
    mask_len, npieces = g[name + ".mask.len"], g[name + ".npieces"]
    masks, piece_flat, piece_len = g[name + ".mask"], g[name + ".piece.flat"], g[name + ".piece.len"]
    m_at = p_at = v_at = 0
    assert len(slices) == len(mask_len) and (mask_len >= 0).sum() > 10
    for i in range(len(slices)):
        q = R.explicit_points(pos, index, slices[i], bool(closed[i])).astype(np.float64)
        if mask_len[i] < 0:          # under 2 explicit points (the reference raised on none)
            assert len(q) < 2
            continue
        q = q[R.dp(q, tol_pre)]
        assert len(q) == mask_len[i]
        mask = R.detect_corners(q, c0c2[min(max(int(poly_batch[i]), 0), c0c2.shape[0] - 1)])
        assert np.array_equal(mask, masks[m_at:m_at + len(q)]), i
        m_at += len(q)
        pieces = R.split_indices(mask)
        assert len(pieces) == npieces[i], i
        for p in pieces:
            n = piece_len[p_at]
            assert np.array_equal(q[p], piece_flat[v_at:v_at + n]), i
            p_at += 1
            v_at += n
    assert m_at == len(masks) and p_at == len(piece_len) and v_at == len(piece_flat)


def test_the_fixture_holds_what_it_is_meant_to():
    g = golden()
    n = (g["slices"][:, 1] - g["slices"][:, 0]) + g["closed"]
    assert set(range(0, 6)) <= set(int(x) for x in n)          # every size from 2 to 5 explicit points, and the ones that give no piece
    assert g["c0c2"].shape == (3, 4, 32, 40) and 2 not in g["poly_batch"]          # an empty image
    assert (g["closed"] == 1).any() and (g["closed"] == 0).any()
    assert g["pos"][:, 0].min() < -0.5 and g["pos"][:, 1].max() > 39.5          # the pixel clip acts
    res = R.corner_split(*config(g, "acm_1"))
    fl, off = res["stage_flags"], res["offsets"]
    survives_no_corner = [int(((fl[off[i]:off[i + 1]] & 3) == 1).sum()) for i in range(len(off) - 1)]
    assert sum(x > 0 for x in survives_no_corner) >= 2          # the bends of the L and the T survive stage A and are no corners
    assert g["asm.index"].shape[0] > g["asm.pos"].shape[0]          # junction nodes appear on several paths


@pytest.mark.parametrize("name", CONFIGS)
def test_margins_of_the_fixture(name):
    """no decision of the restatement on the fixture is closer to turning than the issue allows: the index-exact GPU comparison is then owed"""
    g = golden()
    mg = R.Margins()
    R.corner_split(*config(g, name), margins=mg)
    d_tol, d_gap, ties, corner = mg.smallest()
    print(name, "smallest |d - tol| %.3g, gap %.3g, exact ties %d, corner margin %.3g" % (d_tol, d_gap, ties, corner))
    assert d_tol >= DP_MARGIN and d_gap >= DP_MARGIN and corner >= CORNER_MARGIN
    assert np.allclose(g[name + ".margins"], [d_tol, d_gap, ties, corner], rtol=1e-9)


def kept(points, tol):
    return list(np.flatnonzero(R.dp(np.array(points, dtype=np.float64), tol)))


def test_square_ring_with_edge_midpoints():
    ring = [(0, 0), (0, 1), (0, 2), (1, 2), (2, 2), (2, 1), (2, 0), (1, 0), (0, 0)]
    assert kept(ring, 0.1) == [0, 2, 4, 6, 8]          # the 4 corners plus the start again


def test_exact_tie_takes_the_lower_index():
    """integer coordinates: both distances are sqrt of the same integer.  The diamond (0,0), (1,4), (2,0), (1,-4) ties its two farthest points in the first,
    degenerate section; in the kite the loser of the tie is then dropped, so the result shows WHICH of the two was taken"""
    diamond = np.array([(0, 0), (1, 4), (2, 0), (1, -4), (0, 0)], dtype=np.float64)
    d = R.section_distances(diamond, 0, 4)
    assert d[0] == d[2] == d.max() == np.sqrt(17.0)
    mg = R.Margins()
    assert list(np.flatnonzero(R.dp(diamond, 0.5, mg))) == [0, 1, 2, 3, 4] and mg.dp_ties == 1
    assert kept(diamond, 4.2) == [0, 4]
    kite = [(0, 0), (3, 4), (4, 3), (0, 0)]          # both 5 away; (4,3) is 1.4 from the segment (3,4)-(0,0), (3,4) is 1.4 from (0,0)-(4,3)
    assert kept(kite, 2.0) == [0, 1, 3]
    assert kept(kite, 1.0) == [0, 1, 2, 3]


def test_collinear_run_degenerate_ring_and_tol_zero():
    line = [(0, 0), (1, 1), (2, 2), (3, 3), (7, 7)]
    assert kept(line, 0.5) == [0, 4]
    ring = [(1, 1), (1, 4), (5, 4), (1, 1)]          # s == e: the distance is the one to that point
    assert np.allclose(R.section_distances(np.array(ring, dtype=np.float64), 0, 3), [3.0, 5.0])
    assert kept(ring, 1.0) == [0, 1, 2, 3] and kept(ring, 4.0) == [0, 2, 3] and kept(ring, 5.0) == [0, 3]
    assert kept(line, 0.0) == [0, 1, 2, 3, 4] and kept(line, -1.0) == [0, 1, 2, 3, 4]
    assert kept([(0, 0), (0, 1)], 1.0) == [0, 1] and kept([(0, 0)], 1.0) == [0]
    # beyond the segment's end the distance is the one to the end, not to the line
    assert np.allclose(R.section_distances(np.array([(0, 0), (0, 5), (0, 2)], dtype=np.float64), 0, 2), [3.0])


def test_pieces_of_a_rectangle():
    """a clean axis-aligned rectangle in an axis-aligned frame field: 4 corners, 4 two-point pieces, the merged one last"""
    c0c2 = np.zeros((1, 4, 16, 16), dtype=np.float32)
    c0c2[0, 0] = -1.0          # c0 = -1, c2 = 0: u, v = the axes
    side = lambda a, b: [tuple(np.array(a) + (np.array(b) - np.array(a)) * t / 4) for t in range(4)]
    ring = side((2, 4), (2, 12)) + side((2, 12), (10, 12)) + side((10, 12), (10, 4)) + side((10, 4), (2, 4))
    ring = ring[2:] + ring[:2]          # the start is no corner
    pos = np.array(ring, dtype=np.float32)
    res = R.corner_split(pos, None, np.array([[0, 16]]), np.array([1]), np.array([0]), c0c2, 1.0, 1.0)
    assert res["counts"] == (8, 4, 2)
    assert np.array_equal(res["piece_slice"], [[0, 2], [2, 4], [4, 6], [6, 8]])
    assert list(res["out_src"]) == [2, 6, 6, 10, 10, 14, 14, 2]          # the merged piece runs over the closing point and drops both of its copies
    fl = res["stage_flags"]
    assert list(np.flatnonzero(fl & 2)) == [2, 6, 10, 14] and fl[0] == 1 and fl[16] == 1          # start and closing point survive A only


def test_entries_are_declared_exported_and_validate_before_any_device_work():
    from pixelspointspolygons_amd._lib import load
    from pixelspointspolygons_amd.build import build_library
    lib = load(build_library(verbose=False))
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    m = re.search(r"\bint\s+p3_corner_split\s*\(([^;{}]*?)\)\s*;", text, flags=re.S)
    assert m and len(m.group(1).split(",")) == 28
    assert re.search(r"\bint64_t\s+p3_corner_split_workspace_bytes\s*\(\s*int64_t\s+E\s*,\s*int\s+P\s*\)\s*;", text)
    comment = [c for c in re.findall(r"/\*.*?\*/", raw, flags=re.S) if "FFL corner-aware contour simplification" in c]
    assert comment and "frame_field_utils.detect_corners" in comment[0] and "split_polylines_corner" in comment[0]
    assert hasattr(lib, "p3_corner_split") and hasattr(lib, "p3_corner_split_workspace_bytes")
    n64, dbl = ctypes.c_int64, ctypes.c_double
    one = ctypes.c_void_p(8)          # a non-null pointer that is never followed: every call below fails its checks first

    def call(N=16, K=0, P=2, B=1, H=8, W=8, nv=32, nq=16, tol=1.0, counts=None, index=None):
        return lib.p3_corner_split(None, n64(N), index, n64(K), None, None, None, P, None, B, H, W, dbl(1.0), dbl(tol), 0, 0, nv, nq, None, None, None, None,
                                   None, None, counts, counts, None, None)

    assert call() == -1 and b"p3_corner_split" in lib.p3_last_error_string()          # null counts / status
    assert call(counts=one) == -1          # null inputs
    assert call(N=-1) == -2 and call(P=-1) == -2 and call(K=-1) == -2 and call(nv=-1) == -2 and call(nq=-1) == -2
    assert call(H=0) == -2 and call(W=0) == -2 and call(B=0) == -2
    assert call(N=1 << 30) == -2
    assert call(counts=one, tol=float("nan")) == -1 and call(counts=one, K=4) == -1          # K without index
    assert lib.p3_corner_split_workspace_bytes(n64(0), 3) == 0 and lib.p3_corner_split_workspace_bytes(n64(10), 0) == 0
    a, b = lib.p3_corner_split_workspace_bytes(n64(1000), 10), lib.p3_corner_split_workspace_bytes(n64(2000), 10)
    assert 0 < a < b <= 2 * a


def test_wrappers_refuse_host_tensors():
    from pixelspointspolygons_amd import hip, polygonize_acm as A, polygonize_asm as S, polygonize_post as Q
    pos = torch.zeros(4, 2)
    sl, closed, pb, cf = torch.tensor([[0, 4]]), torch.tensor([True]), torch.tensor([0]), torch.zeros(1, 4, 8, 8)
    with pytest.raises(hip.P3Error):
        hip.corner_split_device(pos, None, sl, closed, pb, cf, 1.0, 1.0)
    with pytest.raises(hip.P3Error):
        hip.corner_split(pos, None, sl, closed, pb, cf, 1.0, 1.0)
    tp = A.TensorPoly(pos, sl, torch.zeros(4, dtype=torch.long), 1, torch.zeros(4, dtype=torch.bool))
    with pytest.raises(hip.P3Error):
        Q.corner_split_tensorpoly(tp, cf, 1.0)
    with pytest.raises(hip.P3Error):
        Q.corner_split_tensorpoly(tp, cf, [0.125, 1])
    ts = S.TensorSkeleton(pos, torch.ones(4, dtype=torch.long), torch.arange(4), torch.tensor([0, 4]), torch.zeros(4, dtype=torch.long), torch.tensor([0, 4]), 1)
    with pytest.raises(hip.P3Error):
        Q.corner_split_skeleton(ts, cf, 1.0)
    with pytest.raises(hip.P3Error):
        Q.polygonize_acm_pieces(torch.zeros(1, 1, 8, 8), cf)
