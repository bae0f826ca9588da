"""p3_corner_split (csrc/corner_split.hip) through hip.corner_split(_device) and pixelspointspolygons_amd.polygonize_post.

Every comparison is index-exact against the float64 restatement (tests/corner_split_ref.py) on inputs whose decision margins tests/test_corner_split_cpu.py
shows to be >= 1e-4 px (Douglas-Peucker) and >= 1e-3 (corners), or on integer-coordinate cases that are exact by construction: the kernel evaluates the same
double expressions, so there is no tolerance anywhere in this file."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import corner_split_ref as R
from tests import guard as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
KEYS = ("out_pos", "out_src", "piece_slice", "piece_poly", "piece_batch")


@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "corner_split.npz"))
    return {k: g[k] for k in g.files}


def scene(form):
    g = golden()
    if form == "asm":
        return g["asm.pos"], g["asm.index"], g["asm.slices"], g["asm.closed"], g["asm.poly_batch"], g["asm.c0c2"]
    return g["pos"], None, g["slices"], g["closed"], g["poly_batch"], g["c0c2"]


@functools.lru_cache(maxsize=None)
def expected(form, tol_pre, tol):
    return R.corner_split(*scene(form), tol_pre, tol)


def dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def run(pos, index, slices, closed, poly_batch, c0c2, tol_pre, tol, **kw):
    from pixelspointspolygons_amd import hip
    return hip.corner_split(dev(pos, torch.float32), dev(index), dev(slices), dev(closed), dev(poly_batch), dev(c0c2), tol_pre, tol, stage_flags=True, **kw)


def host(out, n_flags=None):
    res = {k: out[k].cpu().numpy() for k in KEYS}
    res["counts"] = tuple(out["counts"])
    if "stage_flags" in out:
        res["stage_flags"] = out["stage_flags"].cpu().numpy()[:n_flags]
    return res


def same(got, want, pos=None):
    for k in KEYS + ("stage_flags",):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert tuple(got["counts"]) == tuple(want["counts"])
    assert got["out_pos"].tobytes() == want["out_pos"].tobytes()          # bit copies of the gathered input positions


FORMS = {"acm_0.125": ("acm", 0.125, 0.125), "acm_1": ("acm", 1.0, 1.0), "asm_1": ("asm", 0.0, 1.0), "acm_tol0": ("acm", 1.0, 0.0)}


@pytest.mark.parametrize("fallback", [False, True], ids=["lds", "fallback"])
@pytest.mark.parametrize("name", sorted(FORMS))
def test_device_equals_the_restatement(name, fallback):
    form, tol_pre, tol = FORMS[name]
    want = expected(form, tol_pre, tol)
    got = host(run(*scene(form), tol_pre, tol, force_fallback=fallback), want["offsets"][-1])
    same(got, want)
    assert want["counts"][1] > 40


def test_two_runs_and_both_forms_give_the_same_bits():
    a = host(run(*scene("acm"), 0.3, 0.3), None)
    b = host(run(*scene("acm"), 0.3, 0.3), None)
    c = host(run(*scene("acm"), 0.3, 0.3, force_fallback=True), None)
    for k in KEYS + ("stage_flags",):
        assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes(), k
    same({**a, "stage_flags": a["stage_flags"][:expected("acm", 0.3, 0.3)["offsets"][-1]]}, expected("acm", 0.3, 0.3))


def test_an_image_alone_equals_itself_inside_the_batch():
    pos, index, slices, closed, poly_batch, c0c2 = scene("acm")
    whole = expected("acm", 1.0, 1.0)
    for b in (0, 1, 2):
        sel = np.flatnonzero(poly_batch == b)
        got = host(run(pos, None, slices[sel], closed[sel], np.zeros(len(sel), dtype=np.int32), c0c2[b:b + 1], 1.0, 1.0), None)
        pieces = np.flatnonzero(whole["piece_batch"] == b)
        assert got["counts"][1] == len(pieces)
        if not len(pieces):
            continue
        v0, v1 = whole["piece_slice"][pieces[0], 0], whole["piece_slice"][pieces[-1], 1]
        assert got["out_pos"].tobytes() == whole["out_pos"][v0:v1].tobytes() and np.array_equal(got["out_src"], whole["out_src"][v0:v1])
        assert np.array_equal(got["piece_slice"], whole["piece_slice"][pieces] - v0)
        assert np.array_equal(sel[got["piece_poly"]], whole["piece_poly"][pieces])


def one_ring(points, c0c2=None, closed=0):
    pos = np.asarray(points, dtype=np.float32)
    if c0c2 is None:
        c0c2 = np.zeros((1, 4, 8, 8), dtype=np.float32)
        c0c2[0, 0] = -1.0
    return pos, None, np.array([[0, len(pos)]], dtype=np.int64), np.array([closed], dtype=np.uint8), np.array([0], dtype=np.int32), c0c2


def test_a_polyline_over_the_cap_takes_the_fallback_by_itself():
    rng = np.random.default_rng(7)
    k = 4200
    w = np.arange(k) * 2 * np.pi / k
    circle = np.stack([60 + 50 * np.cos(w), 64 + 52 * np.sin(w)], 1) + rng.normal(0, 0.2, (k, 2))
    c0c2 = np.zeros((1, 4, 128, 128), dtype=np.float32)
    c0c2[0, 0], c0c2[0, 3] = -1.0, 0.05
    args = one_ring(circle, c0c2, closed=1)
    mg = R.Margins()
    want = R.corner_split(*args, 1.0, 1.0, margins=mg)
    d_tol, d_gap, _, corner = mg.smallest()
    print("4200-point circle: smallest |d - tol| %.3g, gap %.3g, corner margin %.3g; %d vertices in %d pieces" % (d_tol, d_gap, corner, *want["counts"][:2]))
    assert min(d_tol, d_gap) >= 1e-6 and corner >= 1e-6          # double against double: seven orders over the rounding of one operation
    same(host(run(*args, 1.0, 1.0, max_len=k), k + 1), want)
    same(host(run(*args, 1.0, 1.0), k + 1), want)          # max_len unknown: both kernels are launched
    assert want["counts"][0] < k // 10


def test_more_polylines_than_one_pass_of_the_scan_workgroup():
    """1025 polylines of 3 points: cs_offsets and cs_scan are one workgroup of 1024 threads, so the last polyline's offsets come from the carry of the first pass.
    Right angles with legs a != b on an axis-aligned field: the middle point lies a b / sqrt(a^2 + b^2) >= 0.89 from the chord (tolerance 0.5), no edge on a diagonal."""
    P = 1025
    i = np.arange(P)
    a, b = 1 + i % 3, 2 + i % 3 + (i // 3) % 2
    pos = np.stack([np.stack([np.ones(P), np.ones(P)], 1), np.stack([np.ones(P), 1 + a], 1), np.stack([1 + b, 1 + a], 1)], 1).reshape(3 * P, 2)
    assert pos.max() <= 7
    slices = np.stack([3 * i, 3 * i + 3], 1).astype(np.int64)
    c0c2 = np.zeros((1, 4, 8, 8), dtype=np.float32)
    c0c2[0, 0] = -1.0
    args = (pos.astype(np.float32), None, slices, (i % 2).astype(np.uint8), np.zeros(P, dtype=np.int32), c0c2)
    want = R.corner_split(*args, 0.5, 0.5)
    assert want["counts"][1] >= P
    for fallback in (False, True):
        same(host(run(*args, 0.5, 0.5, force_fallback=fallback), want["offsets"][-1]), want)


def test_staircase_peels_one_point_per_round():
    """200 points of a zigzag whose amplitude decays by 3 % per point: the farthest point of every section is the one right behind its start, so
    Douglas-Peucker keeps one point per level and the recursion is 198 deep"""
    k = np.arange(200, dtype=np.float64)
    pts = np.stack([100.0 + 100.0 * (-1.0) ** k * 0.97 ** k, k], 1).astype(np.float32)
    q = pts.astype(np.float64)
    gaps = []
    for s in range(0, 198):
        d = R.section_distances(q, s, 199)
        assert int(np.argmax(d)) == 0 and d[0] > 1e-3
        if len(d) > 1:
            gaps.append(d[0] - np.sort(d)[-2])
    assert min(gaps) > 1e-3
    c0c2 = np.zeros((1, 4, 208, 200), dtype=np.float32)
    c0c2[0, 0] = -1.0
    args = one_ring(pts, c0c2)
    want = R.corner_split(*args, 1e-3, 0.0)
    assert (want["stage_flags"] & 1).all()
    same(host(run(*args, 1e-3, 0.0, max_len=200), 200), want)
    same(host(run(*args, 1e-3, 0.0, max_len=200, force_fallback=True), 200), want)


def test_exact_ties_take_the_lower_index():
    kite = [(0, 0), (3, 4), (4, 3)]
    diamond = [(0, 0), (1, 4), (2, 0), (1, -4)]
    for pts, tol, src in ((kite, 2.0, [0, 1, 3]), (diamond, 0.5, [0, 1, 2, 3, 4]), (diamond, 4.2, [0, 4])):
        args = one_ring(pts, closed=1)
        want = R.corner_split(*args, tol, 0.0)
        assert list(np.flatnonzero(want["stage_flags"] & 1)) == src
        for fb in (False, True):
            same(host(run(*args, tol, 0.0, force_fallback=fb), len(pts) + 1), want)


def test_no_polyline_and_polylines_without_points():
    from pixelspointspolygons_amd import hip
    c0c2 = torch.zeros(1, 4, 8, 8, device=DEV)
    empty = lambda dt, *s: torch.zeros(s, dtype=dt, device=DEV)
    out = hip.corner_split(empty(torch.float32, 5, 2), None, empty(torch.int64, 0, 2), empty(torch.uint8, 0), empty(torch.int32, 0), c0c2, 1.0, 1.0)
    assert out["counts"] == (0, 0, 0) and out["out_pos"].shape == (0, 2) and out["piece_slice"].shape == (0, 2)
    out = hip.corner_split(empty(torch.float32, 0, 2), None, empty(torch.int64, 2, 2), empty(torch.uint8, 2), empty(torch.int32, 2), c0c2, 1.0, 1.0)
    assert out["counts"] == (0, 0, 0)
    out = hip.corner_split(empty(torch.float32, 5, 2), None, torch.tensor([[0, 1], [3, 3]], device=DEV), torch.tensor([0, 1], device=DEV, dtype=torch.uint8),
                           empty(torch.int32, 2), c0c2, 1.0, 1.0)
    assert out["counts"] == (0, 0, 0)


def test_overflow_reports_the_true_totals_and_writes_nothing_past_the_capacities():
    from pixelspointspolygons_amd import hip
    pos, index, slices, closed, poly_batch, c0c2 = scene("acm")
    want = expected("acm", 1.0, 1.0)
    V, Q, longest = want["counts"]
    nv, nq = V // 2, Q // 3
    args = (dev(pos, torch.float32), None, dev(slices), dev(closed), dev(poly_batch), dev(c0c2), 1.0, 1.0)
    # every output between guard bands and written up to its capacity; stage_flags (uint8) only up to the explicit points that exist
    out = G.guarded_run(lambda **kw: hip.corner_split_device(*args, max_vertices=nv, max_pieces=nq, stage_flags=True, **kw), unwritten=("stage_flags",))
    assert out["status"].tolist() == [1] and out["counts"].tolist() == [V, Q, longest] and out["stage_flags"].dtype == torch.uint8
    assert out["out_pos"].cpu().numpy().tobytes() == want["out_pos"][:nv].tobytes() and np.array_equal(out["out_src"].cpu().numpy(), want["out_src"][:nv])
    assert np.array_equal(out["piece_slice"].cpu().numpy(), want["piece_slice"][:nq]) and np.array_equal(out["piece_poly"].cpu().numpy(), want["piece_poly"][:nq])
    with pytest.raises(hip.P3Error):
        hip.corner_split(dev(pos, torch.float32), None, dev(slices), dev(closed), dev(poly_batch), dev(c0c2), 1.0, 1.0, max_vertices=nv)
    assert G.guarded_run(lambda **kw: hip.corner_split_device(*args, max_vertices=V, max_pieces=Q, **kw))["status"].tolist() == [0]


def test_the_containers_the_list_of_tolerances_and_the_host_pieces():
    from pixelspointspolygons_amd import polygonize_acm as A, polygonize_asm as S, polygonize_post as Q
    pos, _, slices, closed, poly_batch, c0c2 = scene("acm")
    keep = np.flatnonzero(slices[:, 1] > slices[:, 0])          # a TensorPoly has no empty contour
    is_endpoint = np.zeros(len(pos), dtype=bool)
    for i in keep:
        if not closed[i]:
            is_endpoint[slices[i, 0]] = is_endpoint[slices[i, 1] - 1] = True
    batch = np.zeros(len(pos), dtype=np.int64)
    for i in keep:
        batch[slices[i, 0]:slices[i, 1]] = poly_batch[i]
    tp = A.TensorPoly(dev(pos, torch.float32), dev(slices[keep]), dev(batch), 3, dev(is_endpoint))
    got = Q.corner_split_tensorpoly(tp, dev(c0c2), [0.125, 1], stage_flags=True)
    assert sorted(got) == ["tol_0.125", "tol_1"]
    for key, t in (("tol_0.125", 0.125), ("tol_1", 1.0)):
        want = R.corner_split(pos, None, slices[keep], closed[keep], poly_batch[keep], c0c2, min(1.0, t), t)
        same(host(got[key], want["offsets"][-1]), want)
    pieces = Q.pieces_to_host(got)
    assert sorted(pieces) == ["tol_0.125", "tol_1"] and len(pieces["tol_1"]) == 3 and pieces["tol_1"][2] == []
    want = R.corner_split(pos, None, slices[keep], closed[keep], poly_batch[keep], c0c2, 1.0, 1.0)
    flat = [p for image in pieces["tol_1"] for p in image]
    assert len(flat) == want["counts"][1] and all(p.dtype == np.float64 for p in flat)
    assert all(np.array_equal(p, want["out_pos"][s:e].astype(np.float64)) for p, (s, e) in zip(flat, want["piece_slice"]))
    # the ASM form through the skeleton container
    apos, index, aslices, _, _, ac = scene("asm")
    g = np.load(os.path.join(ROOT, "tests", "golden", "asm.npz"))
    ts = S.TensorSkeleton(dev(apos, torch.float32), dev(g["ts.degrees"]), dev(index), dev(g["ts.path_delim"]), dev(g["ts.batch"]), dev(g["ts.batch_delim"]), 3)
    same(host(Q.corner_split_skeleton(ts, dev(ac), 1.0, stage_flags=True), expected("asm", 0.0, 1.0)["offsets"][-1]), expected("asm", 0.0, 1.0))


def test_polygonize_acm_pieces_equals_polygonize_device_and_the_restatement():
    from pixelspointspolygons_amd import polygonize_acm as A, polygonize_post as Q
    g = np.load(os.path.join(ROOT, "tests", "golden", "acm.npz"))
    ind, c0c2 = torch.from_numpy(g["indicator"]).to(DEV), torch.from_numpy(g["c0c2"]).to(DEV)
    seg = ind[:, None].contiguous()
    cfg = dict(A.ACM_DEFAULTS, steps=20)
    tp = A.polygonize_device(seg, c0c2, cfg)
    contours = A.tensorpoly_to_contours_batch(tp)
    got = Q.pieces_to_host(Q.polygonize_acm_pieces(seg, c0c2, cfg))
    assert sorted(got) == ["tol_1"]
    want = [[p for c in cs for p in R.pieces_of_contour(c, g["c0c2"][b], 1.0, 1.0)] for b, cs in enumerate(contours)]
    mg = R.Margins()
    for b, cs in enumerate(contours):
        for c in cs:
            q = np.asarray(c, dtype=np.float64)
            keep = R.dp(q, 1.0, mg)
            for p in R.split_indices(R.detect_corners(q[keep], g["c0c2"][b], mg)):
                R.dp(q[keep][p], 1.0, mg)
    print("optimised contours: %d vertices in %d contours -> %d pieces; smallest margins |d - tol| %.3g, gap %.3g, corner %.3g" % (
        tp.pos.shape[0], sum(len(cs) for cs in contours), sum(len(x) for x in want), *[mg.smallest()[i] for i in (0, 1, 3)]))
    assert len(got["tol_1"]) == len(want)
    for a, b in zip(got["tol_1"], want):
        assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
