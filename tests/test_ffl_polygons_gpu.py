"""FFL polygons on the device against the float64 restatement tests/ffl_polygons_ref.py: indices, flags and ring positions equal,
areas within 1e-6 relative, probabilities within 1e-6 absolute.  The indicator maps hold multiples of 1 / 1024, so the float64 sum of any pixel set is
exact whatever its order and the probability flags cannot differ between the two."""
import numpy as np
import pytest
import torch

from tests import ffl_polygons_cases as C
from tests import ffl_polygons_ref as R
from tests.guard import guarded_set

pytestmark = pytest.mark.gpu
DEV = "cuda"
MIN_AREA, THRESHOLD = 12.3, 0.4990234          # no area of the cases (multiples of 1 / 8) lies near 12.3; the probabilities are exact quotients (above)
INT_KEYS = ("ring_slice", "poly_rings", "poly_batch", "poly_flags", "image_status")


def pack(pieces_batch):
    pos = [p for pieces in pieces_batch for p in pieces]
    lens = np.array([len(p) for p in pos], dtype=np.int64)
    ends = np.cumsum(lens)
    out_pos = torch.from_numpy(np.concatenate(pos + [np.zeros((0, 2), np.float32)]).astype(np.float32)).to(DEV)
    sl = torch.from_numpy(np.stack([ends - lens, ends], 1).reshape(-1, 2)).to(DEV)
    pb = torch.tensor([b for b, pieces in enumerate(pieces_batch) for _ in pieces], dtype=torch.int32, device=DEV)
    return out_pos, sl, pb


def indicators(n, h=C.H, w=C.W, seed=0):
    return np.stack([C.graded_indicator(h, w, seed + i) for i in range(n)])


def device(pieces_batch, ind, min_area=MIN_AREA, thr=THRESHOLD, **kw):
    from pixelspointspolygons_amd import hip
    out = hip.ffl_polygons(*pack(pieces_batch), torch.from_numpy(ind).to(DEV), min_area, thr, **kw)
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def same(got, want, what=""):
    assert tuple(got["counts"]) == tuple(want["counts"]), (what, got["counts"], want["counts"])
    for k in INT_KEYS:
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    assert got["ring_pos"].dtype == np.float32 and np.array_equal(got["ring_pos"].view(np.int32), want["ring_pos"].view(np.int32)), what
    assert np.all(np.abs(got["poly_area"] - want["poly_area"]) <= 1e-6 * np.abs(want["poly_area"])), (what, got["poly_area"], want["poly_area"])
    assert np.all(np.abs(got["poly_prob"] - want["poly_prob"]) <= 1e-6), (what, got["poly_prob"], want["poly_prob"])


def bits_equal(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
        else:
            assert a[k] == b[k], k


@pytest.fixture(scope="module")
def batches():
    """every hand case and 8 random graphs, three images per call; the restatement of each batch is computed once"""
    names = sorted(C.HAND)
    images = [(n, C.HAND[n][0]) for n in names] + [("random_%d" % s, C.random_graph(s)) for s in range(8)] + [("pad", [])]
    out = []
    for i in range(0, len(images), 3):
        chunk = images[i:i + 3]
        ind = indicators(3, seed=10 * i)
        out.append(([n for n, _ in chunk], [p for _, p in chunk], ind, R.run([p for _, p in chunk], ind, MIN_AREA, THRESHOLD)))
    assert len(out) == 7 and all(len(b[0]) == 3 for b in out)
    return out


@pytest.mark.parametrize("i", range(7))
def test_device_equals_the_restatement(batches, i):
    names, pieces, ind, want = batches[i]
    got = device(pieces, ind)
    print(names, "counts", got["counts"], "status", got["image_status"], "areas", got["poly_area"], "probs", got["poly_prob"])
    same(got, want, names)
    assert np.all(np.abs(want["poly_area"] - MIN_AREA) > 1e-4)          # no area is a tie; the probabilities are exact quotients on both sides


def test_more_images_than_one_pass_of_the_scan_workgroups():
    """1025 indicators of 2 x 2 and no piece: every image gives its border polygon (area 1), and the 1025th takes its edge slots (ffp_offsets) and its place in
    the outputs (ffp_scan) from the carry of the first pass of the 1024-thread scans"""
    five = indicators(5, 2, 2)
    ind = five[np.arange(1025) % 5]
    pieces = [[] for _ in range(1025)]
    want = R.run(pieces, ind, 0.5, THRESHOLD)
    assert tuple(want["counts"]) == (1025, 1025, 5 * 1025) and want["poly_batch"].tolist() == list(range(1025))
    for fallback in (False, True):
        same(device(pieces, ind, min_area=0.5, force_fallback=fallback), want, f"fallback={fallback}")


def test_hand_cases_have_their_written_out_rings_on_the_device():
    for name in ("touching_squares", "theta", "open_polyline"):
        pieces, _, polygons, areas = C.HAND[name]
        got = device([pieces], indicators(1))
        rings = [[(float(x), float(y)) for y, x in got["ring_pos"][s:e]] for s, e in got["ring_slice"]]
        assert [rings[a:b] for a, b in got["poly_rings"]] == polygons, name
        assert got["poly_area"].tolist() == [float(a) for a in areas]


def test_one_flagged_image_leaves_the_others_alone():
    a, x, b = C.HAND["ring_in_ring"][0], C.HAND["x_crossing"][0], C.random_graph(3)
    ind = indicators(3, seed=5)
    got = device([a, x, b], ind)
    assert got["image_status"].tolist() == [0, 1, 0] and not np.any(got["poly_batch"] == 1)
    for img, pieces in ((0, a), (2, b)):
        alone = device([pieces], ind[img:img + 1])
        sel = got["poly_batch"] == img
        assert int(sel.sum()) == alone["counts"][0] > 0
        r0, v0 = got["poly_rings"][sel][0, 0], got["ring_slice"][got["poly_rings"][sel][0, 0], 0]
        assert np.array_equal(got["poly_rings"][sel] - r0, alone["poly_rings"])
        nr, nv = alone["counts"][1], alone["counts"][2]
        assert np.array_equal(got["ring_slice"][r0:r0 + nr] - v0, alone["ring_slice"])
        assert np.array_equal(got["ring_pos"][v0:v0 + nv].view(np.int32), alone["ring_pos"].view(np.int32))
        for k in ("poly_area", "poly_prob", "poly_flags"):
            assert np.array_equal(got[k][sel].view(np.int32), alone[k].view(np.int32)), k


def ngon(n, h=64, w=64):
    """a convex n-gon as one closed piece: n segments, none on the border, so n + 4 edge slots"""
    t = 2 * np.pi * np.arange(n + 1) / n
    t[-1] = 0.0
    return [np.stack([h / 2 + 25 * np.sin(t), w / 2 + 25 * np.cos(t)], 1).astype(np.float32)]


def test_fallback_equals_the_lds_path_and_is_taken_over_the_limit(batches):
    from pixelspointspolygons_amd import hip
    for names, pieces, ind, want in batches[:2] + batches[5:6]:
        bits_equal(device(pieces, ind), device(pieces, ind, force_fallback=True))
    cap = hip.FFL_POLY_LDS_CAP
    ind = indicators(2, 64, 64, seed=3)
    at, over = ngon(cap - 4), ngon(cap - 3)          # exactly the limit: LDS; one edge slot more: the workspace form, by itself
    want = R.run([at, over], ind, MIN_AREA, THRESHOLD)
    assert want["counts"] == (4, 6, 2 * (5 + 2 * cap - 7 + 2)) and want["image_status"].tolist() == [0, 0]
    got = device([at, over], ind)
    same(got, want, "at and over the LDS limit")
    bits_equal(got, device([at, over], ind, force_fallback=True))


def test_a_polygon_too_long_for_the_probability_kernels_lds():
    """4 200 vertices: the faces run over the workspace, and the probability kernel reads the rounded rings from the workspace instead of its 4 096 LDS
    entries.  The restatement's planarity test would need 4 204^2 float64 tables, so here its area and probability rules are applied to the rings the
    device put out, and the rings are held to the input."""
    n = 4200
    piece = ngon(n)[0]
    ind = indicators(1, 64, 64, seed=11)
    got = device([[piece]], ind)
    assert got["counts"] == (2, 3, 5 + 2 * (n + 1)) and got["image_status"].tolist() == [0] and got["poly_rings"].tolist() == [[0, 2], [2, 3]]
    rings = [[(float(x), float(y)) for y, x in got["ring_pos"][s:e]] for s, e in got["ring_slice"]]
    assert rings[0] == C.ring((0, 0), (63, 0), (63, 63), (0, 63), (0, 0))
    pts = {(float(x), float(y)) for y, x in piece}
    assert set(rings[1]) == pts and set(rings[2]) == pts and rings[1][1:] == rings[2][-2::-1] and rings[2][0] == min(pts)
    for poly, area, prob in (([rings[0], rings[1]], got["poly_area"][0], got["poly_prob"][0]), ([rings[2]], got["poly_area"][1], got["poly_prob"][1])):
        assert abs(area - R.polygon_area(poly)) <= 1e-6 * R.polygon_area(poly)
        assert abs(prob - R.geom_prob(poly, ind[0])) <= 1e-6
    assert R.shoelace(rings[2]) > 0 > R.shoelace(rings[1])


def test_capacities_guard_bands_and_the_checking_form():
    from pixelspointspolygons_amd import hip
    pieces = [C.HAND["ring_in_ring"][0], C.HAND["theta"][0], C.random_graph(1)]
    ind = indicators(3, seed=7)
    want = R.run(pieces, ind, MIN_AREA, THRESHOLD)
    P, Rn, V = want["counts"]
    args = pack(pieces) + (torch.from_numpy(ind).to(DEV), MIN_AREA, THRESHOLD)
    f32, i32, i64 = torch.float32, torch.int32, torch.int64

    def spec(p, r, v):
        return dict(ring_pos=(v, 2, f32), ring_slice=(r, 2, i64), poly_rings=(p, 2, i64), poly_batch=(p, 1, i32), poly_area=(p, 1, f32), poly_prob=(p, 1, f32),
                    poly_flags=(p, 1, i32), image_status=(3, 1, i32), counts=(3, 1, i32), status=(1, 1, i32))

    views, guards = guarded_set(spec(P, Rn, V), DEV)          # exactly fitting: every element is written, nothing else
    out = hip.ffl_polygons_device(*args, max_polygons=P, max_rings=Rn, max_vertices=V, out=views)
    torch.cuda.synchronize()
    for g in guards.values():
        g.check()
    assert out["status"].item() == 0 and out["counts"].tolist() == [P, Rn, V]
    got = {k: v.cpu().numpy().reshape(want[k].shape) for k, v in out.items() if k in want and k != "counts"}
    got["counts"] = tuple(out["counts"].tolist())
    same(got, want, "exactly fitting capacities")
    for short in ((P - 1, Rn, V), (P, Rn - 1, V), (P, Rn, V - 1)):
        views, guards = guarded_set(spec(*short), DEV)
        out = hip.ffl_polygons_device(*args, max_polygons=short[0], max_rings=short[1], max_vertices=short[2], out=views)
        torch.cuda.synchronize()
        for k, g in guards.items():
            g.check(written=k in ("image_status", "counts", "status"))
        assert out["status"].item() & 1 and out["counts"].tolist() == [P, Rn, V], short
        with pytest.raises(hip.P3Error, match="do not fit"):
            hip.ffl_polygons(*args, max_polygons=short[0], max_rings=short[1], max_vertices=short[2])
    with pytest.raises(hip.P3Error):
        hip.ffl_polygons_device(*args, out={"ring_pos": torch.zeros(3, 2, device=DEV)})          # does not fit the default capacity
    bad = pack(pieces)
    bad[2][0] = 3          # piece_batch outside [0, B): left out on the device, status bit 1, the checking form raises
    with pytest.raises(hip.P3Error, match="piece_batch"):
        hip.ffl_polygons(*bad, torch.from_numpy(ind).to(DEV), MIN_AREA, THRESHOLD)


def test_two_calls_give_the_same_bits(batches):
    names, pieces, ind, _ = batches[4]
    bits_equal(device(pieces, ind), device(pieces, ind))


def test_filters_and_polygons_to_host():
    from pixelspointspolygons_amd import polygonize_post as Q
    pieces = [C.HAND["ring_in_ring"][0], C.HAND["bridge"][0]]
    ind = np.zeros((2, 16, 16), np.float32)
    ind[0, 2:13, 2:13] = 0.75          # the outer square's band and the inner square
    ind[1, 2:6, 2:6] = 0.75          # square A only
    pos, sl, pb = pack(pieces)
    res = {"out_pos": pos, "piece_slice": sl, "piece_batch": pb, "batch_size": 2}
    seg = torch.from_numpy(ind[:, None]).to(DEV)
    cfg = {"min_area": 12.3, "seg_threshold": 0.5}
    out = Q.polygons_from_pieces(res, seg, cfg)
    want = R.run(pieces, ind, 12.3, 0.5)
    print("areas", want["poly_area"], "probs", want["poly_prob"], "flags", want["poly_flags"])
    assert np.all(np.abs(want["poly_area"] - 12.3) > 0.1) and np.all(np.abs(want["poly_prob"] - 0.5) > 0.1)          # no tie
    assert want["poly_flags"].tolist() == [2, 0, 0, 2, 1, 3]
    assert out["poly_flags"].tolist() == want["poly_flags"].tolist() and out["batch_size"] == 2
    kept, probs, status = Q.polygons_to_host(out)
    assert status == [0, 0] and [len(k) for k in kept] == [2, 0] and [len(p) for p in probs] == [2, 0]
    ext, holes = kept[0][0]
    assert ext.dtype == np.float64 and ext.tolist() == [list(p) for p in C.square(2, 2, 12, 12)[0]]          # (x, y), closed
    assert [h.tolist() for h in holes] == [[list(p) for p in C.square(5, 5, 9, 9)[1]]]
    assert kept[0][1][1] == [] and probs[0] == [0.75, 0.75]
    everything, all_probs, _ = Q.polygons_to_host(out, kept_only=False)
    assert [len(k) for k in everything] == [3, 3] and [len(p) for p in all_probs] == [3, 3]
    many = Q.polygons_to_host({"tol_1": out, "tol_3": out})
    assert sorted(many) == ["tol_1", "tol_3"] and [len(k) for k in many["tol_3"][0]] == [2, 0]


def planted():
    """2 x 1 x 64 x 64: image 0 holds a rectangle, a rectangle with a courtyard and a rectangle cut by the right border; image 1 one rectangle"""
    m = np.zeros((2, 64, 64), np.float32)
    m[0, 8:21, 8:25] = 1
    m[0, 28:57, 10:41] = 1
    m[0, 36:49, 18:33] = 0          # the courtyard: 13 x 15 pixels, far above min_area = 10
    m[0, 20:41, 50:64] = 1
    m[1, 16:48, 12:52] = 1
    cf = np.zeros((2, 4, 64, 64), np.float32)
    cf[:, 0] = -1.0          # u = 1, v = i: c0 = u^2 v^2 = -1, c2 = -(u^2 + v^2) = 0, the zero-angle frame field
    inside = {0: [(14, 16), (32, 14), (30, 57)], 1: [(32, 32)]}          # (row, col): a point of every planted building
    outside = {0: [(42, 25), (4, 45)], 1: [(4, 4)]}          # the courtyard's centre, background
    return torch.from_numpy(m[:, None]).to(DEV), torch.from_numpy(cf).to(DEV), m, inside, outside


@pytest.mark.parametrize("method", ["acm", "asm"])
def test_end_to_end_on_a_planted_map(method):
    from pixelspointspolygons_amd import polygonize_acm as A, polygonize_asm as S, polygonize_post as Q
    seg, cf, m, inside, outside = planted()
    if method == "acm":
        cfg = dict(A.ACM_DEFAULTS, steps=50)
        run, run_pieces = Q.polygonize_acm_polygons, Q.polygonize_acm_pieces
    else:
        cfg = {**S.ASM_DEFAULTS, "init_method": "marching_squares"}
        run, run_pieces = Q.polygonize_asm_polygons, Q.polygonize_asm_pieces
    got = run(seg, cf, cfg)
    assert sorted(got) == ["tol_1"]          # the config's tolerance list
    got = got["tol_1"]
    pieces = Q.pieces_to_host(run_pieces(seg, cf, cfg, tolerance=1))
    want = R.run([[p.astype(np.float32) for p in image] for image in pieces], m, cfg["min_area"], cfg["seg_threshold"])
    host = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in got.items()}
    print(method, "counts", host["counts"], "areas", host["poly_area"], "probs", host["poly_prob"], "flags", host["poly_flags"])
    same(host, want, method)
    assert host["image_status"].tolist() == [0, 0]
    kept, probs, status = Q.polygons_to_host(got)
    assert status == [0, 0] and [len(k) for k in kept] == [3, 1]

    def holds(poly, rc):
        p = (float(rc[1]) + 0.25, float(rc[0]) + 0.125)          # off every lattice line
        as_ring = lambda a: [tuple(v) for v in a.tolist()]
        return R.point_in_polygon([as_ring(poly[0])] + [as_ring(h) for h in poly[1]], p)

    for b in (0, 1):
        for rc in inside[b]:
            assert sum(holds(poly, rc) for poly in kept[b]) == 1, (b, rc)
        for rc in outside[b]:
            assert sum(holds(poly, rc) for poly in kept[b]) == 0, (b, rc)
    assert sum(len(poly[1]) for poly in kept[0]) == 1          # the courtyard is a hole of its building
    assert all(p > 0.9 for ps in probs for p in ps)


def test_all_background_input_gives_the_empty_result():
    from pixelspointspolygons_amd import polygonize_acm as A, polygonize_asm as S, polygonize_post as Q
    seg, cf = torch.zeros(2, 1, 32, 32, device=DEV), torch.zeros(2, 4, 32, 32, device=DEV)
    cf[:, 0] = -1.0
    for got in (Q.polygonize_acm_polygons(seg, cf, tolerance=1), Q.polygonize_asm_polygons(seg, cf, {**S.ASM_DEFAULTS, "init_method": "marching_squares"}, tolerance=1)):
        assert got is not None and got["batch_size"] == 2
        assert got["counts"] == (2, 2, 10) and got["poly_flags"].tolist() == [2, 2]          # the border polygon of each image, probability 0
        assert Q.polygons_to_host(got) == ([[], []], [[], []], [0, 0])
    assert sorted(Q.polygonize_acm_polygons(seg, cf, dict(A.ACM_DEFAULTS, tolerance=[1, 3]))) == ["tol_1", "tol_3"]
