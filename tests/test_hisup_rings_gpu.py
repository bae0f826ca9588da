"""p3_hisup_polygons_rings on the GPU through the public wrappers: every output equals the restatements (tests/hisup_polygon_ref.py for the outer polygons,
tests/hisup_rings_ref.py for the inner rings, pinned to the reference's `get_poly_crowdai` by the CPU tests) bit for bit.  Inputs are made the way
p3_hisup_regions / p3_hisup_junctions write them.  No t_i lies within 1e-9 degrees of 10 or 350 and no distance within 1e-9 of 5 (asserted), so the last
bit of atan2 or of a root decides nothing."""
import functools

import numpy as np
import pytest
import torch

from tests import guard as G
from tests import hisup_polygon_ref as R
from tests import hisup_rings_ref as Q

pytestmark = pytest.mark.gpu
DEV = "cuda"
OUTER = ("pos", "src", "poly_slice", "poly_flags", "hole_pixels", "n_vertices", "counts")
RINGS = ("ring_pos", "ring_src", "ring_slice", "ring_region", "ring_flags", "ring_area2", "region_rings", "n_holes", "ring_counts")
KEYS = OUTER + RINGS + ("status",)
NOJ = np.zeros((0, 2))


def _hip():
    from pixelspointspolygons_amd import hip
    return hip


def inputs(fg, juncs):
    labels, n_regions, bbox, Rr = R.region_inputs(fg)
    ju, counts = R.junction_inputs(juncs)
    return dict(labels=labels, n_regions=n_regions, bbox=bbox, juncs=ju, counts=counts, R=Rr)


def tensors(inp, sel=slice(None)):
    return [torch.from_numpy(np.ascontiguousarray(inp[k][sel])).to(DEV) for k in ("labels", "n_regions", "bbox", "juncs", "counts")]


def run(inp, sel=slice(None), **kw):
    out = _hip().hisup_polygon_rings_device(*tensors(inp, sel), **kw)
    assert sorted(out) == sorted(KEYS)
    return {k: out[k].cpu().numpy() for k in KEYS}


def expected(inp, sel=slice(None)):
    a = (inp["labels"][sel], inp["n_regions"][sel], inp["juncs"][sel], inp["counts"][sel], inp["R"])
    outer, inner = R.polygons(*a), Q.rings(*a)
    assert min(outer["margin_t"], inner["margin_t"]) >= 1e-9 and min(outer["margin_d"], inner["margin_d"]) >= 1e-9
    return outer, inner


@functools.lru_cache(maxsize=None)
def case(name):
    """the inputs of a named set and what the restatements give for them, computed once"""
    if name == "hand":
        (fg, juncs), (dfg, dj) = (Q.hand_set(), [NOJ] * 2), Q.disc_cases()
        fg, juncs = np.concatenate([fg, dfg]), juncs + dj
    elif name == "big":
        fg, juncs = Q.big_ring_set()
    inp = inputs(fg, juncs)
    return inp, expected(inp)


def same_outer(got, want):
    V, longest = want["counts"]
    assert got["counts"].tolist() == [V, longest]
    assert np.array_equal(got["poly_slice"], want["poly_slice"]) and np.array_equal(got["poly_flags"], want["poly_flags"])
    assert np.array_equal(got["hole_pixels"], want["hole_pixels"]) and np.array_equal(got["n_vertices"], want["n_vertices"])
    assert np.array_equal(got["src"][:V], want["src"])
    assert got["pos"][:V].tobytes() == want["pos"].tobytes()


def same_rings(got, want, vertices=True):
    n, V, longest = want["ring_counts"]
    assert got["ring_counts"].tolist() == [n, V, longest]
    assert np.array_equal(got["region_rings"], want["region_rings"]) and np.array_equal(got["n_holes"], want["n_holes"])
    for k in ("ring_slice", "ring_region", "ring_flags", "ring_area2"):
        assert np.array_equal(got[k][:n], want[k]), k
    if vertices:
        assert np.array_equal(got["ring_src"][:V], want["ring_src"])
        assert got["ring_pos"][:V].tobytes() == want["ring_pos"].tobytes()


def same(got, want):
    assert got["status"].tolist() == [0]
    same_outer(got, want[0])
    same_rings(got, want[1])


def bits(a, b):
    """two results of the same inputs hold the same bits wherever the call defines them"""
    V, (n, RV, _) = int(a["counts"][0]), a["ring_counts"].tolist()
    cut = dict(pos=V, src=V, ring_pos=RV, ring_src=RV, ring_slice=n, ring_region=n, ring_flags=n, ring_area2=n)
    return all(a[k][:cut.get(k)].tobytes() == b[k][:cut.get(k)].tobytes() for k in KEYS)


# ------------------------------------------------------------------------------------------------ (a) the reference's own output
@pytest.mark.parametrize("first", [0, 3])
def test_golden_regions(first):
    fg, juncs, polys = Q.load_fixture()
    inp = inputs(fg, juncs)
    sel = slice(first, first + 3)
    got = run(inp, sel)
    want = expected(inp, sel)
    same(got, want)
    seen = rings = 0
    for b in range(3):
        for l in range(1, int(inp["n_regions"][first + b]) + 1):
            poly, parts = Q.concatenated(got, got, b, l - 1)                     # the concatenation of forward_val, from the kernel's outputs
            assert poly.tobytes() == polys[(first + b, l)][0].tobytes() and parts == polys[(first + b, l)][1]      # the fixture itself
            seen += 1
            rings += len(parts) - 1
    assert seen >= 15 and rings >= 8


@pytest.mark.parametrize("case_", ["squares", "courtyards"])
def test_more_region_slots_than_one_pass_of_the_offset_scans(case_):
    """400 region slots per image against the 1024 threads of hp_offsets_kernel and hp_ring_offsets_kernel.
    squares: 3 images (1200 slots) of 8 x 8 labels, one 2 x 2 region in images 0 and 2; the empty slots 1024 .. 1199 and n_vertices[2] hold the carry of the first
    pass, the ring carries stay 0 (no hole).
    courtyards: 4 images (1600 slots) of 12 x 12, a 10 x 10 block with an 8 x 8 hole in images 0 and 3; image 3's region is slot 1200, in the second pass, so its
    polygon, its ring and its ring's vertices start at non-zero carries."""
    if case_ == "squares":
        fg = np.zeros((3, 8, 8), bool)
        fg[0, 1:3, 1:3] = fg[2, 4:6, 3:5] = True
    else:
        fg = np.zeros((4, 12, 12), bool)
        fg[0, 1:11, 1:11] = fg[3, 1:11, 1:11] = True
        fg[0, 2:10, 2:10] = fg[3, 2:10, 2:10] = False
    last = len(fg) - 1
    inp = inputs(fg, [NOJ] * len(fg))
    inp["bbox"] = np.concatenate([inp["bbox"], np.zeros((len(fg), 399, 4), np.int32)], 1)
    inp["R"] = 400
    want = expected(inp)
    assert want[0]["poly_slice"][last, 0].tolist() == [want[0]["n_vertices"][0], want[0]["counts"][0]] and want[0]["n_vertices"][0] > 0
    assert want[1]["region_rings"].shape == (len(fg), 400, 2)
    if case_ == "squares":
        assert want[1]["ring_counts"][0] == 0
    else:
        assert want[1]["ring_counts"][0] == 2 and want[1]["region_rings"][last, 0].tolist() == [1, 2] and want[1]["ring_slice"][1, 0] > 0
    got = run(inp)
    same(got, want)
    assert bits(got, run(inp, force_fallback=True))


# ------------------------------------------------------------------------------------------------ (b) hand shapes
def test_hand_shapes():
    inp, want = case("hand")
    got = run(inp)
    same(got, want)
    assert inp["n_regions"].tolist() == [5, 4, 1, 1, 1]
    # image 0, regions in raster order of their first pixels: corner block, 6 x 7, 6 x 6, 3 x 3, wall
    assert got["n_holes"][0].tolist() == [1, 1, 1, 1, 2] and (got["region_rings"][0, :, 1] - got["region_rings"][0, :, 0]).tolist() == [1, 1, 0, 0, 2]
    assert got["ring_area2"][:4].tolist() == [158, 108, 158, 176] and got["ring_region"][:4].tolist() == [0, 1, 4, 4]
    sl = got["ring_slice"]
    ring = lambda q: got["ring_pos"][sl[q, 0]:sl[q, 1]].tolist()
    assert ring(0) == [[9, 1], [9, 9], [1, 9], [1, 1], [9, 1]]                                                # one pixel from the image corner
    assert ring(1) == [[23, 2], [23, 8], [16, 8], [16, 2], [23, 2]]                                           # the 6 x 7 hole
    assert ring(2) == [[12, 16], [12, 24], [4, 24], [4, 16], [12, 16]] and ring(3) == [[22, 16], [22, 24], [13, 24], [13, 16], [22, 16]]      # the wall
    # image 1: spur, island (its own region has no hole), diamond - the staircase takes all four insertions of step D in the reversed order
    assert got["n_holes"][1, :4].tolist() == [1, 1, 0, 1]
    q = int(got["region_rings"][1, 3, 0])
    d = np.diff(got["ring_pos"][sl[q, 0]:sl[q, 1]], axis=0)
    assert sl[q, 1] - sl[q, 0] > 40 and {tuple(v) for v in d.tolist()} >= {(1, 0), (-1, 0), (0, 1), (0, -1)}
    # the discs: nothing kept (bits 0 and 2), a junction ring, two matched junctions leave the ring
    q0 = int(got["region_rings"][2, 0, 0])
    assert got["ring_flags"][q0:q0 + 3].tolist() == [5, 1, 0] and (sl[q0:q0 + 3, 1] - sl[q0:q0 + 3, 0]).tolist()[:2] == [0, 25]
    assert bits(got, run(inp)) and bits(got, run(inp, force_fallback=True))


# ------------------------------------------------------------------------------------------------ (c) the outer outputs are those of p3_hisup_polygons
@pytest.mark.parametrize("name", ["shape_set", "junction_cases", "big_set"])
def test_outer_outputs_equal_the_outer_entry(name):
    inp = inputs(R.shape_set(), [NOJ] * 3) if name == "shape_set" else inputs(*getattr(R, name)())
    t = tensors(inp)
    old, new = _hip().hisup_polygons_device(*t), _hip().hisup_polygon_rings_device(*t)
    V = int(old["counts"][0])
    assert V > 0 and int(new["status"]) == 0 == int(old["status"])
    for k in OUTER:
        a, b = old[k].cpu().numpy(), new[k].cpu().numpy()
        assert a.shape == b.shape and a[:V if k in ("pos", "src") else None].tobytes() == b[:V if k in ("pos", "src") else None].tobytes(), k


# ------------------------------------------------------------------------------------------------ (d) 224 x 224: both forms, the hand-over between them
def test_big_images_both_forms_and_an_image_alone():
    """a region whose box is past the LDS form with a 20 x 20 and a 5 x 5 hole, a 40 x 40 block with a 30 x 30 hole, and a region whose box fits the LDS
    form while the ring of its comb hole does not: the second form takes it over at that hole"""
    inp, want = case("big")
    got = run(inp)
    same(got, want)
    n, V, longest = want[1]["ring_counts"]
    assert n == 4 and longest > 100 and want[1]["ring_flags"].tolist()[:3] == [0, 1, 1] and want[1]["n_holes"][0].sum() == 3
    assert len(Q.region_rings(inp["labels"][2] == 2, NOJ)[1][0]["ring"]) > 5120                              # past the LDS ring
    assert bits(got, run(inp, force_fallback=True)) and bits(got, run(inp))
    alone = run(inp, sel=slice(0, 1))
    r0, v0 = int(got["region_rings"][0, -1, 1]), int(got["ring_slice"][got["region_rings"][0, -1, 1] - 1, 1])
    assert alone["ring_counts"][:2].tolist() == [r0, v0] and np.array_equal(alone["region_rings"][0], got["region_rings"][0])
    assert alone["ring_pos"][:v0].tobytes() == got["ring_pos"][:v0].tobytes() and np.array_equal(alone["ring_src"][:v0], got["ring_src"][:v0])
    for k in ("ring_slice", "ring_region", "ring_flags", "ring_area2"):
        assert np.array_equal(alone[k][:r0], got[k][:r0]), k
    assert np.array_equal(alone["n_holes"][0], got["n_holes"][0]) and alone["pos"][:alone["counts"][0]].tobytes() == got["pos"][:alone["counts"][0]].tobytes()
    last = run(inp, sel=slice(2, 3))                                                                          # the image with the hand-over, alone
    n2 = int(last["ring_counts"][0])
    assert n2 == n - r0 and np.array_equal(last["ring_area2"][:n2], got["ring_area2"][r0:n]) and np.array_equal(last["ring_flags"][:n2], got["ring_flags"][r0:n])
    assert last["ring_pos"][:V - v0].tobytes() == got["ring_pos"][v0:V].tobytes()


# ------------------------------------------------------------------------------------------------ (e) capacities
@pytest.mark.parametrize("short", ["max_rings", "max_ring_vertices", None])
def test_capacity_one_short_sets_the_status_and_writes_nothing_outside(short):
    hip = _hip()
    inp, want = case("hand")
    n, V, longest = want[1]["ring_counts"]
    t = tensors(inp)
    caps = dict(max_vertices=want[0]["counts"][0], max_rings=n, max_ring_vertices=V)
    if short:
        caps[short] -= 1
    status = {"max_rings": 8, "max_ring_vertices": 16, None: 0}[short]
    untouched = {"max_rings": ("ring_pos", "ring_src", "ring_slice", "ring_region", "ring_flags", "ring_area2"), "max_ring_vertices": ("ring_pos", "ring_src"),
                 None: ()}[short]
    out = G.guarded_run(lambda **kw: hip.hisup_polygon_rings_device(*t, **caps, **kw), untouched=untouched)
    got = {k: out[k].cpu().numpy() for k in KEYS}
    assert got["status"].tolist() == [status] and got["ring_counts"].tolist() == [n, V, longest]             # the true counts either way
    same_outer(got, want[0])
    assert np.array_equal(got["region_rings"], want[1]["region_rings"]) and np.array_equal(got["n_holes"], want[1]["n_holes"])
    if short == "max_ring_vertices":
        same_rings(got, want[1], vertices=False)
    if short is None:
        same(got, want)
        full = hip.hisup_polygon_rings(*t)
        assert full["counts"] == tuple(want[0]["counts"]) and full["ring_counts"] == (n, V, longest)
        assert full["ring_pos"].shape == (V, 2) and full["ring_flags"].shape == (n,) and full["ring_pos"].cpu().numpy().tobytes() == want[1]["ring_pos"].tobytes()
    else:
        with pytest.raises(hip.P3Error, match=short):
            hip.hisup_polygon_rings(*t, **caps)


# ------------------------------------------------------------------------------------------------ (f) the whole model
def test_whole_model_forward_val_with_inner_rings(monkeypatch):
    """the model with random weights finds next to no region, so the remask logits that reach p3_hisup_regions are planted (tests/hisup_predict_ref.py):
    the first and the last image of big_ring_set; everything after the region kernel is the model's own path"""
    from pixelspointspolygons_amd import hip, hisup
    from pixelspointspolygons_amd.config import make_config
    from pixelspointspolygons_amd.synthetic import make_inputs
    from tests import hisup_predict_ref as P
    torch.manual_seed(11)
    cfg = make_config("vit_cnn", "hisup", vit_depth=1, precision="fp32", device=DEV)
    model = hisup.HiSupModel(cfg, local_rank=0).eval()
    B = 2
    img = make_inputs(B, seed=4)["image"].to(DEV)
    fg = Q.big_ring_set()[0][[0, 2]]
    logits = torch.from_numpy(np.stack([P.planted_mask_logits(fg[b], seed=21 + b) for b in range(B)])).to(DEV)
    real = hip.hisup_regions_device
    monkeypatch.setattr(hip, "hisup_regions_device", lambda remask, *a, **kw: real(logits, *a, **kw))
    plain, _ = model.forward_val(img, None, None, polygons=True)
    again, _ = model.forward_val(img, None, None, polygons=True, inner_rings=False)
    assert set(plain) == set(again) == {"juncs_pred", "mask_pred", "regions", "polys_pred", "scores", "poly_flags"}      # the default is unchanged
    dev, _ = model.forward_val_device(img, None, None, polygons=True, inner_rings=True)
    assert set(dev["polygons"]) == set(KEYS)
    out, _ = model.forward_val(img, None, None, polygons=True, inner_rings=True)
    assert set(out) == set(plain) | {"poly_parts"}
    total = rings = 0
    for b in range(B):
        rg, jp = out["regions"][b], out["juncs_pred"][b]
        n = len(rg["area"])
        ju, counts = R.junction_inputs([jp])
        a = (rg["labels"][None], [n], ju, counts, max(n, 1))
        outer, inner = R.polygons(*a), Q.rings(*a)
        assert min(outer["margin_t"], inner["margin_t"]) >= 1e-9 and min(outer["margin_d"], inner["margin_d"]) >= 1e-9
        keep = [i for i in range(n) if not outer["poly_flags"][0, i] & 4]
        assert np.array_equal(out["poly_flags"][b], outer["poly_flags"][0, :n]) and np.array_equal(out["scores"][b], rg["score"][keep])
        assert len(out["polys_pred"][b]) == len(out["poly_parts"][b]) == len(keep) == len(plain["polys_pred"][b])
        for poly, parts, old, i in zip(out["polys_pred"][b], out["poly_parts"][b], plain["polys_pred"][b], keep):
            want, want_parts = Q.concatenated(outer, inner, 0, i)
            assert poly.dtype == np.float64 and poly.tobytes() == want.tobytes() and parts == want_parts
            assert poly[:parts[0]].tobytes() == old.tobytes()                                                # the outer polygon of the plain call comes first
            rings += len(parts) - 1
        assert all(p.tobytes() == q.tobytes() for p, q in zip(plain["polys_pred"][b], again["polys_pred"][b]))
        total += len(keep)
    print("regions with a polygon:", total, "inner rings:", rings)
    assert total == 7 and rings == 4 and [int(n) for n in (len(r["area"]) for r in out["regions"])] == [5, 2]
