"""p3_hisup_polygons on the GPU through the public wrappers: every output equals the restatement (tests/hisup_polygon_ref.py, pinned to the reference's
`get_poly_crowdai` by tests/test_hisup_polygon_cpu.py) bit for bit - positions, sources, slices, flags, hole pixels and counts.  Inputs are made the way
p3_hisup_regions / p3_hisup_junctions write them.  No t_i lies within 1e-9 degrees of 10 or 350 and no distance within 1e-9 of 5 (asserted), so the last
bit of atan2 or of a root decides nothing."""
import numpy as np
import pytest
import torch

from tests import guard as G
from tests import hisup_polygon_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("pos", "src", "poly_slice", "poly_flags", "hole_pixels", "n_vertices", "counts", "status")


def _hip():
    from pixelspointspolygons_amd import hip
    return hip


def inputs(fg, juncs):
    labels, n_regions, bbox, Rr = R.region_inputs(fg)
    ju, counts = R.junction_inputs(juncs)
    return dict(labels=labels, n_regions=n_regions, bbox=bbox, juncs=ju, counts=counts, R=Rr)


def run(inp, sel=slice(None), **kw):
    t = [torch.from_numpy(np.ascontiguousarray(inp[k][sel])).to(DEV) for k in ("labels", "n_regions", "bbox", "juncs", "counts")]
    out = _hip().hisup_polygons_device(*t, **kw)
    return {k: out[k].cpu().numpy() for k in KEYS}


def expected(inp, sel=slice(None)):
    want = R.polygons(inp["labels"][sel], inp["n_regions"][sel], inp["juncs"][sel], inp["counts"][sel], inp["R"])
    assert want["margin_t"] >= 1e-9 and want["margin_d"] >= 1e-9
    return want


def same(got, want):
    V, longest = want["counts"]
    assert got["status"].tolist() == [0] and got["counts"].tolist() == [V, longest]
    assert np.array_equal(got["poly_slice"], want["poly_slice"]) and np.array_equal(got["poly_flags"], want["poly_flags"])
    assert np.array_equal(got["hole_pixels"], want["hole_pixels"]) and np.array_equal(got["n_vertices"], want["n_vertices"])
    assert np.array_equal(got["src"][:V], want["src"])
    assert got["pos"][:V].tobytes() == want["pos"].tobytes()


def bits(a, b):
    V = int(a["counts"][0])
    return all(np.array_equal(a[k], b[k]) for k in KEYS[2:]) and a["pos"][:V].tobytes() == b["pos"][:V].tobytes() and np.array_equal(a["src"][:V], b["src"][:V])


# ------------------------------------------------------------------------------------------------ (a) the reference's own output
@pytest.mark.parametrize("first", [0, 3])
def test_golden_regions(first):
    fg, juncs, polys = R.load_fixture()
    inp = inputs(fg[first:first + 3], juncs[first:first + 3])
    got = run(inp)
    same(got, expected(inp))
    seen = 0
    for b in range(3):
        for l in range(1, int(inp["n_regions"][b]) + 1):
            s = got["poly_slice"][b, l - 1]
            assert got["pos"][s[0]:s[1]].astype(np.float64).tobytes() == polys[(first + b, l)].tobytes()       # the fixture itself
            seen += 1
    assert seen >= 60


# ------------------------------------------------------------------------------------------------ (b) shapes
def test_shape_set():
    inp = inputs(R.shape_set(), [np.zeros((0, 2))] * 3)
    got = run(inp)
    same(got, expected(inp))
    assert inp["n_regions"].tolist() == [6, 3, 1]
    sl = got["poly_slice"]
    assert got["pos"][sl[0, 1, 0]:sl[0, 1, 1]].tolist() == [[3, 2], [3, 5], [8, 5], [8, 2], [3, 2]]           # the rectangle: top-left first, then down
    assert (sl[0, :, 1] - sl[0, :, 0]).tolist() == [21, 5, 7, 5, 9, 5]       # diagonal, rectangle, L, pixel, diagonal contact, U (raster order of first pixels)
    assert got["poly_flags"][1, :3].tolist() == [0, 2, 0] and got["hole_pixels"][1, 1] == 9                   # the ring keeps its outer polygon
    assert got["pos"][sl[2, 0, 0]:sl[2, 0, 1]].tolist() == [[0, 0], [0, 48], [48, 48], [48, 0], [0, 0]]       # the full image


def test_big_images_take_the_workspace_form():
    """224 x 224: a region whose box is past the LDS form, one whose ring is, the full image; junction polygons among them"""
    fg, juncs = R.big_set()
    inp = inputs(fg, juncs)
    want = expected(inp)
    got = run(inp)
    same(got, want)
    assert want["poly_flags"][0, :5].tolist() == [0, 1, 2, 1, 0] and want["poly_flags"][1, 0] == 1 and want["counts"][1] > 100
    assert bits(got, run(inp, force_fallback=True))


@pytest.mark.parametrize("images", [3, 4])
def test_more_region_slots_than_one_pass_of_the_offset_scan(images):
    """400 region slots per image against the 1024 threads of hp_offsets_kernel, 8 x 8 labels, one 2 x 2 region in the first and in the last image.  3 images
    (1200 slots): the empty slots 1024 .. 1199 and n_vertices[2] hold the carry of the first pass.  4 images (1600 slots): the last image's polygon is slot 1200,
    in the second pass, and starts at the carry."""
    fg = np.zeros((images, 8, 8), bool)
    fg[0, 1:3, 1:3] = fg[images - 1, 4:6, 3:5] = True
    inp = inputs(fg, [np.zeros((0, 2))] * images)
    inp["bbox"] = np.concatenate([inp["bbox"], np.zeros((images, 399, 4), np.int32)], 1)
    inp["R"] = 400
    want = expected(inp)
    assert want["n_vertices"][0] > 0 and want["n_vertices"][1] == 0 and want["poly_slice"][images - 1, 0].tolist() == [want["n_vertices"][0], want["counts"][0]]
    got = run(inp)
    same(got, want)
    assert bits(got, run(inp, force_fallback=True))


# ------------------------------------------------------------------------------------------------ (c) junctions
def test_junction_cases():
    fg, juncs = R.junction_cases()
    inp = inputs(fg, juncs)
    got = run(inp)
    same(got, expected(inp))
    assert got["poly_flags"][0, :2].tolist() == [0, 0] and got["poly_flags"][1, :3].tolist() == [0, 1, 0]
    assert inp["counts"][2].sum() == 600 and (got["poly_flags"][2] & 1).sum() >= 10


def test_smooth_junction_polygon_keeps_no_vertex():
    """the exit after step F: more than two matched junctions and no turn over 10 degrees -> flag bits 0 and 2, no vertex"""
    inp = inputs(*R.smooth_cases())
    got = run(inp)
    same(got, expected(inp))
    assert got["poly_flags"][:, 0].tolist() == [5, 1, 0] and got["n_vertices"].tolist()[:2] == [0, 25]
    assert bits(got, run(inp, force_fallback=True))


def test_measurement_switch_marks_the_status(monkeypatch):
    """P3_HISUP_POLY_STOP cuts the kernel short for tools/bench_hisup_polygons.py: status bit 2 says so and the checking wrapper raises"""
    hip = _hip()
    inp = inputs(*R.smooth_cases())
    monkeypatch.setenv("P3_HISUP_POLY_STOP", "2")
    got = run(inp)
    assert got["status"].tolist() == [4] and got["counts"].tolist() == [0, 0]
    t = [torch.from_numpy(inp[k]).to(DEV) for k in ("labels", "n_regions", "bbox", "juncs", "counts")]
    with pytest.raises(hip.P3Error, match="P3_HISUP_POLY_STOP"):
        hip.hisup_polygons(*t)
    monkeypatch.delenv("P3_HISUP_POLY_STOP")
    assert run(inp)["status"].tolist() == [0]


def test_image_without_regions_and_label_without_pixels():
    fg, juncs = R.junction_cases()
    fg[0] = False                                                # n_regions[0] == 0; its junction list is empty too
    inp = inputs(fg, juncs)
    assert inp["n_regions"][0] == 0
    got = run(inp)
    same(got, expected(inp))
    assert got["n_vertices"][0] == 0 and not got["poly_flags"][0].any()
    # inconsistent inputs: one region more than the label map holds, with a box somewhere -> no polygon (flag bit 2), everything else as before
    inp["n_regions"] = inp["n_regions"].copy()
    inp["bbox"] = inp["bbox"].copy()
    inp["n_regions"][1] += 1
    inp["bbox"][1, 3] = (20, 20, 28, 28)
    got = run(inp)
    same(got, expected(inp))
    assert got["poly_flags"][1, 3] == 4 and got["poly_slice"][1, 3, 0] == got["poly_slice"][1, 3, 1]


# ------------------------------------------------------------------------------------------------ (d), (e) the forms, repeats, batches
@pytest.mark.parametrize("case", ["shapes", "junctions"])
def test_both_forms_and_two_runs_give_the_same_bits(case):
    inp = inputs(R.shape_set(), [np.zeros((0, 2))] * 3) if case == "shapes" else inputs(*R.junction_cases())
    a, b, c = run(inp), run(inp), run(inp, force_fallback=True)
    assert bits(a, b) and bits(a, c)
    same(c, expected(inp))


def test_an_image_alone_equals_the_image_inside_the_batch():
    inp = inputs(*R.junction_cases())
    whole = run(inp)
    for b in range(3):
        alone = run(inp, sel=slice(b, b + 1))
        s0 = whole["poly_slice"][b, 0, 0]
        n = int(whole["n_vertices"][b])
        assert alone["counts"][0] == n and np.array_equal(alone["poly_slice"][0], whole["poly_slice"][b] - s0)
        assert alone["pos"][:n].tobytes() == whole["pos"][s0:s0 + n].tobytes() and np.array_equal(alone["src"][:n], whole["src"][s0:s0 + n])
        assert np.array_equal(alone["poly_flags"][0], whole["poly_flags"][b]) and np.array_equal(alone["hole_pixels"][0], whole["hole_pixels"][b])


# ------------------------------------------------------------------------------------------------ (f) capacity
def test_capacity_one_short_sets_the_status_and_writes_nothing_outside():
    hip = _hip()
    inp = inputs(*R.junction_cases())
    want = expected(inp)
    V, longest = want["counts"]
    t = [torch.from_numpy(inp[k]).to(DEV) for k in ("labels", "n_regions", "bbox", "juncs", "counts")]
    for nv, status in ((V - 1, 1), (V, 0)):
        out = G.guarded_run(lambda **kw: hip.hisup_polygons_device(*t, max_vertices=nv, **kw), untouched=("pos", "src") if status else ())      # documented: pos / src stay untouched
        got = {k: out[k].cpu().numpy() for k in KEYS}
        assert len(out) == 8 and got["status"].tolist() == [status] and got["counts"].tolist() == [V, longest]                  # the true counts either way
        assert np.array_equal(got["poly_slice"], want["poly_slice"]) and np.array_equal(got["n_vertices"], want["n_vertices"])
        assert np.array_equal(got["poly_flags"], want["poly_flags"]) and np.array_equal(got["hole_pixels"], want["hole_pixels"])
        if status == 0:
            same(got, want)
    with pytest.raises(hip.P3Error, match="max_vertices"):
        hip.hisup_polygons(*t, max_vertices=V - 1)
    full = hip.hisup_polygons(*t)
    assert full["counts"] == (V, longest) and full["pos"].shape == (V, 2) and full["pos"].cpu().numpy().tobytes() == want["pos"].tobytes()


# ------------------------------------------------------------------------------------------------ (g) the whole model
def test_whole_model_forward_val_with_polygons():
    from pixelspointspolygons_amd import hisup
    from pixelspointspolygons_amd.config import make_config
    from pixelspointspolygons_amd.synthetic import make_inputs
    torch.manual_seed(11)
    cfg = make_config("vit_cnn", "hisup", vit_depth=1, precision="fp32", device=DEV)
    model = hisup.HiSupModel(cfg, local_rank=0).eval()
    model.max_regions = 112 * 112
    B = 2
    img = make_inputs(B, seed=4)["image"].to(DEV)
    plain, _ = model.forward_val(img, None, None)
    assert set(plain) == {"juncs_pred", "mask_pred", "regions"}                                               # the default call is unchanged
    dev, _ = model.forward_val_device(img, None, None)
    assert "polygons" not in dev
    out, _ = model.forward_val(img, None, None, polygons=True)
    assert set(out) == {"juncs_pred", "mask_pred", "regions", "polys_pred", "scores", "poly_flags"}
    total = 0
    for b in range(B):
        rg, jp = out["regions"][b], out["juncs_pred"][b]
        n = len(rg["area"])
        assert np.array_equal(rg["labels"], plain["regions"][b]["labels"]) and np.array_equal(jp, plain["juncs_pred"][b])
        ju, counts = R.junction_inputs([jp])
        want = R.polygons(rg["labels"][None], [n], ju, counts, max(n, 1))
        assert want["margin_t"] >= 1e-9 and want["margin_d"] >= 1e-9
        flags = want["poly_flags"][0, :n]
        assert np.array_equal(out["poly_flags"][b], flags)
        keep = [i for i in range(n) if not flags[i] & 4]
        assert len(out["polys_pred"][b]) == len(keep) == len(out["scores"][b])
        assert np.array_equal(out["scores"][b], rg["score"][keep])
        for poly, i in zip(out["polys_pred"][b], keep):
            s = want["poly_slice"][0, i]
            assert poly.dtype == np.float64 and poly.shape == (s[1] - s[0], 2) and np.array_equal(poly[0], poly[-1])
            assert poly.tobytes() == want["pos"][s[0]:s[1]].astype(np.float64).tobytes()
        total += len(keep)
    print("regions with a polygon:", total)
    assert total > 0
