"""p3_init_contours (csrc/contours.hip) through hip.init_contours(_device) and polygonize_acm.init_contours / polygonize_device.
Reference: tests/marching_ref.find_contours_ref, the sequential coordinate-joining assembly in float64, cast to float32 - EQUAL means the same count, order,
start vertex, closedness and bits (np.array_equal, no tolerance).  A map with pixels equal to the level is held to marching_ref.link_by_edges_ref instead
(the known deviation of coordinate joining)."""
import numpy as np
import pytest
import torch

from tests import guard as G
from tests import marching_ref as M

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def want():
    """name -> the reference contours in float32, computed once"""
    return {k: M.as_float32(M.find_contours_ref(img, lv)) for k, (img, lv) in M.cases().items()}


def device_contours(maps, level):
    """[B, H, W] numpy -> (contours per image from the device TensorPoly, the TensorPoly or None)"""
    from pixelspointspolygons_amd import polygonize_acm as A
    tp = A.init_contours(torch.tensor(np.asarray(maps)).to(DEV), level)
    if tp is None:
        return [[] for _ in range(len(maps))], None
    assert tp.pos.is_cuda and tp.poly_slice.is_cuda and tp.batch.is_cuda and tp.is_endpoint.is_cuda
    return A.tensorpoly_to_contours_batch(tp), tp


def assert_same(got, ref, what):
    assert len(got) == len(ref), f"{what}: {len(got)} contours, the reference has {len(ref)}"
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.dtype == np.float32 and g.shape == r.shape, f"{what}: contour {i} has shape {g.shape}, the reference {r.shape}"
        assert np.array_equal(g, r), f"{what}: contour {i} differs, first at row {int(np.argmax((g != r).any(1)))}"


def assert_fields(tp, ref_contours_batch):
    """every field of the device TensorPoly against contours_batch_to_tensorpoly of the reference's contours"""
    from pixelspointspolygons_amd import polygonize_acm as A
    ref = A.contours_batch_to_tensorpoly(ref_contours_batch)
    assert tp.pos.dtype == torch.float32 and torch.equal(tp.pos.cpu(), ref.pos)
    assert tp.poly_slice.dtype == torch.long and torch.equal(tp.poly_slice.cpu(), ref.poly_slice)
    assert tp.batch.dtype == torch.long and torch.equal(tp.batch.cpu(), ref.batch)
    assert tp.is_endpoint.dtype == torch.bool and torch.equal(tp.is_endpoint.cpu(), ref.is_endpoint)
    assert tp.batch_size == ref.batch_size and tp.max_len == ref.max_len


@pytest.mark.parametrize("name", sorted(M.cases()))
def test_equals_find_contours_ref(want, name):
    image, level = M.cases()[name]
    got, tp = device_contours(image[None], level)
    assert_same(got[0], want[name], name)
    if want[name]:
        assert_fields(tp, [[c.astype(np.float64) for c in want[name]]])
    else:
        assert tp is None


def picked_kernel(fn):
    """what fn() returns, and the form of the doubling passes the library took for its last call"""
    from pixelspointspolygons_amd._lib import lib
    lib().p3_trace_kernels(1)
    try:
        out = fn()
        return out, lib().p3_last_kernel().decode()
    finally:
        lib().p3_trace_kernels(0)


@pytest.mark.parametrize("mode", ["image", "rounds"])
def test_both_forms_of_the_doubling_passes_equal_the_reference(want, mode, monkeypatch):
    """one launch per pass with a workgroup per image (small maps) and one launch per round (large ones), each forced on the same inputs"""
    monkeypatch.setenv("P3_IC_DOUBLING", mode)
    for name in ("serpentine96", "checkerboard12", "cross10x13", "nan9x11", "smooth33x20"):
        image, level = M.cases()[name]
        (got, _), kernel = picked_kernel(lambda: device_contours(image[None], level))
        assert kernel == {"image": "ic_rank_image_kernel", "rounds": "ic_rank_round_kernel"}[mode]
        assert_same(got[0], want[name], f"{name} ({mode})")
    a, b = M.smooth(33, 20, 7), M.smooth(33, 20, 4)
    got, tp = device_contours(np.stack([a, b]), 0.5)
    assert_fields(tp, [M.find_contours_ref(a), M.find_contours_ref(b)])


def test_a_map_over_the_one_workgroup_limit_takes_a_launch_per_round():
    """2 * 260 * 259 = 134680 edges per image, more than the 2^17 up to which one workgroup ranks an image: the library's own choice changes here"""
    image = M.smooth(260, 260, 39, bumps=14)
    ref = M.find_contours_ref(image)
    closed = [bool(np.array_equal(c[0], c[-1])) for c in ref]
    assert any(closed) and not all(closed)
    (got, tp), kernel = picked_kernel(lambda: device_contours(image[None], 0.5))
    assert kernel == "ic_rank_round_kernel"
    assert_same(got[0], M.as_float32(ref), "260 x 260")
    assert_fields(tp, [ref])
    _, kernel = picked_kernel(lambda: device_contours(M.smooth(33, 20, 7)[None], 0.5))
    assert kernel == "ic_rank_image_kernel"


def test_batch_is_image_major_and_an_image_alone_gives_the_same(want):
    from pixelspointspolygons_amd import hip
    image, level = M.cases()["smooth33x20"]
    maps = np.stack([np.full_like(image, 0.1), image, np.full_like(image, 0.9)])
    ref = want["smooth33x20"]
    got, tp = device_contours(maps, level)
    assert got[0] == [] and got[2] == []
    assert_same(got[1], ref, "image 1 of 3")
    assert_fields(tp, [[], [c.astype(np.float64) for c in ref], []])
    out = hip.init_contours(torch.tensor(maps).to(DEV), level)
    lens = [len(c) - (1 if np.array_equal(c[0], c[-1]) else 0) for c in ref]
    N, P = sum(lens), len(ref)
    assert out["counts"] == (N, P, max(lens))
    assert out["n_contours"].tolist() == [0, P, 0] and out["n_vertices"].tolist() == [0, N, 0]
    assert out["poly_batch"].dtype == torch.int32 and out["poly_batch"].tolist() == [1] * P and out["batch"].tolist() == [1] * N
    ends = np.cumsum(lens)
    assert out["poly_slice"].tolist() == [[int(e - n), int(e)] for e, n in zip(ends, lens)]
    flags = np.zeros(N, dtype=np.uint8)
    for e, n, c in zip(ends, lens, ref):
        if not np.array_equal(c[0], c[-1]):
            flags[e - n] = flags[e - 1] = 1
    assert out["is_endpoint"].dtype == torch.uint8 and np.array_equal(out["is_endpoint"].cpu().numpy(), flags)
    for b in range(3):
        alone, _ = device_contours(maps[b:b + 1], level)
        assert_same(alone[0], got[b], f"image {b} alone")


def test_more_tiles_than_one_pass_of_the_tile_scans():
    """1025 maps of 2 x 2 are 1025 edge tiles and 1025 key tiles; the workgroup that scans them has 1024 threads, so the last image's offsets come from the carry
    of the first pass.  One corner pixel above the level in every third image: a two-vertex open contour there, nothing elsewhere."""
    maps = np.zeros((1025, 2, 2), dtype=np.float32)
    maps[::3, 0, 0] = 1.0
    with_corner, empty = M.find_contours_ref(maps[0]), M.find_contours_ref(maps[1])
    assert len(with_corner) == 1 and empty == []
    ref = [with_corner if b % 3 == 0 else [] for b in range(len(maps))]
    got, tp = device_contours(maps, 0.5)
    for b in (0, 1, 3, 1020, 1023, 1024):
        assert_same(got[b], M.as_float32(ref[b]), f"image {b}")
    assert_fields(tp, ref)


def test_two_images_with_contours_keep_image_major_order():
    a, b = M.smooth(33, 20, 7), M.smooth(33, 20, 4)
    ref = [M.find_contours_ref(a), M.find_contours_ref(b)]
    assert ref[0] and ref[1]
    got, tp = device_contours(np.stack([a, b]), 0.5)
    for i in range(2):
        assert_same(got[i], M.as_float32(ref[i]), f"image {i}")
    assert_fields(tp, ref)


def test_channel_0_is_read_through_its_strides():
    from pixelspointspolygons_amd import hip
    seg = torch.tensor(np.stack([np.stack([M.smooth(16, 16, 20 + 3 * b + ch, bumps=3) for ch in range(3)]) for b in range(2)])).to(DEV)
    view = seg[:, 0]
    assert not view.is_contiguous()
    a, b = hip.init_contours(view), hip.init_contours(view.contiguous())
    assert a["counts"] == b["counts"] and a["counts"][1] > 0
    for k in ("pos", "poly_slice", "poly_batch", "batch", "is_endpoint", "n_contours", "n_vertices"):
        assert torch.equal(a[k], b[k]), k
    from pixelspointspolygons_amd import polygonize_acm as A
    got = A.tensorpoly_to_contours_batch(A.init_contours(seg))          # the 4-d form takes channel 0 itself
    for i in range(2):
        assert_same(got[i], M.as_float32(M.find_contours_ref(seg[i, 0].cpu().numpy())), f"image {i}")


def test_level_valued_pixels_follow_the_edge_definition():
    image = M.level_valued()
    assert M.has_level_pixels(image)
    got, _ = device_contours(image[None], 0.5)
    assert_same(got[0], M.as_float32(M.link_by_edges_ref(image, 0.5)), "level-valued 8 x 8")


@pytest.mark.parametrize("short", ["max_vertices", "max_contours"])
def test_overflow_sets_status_keeps_the_totals_and_writes_nothing_outside(short):
    from pixelspointspolygons_amd import hip
    x = torch.tensor(M.cases()["smooth33x20"][0][None]).to(DEV)
    full = hip.init_contours(x)
    N, P, longest = full["counts"]
    assert N > 1 and P > 1
    caps = {"max_vertices": N, "max_contours": P}
    run = lambda: G.guarded_run(lambda **kw: hip.init_contours_device(x, **caps, **kw))          # all nine outputs between guard bands, each written up to its capacity
    exact = run()          # the exact capacities fit
    assert exact["status"].tolist() == [0] and torch.equal(exact["pos"], full["pos"]) and torch.equal(exact["poly_slice"], full["poly_slice"])
    caps[short] -= 1
    out = run()
    assert out["status"].tolist() == [1] and out["counts"].tolist() == [N, P, longest]
    assert out["n_contours"].tolist() == [P] and out["n_vertices"].tolist() == [N]
    assert out["pos"].shape[0] == caps["max_vertices"] and out["poly_slice"].shape[0] == caps["max_contours"] and len(exact) == len(out) == 9
    with pytest.raises(hip.P3Error):
        hip.init_contours(x, **caps)


def test_an_output_of_the_wrong_dtype_is_refused():
    from pixelspointspolygons_amd import hip
    x = torch.tensor(M.level_valued()[None]).to(DEV)
    with pytest.raises(hip.P3Error, match="init_contours.*pos"):          # the default capacity of the 8 x 8 map, 2 * 8 * 7 vertices, in float64
        hip.init_contours_device(x, out=dict(pos=torch.empty((112, 2), dtype=torch.float64, device=DEV)))


def test_two_runs_give_the_same_bits():
    from pixelspointspolygons_amd import hip
    image, level = M.cases()["smooth64_l045"]
    x = torch.tensor(np.stack([image, M.checkerboard(64, seed=9)])).to(DEV)
    a, b = hip.init_contours(x, level), hip.init_contours(x, level)
    assert a["counts"] == b["counts"] and a["counts"][1] > 100
    for k in ("pos", "poly_slice", "poly_batch", "batch", "is_endpoint", "n_contours", "n_vertices"):
        assert torch.equal(a[k], b[k]), k


def test_polygonize_device_equals_optimize_contours_on_the_reference_contours():
    """seg -> optimised contours without a host contour: the same positions in the same order go into the same kernel, so the result is the same bits"""
    from pixelspointspolygons_amd import polygonize_acm as A
    maps = np.stack([M.smooth(33, 20, 7), M.smooth(33, 20, 4)])
    rng = np.random.default_rng(23)
    seg = torch.tensor(np.stack([maps, rng.uniform(0, 1, maps.shape).astype(np.float32)], 1)).to(DEV)          # [2, 2, 33, 20]: channel 1 is never looked at
    theta = rng.uniform(0, np.pi, maps.shape)
    c0, c2 = -np.exp(4j * theta), rng.normal(0, 0.05, maps.shape) + 1j * rng.normal(0, 0.05, maps.shape)
    cf = torch.tensor(np.stack([c0.real, c0.imag, c2.real, c2.imag], 1), dtype=torch.float32).to(DEV)
    cfg = dict(A.ACM_DEFAULTS, steps=20)
    host = [M.find_contours_ref(m, cfg["data_level"]) for m in maps]
    want = A.optimize_contours(seg, cf, host, cfg)
    tp = A.polygonize_device(seg, cf, cfg)
    assert tp.pos.is_cuda
    got = A.tensorpoly_to_contours_batch(tp)
    moved = 0.0
    for i in range(2):
        assert_same(got[i], want[i], f"image {i}")
        moved = max(moved, max(float(np.abs(g[:len(h)] - h[:len(g)].astype(np.float32)).max()) for g, h in zip(got[i], host[i])))
    assert moved > 1e-3          # the optimiser did run
    assert A.polygonize_device(torch.zeros(1, 1, 8, 8, device=DEV), torch.zeros(1, 4, 8, 8, device=DEV), cfg) is None
