"""p3_skeleton_from_contours and p3_asm_plan (csrc/skeleton_init.hip) through hip.skeleton_from_contours / hip.asm_plan, polygonize_asm.init_skeletons /
asm_plan_device / polygonize_device and polygonize_post.polygonize_asm_pieces.  Oracles (tests/skeleton_init_ref.py): find_contours_ref -> as_float32 ->
contours_to_skeleton(min_area) -> skeletons_to_tensorskeleton for the container, the host AsmPlan for the plan.  Every comparison is exact: torch.equal on the
integer arrays and on the fp32 bits of pos."""
import numpy as np
import pytest
import torch

from tests import asm_ref as R
from tests import guard as G
from tests import skeleton_init_ref as S
from tests.helpers import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
BATCH = ["flat", "s1", "checker", "s5", "s6", "checker"]          # images without a kept path at the start, in the middle and at the end
CONTAINER = ("pos", "degrees", "path_index", "path_delim", "batch", "batch_delim")


def device_skeleton(names, min_area=S.MIN_AREA):
    from pixelspointspolygons_amd import polygonize_asm as A
    return A.init_skeletons(torch.tensor(S.maps(names)).to(DEV), S.LEVEL, min_area)


def assert_container(ts, ref, what=""):
    for k in CONTAINER:
        got, want = getattr(ts, k), getattr(ref, k)
        assert got.is_cuda and got.dtype == want.dtype and got.shape == want.shape, f"{what}{k}: {got.dtype} {tuple(got.shape)}, the oracle {want.dtype} {tuple(want.shape)}"
        same = torch.equal(got.cpu().view(torch.int32), want.view(torch.int32)) if k == "pos" else torch.equal(got.cpu(), want)
        assert same, f"{what}{k} differs"
    assert ts.batch_size == ref.batch_size


def assert_plan(plan, host, what=""):
    for k in host.FIELDS:
        got, want = getattr(plan, k), getattr(host, k)
        assert got.is_cuda and got.dtype == torch.int32 and got.shape == want.shape and torch.equal(got.cpu(), want.cpu()), f"{what}{k}"
    assert (plan.num_nodes, plan.num_slots, plan.num_comps, plan.max_comp) == (host.num_nodes, host.num_slots, host.num_comps, host.max_comp), what


def plan_of(path_index, path_delim, N):
    from pixelspointspolygons_amd import hip, polygonize_asm as A
    idx, delim = torch.as_tensor(path_index).to(DEV), torch.as_tensor(path_delim).to(DEV)
    return A.AsmDevicePlan(hip.asm_plan(idx, delim, N), N, idx.shape[0])


# ---------------------------------------------------------------------------------------------------------------- container
@pytest.mark.parametrize("seed", range(1, 9))
def test_single_images_equal_the_oracle(seed):
    name = f"s{seed}"
    S.check_input([name])
    ts, ref = device_skeleton([name]), S.oracle([name])
    assert_container(ts, ref)
    assert_plan(ts.plan, ref.plan)                                    # components are the paths
    firsts = ref.path_index[ref.path_delim[:-1]]
    closed = firsts == ref.path_index[ref.path_delim[1:] - 1]
    assert torch.equal(torch.diff(ts.plan.cn_occ.cpu())[firsts[closed]], torch.full((int(closed.sum()),), 2, dtype=torch.int32))


def test_batch_with_empty_images_and_each_image_alone():
    S.check_input(BATCH)
    ts, ref = device_skeleton(BATCH), S.oracle(BATCH)
    assert ref.batch_delim[1] == 0 and ref.batch_delim[2] == ref.batch_delim[3] and ref.batch_delim[5] == ref.batch_delim[6] and ref.num_paths > 8
    assert_container(ts, ref)
    assert_plan(ts.plan, ref.plan)
    for b, name in enumerate(BATCH):
        if name in ("flat", "checker"):
            continue
        alone = device_skeleton([name])
        rows = (ts.batch == b).nonzero()[:, 0]
        n0, p0, p1 = int(rows[0]), int(ts.batch_delim[b]), int(ts.batch_delim[b + 1])
        m0, m1 = int(ts.path_delim[p0]), int(ts.path_delim[p1])
        assert torch.equal(alone.pos.view(torch.int32), ts.pos[rows].view(torch.int32)) and torch.equal(alone.degrees, ts.degrees[rows])
        assert torch.equal(alone.path_index, ts.path_index[m0:m1] - n0) and torch.equal(alone.path_delim, ts.path_delim[p0:p1 + 1] - m0)


def test_min_area_variants_on_the_checkerboard():
    from pixelspointspolygons_amd import hip
    S.check_input(["checker"])
    S.check_input(["checker"], -1.0)
    for min_area, paths in ((-1.0, 1038), (None, 1040)):          # -1: only the length rule drops (the two 2-point open contours; a closed one counts its repeated point)
        ts, ref = device_skeleton(["checker"], min_area), S.oracle(["checker"], min_area)
        assert ref.num_paths == paths
        assert_container(ts, ref, f"min_area={min_area}: ")
    assert device_skeleton(["checker"]) is None and device_skeleton(["flat"]) is None
    c = hip.init_contours(torch.tensor(S.maps(["checker"])).to(DEV), S.LEVEL)
    out = hip.skeleton_from_contours(c["pos"], c["poly_slice"], c["poly_batch"], c["is_endpoint"], 1, S.MIN_AREA)
    assert out["counts"] == (0, 0, 0, 0) and out["batch_delim"].tolist() == [0, 0] and out["path_delim"].tolist() == [0] and out["pos"].shape == (0, 2)


def test_larger_maps_equal_the_oracle_and_two_runs_give_the_same_bits():
    names = ["L1", "L2"]
    S.check_input(names)
    ref = S.oracle(names)
    lens = torch.diff(ref.path_delim)
    assert int(lens.max()) > 256 and sum(len(S.contours(n)) for n in names) > 64          # contours longer than a workgroup, more contours than a wave
    a, b = device_skeleton(names), device_skeleton(names)
    assert_container(a, ref)
    assert_plan(a.plan, ref.plan)
    for k in CONTAINER:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    for k in ref.plan.FIELDS:
        assert torch.equal(getattr(a.plan, k), getattr(b.plan, k)), k


@pytest.mark.parametrize("short", ["exact", "nodes", "slots", "paths"])
def test_a_capacity_one_short_sets_status_keeps_the_counts_and_the_guards(short):
    from pixelspointspolygons_amd import hip
    names = ["s1", "s5"]
    ref = S.oracle(names)
    N, M, P = ref.num_nodes, ref.path_index.shape[0], ref.num_paths
    longest = int((torch.diff(ref.path_delim) - (ref.path_index[ref.path_delim[:-1]] == ref.path_index[ref.path_delim[1:] - 1]).long()).max())
    c = hip.init_contours(torch.tensor(S.maps(names)).to(DEV), S.LEVEL)
    caps = dict(nodes=N, slots=M, paths=P)
    if short != "exact":
        caps[short] -= 1
    v = G.guarded_run(lambda **kw: hip.skeleton_from_contours_device(c["pos"], c["poly_slice"], c["poly_batch"], c["is_endpoint"], 2, S.MIN_AREA, caps["nodes"],
                                                                     caps["slots"], caps["paths"], **kw), unwritten=short != "exact")
    # nothing outside the views; with the exact capacities every element was written
    assert len(v) == 8 and v["counts"].tolist() == [N, M, P, longest] and v["status"].item() == (0 if short == "exact" else 1)
    if short == "exact":
        for k in ("degrees", "path_index", "path_delim", "batch", "batch_delim"):
            assert torch.equal(v[k].cpu(), getattr(ref, k)), k
        assert torch.equal(v["pos"].cpu().view(torch.int32), ref.pos.view(torch.int32))
    else:
        assert torch.equal(v["batch_delim"].cpu(), ref.batch_delim)
        with pytest.raises(hip.P3Error):
            hip.skeleton_from_contours(c["pos"], c["poly_slice"], c["poly_batch"], c["is_endpoint"], 2, S.MIN_AREA, max_nodes=caps["nodes"], max_slots=caps["slots"],
                                       max_paths=caps["paths"])


def test_more_contours_than_one_pass_of_the_scan_workgroup():
    """1025 open contours of 3 points, 600 in image 0 and 425 in image 1, no filter: sk_scan_kernel is one workgroup of 1024 threads, so the last contour takes
    its first node, its first slot and its path number from the carry of the first pass"""
    from pixelspointspolygons_amd import hip, polygonize_asm as A
    P, split = 1025, 600
    i = np.arange(P, dtype=np.float32)
    cs = [np.array([[1 + k, 1], [1 + k, 2], [1.5 + k, 2]], dtype=np.float32) for k in i]
    ref = A.skeletons_to_tensorskeleton([A.contours_to_skeleton(cs[:split], None), A.contours_to_skeleton(cs[split:], None)])
    assert ref.num_paths == P and ref.pos.shape[0] == 3 * P
    sl = torch.arange(P, dtype=torch.int64)
    end = torch.tensor([1, 0, 1], dtype=torch.uint8).repeat(P)
    out = hip.skeleton_from_contours(torch.from_numpy(np.concatenate(cs)).to(DEV), torch.stack([3 * sl, 3 * sl + 3], 1).to(DEV),
                                     (sl >= split).to(torch.int32).to(DEV), end.to(DEV), 2, None)
    assert out["counts"] == (3 * P, 3 * P, P, 3)
    assert torch.equal(out["pos"].cpu().view(torch.int32), ref.pos.view(torch.int32))
    for k in ("degrees", "path_index", "path_delim", "batch", "batch_delim"):
        assert torch.equal(out[k].cpu(), getattr(ref, k)), k


# ---------------------------------------------------------------------------------------------------------------- plan
def test_plan_of_the_fixture_container_equals_the_host_plan():
    from pixelspointspolygons_amd import polygonize_asm as A
    ts = R.tensors_of(load_golden("asm.npz")[0])
    N = ts["pos"].shape[0]
    host = A.AsmPlan(ts["path_index"].numpy(), ts["path_delim"].numpy(), N)
    plan = plan_of(ts["path_index"], ts["path_delim"], N)
    assert (plan.num_comps, plan.max_comp) == (10, 80)
    assert_plan(plan, host)


def test_plan_of_a_path_longer_than_one_pass_of_the_scan_workgroup():
    """one open path over 4097 nodes in a permuted order: ap_scan takes 1024 threads x 4 entries = 4096 a pass, so the last slot and the last node take their
    prefix from the carry of the first pass; the link scan of ap_components (1024 a pass) crosses four times and finds no link"""
    from pixelspointspolygons_amd import polygonize_asm as A
    N = 4097
    idx, delim = np.random.default_rng(3).permutation(N).astype(np.int64), np.array([0, N], dtype=np.int64)
    host = A.AsmPlan(idx, delim, N)
    assert (host.num_comps, host.max_comp) == (1, N)
    assert_plan(plan_of(idx, delim, N), host)


def test_plan_of_the_adversarial_graph_equals_the_host_plan():
    from pixelspointspolygons_amd import polygonize_asm as A
    idx, delim, N = S.adversarial_graph()
    host = A.AsmPlan(idx, delim, N)
    assert (host.num_comps, host.max_comp) == (172, 720)
    a, b = plan_of(idx, delim, N), plan_of(idx, delim, N)
    assert_plan(a, host)
    for k in host.FIELDS:
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def test_plan_of_degenerate_sizes():
    from pixelspointspolygons_amd import polygonize_asm as A
    none = np.zeros(0, dtype=np.int64)
    for idx, delim, N in ((none, np.zeros(1, dtype=np.int64), 7), (none, np.zeros(1, dtype=np.int64), 0), (none, none, 3)):
        host = A.AsmPlan(idx, delim, N)
        assert host.num_comps == N and host.max_comp == min(N, 1)          # N single-node components
        assert_plan(plan_of(idx, delim, N), host, f"N={N}: ")
    ring = np.concatenate([np.arange(5000), [0]]).astype(np.int64)
    delim = np.array([0, 5001], dtype=np.int64)
    host = A.AsmPlan(ring, delim, 5000)
    assert host.num_comps == 1 and host.max_comp == 5000          # above the optimiser's 4096-node LDS cap
    assert_plan(plan_of(ring, delim, 5000), host, "ring: ")


def test_a_node_id_equal_to_n_raises_and_writes_nothing_outside_the_outputs():
    from pixelspointspolygons_amd import hip
    N = 12
    idx = torch.tensor([0, 1, 2, 3, 0, 4, 5, N, 7, 8], dtype=torch.int64, device=DEV)
    delim = torch.tensor([0, 5, 10], dtype=torch.int64, device=DEV)
    v = G.guarded_run(lambda **kw: hip.asm_plan_device(idx, delim, N, **kw), unwritten=True)
    assert len(v) == 8 and v["status"].item() & 2
    with pytest.raises(hip.P3Error, match="outside"):
        hip.asm_plan(idx, delim, N)
    with pytest.raises(hip.P3Error, match="outside"):
        hip.asm_plan(torch.tensor([0, -1], dtype=torch.int64, device=DEV), delim[:1], N)
    with pytest.raises(hip.P3Error, match="outside"):
        hip.asm_plan(idx[:3], delim[:1], 0)


def test_asm_plan_device_builds_the_plan_of_a_foreign_container_and_the_optimiser_takes_it():
    """a container that is no TensorSkeleton of this package: the optimiser trusts the device-built plan on it and does not rebuild it on the host"""
    from types import SimpleNamespace

    from pixelspointspolygons_amd import polygonize_asm as A
    ref = S.oracle(["s1"])
    foreign = SimpleNamespace(**{k: getattr(ref, k).to(DEV) for k in CONTAINER}, batch_size=1)
    foreign.plan = A.asm_plan_device(foreign)
    assert_plan(foreign.plan, ref.plan)
    seg, cf = _maps(["s1"])
    opt = A.TensorSkeletonOptimizer(A.ASM_DEFAULTS, foreign, seg[:, 0], cf)
    assert opt.plan is foreign.plan


# ---------------------------------------------------------------------------------------------------------------- chain
def _maps(names):
    """seg [B, 1, H, W] and the frame field of test_init_contours_gpu.py's chain test (random directions, a small c2)"""
    m = S.maps(names)
    rng = np.random.default_rng(23)
    theta = rng.uniform(0, np.pi, m.shape)
    c0, c2 = -np.exp(4j * theta), rng.normal(0, 0.05, m.shape) + 1j * rng.normal(0, 0.05, m.shape)
    cf = torch.tensor(np.stack([c0.real, c0.imag, c2.real, c2.imag], 1), dtype=torch.float32).to(DEV)
    return torch.tensor(m[:, None]).to(DEV), cf


def _todays_path(seg, cf, cfg):
    """init_contours, download, contours_to_skeleton(min_area), skeletons_to_tensorskeleton, .to(device), TensorSkeletonOptimizer.optimize()"""
    from pixelspointspolygons_amd import polygonize_acm, polygonize_asm as A
    tp = polygonize_acm.init_contours(seg, cfg["data_level"])
    contours_batch = polygonize_acm.tensorpoly_to_contours_batch(tp)
    ts = A.skeletons_to_tensorskeleton([A.contours_to_skeleton(c, cfg["min_area"]) for c in contours_batch]).to(seg.device)
    return A.TensorSkeletonOptimizer(cfg, ts, seg[:, 0], cf).optimize()


@pytest.fixture(scope="module")
def chain():
    from pixelspointspolygons_amd import polygonize_asm as A
    seg, cf = _maps(BATCH)
    cfg = {**A.ASM_DEFAULTS, "init_method": "marching_squares"}
    return seg, cf, cfg, A.polygonize_device(seg, cf, cfg)


def test_polygonize_device_equals_todays_path(chain):
    from pixelspointspolygons_amd import polygonize_asm as A
    seg, cf, cfg, got = chain
    S.check_input(BATCH)
    want = _todays_path(seg, cf, cfg)
    assert got.pos.is_cuda and isinstance(got.plan, A.AsmDevicePlan)
    assert torch.equal(got.pos.view(torch.int32), want.pos.view(torch.int32)) and torch.equal(got.path_index, want.path_index)
    assert float((got.pos.cpu() - S.oracle(BATCH).pos).abs().max()) > 1e-3          # the optimiser did run
    short = {**cfg, "loss_params": {**cfg["loss_params"], "coefs": {**cfg["loss_params"]["coefs"], "step_thresholds": [0, 2, 4, 5]}}}
    a, b = A.polygonize_device(seg, cf, short), _todays_path(seg, cf, short)
    assert torch.equal(a.pos.view(torch.int32), b.pos.view(torch.int32)) and not torch.equal(a.pos, got.pos)
    flat_seg, flat_cf = _maps(["flat", "checker"])
    assert A.polygonize_device(flat_seg, flat_cf, cfg) is None


def test_polygonize_asm_pieces_equals_the_corner_split_of_the_optimised_skeleton(chain):
    from pixelspointspolygons_amd import polygonize_post as Q
    seg, cf, cfg, ts = chain
    keys = ("out_pos", "out_src", "piece_slice", "piece_poly", "piece_batch")
    want, got = Q.corner_split_skeleton(ts, cf, 1), Q.polygonize_asm_pieces(seg, cf, cfg, tolerance=1)
    assert got["counts"] == want["counts"] and got["counts"][1] > 0 and got["batch_size"] == len(BATCH)
    for k in keys:
        assert torch.equal(got[k], want[k]), k
    many = Q.polygonize_asm_pieces(seg, cf, {**cfg, "tolerance": [0.5, 2]})
    assert sorted(many) == ["tol_0.5", "tol_2"]
    for t in (0.5, 2):
        w = Q.corner_split_skeleton(ts, cf, t)
        for k in keys:
            assert torch.equal(many[f"tol_{t}"][k], w[k]), (t, k)
    flat_seg, flat_cf = _maps(["flat", "checker"])
    acm = Q.polygonize_acm_pieces(flat_seg[:1], flat_cf[:1], tolerance=1)
    empty = Q.polygonize_asm_pieces(flat_seg, flat_cf, cfg, tolerance=1)
    assert empty["counts"] == (0, 0, 0) and empty["batch_size"] == 2 and sorted(empty) == sorted(acm)
    for k in keys:
        assert empty[k].shape == acm[k].shape and empty[k].dtype == acm[k].dtype
    assert sorted(Q.polygonize_asm_pieces(flat_seg, flat_cf, cfg, tolerance=[1, 3])) == ["tol_1", "tol_3"]
