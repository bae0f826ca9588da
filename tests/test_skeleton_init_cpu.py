"""ASM initialisation from marching squares on the device, the parts that need no GPU: the plan's definition restated over scipy's connected components
against the host AsmPlan, the stated properties of the seeded inputs the GPU tests use (tests/skeleton_init_ref.py), and the argument checks of the two C
entries and their wrappers."""
import numpy as np
import pytest
import torch

from tests import asm_ref as R
from tests import skeleton_init_ref as S
from tests.helpers import load_golden


def assert_plan_equals_scipy(path_index, path_delim, N, C, max_comp):
    from pixelspointspolygons_amd import polygonize_asm as A
    host, want = A.AsmPlan(path_index, path_delim, N), S.plan_by_scipy(path_index, path_delim, N)
    assert (host.num_comps, host.max_comp) == (C, max_comp) == (want["num_comps"], want["max_comp"])
    assert (host.num_nodes, host.num_slots) == (N, len(path_index))
    for k in A.AsmPlan.FIELDS:
        got = getattr(host, k)
        assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want[k]), k


def test_host_plan_equals_the_scipy_restatement_on_the_fixture_container():
    ts = R.tensors_of(load_golden("asm.npz")[0])
    N, M, P = ts["pos"].shape[0], ts["path_index"].shape[0], ts["path_delim"].shape[0] - 1
    assert (N, M, P) == (348, 362, 16)
    assert_plan_equals_scipy(ts["path_index"].numpy(), ts["path_delim"].numpy(), N, 10, 80)


def test_host_plan_equals_the_scipy_restatement_on_the_adversarial_graph():
    idx, delim, N = S.adversarial_graph()
    assert N == 900 and delim.shape[0] == 45 and int((np.diff(delim) == 0).sum()) == 1          # 44 paths, one of them empty
    assert np.unique(idx).shape[0] == 900 - 169 and int(np.bincount(idx, minlength=N).max()) >= 2
    assert_plan_equals_scipy(idx, delim, N, 172, 720)


def _census(name):
    cs = S.contours(name)
    closed = [S.is_closed(c) for c in cs]
    keep = [3 <= c.shape[0] and S.MIN_AREA < S.area(c) for c in cs]
    return cs, closed, keep


def test_small_speckled_maps_have_the_stated_contours():
    kinds, margin = set(), {}
    for seed in range(1, 9):
        name = f"s{seed}"
        cs, closed, keep = _census(name)
        assert 6 <= len(cs) <= 16 and 3 <= sum(keep) <= 10, (name, len(cs), sum(keep))
        kinds |= set(zip(closed, keep))
        margin[seed] = min(abs(S.area(c) - S.MIN_AREA) for c in cs)
        S.check_input([name])
    assert kinds == {(True, True), (True, False), (False, True), (False, False)}          # kept and dropped, open and closed
    assert min(margin, key=margin.get) == 5 and 0.21 < margin[5] < 0.23


def test_large_speckled_maps_have_the_stated_contours():
    want = {1: (32, 26, 442, 0.16), 2: (58, 35, 381, 0.064), 3: (46, 30, 558, 0.13)}
    nodes = 0
    for seed, (n, k, longest, margin) in want.items():
        name = f"L{seed}"
        cs, closed, keep = _census(name)
        assert (len(cs), sum(keep), max(c.shape[0] for c in cs)) == (n, k, longest), name
        assert 4 <= sum(1 for c, kp in zip(closed, keep) if kp and not c) <= 6
        assert 0.9 * margin < min(abs(S.area(c) - S.MIN_AREA) for c in cs) < 1.1 * margin
        nodes += sum(c.shape[0] for c in cs)
        S.check_input([name])
    assert 1500 < nodes / 3 < 2300          # about 1 900 vertices per map


def test_the_checkerboard_has_only_small_contours_and_two_short_open_ones():
    cs, closed, keep = _census("checker")
    assert len(cs) == 1040 and not any(keep)
    assert 0.55 < max(S.area(c) for c in cs) < 0.65
    assert sorted(c.shape[0] for c, cl in zip(cs, closed) if not cl)[:3][:2] == [2, 2] and sum(1 for c, cl in zip(cs, closed) if not cl and c.shape[0] == 2) == 2
    S.check_input(["checker"])
    S.check_input(["checker"], -1.0)
    assert S.oracle(["checker"]).num_paths == 0 and S.oracle(["checker"], None).num_paths == 1040 and S.oracle(["checker"], -1.0).num_paths == 1038


def test_the_oracle_has_the_documented_layout():
    ts = S.oracle(["flat", "s1", "checker"])
    k = S.kept("s1")
    nodes = sum(c.shape[0] - (1 if S.is_closed(c) else 0) for c in k)
    assert ts.batch_delim.tolist() == [0, 0, len(k), len(k)] and ts.num_nodes == nodes and ts.path_index.shape[0] == nodes + sum(S.is_closed(c) for c in k)
    assert int(ts.path_delim[-1]) == ts.path_index.shape[0] and set(ts.batch.tolist()) == {1}


# ---------------------------------------------------------------------------------------------------------------- the C entries, without a device
def _lib():
    from pixelspointspolygons_amd._lib import lib
    return lib()


P3_EINVAL, P3_ESHAPE = -1, -2


def test_skeleton_from_contours_refuses_bad_arguments_without_a_device():
    L = _lib()
    buf = torch.zeros(64, dtype=torch.int64)
    p = buf.data_ptr()
    args = lambda **kw: [kw.get(k, d) for k, d in (("pos", p), ("N", 4), ("slice", p), ("pbatch", p), ("ep", p), ("P", 1), ("B", 1), ("filter", 1), ("min_area", 10.0),
                                                   ("max_nodes", 4), ("max_slots", 5), ("max_paths", 1), ("out_pos", p), ("degrees", p), ("path_index", p),
                                                   ("path_delim", p), ("batch", p), ("batch_delim", p), ("counts", p), ("status", p), ("ws", p), ("stream", None))]
    for bad in (dict(N=-1), dict(P=-1), dict(B=0), dict(max_nodes=-1), dict(max_slots=-1), dict(max_paths=-1), dict(N=(1 << 31))):
        assert L.p3_skeleton_from_contours(*args(**bad)) == P3_ESHAPE, bad
    for bad in ("pos", "slice", "pbatch", "ep", "out_pos", "degrees", "path_index", "path_delim", "batch", "batch_delim", "counts", "status", "ws"):
        assert L.p3_skeleton_from_contours(*args(**{bad: None})) == P3_EINVAL, bad
    assert L.p3_skeleton_from_contours(*args(min_area=float("nan"))) == P3_EINVAL
    assert b"p3_skeleton_from_contours" in L.p3_last_error_string()
    assert L.p3_skeleton_from_contours_workspace_bytes(0) == 0 and L.p3_skeleton_from_contours_workspace_bytes(100) >= 5 * 400


def test_asm_plan_refuses_bad_arguments_without_a_device():
    L = _lib()
    buf = torch.zeros(64, dtype=torch.int64)
    p = buf.data_ptr()
    args = lambda **kw: [kw.get(k, d) for k, d in (("idx", p), ("M", 6), ("delim", p), ("D", 2), ("N", 5), ("comp_ptr", p), ("cn_node", p), ("cn_occ", p), ("slot_nb", p),
                                                   ("node_local", p), ("slot_k", p), ("counts", p), ("status", p), ("ws", p), ("stream", None))]
    for bad in (dict(N=-1), dict(M=-1), dict(D=-1), dict(N=(1 << 31)), dict(M=(1 << 31))):
        assert L.p3_asm_plan(*args(**bad)) == P3_ESHAPE, bad
    for bad in ("idx", "delim", "comp_ptr", "cn_node", "cn_occ", "slot_nb", "node_local", "slot_k", "counts", "status", "ws"):
        assert L.p3_asm_plan(*args(**{bad: None})) == P3_EINVAL, bad
    assert b"p3_asm_plan" in L.p3_last_error_string()
    assert L.p3_asm_plan_workspace_bytes(0, 0) >= 0 and L.p3_asm_plan_workspace_bytes(10, 20) >= 20 * 8 * 2 + 10 * 8 * 2


def test_the_wrappers_raise_on_host_tensors():
    from pixelspointspolygons_amd import hip, polygonize_asm as A, polygonize_post as Q
    ts = S.oracle(["s1"])
    pos, sl = torch.zeros(4, 2), torch.tensor([[0, 4]])
    for call in (lambda: hip.skeleton_from_contours_device(pos, sl, torch.zeros(1, dtype=torch.int32), torch.zeros(4, dtype=torch.uint8), 1, 10),
                 lambda: hip.skeleton_from_contours(pos, sl, torch.zeros(1, dtype=torch.int32), torch.zeros(4, dtype=torch.uint8), 1),
                 lambda: hip.asm_plan_device(ts.path_index, ts.path_delim, ts.num_nodes), lambda: hip.asm_plan(ts.path_index, ts.path_delim, ts.num_nodes),
                 lambda: A.asm_plan_device(ts), lambda: A.init_skeletons(torch.zeros(1, 8, 8)),
                 lambda: A.polygonize_device(torch.zeros(1, 1, 8, 8), torch.zeros(1, 4, 8, 8), {**A.ASM_DEFAULTS, "init_method": "marching_squares"}),
                 lambda: Q.polygonize_asm_pieces(torch.zeros(1, 1, 8, 8), torch.zeros(1, 4, 8, 8), {**A.ASM_DEFAULTS, "init_method": "marching_squares"})):
        with pytest.raises(hip.P3Error):
            call()


def test_polygonize_device_names_the_host_initialisation_it_does_not_build():
    from pixelspointspolygons_amd import polygonize_asm as A, polygonize_post as Q
    assert A.ASM_DEFAULTS["init_method"] == "skeleton"          # the reference's default stays
    for fn in (A.polygonize_device, Q.polygonize_asm_pieces):
        with pytest.raises(NotImplementedError, match="skimage.*skan"):
            fn(torch.zeros(1, 1, 8, 8), torch.zeros(1, 4, 8, 8), A.ASM_DEFAULTS)


def test_the_header_declares_both_entries():
    from pixelspointspolygons_amd import _lib
    protos = _lib.prototypes()
    assert len(protos["p3_skeleton_from_contours"][1]) == 22 and len(protos["p3_asm_plan"][1]) == 15
    assert "p3_skeleton_from_contours_workspace_bytes" in protos and "p3_asm_plan_workspace_bytes" in protos
