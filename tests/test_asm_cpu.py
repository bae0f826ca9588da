"""The FFL active-skeleton optimiser, the parts that need no GPU: the skeleton containers against the reference's own (tests/golden/asm.npz, written by
tests/golden/make_asm_golden.py from the reference's polygonize_asm.py / tensorskeleton.py), the coefficient and learning-rate schedules against the
reference's interp1d objects and its ExponentialLR, the torch restatement the GPU tests compare with (tests/asm_ref.py) against the reference's positions,
losses and float64 gradients, the plan the kernel works from, what the reference's fp32 run differs from its own float64 run by (the yardstick of the GPU
tolerances), and the C-ABI entries."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import asm_ref as R
from tests.helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "p3hip.h")
KNOTS = [R.KNOTS[k] for k in ("step_thresholds", "data", "length", "crossfield")]


@pytest.fixture(scope="module")
def gold():
    return load_golden("asm.npz")[0]


def skeletons_of(gold):
    from pixelspointspolygons_amd import polygonize_asm as A
    return [A.Skeleton(c, A.Paths(i, p), d) for c, i, p, d in R.skeleton_arrays_of(gold)]


def test_fixture_holds_every_incidence_kind(gold):
    ts = R.tensors_of(gold)
    N, M, P = ts["pos"].shape[0], ts["path_index"].shape[0], ts["path_delim"].shape[0] - 1
    assert (N, M, P) == (348, 362, 16) and int(gold["ts.batch_size"]) == 3
    assert ts["batch_delim"].tolist() == [0, 6, 16, 16]          # image 2 is empty
    deg = ts["degrees"]
    assert sorted(set(deg.tolist())) == [0, 1, 2, 3, 4]
    assert int((deg == 3).sum()) == 4 and int((deg == 4).sum()) == 1 and int((deg == 0).sum()) == 1 and int((deg == 1).sum()) == 2 * 2 + 4
    lens = (ts["path_delim"][1:] - ts["path_delim"][:-1]).tolist()
    assert lens.count(16) == 6 and lens.count(2) == 1 and lens.count(6) == 3 + 2          # theta paths, the junction-to-tip path, the arms and the two 5-gons
    first, last = ts["path_index"][ts["path_delim"][:-1]], ts["path_index"][ts["path_delim"][1:] - 1]
    assert int((first == last).sum()) == 4          # two rings and two 5-gons repeat their first node id
    assert int(np.bincount(ts["path_index"].numpy(), minlength=N).max()) == 4 and int((np.bincount(ts["path_index"].numpy(), minlength=N) == 0).sum()) == 1
    assert float(gold["margin0"]) > 1e-4 and abs(R.decision_margin(ts["pos"], ts) - float(gold["margin0"])) < 1e-12


def test_container_fields_equal_the_reference_and_round_trip(gold):
    from pixelspointspolygons_amd import polygonize_asm as A
    sks = skeletons_of(gold)
    before = [s.paths.indptr.copy() for s in sks]
    ts = A.skeletons_to_tensorskeleton(sks)
    assert all(np.array_equal(s.paths.indptr, b) for s, b in zip(sks, before))          # the inputs are left as they were
    assert ts.pos.dtype == torch.float32
    for k in ("pos", "degrees", "path_index", "path_delim", "batch", "batch_delim"):
        got = getattr(ts, k)
        assert got.dtype == gold["ts." + k].dtype and torch.equal(got, gold["ts." + k]), k
    assert ts.batch_size == 3 and ts.num_nodes == 348 and ts.num_paths == 16 and ts.plan is not None
    back = A.tensorskeleton_to_skeletons(ts)
    assert len(back) == 3
    for b, sk in enumerate(back):
        assert np.array_equal(sk.coordinates, gold[f"rt{b}.coordinates"].numpy()) and sk.coordinates.shape[1] == 2
        assert np.array_equal(sk.paths.indices, gold[f"rt{b}.indices"].numpy()) and np.array_equal(sk.paths.indptr, gold[f"rt{b}.indptr"].numpy())
        if b < 2:
            assert np.array_equal(sk.paths.indices, sks[b].paths.indices) and np.array_equal(sk.paths.indptr, sks[b].paths.indptr)
            lines = A.skeleton_to_polylines(sk)
            assert [len(p) for p in lines] == np.diff(sks[b].paths.indptr).tolist()
            assert np.array_equal(lines[0][0], lines[0][-1]) and not np.array_equal(lines[1][0], lines[1][-1])          # the ring is closed, the line is not
    assert back[2].coordinates.shape == (0, 2) and back[2].paths.indptr.shape[0] <= 1 and A.skeleton_to_polylines(back[2]) == []
    # a default Skeleton() behind the others: path_delim still ends with M (the module's docstring says where the reference differs)
    ts2 = A.skeletons_to_tensorskeleton(sks[:2] + [A.Skeleton()])
    assert torch.equal(ts2.path_delim, ts.path_delim) and torch.equal(ts2.batch_delim, ts.batch_delim)
    empty = A.skeletons_to_tensorskeleton([A.Skeleton(), A.Skeleton()])
    assert empty.num_paths == 0 and empty.num_nodes == 0 and empty.batch_delim.tolist() == [0, 0, 0]


def test_contours_to_skeleton_is_the_marching_squares_conversion(gold):
    from pixelspointspolygons_amd import polygonize_asm as A
    c, i, p, d = R.skeleton_arrays_of(gold)[0]
    contours = []
    for s, e in zip(p[:3], p[1:4]):          # the ring, the line and the 5-gon as contours: a closed one repeats its first point
        contours.append(c[i[s:e]])
    sk = A.contours_to_skeleton(contours)
    n = 80 + 40 + 5
    assert np.array_equal(sk.coordinates, c[:n]) and np.array_equal(sk.degrees, d[:n])
    assert np.array_equal(sk.paths.indices, i[:p[3]]) and np.array_equal(sk.paths.indptr, p[:4])
    assert sk.degrees[sk.paths.indices[p[1]]] == 1 and sk.degrees[sk.paths.indices[p[2] - 1]] == 1 and int((sk.degrees == 1).sum()) == 2
    # the optional filter: at least 3 vertices and a shoelace area above min_area
    square = np.array([[0.0, 0.0], [0.0, 4.0], [4.0, 4.0], [4.0, 0.0], [0.0, 0.0]])
    kept = A.contours_to_skeleton([square, square[:2], square * 0.5], min_area=10)
    assert kept.coordinates.shape == (4, 2) and kept.paths.indices.tolist() == [0, 1, 2, 3, 0] and kept.paths.indptr.tolist() == [0, 5]
    none = A.contours_to_skeleton([square * 0.5], min_area=10)
    assert none.coordinates.shape == (0, 2) and none.paths.indptr.shape[0] == 0
    assert A.contours_to_skeleton([square]).coordinates.shape == (4, 2)


def test_schedules_equal_the_reference_interpolators_and_exponential_lr(gold):
    from pixelspointspolygons_amd import hip, polygonize_asm as A
    want = gold["sched"].numpy()
    assert want.shape == (300, 4) and A.ASM_DEFAULTS["loss_params"]["coefs"]["step_thresholds"][-1] == 300
    for k in ("step_thresholds", "data", "length", "crossfield"):
        assert A.ASM_DEFAULTS["loss_params"]["coefs"][k] == R.KNOTS[k], k
    assert (A.ASM_DEFAULTS["lr"], A.ASM_DEFAULTS["gamma"], A.ASM_DEFAULTS["data_level"]) == (R.DEFAULTS["lr"], R.DEFAULTS["gamma"], R.DEFAULTS["data_level"])
    py = np.array([A.asm_schedule(i) for i in range(300)])
    rs = np.array([R.schedule(i, R.DEFAULTS) for i in range(300)])
    c = np.array([hip.asm_schedule(i, KNOTS, lr=0.1, gamma=0.995) for i in range(300)])
    for name, got in (("asm_schedule", py), ("asm_ref.schedule", rs)):
        rel = np.abs(got[:, :3] - want[:, :3]) / np.maximum(np.abs(want[:, :3]), 1e-300)
        assert rel.max() <= 1e-15, (name, rel.max())
        assert np.array_equal(got[:, 3], want[:, 3]), name          # the chained lr: exactly
    # the C function returns the floats the kernel uses: the double values rounded once
    assert np.array_equal(c, want.astype(np.float32).astype(np.float64))
    assert want[0].tolist()[:3] == [1.0, 0.1, 0.0] and abs(want[100, 2] - 0.05) < 1e-17 and not want[200:, :3].any() and want[199, :3].all()
    assert want[0, 3] == 0.1 and want[299, 3] < want[298, 3]
    assert hip.asm_schedule(300, KNOTS) [:3] == (0.0, 0.0, 0.0)
    with pytest.raises(hip.P3Error):
        hip.asm_schedule(0, [[0, 0], [1, 1], [1, 1], [1, 1]])          # thresholds must increase
    with pytest.raises(hip.P3Error):
        hip.asm_schedule(0, KNOTS[:3])


@pytest.mark.parametrize("steps", [1, 5])
def test_restatement_fp32_reproduces_the_reference(gold, steps):
    ts = R.tensors_of(gold)
    pos, _, last = R.optimize(ts["pos"], torch.zeros_like(ts["pos"]), ts, gold["indicator"], gold["c0c2"], R.DEFAULTS, steps=steps, dtype=torch.float32)
    err = float((pos - gold[f"ref32.pos{steps}"]).abs().max())
    rel = np.abs(np.array(last) / gold[f"ref32.loss{steps}"].numpy() - 1).max()
    print(f"{steps} steps: max |pos - reference| = {err:.3g}, losses rel = {rel:.3g}")
    assert err <= 1e-5 and rel <= 1e-5
    assert float((gold[f"ref32.pos{steps}"] - ts["pos"]).abs().max()) > 1e-3          # the skeleton did move
    tip = ts["degrees"] == 1
    assert torch.equal(gold[f"ref32.pos{steps}"][tip], ts["pos"][tip])                 # and its tips did not


@pytest.mark.parametrize("name,cfg,it", [("it0", R.DEFAULTS, 0), ("it100", R.DEFAULTS, 100), ("align", R.ALIGN_ONLY, 0)])
def test_restatement_float64_gradient_is_the_reference_float64_gradient(gold, name, cfg, it):
    ts = R.tensors_of(gold)
    g, _ = R.gradient(ts["pos"], ts, gold["indicator"], gold["c0c2"], cfg, it)
    want = gold[f"ref64.grad.{name}"]
    err = float((g - want).abs().max())
    print(f"{name}: max |g - reference| = {err:.3g}, largest component {float(want.abs().max()):.3g}")
    assert err <= 1e-12 * max(1.0, float(want.abs().max()))
    lone = int(torch.nonzero(ts["degrees"] == 0)[0])          # the node on no path has a level term and nothing else
    assert float(want.abs().max()) > 0.5 and (float(want[lone].abs().max()) == 0.0) == (name == "align")


def test_plan_components_occurrences_and_the_singleton(gold):
    from pixelspointspolygons_amd import polygonize_asm as A
    ts = R.tensors_of(gold)
    idx, delim, N = ts["path_index"].numpy(), ts["path_delim"].numpy(), ts["pos"].shape[0]
    plan = A.AsmPlan(idx, delim, N)
    comp_ptr, cn_node, cn_occ, slot_nb, node_local, slot_k = (getattr(plan, k).numpy() for k in A.AsmPlan.FIELDS)
    # per image: ring, line, 5-gon, theta graph; image 1: + the degree-4 star + the node on no path
    assert plan.num_comps == 10 and comp_ptr[0] == 0 and comp_ptr[-1] == N and plan.max_comp == int(np.diff(comp_ptr).max()) == 80
    assert sorted(np.diff(comp_ptr).tolist()) == sorted([80, 40, 5, 44, 72, 40, 5, 44, 17, 1])
    assert sorted(cn_node.tolist()) == list(range(N))          # every node in exactly one component
    comp_of = np.empty(N, dtype=np.int64)
    for c in range(plan.num_comps):
        nodes = cn_node[comp_ptr[c]:comp_ptr[c + 1]]
        assert np.all(np.diff(nodes) > 0)
        comp_of[nodes] = c
        assert np.array_equal(node_local[nodes], np.arange(len(nodes)))
    assert np.all(np.diff(cn_node[comp_ptr[:-1]]) > 0)          # components ordered by their smallest node
    # independent labelling: union-find over the edges inside paths
    parent = list(range(N))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    for s, e in zip(delim[:-1], delim[1:]):
        for k in range(s, e - 1):
            parent[find(int(idx[k]))] = find(int(idx[k + 1]))
    roots = np.array([find(v) for v in range(N)])
    for c in range(plan.num_comps):
        nodes = cn_node[comp_ptr[c]:comp_ptr[c + 1]]
        assert len(set(roots[nodes].tolist())) == 1 and int((roots == roots[nodes[0]]).sum()) == len(nodes)
    # occurrence lists: ascending positions in path_index, all of them, with the neighbours' local indices (-1 at a path start / end)
    assert cn_occ[0] == 0 and cn_occ[-1] == len(idx) == plan.num_slots and sorted(slot_k.tolist()) == list(range(len(idx)))
    starts, ends = set(delim[:-1].tolist()), set((delim[1:] - 1).tolist())
    for i, v in enumerate(cn_node):
        ks = slot_k[cn_occ[i]:cn_occ[i + 1]]
        assert np.all(np.diff(ks) > 0) and np.all(idx[ks] == v) and len(ks) == int((idx == v).sum())
        for s, k in zip(range(cn_occ[i], cn_occ[i + 1]), ks):
            assert slot_nb[s, 0] == (-1 if k in starts else node_local[idx[k - 1]]) and slot_nb[s, 1] == (-1 if k in ends else node_local[idx[k + 1]])
            assert k in starts or comp_of[idx[k - 1]] == comp_of[v]
    lone = int(torch.nonzero(ts["degrees"] == 0)[0])
    c = comp_of[lone]
    assert comp_ptr[c + 1] - comp_ptr[c] == 1 and cn_occ[comp_ptr[c] + 1] == cn_occ[comp_ptr[c]]          # a component of its own, without an occurrence
    x = int(torch.nonzero(ts["degrees"] == 4)[0])
    assert cn_occ[np.flatnonzero(cn_node == x)[0] + 1] - cn_occ[np.flatnonzero(cn_node == x)[0]] == 4
    # no path at all, and node ids outside pos
    e = A.AsmPlan(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), 3)
    assert e.num_comps == 3 and e.max_comp == 1 and e.slot_nb.shape == (0, 2) and e.cn_occ.tolist() == [0, 0, 0, 0]
    assert A.AsmPlan(np.zeros(0, dtype=np.int64), np.zeros(1, dtype=np.int64), 0).num_comps == 0
    from pixelspointspolygons_amd import hip
    with pytest.raises(hip.P3Error):
        A.AsmPlan(np.array([0, 5]), np.array([0, 2]), 3)


def test_reference_alone_stays_within_the_generators_conditions(gold):
    """tests/test_asm_gpu.py allows the kernel 1e-3 of node comparisons over 1e-4 px, 3e-4 over 1e-2 px and a median of max(4 x this median, 4e-6): the
    reference's fp32 run against its own float64 run, re-synchronised every 5 steps in the same way, must sit well inside that"""
    share4, share2, median, worst, moved = gold["alone.traj"].tolist()
    print(f"reference alone: share over 1e-4 = {share4:.3g}, over 1e-2 = {share2:.3g}, median = {median:.3g}, worst = {worst:.3g}, moved {moved:.3g} px")
    assert share4 <= 5e-4 and share2 == 0 and median <= 2e-6 and moved > 0.1
    for name in ("it0", "it100", "align"):
        a, g = float(gold[f"alone.grad.{name}"][0]), float(gold[f"ref64.grad.{name}"].abs().max())
        print(f"gradient {name}: reference alone {a:.3g} on a largest component of {g:.3g}")
        assert 0 < a < 1e-6 * max(g, 1.0)
    assert 0 < float(gold["alone.pos5"][0]) < 1e-4
    assert torch.equal(gold["ref32.pos300"][gold["ts.degrees"] == 1], gold["ts.pos"][gold["ts.degrees"] == 1])


def test_entries_are_declared_exported_and_validate_before_any_device_work():
    from pixelspointspolygons_amd._lib import load
    from pixelspointspolygons_amd.build import build_library
    lib = load(build_library(verbose=False))
    raw = open(HEADER).read()
    assert "polygonize_asm.py:133-421" in raw and "tensorskeleton.py" in raw
    text = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    m = re.search(r"\bint\s+p3_asm_optimize\s*\(([^;{}]*?)\)\s*;", text, flags=re.S)
    assert m and len(m.group(1).split(",")) == 30
    assert hasattr(lib, "p3_asm_optimize") and hasattr(lib, "p3_asm_workspace_bytes") and hasattr(lib, "p3_asm_schedule")
    f, dbl, n64 = ctypes.c_float, ctypes.c_double, ctypes.c_int64
    knots = (ctypes.c_double * 16)(*[float(v) for r in KNOTS for v in r])

    def call(N, C, steps, B=1, first_iter=0, CN=None, nk=4, kn=knots):
        return lib.p3_asm_optimize(None, None, n64(N), None, C, None, None, n64(N if CN is None else CN), None, n64(0), None, None, None, None, B, 8, 8, f(0.5),
                                   kn, nk, dbl(0.1), dbl(0.995), first_iter, steps, 0, 0, None, None, None, None)

    assert call(4, 1, 5) == -1 and b"p3_asm_optimize" in lib.p3_last_error_string()
    assert call(4, 0, 5) == 0 and call(4, 1, 0) == 0 and call(0, 1, 5) == 0 and call(4, 1, 5, CN=0) == 0          # nothing to do: no launch, no pointer is looked at
    assert call(4, -1, 5) == -2 and call(4, 1, -1) == -2 and call(4, 1, 5, first_iter=-1) == -2 and call(-1, 1, 5) == -2
    assert lib.p3_asm_workspace_bytes(n64(100), n64(90)) == 100 * 8 + 90 * 12 and lib.p3_asm_workspace_bytes(n64(0), n64(0)) == 0
    out = (ctypes.c_double * 4)()
    assert lib.p3_asm_schedule(50, knots, 4, dbl(0.1), dbl(0.995), out) == 0
    assert list(out)[:3] == [float(np.float32(0.55)), float(np.float32(0.055)), float(np.float32(0.025))]
    assert lib.p3_asm_schedule(50, None, 4, dbl(0.1), dbl(0.995), out) == -2 and lib.p3_asm_schedule(50, knots, 9, dbl(0.1), dbl(0.995), out) == -2
    assert lib.p3_asm_schedule(50, knots, 4, dbl(0.1), dbl(0.995), None) == -1 and lib.p3_asm_schedule(-1, knots, 4, dbl(0.1), dbl(0.995), out) == -1


def test_wrappers_refuse_host_tensors(gold):
    from pixelspointspolygons_amd import hip, polygonize_asm as A
    ts = A.skeletons_to_tensorskeleton(skeletons_of(gold))
    with pytest.raises(hip.P3Error):
        hip.asm_optimize(ts.pos, torch.zeros_like(ts.pos), ts.plan, ts.degrees == 1, ts.batch, gold["indicator"], gold["c0c2"], KNOTS)
    with pytest.raises(hip.P3Error):
        A.TensorSkeletonOptimizer(A.ASM_DEFAULTS, ts, gold["indicator"], gold["c0c2"])
    with pytest.raises(hip.P3Error):
        A.optimize_skeletons(torch.zeros(3, 1, 32, 40), gold["c0c2"], skeletons_of(gold))
