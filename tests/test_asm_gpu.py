"""p3_asm_optimize (csrc/asm.hip) through hip.asm_optimize and the public pixelspointspolygons_amd.polygonize_asm interface.
References: tests/golden/asm.npz (the reference's own classes on the CPU) and tests/asm_ref.py (their torch-autograd restatement, pinned to the fixture by
tests/test_asm_cpu.py) in float64.  The tolerances of the gradient and trajectory tests are multiples of what the REFERENCE's fp32 run differs from its own
float64 run by, measured by the fixture's generator and stored in it (`alone.grad.*`, `alone.traj`, `alone.pos5`)."""
import types

import numpy as np
import pytest
import torch

from tests import asm_ref as R
from tests.helpers import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"


def knots_of(cfg):
    return [cfg["coefs"][k] for k in ("step_thresholds", "data", "length", "crossfield")]


class Scene:
    """a container (dict of host tensors as tests/asm_ref.py takes it) with its maps, and the same on the device with the plan"""

    def __init__(self, ts, indicator, c0c2):
        from pixelspointspolygons_amd import polygonize_asm as A
        self.ts, self.ind, self.cf = ts, indicator, c0c2
        self.N = ts["pos"].shape[0]
        self.plan = A.AsmPlan(ts["path_index"].numpy(), ts["path_delim"].numpy(), self.N).to(DEV)
        self.pos = ts["pos"].float().to(DEV)
        self.tip, self.batch, self.d_ind, self.d_cf = (ts["degrees"] == 1).to(DEV), ts["batch"].to(DEV), indicator.to(DEV), c0c2.to(DEV)

    def run(self, cfg=R.DEFAULTS, first_iter=0, steps=1, pos=None, sq=None, losses=False, **kw):
        """-> (pos, sq, grad[, losses]) as new device tensors; the inputs are cloned"""
        from pixelspointspolygons_amd import hip
        p = (self.pos if pos is None else pos).clone()
        s = torch.zeros_like(p) if sq is None else sq.clone()
        g = torch.full_like(p, float("nan"))
        out = hip.asm_optimize(p, s, self.plan, self.tip, self.batch, self.d_ind, self.d_cf, knots_of(cfg), data_level=cfg["data_level"], lr=cfg["lr"],
                               gamma=cfg["gamma"], first_iter=first_iter, steps=steps, grad_out=g, losses=losses, **kw)
        return (p, s, g, out[1]) if losses else (p, s, g)

    def ref64(self, pos, sq, cfg, first_iter, steps):
        return R.optimize(pos.cpu(), sq.cpu(), self.ts, self.ind, self.cf, cfg, first_iter=first_iter, steps=steps)


@pytest.fixture(scope="module")
def gold():
    return load_golden("asm.npz")[0]


@pytest.fixture(scope="module")
def scene(gold):
    return Scene(R.tensors_of(gold), gold["indicator"], gold["c0c2"])


def skeletons_of(gold):
    from pixelspointspolygons_amd import polygonize_asm as A
    return [A.Skeleton(c, A.Paths(i, p), d) for c, i, p, d in R.skeleton_arrays_of(gold)]


# ------------------------------------------------------------------------------------------------ gradient
@pytest.mark.parametrize("name,cfg,it", [("it0", R.DEFAULTS, 0), ("it100", R.DEFAULTS, 100), ("align", R.ALIGN_ONLY, 0)])
def test_grad_out_of_one_step_is_the_float64_gradient(gold, scene, name, cfg, it):
    """Bound: 4 x the reference's own fp32-vs-float64 gradient deviation at the same setting on this fixture (the kernel sums in another order); the generator
    checked that no node or midpoint is within 1e-4 of a floor / round / 0.1 decision, so every node counts.  The shipped table has crossfield = 0 at
    iteration 0: the align-only table is what checks that term."""
    _, _, g = scene.run(cfg, first_iter=it, steps=1)
    want, _ = R.gradient(scene.ts["pos"], scene.ts, scene.ind, scene.cf, cfg, it)
    assert float((want - gold[f"ref64.grad.{name}"]).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    err, alone = float((g.cpu().double() - want).abs().max()), float(gold[f"alone.grad.{name}"][0])
    print(f"gradient {name}: max |kernel - float64| = {err:.3g}, reference alone {alone:.3g}, largest component {float(want.abs().max()):.3g}")
    assert float(gold["margin0"]) > 1e-4
    assert err <= 4 * alone


# ------------------------------------------------------------------------------------------------ update rule
@pytest.mark.parametrize("it", [0, 100])
def test_update_is_rmsprop_on_the_kernels_own_gradient(scene, it):
    """sq within 1e-6 relative of 0.9 sq + 0.1 g^2 and pos within 2^-16 + 1e-6 |update| of pos - lr g / (sqrt(sq) + 1e-8) in float64 from the kernel's own
    grad_out: one rounding of a coordinate below 256, plus about six fp32 roundings of the update.  Tips keep their bits, and their sq is updated too."""
    gen = torch.Generator().manual_seed(3)
    sq0 = (0.01 + torch.rand(scene.N, 2, generator=gen)).to(DEV)
    p, s, g = scene.run(first_iter=it, steps=1, sq=sq0)
    g64, p0, tip = g.cpu().double(), scene.pos.cpu().double(), scene.tip.cpu()
    lr = R.schedule(it, R.DEFAULTS)[3]
    sq_want = 0.9 * sq0.cpu().double() + 0.1 * g64 * g64
    upd = lr * g64 / (sq_want.sqrt() + 1e-8)
    pos_want = torch.where(tip[:, None], p0, p0 - upd)
    rel = float(((s.cpu().double() - sq_want).abs() / sq_want).max())
    over = float(((p.cpu().double() - pos_want).abs() - (2.0 ** -16 + 1e-6 * upd.abs())).max())
    print(f"iteration {it}: sq rel = {rel:.3g}, largest |pos - formula| = {float((p.cpu().double() - pos_want).abs().max()):.3g}, largest update {float(upd.abs().max()):.3g}")
    assert torch.isfinite(g).all() and rel <= 1e-6 and over <= 0
    assert torch.equal(p[scene.tip], scene.pos[scene.tip]) and int(tip.sum()) == 8
    assert float(upd.abs().max()) > 1e-3 and not torch.equal(p[~scene.tip], scene.pos[~scene.tip])


# ------------------------------------------------------------------------------------------------ whole trajectory, re-synchronised
def test_42_calls_of_5_steps_follow_float64_from_the_kernels_own_positions_and_state(gold, scene):
    pos, sq, devs, seen = scene.pos.clone(), torch.zeros_like(scene.pos), [], []
    for k in range(42):
        nxt, nsq, _ = scene.run(first_iter=5 * k, steps=5, pos=pos, sq=sq)
        want, _, _ = scene.ref64(pos, sq, R.DEFAULTS, 5 * k, 5)
        devs.append((nxt.cpu().double() - want).abs())
        pos, sq = nxt, nsq
        seen.append(nxt)
    devs = torch.stack(devs)
    share4, share2, median, worst = float((devs > 1e-4).double().mean()), float((devs > 1e-2).double().mean()), float(devs.median()), float(devs.max())
    a4, a2, a_median, a_worst, a_moved = gold["alone.traj"].tolist()
    moved = float((pos - scene.pos).abs().max())
    print(f"kernel: share over 1e-4 = {share4:.3g}, over 1e-2 = {share2:.3g}, median = {median:.3g}, worst = {worst:.3g}, moved {moved:.3g} px; "
          f"reference alone: {a4:.3g}, {a2:.3g}, {a_median:.3g}, {a_worst:.3g}, {a_moved:.3g}")
    assert devs.shape == (42, scene.N, 2) and torch.isfinite(devs).all()
    assert share4 <= 1e-3
    assert share2 <= 3e-4
    assert median <= max(4 * a_median, 4e-6)
    assert moved > 0.1
    assert torch.equal(seen[41], seen[39]) and torch.equal(seen[40], seen[39])          # iterations 200 .. 209: every coefficient is 0


# ------------------------------------------------------------------------------------------------ exactness, bit for bit
def test_runs_repeat_split_the_fallback_and_an_image_alone_give_the_same_bits(gold, scene):
    from pixelspointspolygons_amd import polygonize_asm as A
    full = scene.run(steps=300)
    again = scene.run(steps=300)
    assert all(torch.equal(a, b) for a, b in zip(full, again))
    assert all(torch.isfinite(t).all() for t in full)
    p120, s120, _ = scene.run(steps=120)
    split = scene.run(first_iter=120, steps=180, pos=p120, sq=s120)
    assert all(torch.equal(a, b) for a, b in zip(full, split))
    for steps in (300, 7):          # an odd number of steps: the fallback's result comes home from its workspace
        fast, slow = scene.run(steps=steps, losses=True), scene.run(steps=steps, losses=True, force_fallback=True)
        assert all(torch.equal(a, b) for a, b in zip(fast, slow)), steps
        assert torch.equal(fast[0][scene.tip], scene.pos[scene.tip]) and not torch.equal(fast[0][~scene.tip], scene.pos[~scene.tip])
    # image 1 alone: its nodes as they are inside the batch
    ts1 = A.skeletons_to_tensorskeleton(skeletons_of(gold)[1:2])
    sc1 = Scene({k: getattr(ts1, k) for k in ("pos", "degrees", "path_index", "path_delim", "batch", "batch_delim")}, gold["indicator"][1:2], gold["c0c2"][1:2])
    sel = scene.batch == 1
    assert int(sel.sum()) == sc1.N == 179 and torch.equal(sc1.pos, scene.pos[sel])
    alone = sc1.run(steps=300)
    assert all(torch.equal(a, b[sel]) for a, b in zip(alone, full))


# ------------------------------------------------------------------------------------------------ edge shapes
def _fields(Hb, Wb, seed):
    """a blob's indicator and a noisy radial frame field of any size: (indicator [1,Hb,Wb], c0c2 [1,4,Hb,Wb]) fp32"""
    g = torch.Generator().manual_seed(seed)
    rr, cc = torch.meshgrid(torch.arange(Hb, dtype=torch.float64), torch.arange(Wb, dtype=torch.float64), indexing="ij")
    noise = lambda s: s * torch.randn(Hb, Wb, generator=g, dtype=torch.float64)
    ind = torch.sigmoid((0.35 * Hb - torch.hypot(rr - Hb / 2, (cc - Wb / 2) * Hb / Wb)) / 2) + noise(0.02)
    th = torch.atan2(rr - Hb / 2, cc - Wb / 2) + noise(0.05)
    cf = torch.stack([-torch.cos(4 * th), -torch.sin(4 * th), noise(0.05), noise(0.05)])
    return ind[None].float(), cf[None].float()


def _ring(n, centre, radius, seed, jitter=0.2):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) * (2 * np.pi / n)
    p = torch.stack([centre[0] + radius * torch.sin(t), centre[1] + radius * torch.cos(t)], 1)
    return (p + jitter * torch.randn(n, 2, generator=g, dtype=torch.float64)).numpy()


def _edge_case(name, gold):
    """-> ([(coordinates, paths as lists of node ids, degrees)], indicator, c0c2, config): one skeleton per image"""
    ind, cf = gold["indicator"][:1], gold["c0c2"][:1]
    H, W = ind.shape[1:]
    closed = lambda n: list(range(n)) + [0]
    if name == "two_tips":                    # a single 2-entry path between two tips
        return [(np.array([[10.3, 8.4], [12.1, 9.7]]), [[0, 1]], [1, 1])], ind, cf, R.DEFAULTS
    if name == "three_entries":
        return [(np.array([[10.3, 8.4], [11.4, 9.2], [12.1, 10.7]]), [[0, 1, 2]], [1, 2, 1])], ind, cf, R.DEFAULTS
    if name == "closed_triangle":
        return [(np.array([[10.3, 8.4], [14.4, 9.2], [12.1, 13.7]]), [closed(3)], [2, 2, 2])], ind, cf, R.DEFAULTS
    if name == "coincident_nodes":            # |t| = 0: masked, gradient exactly 0 through the norm, never NaN
        c = np.array([[10.3, 8.4], [11.4, 9.2], [12.6, 10.1], [12.6, 10.1], [13.8, 11.2], [14.9, 12.4]])
        return [(c, [[0, 1, 2, 3, 4, 5]], [1, 2, 2, 2, 2, 1])], ind, cf, R.DEFAULTS
    if name == "outside_the_map":             # 10 px beyond a border, H != W: every clamp of the gathers
        c = np.array([[5.3, 6.4], [-10.2, 7.9], [4.6, W + 9.3], [H + 9.8, 20.1], [16.2, -10.4], [H + 9.6, W + 9.7]])
        return [(c, [closed(6)], [2] * 6)], ind, cf, R.DEFAULTS
    if name == "all_zero_table":
        return [(_ring(30, (16, 20), 8, 15), [closed(30)], [2] * 30)], ind, cf, R.ALL_ZERO
    if name == "nodes_without_paths":         # P = 0: the level term alone
        return [(np.array([[10.3, 8.4], [14.4, 9.2]]), [], [0, 0])], ind, cf, R.DEFAULTS
    if name == "n_256_257":                   # a thread's second pass begins at the 257th node of a component; 256 as an open polyline
        i2, c2 = _fields(120, 136, 9)
        a, b = _ring(257, (60, 68), 45, 8), _ring(256, (61, 67), 42, 9)
        return [(np.concatenate([a, b]), [closed(257), list(range(257, 513))], [2] * 257 + [1] + [2] * 254 + [1])], i2, c2, R.DEFAULTS
    if name == "over_the_cap":                # 4200 > 4096 nodes: seven turns of a wavy circle in ~1 px steps; the small ring beside it takes the fast path in the same call
        i2, c2 = _fields(256, 264, 10)
        t = torch.arange(4200, dtype=torch.float64) * (14 * np.pi / 4200)
        rad = 1 + 0.25 * torch.sin(t / 7)
        big = torch.stack([128 + 95 * rad * torch.sin(t), 132 + 100 * rad * torch.cos(t)], 1).numpy()
        return [(np.concatenate([_ring(40, (120, 130), 8, 11), big]), [closed(40), [40 + v for v in closed(4200)]], [2] * 4240)], i2, c2, R.DEFAULTS
    raise KeyError(name)


@pytest.mark.parametrize("name", ["two_tips", "three_entries", "closed_triangle", "coincident_nodes", "outside_the_map", "all_zero_table",
                                  "nodes_without_paths", "n_256_257", "over_the_cap"])
def test_edge_shapes_are_finite_and_follow_float64(gold, name):
    """Five iterations from iteration 50, where all three coefficients are non-zero, on both paths: the same bits, all finite, tips where they were.  The
    gradient of the first of them against the restatement in float64; bound: 4 x what the restatement's own fp32 gradient differs from its float64 one by on
    this case, and no less than 4 ulp of the largest component (a case of three nodes can agree by accident)."""
    from pixelspointspolygons_amd import hip, polygonize_asm as A
    sks, ind, cf, cfg = _edge_case(name, gold)
    skeletons = []
    for c, paths, deg in sks:
        indptr = np.cumsum([0] + [len(p) for p in paths]).astype(np.int64)
        skeletons.append(A.Skeleton(c, A.Paths(np.array([v for p in paths for v in p], dtype=np.int64), indptr), np.array(deg, dtype=np.int64)))
    ts = A.skeletons_to_tensorskeleton(skeletons)
    sc = Scene({k: getattr(ts, k) for k in ("pos", "degrees", "path_index", "path_delim", "batch", "batch_delim")}, ind, cf)
    if name == "over_the_cap":
        assert sc.plan.max_comp == 4200 > hip.ASM_LDS_CAP and sc.plan.num_comps == 2
    fast, slow = sc.run(cfg, first_iter=50, steps=5, losses=True), sc.run(cfg, first_iter=50, steps=5, losses=True, force_fallback=True)
    assert all(torch.equal(a, b) for a, b in zip(fast, slow))
    assert all(torch.isfinite(t).all() for t in fast)
    assert torch.equal(fast[0][sc.tip], sc.pos[sc.tip])
    _, _, g = sc.run(cfg, first_iter=50, steps=1)
    assert R.decision_margin(sc.pos.cpu(), sc.ts) > 1e-5          # of the case itself: no midpoint of it sits on a rounding tie, where fp32 and float64 may part
    g64, _ = R.gradient(sc.pos.cpu(), sc.ts, ind, cf, cfg, 50)
    g32, _ = R.gradient(sc.pos.cpu(), sc.ts, ind, cf, cfg, 50, dtype=torch.float32)
    err, own = float((g.cpu().double() - g64).abs().max()), float((g32.double() - g64).abs().max())
    bound = max(4 * own, 4 * float(np.spacing(np.float32(g64.abs().max()))))
    print(f"{name}: N = {sc.N}, components {sc.plan.num_comps}, max |grad - float64| = {err:.3g} (bound {bound:.3g}), moved {float((fast[0] - sc.pos).abs().max()):.3g}")
    assert err <= bound
    if name in ("two_tips", "all_zero_table"):
        assert torch.equal(fast[0], sc.pos)                      # nothing moves, bit for bit
    else:
        assert not torch.equal(fast[0], sc.pos)
    if name == "all_zero_table":
        assert not fast[1].any() and not fast[2].any() and fast[3][0, 0] > 0          # no gradient and no state; the loss terms are still reported


def test_nothing_to_optimise_is_no_launch_and_no_error(scene):
    from pixelspointspolygons_amd import hip, polygonize_asm as A
    e = lambda *s, dtype=torch.float32: torch.empty(s, dtype=dtype, device=DEV)
    plan = A.AsmPlan(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), 0).to(DEV)
    pos, losses = hip.asm_optimize(e(0, 2), e(0, 2), plan, e(0, dtype=torch.bool), e(0, dtype=torch.long), scene.d_ind, scene.d_cf, knots_of(R.DEFAULTS), losses=True)
    assert pos.shape == (0, 2) and losses.shape == (0, 3)
    seg = scene.d_ind[:, None]
    assert A.optimize_skeletons(seg, scene.d_cf, [A.Skeleton(), A.Skeleton(), A.Skeleton()]) == [[], [], []]
    p, s, _ = scene.run(steps=0)
    assert torch.equal(p, scene.pos) and not s.any()


# ------------------------------------------------------------------------------------------------ losses and interface
def test_step_returns_the_losses_of_the_reference_before_the_update(gold, scene):
    from pixelspointspolygons_amd import polygonize_asm as A
    ts = types.SimpleNamespace(pos=scene.pos.clone(), degrees=scene.ts["degrees"].to(DEV), path_index=scene.ts["path_index"].to(DEV),
                               path_delim=scene.ts["path_delim"].to(DEV), batch=scene.batch, batch_delim=scene.ts["batch_delim"].to(DEV), batch_size=3)
    opt = A.TensorSkeletonOptimizer(A.ASM_DEFAULTS, ts, scene.d_ind, scene.d_cf)          # any object with the fields: the plan is built from it
    loss, parts = opt.step(0)
    want = gold["ref32.loss1"].tolist()                     # the reference's own (loss, align, level, length) of its first step
    got = [loss, parts["align"], parts["level"], parts["length"]]
    print("step(0):", got, "reference fp32:", want)
    assert set(parts) == {"align", "level", "length"}
    for g, w in zip(got, want):
        assert abs(g / w - 1) <= 1e-5
    p1, s1, g1, per = scene.run(steps=1, losses=True)
    assert torch.equal(ts.pos, p1) and torch.equal(opt.sq, s1) and torch.equal(opt.grad, g1)         # and it did the step
    assert per.shape == (10, 3) and float(per[:, 0].min()) >= 0 and float(per[9, 0]) == 0 and float(per[9, 2]) == 0 and float(per[9, 1]) > 0          # the lone node
    p5, _, _, per5 = scene.run(steps=5, losses=True)          # of the LAST executed step
    p4, s4, _ = scene.run(steps=4)
    _, _, _, per41 = scene.run(first_iter=4, steps=1, pos=p4, sq=s4, losses=True)
    assert torch.equal(per5, per41) and not torch.equal(per5, per)


def test_optimize_skeletons_and_five_steps_through_the_public_interface(gold, scene):
    from pixelspointspolygons_amd import polygonize_asm as A
    sks = skeletons_of(gold)
    seg = torch.stack([scene.d_ind, 1 - scene.d_ind], 1)          # [B, 2, H, W]; channel 0 is the indicator
    out = A.optimize_skeletons(seg, scene.d_cf, sks)
    full = scene.run(steps=300)[0].cpu().numpy()
    assert len(out) == 3 and out[2] == []
    at = 0
    for b in range(2):
        c, idx, indptr, deg = R.skeleton_arrays_of(gold)[b]
        assert len(out[b]) == len(indptr) - 1
        for line, s, e in zip(out[b], indptr[:-1], indptr[1:]):
            assert line.shape == (e - s, 2) and line.dtype == np.float32 and np.array_equal(line, full[at + idx[s:e]])
            if idx[s] == idx[e - 1]:
                assert np.array_equal(line[0], line[-1])          # a closed path keeps its repeated end point
            for v, pt in ((idx[s], line[0]), (idx[e - 1], line[-1])):
                if deg[v] == 1:
                    assert np.array_equal(pt, c[v].astype(np.float32))          # a tip stays where it was
        at += len(c)
    # five steps through the optimiser class and tensorskeleton_to_skeletons against the reference's stored positions; bound: 4 x what the reference's fp32
    # positions differ from its own float64 ones by after these 5 steps
    ts = A.skeletons_to_tensorskeleton(sks, device=DEV)
    opt = A.TensorSkeletonOptimizer(A.ASM_DEFAULTS, ts, scene.d_ind, scene.d_cf)
    for i in range(5):
        opt.step(i)
    back = A.tensorskeleton_to_skeletons(opt.tensorskeleton)
    got = np.concatenate([sk.coordinates for sk in back])
    err, alone = float(np.abs(got.astype(np.float64) - gold["ref32.pos5"].numpy().astype(np.float64)).max()), float(gold["alone.pos5"][0])
    print(f"5 steps: max |pos - reference fp32| = {err:.3g}, reference alone {alone:.3g}")
    assert got.shape == (348, 2) and err <= 4 * alone
    assert torch.equal(ts.pos, scene.run(steps=5)[0])
