"""Golden vectors for the FFL active-skeleton optimiser: the reference's own `TensorSkeletonOptimizer` and `AlignLoss` (predict/ffl/polygonize_asm.py:133-421)
with its `tensorskeleton.py` and `bilinear_interpolate`, run on the CPU in fp32 and float64.  Build-container only (imports the reference); emits
tests/golden/asm.npz (arrays only).  skan / skimage / shapely / matplotlib / omegaconf / lydorn_utils are stubs: nothing of them runs in these classes.
torch_scatter is not installed either and AlignLoss calls it: gather_csr, segment_sum_csr and segment_max_csr are a few lines of torch below; they feed
only the curvature term, which is outside total_loss (:353).

The scene extends the ACM generator's (make_acm_golden.scene): B = 3, 32 x 40.  Images 0 and 1 hold the closed ring, the open border-to-border line (two
tips), the 5-gon and a "shared wall" theta graph (two degree-3 junctions joined by three 16-entry paths); image 1 also a degree-4 junction with a
2-entry path to a tip, and one node on no path; image 2 is empty.

Besides the inputs and the reference's outputs the file holds what the reference's fp32 run differs from ITS OWN float64 run by (`alone.*`): the tolerances
of tests/test_asm_gpu.py are multiples of those numbers, not of anything the kernel produced."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_acm_golden as G  # noqa: E402
import asm_ref as R  # noqa: E402

REF, LYDORN = G.REF, G.LYDORN
B, H, W = 3, 32, 40
CALLS, CHUNK = 42, 5          # the re-synchronised trajectory: iterations 0 .. 209, the last two calls past the end of the schedule's non-zero part


def _scatter_stub():
    m = G._stub("torch_scatter")
    counts = lambda indptr: (indptr[1:] - indptr[:-1])
    m.gather_csr = lambda src, indptr: torch.repeat_interleave(src, counts(indptr), dim=0)

    def segment_sum_csr(src, indptr):
        return torch.stack([src[s:e].sum(0) for s, e in zip(indptr[:-1].tolist(), indptr[1:].tolist())])

    def segment_max_csr(src, indptr):
        out = [src[s:e].max(0) if e > s else (src.new_zeros(()), torch.tensor(0)) for s, e in zip(indptr[:-1].tolist(), indptr[1:].tolist())]
        return torch.stack([o[0] for o in out]), torch.stack([torch.as_tensor(o[1]) for o in out])

    m.segment_sum_csr, m.segment_max_csr = segment_sum_csr, segment_max_csr


def load_reference():
    if not hasattr(np, "float_"):
        np.float_ = np.float64          # tensorskeleton.py predates numpy 2
    for name in ("skimage", "shapely", "lydorn_utils", "matplotlib", "torch_lydorn", "torch_lydorn.torch", "torch_lydorn.torch.nn",
                 "torch_lydorn.torch.utils", "torch_lydorn.torchvision", "pixelspointspolygons", "pixelspointspolygons.predict",
                 "pixelspointspolygons.predict.ffl", "pixelspointspolygons.models", "pixelspointspolygons.models.ffl"):
        G._stub(name, pkg=True)
    for name in ("skimage.measure", "skimage.morphology", "skimage.io", "shapely.geometry", "shapely.ops", "shapely.prepared", "omegaconf", "skan",
                 "matplotlib.pyplot", "lydorn_utils.math_utils", "lydorn_utils.python_utils", "lydorn_utils.print_utils", "torch_lydorn.kornia",
                 "pixelspointspolygons.predict.ffl.polygonize_utils"):
        G._stub(name)
    if "tqdm" not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:
            G._stub("tqdm").tqdm = lambda it, **k: it
    _scatter_stub()
    G._load("torch_lydorn.torch.utils.complex", LYDORN + "/torch/utils/complex.py")
    G._load("torch_lydorn.torch.nn.functionnal", LYDORN + "/torch/nn/functionnal.py")
    tr = G._stub("torch_lydorn.torchvision.transforms", pkg=True)
    tsk = G._load("torch_lydorn.torchvision.transforms.tensorskeleton", LYDORN + "/torchvision/transforms/tensorskeleton.py")
    for k in ("Paths", "Skeleton", "TensorSkeleton", "skeletons_to_tensorskeleton", "tensorskeleton_to_skeletons"):
        setattr(tr, k, getattr(tsk, k))
    G._load("pixelspointspolygons.models.ffl.frame_field_utils", REF + "/pixelspointspolygons/models/ffl/frame_field_utils.py")
    return G._load("pixelspointspolygons.predict.ffl.polygonize_asm", REF + "/pixelspointspolygons/predict/ffl/polygonize_asm.py"), tsk


class SkeletonBuilder:
    def __init__(self):
        self.coords, self.degrees, self.indices, self.indptr = [], [], [], [0]

    def node(self, p, degree):
        self.coords.append(np.asarray(p, dtype=np.float64)); self.degrees.append(degree)
        return len(self.coords) - 1

    def path(self, ids):
        self.indices += list(ids); self.indptr.append(len(self.indices))

    def contour(self, c):
        """a marching-squares contour as get_marching_squares_skeleton converts it (:610-628)"""
        closed = np.max(np.abs(c[0] - c[-1])) < 1e-6
        pts = c[:-1] if closed else c
        ids = [self.node(p, 2) for p in pts]
        if closed:
            ids.append(ids[0])
        else:
            self.degrees[ids[0]] = self.degrees[ids[-1]] = 1
        self.path(ids)

    def chain(self, first, last, between):
        """path first -> last through new degree-2 nodes at `between`"""
        self.path([first] + [self.node(p, 2) for p in between] + [last])

    def arrays(self):
        return (np.array(self.coords, dtype=np.float64).reshape(-1, 2), np.array(self.indices, dtype=np.int64), np.array(self.indptr, dtype=np.int64),
                np.array(self.degrees, dtype=np.int64))


def scene(seed):
    """-> indicator [3,H,W], c0c2 [3,4,H,W] (fp32) and one (coordinates, indices, indptr, degrees) per image"""
    ind2, cf2, contours = G.scene(seed)
    rng = np.random.default_rng(seed + 1000)
    ind = torch.cat([ind2, torch.tensor(0.5 + rng.normal(0, 0.02, (1, H, W)), dtype=torch.float32)])
    cf = torch.cat([cf2, torch.tensor(rng.normal(0, 0.3, (1, 4, H, W)), dtype=torch.float32)])
    jit = lambda n: rng.normal(0, 0.2, (n, 2))
    skeletons = []
    for b, (cr, cx) in enumerate(((16.0, 20.0), (15.0, 21.0))):
        sb = SkeletonBuilder()
        for c in contours[b]:
            sb.contour(c)
        # theta graph: two degree-3 junctions 18 px apart joined by three 16-entry paths (straight, bowed up, bowed down); the middle one runs backwards
        j1, j2 = sb.node(np.array([cr + 0.3, cx - 9.2]) + jit(1)[0], 3), sb.node(np.array([cr - 0.4, cx + 9.1]) + jit(1)[0], 3)
        p1, p2 = sb.coords[j1], sb.coords[j2]
        t = (np.arange(1, 15) / 15.0)[:, None]
        for bow, backwards in ((0.0, False), (5.0, True), (-5.0, False)):
            mid = p1 * (1 - t) + p2 * t + np.concatenate([bow * np.sin(np.pi * t), 0 * t], 1) + jit(14)
            if backwards:
                sb.chain(j2, j1, mid[::-1])
            else:
                sb.chain(j1, j2, mid)
        if b == 1:
            # degree-4 junction: three 6-entry arms to tips (one of them stored tip -> junction) and a 2-entry path junction -> tip
            x = sb.node(np.array([24.3, 8.6]), 4)
            for d, towards in (((-1.1, 0.2), False), ((0.3, 1.2), True), ((1.0, -0.4), False)):
                pts = sb.coords[x] + np.arange(1, 6)[:, None] * np.array(d) + jit(5)
                tip = sb.node(pts[-1], 1)
                if towards:
                    sb.chain(tip, x, pts[:-1][::-1])
                else:
                    sb.chain(x, tip, pts[:-1])
            sb.path([x, sb.node(sb.coords[x] + np.array([-0.6, -1.3]), 1)])
            sb.node(np.array([5.3, 5.7]), 0)          # on no path
        skeletons.append(sb.arrays())
    skeletons.append((np.zeros((0, 2)), np.zeros(0, dtype=np.int64), np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64)))
    return ind, cf, skeletons


def make_ts(tsk, skeletons, dtype=torch.float32, pos=None):
    ts = tsk.skeletons_to_tensorskeleton([tsk.Skeleton(c.copy(), tsk.Paths(i.copy(), p.copy()), d.copy()) for c, i, p, d in skeletons])
    if pos is not None:
        ts.pos = pos.clone()
    ts.pos = ts.pos.detach().to(dtype)
    return ts


def make_optimizer(asm, tsk, skeletons, ind, cf, cfg, dtype, pos=None, sq=None, lr=None):
    opt = asm.TensorSkeletonOptimizer(R.config_of(cfg), make_ts(tsk, skeletons, dtype, pos), ind.to(dtype), cf.to(dtype))
    if sq is not None:
        p = opt.tensorskeleton.pos
        opt.optimizer.state[p]["step"] = torch.zeros((), dtype=torch.float32)
        opt.optimizer.state[p]["square_avg"] = sq.detach().to(dtype).clone()
    if lr is not None:
        opt.optimizer.param_groups[0]["lr"] = lr
    return opt


def square_avg(opt):
    return opt.optimizer.state[opt.tensorskeleton.pos]["square_avg"].detach().clone()


def reference_alone(asm, tsk, skeletons, ind, cf):
    """the reference's fp32 run, CALLS x CHUNK iterations, against its own float64 run of each chunk from the fp32 run's positions and state"""
    o32 = make_optimizer(asm, tsk, skeletons, ind, cf, R.DEFAULTS, torch.float32)
    pos = [o32.tensorskeleton.pos.detach().clone()]
    sq, lrs = [torch.zeros_like(pos[0])], []
    for i in range(CALLS * CHUNK):
        lrs.append(o32.optimizer.param_groups[0]["lr"])
        o32.step(i)
        if (i + 1) % CHUNK == 0:
            pos.append(o32.tensorskeleton.pos.detach().clone()); sq.append(square_avg(o32))
    devs = []
    for k in range(CALLS):
        o64 = make_optimizer(asm, tsk, skeletons, ind, cf, R.DEFAULTS, torch.float64, pos=pos[k], sq=sq[k], lr=lrs[CHUNK * k])
        for i in range(CHUNK * k, CHUNK * k + CHUNK):
            o64.step(i)
        devs.append((pos[k + 1].double() - o64.tensorskeleton.pos.detach()).abs())
    devs = torch.stack(devs)
    moved = float((pos[-1] - pos[0]).abs().max())
    still = bool(torch.equal(pos[-1], pos[-3]))
    return np.array([float((devs > 1e-4).double().mean()), float((devs > 1e-2).double().mean()), float(devs.median()), float(devs.max()), moved]), still


def main():
    import warnings
    warnings.filterwarnings("ignore")
    asm, tsk = load_reference()
    for seed in range(20, 60):
        ind, cf, skeletons = scene(seed)
        ts = make_ts(tsk, skeletons)
        tsd = {k: getattr(ts, k) for k in ("pos", "degrees", "path_index", "path_delim", "batch", "batch_delim")}
        margin = R.decision_margin(ts.pos, tsd)
        if margin <= 1e-4:
            print("seed", seed, "decision margin", margin, ": next")
            continue
        alone, still = reference_alone(asm, tsk, skeletons, ind, cf)
        print("seed %d: reference alone, %d x %d steps: share over 1e-4 = %.3g, over 1e-2 = %.3g, median = %.3g, worst = %.3g, moved %.3g px, last two calls still: %s"
              % ((seed, CALLS, CHUNK) + tuple(alone) + (still,)))
        if alone[0] <= 5e-4 and alone[1] == 0 and alone[2] <= 2e-6 and alone[4] > 0.1 and still:
            break
    else:
        raise SystemExit("no seed meets the conditions")
    print("seed", seed, "decision margin at step 0:", margin, "nodes:", ts.pos.shape[0], "path entries:", ts.path_index.shape[0], "paths:", ts.num_paths)
    out = {"seed": np.array(seed), "margin0": np.array(margin), "indicator": ind.numpy(), "c0c2": cf.numpy(), "alone.traj": alone,
           "ts.batch_size": np.array(ts.batch_size)}
    for k, v in tsd.items():
        out["ts." + k] = v.numpy().copy()
    for b, (c, i, p, d) in enumerate(skeletons):
        out.update({f"sk{b}.coordinates": c, f"sk{b}.indices": i, f"sk{b}.indptr": p, f"sk{b}.degrees": d})
    for b, sk in enumerate(tsk.tensorskeleton_to_skeletons(ts)):          # the reference's round trip
        out.update({f"rt{b}.coordinates": sk.coordinates, f"rt{b}.indices": sk.paths.indices.astype(np.int64), f"rt{b}.indptr": sk.paths.indptr.astype(np.int64)})
    pos0 = ts.pos.clone()

    # ---- the schedules: the reference's interpolators and its ExponentialLR, all 300 iterations
    opt = make_optimizer(asm, tsk, skeletons, ind, cf, R.DEFAULTS, torch.float32)
    sched = []
    for i in range(300):
        c = opt.criterion
        sched.append([float(c.data_coef_interp(i)), float(c.length_coef_interp(i)), float(c.crossfield_coef_interp(i)), opt.optimizer.param_groups[0]["lr"]])
        loss, parts = opt.step(i)
        if i + 1 in (1, 5):
            out[f"ref32.pos{i + 1}"] = opt.tensorskeleton.pos.detach().numpy().copy()
            out[f"ref32.loss{i + 1}"] = np.array([loss, parts["align"], parts["level"], parts["length"]], dtype=np.float64)
    out["sched"] = np.array(sched, dtype=np.float64)
    out["ref32.pos300"] = opt.tensorskeleton.pos.detach().numpy().copy()

    # ---- five steps in float64 from the same start: what the reference's fp32 positions differ from its float64 ones by
    o64 = make_optimizer(asm, tsk, skeletons, ind, cf, R.DEFAULTS, torch.float64)
    for i in range(5):
        o64.step(i)
    out["alone.pos5"] = np.array([float((torch.from_numpy(out["ref32.pos5"]).double() - o64.tensorskeleton.pos.detach()).abs().max())])
    print("reference alone, 5 steps: max |fp32 - float64| = %.3g" % out["alone.pos5"][0])

    # ---- gradients: the reference's pos.grad in float64 and what its fp32 one differs from it by, at three settings
    for name, cfg, it in (("it0", R.DEFAULTS, 0), ("it100", R.DEFAULTS, 100), ("align", R.ALIGN_ONLY, 0)):
        g = {}
        for dtype in (torch.float32, torch.float64):
            o = make_optimizer(asm, tsk, skeletons, ind, cf, cfg, dtype)
            o.step(it)
            g[dtype] = o.tensorskeleton.pos.grad.detach().double().clone()
        out[f"ref64.grad.{name}"] = g[torch.float64].numpy()
        out[f"alone.grad.{name}"] = np.array([float((g[torch.float32] - g[torch.float64]).abs().max())])
        print("gradient %s: reference alone max |fp32 - float64| = %.3g (largest component %.3g)" % (name, out[f"alone.grad.{name}"][0], float(g[torch.float64].abs().max())))

    # ---- the restatement the GPU tests use reproduces the reference (asserted again by tests/test_asm_cpu.py)
    for n in (1, 5):
        mine, _, last = R.optimize(pos0, torch.zeros_like(pos0), tsd, ind, cf, R.DEFAULTS, steps=n, dtype=torch.float32)
        print(f"restatement fp32 after {n} steps: max |pos - reference| = %.3g, losses rel %.3g" % (
            float((mine - torch.from_numpy(out[f'ref32.pos{n}'])).abs().max()), float(np.max(np.abs(np.array(last) / out[f'ref32.loss{n}'] - 1)))))
    for name, cfg, it in (("it0", R.DEFAULTS, 0), ("it100", R.DEFAULTS, 100), ("align", R.ALIGN_ONLY, 0)):
        g, _ = R.gradient(pos0, tsd, ind, cf, cfg, it)
        print(f"restatement float64 gradient {name}: max |g - reference| = %.3g" % float((g - torch.from_numpy(out[f"ref64.grad.{name}"])).abs().max()))
    np.savez_compressed(os.path.join(HERE, "asm.npz"), **out)
    print("wrote asm.npz", os.path.getsize(os.path.join(HERE, "asm.npz")), "bytes")


if __name__ == "__main__":
    main()
