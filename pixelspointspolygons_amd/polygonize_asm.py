"""FFL active-skeleton (ASM) optimisation: the device part of predict/ffl/polygonize_asm.py of the reference (`AlignLoss` and `TensorSkeletonOptimizer`,
:133-421, and lines 731-752 of `PolygonizerASM.__call__`), as one HIP kernel (csrc/asm.hip, p3_asm_optimize) instead of 300 autograd steps.

The reference differentiates `data_coef * level_loss + length_coef * total_length_loss + crossfield_coef * total_align_loss` (:353): its curvature, corner
and junction terms are computed and reported but never reach the positions.  They are not built here, and `step()` does not report them.

The marching-squares initialisation in front (`init_method: marching_squares`, get_marching_squares_skeleton :581-638) runs on the device too:
`init_skeletons` chains p3_init_contours, p3_skeleton_from_contours and p3_asm_plan (csrc/skeleton_init.hip), and `polygonize_device` is seg and crossfield
on the device -> optimised skeleton on the device, with one read-back of a few counts per stage and no host contour.
`contours_to_skeleton`, `skeletons_to_tensorskeleton` and the host `AsmPlan` stay for callers that already hold host contours or skeletons.

The reference's default initialisation (`init_method: skeleton`, compute_skeletons :655-675 and get_skeleton: skimage binary_closing, skimage skeletonize,
skan.Skeleton) has a device restatement under a name of its own, `init_method: skeleton_device`: p3_skeleton_from_seg (csrc/skeleton_thin.hip) builds the edge
mask, closes it, thins it with Zhang-Suen and reads the path graph off the skeleton, junctions and shared walls included (DESIGN.md section 20 holds the
definition and the two stated deviations from skimage and skan).  `init_skeletons(..., method="skeleton_device")` and `polygonize_device` take it.

What stays host code of the caller: the `skimage` skeletonize plus `skan` initialisation itself (`init_method: skeleton`), which still raises here.
`post_process` behind is polygonize_post.py: `corner_split_skeleton`, and `polygonize_asm_polygons` for the whole of `PolygonizerASM.__call__` down to the
filtered polygons.

`Skeleton`, `Paths`, `TensorSkeleton`, `skeletons_to_tensorskeleton` and `tensorskeleton_to_skeletons` keep the fields of
torch_lydorn/torchvision/transforms/tensorskeleton.py: pos [N,2] (row, col), degrees [N], path_index [M], path_delim [P+1], batch [N], batch_delim [B+1],
batch_size.  One difference: path_delim always ends with M here.  The reference drops that last entry when the LAST skeleton of a batch is a default
`Skeleton()` (whose indptr is empty instead of [0]), which merges the batch's last two paths; for every other batch the fields are equal."""
import numpy as np
import torch

from . import hip
from .polygonize_acm import _check_maps

# config/polygonization/asm_acm.yaml, asm_method
ASM_DEFAULTS = {
    "init_method": "skeleton",
    "data_level": 0.5,
    "loss_params": {
        "coefs": {
            "step_thresholds": [0, 100, 200, 300],
            "data": [1.0, 0.1, 0.0, 0.0],
            "crossfield": [0.0, 0.05, 0.0, 0.0],
            "length": [0.1, 0.01, 0.0, 0.0],
            "curvature": [0.0, 0.0, 1.0, 0.0],
            "corner": [0.0, 0.0, 0.5, 0.0],
            "junction": [0.0, 0.0, 0.5, 0.0],
        },
        "curvature_dissimilarity_threshold": 2,
        "corner_angles": [45, 90, 135],
        "corner_angle_threshold": 22.5,
        "junction_angles": [0, 45, 90, 135],
        "junction_angle_weights": [1, 0.01, 0.1, 0.01],
        "junction_angle_threshold": 22.5,
    },
    "lr": 0.1,
    "gamma": 0.995,
    "device": "cuda",
    "tolerance": [1],
    "seg_threshold": 0.5,
    "min_area": 10,
}


class Skeleton:
    def __init__(self, coordinates=None, paths=None, degrees=None):
        self.coordinates = np.empty((0, 2), dtype=np.float64) if coordinates is None else coordinates
        self.paths = Paths() if paths is None else paths
        self.degrees = np.empty(0, dtype=np.int64) if degrees is None else degrees


class Paths:
    def __init__(self, indices=None, indptr=None):
        self.indices = np.empty(0, dtype=np.int64) if indices is None else indices
        self.indptr = np.empty(0, dtype=np.int64) if indptr is None else indptr


class TensorSkeleton(object):
    def __init__(self, pos, degrees, path_index, path_delim, batch, batch_delim, batch_size):
        assert pos.shape[0] == batch.shape[0]
        self.pos = pos
        self.degrees = degrees
        self.path_index = path_index
        self.path_delim = path_delim
        self.batch = batch
        self.batch_delim = batch_delim
        self.batch_size = batch_size
        self.plan = None          # AsmPlan, known on the host when built by skeletons_to_tensorskeleton: spares the optimiser its one read-back

    @property
    def num_nodes(self):
        return self.pos.shape[0]

    @property
    def num_paths(self):
        return max(0, self.path_delim.shape[0] - 1)

    def to(self, device):
        for k in ("pos", "degrees", "path_index", "path_delim", "batch", "batch_delim"):
            setattr(self, k, getattr(self, k).to(device))
        if self.plan is not None:
            self.plan = self.plan.to(device)
        return self


class AsmPlan:
    """What p3_asm_optimize needs besides the containers, derived from path_index / path_delim on the host (csrc/asm.hip explains the arrays).  Components are
    ordered by their smallest node id and list their nodes in ascending id; `node_local` is a node's index inside its component, `slot_k` the position in
    path_index of each occurrence slot (ascending per node).  Path boundaries are the INTERIOR entries of path_delim, as AlignLoss reads them (:185, :230-233):
    the first path starts at 0 and the last ends at M."""

    FIELDS = ("comp_ptr", "cn_node", "cn_occ", "slot_nb", "node_local", "slot_k")

    def __init__(self, path_index, path_delim, num_nodes):
        idx = np.asarray(path_index, dtype=np.int64).reshape(-1)
        delim = np.asarray(path_delim, dtype=np.int64).reshape(-1)
        N, M = int(num_nodes), idx.shape[0]
        if M and (idx.min() < 0 or idx.max() >= N):
            raise hip.P3Error(f"AsmPlan: path_index holds node ids outside [0, {N})")
        start, end = np.zeros(M, dtype=bool), np.zeros(M, dtype=bool)
        if M:
            cuts = delim[1:-1]
            cuts = cuts[(cuts >= 1) & (cuts <= M - 1)]
            start[0] = end[M - 1] = True
            start[cuts] = True
            end[cuts - 1] = True
        # connected components: hook every edge's two labels to the smaller one, then jump, until nothing changes; a node's label ends as its component's smallest id
        a, b = idx[:-1][~end[:-1]], idx[1:][~end[:-1]]
        lab = np.arange(N, dtype=np.int64)
        while a.size:
            m = np.minimum(lab[a], lab[b])
            new = lab.copy()
            np.minimum.at(new, a, m)
            np.minimum.at(new, b, m)
            new = new[new]
            if np.array_equal(new, lab):
                break
            lab = new
        cn_node = np.argsort(lab, kind="stable")
        firsts = np.flatnonzero(np.diff(lab[cn_node], prepend=-1) != 0) if N else np.zeros(0, dtype=np.int64)
        comp_ptr = np.concatenate([firsts, [N]])
        cn_pos = np.empty(N, dtype=np.int64)
        cn_pos[cn_node] = np.arange(N)
        comp_of = np.repeat(np.arange(len(firsts)), np.diff(comp_ptr))          # per cn entry
        node_local = np.empty(N, dtype=np.int64)
        node_local[cn_node] = np.arange(N) - firsts[comp_of] if N else 0
        slot_k = np.argsort(cn_pos[idx], kind="stable")
        cn_occ = np.concatenate([[0], np.cumsum(np.bincount(cn_pos[idx], minlength=N))])
        prev = np.where(start, -1, node_local[idx[np.maximum(np.arange(M) - 1, 0)]]) if M else np.zeros(0, dtype=np.int64)
        nxt = np.where(end, -1, node_local[idx[np.minimum(np.arange(M) + 1, M - 1)]]) if M else np.zeros(0, dtype=np.int64)
        slot_nb = np.stack([prev[slot_k], nxt[slot_k]], 1) if M else np.zeros((0, 2), dtype=np.int64)
        self.num_nodes, self.num_slots, self.num_comps = N, M, len(firsts)
        self.max_comp = int(np.diff(comp_ptr).max()) if len(firsts) else 0
        for k, v in zip(self.FIELDS, (comp_ptr, cn_node, cn_occ, slot_nb, node_local, slot_k)):
            setattr(self, k, torch.from_numpy(np.ascontiguousarray(v, dtype=np.int32)))

    def to(self, device):
        for k in self.FIELDS:
            setattr(self, k, getattr(self, k).to(device))
        return self


class AsmDevicePlan:
    """The plan of p3_asm_optimize built on the device by p3_asm_plan (hip.asm_plan): the six arrays of AsmPlan.FIELDS, equal to the host class entry for
    entry, and the same four counts; the host has seen the component count and the largest component only."""

    FIELDS = AsmPlan.FIELDS

    def __init__(self, arrays, num_nodes, num_slots):
        for k in self.FIELDS:
            setattr(self, k, arrays[k])
        self.num_nodes, self.num_slots = int(num_nodes), int(num_slots)
        self.num_comps, self.max_comp = arrays["counts"]

    def to(self, device):
        for k in self.FIELDS:
            setattr(self, k, getattr(self, k).to(device))
        return self


def asm_plan_device(tensorskeleton):
    """The plan of any container with pos / path_index / path_delim on the device (the reference's own TensorSkeleton included), built there: one read-back
    of (components, largest component, status).  Raises P3Error on a node id outside [0, N).  TensorSkeletonOptimizer takes it as `tensorskeleton.plan`."""
    if not tensorskeleton.path_index.is_cuda or not tensorskeleton.path_delim.is_cuda:
        raise hip.P3Error("asm_plan_device: the tensorskeleton must be on the device; AsmPlan builds the plan on the host")
    N = tensorskeleton.pos.shape[0]
    return AsmDevicePlan(hip.asm_plan(tensorskeleton.path_index, tensorskeleton.path_delim, N), N, tensorskeleton.path_index.shape[0])


def skeletons_to_tensorskeleton(skeletons_batch, device=None):
    """tensorskeleton.py:87-159: B skeletons -> one TensorSkeleton (node ids, path positions and path numbers offset image by image).  The skeletons are
    not modified.  The result carries its AsmPlan."""
    batch_size = len(skeletons_batch)
    pos, degrees, path_index, path_delim, batch, batch_delim = [], [], [], [np.zeros(1, dtype=np.int64)], [], [0] if batch_size else []
    n_off = m_off = p_off = 0
    for i, sk in enumerate(skeletons_batch):
        n, m = sk.coordinates.shape[0], sk.paths.indices.shape[0]
        pos.append(np.asarray(sk.coordinates, dtype=np.float64).reshape(-1, 2))
        degrees.append(np.asarray(sk.degrees, dtype=np.int64))
        path_index.append(np.asarray(sk.paths.indices, dtype=np.int64) + n_off)
        path_delim.append(np.asarray(sk.paths.indptr, dtype=np.int64)[1:] + m_off)
        batch.append(np.full(n, i, dtype=np.int64))
        n_off, m_off, p_off = n_off + n, m_off + m, p_off + max(0, sk.paths.indptr.shape[0] - 1)
        batch_delim.append(p_off)
    cat = lambda parts, shape: np.concatenate(parts, axis=0) if parts else np.zeros(shape, dtype=np.int64)
    ts = TensorSkeleton(pos=torch.tensor(cat(pos, (0, 2)), dtype=torch.float), degrees=torch.tensor(cat(degrees, 0), dtype=torch.long),
                        path_index=torch.tensor(cat(path_index, 0), dtype=torch.long), path_delim=torch.tensor(cat(path_delim, 0), dtype=torch.long),
                        batch=torch.tensor(cat(batch, 0), dtype=torch.long), batch_delim=torch.tensor(batch_delim, dtype=torch.long), batch_size=batch_size)
    ts.plan = AsmPlan(ts.path_index.numpy(), ts.path_delim.numpy(), ts.num_nodes)
    return ts.to(device) if device is not None else ts


def tensorskeleton_to_skeletons(tensorskeleton):
    """tensorskeleton.py:162-192: back to one Skeleton per image (coordinates float32, paths with image-local ids; degrees are not carried, as in the
    reference); an image without a path gives an empty Skeleton()."""
    pos = tensorskeleton.pos.detach().cpu().numpy()
    path_index, path_delim = tensorskeleton.path_index.cpu().numpy(), tensorskeleton.path_delim.cpu().numpy()
    batch, batch_delim = tensorskeleton.batch.cpu().numpy(), tensorskeleton.batch_delim.cpu().numpy()
    skeletons, n_off, m_off = [], 0, 0
    for i in range(tensorskeleton.batch_size):
        indptr = path_delim[batch_delim[i]:batch_delim[i + 1] + 1]
        coordinates = pos[batch == i]
        if indptr.shape[0] >= 2:
            indices = path_index[indptr[0]:indptr[-1]]
            skeletons.append(Skeleton(coordinates, Paths(indices - n_off, indptr - m_off)))
            m_off += indices.shape[0]
        else:
            skeletons.append(Skeleton())
        n_off += coordinates.shape[0]          # also for an image with nodes and no path (the reference forgets those nodes in its offset)
    return skeletons


def skeleton_to_polylines(skeleton):
    """polygonize_asm.py:697-704: one [n, 2] array per path; a closed path keeps its repeated end point"""
    polylines = []
    for path_i in range(skeleton.paths.indptr.shape[0] - 1):
        start, stop = skeleton.paths.indptr[path_i:path_i + 2]
        polylines.append(skeleton.coordinates[skeleton.paths.indices[start:stop]])
    return polylines


def contours_to_skeleton(contours, min_area=None):
    """The conversion half of get_marching_squares_skeleton (:603-638): contours ([n, 2] arrays, (row, col)) -> Skeleton.  A closed contour (first and last
    points within 1e-6) drops its repeated point and repeats its index; an open one gets degree-1 ends.  min_area: keep only contours with at least 3
    vertices and a shoelace area above it (:591-592, what shapely's Polygon(contour).area computes)."""
    contours = [np.asarray(c, dtype=np.float64) for c in contours]
    if min_area is not None:
        area = lambda c: 0.5 * abs(float(np.dot(c[:, 0], np.roll(c[:, 1], -1)) - np.dot(c[:, 1], np.roll(c[:, 0], -1))))
        contours = [c for c in contours if 3 <= c.shape[0] and min_area < area(c)]
    if len(contours) == 0:
        return Skeleton()
    coordinates, degrees, indices, indptr, off = [], [], [], [0], 0
    for contour in contours:
        is_closed = np.max(np.abs(contour[0] - contour[-1])) < 1e-6
        c = contour[:-1, :] if is_closed else contour
        d = 2 * np.ones(c.shape[0], dtype=np.int64)
        if not is_closed:
            d[0] = d[-1] = 1
        ids = list(range(off, off + c.shape[0]))
        if is_closed:
            ids.append(ids[0])
        coordinates.append(c); degrees.append(d); indices.extend(ids)
        indptr.append(indptr[-1] + len(ids))
        off += c.shape[0]
    return Skeleton(np.concatenate(coordinates, axis=0), Paths(np.array(indices, dtype=np.int64), np.array(indptr, dtype=np.int64)), np.concatenate(degrees, axis=0))


def _knots(config):
    c = config["loss_params"]["coefs"]
    return [[float(v) for v in c[k]] for k in ("step_thresholds", "data", "length", "crossfield")]


def asm_schedule(iter_num, config=ASM_DEFAULTS):
    """(data_coef, length_coef, crossfield_coef, lr) of iteration iter_num as Python floats: scipy's linear interp1d over loss_params.coefs (:151-156,
    342-344; numpy.interp's segment choice, so a knot gives its own value exactly) and ExponentialLR's chained lr * gamma^i (:381); the kernel evaluates
    the same expressions in double and rounds them to float"""
    x, *ys = _knots(config)
    lo = 0
    for j in range(1, len(x) - 1):
        if x[j] <= iter_num:
            lo = j
    out = []
    for y in ys:
        slope = (y[lo + 1] - y[lo]) / (x[lo + 1] - x[lo])
        out.append(y[lo + 1] if iter_num == x[lo + 1] else slope * (iter_num - x[lo]) + y[lo])
    lr = float(config["lr"])
    for _ in range(iter_num):
        lr = lr * config["gamma"]
    return (*out, lr)


class TensorSkeletonOptimizer:
    """The reference's class of the same name with the same constructor; `tensorskeleton` is anything with pos / degrees / path_index / path_delim / batch on
    the device (the reference's own TensorSkeleton included: its plan is then built here on the host, with one read-back of path_index and path_delim, unless
    its `plan` attribute holds the result of asm_plan_device).  optimize() runs
    step_thresholds[-1] iterations in one kernel launch, reads nothing back and returns the tensorskeleton, whose pos is updated in place.  step(iter_num)
    runs one iteration and returns (loss, losses_dict) - one launch and one read-back per call, meant for inspection, not for speed.  losses_dict holds
    "align", "level" and "length"; the reference's "curvature", "corner" and "junction" entries, which never enter its total_loss, are not produced.
    The RMSprop state lives in self.sq, the gradient of the last step() in self.grad (the reference's pos.grad)."""

    def __init__(self, config, tensorskeleton, indicator, c0c2):
        assert len(indicator.shape) == 3, f"indicator should be of shape (N, H, W), not {indicator.shape}"
        assert len(c0c2.shape) == 4 and c0c2.shape[1] == 4, f"c0c2 should be of shape (N, 4, H, W), not {c0c2.shape}"
        self.config = config
        self.tensorskeleton = tensorskeleton
        pos = tensorskeleton.pos
        if not pos.is_cuda or not indicator.is_cuda or not c0c2.is_cuda:
            raise hip.P3Error("TensorSkeletonOptimizer: the tensorskeleton and the maps must be on the device; there is no CPU path")
        if pos.dtype != torch.float32 or not pos.is_contiguous() or pos.requires_grad:
            tensorskeleton.pos = pos = pos.detach().float().contiguous()
        N = pos.shape[0]
        self.is_tip = (tensorskeleton.degrees == 1)[:N].to(torch.uint8).contiguous()          # the reference clamps the length too (:372)
        self.batch = tensorskeleton.batch.to(torch.int32).contiguous()
        self.indicator = indicator.contiguous().float()
        self.c0c2 = c0c2.contiguous().float()
        plan = getattr(tensorskeleton, "plan", None)
        if not isinstance(tensorskeleton, TensorSkeleton) and not isinstance(plan, AsmDevicePlan):          # only a container or a plan built here is trusted
            plan = None
        if plan is None:
            plan = AsmPlan(tensorskeleton.path_index.cpu().numpy(), tensorskeleton.path_delim.cpu().numpy(), N).to(pos.device)
        self.plan = plan
        self.knots = _knots(config)
        self.sq = torch.zeros_like(pos)
        self.grad = torch.zeros_like(pos)

    def _run(self, first_iter, steps, inspect):
        c, t = self.config, self.tensorskeleton
        return hip.asm_optimize(t.pos, self.sq, self.plan, self.is_tip, self.batch, self.indicator, self.c0c2, self.knots, data_level=c["data_level"], lr=c["lr"],
                                gamma=c["gamma"], first_iter=first_iter, steps=steps, grad_out=self.grad if inspect else None, losses=inspect)

    def step(self, iter_num):
        _, per_comp = self._run(iter_num, 1, True)
        align, level, length = (float(v) for v in per_comp.double().sum(0))
        data_coef, length_coef, crossfield_coef, _ = asm_schedule(iter_num, self.config)
        loss = data_coef * level + length_coef * length + crossfield_coef * align
        return loss, {"align": align, "level": level, "length": length}

    def optimize(self):
        self._run(0, int(self.config["loss_params"]["coefs"]["step_thresholds"][-1]), False)
        return self.tensorskeleton


def optimize_skeletons(seg_batch, crossfield_batch, skeletons_batch, config=ASM_DEFAULTS):
    """Lines 731-752 of PolygonizerASM.__call__: initial skeletons per image -> optimised polylines per image ([n, 2] float32 arrays, one per path); empty
    lists when no image has a path.  seg_batch [B, C, H, W] (channel 0 is the indicator) and crossfield_batch [B, 4, H, W] on the device."""
    _check_maps("optimize_skeletons", seg_batch, crossfield_batch)
    tensorskeleton = skeletons_to_tensorskeleton(skeletons_batch)
    if tensorskeleton.num_paths == 0:
        return [[] for _ in range(seg_batch.shape[0])]
    tensorskeleton.to(seg_batch.device)
    optimizer = TensorSkeletonOptimizer(config, tensorskeleton, seg_batch[:, 0, :, :], crossfield_batch)
    return [skeleton_to_polylines(sk) for sk in tensorskeleton_to_skeletons(optimizer.optimize())]


INIT_METHODS = ("marching_squares", "skeleton_device")          # what init_skeletons builds on the device


def init_skeletons(seg_or_indicator, level=0.5, min_area=10, method="marching_squares"):
    """The initial skeletons of a batch on the device: seg [B, C, H, W] (channel 0 is the indicator, read in place) or indicator [B, H, W] -> a device
    TensorSkeleton that carries its device-built plan, None when no path is kept.  No contour, node or path index reaches the host.
    method "marching_squares": get_marching_squares_skeleton per image + skeletons_to_tensorskeleton; min_area None keeps every contour.  Three stages
    (contours, skeleton, plan), each with one read-back of its counts.
    method "skeleton_device": p3_skeleton_from_seg (edge mask from channel 0 and, when there is one, the edge channel 1; closing; thinning; path graph) and
    the plan, two read-backs.  min_area is unused there, as in the reference's get_skeleton."""
    if method not in INIT_METHODS:
        raise ValueError(f"init_skeletons: method = {method!r}; built on the device: {', '.join(INIT_METHODS)}")
    if not seg_or_indicator.is_cuda:
        raise hip.P3Error("init_skeletons: the map must be a device tensor (there is no CPU path)")
    B = seg_or_indicator.shape[0]
    if method == "skeleton_device":
        sk = hip.skeleton_from_seg(seg_or_indicator if seg_or_indicator.dim() == 4 else seg_or_indicator[:, None], level)
    else:
        c = hip.init_contours(seg_or_indicator, level)
        if c["counts"][1] == 0:
            return None
        sk = hip.skeleton_from_contours(c["pos"], c["poly_slice"], c["poly_batch"], c["is_endpoint"], B, min_area)
    if sk["counts"][2] == 0:
        return None
    tensorskeleton = TensorSkeleton(pos=sk["pos"], degrees=sk["degrees"], path_index=sk["path_index"], path_delim=sk["path_delim"], batch=sk["batch"],
                                    batch_delim=sk["batch_delim"], batch_size=B)
    tensorskeleton.plan = asm_plan_device(tensorskeleton)
    return tensorskeleton


def polygonize_device(seg_batch, crossfield_batch, config=ASM_DEFAULTS):
    """PolygonizerASM.__call__ (:715-752) without a host skeleton: initial skeletons at config["data_level"] (and config["min_area"] for marching squares),
    the plan and the optimiser, all on the device.  -> the optimised device TensorSkeleton (polygonize_post.corner_split_skeleton or
    tensorskeleton_to_skeletons take it from there), None when no path is kept.  config["init_method"]: "marching_squares" or "skeleton_device" (DESIGN.md
    section 20).  ASM_DEFAULTS keeps the reference's "skeleton", the skimage / skan route itself, which is not built: pass
    {**ASM_DEFAULTS, "init_method": "skeleton_device"}."""
    method = config["init_method"]
    if method == "skeleton":
        # the message this case has always raised, word for word, and behind it where the device restatement is found
        raise NotImplementedError(f"init_method = {method!r}: only \"marching_squares\" is built on the device; the skimage skeletonize / skan "
                                  "initialisation (\"skeleton\") is host code of the caller, whose skeletons optimize_skeletons takes.  Of the reference's "
                                  "methods, that is: a device restatement of \"skeleton\" with two stated deviations from skimage and skan has a name of its "
                                  "own, init_method \"skeleton_device\" (DESIGN.md section 20)")
    if method not in INIT_METHODS:
        raise NotImplementedError(f"init_method = {method!r} not recognized; built on the device: {', '.join(INIT_METHODS)}")
    _check_maps("polygonize_device", seg_batch, crossfield_batch)
    tensorskeleton = init_skeletons(seg_batch, config["data_level"], config["min_area"], method)
    if tensorskeleton is None:
        return None
    return TensorSkeletonOptimizer(config, tensorskeleton, seg_batch[:, 0, :, :], crossfield_batch).optimize()
