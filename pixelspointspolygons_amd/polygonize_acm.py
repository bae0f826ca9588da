"""FFL active-contour (ACM) polygon optimisation: the device part of predict/ffl/polygonize_acm.py of the reference (`PolygonAlignLoss` and
`TensorPolyOptimizer`, :77-220, and lines 383-398 of `polygonize()`), as one HIP kernel (csrc/acm.hip, p3_acm_optimize) instead of 500 autograd steps.

The marching-squares initial contours in front (`polygonize_utils.compute_init_contours_batch`, polygonize_utils.py:15-44: skimage's find_contours per image
on the host) are built on the device too: `init_contours` (csrc/contours.hip, p3_init_contours) makes the `TensorPoly` straight from the segmentation map, and
`polygonize_device` is lines 346-398 of `polygonize()` - seg and crossfield on the device -> optimised contours on the device - with one read-back of three
counts and no host contour.  The definition init_contours is held to is DESIGN.md section 13 (a pixel that equals the level exactly is linked by grid edge,
not by coordinate).  `optimize_contours` still takes host contours a caller already has (`pre_computed={"init_contours_batch": ...}` of the reference).

`post_process` behind is polygonize_post.py: its array half (Douglas-Peucker, corner split) and its shapely half (union, polygon assembly, filters;
`polygonize_post.polygonize_acm_polygons` is the whole of `PolygonizerACM.__call__`).  `tensorpoly_to_contours_batch` still hands a caller's own post-process
the contours.
The optional `dist` term (not in the shipped config) is not built; the ASM method is polygonize_asm.py.

`TensorPoly`, `contours_batch_to_tensorpoly` and `tensorpoly_to_contours_batch` keep the reference's fields (torch_lydorn/torchvision/transforms/tensorpoly.py):
pos [N,2] (row, col), poly_slice [P,2], batch [N], batch_size, is_endpoint [N]."""
import numpy as np
import torch

from . import hip

# config/polygonization/asm_acm.yaml, acm_method
ACM_DEFAULTS = {
    "steps": 500,
    "data_level": 0.5,
    "data_coef": 0.1,
    "length_coef": 0.4,
    "crossfield_coef": 0.5,
    "poly_lr": 0.01,
    "warmup_iters": 100,
    "warmup_factor": 0.1,
    "device": "cuda",
    "tolerance": [1],
    "seg_threshold": 0.5,
    "min_area": 10,
}


def lr_coef(iter_num, warmup_iters, warmup_factor):
    """the factor on poly_lr at iteration iter_num (polygonize_acm.py:183-188; the kernel evaluates the same expression in double)"""
    if iter_num < warmup_iters:
        return 1 + (warmup_factor - 1) * (warmup_iters - iter_num) / warmup_iters
    return 1


class TensorPoly(object):
    def __init__(self, pos, poly_slice, batch, batch_size, is_endpoint=None):
        assert pos.shape[0] == batch.shape[0]
        self.pos = pos
        self.poly_slice = poly_slice
        self.batch = batch
        self.batch_size = batch_size
        self.is_endpoint = is_endpoint
        self.max_len = None          # longest polygon, known on the host when built from contours: spares the optimiser one read-back

    @property
    def num_nodes(self):
        return self.pos.shape[0]

    def to(self, device):
        self.pos = self.pos.to(device)
        self.poly_slice = self.poly_slice.to(device)
        self.batch = self.batch.to(device)
        if self.is_endpoint is not None:
            self.is_endpoint = self.is_endpoint.to(device)
        return self


def contours_batch_to_tensorpoly(contours_batch):
    """[[(n, 2) array, ...] per image] -> TensorPoly on the host, None without any contour.  A contour whose first and last points differ by >= 1e-6 is an
    open polyline (its two ends are endpoints and never move); a closed one loses its repeated last point."""
    batch_size = len(contours_batch)
    pos, batch, is_endpoint, poly_slice, at = [], [], [], [], 0
    for i, contours in enumerate(contours_batch):
        for contour in contours:
            contour = np.asarray(contour)
            ends = np.zeros(contour.shape[0], dtype=bool)
            if not np.max(np.abs(contour[0] - contour[-1])) < 1e-6:
                ends[0] = ends[-1] = True
            else:
                contour, ends = contour[:-1, :], ends[:-1]
            pos.append(contour)
            is_endpoint.append(ends)
            batch.append(np.full(contour.shape[0], i, dtype=np.int64))
            poly_slice.append((at, at + contour.shape[0]))
            at += contour.shape[0]
    if not pos:
        return None
    tensorpoly = TensorPoly(pos=torch.tensor(np.concatenate(pos, axis=0), dtype=torch.float), poly_slice=torch.tensor(poly_slice, dtype=torch.long),
                            batch=torch.tensor(np.concatenate(batch, axis=0), dtype=torch.long), batch_size=batch_size,
                            is_endpoint=torch.tensor(np.concatenate(is_endpoint, axis=0), dtype=torch.bool))
    tensorpoly.max_len = max(e - s for s, e in poly_slice)
    return tensorpoly


def tensorpoly_to_contours_batch(tensorpoly):
    """back to [[(n, 2) float32 array, ...] per image]; closed contours get their first point appended again"""
    contours_batch = [[] for _ in range(tensorpoly.batch_size)]
    pos = tensorpoly.pos.detach().cpu().numpy()
    poly_slice = tensorpoly.poly_slice.cpu().numpy()
    is_endpoint = tensorpoly.is_endpoint.cpu().numpy()
    batch = tensorpoly.batch.cpu().numpy()
    for s, e in poly_slice:
        contour = np.array(pos[s:e, :])
        if not is_endpoint[s]:          # open = the first vertex is an endpoint
            contour = np.concatenate([contour, contour[:1, :]], axis=0)
        contours_batch[int(batch[s])].append(contour)
    return contours_batch


class TensorPolyOptimizer:
    """The reference's class of the same name with the same constructor; `tensorpoly` is anything with pos / poly_slice / batch / is_endpoint on the device
    (the reference's own TensorPoly included).  optimize() runs config["steps"] iterations in one kernel launch and returns the tensorpoly, whose pos is
    updated in place; step(iter_num) runs one iteration and returns (loss, losses_dict) as the reference does - one launch and one read-back per call, meant
    for inspection, not for speed."""

    def __init__(self, config, tensorpoly, indicator, c0c2, data_coef, length_coef, crossfield_coef, dist=None, dist_coef=None):
        assert len(indicator.shape) == 3, "indicator: (N, H, W)"
        assert len(c0c2.shape) == 4 and c0c2.shape[1] == 4, "c0c2: (N, 4, H, W)"
        if dist is not None:
            raise NotImplementedError("the `dist` term of PolygonAlignLoss is not built (the shipped acm_method config has no dist_coef)")
        self.config = config
        self.tensorpoly = tensorpoly
        pos = tensorpoly.pos
        if not pos.is_cuda:
            raise hip.P3Error("TensorPolyOptimizer: the tensorpoly must be on the device (tensorpoly.to(device)); there is no CPU path")
        if pos.dtype != torch.float32 or not pos.is_contiguous():
            tensorpoly.pos = pos = pos.detach().float().contiguous()
        self.indicator = indicator.contiguous().float()
        self.c0c2 = c0c2.contiguous().float()
        self.coefs = (float(data_coef), float(length_coef), float(crossfield_coef))
        max_len = tensorpoly.max_len if isinstance(tensorpoly, TensorPoly) else None          # only a container built here is trusted to know its longest polygon
        if max_len is None:
            sl = tensorpoly.poly_slice
            max_len = int((sl[:, 1] - sl[:, 0]).max()) if sl.shape[0] else 0
        self.max_len = max_len

    def _run(self, first_iter, steps, losses):
        c, t = self.config, self.tensorpoly
        return hip.acm_optimize(t.pos.detach(), t.poly_slice, t.batch, t.is_endpoint, self.indicator, self.c0c2, *self.coefs, data_level=c["data_level"],
                                poly_lr=c["poly_lr"], warmup_iters=c["warmup_iters"], warmup_factor=c["warmup_factor"], first_iter=first_iter, steps=steps,
                                losses=losses, max_len=self.max_len)

    def step(self, iter_num):
        _, per_poly = self._run(iter_num, 1, True)
        align, level, length = (float(v) for v in per_poly.double().sum(0))
        data_coef, length_coef, crossfield_coef = self.coefs
        loss = (data_coef * level + length_coef * length + crossfield_coef * align) / (data_coef + length_coef + crossfield_coef)
        return loss, {"align": align, "level": level, "length": length}

    def optimize(self):
        self._run(0, self.config["steps"], False)
        return self.tensorpoly


def _check_maps(who, seg_batch, crossfield_batch):
    """the reference's assertions on the two maps (polygonize_acm.py:339-343, polygonize_asm.py:718-722), and: both on the device"""
    assert len(seg_batch.shape) == 4 and seg_batch.shape[1] <= 3, "seg_batch should be (N, C, H, W) with C <= 3, not {}".format(seg_batch.shape)
    assert len(crossfield_batch.shape) == 4 and crossfield_batch.shape[1] == 4, "crossfield_batch should be (N, 4, H, W)"
    assert seg_batch.shape[0] == crossfield_batch.shape[0], "Batch size for seg and crossfield should match"
    if not seg_batch.is_cuda or not crossfield_batch.is_cuda:
        raise hip.P3Error(f"{who}: seg_batch and crossfield_batch must be device tensors (there is no CPU path)")


def optimize_contours(seg_batch, crossfield_batch, init_contours_batch, config=ACM_DEFAULTS):
    """Lines 383-398 of the reference's polygonize(): initial contours per image -> optimised contours per image (same structure, closed ones closed again).
    seg_batch [B, C, H, W] (channel 0 is the indicator) and crossfield_batch [B, 4, H, W] on the device."""
    _check_maps("optimize_contours", seg_batch, crossfield_batch)
    tensorpoly = contours_batch_to_tensorpoly(init_contours_batch)
    if tensorpoly is None:
        return [[] for _ in init_contours_batch]
    tensorpoly.to(seg_batch.device)
    optimizer = TensorPolyOptimizer(config, tensorpoly, seg_batch[:, 0, :, :], crossfield_batch, config["data_coef"], config["length_coef"],
                                    config["crossfield_coef"])
    return tensorpoly_to_contours_batch(optimizer.optimize())


def init_contours(seg_or_indicator, level=0.5):
    """polygonize_utils.compute_init_contours_batch + contours_batch_to_tensorpoly on the device: seg [B, C, H, W] (channel 0 is the indicator, read in place)
    or indicator [B, H, W] -> a device TensorPoly whose max_len is filled from the one read-back (vertices, contours, longest), None without any contour."""
    if not seg_or_indicator.is_cuda:
        raise hip.P3Error("init_contours: the map must be a device tensor (there is no CPU path)")
    out = hip.init_contours(seg_or_indicator, level)
    _, P, longest = out["counts"]
    if P == 0:
        return None
    tensorpoly = TensorPoly(pos=out["pos"], poly_slice=out["poly_slice"], batch=out["batch"], batch_size=seg_or_indicator.shape[0],
                            is_endpoint=out["is_endpoint"].bool())
    tensorpoly.max_len = longest
    return tensorpoly


def polygonize_device(seg_batch, crossfield_batch, config=ACM_DEFAULTS):
    """Lines 346-398 of the reference's polygonize() without a host contour: initial contours at config["data_level"] and the optimiser, both on the device.
    -> the optimised device TensorPoly (tensorpoly_to_contours_batch hands it to the shapely stage), None without any contour."""
    _check_maps("polygonize_device", seg_batch, crossfield_batch)
    tensorpoly = init_contours(seg_batch, config["data_level"])
    if tensorpoly is None:
        return None
    optimizer = TensorPolyOptimizer(config, tensorpoly, seg_batch[:, 0, :, :], crossfield_batch, config["data_coef"], config["length_coef"],
                                    config["crossfield_coef"])
    return optimizer.optimize()
