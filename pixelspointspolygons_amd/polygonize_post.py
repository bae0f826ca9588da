"""FFL corner-aware contour simplification on the device: the array half of the reference's `post_process` (predict/ffl/polygonize_acm.py:260-284 and
polygonize_asm.py:498-504) - approximate_polygon, detect_corners over compute_crossfield_uv, split_polylines_corner and LineString.simplify per piece -
as one call of csrc/corner_split.hip (p3_corner_split) on the optimised `TensorPoly` (ACM) or `TensorSkeleton` (ASM) that never left the GPU.  DESIGN.md
section 14 holds the definition; Douglas-Peucker is held to a float64 restatement and hand-checkable cases, not to skimage or GEOS.

The planar-graph half behind it - `LineString(piece[:, ::-1])` per piece, the border ring, `shapely.ops.unary_union`, `polygonize_full`, the area /
probability filters - runs on the device too: `polygons_from_pieces` (csrc/ffl_polygons.hip, p3_ffl_polygons) makes polygons with
holes, areas, probabilities and filter flags out of the pieces, `polygonize_acm_polygons` / `polygonize_asm_polygons` are the whole of
`PolygonizerACM.__call__` / `PolygonizerASM.__call__`, and `polygons_to_host` gives the reference's (polygons_batch, probs_batch).  An image whose pieces
are not planar as given (GEOS would insert nodes there) is flagged in image_status and gives no polygon: for that image the caller runs the shapely block of
INTEGRATION.md on `pieces_to_host`.

A tolerance list gives a dict keyed "tol_{}", as the reference's shapely_postprocess does."""
import numpy as np
import torch

from . import hip, polygonize_acm, polygonize_asm


def _is_list(tolerance):
    return not isinstance(tolerance, (int, float)) and hasattr(tolerance, "__iter__")


def _check(container, crossfield_batch, name):
    if not container.pos.is_cuda or not crossfield_batch.is_cuda:
        raise hip.P3Error(f"{name}: the container and crossfield_batch must be on the device (there is no CPU path)")
    if crossfield_batch.dim() != 4 or crossfield_batch.shape[1] != 4:
        raise hip.P3Error(f"{name}: crossfield_batch should be (N, 4, H, W), got {tuple(crossfield_batch.shape)}")


def corner_split_tensorpoly(tensorpoly, crossfield_batch, tolerance, force_fallback=False, stage_flags=False):
    """The ACM form (polygonize_acm.py:277-284): a contour whose first vertex is no endpoint is closed (its first point is appended again, as
    tensorpoly_to_contours_batch does), stage A runs at min(1, tolerance).  -> the trimmed dict of hip.corner_split plus batch_size, or a dict of those
    keyed "tol_{}" for a tolerance list.  One read-back (counts and status) per tolerance."""
    _check(tensorpoly, crossfield_batch, "corner_split_tensorpoly")
    if _is_list(tolerance):
        return {"tol_{}".format(t): corner_split_tensorpoly(tensorpoly, crossfield_batch, t, force_fallback, stage_flags) for t in tolerance}
    sl, N = tensorpoly.poly_slice, tensorpoly.pos.shape[0]
    first = sl[:, 0].clamp(0, max(N - 1, 0)).long()
    closed = ~tensorpoly.is_endpoint.bool().index_select(0, first) if N else torch.zeros(sl.shape[0], dtype=torch.bool, device=sl.device)
    poly_batch = tensorpoly.batch.index_select(0, first) if N else torch.zeros(sl.shape[0], dtype=torch.long, device=sl.device)
    out = hip.corner_split(tensorpoly.pos.detach().float(), None, sl, closed, poly_batch, crossfield_batch, min(1, tolerance), tolerance,
                           max_len=getattr(tensorpoly, "max_len", None), force_fallback=force_fallback, stage_flags=stage_flags)
    out["batch_size"] = tensorpoly.batch_size
    return out


def corner_split_skeleton(tensorskeleton, crossfield_batch, tolerance, force_fallback=False, stage_flags=False):
    """The ASM form (polygonize_asm.py:498-504): the paths of path_index / path_delim as they are (a ring already repeats its node), no stage A."""
    _check(tensorskeleton, crossfield_batch, "corner_split_skeleton")
    if _is_list(tolerance):
        return {"tol_{}".format(t): corner_split_skeleton(tensorskeleton, crossfield_batch, t, force_fallback, stage_flags) for t in tolerance}
    idx, delim, N = tensorskeleton.path_index.long(), tensorskeleton.path_delim.long(), tensorskeleton.pos.shape[0]
    P = max(delim.shape[0] - 1, 0)
    sl = torch.stack([delim[:-1], delim[1:]], 1) if P else torch.zeros((0, 2), dtype=torch.long, device=idx.device)
    closed = torch.zeros(P, dtype=torch.bool, device=idx.device)
    if P and N and idx.shape[0]:
        node = idx.index_select(0, sl[:, 0].clamp(0, idx.shape[0] - 1)).clamp(0, N - 1)          # image of a path = image of its first node
        poly_batch = tensorskeleton.batch.index_select(0, node)
    else:
        poly_batch = torch.zeros(P, dtype=torch.long, device=idx.device)
    out = hip.corner_split(tensorskeleton.pos.detach().float(), idx, sl, closed, poly_batch, crossfield_batch, 0.0, tolerance, force_fallback=force_fallback,
                           stage_flags=stage_flags)
    out["batch_size"] = tensorskeleton.batch_size
    return out


def pieces_to_host(result):
    """-> per image a list of float64 [n, 2] (row, col) arrays, in the device's order; one download per field.  A "tol_{}" dict gives a dict of those."""
    if "out_pos" not in result:
        return {k: pieces_to_host(v) for k, v in result.items()}
    pos = result["out_pos"].cpu().numpy().astype(np.float64)
    sl = result["piece_slice"].cpu().numpy()
    pb = result["piece_batch"].cpu().numpy()
    out = [[] for _ in range(int(result["batch_size"]))]
    for (s, e), b in zip(sl, pb):
        out[int(b)].append(pos[s:e])
    return out


def _empty_pieces(seg_batch, tolerance):
    dev = seg_batch.device
    empty = lambda: {"out_pos": torch.zeros((0, 2), dtype=torch.float32, device=dev), "out_src": torch.zeros(0, dtype=torch.int32, device=dev),
                     "piece_slice": torch.zeros((0, 2), dtype=torch.int64, device=dev), "piece_poly": torch.zeros(0, dtype=torch.int32, device=dev),
                     "piece_batch": torch.zeros(0, dtype=torch.int32, device=dev), "counts": (0, 0, 0), "batch_size": seg_batch.shape[0]}
    return {"tol_{}".format(t): empty() for t in tolerance} if _is_list(tolerance) else empty()


def polygonize_acm_pieces(seg_batch, crossfield_batch, config=polygonize_acm.ACM_DEFAULTS, tolerance=None):
    """polygonize_acm.polygonize_device followed by the ACM form at config["tolerance"] (or `tolerance`): seg and crossfield on the device -> the pieces on the
    device.  Without any contour: an empty result (None per tolerance is never returned)."""
    tolerance = config["tolerance"] if tolerance is None else tolerance
    tensorpoly = polygonize_acm.polygonize_device(seg_batch, crossfield_batch, config)
    if tensorpoly is None:
        return _empty_pieces(seg_batch, tolerance)
    return corner_split_tensorpoly(tensorpoly, crossfield_batch, tolerance)


def polygonize_asm_pieces(seg_batch, crossfield_batch, config, tolerance=None):
    """The ASM twin: polygonize_asm.polygonize_device (config["init_method"]: "marching_squares" or "skeleton_device") followed by the ASM form at config["tolerance"] (or
    `tolerance`).  Without any kept path: the same empty result as polygonize_acm_pieces."""
    tolerance = config["tolerance"] if tolerance is None else tolerance
    tensorskeleton = polygonize_asm.polygonize_device(seg_batch, crossfield_batch, config)
    if tensorskeleton is None:
        return _empty_pieces(seg_batch, tolerance)
    return corner_split_skeleton(tensorskeleton, crossfield_batch, tolerance)


# ------------------------------------------------------------------------------------------ polygons
def _indicator(seg_batch, name):
    if not torch.is_tensor(seg_batch) or not seg_batch.is_cuda:
        raise hip.P3Error(f"{name}: seg_batch must be on the device (there is no CPU path)")
    if seg_batch.dim() != 4 or seg_batch.shape[1] < 1:
        raise hip.P3Error(f"{name}: seg_batch should be (N, C, H, W), got {tuple(seg_batch.shape)}")
    return seg_batch[:, 0]


def polygons_from_pieces(result, seg_batch, config, force_fallback=False):
    """The pieces of a corner-split result (or its "tol_{}" dict) -> polygons on the device: hip.ffl_polygons on the indicator seg_batch[:, 0] with
    config["min_area"] and config["seg_threshold"].  -> the trimmed dict of hip.ffl_polygons plus batch_size, or a dict of those keyed "tol_{}".  One
    read-back (counts and status) per tolerance."""
    indicator = _indicator(seg_batch, "polygons_from_pieces")
    if "out_pos" not in result:
        return {k: polygons_from_pieces(v, seg_batch, config, force_fallback) for k, v in result.items()}
    if not result["out_pos"].is_cuda:
        raise hip.P3Error("polygons_from_pieces: the pieces must be on the device (there is no CPU path)")
    if int(result["batch_size"]) != indicator.shape[0]:
        raise hip.P3Error(f"polygons_from_pieces: the pieces come from {result['batch_size']} images, seg_batch holds {indicator.shape[0]}")
    out = hip.ffl_polygons(result["out_pos"], result["piece_slice"], result["piece_batch"], indicator, config["min_area"], config["seg_threshold"],
                           force_fallback=force_fallback)
    out["batch_size"] = indicator.shape[0]
    return out


def polygonize_acm_polygons(seg_batch, crossfield_batch, config=polygonize_acm.ACM_DEFAULTS, tolerance=None):
    """PolygonizerACM.__call__ on the device: polygonize_acm_pieces followed by polygons_from_pieces.  A batch without any contour gives the border
    polygon of every image (the filters decide about it), never None."""
    _indicator(seg_batch, "polygonize_acm_polygons")
    return polygons_from_pieces(polygonize_acm_pieces(seg_batch, crossfield_batch, config, tolerance), seg_batch, config)


def polygonize_asm_polygons(seg_batch, crossfield_batch, config, tolerance=None):
    """PolygonizerASM.__call__ (config["init_method"]: "marching_squares" or "skeleton_device") on the device: polygonize_asm_pieces followed by polygons_from_pieces."""
    _indicator(seg_batch, "polygonize_asm_polygons")
    return polygons_from_pieces(polygonize_asm_pieces(seg_batch, crossfield_batch, config, tolerance), seg_batch, config)


def polygons_to_host(result, kept_only=True):
    """-> (polygons_batch, probs_batch, image_status): per image a list of (exterior, [interiors]) with float64 [n, 2] (x, y) arrays, closed, ready for
    shapely.geometry.Polygon(*p), and the list of their probabilities, in the device's order; image_status as a list of ints (an image with a bit set has
    no polygon here: INTEGRATION.md).  kept_only: leave out the polygons a filter flagged (poly_flags != 0), as the reference does.  A "tol_{}" dict
    gives a dict of those.  One download per field."""
    if "ring_pos" not in result:
        return {k: polygons_to_host(v, kept_only) for k, v in result.items()}
    pos = result["ring_pos"].cpu().numpy().astype(np.float64)[:, ::-1]
    rsl, prs = result["ring_slice"].cpu().numpy(), result["poly_rings"].cpu().numpy()
    pb, prob, flags = result["poly_batch"].cpu().numpy(), result["poly_prob"].cpu().numpy(), result["poly_flags"].cpu().numpy()
    B = int(result["batch_size"])
    polygons, probs = [[] for _ in range(B)], [[] for _ in range(B)]
    for (r0, r1), b, p, f in zip(prs, pb, prob, flags):
        if kept_only and f:
            continue
        rings = [np.ascontiguousarray(pos[s:e]) for s, e in rsl[r0:r1]]
        polygons[int(b)].append((rings[0], rings[1:]))
        probs[int(b)].append(float(p))
    return polygons, probs, result["image_status"].cpu().tolist()
