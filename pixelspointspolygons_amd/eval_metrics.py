"""Polygon metrics on the device: the figures of the reference's `Evaluator.evaluate` that depend only on the predicted and the ground-truth polygons and
the image size - IoU, C-IoU and NR (eval/cIoU.py) and POLIS, chamfer and Hausdorff (eval/polis_chamfer_hausdorff.py, IoU threshold 0.5, sampling distance
0.1) - from packed rings to the six means in p3_polygon_metrics (csrc/poly_metrics.hip; the definition is in include/p3hip.h and DESIGN.md section 21).

A ring set is a dict(pos fp32 [V,2] in (x, y) order, ring_slice int64 [R,2], ring_image int32 [R] non-decreasing, batch_size): open exterior rings.
`pack_rings` builds one from per-image lists; `rings_from_ffl`, `rings_from_hisup` and `rings_from_pix2poly` build one from what the three models return.
`polygon_metrics(pred, gt, height, width)` scores a batch with one read-back.  There is no CPU path: host tensors raise hip.P3Error.

`coco_metrics(pred, gt, height, width)` gives the reference's COCO columns - AP, AP50, AP75, AP and AR by size, AR at 1, 10 and 100 detections
(Evaluator.compute_coco_metrics) and the same on the boundaries of the masks (compute_boundary_coco_metrics) - from p3_coco_metrics (csrc/coco_metrics.hip,
DESIGN.md section 22), with one read-back.  For it a ring set may carry "score" (predictions, fp32 [R]; missing: every score 1.0, which is what the
reference's annotation writer puts) and "area" (ground truth, fp32 [R]: the annotation's area for the size buckets; missing: the ring's pixel count).

`max_tangent_angle(pred, gt, height, width)` gives the reference's "MTA" column - the mean max tangent angle error of eval/angle_eval.py, in degrees -
from p3_max_tangent_angle (csrc/mta_metrics.hip), with one read-back.  A "score" or "area" field of a ring set is ignored.

`mask_metrics(pred, gt, height, width)` gives the reference's modes "topdig" (eval/topdig_metrics.py: IoU, pixel accuracy and F1 of the filled masks and
of the outlines stroked 5 pixels thick), "subset_iou" (compute_IoU_cIoU(subset=True)) and "stats" (compute_coco_stats) from p3_mask_metrics
(csrc/mask_metrics.hip), with one read-back.  `evaluate(pred, gt, height, width, modes)` takes the reference's
cfg.evaluation.modes and makes at most four such calls.

Host synchronisations: `polygon_metrics`, `coco_metrics`, `max_tangent_angle` and `mask_metrics` have one each, the read-back; `evaluate` has one per call it makes.  `rings_from_ffl` and `rings_from_hisup` (device dict) each select the kept rings with a
boolean mask, which makes torch read the number of kept rings back once per indexed tensor (two per call); no coordinate, slice or flag reaches the host.
`pack_rings` and `rings_from_pix2poly` start from host lists and upload."""
import numpy as np
import torch

from . import hip

MODES = {"iou": hip.PM_IOU, "polis": hip.PM_POLIS, "chamfer": hip.PM_SAMPLES, "hausdorff": hip.PM_SAMPLES}
KEYS = ("IoU", "C-IoU", "NR", "POLIS", "chamfer", "hausdorff")
IOU_TYPES = {"segm": hip.COCO_SEGM, "boundary": hip.COCO_BOUNDARY}
MASK_MODES = {"topdig": hip.MM_TOPDIG, "subset_iou": hip.MM_SUBSET, "stats": hip.MM_STATS}
MASK_KEYS = ("IoU_", "P-Acc", "F1-Score", "IoU-Topo", "P-Acc-Topo", "F1-Score-Topo", "sIoU", "sC-IoU", "sNR")
STATS_KEYS = ("#images", "GT #images w/ polys", "Pred #images w/ polys", "GT #polygons", "Pred #polygons", "GT #vertices", "Pred #vertices")
EVALUATE_MODES = ("iou", "polis", "chamfer", "hausdorff", "topdig", "subset_iou", "stats", "mta", "coco", "boundary-coco", "ldof")
COCO_KEYS = ("AP", "AP50", "AP75", "AP_small", "AP_medium", "AP_large", "AR1", "AR10", "AR100", "AR_small", "AR_medium", "AR_large")


def _per_ring(values, polygons_batch, name):
    """per image a list of one number per ring -> float32 [R]"""
    flat = [float(v) for per_image in values for v in per_image]
    if len(values) != len(polygons_batch) or [len(v) for v in values] != [len(p) for p in polygons_batch]:
        raise hip.P3Error(f"pack_rings: {name} must hold one number per ring, image by image")
    return torch.tensor(flat, dtype=torch.float32)


def pack_rings(polygons_batch, device, scores=None, areas=None):
    """per image a list of [n, 2] (x, y) arrays (numpy, torch or nested lists) -> ring set on `device`.  A closing duplicate of the first vertex is dropped;
    rings keep their order, images too.  One upload per field (polygon_metrics refuses a ring set packed onto the host).  scores / areas: per image a list
    of one number per ring -> the "score" / "area" field (coco_metrics)."""
    pos, sl, img, at = [], [], [], 0
    for b, polygons in enumerate(polygons_batch):
        for poly in polygons:
            p = poly.detach().cpu().numpy() if torch.is_tensor(poly) else np.asarray(poly)
            p = p.astype(np.float32).reshape(-1, 2)
            if len(p) > 1 and np.array_equal(p[0], p[-1]):
                p = p[:-1]
            pos.append(p)
            sl.append((at, at + len(p)))
            img.append(b)
            at += len(p)
    rings = {"pos": torch.from_numpy(np.concatenate(pos) if pos else np.zeros((0, 2), np.float32)).to(device),
             "ring_slice": torch.tensor(sl, dtype=torch.int64).reshape(-1, 2).to(device), "ring_image": torch.tensor(img, dtype=torch.int32).to(device),
             "batch_size": len(polygons_batch)}
    if scores is not None:
        rings["score"] = _per_ring(scores, polygons_batch, "scores").to(device)
    if areas is not None:
        rings["area"] = _per_ring(areas, polygons_batch, "areas").to(device)
    return rings


def _open_rings(pos, ring_slice):
    """closed rings (first vertex again at the end) -> the same slices without the closing vertex, on the device"""
    first, last = ring_slice[:, 0], ring_slice[:, 1] - 1
    n = ring_slice[:, 1] - ring_slice[:, 0]
    safe = pos.shape[0] - 1
    closed = (n > 1) & (pos[first.clamp(0, safe)] == pos[last.clamp(0, safe)]).all(dim=1) if pos.shape[0] else torch.zeros_like(n, dtype=torch.bool)
    return torch.stack([ring_slice[:, 0], ring_slice[:, 1] - closed.to(ring_slice.dtype)], dim=1)


def rings_from_ffl(result, unit_scores=False):
    """the dict of polygonize_post.polygons_from_pieces / polygonize_acm_polygons / polygonize_asm_polygons -> ring set: the shells of the polygons no
    filter flagged (poly_flags == 0), (row, col) flipped to (x, y), the closing vertex dropped.  The coordinates stay on the device; selecting the kept
    polygons by a boolean mask synchronises with the host twice (poly_rings[keep], poly_batch[keep]: torch reads the number of kept polygons).  "score" is
    the kept polygons' poly_prob (torch sizes that selection from the count it already read); unit_scores=True leaves it out, so that every score is 1.0 as
    in the reference's protocol."""
    if "ring_pos" not in result:
        raise hip.P3Error("rings_from_ffl: one polygon dict expected (pick a tolerance of a 'tol_{}' dict first)")
    hip._dev(result["ring_pos"])
    keep = result["poly_flags"] == 0
    shell = result["poly_rings"][keep][:, 0]
    pos = result["ring_pos"].flip(1).contiguous()
    rings = {"pos": pos, "ring_slice": _open_rings(pos, result["ring_slice"][shell]), "ring_image": result["poly_batch"][keep].to(torch.int32),
             "batch_size": int(result["batch_size"])}
    if not unit_scores and "poly_prob" in result:
        rings["score"] = result["poly_prob"][keep].to(torch.float32)
    return rings


def rings_from_hisup(output, device=None, unit_scores=False):
    """the output of HiSup `forward_val_device(polygons=True)` (device dict output["polygons"]: pos (x, y), poly_slice [B,R,2], poly_flags [B,R]; regions'
    n_regions [B]) -> ring set of the outer polygons that exist (poly_flags bit 2 clear), the closing vertex dropped, without a copy of the coordinates.
    Selecting those polygons by a boolean mask synchronises with the host twice (poly_slice[keep], image[keep]: torch reads their number).
    The host form of `forward_val(polygons=True)` (`polys_pred`, with `poly_parts` when inner rings were built) is packed onto `device`.
    "score" is the region score of the device dict (regions' score [B,R]) where it is there; unit_scores=True leaves it out, so that every score is 1.0 as in
    the reference's protocol.  The host lists carry no score per polygon."""
    if "polygons" in output:
        pg, n_regions = output["polygons"], output["regions"]["n_regions"]
        hip._dev(pg["pos"])
        B, R = pg["poly_flags"].shape
        keep = (torch.arange(R, device=n_regions.device)[None, :] < n_regions[:, None]) & ((pg["poly_flags"] & 4) == 0)
        image = torch.arange(B, device=n_regions.device, dtype=torch.int32)[:, None].expand(B, R)
        rings = {"pos": pg["pos"], "ring_slice": _open_rings(pg["pos"], pg["poly_slice"][keep]), "ring_image": image[keep], "batch_size": B}
        if not unit_scores and "score" in output["regions"]:
            rings["score"] = output["regions"]["score"][keep].to(torch.float32)
        return rings
    if "polys_pred" not in output:
        raise hip.P3Error("rings_from_hisup: the output of forward_val_device(polygons=True) or of forward_val(polygons=True) expected")
    if device is None:
        raise hip.P3Error("rings_from_hisup: the host lists of forward_val need the device to pack them onto (there is no CPU path)")
    parts = output.get("poly_parts")
    outer = [[p[:parts[b][i][0]] if parts is not None else p for i, p in enumerate(polys)] for b, polys in enumerate(output["polys_pred"])]
    return pack_rings(outer, device)


def rings_from_pix2poly(polygons, device, unit_scores=False):
    """the per-tile lists of [n, 2] (x, y) tensors `postprocess.batch_to_polygons` returns (host tensors: the permutation decoding ends there) -> ring set.
    The decoder gives no score per polygon, so the set carries none and every score is 1.0 with or without unit_scores (the keyword of the other two)."""
    return pack_rings(polygons, device)


def _fields(rings, name, who="polygon_metrics"):
    try:
        return rings["pos"], rings["ring_slice"], rings["ring_image"], int(rings["batch_size"])
    except (KeyError, TypeError, IndexError):
        raise hip.P3Error(f"{who}: {name} is not a ring set (pos, ring_slice, ring_image, batch_size): see pack_rings") from None


def polygon_metrics(pred, gt, height, width, modes=("iou", "polis", "chamfer", "hausdorff"), out=None):
    """pred, gt: ring sets of the same batch.  -> dict with the reference's keys "IoU", "C-IoU", "NR", "POLIS", "chamfer", "hausdorff" as Python floats (NaN
    for a mode left out, and for the last three when no image has a counted pair), "status" (int; bit 0 an invalid ring, bit 1 a ring left out), and the
    device tensors "per_image" (iou, nr, polis, chamfer, hausdorff, valid, counts = (I, U), invalid_rings) and "pairs" (match, polis, chamfer, hausdorff
    per gt ring).  One read-back: the six means and the status."""
    dp, ds, di, B = _fields(pred, "pred")
    gp, gs, gi, Bg = _fields(gt, "gt")
    if B != Bg:
        raise hip.P3Error(f"polygon_metrics: pred holds {B} images, gt {Bg}")
    bits = 0
    for m in modes:
        if m not in MODES:
            raise hip.P3Error(f"polygon_metrics: unknown mode {m!r}; the modes are {sorted(MODES)}")
        bits |= MODES[m]
    o = hip.polygon_metrics_device(gp, gs, gi, dp, ds, di, B, height, width, bits, out=out)
    *means, status = torch.cat([o["metrics"], o["status"].to(torch.float64)]).tolist()
    res = dict(zip(KEYS, means))
    res["status"] = int(status)
    res["per_image"] = {"iou": o["image_iou"], "nr": o["image_nr"], "polis": o["image_polis"], "chamfer": o["image_chamfer"],
                        "hausdorff": o["image_hausdorff"], "valid": o["image_valid"], "counts": o["image_counts"], "invalid_rings": o["invalid_rings"]}
    res["pairs"] = {"match": o["match"], "polis": o["pair_polis"], "chamfer": o["pair_chamfer"], "hausdorff": o["pair_hausdorff"]}
    return res


def coco_metrics(pred, gt, height, width, iou_types=("segm", "boundary"), out=None):
    """pred, gt: ring sets of the same batch; pred may carry "score", gt "area".  -> dict with the reference's keys "AP", "AP50", "AP75", "AP_small",
    "AP_medium", "AP_large", "AR1", "AR10", "AR100", "AR_small", "AR_medium", "AR_large" as Python floats for the instance masks, the same keys under
    "boundary" for boundary IoU (NaN for a type left out, -1 where COCO has no entry to average), "status" (int; bit 0 an invalid ring, bit 1 a ring left
    out), and the device tensors "tables" (stats, precision, recall) and "pairs" (gt_area_px, dt_area_px, gt_boundary_px, dt_boundary_px, dt_rank,
    pair_inter, dt_match, dt_ignore, gt_match).  One read-back: the 24 stats and the status."""
    dp, ds, di, B = _fields(pred, "pred", "coco_metrics")
    gp, gs, gi, Bg = _fields(gt, "gt", "coco_metrics")
    if B != Bg:
        raise hip.P3Error(f"coco_metrics: pred holds {B} images, gt {Bg}")
    bits = 0
    for t in iou_types:
        if t not in IOU_TYPES:
            raise hip.P3Error(f"coco_metrics: unknown iou type {t!r}; the types are {sorted(IOU_TYPES)}")
        bits |= IOU_TYPES[t]
    if not bits:
        raise hip.P3Error(f"coco_metrics: iou_types is empty; the types are {sorted(IOU_TYPES)}")
    o = hip.coco_metrics_device(gp, gs, gi, dp, ds, di, B, height, width, bits, dt_score=pred.get("score"), gt_area=gt.get("area"), out=out)
    *stats, status = torch.cat([o["stats"].reshape(-1), o["status"].to(torch.float64)]).tolist()
    res = dict(zip(COCO_KEYS, stats[:12]))
    res["boundary"] = dict(zip(COCO_KEYS, stats[12:]))
    res["status"] = int(status)
    res["tables"] = {k: o[k] for k in ("stats", "precision", "recall")}
    res["pairs"] = {k: o[k] for k in ("gt_area_px", "dt_area_px", "gt_boundary_px", "dt_boundary_px", "dt_rank", "pair_inter", "dt_match", "dt_ignore",
                                      "gt_match")}
    return res


def max_tangent_angle(pred, gt, height, width, sampling_spacing=2.0, min_precision=0.5, max_stretch=2.0, out=None):
    """pred, gt: ring sets of the same batch (a "score" or "area" field is ignored).  -> dict with the reference's key "MTA" as a Python float in degrees
    (NaN when no ring is counted), "counted" (int: the rings the mean runs over), "status" (int; bit 0 an invalid ring, bit 1 a ring left out, bit 2
    predictions of an image overlap: the reference would have merged them), and the device tensors "per_ring" (angle in radians, cos, state = hip.MTA_*,
    px = (A, I)) and "per_image" (overlap_px, invalid_rings).  The defaults are the reference's.  One read-back: MTA, counted and status together."""
    dp, ds, di, B = _fields(pred, "pred", "max_tangent_angle")
    gp, gs, gi, Bg = _fields(gt, "gt", "max_tangent_angle")
    if B != Bg:
        raise hip.P3Error(f"max_tangent_angle: pred holds {B} images, gt {Bg}")
    o = hip.max_tangent_angle_device(gp, gs, gi, dp, ds, di, B, height, width, sampling_spacing, min_precision, max_stretch, out=out)
    mta, counted, status = torch.cat([o["mta"], o["counted"].to(torch.float64), o["status"].to(torch.float64)]).tolist()
    return {"MTA": mta, "counted": int(counted), "status": int(status),
            "per_ring": {"angle": o["ring_angle"], "cos": o["ring_cos"], "state": o["ring_state"], "px": o["ring_px"]},
            "per_image": {"overlap_px": o["image_overlap_px"], "invalid_rings": o["invalid_rings"]}}


def mask_metrics(pred, gt, height, width, modes=("topdig", "subset_iou", "stats"), buffer_thickness=5, out=None):
    """pred, gt: ring sets of the same batch (a "score" or "area" field is ignored).  -> dict with the reference's keys "IoU_", "P-Acc", "F1-Score",
    "IoU-Topo", "P-Acc-Topo", "F1-Score-Topo" (topdig) and "sIoU", "sC-IoU", "sNR" (subset_iou; NaN when no image has a prediction) as Python floats, NaN
    for a mode left out; "#images", "GT #images w/ polys", "Pred #images w/ polys", "GT #polygons", "Pred #polygons", "GT #vertices", "Pred #vertices"
    (stats) as ints, 0 when left out; "status" (int; bit 0 an invalid ring, bit 1 a ring left out), and the device tensors "per_image" (conf = (filled,
    stroked) x (TP, FP, FN, TN), scores in the order of the six topdig keys, nr, subset, invalid_rings).  buffer_thickness: the width of the stroked
    outlines, the reference's 5.  One read-back: the nine means, the seven counts and the status."""
    dp, ds, di, B = _fields(pred, "pred", "mask_metrics")
    gp, gs, gi, Bg = _fields(gt, "gt", "mask_metrics")
    if B != Bg:
        raise hip.P3Error(f"mask_metrics: pred holds {B} images, gt {Bg}")
    bits = 0
    for m in modes:
        if m not in MASK_MODES:
            raise hip.P3Error(f"mask_metrics: unknown mode {m!r}; the modes are {sorted(MASK_MODES)}")
        bits |= MASK_MODES[m]
    if not bits:
        raise hip.P3Error(f"mask_metrics: modes is empty; the modes are {sorted(MASK_MODES)}")
    o = hip.mask_metrics_device(gp, gs, gi, dp, ds, di, B, height, width, buffer_thickness, bits, out=out)
    # counts below 2^53 are exact as doubles: that is every ring set whose slices do not overlap
    flat = torch.cat([o["metrics"], o["stats"].to(torch.float64), o["status"].to(torch.float64)]).tolist()
    res = dict(zip(MASK_KEYS, flat[:9]))
    res.update(zip(STATS_KEYS, (int(v) for v in flat[9:16])))
    res["status"] = int(flat[16])
    res["per_image"] = {"conf": o["image_conf"], "scores": o["image_scores"], "nr": o["image_nr"], "subset": o["image_subset"],
                        "invalid_rings": o["invalid_rings"]}
    return res


def evaluate(pred, gt, height, width, modes):
    """the polygon-only part of the reference's Evaluator.evaluate: modes with the reference's names (cfg.evaluation.modes), grouped into at most four
    calls - polygon_metrics for "iou", "polis", "chamfer", "hausdorff"; mask_metrics for "topdig", "subset_iou", "stats"; max_tangent_angle for "mta";
    coco_metrics for "coco", "boundary-coco" - each with its defaults.  -> dict with the reference's keys of the modes asked for merged into one (the
    boundary table under "boundary", as coco_metrics returns it), "status": the statuses ORed, and "calls": function name -> that call's full result.  One
    read-back per call made.  "ldof" needs the reference's external executable and raises."""
    modes = list(modes)
    for m in modes:
        if m not in EVALUATE_MODES:
            raise hip.P3Error(f"evaluate: unknown mode {m!r}; the modes are {list(EVALUATE_MODES)}")
    if "ldof" in modes:
        raise hip.P3Error("evaluate: the mode 'ldof' needs the reference's external executable (its ldof binary) and has no device path")
    if not modes:
        raise hip.P3Error(f"evaluate: modes is empty; the modes are {list(EVALUATE_MODES)}")
    res, calls, status = {}, {}, 0
    pm = [m for m in modes if m in MODES]
    if pm:
        c = calls["polygon_metrics"] = polygon_metrics(pred, gt, height, width, modes=pm)
        if "iou" in pm:
            res.update({k: c[k] for k in KEYS[:3]})
        res.update({k: c[k] for k in KEYS[3:] if k.lower() in pm})
    mm = [m for m in modes if m in MASK_MODES]
    if mm:
        c = calls["mask_metrics"] = mask_metrics(pred, gt, height, width, modes=mm)
        for m, keys in (("topdig", MASK_KEYS[:6]), ("subset_iou", MASK_KEYS[6:]), ("stats", STATS_KEYS)):
            if m in mm:
                res.update({k: c[k] for k in keys})
    if "mta" in modes:
        c = calls["max_tangent_angle"] = max_tangent_angle(pred, gt, height, width)
        res["MTA"] = c["MTA"]
    types = [t for m, t in (("coco", "segm"), ("boundary-coco", "boundary")) if m in modes]
    if types:
        c = calls["coco_metrics"] = coco_metrics(pred, gt, height, width, iou_types=types)
        if "coco" in modes:
            res.update({k: c[k] for k in COCO_KEYS})
        if "boundary-coco" in modes:
            res["boundary"] = c["boundary"]
    for c in calls.values():
        status |= c["status"]
    res["status"] = status
    res["calls"] = calls
    return res
