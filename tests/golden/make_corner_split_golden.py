"""Golden vectors for the corner-aware contour simplification (p3_corner_split): the reference's own `compute_crossfield_uv` (lydorn_utils/math_utils.py:140),
`detect_corners` (models/ffl/frame_field_utils.py:71-114) and `split_polylines_corner` (predict/ffl/polygonize_utils.py:47-61), loaded by file path and run on
the CPU on the stage-A output of the float64 restatement (tests/corner_split_ref.py).  Build-container only (imports the reference); emits
tests/golden/corner_split.npz (arrays only).  skimage / shapely / cv2 / sklearn / scipy.stats are stubs: nothing of them runs in these three functions.
Douglas-Peucker itself (skimage's approximate_polygon, GEOS's simplify) is installed nowhere here and is NOT pinned by this file.

Scene: B = 3, 32 x 40, image 2 empty.  A smooth rotated frame field per image; noisy rectangle and ellipse rings, L- and T-shaped outlines whose long sides
carry bends of 15 - 30 degrees (they survive stage A and are no corners), open lines, a zigzag whose apexes lie outside the map (the pixel clip acts), every
size from 0 to 5 explicit points open and closed; and the ASM form on the paths of tests/golden/asm.npz (two junction graphs) with jittered positions.

The generator ASSERTS, for every configuration the tests run and with no decision left out, that every Douglas-Peucker margin (|largest distance - tol| of
a section, gap between the two largest distances of a splitting section; exact ties apart) is >= 1e-4 px and every corner margin >= 1e-3, and draws the
next seed otherwise.  The margins are stored."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_acm_golden as G  # noqa: E402
import corner_split_ref as R  # noqa: E402

REF = G.REF
B, H, W = 3, 32, 40
ACM_TOLS = (0.125, 0.3, 1.0)          # tolerance of the ACM form: stage A at min(1, tolerance), stage D at tolerance
DP_MARGIN, CORNER_MARGIN = 1e-4, 1e-3


def load_reference():
    for name in ("skimage", "shapely", "sklearn", "lydorn_utils", "torch_lydorn", "torch_lydorn.torch", "torch_lydorn.torch.utils", "pixelspointspolygons",
                 "pixelspointspolygons.models", "pixelspointspolygons.models.ffl", "pixelspointspolygons.predict", "pixelspointspolygons.predict.ffl"):
        G._stub(name, pkg=True)
    for name in ("skimage.measure", "skimage.transform", "shapely.geometry", "shapely.ops", "shapely.affinity", "cv2", "sklearn.datasets",
                 "lydorn_utils.print_utils", "lydorn_utils.image_utils"):
        G._stub(name)
    try:
        import scipy.stats  # noqa: F401
    except ImportError:
        G._stub("scipy", pkg=True)
        G._stub("scipy.stats")
    G._stub("lydorn_utils.python_utils").module_exists = lambda name: False
    G._load("torch_lydorn.torch.utils.complex", G.LYDORN + "/torch/utils/complex.py")
    mu = G._load("lydorn_utils.math_utils", REF + "/ffl_submodules/lydorn_utils/lydorn_utils/math_utils.py")
    ffu = G._load("pixelspointspolygons.models.ffl.frame_field_utils", REF + "/pixelspointspolygons/models/ffl/frame_field_utils.py")
    pu = G._load("pixelspointspolygons.predict.ffl.polygonize_utils", REF + "/pixelspointspolygons/predict/ffl/polygonize_utils.py")
    return mu.compute_crossfield_uv, ffu.detect_corners, pu.split_polylines_corner


def _outline(corners, step=1.0):
    """closed outline through `corners` (local coordinates) in ~step px steps, the first point not repeated"""
    pts = []
    for p0, p1 in zip(corners, np.roll(corners, -1, axis=0)):
        k = max(int(round(np.linalg.norm(p1 - p0) / step)), 1)
        pts += [p0 + (p1 - p0) * t / k for t in range(k)]
    return np.array(pts)


def _place(local, centre, ang):
    """local (along, across) -> (row, col): `along` points in direction (sin ang, cos ang) of the (row, col) plane"""
    a, b = local[:, 0], local[:, 1]
    return np.stack([centre[0] + a * np.sin(ang) + b * np.cos(ang), centre[1] + a * np.cos(ang) - b * np.sin(ang)], 1)


def scene(seed):
    """-> c0c2 fp32 [B,4,H,W], pos fp32 [N,2], slices int64 [P,2], closed uint8 [P], poly_batch int32 [P]"""
    rng = np.random.default_rng(seed)
    rr, cc = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    angs = (0.3, -0.5, 0.1)
    cf = []
    for ang in angs:
        theta = ang + 0.08 * np.sin(cc / 9) + 0.05 * np.cos(rr / 7)          # smooth: no noise, neighbouring pixels agree
        w = np.sin(theta) + 1j * np.cos(theta)                                # the `along` direction as row + i col
        c0 = -w ** 4
        c2 = 0.03 * np.sin(rr / 5) + 0.03j * np.cos(cc / 6)
        cf.append(np.stack([c0.real, c0.imag, c2.real, c2.imag]))
    polys = []          # (image, points, closed)
    noisy = lambda p, s: p + rng.normal(0, s, p.shape)
    ell = lambda a, b, k: np.stack([a * np.cos(np.arange(k) * 2 * np.pi / k), b * np.sin(np.arange(k) * 2 * np.pi / k)], 1)
    # image 0
    a0 = angs[0]
    rect = _outline(np.array([(-9.0, -5.0), (9.0, -5.0), (9.0, 5.0), (-9.0, 5.0)]))
    polys.append((0, noisy(_place(rect, (12.0, 14.0), a0), 0.12), 1))
    polys.append((0, noisy(_place(ell(5.0, 3.0, 22), (25.0, 30.0), a0), 0.15), 1))
    bend = np.tan(np.deg2rad(20.0)) * 6.0          # an L whose long sides bend by 20 degrees in their middle
    ell_shape = _outline(np.array([(-7.0, -6.0), (-1.0, -6.0 - bend), (6.0, -6.0), (6.0, -1.0), (0.0, -1.0), (0.0, 6.0), (-7.0, 6.0), (-7.0 - bend, 0.0)]))
    polys.append((0, noisy(_place(ell_shape, (20.0, 27.0), a0), 0.05), 1))
    zig = np.array([(3.0, 2.0), (-0.8, 10.0), (3.0, 18.0), (-0.7, 26.0), (3.0, 34.0), (8.0, 39.8), (14.0, 36.0)])          # apexes outside the map
    zz = np.concatenate([np.linspace(p0, p1, 6, endpoint=False) for p0, p1 in zip(zig[:-1], zig[1:])] + [zig[-1:]])
    polys.append((0, zz + np.where(np.isin(np.arange(len(zz)) % 6, [0]), 0.0, 1.0)[:, None] * rng.normal(0, 0.05, zz.shape), 0))
    # image 1
    a1 = angs[1]
    polys.append((1, noisy(_place(ell(9.0, 6.0, 40), (15.0, 20.0), a1), 0.2), 1))
    polys.append((1, noisy(_place(ell(4.0, 2.5, 16), (6.0, 33.0), a1), 0.15), 1))
    b30 = np.tan(np.deg2rad(15.0)) * 5.0          # a T; the bar's top side bends by 2 x 15 = 30 degrees
    tee = _outline(np.array([(-8.0, -4.0), (0.0, -4.0 - b30), (8.0, -4.0), (8.0, -1.0), (1.5, -1.0), (1.5, 7.0), (-1.5, 7.0), (-1.5, -1.0), (-8.0, -1.0)]))
    polys.append((1, noisy(_place(tee, (22.0, 12.0), a1), 0.05), 1))
    t = np.linspace(0, 1, 30)[:, None]
    line = np.array([0.0, 6.3]) * (1 - t) + np.array([24.4, W - 1.0]) * t
    line[1:-1] += rng.normal(0, 0.25, (28, 2))
    polys.append((1, line, 0))
    for k in (0, 1, 2, 3, 4, 5):          # tiny polylines, open (k explicit points) and closed (k + 1)
        base = np.array([4.0 + 4 * (k % 3), 3.0 + 2 * k])
        pts = base + np.cumsum(rng.normal(0, 1.2, (k, 2)), axis=0) if k else np.zeros((0, 2))
        polys.append((1, pts, 0))
        if k:
            polys.append((1, pts + np.array([12.0, 1.0]), 1))
    pos = np.concatenate([p for _, p, _ in polys]).astype(np.float32)
    ends = np.cumsum([len(p) for _, p, _ in polys])
    slices = np.stack([ends - np.array([len(p) for _, p, _ in polys]), ends], 1).astype(np.int64)
    return (np.stack(cf).astype(np.float32), pos, slices, np.array([c for _, _, c in polys], dtype=np.uint8),
            np.array([b for b, _, _ in polys], dtype=np.int32))


def stage_a(pos, index, slices, closed, tol_pre, margins):
    out = []
    for i in range(len(slices)):
        q = R.explicit_points(pos, index, slices[i], bool(closed[i])).astype(np.float64)
        out.append(q[R.dp(q, tol_pre, margins)] if len(q) >= 2 else None)
    return out


def reference_masks_pieces(fns, polylines, poly_batch, c0c2):
    """the reference's functions, one polyline at a time so that one that raises is known -> masks, pieces per polyline (None: < 2 points or raised)"""
    uv, detect, split = fns
    fields = [uv(np.ascontiguousarray(np.moveaxis(c0c2[b].astype(np.float64), 0, -1))) for b in range(c0c2.shape[0])]
    masks, pieces, raised = [], [], 0
    for q, b in zip(polylines, poly_batch):
        if q is None:
            masks.append(None); pieces.append(None)
            continue
        try:
            m = detect([q], *fields[int(b)])
            masks.append(np.asarray(m[0], dtype=bool))
            pieces.append([np.asarray(p, dtype=np.float64) for p in split([q], m)])
        except Exception as exc:          # noqa: BLE001
            print("  the reference raised on a polyline of", len(q), "points:", repr(exc))
            masks.append(None); pieces.append(None)
            raised += 1
    return masks, pieces, raised


def pack(prefix, masks, pieces, out):
    out[prefix + ".mask.len"] = np.array([-1 if m is None else len(m) for m in masks], dtype=np.int64)
    out[prefix + ".mask"] = np.concatenate([m for m in masks if m is not None] + [np.zeros(0, dtype=bool)])
    out[prefix + ".npieces"] = np.array([-1 if p is None else len(p) for p in pieces], dtype=np.int64)
    flat = [x for p in pieces if p is not None for x in p]
    out[prefix + ".piece.len"] = np.array([len(x) for x in flat], dtype=np.int64)
    out[prefix + ".piece.flat"] = np.concatenate(flat + [np.zeros((0, 2))])


def configs(c0c2, pos, slices, closed, poly_batch, asm):
    """(name, pos, index, slices, closed, poly_batch, c0c2, tol_pre, tol) of every configuration the tests run"""
    out = [("acm_%g" % t, pos, None, slices, closed, poly_batch, c0c2, min(1.0, t), t) for t in ACM_TOLS]
    out.append(("acm_pre1_tol0", pos, None, slices, closed, poly_batch, c0c2, 1.0, 0.0))
    out.append(("asm_1",) + asm + (0.0, 1.0))
    return out


def asm_scene(seed):
    d = np.load(os.path.join(HERE, "asm.npz"))
    rng = np.random.default_rng(1000 + seed)
    pos = (d["ref32.pos300"].astype(np.float64) + rng.normal(0, 0.05, d["ref32.pos300"].shape)).astype(np.float32)
    index, delim = d["ts.path_index"].astype(np.int64), d["ts.path_delim"].astype(np.int64)
    slices = np.stack([delim[:-1], delim[1:]], 1)
    poly_batch = d["ts.batch"][index[np.minimum(slices[:, 0], len(index) - 1)]].astype(np.int32)
    return pos, index, slices, np.zeros(len(slices), dtype=np.uint8), poly_batch, d["c0c2"].astype(np.float32)


def main():
    fns = load_reference()
    for seed in range(400):
        c0c2, pos, slices, closed, poly_batch = scene(seed)
        asm = asm_scene(seed)
        ok, summary = True, {}
        for name, p, idx, sl, cl, pb, cf, tol_pre, tol in configs(c0c2, pos, slices, closed, poly_batch, asm):
            mg = R.Margins()
            R.corner_split(p, idx, sl, cl, pb, cf, tol_pre, tol, mg)
            d_tol, d_gap, ties, corner = mg.smallest()
            summary[name] = (d_tol, d_gap, ties, corner)
            if min(d_tol, d_gap) < DP_MARGIN or corner < CORNER_MARGIN:
                ok = False
                break
        if ok:
            break
    else:
        raise SystemExit("no seed meets the margin conditions")
    print("seed", seed)
    out = {"seed": np.array(seed), "c0c2": c0c2, "pos": pos, "slices": slices, "closed": closed, "poly_batch": poly_batch,
           "asm.pos": asm[0], "asm.index": asm[1], "asm.slices": asm[2], "asm.closed": asm[3], "asm.poly_batch": asm[4], "asm.c0c2": asm[5],
           "config.names": np.array([c[0] for c in configs(c0c2, pos, slices, closed, poly_batch, asm)]),
           "config.tols": np.array([c[-2:] for c in configs(c0c2, pos, slices, closed, poly_batch, asm)], dtype=np.float64)}
    total_raised = 0
    for name, p, idx, sl, cl, pb, cf, tol_pre, tol in configs(c0c2, pos, slices, closed, poly_batch, asm):
        mg = R.Margins()
        polylines = stage_a(p, idx, sl, cl, tol_pre, mg)
        masks, pieces, raised = reference_masks_pieces(fns, polylines, pb, cf)
        total_raised += raised
        pack(name, masks, pieces, out)
        out[name + ".margins"] = np.array(summary[name], dtype=np.float64)          # |d - tol|, gap, exact ties, corner
        res = R.corner_split(p, idx, sl, cl, pb, cf, tol_pre, tol)
        nm = sum(int(m.sum()) for m in masks if m is not None)
        print("%-14s explicit %4d  after A %4d  corners %3d  pieces %3d  vertices out %4d | margins: |d - tol| %.2e, gap %.2e, exact ties %d, corner %.2e" % (
            name, res["offsets"][-1], sum(len(q) for q in polylines if q is not None), nm, res["counts"][1], res["counts"][0], *summary[name]))
    print("polylines on which the reference raised:", total_raised)
    path = os.path.join(HERE, "corner_split.npz")
    np.savez_compressed(path, **out)
    print("wrote corner_split.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
