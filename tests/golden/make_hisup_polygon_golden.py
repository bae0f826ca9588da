"""Golden vectors for the HiSup polygon step: the reference's own `get_poly_crowdai` (models/hisup/polygon.py:138-169, with `ext_c_to_poly_coco`,
`diagonal_to_square` and `simple_polygon` behind it) per region of seeded 48 x 48 images.  Build-container only (loads the reference's polygon.py);
emits tests/golden/hisup_polygon.npz (arrays only).

OpenCV is not installed: polygon.py is loaded with a stub `cv2` whose findContours, drawContours and contourArea are the restatement's border follower,
fill and shoelace (tests/hisup_polygon_ref.py).  That pins squaring, junction match, simplification and the control flow to the reference's code; only those
three calls are substituted.  np.int0, which numpy 2 removed, is defined in this process only.

Fixture conditions (asserted below, so that float32 against float64 angles and the last bit of a distance cannot decide anything):
every |t - 10| and |t - 350| >= 0.01 degrees, every |d - 5| >= 1e-6, no hole whose border has an area >= 50 (the reference would add an inner ring)."""
import importlib.util
import os
import sys
import types

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import hisup_polygon_ref as R  # noqa: E402
from _ref_import import REF_ROOT  # noqa: E402

REF = REF_ROOT + "/pixelspointspolygons/models/hisup/polygon.py"
SEEDS = (3, 5, 8, 13, 21, 34)
SIZE = 48


def _contour(pts):
    return np.asarray(pts, dtype=np.int32).reshape(-1, 1, 2)


def _cv2_stub():
    cv2 = types.ModuleType("cv2")
    cv2.RETR_EXTERNAL, cv2.RETR_TREE, cv2.CHAIN_APPROX_NONE = 0, 3, 1

    def findContours(mask, mode, method):
        assert method == cv2.CHAIN_APPROX_NONE
        m = np.asarray(mask) != 0
        contours, hier = [_contour(R.outer_border(m))], [[-1, -1, -1, -1]]
        if mode == cv2.RETR_TREE:
            holes, n = ndimage.label(R.fill(m) & ~m)               # 4-connected background components the region encloses
            for h in range(1, n + 1):
                ring = ndimage.binary_dilation(holes == h, structure=np.ones((3, 3)))      # the hole and the pixels around it: its border runs through these
                contours.append(_contour(R.outer_border(ring)))
                hier.append([-1, -1, -1, 0])
        return contours, np.asarray([hier])

    def drawContours(mask, contours, idx, color=1, thickness=-1):
        assert thickness == -1 and len(contours) == 1
        c = np.asarray(contours[0]).reshape(-1, 2)
        m = np.zeros(mask.shape, bool)
        m[c[:, 1], c[:, 0]] = True
        mask[R.fill(m)] = color
        return mask

    cv2.findContours, cv2.drawContours, cv2.contourArea = findContours, drawContours, lambda c: R.shoelace(np.asarray(c).reshape(-1, 2))
    return cv2


def load_polygon():
    sys.modules["cv2"] = _cv2_stub()
    if not hasattr(np, "int0"):
        np.int0 = lambda a: np.asarray(a).astype(np.intp)
    spec = importlib.util.spec_from_file_location("ref_hisup_polygon", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Prop:
    def __init__(self, mask):
        self.coords = np.argwhere(mask)


def main():
    poly = load_polygon()
    cv2 = sys.modules["cv2"]
    fgs, juncs = [], []
    for seed in SEEDS:
        rs = np.random.RandomState(seed)
        fg = R.random_regions(rs, SIZE)
        fgs.append(fg)
        juncs.append(R.corner_junctions(rs, fg))
    fgs = np.stack(fgs)
    labels, n_regions, _, _ = R.region_inputs(fgs)
    out = {"fg": np.packbits(fgs, axis=None), "shape": np.asarray(fgs.shape), "junc_n": np.asarray([len(j) for j in juncs])}
    out["juncs"] = np.concatenate(juncs).astype(np.float32)
    polys, rows, n_junc, worst_t, worst_d = [], [], 0, np.inf, np.inf
    for b in range(len(SEEDS)):
        mask_pred = fgs[b].astype(np.float32)
        for l in range(1, int(n_regions[b]) + 1):
            M = labels[b] == l
            contours, hierarchy = cv2.findContours(M.astype(np.uint8), cv2.RETR_TREE, cv2.CHAIN_APPROX_NONE)
            for c, h in zip(contours, hierarchy[0]):
                assert h[3] == -1 or cv2.contourArea(c) < 50, "a hole with a border area >= 50: the reference adds an inner ring"
            mine = R.region_polygon(M, juncs[b])
            worst_t, worst_d = min(worst_t, mine["margin_t"]), min(worst_d, mine["margin_d"])
            try:
                got, score, edge_index = poly.get_poly_crowdai(_Prop(M), mask_pred, juncs[b])
                got = np.asarray(got, dtype=np.float64).reshape(-1, 2)
            except IndexError:                                        # simple_polygon keeps nothing: simple_poly[0] raises
                got = np.zeros((0, 2))
            assert len(edge_index) <= 1 if len(got) else True
            n_junc += bool(mine["flags"] & 1)
            rows.append((b, l, len(got)))
            polys.append(got)
    assert worst_t >= 0.01 and worst_d >= 1e-6, (worst_t, worst_d)
    out["rows"] = np.asarray(rows, dtype=np.int64)
    out["polys"] = np.concatenate(polys)
    path = os.path.join(HERE, "hisup_polygon.npz")
    np.savez_compressed(path, **out)
    print(f"wrote hisup_polygon.npz: {os.path.getsize(path)} bytes, {len(rows)} regions, {n_junc} junction polygons, margins t {worst_t:.4f} deg, d {worst_d:.2e}")


if __name__ == "__main__":
    main()
