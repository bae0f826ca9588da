"""The *_workspace_bytes entries of the polygon stages and of the pillar stem against byte counts recorded from a build of the commit BEFORE their layouts
moved onto P3Carve (csrc/p3_common.h): a layout function states each section once, and these tables hold it to the sizes callers already allocate.
Per entry: the degenerate tuples (0, or the N = 0 case of asm_plan), the smallest valid one, an odd-sized one, the shape of the chunk-boundary GPU test and
the bench shape (64 images of 224 x 224 or its equivalent)."""
from ctypes import byref

import pytest

RECORDED = {
    "p3_init_contours_workspace_bytes": [((1, 1, 5), 0), ((0, 8, 8), 0), ((1, 2, 2), 3584), ((3, 33, 21), 287488), ((1025, 2, 2), 290304),
                                         ((64, 224, 224), 460115968)],
    "p3_corner_split_workspace_bytes": [((0, 3), 0), ((10, 0), 0), ((1, 1), 3328), ((1001, 7), 50432), ((4100, 1025), 367872), ((266240, 4096), 13201920)],
    "p3_skeleton_from_contours_workspace_bytes": [((0,), 0), ((-3,), 0), ((1,), 1280), ((77,), 2560), ((1025,), 21760), ((4096,), 81920)],
    "p3_asm_plan_workspace_bytes": [((0, 0), 512), ((-1, -1), 512), ((1, 1), 4096), ((77, 91), 9472), ((4097, 4097), 348160), ((262144, 266240), 22200832)],
    "p3_hisup_polygons_workspace_bytes": [((0, 8, 8, 4, 100), 0), ((2, 8, 8, 4, 0), 0), ((1, 1, 1, 1, 1), 2304), ((3, 37, 29, 7, 501), 437248),
                                          ((3, 8, 8, 400, 4800), 187136), ((64, 224, 224, 64, 65536), 59080960),
                                          ((2, 4096, 1024, 2, 1000), 302292992)],          # the last one: slabs capped at 1 GiB
    "p3_hisup_polygons_rings_workspace_bytes": [((2, 8, 8, 4, 100, 0, 10), 0), ((2, 8, 8, 4, 100, 10, 0), 0), ((1, 1, 1, 1, 1, 1, 1), 4608),
                                                ((3, 37, 29, 7, 501, 5, 203), 441856), ((3, 8, 8, 400, 4800, 1200, 4800), 302848),
                                                ((64, 224, 224, 64, 65536, 4096, 65536), 60064000)],
    "p3_ffl_polygons_workspace_bytes": [((-1, 2), 0), ((10, 0), 0), ((0, 1), 5376), ((1001, 3), 640768), ((0, 1025), 1316096), ((262144, 64), 166019840)],
}
# (B, total_points, nx, ny, max_points, max_voxels, C) per dtype
PILLAR = [((3, 7001, 28, 27, 32, 333, 128), {"BF16": 4564480, "F32X3": 7636480}), ((64, 192000, 56, 56, 32, 784, 384), {"BF16": 390719232, "F32X3": 607708928})]


@pytest.mark.parametrize("entry", sorted(RECORDED))
def test_polygon_stage_workspaces_keep_their_recorded_sizes(entry):
    from pixelspointspolygons_amd._lib import lib
    assert len(RECORDED[entry]) >= 4
    for args, nbytes in RECORDED[entry]:
        assert getattr(lib(), entry)(*args) == nbytes, (entry, args)


@pytest.mark.parametrize("dtype", ["BF16", "F32X3"])
def test_pillar_stem_workspace_keeps_its_recorded_sizes(dtype):
    from pixelspointspolygons_amd import hip
    for (B, total, nx, ny, max_points, max_voxels, C), nbytes in PILLAR:
        d = hip.PillarDesc()
        d.B, d.total_points, d.nx, d.ny = B, total, nx, ny
        d.vx, d.vy, d.vz, d.zmax = 0.5, 0.5, 8.0, 8.0
        d.max_points, d.max_voxels, d.C = max_points, max_voxels, C
        d.training, d.bn_eps, d.bn_momentum = 1, 1e-3, 0.01
        d.dtype, d.out_ld, d.out_col_off, d.no_backward = getattr(hip, dtype), C, 0, 0
        assert hip.lib().p3_pillar_stem_workspace_bytes(byref(d)) == nbytes[dtype], (dtype, B, total, C)
