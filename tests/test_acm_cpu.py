"""The FFL active-contour optimiser, the parts that need no GPU: the contour container against the reference's own (tests/golden/acm.npz, written by
tests/golden/make_acm_golden.py from the reference's polygonize_acm.py / tensorpoly.py), the learning-rate schedule against the reference's LambdaLR, the
torch restatement the GPU tests compare with (tests/acm_ref.py) against the reference's positions and losses after 1 and 5 steps, what the reference's fp32
run differs from its own float64 run by (the yardstick of the GPU tolerances), and the C-ABI entry."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import acm_ref as R
from tests.helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "p3hip.h")


@pytest.fixture(scope="module")
def gold():
    return load_golden("acm.npz")[0]


def test_container_fields_equal_the_reference_and_round_trip(gold):
    from pixelspointspolygons_amd import polygonize_acm as A
    contours = R.contours_of(gold)
    tp = A.contours_batch_to_tensorpoly(contours)
    assert tp.pos.dtype == torch.float32 and torch.equal(tp.pos, gold["tp.pos"])
    assert tp.poly_slice.dtype == torch.long and torch.equal(tp.poly_slice, gold["tp.poly_slice"])
    assert tp.batch.dtype == torch.long and torch.equal(tp.batch, gold["tp.batch"])
    assert tp.is_endpoint.dtype == torch.bool and torch.equal(tp.is_endpoint, gold["tp.is_endpoint"])
    assert tp.batch_size == int(gold["tp.batch_size"]) and tp.num_nodes == gold["tp.pos"].shape[0]
    assert tp.max_len == int((gold["tp.poly_slice"][:, 1] - gold["tp.poly_slice"][:, 0]).max())
    back = A.tensorpoly_to_contours_batch(tp)
    assert [len(c) for c in back] == [len(c) for c in contours]
    for got_img, want_img in zip(back, contours):
        for got, want in zip(got_img, want_img):
            assert got.shape == want.shape and np.array_equal(got, want.astype(np.float32))          # closed ones got their first point back
    assert A.contours_batch_to_tensorpoly([[], []]) is None
    # the restatement's container is the same one
    pos, sl, batch, ep = R.container(contours)
    assert torch.equal(pos.float(), gold["tp.pos"]) and torch.equal(sl, gold["tp.poly_slice"]) and torch.equal(batch, gold["tp.batch"])
    assert torch.equal(ep, gold["tp.is_endpoint"]) and int(ep.sum()) == 4          # two open polylines


def test_schedule_equals_the_reference_lambda_lr(gold):
    from pixelspointspolygons_amd import polygonize_acm as A
    c = A.ACM_DEFAULTS
    lrs = gold["lrs"].numpy()
    assert lrs.shape == (500,) and c["steps"] == 500
    mine = np.array([c["poly_lr"] * A.lr_coef(i, c["warmup_iters"], c["warmup_factor"]) for i in range(500)])
    assert np.array_equal(mine, lrs)
    assert abs(mine[0] / (c["poly_lr"] * c["warmup_factor"]) - 1) < 1e-15 and mine[99] < mine[100] and mine[100] == c["poly_lr"] and A.lr_coef(0, 0, 0.1) == 1
    assert np.array_equal(np.array([R.DEFAULTS["poly_lr"] * R.lr_coef(i, 100, 0.1) for i in range(500)]), lrs)
    for k in ("steps", "data_level", "data_coef", "length_coef", "crossfield_coef", "poly_lr", "warmup_iters", "warmup_factor"):
        assert c[k] == R.DEFAULTS[k], k


@pytest.mark.parametrize("steps", [1, 5])
def test_restatement_fp32_reproduces_the_reference(gold, steps):
    pos, last = R.optimize(gold["tp.pos"], gold["tp.poly_slice"], gold["tp.batch"], gold["tp.is_endpoint"], gold["indicator"], gold["c0c2"], R.DEFAULTS,
                           steps=steps, dtype=torch.float32)
    err = float((pos - gold[f"ref32.pos{steps}"]).abs().max())
    rel = np.abs(np.array(last) / gold[f"ref32.loss{steps}"].numpy() - 1).max()
    print(f"{steps} steps: max |pos - reference| = {err:.3g}, losses rel = {rel:.3g}")
    assert err <= 1e-5 and rel <= 1e-5
    assert float((gold[f"ref32.pos{steps}"] - gold["tp.pos"]).abs().max()) > 1e-3          # the contours did move


def test_restatement_float64_is_the_reference_float64(gold):
    cfg = dict(R.DEFAULTS, poly_lr=1.0, warmup_iters=0)
    pos, _ = R.optimize(gold["tp.pos"], gold["tp.poly_slice"], gold["tp.batch"], gold["tp.is_endpoint"], gold["indicator"], gold["c0c2"], cfg, steps=1)
    assert float((pos - gold["ref64.grad_pos1"]).abs().max()) <= 1e-12


def test_reference_alone_stays_within_half_of_the_gpu_caps(gold):
    """tests/test_acm_gpu.py allows the kernel 0.2 % of vertex comparisons over 1e-4 px, none over 4e-3 and a median of max(4 x this median, 4e-6): the
    reference's fp32 run against its own float64 run, re-synchronised every 5 steps in the same way, must sit well inside that"""
    share, worst, median = gold["alone.traj"].tolist()
    print(f"reference alone: share over 1e-4 = {share:.3g}, worst = {worst:.3g}, median = {median:.3g}; one step at lr 1: {float(gold['alone.grad'][0]):.3g}")
    assert share <= 1e-3 and worst <= 2e-3 and median <= 2e-6          # half of 0.2 %, of 4e-3 and of the 4e-6 floor of the median cap
    assert 0 < float(gold["alone.grad"][0]) < 1e-4
    assert float(gold["margin0"]) > 1e-4          # no vertex or midpoint of the fixture sits on a floor / round / 0.1 decision at step 0


def test_entry_is_declared_exported_and_validates_before_any_device_work():
    from pixelspointspolygons_amd._lib import load
    from pixelspointspolygons_amd.build import build_library
    lib = load(build_library(verbose=False))
    raw = open(HEADER).read()
    assert "polygonize_acm.py:77-220" in raw
    text = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    m = re.search(r"\bint\s+p3_acm_optimize\s*\(([^;{}]*?)\)\s*;", text, flags=re.S)
    assert m and len(m.group(1).split(",")) == 25
    assert hasattr(lib, "p3_acm_optimize") and hasattr(lib, "p3_acm_workspace_bytes")
    f, dbl, n64 = ctypes.c_float, ctypes.c_double, ctypes.c_int64

    def call(N, P, steps, B=1, first_iter=0):
        return lib.p3_acm_optimize(None, n64(N), None, None, P, None, None, None, B, 8, 8, f(0.1), f(0.4), f(0.5), f(0.5), dbl(0.01), 100, dbl(0.1), first_iter,
                                   steps, 0, 0, None, None, None)

    assert call(4, 1, 5) == -1 and b"p3_acm_optimize" in lib.p3_last_error_string()
    assert call(4, 0, 5) == 0 and call(4, 1, 0) == 0 and call(0, 1, 5) == 0          # nothing to do: no launch, no pointer is looked at
    assert call(4, -1, 5) == -2 and call(4, 1, -1) == -2 and call(4, 1, 5, first_iter=-1) == -2
    assert lib.p3_acm_workspace_bytes(n64(100)) == 100 * 20 and lib.p3_acm_workspace_bytes(n64(0)) == 0


def test_wrappers_refuse_host_tensors_and_the_dist_term(gold):
    from pixelspointspolygons_amd import hip, polygonize_acm as A
    tp = A.contours_batch_to_tensorpoly(R.contours_of(gold))
    with pytest.raises(hip.P3Error):
        hip.acm_optimize(tp.pos, tp.poly_slice, tp.batch, tp.is_endpoint, gold["indicator"], gold["c0c2"], 0.1, 0.4, 0.5)
    with pytest.raises(hip.P3Error):
        A.TensorPolyOptimizer(A.ACM_DEFAULTS, tp, gold["indicator"], gold["c0c2"], 0.1, 0.4, 0.5)
    with pytest.raises(hip.P3Error):
        A.optimize_contours(torch.zeros(2, 1, 32, 40), gold["c0c2"], R.contours_of(gold))
    with pytest.raises(NotImplementedError):
        A.TensorPolyOptimizer(A.ACM_DEFAULTS, tp, gold["indicator"], gold["c0c2"], 0.1, 0.4, 0.5, dist=gold["indicator"], dist_coef=0.1)
