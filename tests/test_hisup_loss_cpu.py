"""HiSup training losses, the parts that need no GPU: the float64 reference and the analytic restatement of the gradient formulas
(tests/hisup_loss_ref.py) against the reference's own numbers (tests/golden/hisup_loss.npz, written by tests/golden/make_hisup_loss_golden.py), the
shared input generator, the new C-ABI entries, the wrapper's refusals and `HiSupCriterion`'s weights."""
import os
import re

import numpy as np
import pytest
import torch

from tests import hisup_loss_ref as L
from tests.helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "p3hip.h")


def fixture_inputs():
    d, _ = load_golden("hisup_loss.npz")
    inp = dict(pred=[d["pred." + n] for n in L.NAMES], t_jloc=d["t_jloc"], t_joff=d["t_joff"], t_mask=d["t_mask"], t_afm=d["t_afm"])
    return d, inp


# ------------------------------------------------------------------------------------------------ reference, restatement, generator
def test_analytic_gradient_formulas_equal_the_reference_autograd():
    """the formulas of p3hip.h, evaluated in float64, against torch.autograd through the reference's own functions: 1e-12 on every map"""
    d, inp = fixture_inputs()
    assert tuple(d["weights"].tolist()) == L.WEIGHTS
    got = L.analytic_gradients(inp, L.WEIGHTS)
    for n, g in zip(L.NAMES, got):
        assert g.shape == tuple(d["grad." + n].shape)
        err = L.grad_err(torch.from_numpy(g), d["grad." + n])
        assert err <= 1e-12, (n, err)
    # the one factor the reference itself evaluates in float32 (t / w of sigmoid_l1_loss): the exact H * W / c_b the kernel uses differs from it by
    # at most the roundings of two fp32 means and one fp32 division (pairwise sums over <= 224 terms: about 11 roundings of 2^-24)
    exact = L.analytic_gradients(inp, L.WEIGHTS, exact_factor=True)[1]
    assert L.grad_err(torch.from_numpy(exact), d["grad.joff"]) <= 11 * 2.0 ** -24
    # an image without junctions has an all-zero joff gradient, the image without edges a pure sign(afm)
    assert not d["grad.joff"][1].any() and int((d["grad.joff"][2] != 0).sum()) == 2
    assert torch.equal(d["grad.afm"][0], 0.1 / (2 * d["t_jloc"].numel()) * torch.sign(d["pred.afm"][0].double()))


def test_float64_reference_reproduces_the_fixture():
    d, inp = fixture_inputs()
    losses, total, grads = L.reference(inp, L.WEIGHTS)
    assert losses.dtype == torch.float64 and torch.allclose(losses, d["losses"], rtol=1e-12, atol=0)
    assert abs(float(total) - float(d["total"])) <= 1e-12 * abs(float(d["total"]))
    for n, g in zip(L.NAMES, grads):
        assert L.grad_err(g, d["grad." + n]) <= 1e-12, n
    # the upstream gradient multiplies every map
    _, _, g3 = L.reference(inp, L.WEIGHTS, upstream=3.0)
    for a, b in zip(g3, grads):
        assert L.grad_err(a, 3.0 * b) <= 1e-15


def test_generator_draws_what_the_fixture_stores_and_has_the_planted_images():
    d, inp = fixture_inputs()
    B, H, W, seed = L.CASES["fixture"]
    again = L.make_inputs(B, H, W, seed)
    if torch.equal(again["pred"][0], inp["pred"][0]):       # a later torch may draw differently: then only the stored inputs count
        for a, b in zip(again["pred"] + L.targets_of(again), inp["pred"] + L.targets_of(inp)):
            assert torch.equal(a, b)
    for name in ("odd", "small"):
        inp, _ = L.case(name)
        junctions = [int(((inp["t_jloc"][b] == 1) | (inp["t_jloc"][b] == 2)).sum()) for b in range(inp["t_jloc"].shape[0])]
        assert junctions[1] == 0 and junctions[2] == 1 and junctions[0] > 1, junctions
        assert not inp["t_afm"][0].any() and 0.2 < float(inp["t_mask"].mean()) < 0.4
    assert int((L.case("one")[0]["t_jloc"] > 0).sum()) == 1


def test_fp32_torch_stays_well_inside_the_gpu_tolerances():
    """what the GPU test asks of the kernel (2e-6 per gradient map, 1e-5 per loss) is several times what plain fp32 arithmetic needs on these inputs"""
    inp, (l64, _, g64) = L.case("odd")
    l32, _, g32 = L.reference(inp, dtype=torch.float32)
    assert float(((l32.double() - l64).abs() / l64.abs()).max()) <= 1e-6
    for n, a, b in zip(L.NAMES, g32, g64):
        assert L.grad_err(a, b) <= 5e-7, n


# ------------------------------------------------------------------------------------------------ C-ABI
def test_new_entries_are_exported_with_the_declared_arity():
    from pixelspointspolygons_amd._lib import load, prototypes
    from pixelspointspolygons_amd.build import build_library
    lib = load(build_library(verbose=False))
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    arity = {"p3_hisup_train_loss": 36, "p3_hisup_train_loss_workspace_bytes": 3}
    protos = prototypes()
    for name, n in arity.items():
        assert hasattr(lib, name), name
        m = re.search(r"\b" + name + r"\s*\(([^;{}]*?)\)\s*;", text, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == n and len(protos[name][1]) == n, (name, len(m.group(1).split(",")))
    src = open(os.path.join(ROOT, "pixelspointspolygons_amd", "hip.py")).read()
    for name, n in arity.items():                       # the ctypes call sites pass as many arguments
        i = src.index("lib()." + name + "(") + len("lib()." + name + "(")
        depth, j, commas = 1, i, 0
        while depth:
            depth += {"(": 1, ")": -1}.get(src[j], 0)
            commas += src[j] == "," and depth == 1
            j += 1
        assert commas + 1 == n, (name, commas + 1)
    assert lib.p3_hisup_train_loss_workspace_bytes(2, 224, 224) >= 2 * 49 * 6 * 4
    z = 0
    null = [None, z, z, z] * 5 + [None] * 4 + [1, 8, 8] + [None] * 9
    assert len(null) == 36
    assert lib.p3_hisup_train_loss(*null) == -1
    assert b"p3_hisup_train_loss" in lib.p3_last_error_string()


# ------------------------------------------------------------------------------------------------ wrapper and criterion
def _host(B=1, H=8, W=8):
    return [torch.zeros(B, n, H, W) for n in (3, 2, 2, 2, 2)] + [torch.zeros(B, 1, H, W, dtype=torch.long), torch.zeros(B, 2, H, W),
                                                                torch.zeros(B, 1, H, W), torch.zeros(B, 2, H, W)]


def test_wrapper_refuses_host_tensors_and_mismatched_shapes():
    from pixelspointspolygons_amd import hip
    with pytest.raises(hip.P3Error, match="device tensors"):
        hip.hisup_train_loss(*_host(), L.WEIGHTS)
    a = _host()
    a[3] = torch.zeros(1, 2, 8, 9)                       # afm of another width
    with pytest.raises(hip.P3Error, match="share one"):
        hip.hisup_train_loss(*a, L.WEIGHTS)
    a = _host()
    a[6] = torch.zeros(1, 1, 8, 8)                       # t_joff with one channel
    with pytest.raises(hip.P3Error, match="target 1 must be"):
        hip.hisup_train_loss(*a, L.WEIGHTS)
    a = _host()
    a[1] = torch.zeros(64, 8)                            # rows without shape=
    with pytest.raises(hip.P3Error):
        hip.hisup_train_loss(*a, L.WEIGHTS)
    with pytest.raises(hip.P3Error, match="five loss weights"):
        hip.hisup_train_loss(*_host(), (1.0, 2.0))
    big = [torch.zeros(1, 1, 1, 1, dtype=t.dtype).expand(1, t.shape[1], 2048, 2049) for t in _host()]      # no storage behind them
    with pytest.raises(hip.P3Error, match="beyond"):
        hip.hisup_train_loss(*big, L.WEIGHTS)


def test_criterion_reads_the_weights_from_the_config():
    from pixelspointspolygons_amd import hisup
    from pixelspointspolygons_amd.config import make_config
    from pixelspointspolygons_amd.hisup_losses import HEAD_KEYS, HiSupCriterion
    cfg = make_config("vit_cnn", model="hisup", vit_depth=1, device="cpu")
    crit = HiSupCriterion(cfg)
    assert crit.loss_weights == dict(cfg.experiment.model.loss_weights) and tuple(crit.weights) == L.WEIGHTS
    assert tuple("loss_" + k for k in HEAD_KEYS) == hisup.LOSS_KEYS == tuple("loss_" + n for n in L.NAMES)
    cfg.experiment.model.loss_weights["loss_afm"] = 0.5
    assert HiSupCriterion(cfg).weights == [8.0, 0.25, 1.0, 0.5, 1.0]
    del cfg.experiment.model.loss_weights["loss_mask"]
    with pytest.raises(ValueError, match="loss_weights"):
        HiSupCriterion(cfg)
    # training through the model itself stays refused, message included
    model = hisup.HiSupModel(make_config("vit_cnn", model="hisup", vit_depth=1, device="cpu"), 0).train()
    with pytest.raises(NotImplementedError, match="the head set has no backward yet"):
        model(torch.zeros(1, 3, 224, 224), None, None)
