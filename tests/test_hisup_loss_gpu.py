"""p3_hisup_train_loss on the GPU through `hip.hisup_train_loss` and `hisup_losses.HiSupCriterion`: the five HiSup training losses and the gradients of
their weighted total against the reference's own numbers (tests/golden/hisup_loss.npz) and against float64 autograd of the reference's five lines
(tests/hisup_loss_ref.py, pinned to the fixture by tests/test_hisup_loss_cpu.py).

Tolerances: losses within 1e-5 relative of float64 (the project's figure for p3_hisup_val_loss); gradients max|g - g64| / max|g64| <= 2e-6 per map
(about 16 fp32 ulps for values that come from roughly ten roundings and an expf; fp32 torch on the CPU measures 3e-7 on the same inputs).
Measured on an MI355X: see the figures each test prints and DESIGN.md section 16."""
import functools

import pytest
import torch

from tests import hisup_loss_ref as L
from tests.guard import guarded, poisoned
from tests.helpers import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOSS_TOL, GRAD_TOL = 1e-5, 2e-6


def _hip():
    from pixelspointspolygons_amd import hip
    return hip


def _dev(inp):
    return [t.to(DEV) for t in inp["pred"] + L.targets_of(inp)]


@functools.lru_cache(maxsize=None)
def _fused(name):
    """the all-NCHW result of a shared case, computed once: (losses, grads) on the device; callers leave them unchanged"""
    return _hip().hisup_train_loss(*_dev(L.case(name)[0]), L.WEIGHTS)


def _check(tag, losses, grads, l64, t64, g64, scale=1.0):
    losses = losses.cpu().double()
    want = torch.cat([torch.as_tensor(l64).double().reshape(-1), torch.as_tensor(t64).double().reshape(1)])
    rel = ((losses - want).abs() / want.abs()).tolist()
    errs = [L.grad_err(g.cpu(), scale * torch.as_tensor(r)) for g, r in zip(grads, g64)] if grads is not None else []
    print(f"[{tag}] loss rel err (jloc, joff, mask, afm, remask, total) {['%.1e' % v for v in rel]}; gradient err {['%.1e' % v for v in errs]}")
    assert losses.shape == (6,) and max(rel) <= LOSS_TOL, rel
    for n, e in zip(L.NAMES, errs):
        assert e <= GRAD_TOL, (n, e)


# ------------------------------------------------------------------------------------------------ 1. the reference's own numbers
def test_fixture_against_the_reference():
    d, _ = load_golden("hisup_loss.npz")
    args = [d["pred." + n] for n in L.NAMES] + [d["t_jloc"], d["t_joff"], d["t_mask"], d["t_afm"]]
    losses, grads = _hip().hisup_train_loss(*[a.to(DEV) for a in args], d["weights"].tolist())
    assert losses.dtype == torch.float32 and all(g.dtype == torch.float32 and g.shape == p.shape for g, p in zip(grads, args))
    _check("fixture 3 x 19 x 23", losses, grads, d["losses"], d["total"], [d["grad." + n] for n in L.NAMES])
    assert not grads[1][1].any() and int((grads[1][2] != 0).sum()) == 2        # the image without junctions, the image with one


# ------------------------------------------------------------------------------------------------ 2.-4. float64 autograd at the shapes that matter
# odd: H * W = 1517, a ragged last workgroup and channel planes off the 16-byte grid (element accesses); one: a single pixel; small: one
# part-filled workgroup per image on 16-byte accesses; full: the model's own map size, 49 workgroups per image
@pytest.mark.parametrize("name", ["odd", "one", "small", "full"])
def test_against_float64_autograd(name):
    inp, (l64, t64, g64) = L.case(name)
    losses, grads = _fused(name)
    _check(name + " %d x %d x %d" % L.CASES[name][:3], losses, grads, l64, t64, g64)
    junction = ((inp["t_jloc"] == 1) | (inp["t_jloc"] == 2)).expand_as(inp["pred"][1])
    assert not grads[1].cpu()[~junction].any()                                 # joff: zero off the junction pixels ...
    if inp["t_jloc"].shape[0] > 1:
        assert not grads[1][1].any()                                           # ... and everywhere in the image without junctions


# ------------------------------------------------------------------------------------------------ 5. token-major rows
@pytest.mark.parametrize("name", ["odd", "small"])
def test_row_layout_is_bit_identical_and_writes_only_the_valid_columns(name):
    hip = _hip()
    inp, (l64, t64, _) = L.case(name)
    B, H, W = L.CASES[name][:3]
    base_losses, base = _fused(name)
    rows = [poisoned(p.permute(0, 2, 3, 1).reshape(-1, p.shape[1]), ld=8, device=DEV) for p in inp["pred"][:4]]      # NaN in the row padding
    preds = rows + [inp["pred"][4].to(DEV)]
    outs = [guarded(B * H * W, n, torch.float32, ld=8, device=DEV) for n in L.CHANNELS[:4]] + [guarded(B * 2, H * W, torch.float32, device=DEV)]
    grads_in = [v for v, _ in outs[:4]] + [outs[4][0].view(B, 2, H, W)]
    losses, grads = hip.hisup_train_loss(*preds, *[t.to(DEV) for t in L.targets_of(inp)], L.WEIGHTS, shape=(B, H, W), grads=grads_in)
    for (view, guard), g, ref, n in zip(outs, grads, base, L.CHANNELS):
        guard.check()                                                          # bands and columns n..7 untouched, every valid element written
        assert g.data_ptr() == view.data_ptr()
        got = g if g.dim() == 4 else g.reshape(B, H, W, n).permute(0, 3, 1, 2)
        assert torch.equal(got, ref)                                           # the per-pixel arithmetic does not depend on the layout
    assert torch.equal(losses, base_losses)                                    # nor does the pixel -> workgroup assignment
    _check(name + " rows", losses, None, l64, t64, None)
    # without caller buffers the row gradients come back as [R, n] views of the predictions' row stride
    _, own = hip.hisup_train_loss(*preds, *[t.to(DEV) for t in L.targets_of(inp)], L.WEIGHTS, shape=(B, H, W))
    for g, ref, n in zip(own[:4], base, L.CHANNELS):
        assert g.shape == (B * H * W, n) and g.stride() == (8, 1) and torch.equal(g.reshape(B, H, W, n).permute(0, 3, 1, 2), ref)
    with pytest.raises(hip.P3Error, match="strides"):                          # a gradient buffer of another row stride is refused
        hip.hisup_train_loss(*preds, *[t.to(DEV) for t in L.targets_of(inp)], L.WEIGHTS, shape=(B, H, W),
                             grads=[torch.empty(B * H * W, 4, device=DEV)[:, :3]] + grads_in[1:])


# ------------------------------------------------------------------------------------------------ 6. NCHW in guard bands, misaligned planes
def test_nchw_gradients_in_guarded_buffers_at_37_x_41():
    inp, _ = L.case("odd")
    B, H, W = L.CASES["odd"][:3]
    base_losses, base = _fused("odd")
    outs = [guarded(B * n, H * W, torch.float32, device=DEV) for n in L.CHANNELS]
    losses, grads = _hip().hisup_train_loss(*_dev(inp), L.WEIGHTS, grads=[v.view(B, n, H, W) for (v, _), n in zip(outs, L.CHANNELS)])
    for (_, guard), g, ref in zip(outs, grads, base):
        guard.check()                                                          # no stray write, every element written
        assert torch.equal(g, ref)
    assert torch.equal(losses, base_losses)


# ------------------------------------------------------------------------------------------------ 7. repeatability, values alone
@pytest.mark.parametrize("name", ["odd", "small", "full"])
def test_two_runs_are_bit_identical_and_values_alone_match(name):
    hip = _hip()
    args = _dev(L.case(name)[0])
    losses, grads = _fused(name)
    again_l, again_g = hip.hisup_train_loss(*args, L.WEIGHTS)
    assert torch.equal(losses, again_l) and all(torch.equal(a, b) for a, b in zip(grads, again_g))
    only_l, none = hip.hisup_train_loss(*args, L.WEIGHTS, need_grad=False)
    assert none is None and torch.equal(only_l, losses)


# ------------------------------------------------------------------------------------------------ 8. weights, upstream gradient
def test_criterion_backward_with_an_upstream_gradient():
    from pixelspointspolygons_amd.config import make_config
    from pixelspointspolygons_amd.hisup_losses import HEAD_KEYS, HiSupCriterion
    from pixelspointspolygons_amd import hisup
    inp, (l64, t64, _) = L.case("odd")
    _, _, g64x3 = L.reference(inp, L.WEIGHTS, upstream=3.0)
    crit = HiSupCriterion(make_config("vit_cnn", "hisup", vit_depth=1, device=DEV))
    heads = {k: p.to(DEV).requires_grad_(True) for k, p in zip(HEAD_KEYS, inp["pred"])}
    targets = dict(zip(("jloc", "joff", "mask", "afmap"), [t.to(DEV) for t in L.targets_of(inp)]))
    total, loss_dict = crit(heads, targets)
    assert total.requires_grad and total.dim() == 0 and tuple(loss_dict) == hisup.LOSS_KEYS
    assert all(v.is_cuda and v.dim() == 0 and not v.requires_grad for v in loss_dict.values())
    (total * 3).backward()
    _check("criterion x 3", torch.stack([loss_dict[k] for k in hisup.LOSS_KEYS] + [total.detach()]), [heads[k].grad for k in HEAD_KEYS], l64, t64, g64x3)
    # maps that need no gradient: the values alone, the same values
    with torch.no_grad():
        plain, plain_dict = crit({k: v.detach() for k, v in heads.items()}, targets)
    assert not plain.requires_grad and torch.equal(plain, total.detach()) and all(torch.equal(plain_dict[k], loss_dict[k]) for k in loss_dict)
    # only some maps need one
    some = {k: v.detach().requires_grad_(k == "afm") for k, v in heads.items()}
    crit(some, targets)[0].backward()
    assert torch.equal(some["afm"].grad * 3, heads["afm"].grad) and all(some[k].grad is None for k in HEAD_KEYS if k != "afm")


def test_a_zero_weight_zeroes_its_map_and_leaves_the_others():
    hip = _hip()
    args = _dev(L.case("small")[0])
    base_losses, base = _fused("small")
    for k, name in enumerate(L.NAMES):
        w = list(L.WEIGHTS)
        w[k] = 0.0
        losses, grads = hip.hisup_train_loss(*args, w)
        assert not grads[k].any(), name
        for j, (g, ref) in enumerate(zip(grads, base)):
            assert j == k or torch.equal(g, ref), (name, L.NAMES[j])
        assert torch.equal(losses[:5], base_losses[:5])                        # the un-weighted losses do not move
        want = float(base_losses[5].double() - L.WEIGHTS[k] * base_losses[k].double())
        assert abs(float(losses[5]) - want) <= 1e-6 * abs(want)


# ------------------------------------------------------------------------------------------------ 9. the whole model
def _annotations(B, seed):
    g = torch.Generator().manual_seed(seed)
    anns = []
    for b in range(B):
        n = 0 if b == 1 else 12
        j = torch.rand(n, 2, generator=g) * 223.0
        edges = torch.stack([torch.arange(n), (torch.arange(n) + 1) % max(n, 1)], 1) if n else torch.zeros((0, 2), dtype=torch.long)
        mask = torch.zeros(224, 224)
        mask[30:90, 40:120] = 1
        anns.append(dict(junctions=j.to(DEV), juncs_tag=torch.randint(1, 3, (n,), generator=g).to(DEV), edges_positive=edges.to(DEV), mask=mask.to(DEV),
                         height=224, width=224, juncs_index=torch.zeros(n, dtype=torch.long), bbox=torch.tensor([[40.0, 30.0, 120.0, 90.0]])))
    return anns


def test_criterion_on_the_models_own_heads():
    from pixelspointspolygons_amd import hisup
    from pixelspointspolygons_amd.config import make_config
    from pixelspointspolygons_amd.hisup_losses import HiSupCriterion
    from pixelspointspolygons_amd.synthetic import make_inputs
    torch.manual_seed(11)
    cfg = make_config("vit_cnn", "hisup", vit_depth=1, precision="fp32", device=DEV)
    model = hisup.HiSupModel(cfg, local_rank=0).eval()
    model.max_regions = 112 * 112                       # random weights: as many regions as a 224 x 224 map can hold
    img = make_inputs(2, seed=4)["image"].to(DEV)
    y = _annotations(2, seed=6)
    targets, heads = model.forward_common(img, None, y)
    crit = HiSupCriterion(cfg)
    total, loss_dict = crit(heads, targets)
    assert not total.requires_grad                      # forward_common's maps carry no graph: the values alone
    _, val = model.forward_val_device(img, None, y)
    for k in hisup.LOSS_KEYS:
        a, b = float(loss_dict[k]), float(val[k])
        print(f"[model] {k}: criterion {a:.7f} forward_val_device {b:.7f}")
        assert abs(a - b) <= 1e-5 * abs(b), (k, a, b)
    # total = the weighted sum, formed in float64 from the un-rounded losses: the fp32 rounding of each of the six values is all that separates them
    want = sum(w * float(loss_dict[k].double()) for w, k in zip(crit.weights, hisup.LOSS_KEYS))
    assert abs(float(total) - want) <= 2.5e-7 * abs(want), (float(total), want)
