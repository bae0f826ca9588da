"""CPU side of the DINOv2 ViT-S/14 encoder (vit_dinov2): configuration, module tree / state_dict contract, the plain-torch restatement against the
independent transformers.Dinov2Model fixture, the host-built bicubic tap tables against F.interpolate, checkpoint interchange."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dinov2_ref as R  # noqa: E402
from helpers import load_golden, rel_err  # noqa: E402

from pixelspointspolygons_amd.config import make_config  # noqa: E402

D = 384


def _expected_encoder_keys(depth):
    want = {"vit.cls_token": (1, 1, D), "vit.pos_embed": (1, 1370, D), "vit.mask_token": (1, D),
            "vit.patch_embed.proj.weight": (D, 3, 14, 14), "vit.patch_embed.proj.bias": (D,),
            "vit.norm.weight": (D,), "vit.norm.bias": (D,), "norm.weight": (D,), "norm.bias": (D,)}
    for i in range(depth):
        b = f"vit.blocks.{i}."
        for nm, (o, k) in {"attn.qkv": (3 * D, D), "attn.proj": (D, D), "mlp.fc1": (4 * D, D), "mlp.fc2": (D, 4 * D)}.items():
            want[b + nm + ".weight"], want[b + nm + ".bias"] = (o, k), (o,)
        for nm in ("norm1", "norm2"):
            want[b + nm + ".weight"], want[b + nm + ".bias"] = (D,), (D,)
        want[b + "ls1.gamma"], want[b + "ls2.gamma"] = (D,), (D,)
    return want


def test_make_config_vit_dinov2_restates_the_shipped_yaml():
    cfg = make_config("vit_dinov2", device="cpu")
    enc = cfg.experiment.encoder
    assert enc.name == "vit_dinov2" and enc.use_images and not enc.use_lidar
    assert enc.patch_size == 14 and enc.patch_feature_size == 16 and enc.num_patches == 256 and enc.in_size == 224
    assert enc.type == "vit_small_patch14_224.dino" and enc.patch_feature_dim == 384 and enc.out_feature_dim == 256
    assert list(enc.image_mean) == [0.485, 0.456, 0.406] and list(enc.image_std) == [0.228, 0.224, 0.225] and enc.image_max_pixel_value == 255.0
    assert enc.interpolate_offset == 0.1
    other = make_config("vit", device="cpu").experiment.encoder          # the other encoders keep their defaults
    assert other.patch_size == 8 and other.num_patches == 784 and list(other.image_std) == [1.0, 1.0, 1.0] and "interpolate_offset" not in other


def test_pix2poly_model_builds_with_the_reference_state_dict_contract():
    from pixelspointspolygons_amd.pix2poly import Pix2PolyModel, Tokenizer
    from pixelspointspolygons_amd.vision_transformer import ViTDINOv2
    cfg = make_config("vit_dinov2", device="cpu", precision="fp32")
    model = Pix2PolyModel(cfg, Tokenizer(cfg).vocab_size, 0)
    assert isinstance(model.encoder, ViTDINOv2)
    assert model.encoder.norm is model.encoder.vit.norm
    assert isinstance(model.encoder.bottleneck, torch.nn.AdaptiveAvgPool1d)
    got = {k: tuple(v.shape) for k, v in model.encoder.state_dict().items()}
    assert got == _expected_encoder_keys(12)
    assert tuple(model.decoder.encoder_pos_embed.shape)[-2] == 256            # num_patches reaches the Decoder
    assert model.encoder.vit.interpolate_offset == 0.1
    assert ViTDINOv2(cfg, interpolate_offset=0.0).vit.interpolate_offset == 0.0


@pytest.mark.parametrize("encoder", ["vit", "pointpillars_vit", "early_fusion_vit"])
def test_existing_encoders_keep_their_keys(encoder):
    from pixelspointspolygons_amd.pix2poly import Pix2PolyModel, Tokenizer
    cfg = make_config(encoder, device="cpu", vit_depth=2)
    keys = list(Pix2PolyModel(cfg, Tokenizer(cfg).vocab_size, 0).state_dict().keys())
    assert not [k for k in keys if ".ls1." in k or ".ls2." in k or "mask_token" in k]
    blk = [k for k in keys if ".blocks.0." in k]
    assert sorted(k.split(".blocks.0.")[1] for k in blk) == sorted(
        f"{m}.{p}" for m in ("norm1", "attn.qkv", "attn.proj", "norm2", "mlp.fc1", "mlp.fc2") for p in ("weight", "bias"))


def test_pretrained_needs_its_checkpoint_file(tmp_path):
    from pixelspointspolygons_amd.vision_transformer import ViTDINOv2
    cfg = make_config("vit_dinov2", device="cpu", vit_depth=1)
    cfg.experiment.encoder.pretrained = True
    cfg.experiment.encoder.checkpoint_file = str(tmp_path / "absent.pth")
    with pytest.raises(FileNotFoundError):
        ViTDINOv2(cfg)
    vc = dict(R.DINO_S14, depth=1)
    sd = R.make_state_dict(vc, seed=3)
    torch.save({"model": sd}, tmp_path / "wrapped.pth")                       # unwrap "model" / "state_dict", strict=False
    cfg.experiment.encoder.checkpoint_file = str(tmp_path / "wrapped.pth")
    enc = ViTDINOv2(cfg)
    assert torch.equal(enc.vit.blocks[0].ls2.gamma.detach(), sd["blocks.0.ls2.gamma"])
    assert torch.equal(enc.norm.weight.detach(), sd["norm.weight"])


def test_restatement_matches_independent_implementation():
    """tests/dinov2_ref.py against transformers.Dinov2Model (fixture made by tests/golden/make_dinov2_golden.py).  Dinov2Model resamples with
    size=(16, 16): this pins interpolate_offset = 0.0; the 0.1 form must differ visibly (the fixture tells the two conventions apart)."""
    d, _ = load_golden("dinov2_hf_s14.npz")
    sd = R.make_state_dict(R.DINO_S14, seed=42)
    wsum = float(sum(v.double().sum() for v in sd.values() if v.is_floating_point()))
    assert abs(wsum - float(d["wsum"][0])) < 1e-6 * abs(wsum) + 1e-6, "torch RNG drifted: regenerate fixtures"
    img = d["image"].float()
    with torch.no_grad():
        tok = R.patch_tokens(sd, img, 0.0)
        tok1 = R.patch_tokens(sd, img, 0.1)
    e0, e1 = rel_err(tok[:, ::4, :], d["tokens"]), rel_err(tok1[:, ::4, :], d["tokens"])
    print(f"rel err vs Dinov2Model: offset 0.0 {e0:.3e}, offset 0.1 {e1:.3e}")
    assert e0 < 5e-5
    assert e1 > 1e-3


@pytest.mark.parametrize("offset", [0.0, 0.1])
@pytest.mark.parametrize("n_in,n_out", [(37, 16), (37, 37 + 3), (16, 37), (5, 2)])
def test_host_tap_tables_are_torch_bicubic(offset, n_in, n_out):
    from pixelspointspolygons_amd.hip import bicubic_taps
    scale = (n_out + offset) / n_in if offset else None
    taps = bicubic_taps(n_in, n_out, scale)
    assert taps.dtype == torch.float64 and tuple(taps.shape) == (n_out, n_in)
    assert int((taps != 0).sum(1).max()) <= 4
    g = torch.Generator().manual_seed(n_in * 100 + n_out)
    table = torch.randn(1, 6, n_in, n_in, generator=g, dtype=torch.float64)
    if offset:
        ref = F.interpolate(table, scale_factor=(scale, scale), mode="bicubic", align_corners=False)
    else:
        ref = F.interpolate(table, size=(n_out, n_out), mode="bicubic", align_corners=False)
    assert ref.shape[-1] == n_out
    got = torch.einsum("yi,xj,bcij->bcyx", taps, taps, table)
    err = float((got - ref).abs().max())
    print(f"taps vs F.interpolate ({n_in} -> {n_out}, offset {offset}): max abs {err:.2e}")
    assert err <= 1e-12


def test_resample_ref_equals_tap_form_on_the_full_table():
    """the restatement's resample_pos (F.interpolate on [1, D, 37, 37]) is the separable linear map the kernels implement"""
    from pixelspointspolygons_amd.hip import bicubic_taps
    pos = torch.randn(1, 1370, 8, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    for off in (0.0, 0.1):
        taps = bicubic_taps(37, 16, (16 + off) / 37 if off else None)
        want = R.resample_pos(pos, 16, off)
        got = torch.einsum("yi,xj,ijd->yxd", taps, taps, pos[0, 1:].view(37, 37, 8)).reshape(256, 8)
        assert float((got - want[0, 1:]).abs().max()) <= 1e-12 and torch.equal(want[0, 0], pos[0, 0])


def test_checkpoint_accepts_a_bare_backbone_file():
    from pixelspointspolygons_amd import checkpoint as C
    from pixelspointspolygons_amd.pix2poly import Pix2PolyModel, Tokenizer
    cfg = make_config("vit_dinov2", device="cpu", vit_depth=2, precision="fp32")
    model = Pix2PolyModel(cfg, Tokenizer(cfg).vocab_size, 0)
    bare = R.make_state_dict(dict(R.DINO_S14, depth=2), seed=9)                # keys without "encoder.vit."
    rep = C.compare(model, bare)
    enc_keys = ["encoder." + k for k in _expected_encoder_keys(2)]
    assert sorted(rep.matched) == sorted(enc_keys) and not rep.unused and not rep.shape_mismatch
    assert all(not k.startswith("encoder.") for k in rep.missing) and rep.missing
    before = model.decoder.state_dict()
    before = {k: v.clone() for k, v in before.items()}
    C.load_checkpoint(model, {"model": bare}, strict=False)
    sd = model.state_dict()
    for k, v in bare.items():
        assert torch.equal(sd["encoder.vit." + k], v), k
    assert torch.equal(sd["encoder.norm.weight"], bare["norm.weight"])
    assert all(torch.equal(v, model.decoder.state_dict()[k]) for k, v in before.items())
    bad = dict(bare)
    bad["pos_embed"] = bare["pos_embed"][:, :257]                               # a table of another grid is a shape mismatch, not a silent load
    assert [m[0] for m in C.compare(model, bad).shape_mismatch] == ["encoder.vit.pos_embed"]
