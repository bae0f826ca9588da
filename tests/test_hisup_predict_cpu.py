"""HiSup inference, the parts that need no GPU: `make_config(model="hisup")`, the model factory and its state_dict keys, the annotation
encoder's bound check, the three new C-ABI entries, and the CPU restatement (tests/hisup_predict_ref.py) against the values the reference's
own functions produced (tests/golden/hisup_predict.npz, written by tests/golden/make_hisup_predict_golden.py)."""
import ctypes
import hashlib
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import hisup_predict_ref as R
from tests.helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "p3hip.h")
CNN = ("vit_cnn", "pointpillars_vit_cnn", "early_fusion_vit_cnn")


def _digest(cfg):
    return hashlib.sha256(json.dumps(cfg, sort_keys=True).encode()).hexdigest()[:16]


# ------------------------------------------------------------------------------------------------ configuration
@pytest.mark.parametrize("encoder", CNN)
def test_make_config_hisup_describes_the_shipped_model_yaml(encoder):
    from pixelspointspolygons_amd.config import make_config
    cfg = make_config(encoder, model="hisup")
    e, m = cfg.experiment.encoder, cfg.experiment.model
    assert m.name == "hisup" and e.name == encoder
    assert m.decoder.in_feature_size == 224 and m.decoder.in_feature_dim == 256
    assert (e.out_feature_size, e.out_feature_height, e.out_feature_width) == (224, 224, 224)
    assert (e.in_size, e.in_height, e.in_width) == (224, 224, 224) and e.patch_feature_size == 28
    assert dict(m.loss_weights) == {"loss_joff": 0.25, "loss_jloc": 8.0, "loss_mask": 1.0, "loss_afm": 0.1, "loss_remask": 1.0}
    assert m.learning_rate == 1e-4 and m.weight_decay == 1e-4 and m.num_epochs == 200
    small = make_config(encoder, model="hisup", in_size=112)
    assert small.experiment.model.decoder.in_feature_size == 112 and small.experiment.encoder.out_feature_width == 112


# sha256[:16] of json.dumps(make_config(encoder, model), sort_keys=True) at the commit before HiSup inference was added
_PARENT = {
    ("vit", "pix2poly"): "d6f5257d0ad4ca7a", ("vit", "ffl"): "5cd4b7303addcb5f",
    ("vit_dinov2", "pix2poly"): "850446e92ddb71d1", ("vit_dinov2", "ffl"): "86d69b4e34bdb240",
    ("pointpillars_vit", "pix2poly"): "70cb6d158aa2505a", ("pointpillars_vit", "ffl"): "13c5a045fe582d69",
    ("early_fusion_vit", "pix2poly"): "5eb825aafdc9d6ee", ("early_fusion_vit", "ffl"): "ba757a23b570fa8a",
    ("vit_cnn", "pix2poly"): "c9df1402fb114c3a", ("vit_cnn", "ffl"): "a26c5987aa22b288",
    ("pointpillars_vit_cnn", "pix2poly"): "1ea924150df05ebd", ("pointpillars_vit_cnn", "ffl"): "7c778afcf9d5b018",
    ("early_fusion_vit_cnn", "pix2poly"): "daf949bbae8cbe5c", ("early_fusion_vit_cnn", "ffl"): "c2b3f5298c935002",
}
# ... and one of them in full, so that a mismatch can be read
_PARENT_VIT_CNN_FFL = json.loads("""
{"experiment": {"encoder": {"checkpoint_file": null, "image_max_pixel_value": 255.0, "image_mean": [0.0, 0.0, 0.0], "image_std": [1.0, 1.0, 1.0],
"in_height": 224, "in_size": 224, "in_voxel_size": {"x": 8.0, "y": 8.0, "z": 100.0}, "in_width": 224, "max_num_points_per_voxel": 64,
"max_num_voxels": {"test": 784, "train": 784}, "name": "vit_cnn", "num_patches": 784, "out_feature_dim": 256, "out_feature_height": 28,
"out_feature_size": 224, "out_feature_width": 28, "patch_feature_dim": 384, "patch_feature_height": 28, "patch_feature_size": 28,
"patch_feature_width": 28, "patch_size": 8, "pretrained": false, "type": "vit_small_patch8_224.dino", "use_images": true, "use_lidar": false,
"vit": {"checkpoint_file": null, "depth": 12, "mlp_dim": 1536, "num_heads": 6, "pretrained": false, "type": "vit_small_patch8_224.dino"}},
"lidar_dropout": null, "model": {"batch_size": 16, "compute_crossfield": true, "compute_seg": true, "decoder": {"in_feature_dim": 256,
"in_feature_size": 28}, "learning_rate": 0.0003, "loss": {"multi": {"epoch_thresholds": [0, 5, 10], "weights": {"crossfield_align": 1,
"crossfield_align90": 0.5, "crossfield_smooth": 0.005, "seg": 1, "seg_edge_crossfield": [0, 0, 0.2], "seg_edge_interior": [0, 0, 0.2],
"seg_interior_crossfield": [0, 0, 0.2]}}, "seg": {"bce_coef": 1.0, "dice_coef": 0.2, "sigma": 10, "type": "bool", "use_dist": false,
"use_freq": false, "use_size": false, "w0": 50}}, "name": "ffl", "num_epochs": 200, "perm_loss_weight": 10.0, "seg": {"compute_edge": false,
"compute_interior": true, "compute_vertex": false}, "sinkhorn_iterations": 100, "tokenizer": {"generation_steps": null, "max_len": null,
"max_num_vertices": 192, "num_bins": 224, "pad_idx": null, "shuffle_tokens": false}, "vertex_loss_weight": 1.0, "weight_decay": 0.0001}},
"host": {"device": "cuda", "multi_gpu": false}, "precision": "bf16", "run_type": {"batch_size": 16, "logging": "INFO", "name": "release"}}
""")


def test_every_other_make_config_result_is_unchanged():
    from pixelspointspolygons_amd.config import make_config
    assert json.loads(json.dumps(make_config("vit_cnn", "ffl"))) == _PARENT_VIT_CNN_FFL
    for (enc, model), want in _PARENT.items():
        assert _digest(make_config(enc, model)) == want, (enc, model)
    assert _digest(make_config("vit_cnn", "ffl", in_size=112, vit_depth=2, precision="fp32", batch_size=4, lidar_dropout=0.1)) == "f700f2ac4bc8b425"


# ------------------------------------------------------------------------------------------------ factory
def _small_cfg(encoder, **kw):
    from pixelspointspolygons_amd.config import make_config
    return make_config(encoder, model="hisup", vit_depth=1, device="cpu", **kw)


@pytest.mark.parametrize("encoder", CNN)
def test_hisup_model_keys_are_the_reference_modules(encoder):
    """head keys: the reference EncoderDecoder's own state_dict().keys() (fixture, built over a parameter-free encoder); encoder keys: this
    package's `*ViTCNN` encoder (the FFL tests pin those to the reference) under `encoder.`"""
    from pixelspointspolygons_amd import ffl, hisup
    cfg = _small_cfg(encoder)
    model = hisup.HiSupModel(cfg, local_rank=0)
    assert isinstance(model, hisup.EncoderDecoder) and isinstance(model, hisup.HiSupHeads)
    head_keys = bytes(load_golden("hisup_predict.npz")[0]["keys.heads"].numpy()).decode().split("\n")
    assert len(head_keys) == 135 and "mask_head.0.weight" in head_keys and "a2m_att.conv.weight" in head_keys
    enc_cls = {"vit_cnn": ffl.ViTCNN, "pointpillars_vit_cnn": ffl.PointPillarsViTCNN, "early_fusion_vit_cnn": ffl.EarlyFusionViTCNN}[encoder]
    assert type(model.encoder) is enc_cls
    want = set(head_keys) | {"encoder." + k for k in enc_cls(cfg).state_dict().keys()}
    assert set(model.state_dict().keys()) == want
    assert list(hisup.HiSupHeads(dim_in=256, precision="fp32").state_dict().keys()) == head_keys      # HiSupHeads itself keeps its keys
    # a reference-shaped state_dict loads strictly, bare and with the prefix DDP leaves
    from pixelspointspolygons_amd.checkpoint import load_checkpoint
    sd = {k: torch.randn(v.shape) if v.is_floating_point() else v.clone() for k, v in model.state_dict().items()}
    model.load_state_dict(sd, strict=True)
    other = hisup.HiSupModel(cfg, 0)
    load_checkpoint(other, {"model_state_dict": {"module." + k: v for k, v in sd.items()}, "epoch": 3}, strict=True)
    for k, v in other.state_dict().items():
        assert torch.equal(v, sd[k]), k
    load_checkpoint(hisup.HiSupModel(cfg, 0), dict(sd), strict=True)


def test_hisup_model_encoder_dispatch_errors():
    from pixelspointspolygons_amd import hisup
    for name, img, lidar in (("hrnet", True, False), ("fusion_hrnet", True, True), ("pointpillars", False, True)):
        cfg = _small_cfg("vit_cnn")
        cfg.experiment.encoder.update(name=name, use_images=img, use_lidar=lidar)
        with pytest.raises(NotImplementedError, match=f"Encoder {name} not implemented for HiSupModel"):
            hisup.HiSupModel(cfg, 0)
    cfg = _small_cfg("vit_cnn")
    cfg.experiment.encoder.update(use_images=False, use_lidar=False)
    with pytest.raises(ValueError):
        hisup.HiSupModel(cfg, 0)


def test_training_mode_raises_a_clear_error():
    from pixelspointspolygons_amd import hisup
    model = hisup.HiSupModel(_small_cfg("vit_cnn"), 0).train()
    with pytest.raises(NotImplementedError, match="training"):
        model(torch.zeros(1, 3, 224, 224), None, None)


def test_annotation_encoder_bound_check_and_empty_edges():
    from pixelspointspolygons_amd import hisup
    enc = hisup.AnnotationEncoder(_small_cfg("vit_cnn"))
    ann = dict(junctions=torch.tensor([[3.25, 4.75], [10.5, 2.0]]), juncs_tag=torch.tensor([1, 2]), edges_positive=torch.zeros((0, 2), dtype=torch.long),
               mask=torch.zeros(16, 16), height=16, width=16, juncs_index=torch.tensor([0, 0]), bbox=torch.tensor([[0, 0, 16, 16]]))
    t, metas = enc([ann, ann])
    assert t["jloc"].shape == (2, 1, 16, 16) and t["jloc"].dtype == torch.int64 and t["joff"].shape == (2, 2, 16, 16)
    assert t["mask"].shape == (2, 1, 16, 16) and t["afmap"].shape == (2, 2, 16, 16) and not t["afmap"].any()
    assert int(t["jloc"][0, 0, 4, 3]) == 1 and int(t["jloc"][0, 0, 2, 10]) == 2 and int(t["jloc"].sum()) == 6
    assert abs(float(t["joff"][0, 0, 4, 3]) + 0.25) < 1e-6 and abs(float(t["joff"][0, 1, 4, 3]) - 0.25) < 1e-6
    assert len(metas) == 2 and set(metas[0]) == {"junc", "junc_index", "bbox"}
    for bad in ([[16.0, 1.0]], [[1.0, 16.5]], [[-1.5, 1.0]]):
        with pytest.raises(ValueError, match="Junctions out of bound"):
            enc([dict(ann, junctions=torch.tensor(bad), juncs_tag=torch.tensor([1]))])


# ------------------------------------------------------------------------------------------------ C-ABI
def test_new_entries_are_exported_with_the_declared_arity():
    from pixelspointspolygons_amd._lib import load
    from pixelspointspolygons_amd.build import build_library
    lib = load(build_library(verbose=False))
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    arity = {"p3_hisup_junctions": 19, "p3_hisup_regions": 17, "p3_hisup_val_loss": 15, "p3_hisup_junctions_workspace_bytes": 3,
             "p3_hisup_regions_workspace_bytes": 4, "p3_hisup_val_loss_workspace_bytes": 3}
    for name, n in arity.items():
        assert hasattr(lib, name), name
        m = re.search(r"\b" + name + r"\s*\(([^;{}]*?)\)\s*;", text, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == n, (name, len(m.group(1).split(",")))
    src = open(os.path.join(ROOT, "pixelspointspolygons_amd", "hip.py")).read()
    for name, n in arity.items():                       # the ctypes call sites pass as many arguments
        i = src.index("lib()." + name + "(") + len("lib()." + name + "(")
        depth, j, commas = 1, i, 0
        while depth:
            depth += {"(": 1, ")": -1}.get(src[j], 0)
            commas += src[j] == "," and depth == 1
            j += 1
        assert commas + 1 == n, (name, commas + 1)
    z = ctypes.c_int64(0)
    assert lib.p3_hisup_junctions(None, z, z, z, None, z, z, z, 1, 8, 8, ctypes.c_float(1), ctypes.c_float(1), None, None, None, None, None, None) == -1
    assert b"p3_hisup_junctions" in lib.p3_last_error_string()
    assert lib.p3_hisup_regions(None, z, z, z, 1, 8, 8, 16, None, None, None, None, None, None, None, None, None) == -1
    assert lib.p3_hisup_val_loss(None, None, None, None, None, None, None, None, None, 1, 8, 8, None, None, None) == -1


def test_wrappers_refuse_host_tensors():
    from pixelspointspolygons_amd import hip
    with pytest.raises(hip.P3Error):
        hip.hisup_junctions(torch.zeros(1, 3, 8, 8), torch.zeros(1, 2, 8, 8))
    with pytest.raises(hip.P3Error):
        hip.hisup_regions(torch.zeros(1, 2, 8, 8))
    with pytest.raises(hip.P3Error):
        hip.hisup_val_loss(*[torch.zeros(1, n, 8, 8) for n in (3, 2, 2, 2, 2, 1, 2, 1, 2)])


# ------------------------------------------------------------------------------------------------ the restatement the GPU tests use
def test_ref_junctions_reproduce_the_reference_function():
    d, _ = load_golden("hisup_predict.npz")
    ks = [int(k) for k in d["junc.k"]]
    jloc = torch.cat([torch.full_like(d["junc.jloc12"][:, :1], 6.0), d["junc.jloc12"]], 1)
    for i, K in enumerate(ks):
        ref = R.junctions(jloc[i], d["junc.joff"][i])
        R.check_planted(ref, K)
        want = d[f"junc.ref{i}"]
        assert ref["counts"] == (min(K, 300), min(K, 300)) and want.shape == (2 * min(K, 300), 2)
        assert torch.equal(ref["juncs"], want)            # same torch operators in the same order: bit for bit
    # the planted generator still draws what the fixture stores (a later torch may not: then only the stored inputs count)
    again, joff = R.planted_junction_maps(ks, 96, 3, 1, seed=11)
    if torch.equal(again[:, 1:], d["junc.jloc12"]):
        assert torch.equal(joff, d["junc.joff"])


def test_ref_val_losses_reproduce_the_reference_functions():
    d, _ = load_golden("hisup_predict.npz")
    got = R.val_losses(*[d["loss.pred." + k] for k in ("jloc", "joff", "mask", "afm", "remask")], d["loss.t_jloc"], d["loss.t_joff"], d["loss.t_mask"],
                       d["loss.t_afm"])
    assert got.dtype == torch.float64 and torch.allclose(got, d["loss.ref"], rtol=1e-12, atol=0)
    assert not d["loss.t_jloc"][1].any() and d["loss.t_jloc"][0].any() and not d["loss.t_afm"][2].any()     # the w == 0 image, the image without edges
