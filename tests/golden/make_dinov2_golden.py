"""tests/golden/dinov2_hf_s14.npz: the DINOv2 ViT-S/14 body against the independent transformers.Dinov2Model, in the manner of vit_hf_s8.npz.

Usage:  python tests/golden/make_dinov2_golden.py      (needs `transformers`; no reference checkout, no network)
Seeded full-shape weights (tests/dinov2_ref.make_state_dict, seed 42: dim 384, depth 12, 6 heads, 37 x 37 position table, gamma ~ U(0.05, 1.5)) are mapped
into Dinov2Model; one 224 px image (stored as float16, exactly representable) -> last_hidden_state[:, 1:] (final LayerNorm applied, CLS dropped), every
4th token.  The fixture holds no weights: `wsum` guards against torch RNG drift.  Dinov2Model resamples the position table with
F.interpolate(size=(16, 16)), so this fixture pins the interpolate_offset = 0.0 form ONLY; the hub's 0.1 form has no independent pin here."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from transformers import Dinov2Config, Dinov2Model  # noqa: E402
import dinov2_ref as R  # noqa: E402

torch.set_grad_enabled(False)


def hf_dinov2(vc, sd, img):
    c = Dinov2Config(hidden_size=vc["dim"], num_hidden_layers=vc["depth"], num_attention_heads=vc["heads"], mlp_ratio=vc["mlp"] // vc["dim"],
                     image_size=vc["grid"] * vc["patch"], patch_size=vc["patch"], layer_norm_eps=vc["eps"], use_swiglu_ffn=False,
                     hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, drop_path_rate=0.0, qkv_bias=True)
    m = Dinov2Model(c).eval()
    D = vc["dim"]
    t = {"embeddings.cls_token": sd["cls_token"], "embeddings.mask_token": sd["mask_token"], "embeddings.position_embeddings": sd["pos_embed"],
         "embeddings.patch_embeddings.projection.weight": sd["patch_embed.proj.weight"],
         "embeddings.patch_embeddings.projection.bias": sd["patch_embed.proj.bias"],
         "layernorm.weight": sd["norm.weight"], "layernorm.bias": sd["norm.bias"]}
    have = set(m.state_dict().keys())
    for i in range(vc["depth"]):
        p = f"blocks.{i}."
        q = next(pre for pre in (f"encoder.layer.{i}.", f"layers.{i}.", f"encoder.layers.{i}.") if any(k.startswith(pre) for k in have))
        W, b = sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"]
        attn = {k for k in have if k.startswith(q + "attention")}
        for j, (old, new) in enumerate((("attention.attention.query", "attention.q_proj"), ("attention.attention.key", "attention.k_proj"),
                                        ("attention.attention.value", "attention.v_proj"))):
            nme = old if any(k.startswith(q + old) for k in attn) else new
            t[q + nme + ".weight"] = W[j * D:(j + 1) * D]
            t[q + nme + ".bias"] = b[j * D:(j + 1) * D]
        out = "attention.output.dense" if any(k.startswith(q + "attention.output.dense") for k in attn) else "attention.o_proj"
        t[q + out + ".weight"], t[q + out + ".bias"] = sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"]
        for a, bname in (("norm1", "norm1"), ("norm2", "norm2"), ("mlp.fc1", "mlp.fc1"), ("mlp.fc2", "mlp.fc2")):
            t[q + a + ".weight"], t[q + a + ".bias"] = sd[p + bname + ".weight"], sd[p + bname + ".bias"]
        t[q + "layer_scale1.lambda1"], t[q + "layer_scale2.lambda1"] = sd[p + "ls1.gamma"], sd[p + "ls2.gamma"]
    missing = m.load_state_dict(t, strict=True)
    assert not missing.unexpected_keys and not missing.missing_keys, missing
    return m(pixel_values=img).last_hidden_state


if __name__ == "__main__":
    sd = R.make_state_dict(R.DINO_S14, seed=42)
    g = torch.Generator().manual_seed(23)
    img = torch.rand(1, 3, 224, 224, generator=g).to(torch.float16).float()
    out = hf_dinov2(R.DINO_S14, sd, img)[:, 1:]
    for off in (0.0, 0.1):
        ref = R.patch_tokens({k: v.double() for k, v in sd.items()}, img.double(), off)
        print(f"float64 restatement, interpolate_offset={off}: rel err vs Dinov2Model {float((ref - out).abs().max() / out.abs().max()):.3e}")
    np.savez_compressed(os.path.join(HERE, "dinov2_hf_s14.npz"), image_seed=np.array([23]), image=img.to(torch.float16).numpy(),
                        tokens=out[:, ::4, :].numpy(),
                        wsum=np.array([float(sum(v.double().sum() for v in sd.values() if v.is_floating_point()))]))
    print("wrote dinov2_hf_s14.npz", os.path.getsize(os.path.join(HERE, "dinov2_hf_s14.npz")), "bytes")
