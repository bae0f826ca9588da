"""Plain-torch restatement of the DINOv2 ViT-S/14 encoder (models/vision_transformer/vit_dinov2.py over the hub's `dinov2_vits14`), for the tests only:
any dtype (float64 for gradients), autograd straight through.  Takes the reference-named state dict
  {p}cls_token [1,1,D]  {p}pos_embed [1,1+g*g,D]  {p}mask_token [1,D] (unused)  {p}patch_embed.proj.{weight [D,3,P,P],bias}
  {p}blocks.{i}.{norm1,attn.qkv,attn.proj,ls1.gamma,norm2,mlp.fc1,mlp.fc2,ls2.gamma}  {p}norm.{weight,bias}
and `interpolate_offset`: 0.1 = F.interpolate(scale_factor=(n + 0.1) / g) (the hub's dinov2_vits14, as recalled), 0.0 = F.interpolate(size=(n, n))
(transformers.Dinov2Model; pinned by tests/golden/dinov2_hf_s14.npz).  Not imported by the package."""
import math

import torch
import torch.nn.functional as F

DINO_S14 = dict(dim=384, depth=12, heads=6, mlp=1536, patch=14, img=224, grid=37, eps=1e-6)


def make_state_dict(vc=DINO_S14, seed=0, prefix="", dtype=torch.float32):
    """seeded weights with every term visible: gamma ~ U(0.05, 1.5), biases and LayerNorm affines away from 0 / 1"""
    g = torch.Generator().manual_seed(seed)
    D, H, P = vc["dim"], vc["mlp"], vc["patch"]

    def n(*shape, std):
        return torch.randn(*shape, generator=g) * std

    sd = {"cls_token": n(1, 1, D, std=0.02), "pos_embed": n(1, 1 + vc["grid"] ** 2, D, std=0.02), "mask_token": torch.zeros(1, D),
          "patch_embed.proj.weight": n(D, 3, P, P, std=0.03), "patch_embed.proj.bias": n(D, std=0.02)}
    for i in range(vc["depth"]):
        b = f"blocks.{i}."
        for nm, (o, k) in {"attn.qkv": (3 * D, D), "attn.proj": (D, D), "mlp.fc1": (H, D), "mlp.fc2": (D, H)}.items():
            sd[b + nm + ".weight"] = n(o, k, std=0.04)
            sd[b + nm + ".bias"] = n(o, std=0.02)
        for nm in ("norm1", "norm2"):
            sd[b + nm + ".weight"] = 1.0 + n(D, std=0.1)
            sd[b + nm + ".bias"] = n(D, std=0.05)
        for nm in ("ls1", "ls2"):
            sd[b + nm + ".gamma"] = 0.05 + 1.45 * torch.rand(D, generator=g)
    sd["norm.weight"] = 1.0 + n(D, std=0.1)
    sd["norm.bias"] = n(D, std=0.05)
    return {prefix + k: v.to(dtype) for k, v in sd.items()}


def resample_pos(pos_embed, n_out, interpolate_offset):
    """[1, 1 + g*g, D] -> [1, 1 + n_out^2, D]: the hub's interpolate_pos_encoding (bicubic, no antialias); CLS row passes through"""
    D = pos_embed.shape[-1]
    g = int(round(math.sqrt(pos_embed.shape[1] - 1)))
    if g == n_out:
        return pos_embed
    grid = pos_embed[:, 1:].reshape(1, g, g, D).permute(0, 3, 1, 2)
    if interpolate_offset:
        s = float(n_out + interpolate_offset) / g
        grid = F.interpolate(grid, scale_factor=(s, s), mode="bicubic", align_corners=False)
    else:
        grid = F.interpolate(grid, size=(n_out, n_out), mode="bicubic", align_corners=False)
    assert grid.shape[-2:] == (n_out, n_out)
    return torch.cat([pos_embed[:, :1], grid.permute(0, 2, 3, 1).reshape(1, n_out * n_out, D)], dim=1)


def patch_tokens(sd, img, interpolate_offset, prefix="", heads=6, eps=1e-6, depth=None):
    """-> norm(x_prenorm[:, 1:]) [B, np, D]: what vit_dinov2.py hands to its bottleneck"""
    p = prefix
    w = sd[p + "patch_embed.proj.weight"]
    D, P = w.shape[0], w.shape[-1]
    if depth is None:
        depth = 1 + max(int(k[len(p) + 7:].split(".")[0]) for k in sd if k.startswith(p + "blocks."))
    x = F.conv2d(img.to(w.dtype), w, sd[p + "patch_embed.proj.bias"], stride=P).flatten(2).transpose(1, 2)
    B, n, _ = x.shape
    x = torch.cat([sd[p + "cls_token"].expand(B, -1, -1), x], dim=1) + resample_pos(sd[p + "pos_embed"], int(round(math.sqrt(n))), interpolate_offset)
    hd = D // heads
    for i in range(depth):
        b = f"{p}blocks.{i}."
        h = F.layer_norm(x, (D,), sd[b + "norm1.weight"], sd[b + "norm1.bias"], eps)
        qkv = F.linear(h, sd[b + "attn.qkv.weight"], sd[b + "attn.qkv.bias"]).reshape(B, n + 1, 3, heads, hd).permute(2, 0, 3, 1, 4)
        a = torch.softmax(qkv[0] @ qkv[1].transpose(-1, -2) / math.sqrt(hd), dim=-1) @ qkv[2]
        a = a.transpose(1, 2).reshape(B, n + 1, D)
        x = x + sd[b + "ls1.gamma"] * F.linear(a, sd[b + "attn.proj.weight"], sd[b + "attn.proj.bias"])
        h = F.layer_norm(x, (D,), sd[b + "norm2.weight"], sd[b + "norm2.bias"], eps)
        h = F.linear(F.gelu(F.linear(h, sd[b + "mlp.fc1.weight"], sd[b + "mlp.fc1.bias"])), sd[b + "mlp.fc2.weight"], sd[b + "mlp.fc2.bias"])
        x = x + sd[b + "ls2.gamma"] * h
    return F.layer_norm(x[:, 1:], (D,), sd[p + "norm.weight"], sd[p + "norm.bias"], eps)


def encoder(sd, img, interpolate_offset, out_dim=256, **kw):
    """ViTDINOv2(bottleneck=True).forward: patch tokens -> AdaptiveAvgPool1d(out_dim) over channels"""
    t = patch_tokens(sd, img, interpolate_offset, **kw)
    return F.adaptive_avg_pool1d(t, out_dim) if out_dim else t
