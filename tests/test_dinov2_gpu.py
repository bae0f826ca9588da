"""DINOv2 ViT-S/14 encoder (vit_dinov2) on the GPU: the three new kernel families against float64, the encoder against tests/dinov2_ref.py and the
transformers.Dinov2Model fixture, gradients against float64 autograd, a captured train step, greedy decode with 256 memory tokens.

Tolerances are the ones tests/test_model_gpu.py / tests/test_backward_gpu.py apply to ViT-S/8 in the same precision (1e-3 rel for fp32 / fp32x3 outputs,
6e-2 for bf16; parameter gradients 1.5e-3 / 6e-3 L2-relative for fp32 / fp32x3, direction + magnitude within 5e-2 for bf16).
Measured wall time of this file on one MI355X: see DESIGN.md "DINOv2 encoder"."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dinov2_ref as R  # noqa: E402
from oracle import p3_oracle as O  # noqa: E402
from tests.helpers import l2_err, load_golden, rel_err  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {"fp32": 1e-3, "fp32x3": 1e-3, "bf16": 6e-2}                 # tests/test_model_gpu.py TOL32 / TOL16
GTOL = {"fp32": 1.5e-3, "fp32x3": 6e-3, "bf16": 5e-2}              # tests/test_backward_gpu.py test_train_step_gradients_vs_oracle_autograd
NV = 24                                                            # max_num_vertices of the small whole-model cases: 2 * 24 + 1 = 49 decode steps
GREEDY_SEED = 8                                                    # chosen on the CPU: see test_greedy_decode_...


@pytest.fixture(autouse=True)
def _no_precision_scope_leaks():
    import pixelspointspolygons_amd.hip as hip
    assert not hip.split_now()
    yield
    assert not hip.split_now()


def _vc(depth):
    return dict(R.DINO_S14, depth=depth)


def full_state_dict(depth, seed, n_vertices=NV):
    """reference-keyed Pix2Poly state dict: decoder / ScoreNets from the oracle's generator (256 memory tokens), the encoder from dinov2_ref"""
    osd = O.make_state_dict("image", dict(dim=384, depth=0, heads=6, mlp=1536, patch=14, img=224, eps=1e-6), seed=seed, n_vertices=n_vertices)
    sd = {k: v for k, v in osd.items() if not k.startswith("encoder.")}
    enc = R.make_state_dict(_vc(depth), seed=seed + 1)
    sd.update({"encoder.vit." + k: v for k, v in enc.items()})
    sd.update({"encoder." + k: v for k, v in enc.items() if k.startswith("norm.")})
    return sd, enc


def _encoder(precision, depth, enc_sd, offset, bottleneck=True):
    from pixelspointspolygons_amd.config import make_config
    from pixelspointspolygons_amd.vision_transformer import ViTDINOv2
    cfg = make_config("vit_dinov2", precision=precision, device=DEV, vit_depth=depth)
    m = ViTDINOv2(cfg, bottleneck=bottleneck, interpolate_offset=offset)
    sd = {"vit." + k: v for k, v in enc_sd.items()}
    sd.update({k: v for k, v in enc_sd.items() if k.startswith("norm.")})
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


def _model(precision, depth, sd, n_vertices=NV):
    from pixelspointspolygons_amd.config import make_config
    from pixelspointspolygons_amd.pix2poly import Pix2PolyModel, Tokenizer
    cfg = make_config("vit_dinov2", precision=precision, device=DEV, vit_depth=depth, max_num_vertices=n_vertices)
    m = Pix2PolyModel(cfg, Tokenizer(cfg).vocab_size, 0)
    m.load_state_dict(sd, strict=True)
    return m, cfg


# ---------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("P,ldk", [(14, 608), (14, 640), (8, 192), (8, 256)])
def test_padded_patchify(dtype, P, ldk):
    import pixelspointspolygons_amd.hip as h
    img = torch.rand(3, 3, 16 * P, 16 * P, generator=torch.Generator().manual_seed(P)).to(DEV)
    K = 3 * P * P
    dense = h.patchify(img, P, dtype)
    out = h.patchify_ld(img, P, dtype, ldk)
    assert tuple(out.shape) == (3 * 256, ldk)
    assert torch.equal(out[:, :K], dense)
    assert ldk == K or bool((out[:, K:] == 0).all())
    ref = F.unfold(img.cpu(), P, stride=P).transpose(1, 2).reshape(-1, K).to(dtype)          # and the dense entry is the im2col of the conv
    assert torch.equal(dense.cpu(), ref)
    from pixelspointspolygons_amd._lib import P3Error
    with pytest.raises(P3Error):
        h.patchify_ld(img, P, dtype, K - 4)


@pytest.mark.parametrize("offset", [0.0, 0.1])
def test_posembed_resample_forward_backward(offset):
    import pixelspointspolygons_amd.hip as h
    from pixelspointspolygons_amd.vision_transformer import resample_taps
    g = torch.Generator().manual_seed(5)
    table = torch.randn(1, 1370, 384, generator=g)
    dout = torch.randn(1, 257, 384, generator=g)
    t64 = table.double().requires_grad_(True)
    ref = R.resample_pos(t64, 16, offset)
    ref.backward(dout.double())
    taps = resample_taps(37, 16, offset, torch.device(DEV))
    assert taps.dtype == torch.float32 and tuple(taps.shape) == (16, 37)
    out = h.posembed_resample(table[0].to(DEV), taps, taps, 37, 16)
    dt = h.posembed_resample_bwd(dout[0].to(DEV), taps, taps, 37, 16)
    e_f, e_b = rel_err(out.cpu(), ref[0].detach()), rel_err(dt.cpu(), t64.grad[0])
    print(f"[offset {offset}] resample forward rel err {e_f:.2e}, backward {e_b:.2e}")
    assert e_f <= 1e-5 and e_b <= 1e-5
    assert torch.equal(out[0].cpu(), table[0, 0]) and torch.equal(dt[0].cpu(), dout[0, 0])          # the CLS row passes through in both directions
    untouched = (t64.grad[0].abs().sum(-1) == 0)
    assert bool((dt.cpu()[untouched] == 0).all())
    assert torch.equal(out, h.posembed_resample(table[0].to(DEV), taps, taps, 37, 16))             # two runs: the same bits
    assert torch.equal(dt, h.posembed_resample_bwd(dout[0].to(DEV), taps, taps, 37, 16))
    # upsampling (many outputs per source cell in the transposed gather)
    taps_up = resample_taps(16, 37, offset, torch.device(DEV))
    small = torch.randn(1, 257, 384, generator=g)
    s64 = small.double().requires_grad_(True)
    ref_up = R.resample_pos(s64, 37, offset)
    gup = torch.randn(1, 1370, 384, generator=g)
    ref_up.backward(gup.double())
    assert rel_err(h.posembed_resample(small[0].to(DEV), taps_up, taps_up, 16, 37).cpu(), ref_up[0].detach()) <= 1e-5
    assert rel_err(h.posembed_resample_bwd(gup[0].to(DEV), taps_up, taps_up, 16, 37).cpu(), s64.grad[0]) <= 1e-5


@pytest.mark.parametrize("N,K", [(384, 384), (384, 1536), (130, 36)])
def test_layerscale_fold_and_backward(N, K):
    import pixelspointspolygons_amd.hip as h
    g = torch.Generator().manual_seed(N + K)
    gamma = 0.05 + 1.45 * torch.rand(N, generator=g)
    gamma[::7] = 0.0                                       # checkpoints hold values near zero: dgamma must not come from a division by gamma
    gamma[3::7] = 1e-6
    W, b = torch.randn(N, K, generator=g) * 0.05, torch.randn(N, generator=g) * 0.02
    dWf, dbf = torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    Wf, bf = h.layerscale_fold(gamma.to(DEV), W.to(DEV), b.to(DEV))
    assert torch.equal(Wf.cpu(), gamma[:, None] * W) and torch.equal(bf.cpu(), gamma * b)
    dW, db, dg = h.layerscale_fold_bwd(gamma.to(DEV), W.to(DEV), b.to(DEV), dWf.to(DEV), dbf.to(DEV))
    for t in (dW, db, dg):
        assert bool(torch.isfinite(t).all())
    g64, W64, b64 = gamma.double().requires_grad_(True), W.double().requires_grad_(True), b.double().requires_grad_(True)
    ((g64[:, None] * W64) * dWf.double()).sum().add((g64 * b64 * dbf.double()).sum()).backward()
    bound = 1e-5 * ((dWf.double() * W.double()).abs().sum(1) + (dbf.double() * b.double()).abs())
    err = (dg.cpu().double() - g64.grad).abs()
    print(f"[{N}x{K}] dgamma worst |err| / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    assert rel_err(dW.cpu(), W64.grad) <= 1e-6 and rel_err(db.cpu(), b64.grad) <= 1e-6
    assert bool((dW.cpu()[::7] == 0).all())
    dW2, db2, dg2 = h.layerscale_fold_bwd(gamma.to(DEV), W.to(DEV), b.to(DEV), dWf.to(DEV), dbf.to(DEV))
    assert torch.equal(dg, dg2) and torch.equal(dW, dW2)


def test_autograd_of_the_fold_hands_on_all_three_gradients():
    from pixelspointspolygons_amd.vision_transformer import LayerScale
    ls = LayerScale(384, 1.0).to(DEV)
    lin = torch.nn.Linear(384, 384).to(DEV)
    with torch.no_grad():
        ls.gamma.copy_(torch.rand(384))
        ls.gamma[5] = 0.0
    wf, bf = ls.fold(lin.weight, lin.bias)
    gw, gb = torch.randn_like(wf), torch.randn_like(bf)
    ((wf * gw).sum() + (bf * gb).sum()).backward()
    assert rel_err(lin.weight.grad.cpu(), (ls.gamma.detach()[:, None] * gw).cpu()) < 1e-6
    assert rel_err(ls.gamma.grad.cpu(), ((gw * lin.weight.detach()).sum(1) + gb * lin.bias.detach()).cpu()) < 1e-5
    assert rel_err(lin.bias.grad.cpu(), (ls.gamma.detach() * gb).cpu()) < 1e-6


def test_folded_weight_is_never_served_stale_and_leaves_nothing_behind():
    """ops.shadow / the planes cache key a derived (non-parameter) weight by identity: a new gamma must reach the GEMM on the next forward, and the copies of
    the previous step's folded weight must not pile up"""
    from pixelspointspolygons_amd import ops
    from pixelspointspolygons_amd.vision_transformer import Block
    blk = Block(384, 6, 1536, 1e-6, init_values=1.0).to(DEV)
    x = torch.randn(2, 257, 384, device=DEV)
    sizes = []
    with torch.no_grad():
        y1 = blk.run(x, torch.bfloat16)
        for i in range(4):
            blk.ls1.gamma.mul_(0.5)
            blk.ls2.gamma.mul_(0.5)
            y2 = blk.run(x, torch.bfloat16)
            sizes.append((len(ops._shadow_cache), len(ops._planes_cache)))
        blk.ls1.gamma.zero_()
        blk.ls2.gamma.zero_()
        y0 = blk.run(x, torch.bfloat16)
    assert not torch.equal(y1, y2)
    assert torch.equal(y0, x)                                   # gamma = 0: both branches vanish exactly
    assert sizes[-1] == sizes[0], sizes


# ---------------------------------------------------------------------------------------------------------------- encoder forward
@pytest.mark.parametrize("precision", ["fp32", "fp32x3", "bf16"])
def test_encoder_forward_full_depth_vs_restatement_and_independent_fixture(precision):
    """depth 12 on the fixture's image: tokens (no bottleneck) against transformers.Dinov2Model's for interpolate_offset = 0.0 (the form the fixture pins),
    pooled features against the float64 restatement for both offsets, batch 1 and batch 3 (3 * 257 = 771 rows: no multiple of 128)."""
    d, _ = load_golden("dinov2_hf_s14.npz")
    enc_sd = R.make_state_dict(R.DINO_S14, seed=42)
    wsum = float(sum(v.double().sum() for v in enc_sd.values() if v.is_floating_point()))
    assert abs(wsum - float(d["wsum"][0])) < 1e-6 * abs(wsum) + 1e-6, "torch RNG drifted: regenerate fixtures"
    img1 = d["image"].float()
    img3 = torch.cat([img1, torch.rand(2, 3, 224, 224, generator=torch.Generator().manual_seed(2))], 0)
    sd64 = {k: v.double() for k, v in enc_sd.items()}
    m = _encoder(precision, 12, enc_sd, 0.0).eval()
    tol = TOL[precision]
    with torch.no_grad():
        m.out_dim = None                                          # tokens before the bottleneck ...
        tok = m(img1.to(DEV)).float().cpu()
        e = rel_err(tok[:, ::4, :], d["tokens"])
        print(f"[{precision}] tokens vs Dinov2Model (offset 0.0): {e:.3e}")
        assert e < tol
        m.out_dim = 256                                           # ... and the encoder as Pix2Poly uses it
        for off in (0.0, 0.1):
            m.vit.interpolate_offset = off
            ref = R.encoder(sd64, img3.double(), off)
            got3 = m(img3.to(DEV)).float().cpu()
            got1 = m(img1.to(DEV)).float().cpu()
            e3, e1 = rel_err(got3, ref), rel_err(got1, ref[:1])
            print(f"[{precision}] encoder vs float64 restatement, offset {off}: batch 3 {e3:.3e}, batch 1 {e1:.3e}")
            assert tuple(got3.shape) == (3, 256, 256) and e3 < tol and e1 < tol
        other = R.encoder(sd64, img1.double(), 0.0)
        assert rel_err(got1, other) > 3 * tol if precision != "bf16" else True      # the two conventions are told apart at this tolerance


# ---------------------------------------------------------------------------------------------------------------- backward
def _grad_errs(precision, named, ref):
    out = {}
    gmax = max(float(g.abs().max()) for g in ref.values())
    gnorm = max(float(g.norm()) for g in ref.values())
    for k, g in named.items():
        g, r = g.float().cpu(), ref[k]
        if precision != "bf16":
            out[k] = l2_err(g, r, floor=1e-3 * gnorm)
        elif float(r.abs().max()) > 1e-3 * gmax:
            cos = float((g * r).sum() / (g.norm() * r.norm()).clamp_min(1e-30))
            out[k] = max(1.0 - cos, abs(float(g.norm() / r.norm()) - 1.0) * 0.25)
        else:
            out[k] = float((g - r).abs().max()) / (1e-1 * gmax)
    return out


WATCH = ["blocks.0.ls1.gamma", "blocks.1.ls2.gamma", "pos_embed", "patch_embed.proj.weight", "blocks.1.attn.qkv.weight", "blocks.0.attn.proj.weight",
         "blocks.1.mlp.fc2.bias", "cls_token"]


@pytest.mark.parametrize("precision", ["fp32", "fp32x3", "bf16"])
def test_encoder_backward_vs_float64_autograd(precision):
    enc_sd = R.make_state_dict(_vc(2), seed=11)
    img = torch.rand(3, 3, 224, 224, generator=torch.Generator().manual_seed(4))
    G = torch.randn(3, 256, 256, generator=torch.Generator().manual_seed(6))
    p64 = {k: v.double().requires_grad_(True) for k, v in enc_sd.items()}
    (R.encoder(p64, img.double(), 0.1) * G.double()).sum().backward()
    m = _encoder(precision, 2, enc_sd, 0.1).train()
    out = m(img.to(DEV))
    (out.float() * G.to(DEV)).sum().backward()
    named = dict(m.vit.named_parameters())
    errs = _grad_errs(precision, {k: named[k].grad for k in WATCH}, {k: p64[k].grad for k in WATCH})
    print(f"[{precision}] encoder gradients vs float64: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v < GTOL[precision] for v in errs.values()), errs
    gp, rp = named["pos_embed"].grad.cpu(), p64["pos_embed"].grad
    assert tuple(gp.shape) == (1, 1370, 384)
    assert bool((gp[0][rp[0].abs().sum(-1) == 0] == 0).all())           # rows the 16 x 16 grid never taps: exactly zero
    assert named["mask_token"].grad is None


@pytest.mark.parametrize("precision", ["fp32", "fp32x3"])
def test_full_model_backward_vs_float64_autograd(precision):
    """whole Pix2PolyModel (2 DINOv2 blocks, 6 decoder layers, 24 vertices): CE + 10 * BCE, the encoder's gradients against float64 autograd through the
    restatement + the oracle's decoder / ScoreNet / Sinkhorn"""
    from pixelspointspolygons_amd.training import pix2poly_loss
    sd, enc_sd = full_state_dict(2, seed=13)
    inp = O.make_inputs(2, seed=17, n_vertices=NV, min_verts=4)
    m, cfg = _model(precision, 2, sd)
    m.train()
    m.decoder.set_dropout(0.0)
    m.scorenet1.debug_keep = m.scorenet2.debug_keep = True
    d = {k: v.to(DEV) for k, v in inp.items()}
    logits, perm = m(d["image"], None, d["y"][:, :-1])
    loss = pix2poly_loss(logits, perm, d["y"][:, 1:], d["y_perm"])[0]
    loss.backward()
    p64 = {k: (v.double().requires_grad_(True) if v.is_floating_point() and "running" not in k else (v.double() if v.is_floating_point() else v.clone()))
           for k, v in sd.items()}
    enc = R.encoder(p64, inp["image"].double(), 0.1, prefix="encoder.vit.")
    rl, feats = O.decoder_forward(enc, inp["y"][:, :-1], p64)
    # float64 is evaluated AT the product's ScoreNet ReLU decisions, checked to differ from float64's own only at the kink: exactly what
    # test_train_step_gradients_vs_oracle_autograd does for the early-fusion model (a flipped decision is ~3e-4 of every upstream gradient, not arithmetic)
    from tests.test_backward_gpu import _assert_kink_only, _model_scorenet_decisions
    dec, zs = _model_scorenet_decisions(m, 2, NV), {"scorenet1.": [], "scorenet2.": []}
    scores = O.scorenet(feats, p64, "scorenet1.", n_vertices=NV, training=True, decisions=dec["scorenet1."], zs_out=zs["scorenet1."]) + \
        O.scorenet(feats, p64, "scorenet2.", n_vertices=NV, training=True, decisions=dec["scorenet2."], zs_out=zs["scorenet2."]).transpose(1, 2)
    _assert_kink_only(dec, zs, *((1e-3, 4096) if precision == "fp32x3" else (1e-4, 1024)))
    rperm = torch.softmax(O.log_optimal_transport(scores, p64["bin_score"], 100)[:, :NV, :NV], -1)
    ref_loss = O.pix2poly_loss(rl, rperm, inp["y"][:, 1:], inp["y_perm"].double())[0]
    ref_loss.backward()
    assert abs(float(loss.detach()) - float(ref_loss.detach())) < 2e-3 * abs(float(ref_loss.detach()))
    named = dict(m.named_parameters())
    keys = ["encoder.vit." + k for k in WATCH]
    errs = _grad_errs(precision, {k: named[k].grad for k in keys}, {k: p64[k].grad for k in keys})
    print(f"[{precision}] whole-model gradients vs float64: " + ", ".join(f"{k[12:]} {v:.2e}" for k, v in errs.items()))
    assert all(v < GTOL[precision] for v in errs.values()), errs


def test_captured_train_step_fp32x3_is_bit_reproducible_and_stays_off_the_planes_stack(monkeypatch):
    """two eager steps, then the step captured in a hipGraph and replayed twice (FlatAdamW arenas, gradients accumulated in place): every loss finite and the
    same bits in two runs; fp32x3 blocks with LayerScale run Block.run, never ops_x3.vit_stack"""
    from pixelspointspolygons_amd import ops, ops_x3
    from pixelspointspolygons_amd.training import FlatAdamW, pix2poly_loss
    calls = []
    real = ops_x3.vit_stack
    monkeypatch.setattr(ops_x3, "vit_stack", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    # the shipped 192 vertices: at 24 the decoder's LayerNorm parameter gradients are not bit-reproducible in any model (measured; not this encoder's kernels)
    sd, _ = full_state_dict(2, seed=19, n_vertices=O.MAX_VERTS)
    inp = {k: v.to(DEV) for k, v in O.make_inputs(2, seed=23).items()}

    def run():
        ops.reset_process_state()
        m, cfg = _model("fp32x3", 2, sd, n_vertices=O.MAX_VERTS)
        m.train()
        opt = FlatAdamW(m, lr=3e-4, compute_dtype=torch.float32)
        ops.manual_seed(99, DEV)
        losses, gammas = [], None

        def fwd_bwd():
            opt.zero_grad()
            ops.advance_rng(DEV)
            logits, perm = m(inp["image"], None, inp["y"][:, :-1])
            loss = pix2poly_loss(logits, perm, inp["y"][:, 1:], inp["y_perm"])[0]
            loss.backward()
            return loss.detach()
        for _ in range(2):
            opt.prepare_step()
            out = fwd_bwd()
            opt.apply(1.0)
            losses.append(out.clone())
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        opt.prepare_step()
        with torch.cuda.graph(graph):
            out = fwd_bwd()
            opt.apply(1.0)
        graph.replay()
        losses.append(out.clone())
        opt.prepare_step()
        graph.replay()
        losses.append(out.clone())
        torch.cuda.synchronize()
        gammas = m.encoder.vit.blocks[1].ls1.gamma.detach().clone()
        del graph
        opt.close()
        return torch.stack(losses).cpu(), gammas.cpu()
    (la, ga), (lb, gb) = run(), run()
    ops.reset_process_state()
    print("losses", la.tolist())
    assert bool(torch.isfinite(la).all()) and torch.equal(la, lb) and torch.equal(ga, gb)
    assert len(set(la.tolist())) == 4                                  # the weights moved: every step sees the updated (re-folded) weights
    assert not torch.equal(ga, sd["encoder.vit.blocks.1.ls1.gamma"])     # gamma is trained
    assert not calls


# ---------------------------------------------------------------------------------------------------------------- decode
def greedy_reference(seed, depth=2):
    """the oracle's literal greedy loop (Pix2PolyPredictor.test_generate) on the restatement's encoder output, keeping its relative top-2 margins"""
    sd, enc_sd = full_state_dict(depth, seed=seed)
    img = torch.rand(1, 3, 224, 224, generator=torch.Generator().manual_seed(seed + 100))
    with torch.no_grad():
        ref_enc = R.encoder(enc_sd, img, 0.1)
        preds = torch.full((1, 1), O.BOS, dtype=torch.long)
        margins = []
        for _ in range(2 * NV + 1):
            logits, _f = O.decoder_predict(ref_enc, preds, sd, max_len=2 * NV + 2)
            top2 = logits[0].float().topk(2).values
            margins.append(float(top2[0] - top2[1]) / max(1.0, float(top2[0].abs())))
            preds = torch.cat([preds, torch.softmax(logits, -1).argmax(-1, keepdim=True)], 1)
    return sd, img, preds, margins


@pytest.mark.parametrize("precision", ["fp32", "fp32x3"])
def test_greedy_decode_with_256_memory_tokens_equals_the_oracles_loop(precision):
    """two-block DINOv2 model, fused decode layer, 49 greedy steps against the oracle's loop fed with the restatement's encoder output; tokens must be equal
    up to the first step where the ORACLE's own top-2 margin falls below the mode's logit noise (tests/test_model_gpu.py: 1e-5 fp32, 2e-4 fp32x3).
    GREEDY_SEED was picked on the CPU (python tests/test_dinov2_gpu.py) so that the reference's margins allow at least 90 % of the steps to be compared."""
    sd, img, preds, margins = greedy_reference(GREEDY_SEED)
    m, cfg = _model(precision, 2, sd)
    m.eval()
    with torch.no_grad():
        enc = m.encoder(img.to(DEV))
        assert tuple(enc.shape) == (1, 256, 256)
        toks, _ = m.generate(enc)
    steps = 2 * NV + 1
    noise = 1e-5 if precision == "fp32" else 2e-4
    low = [k for k, mg in enumerate(margins) if mg < noise]
    upto = (low[0] + 1) if low else steps + 1
    print(f"\n[{precision}] oracle's first near-tie (margin < {noise:g}) at step {low[0] if low else None} of {steps}; tokens compared: {upto}")
    assert tuple(toks.shape) == (1, steps + 1)
    assert upto - 1 >= 0.9 * steps
    assert torch.equal(toks[:, :upto].cpu(), preds[:, :upto]), int((toks[0, :upto].cpu() != preds[0, :upto]).nonzero()[0])


if __name__ == "__main__":           # CPU: list candidate seeds for GREEDY_SEED with the number of steps their margins allow at the fp32x3 noise figure
    for s in range(1, 13):
        _sd, _img, _p, mg = greedy_reference(s)
        low = [k for k, v in enumerate(mg) if v < 2e-4]
        print(s, "first near-tie:", low[0] if low else None, "min margin %.2e" % min(mg), "distinct tokens", len(set(_p[0].tolist())))
