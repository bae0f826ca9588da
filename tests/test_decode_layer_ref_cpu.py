"""tests/decode_layer_ref.py is what the direct p3_decode_layer tests compare with: here it is proven equal to torch.nn.TransformerDecoderLayer
in float64, and the one-hot key probes of the GPU tests are proven sensitive - a kernel that lost the probed key could not pass."""
import math

import pytest
import torch

from tests import decode_layer_ref as R

EPS = 1e-5


@pytest.mark.parametrize("Lmem", [1, 16, 100])
@pytest.mark.parametrize("t", [0, 5, 70])
def test_reference_equals_torch_decoder_layer(t, Lmem):
    torch.manual_seed(1000 * t + Lmem)
    B, D = 3, R.D
    layer = torch.nn.TransformerDecoderLayer(D, R.H, R.FF, dropout=0.0, batch_first=True).double().eval()
    with torch.no_grad():
        for p in layer.parameters():                     # non-trivial biases and LayerNorm parameters
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    tgt = 0.5 * torch.randn(B, t + 1, D, dtype=torch.float64)
    memory = 0.5 * torch.randn(B, Lmem, D, dtype=torch.float64)
    key_bias = torch.randn(B, t + 1, dtype=torch.float64)
    causal = torch.full((t + 1, t + 1), float("-inf"), dtype=torch.float64).triu(1)
    with torch.no_grad():
        want = layer(tgt, memory, tgt_mask=causal, tgt_key_padding_mask=key_bias)[:, t]
        sa, ca = layer.self_attn, layer.multihead_attn
        # caches from the module's own in-projections; only the k|v columns of the rows in front of t are read
        kv_self = torch.nn.functional.linear(tgt, sa.in_proj_weight, sa.in_proj_bias)
        kv_self[:, t:] = float("nan")
        kv_self[:, :, :D] = float("nan")
        kv_mem = torch.nn.functional.linear(memory, ca.in_proj_weight[D:], ca.in_proj_bias[D:])
        w = dict(w_in=sa.in_proj_weight, b_in=sa.in_proj_bias, w_so=sa.out_proj.weight, b_so=sa.out_proj.bias,
                 w_q=ca.in_proj_weight[:D], b_q=ca.in_proj_bias[:D], w_co=ca.out_proj.weight, b_co=ca.out_proj.bias,
                 w1=layer.linear1.weight, b1=layer.linear1.bias, w2=layer.linear2.weight, b2=layer.linear2.bias,
                 g1=layer.norm1.weight, be1=layer.norm1.bias, g2=layer.norm2.weight, be2=layer.norm2.bias, g3=layer.norm3.weight, be3=layer.norm3.bias)
        got = R.decode_layer_ref(tgt[:, t], kv_self, kv_mem, key_bias, t, {k: v.detach() for k, v in w.items()}, layer.norm1.eps)
    assert torch.isfinite(got["out"]).all()
    assert float((got["out"] - want).abs().max() / want.abs().max()) < 1e-12


def test_bfloat16_rounding_happens_at_the_stage_outputs_only():
    w = R.make_weights(torch.bfloat16)
    case = R.make_case(2, 5, 16, torch.bfloat16, seed=1)
    plain = R.decode_layer_ref(case["x"], case["kv_self"], case["kv_mem"], None, 5, w, EPS)
    r = R.case_ref(case, w, EPS)
    for k in ("qkv", "x1", "x2", "out", "q_mem"):
        assert torch.equal(r[k], R.rounded(r[k], torch.bfloat16)), k
    assert torch.equal(r["qkv"], R.rounded(plain["qkv"], torch.bfloat16))         # the first rounding point: the same arithmetic in front of it
    assert 0 < float(R.rel_err(r["out"], plain["out"]).max()) < R.OUT_TOL[torch.bfloat16]


def _sensitivity(case, jstar, w, where):
    """the probed key holds the softmax (all other keys together: less than 832 e^-20 of the weight, so the attention output is the probed value
    row), and the output moves when it is lost"""
    r = R.case_ref(case, w, EPS)
    ref = r["out"]
    if where == "drop_mem":
        vals, a = case["kv_mem"][..., R.D:], r["a_mem"]
    else:
        vals, a = torch.cat([case["kv_self"][..., 2 * R.D:], r["qkv"][:, None, 2 * R.D:]], 1), r["a_self"]
    probed = vals[torch.arange(len(jstar)), jstar]
    slack = 832 * math.exp(-20.0) * 2 * vals.abs().amax((1, 2))[:, None] + (2.0 ** -8 * probed.abs() if case["dt"] == torch.bfloat16 else 0.0)
    assert bool(((a - probed).abs() <= slack).all())
    lost = R.case_ref(case, w, EPS, **{where: jstar})["out"]
    return R.rel_err(lost, ref)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("Lmem", [784, 832])
def test_memory_probes_decide_the_output(Lmem, dt):
    w = R.make_weights(dt)
    case, jstar = R.mem_probe_case(Lmem, dt, w, EPS)
    assert len(set(jstar.tolist())) == 9
    moved = _sensitivity(case, jstar, w, "drop_mem")
    assert float(moved.min()) > 10 * R.OUT_TOL[dt], moved


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_position_probes_decide_the_output(dt):
    w = R.make_weights(dt)
    case, jstar = R.self_probe_case(dt, w, EPS)
    assert len(set(jstar.tolist())) == 9 and int(jstar[-1]) == case["t"]
    moved = _sensitivity(case, jstar, w, "drop_self")
    assert float(moved.min()) > 10 * R.OUT_TOL[dt], moved
