"""Direct tests of the glue, layout and loss kernels: each hip.py wrapper against a plain float64 (or same-order fp32) CPU reference, at
ragged shapes, both dtypes, every dispatch form (asserted by kernel name) and both reduction paths (atomics / deterministic slabs)."""
import contextlib
import math
from ctypes import c_int, c_int64

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 7.0


def _h():
    import pixelspointspolygons_amd.hip as h
    return h


def _lib():
    from pixelspointspolygons_amd._lib import lib
    return lib()


def _rand(*shape, seed=0, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale + shift


def _q(t, dtype):
    """the values the kernel sees: t rounded to dtype, back in float64 for the reference"""
    return t.to(dtype).double()


def assert_bf16_ulp(got, ref, floor_rel=1e-6):
    """bf16 output within one rounding of the float64 reference: |got - ref| <= 2^-8 |ref| (+ a floor relative to the tensor's scale)"""
    g, r = got.double().cpu(), ref.double().cpu()
    floor = floor_rel * float(r.abs().max().clamp_min(1e-30))
    bad = (g - r).abs() > 2.0 ** -8 * r.abs() + floor
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} elements off by more than 1 bf16 ulp; worst {float(((g - r).abs() - 2.0 ** -8 * r.abs()).max()):.3e}"


def check(got, ref, dtype, tol):
    """fp32: rel_err <= tol against float64; bf16: one ulp per element"""
    if dtype == torch.bfloat16:
        assert got.dtype == torch.bfloat16
        assert_bf16_ulp(got, ref, floor_rel=max(tol, 1e-6))
    else:
        assert got.dtype == torch.float32
        e = rel_err(got.cpu(), ref)
        assert e <= tol, e


@contextlib.contextmanager
def traced():
    h = _h()
    h.KTIMER.enable()
    try:
        yield lambda: _lib().p3_last_kernel().decode()
    finally:
        h.KTIMER.disable()


@pytest.fixture
def det():
    """set the deterministic level for one test; the previous level comes back afterwards"""
    h = _h()
    prev = h.DETERMINISTIC
    yield h.set_deterministic
    h.set_deterministic(prev)


def _affine(C, seed):
    return _rand(C, seed=seed, scale=0.5) + 1.0, _rand(C, seed=seed + 1, scale=0.3)


def _misaligned(t, off=1):
    """a copy of t whose storage starts `off` elements into its buffer (not 16-byte aligned)"""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)
    v = buf[off:].view(t.shape)
    v.copy_(t)
    return v


DTYPES = [torch.float32, torch.bfloat16]


# ------------------------------------------------------------------------------------------------ upsample_bilinear (+ bwd)
UP_SIZES = [(28, 28, 224, 224), (14, 14, 224, 224), (28, 28, 56, 56), (28, 28, 28, 28), (5, 5, 7, 7), (7, 7, 20, 20), (10, 10, 15, 15),
            (100, 100, 150, 150)]


def _up_tol(h, w, tol):
    """the source coordinate (o + 0.5) * h / H - 0.5 is an fp32 value (as in torch's fp32 path): its rounding, up to 2^-23 * max(h, w), moves
    the bilinear weights by as much"""
    return max(tol, 1e-6 + 2.0 ** -22 * max(h, w))


def _up_ref(tok, B, h, w, H, W, tok_off):
    C = tok.shape[-1]
    x = tok[:, tok_off:].reshape(B, h, w, C).permute(0, 3, 1, 2)
    return F.interpolate(x, size=(H, W), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h,w,H,W", UP_SIZES + [(6, 10, 16, 25), (9, 4, 12, 31)])
def test_upsample_bilinear(dtype, h, w, H, W):
    hh = _h()
    B, C, ld = 2, 8, 12
    for tok_off in (0, 1):
        tok = _rand(B, tok_off + h * w, C, seed=h * 7 + W)
        out = torch.full((B, H, W, ld), SENT, dtype=dtype, device=DEV)
        hh.upsample_bilinear(tok.to(dtype).to(DEV), B, h, w, H, W, out, tok_off=tok_off)
        ref = _up_ref(_q(tok, dtype), B, h, w, H, W, tok_off)
        check(out[..., :C], ref, dtype, _up_tol(h, w, 1e-6))
        assert bool((out[..., C:] == SENT).all()), "channels >= C written"


def _up_bwd_call(dUp, B, h, w, H, W, tok_off, dtok):
    hh = _h()
    C = dUp.shape[-1]
    tmp = torch.empty((B, H, w, C), dtype=torch.float32, device=DEV)
    hh.check(_lib().p3_upsample_bilinear_bwd(hh.ptr(dUp), c_int(hh.dt(dUp)), hh.ptr(tmp), hh.ptr(dtok), c_int(B), c_int(h), c_int(w), c_int(C),
                                             c_int(H), c_int(W), c_int(tok_off), c_int(tok_off + h * w), hh.stream()), "p3_upsample_bilinear_bwd")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h,w,H,W", UP_SIZES)
def test_upsample_bilinear_bwd(dtype, h, w, H, W):
    B, C = 2, 8
    for tok_off in (0, 1):
        dUp = _rand(B, H, W, C, seed=H + w)
        dtok = torch.full((B, tok_off + h * w, C), SENT, dtype=dtype, device=DEV)
        _up_bwd_call(dUp.to(dtype).to(DEV), B, h, w, H, W, tok_off, dtok)
        tok = torch.zeros(B, tok_off + h * w, C, dtype=torch.float64, requires_grad=True)
        _up_ref(tok, B, h, w, H, W, tok_off).backward(_q(dUp, dtype))
        check(dtok[:, tok_off:], tok.grad[:, tok_off:], dtype, _up_tol(h, w, 1e-5))
        assert bool((dtok[:, :tok_off] == SENT).all()), "token rows before tok_off written"
    # the wrapper: rows before tok_off come back zero
    out = _h().upsample_bilinear_bwd(dUp.to(dtype).to(DEV), B, h, w, H, W, tok_off=1)
    assert bool((out[:, 0] == 0).all())
    check(out[:, 1:], tok.grad[:, 1:], dtype, _up_tol(h, w, 1e-5))


# ------------------------------------------------------------------------------------------------ head1x1 (+ bwd)
HEAD_CASES = [(1, 0, 1.0), (4, 1, 2.0)]        # (n_out, act, post_mul) as ffl.py passes them: segmentation sigmoid, crossfield 2*tanh


def _head_ref(x, s, b, Wt, bias, act, post):
    z = torch.relu(x * s + b)
    y = z @ Wt.t() + bias
    return (torch.sigmoid(y) if act == 0 else torch.tanh(y)) * post


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_out,act,post", HEAD_CASES)
@pytest.mark.parametrize("B,HW", [(2, 100), (1, 224 * 224)])
def test_head1x1(dtype, n_out, act, post, B, HW):
    hh = _h()
    R, ld = B * HW, 264
    x = _rand(R, ld, seed=3)
    s, b = _affine(256, 4)
    Wt, bias = _rand(n_out, 256, seed=6, scale=0.1), _rand(n_out, seed=7)
    xd = x.to(dtype).to(DEV)
    ref = _head_ref(_q(x, dtype)[:, :256], s.double(), b.double(), Wt.double(), bias.double(), act, post)     # [R, n_out]
    ref_nchw = ref.reshape(B, HW, n_out).permute(0, 2, 1)
    args = (xd, ld, s.to(DEV), b.to(DEV), Wt.to(DEV), bias.to(DEV), act, post, B, HW)
    out = hh.head1x1(*args)
    assert rel_err(out.cpu(), ref_nchw) <= 1e-5
    cd = torch.full((R, 5), SENT, dtype=dtype, device=DEV)
    out2 = hh.head1x1(*args, copy_dst=cd, copy_ld=5)
    assert torch.equal(out2, out)
    assert torch.equal(cd[:, 0].cpu(), out.permute(0, 2, 1).reshape(R, n_out)[:, 0].to(dtype).cpu())
    assert bool((cd[:, 1:] == SENT).all())


def _bn_relu_bwd_ref(dA, H, s, b, mean):
    """dz = dA * [H*s + b > 0] -> (dHd = dz*s, centred dscale = sum dz*(H - mean), dshift = sum dz)"""
    dz = dA * ((H * s + b) > 0)
    return dz * s, (dz * (H - mean)).sum(0), dz.sum(0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_out,act,post", HEAD_CASES)
@pytest.mark.parametrize("level", [0, 1, 2])
def test_head1x1_bwd(det, dtype, n_out, act, post, level):
    det(level)
    hh = _h()
    B, HW = 2, 300
    R = B * HW
    H = _rand(R, 256, seed=11)
    s, b = _affine(256, 12)
    mean = _rand(256, seed=14, scale=0.1)
    Wt, bias = _rand(n_out, 256, seed=15, scale=0.1), _rand(n_out, seed=16)
    Hq = _q(H, dtype)
    pre = (Hq * s.double() + b.double()).requires_grad_(True)
    Wr = Wt.double().requires_grad_(True)
    br = bias.double().requires_grad_(True)
    y = torch.relu(pre) @ Wr.t() + br
    y = (torch.sigmoid(y) if act == 0 else torch.tanh(y)) * post
    dout = _rand(R, n_out, seed=17)
    y.backward(dout.double())
    out_nchw = y.detach().float().reshape(B, HW, n_out).permute(0, 2, 1).contiguous()
    dout_nchw = dout.reshape(B, HW, n_out).permute(0, 2, 1).contiguous()
    dz = pre.grad
    runs = [hh.head1x1_bwd(H.to(dtype).to(DEV), s.to(DEV), b.to(DEV), mean.to(DEV), Wt.to(DEV), out_nchw.to(DEV), dout_nchw.to(DEV), act, post, B, HW)
            for _ in range(2)]
    dHd, acc = runs[0]
    check(dHd, dz * s.double(), dtype, 1e-5)
    acc = acc.cpu()
    assert rel_err(acc[:256], (dz * (Hq - mean.double())).sum(0)) <= 1e-5
    assert rel_err(acc[256:512], dz.sum(0)) <= 1e-5
    assert rel_err(acc[512:512 + n_out * 256], Wr.grad.reshape(-1)) <= 1e-5
    assert rel_err(acc[512 + n_out * 256:], br.grad) <= 1e-5
    if hh.det_on(H.to(dtype)):
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "deterministic launch gave different bits"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("R,ldh", [(2 * 49, 256), (3 * 333, 260)])
def test_affine_relu_bwd256(det, dtype, level, R, ldh):
    det(level)
    hh = _h()
    H, dA = _rand(R, ldh, seed=21), _rand(R, 256, seed=22)
    s, b = _affine(256, 23)
    mean = _rand(256, seed=25, scale=0.1)
    Hq, dAq = _q(H, dtype), _q(dA, dtype)
    rd, rs, rh = _bn_relu_bwd_ref(dAq, Hq[:, :256], s.double(), b.double(), mean.double())
    runs = []
    for _ in range(2):
        out = torch.full((R, 256), SENT, dtype=dtype, device=DEV)
        runs.append(hh.affine_relu_bwd256(dA.to(dtype).to(DEV), H.to(dtype).to(DEV), ldh, s.to(DEV), b.to(DEV), mean.to(DEV), R, out=out))
    out, acc = runs[0]
    check(out, rd, dtype, 1e-5)
    assert rel_err(acc[:256].cpu(), rs) <= 1e-5 and rel_err(acc[256:].cpu(), rh) <= 1e-5
    if hh.det_on(H.to(dtype)):
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "deterministic launch gave different bits"


# ------------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,C,HW,ld", [(2, 256, 28 * 28, 256), (2, 37, 45, 40), (1, 33, 1000, 33)])
@pytest.mark.parametrize("affine", [False, True])
def test_nhwc_to_nchw(dtype, B, C, HW, ld, affine):
    hh = _h()
    x = _rand(B * HW, ld, seed=31)
    s, b = _affine(C, 32) if affine else (None, None)
    out = hh.nhwc_to_nchw(x.to(dtype).to(DEV), ld, s.to(DEV) if affine else None, b.to(DEV) if affine else None, B, C, HW).cpu()
    xq = x.to(dtype).float()[:, :C]
    if affine:
        ref = torch.relu(xq.double() * s.double() + b.double())
        assert rel_err(out, ref.reshape(B, HW, C).permute(0, 2, 1)) <= 1e-6
    else:
        assert torch.equal(out, xq.reshape(B, HW, C).permute(0, 2, 1))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,C,H,W,ld", [(2, 256, 28, 28, 256), (2, 37, 5, 9, 40), (1, 33, 10, 13, 64)])
def test_nchw_to_nhwc(dtype, B, C, H, W, ld):
    hh = _h()
    x = _rand(B, C, H, W, seed=41)
    out = torch.full((B * H * W, ld), SENT, dtype=dtype, device=DEV)
    xd = x.to(DEV)
    hh.check(_lib().p3_nchw_to_nhwc(hh.ptr(xd), hh.ptr(out), c_int(ld), c_int(hh.dt(out)), c_int(B), c_int(C), c_int64(H * W), hh.stream()),
             "p3_nchw_to_nhwc")
    ref = x.permute(0, 2, 3, 1).reshape(B * H * W, C).to(dtype)
    assert torch.equal(out[:, :C].cpu(), ref)
    assert bool((out[:, C:] == SENT).all())
    w = hh.nchw_to_nhwc(x.to(DEV), dtype, ld=ld).cpu()                  # the wrapper zeroes the columns >= C
    assert torch.equal(w[:, :C], ref) and bool((w[:, C:] == 0).all())


# (dtype, C, c_aff, Cp, ld_src, misaligned, kernel)
PAD_CASES = [(torch.bfloat16, 256, 256, 264, 256, False, "pad_nhwc_vec_kernel"),          # hisup.py / ffl.py shape: Cp = C rounded up
             (torch.bfloat16, 32, 16, 40, 40, False, "pad_nhwc_vec_kernel"),
             (torch.float32, 32, 16, 36, 40, False, "pad_nhwc_kernel<float>"),
             (torch.float32, 30, 30, 32, 30, False, "pad_nhwc_kernel<float>"),
             (torch.bfloat16, 20, 20, 24, 20, False, "pad_nhwc_kernel<bf16>"),           # C % 8 != 0
             (torch.bfloat16, 32, 16, 40, 40, True, "pad_nhwc_kernel<bf16>")]             # source not 16-byte aligned


@pytest.mark.parametrize("dtype,C,c_aff,Cp,ld_src,mis,kernel", PAD_CASES)
@pytest.mark.parametrize("affine", [False, True])
def test_pad_nhwc(dtype, C, c_aff, Cp, ld_src, mis, kernel, affine):
    hh = _h()
    B, H, W = 2, 5, 7
    src = _rand(B * H * W, ld_src, seed=51)
    s, b = _affine(C, 52)
    sd = src.to(dtype).to(DEV)
    if mis:
        sd = _misaligned(sd)
    out = torch.full((B, H + 2, W + 2, Cp), SENT, dtype=dtype, device=DEV)
    with traced() as last:
        hh.pad_nhwc(sd, ld_src, s.to(DEV) if affine else None, b.to(DEV) if affine else None, c_aff if affine else 0, C, Cp, B, H, W, out=out)
        assert last() == kernel
    out = out.cpu()
    xq = _q(src, dtype)[:, :C].reshape(B, H, W, C)
    ref = torch.zeros(B, H + 2, W + 2, Cp, dtype=torch.float64)
    inner = xq.clone()
    if affine:
        inner[..., :c_aff] = torch.relu(xq[..., :c_aff] * s[:c_aff].double() + b[:c_aff].double())
    ref[:, 1:H + 1, 1:W + 1, :C] = inner
    # zero border and zero channel padding, whichever way the path clears them (one pass vs memset + interior)
    mask = torch.ones_like(ref, dtype=torch.bool)
    mask[:, 1:H + 1, 1:W + 1, :C] = False
    assert bool((out[mask] == 0).all()), "border / channel padding not zero"
    lo = c_aff if affine else 0
    assert torch.equal(out[:, 1:H + 1, 1:W + 1, lo:C], src.to(dtype)[:, lo:C].reshape(B, H, W, C - lo)), "plain-copy channels"
    if affine and c_aff:
        check(out[:, 1:H + 1, 1:W + 1, :c_aff].contiguous(), ref[:, 1:H + 1, 1:W + 1, :c_aff], dtype, 1e-6)


# ------------------------------------------------------------------------------------------------ HiSup: affine_relu_mix, eca_gate
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("gate_on", [False, True])
@pytest.mark.parametrize("second", [None, "plain", "affine"])
def test_affine_relu_mix(dtype, gate_on, second):
    hh = _h()
    B, HW, C, lda, ldb, ldo = 2, 49, 37, 40, 44, 48
    R = B * HW
    a, bsrc = _rand(R, lda, seed=61), _rand(R, ldb, seed=62)
    sa, ha = _affine(C, 63)
    sb, hb = _affine(C, 65)
    gate = torch.rand(B, C, generator=torch.Generator().manual_seed(67))
    out = torch.full((R, ldo), SENT, dtype=dtype, device=DEV)
    hh.affine_relu_mix(out, a.to(dtype).to(DEV), (sa.to(DEV), ha.to(DEV)), HW, C, gate=gate.to(DEV) if gate_on else None,
                       b=bsrc.to(dtype).to(DEV) if second else None, aff_b=(sb.to(DEV), hb.to(DEV)) if second == "affine" else None)
    ref = torch.relu(_q(a, dtype)[:, :C] * sa.double() + ha.double())
    if gate_on:
        ref = ref * gate.double().repeat_interleave(HW, 0)
    if second:
        v = _q(bsrc, dtype)[:, :C]
        ref = ref + (torch.relu(v * sb.double() + hb.double()) if second == "affine" else v)
    check(out[:, :C].contiguous(), ref, dtype, 1e-6)
    assert bool((out[:, C:] == SENT).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("B,HW,C,ld", [(2, 49, 100, 104), (2, 28 * 28, 256, 256)])
@pytest.mark.parametrize("level", [0, 2])
def test_eca_gate(det, dtype, k, B, HW, C, ld, level):
    det(level)
    hh = _h()
    a1, a2 = _rand(B * HW, ld, seed=71), _rand(B * HW, ld, seed=72)
    s1, h1 = _affine(C, 73)
    s2, h2 = _affine(C, 75)
    w = _rand(1, 1, k, seed=77, scale=0.5)
    args = (a1.to(dtype).to(DEV), (s1.to(DEV), h1.to(DEV)), a2.to(dtype).to(DEV), (s2.to(DEV), h2.to(DEV)), w.to(DEV), B, HW, C)
    g = hh.eca_gate(*args)
    x = torch.relu(_q(a1, dtype)[:, :C] * s1.double() + h1.double()) + torch.relu(_q(a2, dtype)[:, :C] * s2.double() + h2.double())
    pooled = x.reshape(B, HW, C).mean(1)
    ref = torch.sigmoid(F.conv1d(pooled.unsqueeze(1), w.double(), padding=k // 2)).squeeze(1)
    assert rel_err(g.cpu(), ref) <= 1e-5
    assert torch.equal(g, hh.eca_gate(*args)), "fixed-order pool gave different bits"


# ------------------------------------------------------------------------------------------------ ViT input / output glue
# (B, Cin, H, W, P, kernel-form)
PATCH_CASES = [(2, 3, 224, 224, 8, "rows"), (2, 3, 224, 224, 16, "rows"), (1, 3, 32, 48, 8, "rows"), (1, 5, 32, 48, 16, ""), (2, 17, 16, 24, 8, "")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,Cin,H,W,P,form", PATCH_CASES)
def test_patchify(dtype, B, Cin, H, W, P, form):
    hh = _h()
    img = _rand(B, Cin, H, W, seed=81)
    with traced() as last:
        out = hh.patchify(img.to(DEV), P, dtype)
        name = "patchify_rows_kernel" if form == "rows" else "patchify_kernel"
        assert last() == name + ("<bf16>" if dtype == torch.bfloat16 else "<float>")
    ref = img.reshape(B, Cin, H // P, P, W // P, P).permute(0, 2, 4, 1, 3, 5).reshape(B * (H // P) * (W // P), Cin * P * P)
    assert torch.equal(out.cpu(), ref.to(dtype))


# (np, D, src_ld, misaligned, form)
ASM_CASES = [(784, 384, 384, False, "rows"), (50, 64, 72, False, "rows"), (50, 30, 30, False, ""), (50, 64, 72, True, "")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("np_,D,src_ld,mis,form", ASM_CASES)
@pytest.mark.parametrize("affine", [False, True])
def test_tokens_assemble(dtype, np_, D, src_ld, mis, form, affine):
    hh = _h()
    B = 2
    src = _rand(B * np_, src_ld, seed=91)
    cls, pos = _rand(D, seed=92), _rand(np_ + 1, D, seed=93)
    s, b = _affine(D, 94)
    sd = src.to(dtype).to(DEV)
    if mis:
        sd = _misaligned(sd)
    with traced() as last:
        x = hh.tokens_assemble(sd, cls.to(DEV), pos.to(DEV), B, np_, D, scale=s.to(DEV) if affine else None, shift=b.to(DEV) if affine else None,
                               src_ld=src_ld).cpu()
        name = "tokens_assemble_rows_kernel" if form == "rows" else "tokens_assemble_kernel"
        assert last() == name + ("<bf16>" if dtype == torch.bfloat16 else "<float>")
    v = src.to(dtype).float()[:, :D].reshape(B, np_, D)
    assert torch.equal(x[:, 0], (cls + pos[0]).expand(B, D))
    if affine:
        ref = torch.relu(v.double() * s.double() + b.double()) + pos[1:].double()
        assert rel_err(x[:, 1:], ref) <= 1e-6
    else:
        assert torch.equal(x[:, 1:], v + pos[1:])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("np_,D,src_ld", [(784, 384, 384), (50, 30, 36)])
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("level", [0, 1, 2])
def test_tokens_assemble_bwd(det, dtype, np_, D, src_ld, affine, level):
    det(level)
    hh = _h()
    B = 2
    dx, src = _rand(B, np_ + 1, D, seed=101), _rand(B * np_, src_ld, seed=102)
    s, b = _affine(D, 103)
    mean = _rand(D, seed=105, scale=0.1)
    sd = src.to(dtype).to(DEV)
    runs = [hh.tokens_assemble_bwd(dx.to(DEV), sd, s.to(DEV) if affine else None, b.to(DEV) if affine else None, B, np_, D, src_ld,
                                   mean=mean.to(DEV) if affine else None) for _ in range(2)]
    dsrc, dsc, dsh = runs[0]
    g = dx[:, 1:].reshape(B * np_, D).double()
    if affine:
        rd, rs, rh = _bn_relu_bwd_ref(g, _q(src, dtype)[:, :D], s.double(), b.double(), mean.double())
        check(dsrc, rd, dtype, 1e-6)
        assert rel_err(dsc.cpu(), rs) <= 1e-5 and rel_err(dsh.cpu(), rh) <= 1e-5
        if level > 0:        # the partial sums take the scratch slab whenever one is registered, bf16 included
            assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2]), "deterministic launch gave different bits"
    else:
        assert torch.equal(dsrc.cpu(), g.float().to(dtype))
        assert dsc is None and dsh is None


# (Din, Dout, form)
POOL_CASES = [(384, 256, "rows"), (100, 37, "rows"), (256, 256, "rows"), (1100, 1030, "")]


@pytest.mark.parametrize("din_t", DTYPES)
@pytest.mark.parametrize("dout_t", DTYPES)
@pytest.mark.parametrize("Din,Dout,form", POOL_CASES)
def test_pool_pos(din_t, dout_t, Din, Dout, form):
    hh = _h()
    B, L = 2, 50
    y = _rand(B, L, Din, seed=111)
    pos = _rand(L - 1, Dout, seed=112)
    yd = y.to(din_t).to(DEV)
    tn = {torch.float32: "float", torch.bfloat16: "bf16"}
    with traced() as last:
        out, nop = hh.pool_pos(yd, pos.to(DEV), Dout, dout_t, want_nopos=True)
        assert last() == f"pool_pos{'_rows' if form else ''}_kernel<{tn[din_t]}, {tn[dout_t]}>"
    pooled = F.adaptive_avg_pool1d(_q(y, din_t)[:, 1:], Dout)
    check(nop, pooled, dout_t, 1e-5)
    check(out, pooled + pos.double(), dout_t, 1e-5)
    out2 = hh.pool_pos(yd, None, Dout, dout_t)                        # pos = None: the plain pool
    check(out2, pooled, dout_t, 1e-5)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L,max_len", [(14, 20), (20, 20)])
def test_embed_tokens(dtype, L, max_len):
    hh = _h()
    B, D, V, pad = 3, 64, 227, 226
    g = torch.Generator().manual_seed(121)
    tok = torch.randint(0, V - 1, (B, L), generator=g)
    tok[0, 0] = pad                       # PAD at the start, middle and end
    tok[1, L // 2] = pad
    tok[2, L - 3:] = pad
    emb, pos = _rand(V, D, seed=122), _rand(max_len, D, seed=123)
    x, kb = hh.embed_tokens(tok.to(DEV), emb.to(DEV), pos.to(DEV), pad, dtype)
    assert torch.equal(x.cpu(), (emb[tok] + pos[:L]).to(dtype))
    assert torch.equal(kb.cpu(), (tok == pad).float())


@pytest.mark.parametrize("dtype", DTYPES)
def test_add_pos(dtype):
    hh = _h()
    B, L, D = 3, 17, 40
    x, pos = _rand(B, L, D, seed=131), _rand(L, D, seed=132)
    out = hh.add_pos(x.to(dtype).to(DEV), pos.to(DEV)).cpu()
    assert torch.equal(out, (x.to(dtype).float() + pos).to(dtype))


# ------------------------------------------------------------------------------------------------ ScoreNet glue
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [13, 16, 192])
def test_pair_mean_and_bwd(dtype, N):
    hh = _h()
    B, D = 2, 64
    L = 2 * N + 3
    feats = _rand(B, L, D, seed=141)
    out = hh.pair_mean(feats.to(dtype).to(DEV), N).cpu()
    f = feats.to(dtype).float()
    assert torch.equal(out, ((f[:, 1:2 * N + 1:2] + f[:, 2:2 * N + 2:2]) / 2).to(dtype))
    dF = _rand(B, N, D, seed=142)
    ref = torch.zeros(B, L, D)
    ref[:, 1:2 * N + 1] = 0.5 * dF.repeat_interleave(2, dim=1)
    d = hh.pair_mean_bwd(dF.to(DEV), B, L, N, D, dtype).cpu()
    assert torch.equal(d, ref.to(dtype))
    base = _rand(B, L, D, seed=143).to(dtype)
    acc = base.to(DEV)
    hh.pair_mean_bwd(dF.to(DEV), B, L, N, D, dtype, accumulate_into=acc)
    assert torch.equal(acc.cpu(), (base.float() + ref).to(dtype))


def _pair_sums_ref(U, V, B, N):
    h = U.reshape(B, N, 1, -1) + V.reshape(B, 1, N, -1)                # every (i, j) pair explicitly
    return h.sum((0, 1, 2)), (h * h).sum((0, 1, 2))


# Closed-form pair statistics (pair_stats_kernel): the fp32 sums are accurate to a few ulps of sum h^2, so the variance bn_finalize derives
# from them carries a relative error proportional to E[h^2] / Var[h].  The bound written next to the kernel: 2^-17 * E[h^2] / Var[h]
# (an fp32 emulation of the kernel's summation order measured at most 2^-19.4 at N = 13 / 16 / 192, mean / spread up to 100).
PAIR_VAR_BOUND = 2.0 ** -17


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [13, 16, 192])
@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("offset", [0.0, 30.0])
def test_pair_stats(det, dtype, N, level, offset):
    det(level)
    hh = _h()
    B, C = 2, 48
    U, V = _rand(B * N, C, seed=151, shift=offset), _rand(B * N, C, seed=152, shift=-0.5 * offset)
    Uq, Vq = _q(U, dtype), _q(V, dtype)
    r1, r2 = _pair_sums_ref(Uq, Vq, B, N)
    runs = []
    for _ in range(2):
        sums = torch.zeros(2 * C, device=DEV)
        hh.pair_stats(U.to(dtype).to(DEV), V.to(dtype).to(DEV), B, N, sums)
        runs.append(sums)
    got = runs[0].cpu()
    assert rel_err(got[:C], r1) <= 1e-5 and rel_err(got[C:], r2) <= 1e-5
    if hh.det_on(U.to(dtype)):
        assert torch.equal(runs[0], runs[1]), "deterministic launch gave different bits"
    # the variance bn_finalize derives from these sums
    cnt = B * N * N
    var = r2 / cnt - (r1 / cnt) ** 2
    var_k = got[C:].double() / cnt - (got[:C].double() / cnt) ** 2
    ratio = (r2 / cnt) / var
    assert bool(((var_k - var).abs() / var <= PAIR_VAR_BOUND * ratio + 1e-6).all()), float(((var_k - var).abs() / var / ratio).max())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [13, 192])
def test_pair_stats_bwd(dtype, N):
    hh = _h()
    B, C = 2, 48
    U, V = _rand(B * N, C, seed=161), _rand(B * N, C, seed=162)
    a, bc = _rand(C, seed=163, scale=0.01), _rand(C, seed=164, scale=0.01)
    dU0, dV0 = _rand(B * N, C, seed=165), _rand(B * N, C, seed=166)
    dU, dV = dU0.to(DEV), dV0.to(DEV)
    hh.pair_stats_bwd(U.to(dtype).to(DEV), V.to(dtype).to(DEV), a.to(DEV), bc.to(DEV), dU, dV, B, N)
    Uq, Vq = _q(U, dtype).reshape(B, N, C), _q(V, dtype).reshape(B, N, C)
    # gradient of sum_c a_c * S1_c + b_c * S2_c / 2 ... written out per pair: dh = a + b * h, dU[i] = sum_j dh[i, j], dV[j] = sum_i dh[i, j]
    h = Uq.unsqueeze(2) + Vq.unsqueeze(1)
    dh = a.double() + bc.double() * h
    rU = dU0.double() + dh.sum(2).reshape(B * N, C)
    rV = dV0.double() + dh.sum(1).reshape(B * N, C)
    assert rel_err(dU.cpu(), rU) <= 1e-5 and rel_err(dV.cpu(), rV) <= 1e-5


# (dtype, misaligned, kernel)
SCORE_CASES = [(torch.bfloat16, False, "score_out64_kernel"), (torch.bfloat16, True, "score_out_kernel<bf16>"), (torch.float32, False, "score_out_kernel<float>")]


@pytest.mark.parametrize("dtype,mis,kernel", SCORE_CASES)
@pytest.mark.parametrize("transpose", [0, 1])
@pytest.mark.parametrize("B,N", [(2, 13), (2, 192)])
def test_score_out(dtype, mis, kernel, transpose, B, N):
    hh = _h()
    C = 64
    H3 = _rand(B * N * N, C, seed=171)
    s, b = _affine(C, 172)
    w4, b4 = _rand(C, seed=174, scale=0.2), _rand(1, seed=175)
    Hd = H3.to(dtype).to(DEV)
    if mis:
        Hd = _misaligned(Hd, off=4)      # 8-byte aligned, not 16: the generic form's 8-byte loads stay aligned
    base = _rand(B, N, N, seed=176)
    out = base.clone().to(DEV) if transpose else torch.full((B, N, N), SENT, device=DEV)
    with traced() as last:
        hh.score_out(Hd, s.to(DEV), b.to(DEV), w4.to(DEV), b4.to(DEV), out, B, N, transpose)
        assert last() == kernel
    sc = (torch.relu(_q(H3, dtype) * s.double() + b.double()) @ w4.double() + b4.double()).reshape(B, N, N)
    ref = base.double() + sc.transpose(1, 2) if transpose else sc
    assert rel_err(out.cpu(), ref) <= 1e-5


# ------------------------------------------------------------------------------------------------ BatchNorm finalize / backward coefficients
def _bn_ref_from_sums(S1, S2, count, gamma, beta, eps):
    m = S1.double() / count
    v = (S2.double() / count - m * m).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(v + eps)
    scale = gamma.double() * rstd
    return m, v, rstd, scale, beta.double() - m * scale


@pytest.mark.parametrize("count", [2, 4096])
@pytest.mark.parametrize("ratio", [1.0, 1e3])
def test_bn_finalize_training(count, ratio):
    hh = _h()
    C, eps, mom = 40, 1e-5, 0.1
    x = _rand(count, C, seed=181).double()
    if ratio != 1.0:
        x = x * 0.01 + ratio * 0.01        # mean / std = ratio
    S1, S2 = x.sum(0).float(), (x * x).sum(0).float()        # the kernel's input: fp32 sums
    gamma, beta = _rand(C, seed=182) + 1.0, _rand(C, seed=183)
    rm0, rv0 = _rand(C, seed=184), _rand(C, seed=185).abs() + 0.5
    rm, rv = rm0.to(DEV), rv0.to(DEV)
    sums = torch.cat([S1, S2]).to(DEV)
    scale, shift, sm, sr = hh.bn_finalize(sums, float(count), gamma.to(DEV), beta.to(DEV), rm, rv, eps, mom, True, save=True)
    m, v, rstd, rs, rh = _bn_ref_from_sums(S1, S2, count, gamma, beta, eps)
    for got, ref in ((scale, rs), (shift, rh), (sm, m), (sr, rstd)):
        assert rel_err(got.cpu(), ref) <= 1e-5
    assert rel_err(rm.cpu(), (1 - mom) * rm0.double() + mom * m) <= 1e-5
    assert rel_err(rv.cpu(), (1 - mom) * rv0.double() + mom * v * count / (count - 1)) <= 1e-5
    if ratio == 1.0:        # and torch's own running-stat update (momentum, Bessel) on the data behind the sums
        trm, trv = rm0.double().clone(), rv0.double().clone()
        F.batch_norm(x, trm, trv, gamma.double(), beta.double(), training=True, momentum=mom, eps=eps)
        assert rel_err(rm.cpu(), trm) <= 1e-5 and rel_err(rv.cpu(), trv) <= 1e-5


def test_bn_finalize_eval():
    hh = _h()
    C, eps = 40, 1e-5
    gamma, beta = _rand(C, seed=191) + 1.0, _rand(C, seed=192)
    rm0, rv0 = _rand(C, seed=193), _rand(C, seed=194).abs() + 0.5
    rm, rv = rm0.to(DEV), rv0.to(DEV)
    scale, shift = hh.bn_finalize(None, 1.0, gamma.to(DEV), beta.to(DEV), rm, rv, eps, 0.1, False)
    rstd = 1.0 / torch.sqrt(rv0.double() + eps)
    assert rel_err(scale.cpu(), gamma.double() * rstd) <= 1e-6
    assert rel_err(shift.cpu(), beta.double() - rm0.double() * gamma.double() * rstd) <= 1e-6
    assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0)


@pytest.mark.parametrize("count", [2, 4096])
@pytest.mark.parametrize("training", [True, False])
def test_bn_bwd_coeffs(count, training):
    hh = _h()
    C, eps = 40, 1e-5
    x = _rand(count, C, seed=201).double() * 2.0 + 0.5
    gamma, beta = (_rand(C, seed=202) + 1.0).double(), _rand(C, seed=203).double()
    G = _rand(count, C, seed=204).double()
    xr = x.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm, rv = x.mean(0), x.var(0, unbiased=False)
    y = F.batch_norm(xr, None if training else rm, None if training else rv, gr, br, training=training, eps=eps)
    y.backward(G)
    m, v = x.mean(0), x.var(0, unbiased=False)
    rstd = 1.0 / torch.sqrt(v + eps)
    dscale = (G * (x - m)).sum(0)       # the centred form the callers accumulate
    dshift = G.sum(0)
    f = lambda t: t.float().to(DEV)     # noqa: E731
    dg, db, a, b = hh.bn_bwd_coeffs(f(dscale), f(dshift), f(gamma), f(m), f(rstd), float(count), training)
    assert rel_err(dg.cpu(), gr.grad) <= 1e-5 and rel_err(db.cpu(), br.grad) <= 1e-5
    direct = G * (gamma * rstd)
    dx = direct + a.cpu().double() + b.cpu().double() * x
    # the three terms are each of the size of `direct` and cancel (at count 2 the exact gradient is ~eps / var of them): error relative to that
    assert float((dx - xr.grad).abs().max() / direct.abs().max()) <= 1e-5
    if not training:
        assert bool((a == 0).all() and (b == 0).all())
    acc = torch.stack([_rand(C, seed=205), _rand(C, seed=206)]).to(DEV)     # += into the gradient arena
    acc0 = acc.clone().cpu().double()
    hh.bn_bwd_coeffs(f(dscale), f(dshift), f(gamma), f(m), f(rstd), float(count), training, acc=acc)
    assert rel_err(acc[0].cpu(), acc0[0] + gr.grad) <= 1e-5 and rel_err(acc[1].cpu(), acc0[1] + br.grad) <= 1e-5


# ------------------------------------------------------------------------------------------------ argmax, cast
def test_argmax_edges():
    hh = _h()
    nan, inf = float("nan"), float("inf")
    for cols, ld in [(10, 10), (64, 70), (100, 128), (227, 227), (300, 301)]:
        rows = 12
        buf = _rand(rows, ld, seed=cols)
        x = buf[:, :cols].clone()
        x[1, :] = 0.0
        x[1, 5] = x[1, min(70, cols - 1)] = 9.0        # tie across lanes (5 / 70) - or inside one lane when cols is small
        x[2, :] = 0.0
        x[2, 3] = 9.0
        if cols > 67:
            x[2, 67] = 9.0                              # tie inside one lane (3 and 67 share lane 3)
        x[3, :] = -inf                                  # all -inf: index 0
        x[4, cols // 2] = nan                           # one NaN: its index
        x[5, :] = nan                                   # all NaN: index 0
        x[6, cols - 1] = nan
        x[6, cols // 3] = nan                           # two NaN: the first
        x[7, :] = 1.0                                   # all equal
        buf[:, :cols] = x
        xd = buf.to(DEV)[:, :cols]                      # ld > cols: a strided view
        got = hh.argmax(xd).cpu()
        want = torch.argmax(x, dim=1)
        assert bool(((got >= 0) & (got < cols)).all()), got
        assert torch.equal(got, want), (cols, got, want)
        assert int(got[3]) == 0 and int(got[4]) == cols // 2 and int(got[5]) == 0 and int(got[6]) == cols // 3 and int(got[7]) == 0
        assert int(got[1]) == 5 and int(got[2]) == 3


def test_argmax_decode_shape():
    hh = _h()
    x = _rand(64 * 7, 227, seed=211)                  # greedy decode: batch x 227-way logits
    assert torch.equal(hh.argmax(x.to(DEV)).cpu(), torch.argmax(x, dim=1))


def test_cast_edges():
    hh = _h()
    one = 1.0
    vals = [one + 2.0 ** -8, one + 3 * 2.0 ** -8, -(one + 2.0 ** -8), 2.0 ** 20 * (one + 2.0 ** -8), one + 2.0 ** -8 + 2.0 ** -20,
            float("inf"), float("-inf"), 1e-40, -1e-40, 1.4e-45, 3.0e-39, 3.4028235e38, -3.4028235e38, 0.0, -0.0]
    x = torch.tensor(vals, dtype=torch.float32)
    x = torch.cat([x, _rand(1000, seed=221) * 100])
    got = hh.cast(x.to(DEV), torch.bfloat16).cpu()
    assert torch.equal(got.view(torch.int16), x.to(torch.bfloat16).view(torch.int16))
    nans = torch.tensor([0x7FC00000, 0x7F800001, 0xFFC00001 - (1 << 32), 0x7FBFFFFF], dtype=torch.int32).view(torch.float32)
    assert bool(torch.isnan(hh.cast(nans.to(DEV), torch.bfloat16).cpu().float()).all()), "NaN must stay NaN"
    assert torch.equal(hh.cast(got.to(DEV), torch.float32).cpu(), got.float())       # bf16 -> fp32 exact
    assert torch.equal(hh.cast(x.to(DEV), torch.float32).cpu(), x)
    for n in (0, 1):
        y = _rand(n, seed=222)
        assert torch.equal(hh.cast(y.to(DEV), torch.bfloat16).cpu(), y.to(torch.bfloat16))


# ------------------------------------------------------------------------------------------------ losses
IGN = 226


def _ce_bwd_call(logits, tgt, lse, acc, gscale, out, V, vpad):
    hh = _h()
    hh.check(_lib().p3_ce_loss_bwd(hh.ptr(logits), c_int(logits.stride(0)), hh.ptr(tgt), c_int(logits.shape[0]), c_int(V), c_int(IGN), hh.ptr(lse),
                                   hh.ptr(acc), hh.ptr(gscale), hh.ptr(out), c_int(hh.dt(out)), c_int(out.stride(0)), c_int(vpad), hh.stream()),
             "p3_ce_loss_bwd")


@pytest.mark.parametrize("V", [227, 300])
@pytest.mark.parametrize("offset", [0.0, 1e4, -1e4])
@pytest.mark.parametrize("out_t", DTYPES)
@pytest.mark.parametrize("level", [0, 1])
def test_ce_loss(det, V, offset, out_t, level):
    det(level)
    hh = _h()
    R, vpad = 70, V + 13
    g = torch.Generator().manual_seed(231)
    logits = (_rand(R, V, seed=232, scale=3.0) + offset).float()
    tgt = torch.randint(0, V, (R,), generator=g)
    tgt[::5] = IGN
    ld = logits.to(DEV)
    runs = [hh.ce_loss_fwd(ld, tgt.to(DEV), IGN) for _ in range(2)]
    lse, acc = runs[0]
    L = logits.double()
    valid = tgt != IGN
    ref_sum = F.cross_entropy(L, tgt, ignore_index=IGN, reduction="sum")
    ref_lse = torch.logsumexp(L, 1)
    # lse is an fp32 value near |offset|: each row carries up to an ulp of it into the loss (the logits themselves are fp32 at that scale)
    ulp = 2.0 ** (math.frexp(max(abs(offset), 1.0))[1] - 24)
    assert float((lse.cpu().double() - ref_lse).abs().max()) <= 1e-6 * float(ref_lse.abs().max()) + 2 * ulp
    assert abs(float(acc[0]) - float(ref_sum)) <= 1e-5 * abs(float(ref_sum)) + 2 * ulp * int(valid.sum())
    assert float(acc[1]) == float(valid.sum())
    if level > 0:
        assert torch.equal(runs[0][1], runs[1][1]), "deterministic launch gave different bits"
    gscale = torch.tensor([0.7], device=DEV)
    out = torch.full((R, vpad), SENT, dtype=out_t, device=DEV)
    _ce_bwd_call(ld, tgt.to(DEV), lse, acc, gscale, out, V, vpad)
    assert bool((out[:, V:] == 0).all()), "padding columns must be zero"
    # exp(x - lse) with the kernel's fp32 lse (at |offset| = 1e4 an ulp of lse is 1e-3 of the softmax: bounded by the lse check above)
    onehot = F.one_hot(tgt.clamp_max(V - 1), V).double()
    ref = 0.7 / int(valid.sum()) * (torch.exp(L - lse.cpu().double()[:, None]) - onehot) * valid.double()[:, None]
    check(out[:, :V].contiguous(), ref, out_t, 1e-5)
    if offset == 0.0:
        Lr = L.clone().requires_grad_(True)
        (0.7 * F.cross_entropy(Lr, tgt, ignore_index=IGN, reduction="mean")).backward()
        check(out[:, :V].contiguous(), Lr.grad, out_t, 1e-5)


def test_ce_loss_all_ignored():
    """every target ignored: the kernel gives loss sum 0 over 0 rows and an all-zero gradient (torch's mean would be NaN; the callers divide by
    max(count, 1))"""
    hh = _h()
    R, V = 9, 227
    logits = _rand(R, V, seed=241).to(DEV)
    tgt = torch.full((R,), IGN, dtype=torch.int64, device=DEV)
    lse, acc = hh.ce_loss_fwd(logits, tgt, IGN)
    assert float(acc[0]) == 0.0 and float(acc[1]) == 0.0
    out = torch.full((R, V + 3), SENT, device=DEV)
    _ce_bwd_call(logits, tgt, lse, acc, torch.tensor([1.0], device=DEV), out, V, V + 3)
    assert bool((out == 0).all())
    assert not bool(torch.isnan(lse).any())


@pytest.mark.parametrize("n", [1, 3, 4 * 512 * 256 + 77, 1000])
@pytest.mark.parametrize("level", [0, 1])
def test_bce_loss(det, n, level):
    det(level)
    hh = _h()
    g = torch.Generator().manual_seed(251)
    p = torch.rand(n, generator=g) * 0.98 + 0.01
    y = (torch.rand(n, generator=g) > 0.5).float()
    if n >= 4:       # exactly 0 and 1 against both labels: the -100 log clamp and the 1e-12 denominator
        p[:4] = torch.tensor([0.0, 0.0, 1.0, 1.0])
        y[:4] = torch.tensor([0.0, 1.0, 0.0, 1.0])
    pd, yd = p.to(DEV), y.to(DEV)
    runs = [hh.bce_loss_fwd(pd, yd) for _ in range(2)]
    ref = F.binary_cross_entropy(p.double(), y.double(), reduction="sum")
    assert abs(float(runs[0][0]) - float(ref)) <= 1e-5 * abs(float(ref))
    if level > 0:
        assert torch.equal(runs[0], runs[1]), "deterministic launch gave different bits"
    dp = hh.bce_loss_bwd(pd, yd, torch.tensor([0.9], device=DEV)).cpu().double()
    pr = p.double().requires_grad_(True)
    (0.9 * F.binary_cross_entropy(pr, y.double(), reduction="mean")).backward()
    r = pr.grad
    assert bool(((dp - r).abs() <= 1e-5 * r.abs() + 1e-30).all()), float(((dp - r).abs() / r.abs().clamp_min(1e-30)).max())
