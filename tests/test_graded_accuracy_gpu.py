"""Graded-input accuracy of the dense kernels (GEMM family, weight gradients, planes kernels, fusion conv, attention, LayerNorm).

Every other accuracy check of the suite is rel_err = max|a-b| / max|b| over the whole tensor on randn inputs of one scale: an error confined to small rows, columns
or heads is invisible.  Here rows / columns / heads of the operands are multiplied by the power-of-two factors of tests.helpers.grade (2^0 ... 2^-33) and each
case asserts

  (1) equivariance, no tolerance: the output on graded operands is bit-equal to the output on ungraded operands times the same factors (multiplying by a power
      of two is exact in fp32 and bf16 and commutes with rounding and with the hi / lo split) - only where the launch has a fixed summation order (one split, or
      the deterministic level that covers the dtype);
  (2) a per-slice bound: block_err(got, float64 reference of the graded problem, dim) < tol * spread(float64 reference of the ungraded problem, dim), where tol is
      the tolerance the suite already holds that kernel and dtype to (imported from / quoted after tests/test_bounds_gpu.py) and spread is what a slice's own
      maximum can be smaller by than the tensor's on ungraded data.  No tolerance is fitted.

tests/test_graded_accuracy_cpu.py shows on an emulation that (2) catches a magnitude-dependent defect that rel_err does not."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import block_err, grade, rel_err, spread
from tests.test_bounds_gpu import ATTN_KINDS, ATTN_TOL, KINDS, X3_TILES, _attn_ref64, _gemm_tol, _launch, _rand, _scope, _up8, _x3_tile

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
X3_TOL = 1e-5                                   # the planes kernels (test_gemm_x3_plain_and_epilogues, test_gemm_tn_x3_weight_gradient, test_conv_planes_gpu.py)
SKINNY_TOL = {BF: 8e-3, F32: 2e-3}              # by output dtype (test_skinny_gemm_is_bit_identical_to_the_tiled_kernel)
TN_TOL = {"f32": (1e-5, 1e-4), "x3": (1e-5, 1e-5), "bf16": (1e-4, 1e-4)}       # (product, column sums): test_gemm_tn_strided_operand_and_accumulate, test_gemm_tn_and_colsum
LN_TOL = {"y": 2e-6, "y_planes": 3e-5, "dx": 1e-5, "dparam": 1e-5, "stat": 1e-5}        # test_layernorm_fwd_bwd, test_layernorm_planes_forward_backward


def _h():
    import pixelspointspolygons_amd.hip as h
    return h


@pytest.fixture
def det():
    """set the deterministic level for one test; the previous level comes back afterwards (as in test_glue_kernels_gpu.py)"""
    h = _h()
    prev = h.DETERMINISTIC
    yield h.set_deterministic
    h.set_deterministic(prev)


def _f(t):
    return t.detach().float().cpu()


def _bound(tag, got, ref, ref0, dim, tol):
    """block_err(got, ref, dim) < tol * spread(ref0, dim), the measured value printed first"""
    e, rho = block_err(_f(got), ref, dim), spread(ref0, dim)
    print(f"[graded] {tag}: block_err {e:.3e}, bound {tol * rho:.3e} (tol {tol:.0e} x spread {rho:.3g}){'   <-- within 3x' if not e < tol * rho / 3 else ''}")
    assert e < tol * rho, (tag, e, tol, rho)


def _equal(tag, got, got0, factor=None, skip=None):
    """got == got0 * factor bit for bit (compared as fp32: exact for bf16 and fp32 values and power-of-two factors)"""
    if skip:
        print(f"[graded] {tag}: equivariance skipped ({skip})")
        return
    want = _f(got0) if factor is None else _f(got0) * factor
    same = torch.equal(_f(got), want)
    print(f"[graded] {tag}: equivariance asserted{'' if same else ' - FAILED'}")
    if not same:
        bad = (_f(got) != want)
        raise AssertionError((tag, "not bit-equivariant", int(bad.sum()), "elements; first at", bad.nonzero()[0].tolist()))


def _both(tag, got, got0, factor, ref, ref0, dim, tol, skip=None):
    _equal(tag, got, got0, factor, skip)
    _bound(tag, got, ref, ref0, dim, tol)


def _strided(t, ld):
    """t [R, C] on the device as a view with row stride ld >= C (zero padding)"""
    buf = torch.zeros(t.shape[0], ld, dtype=t.dtype, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf[:, :t.shape[1]]


# ====================================================================================================================== p3_gemm
def _gemm(kind, a, w, want=None, **kw):
    """out = epilogue(a w^T) on the kernel of `kind`; operands already rounded to the kind's dtype -> the output, fp32 on the host"""
    h = _h()
    idt, odt, split = KINDS[kind]
    M, N = a.shape[0], w.shape[0]
    out = torch.empty(M, _up8(N), dtype=odt, device=DEV)[:, :N]
    if kw.get("residual") is not None:
        kw["residual"] = _strided(kw["residual"], _up8(N))
    if kw.get("bias") is not None:
        kw["bias"] = kw["bias"].to(DEV)
    with _scope(split):
        _, name = _launch(lambda: h.gemm(a.to(DEV), w.to(DEV), out=out, **kw))
    torch.cuda.synchronize()
    assert want is None or name == want, (name, want)
    return _f(out)


def _gemm_data(kind, M, N, K):
    idt = KINDS[kind][0]
    return _rand(M, K, seed=1).to(idt), _rand(N, K, seed=2, scale=0.1).to(idt), _rand(N, seed=3)


GEMM_SHAPES = [(255, 227, 32), (129, 136, 64)]


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
@pytest.mark.parametrize("kind", list(KINDS))
def test_gemm_row_graded_a(kind, M, N, K):
    """rows of A scaled: the output rows carry the factor (no bias: it is per column); epilogues none and ReLU.  One workgroup adds a whole K: fixed order."""
    h = _h()
    a, w, _ = _gemm_data(kind, M, N, K)
    r = grade(M)[:, None]
    ag = (a.float() * r).to(a.dtype)
    ref0, ref = a.double() @ w.double().t(), ag.double() @ w.double().t()
    for epi, kw, fn in (("none", {}, lambda t: t), ("relu", {"act": h.ACT_RELU}, F.relu)):
        _both(f"gemm {kind} {M}x{N}x{K} rows {epi}", _gemm(kind, ag, w, **kw), _gemm(kind, a, w, **kw), r, fn(ref), fn(ref0), 0, _gemm_tol(kind, epi))


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
@pytest.mark.parametrize("kind", list(KINDS))
def test_gemm_column_graded_w(kind, M, N, K):
    """rows of W (output columns) scaled, bias and residual with them: bias, bias + ReLU, fp32 and bf16 residual - equivariant; GELU is not (bound only, against
    float64 GELU of the graded pre-activation, per column)."""
    h = _h()
    a, w, bias = _gemm_data(kind, M, N, K)
    c = grade(N)
    wg, bg = (w.float() * c[:, None]).to(w.dtype), bias * c
    pre0, pre = a.double() @ w.double().t() + bias.double(), a.double() @ wg.double().t() + bg.double()
    tag = f"gemm {kind} {M}x{N}x{K} cols "
    _both(tag + "bias", _gemm(kind, a, wg, bias=bg), _gemm(kind, a, w, bias=bias), c, pre, pre0, 1, _gemm_tol(kind, "bias"))
    _both(tag + "relu", _gemm(kind, a, wg, bias=bg, act=h.ACT_RELU), _gemm(kind, a, w, bias=bias, act=h.ACT_RELU), c, F.relu(pre), F.relu(pre0), 1,
          _gemm_tol(kind, "relu"))
    for epi, rdt in (("res_f32", F32), ("res_bf16", BF)):
        res = _rand(M, N, seed=4).to(rdt)
        rg = (res.float() * c).to(rdt)
        _both(tag + epi, _gemm(kind, a, wg, bias=bg, residual=rg), _gemm(kind, a, w, bias=bias, residual=res), c, pre + rg.double(), pre0 + res.double(), 1,
              _gemm_tol(kind, epi))
    _equal(tag + "gelu", None, None, skip="GELU does not commute with scaling")
    _bound(tag + "gelu", _gemm(kind, a, wg, bias=bg, act=h.ACT_GELU), F.gelu(pre), F.gelu(pre0), 1, _gemm_tol(kind, "gelu"))


@pytest.mark.parametrize("M,N,K,waves", [(3, 227, 256, 1), (33, 40, 1536, 8)])
@pytest.mark.parametrize("kind", ["bf16", "bf16_f32"])
def test_gemm_skinny_kernel_graded(kind, M, N, K, waves):
    """the M <= 128 one-wave kernel and its K >= 1024 form (eight waves split K and add their parts through LDS in wave order: fixed); rows of A, then rows of W
    with bias and residual"""
    a, w, bias = _gemm_data(kind, M, N, K)
    want, tol = f"gemm_skinny_kernel<{waves}>", SKINNY_TOL[KINDS[kind][1]]
    r, c = grade(M)[:, None], grade(N)
    ag, wg, bg = (a.float() * r).to(BF), (w.float() * c[:, None]).to(BF), bias * c
    res = _rand(M, N, seed=4)
    tag = f"skinny {kind} {M}x{N}x{K} "
    _both(tag + "rows", _gemm(kind, ag, w, want), _gemm(kind, a, w, want), r, ag.double() @ w.double().t(), a.double() @ w.double().t(), 0, tol)
    pre0, pre = a.double() @ w.double().t() + bias.double() + res.double(), a.double() @ wg.double().t() + bg.double() + (res * c).double()
    _both(tag + "cols bias+residual", _gemm(kind, a, wg, want, bias=bg, residual=res * c), _gemm(kind, a, w, want, bias=bias, residual=res), c, pre, pre0, 1, tol)


# ====================================================================================================================== p3_gemm_x3
def _pval(p):
    return (p.hi[:p.rows].float() + p.lo[:p.rows].float()).cpu().double()


def _x3_run(ap, wp, planes, **kw):
    """-> (value fp32 on the host, raw hi plane, raw lo plane) of one p3_gemm_x3 launch"""
    h = _h()
    kw = {k: (v.to(DEV) if v is not None else None) for k, v in kw.items()}
    out = h.gemm_x3(ap, wp, out_planes=planes, **kw)
    torch.cuda.synchronize()
    if planes:
        return _f(h.from_planes(out)), _f(out.hi[:out.rows]), _f(out.lo[:out.rows])
    return _f(out), None, None


def _x3_case(tile, M, N, K, how):
    h = _h()
    a, w = _rand(M, K, seed=1), _rand(N, K, seed=2, scale=0.1)
    bias, res, mul = _rand(N, seed=3), _rand(M, N, seed=4), _rand(M, N, seed=5)
    rows = how == "rows"
    s = grade(M)[:, None] if rows else grade(N)[None, :]                       # the output's factors
    ag, wg = (a * s, w) if rows else (a, w * grade(N)[:, None])
    ap0, wp0, apg, wpg = h.to_planes(a.to(DEV)), h.to_planes(w.to(DEV), pad=1), h.to_planes(ag.to(DEV)), h.to_planes(wg.to(DEV), pad=1)
    ref0, ref = _pval(ap0) @ _pval(wp0).t(), _pval(apg) @ _pval(wpg).t()       # the planes' own values
    b0, bg = (None, None) if rows else (bias, bias * s[0])                     # a bias is per column: not with row factors
    forms = [("plain", {}, {}, s, ref, ref0),
             ("residual" if rows else "bias+residual", dict(bias=b0, residual=res), dict(bias=bg, residual=res * s), s,
              ref + (res * s).double() + (bg.double() if bg is not None else 0.0), ref0 + res.double() + (b0.double() if b0 is not None else 0.0)),
             ("mul", dict(mul=mul), dict(mul=mul * s), s * s, ref * (mul * s).double(), ref0 * mul.double())]          # the multiplier graded with the output
    dim = 0 if rows else 1
    with _x3_tile(tile):
        if tile == 3:                           # the kernel timer names the launch (as test_gemm_x3_a_stationary_kernel)
            h.KTIMER.enable()
            try:
                h.gemm_x3(ap0, wp0)
                names = dict(h.KTIMER.summary())
            finally:
                h.KTIMER.disable()
            assert any(k.startswith("gemm_x3_as_kernel") for k in names), names
        for name, kw0, kwg, fac, r, r0 in forms:
            for planes in (False, True):
                if tile == 3 and planes and kw0.get("residual") is not None:
                    continue                    # gemm_x3_as.hip builds no residual -> planes epilogue (as_epi_built): the library refuses it, no model path asks for it
                tag = f"gemm_x3 tile {tile} {M}x{N}x{K} {how} {name} -> {'planes' if planes else 'fp32'}"
                g, ghi, glo = _x3_run(apg, wpg, planes, **kwg)
                g0, hi0, lo0 = _x3_run(ap0, wp0, planes, **kw0)
                if planes:
                    _equal(tag + " hi", ghi, hi0, fac)
                    _equal(tag + " lo", glo, lo0, fac)
                _both(tag, g, g0, fac, r, r0, dim, X3_TOL)


@pytest.mark.parametrize("how", ["rows", "cols"])
@pytest.mark.parametrize("tile,M,N,K", X3_TILES + [(3, 100, 1536, 384)])
def test_gemm_x3_graded_planes(tile, M, N, K, how):
    """p3_gemm_x3 on its three tile kernels (and the A-stationary one at the decoder FFN's width): rows of the A planes / rows of the W planes graded; fp32 and
    planes outputs (both planes through from_planes, equivariance on the raw hi and lo planes too); plain, (bias +) residual, multiplier.  Every output element
    is one workgroup's sum over K: fixed order."""
    _x3_case(tile, M, N, K, how)


# ====================================================================================================================== weight gradients
def _tn_check(tag, run, dy, x, dyg, xg, preset, fr, fc, dim, tol, cstol, dyv=None):
    """out (+)= dy^T x with dy columns graded by fr (output rows, bias sums) or x columns graded by fc (output columns); preset graded like the output"""
    N, K = dy.shape[1], x.shape[1]
    fac = fr[:, None] * fc[None, :]
    p0 = preset if preset is not None else torch.zeros(N, K)
    pg = p0 * fac
    out0, cs0 = run(dy, x, p0)
    outg, csg = run(dyg, xg, pg)
    v = (lambda t: t.double()) if dyv is None else dyv
    ref0, ref = p0.double() + v(dy).t() @ v(x), pg.double() + v(dyg).t() @ v(xg)
    _both(tag, outg, out0, fac, ref, ref0, dim, tol)
    _both(tag + " colsum", csg, cs0, fr, v(dyg).sum(0), v(dy).sum(0), 0, cstol)


@pytest.mark.parametrize("M,N,K,acc", [(70, 136, 72, False), (257, 136, 136, True)])
@pytest.mark.parametrize("kind", ["bf16", "f32", "x3"])
def test_gemm_tn_graded(det, kind, M, N, K, acc):
    """p3_gemm_tn: columns of dy graded (output rows and the bias column sums carry the factor), then columns of x (output columns).  (257, ...) accumulates into
    existing contents graded like the output.  M = 257 runs several M splits: the deterministic level that covers the dtype fixes their order (1: fp32 and fp32x3,
    2: bf16) - slabs added in split order in float64, which commutes with the scaling."""
    h = _h()
    det(2 if kind == "bf16" else 1)
    idt, _, split = KINDS[kind]
    dy, x = _rand(M, N, seed=21).to(idt), _rand(M, K, seed=22).to(idt)
    fr, fc = grade(N), grade(K)
    preset = _rand(N, K, seed=31) if acc else None

    def run(a, b, p):
        out, cs = p.clone().to(DEV), torch.zeros(N, device=DEV)
        with _scope(split):
            h.gemm_tn(a.to(DEV), b.to(DEV), out=out, colsum_out=cs)
        torch.cuda.synchronize()
        return _f(out), _f(cs)
    tol, cstol = TN_TOL[kind]
    one_n, one_k = torch.ones(N), torch.ones(K)
    tag = f"gemm_tn {kind} {M}x{N}x{K}{' accumulate' if acc else ''} "
    _tn_check(tag + "dy cols", run, dy, x, (dy.float() * fr).to(idt), x, preset, fr, one_k, 0, tol, cstol)
    _tn_check(tag + "x cols", run, dy, x, dy, (x.float() * fc).to(idt), preset, one_n, fc, 1, tol, cstol)


@pytest.mark.parametrize("wide", [0, 1])
def test_gemm_tn_x3_graded_planes(det, wide):
    """p3_gemm_tn_x3 at (130, 768, 768) on both tiles (128 x 128 and, wide = 1, 128 x 384); deterministic level 1 fixes the order of the M splits; wide = 1
    accumulates into graded contents"""
    h = _h()
    det(1)
    M, N, K = 130, 768, 768
    dy, x = _rand(M, N, seed=21), _rand(M, K, seed=22)
    fr, fc = grade(N), grade(K)
    preset = _rand(N, K, seed=31) if wide else None
    L = h.lib()
    was = L.p3_gemm_tn_x3_wide(wide)
    try:
        def run(a, b, p):
            out, cs = p.clone().to(DEV), torch.zeros(N, device=DEV)
            h.KTIMER.enable()
            try:
                h.gemm_tn_x3(h.to_planes(a.to(DEV)), h.to_planes(b.to(DEV)), out=out, colsum_out=cs)
                names = dict(h.KTIMER.summary())
            finally:
                h.KTIMER.disable()
            assert any(k.startswith("gemm_tn_x3_wide_kernel") for k in names) == bool(wide), names
            return _f(out), _f(cs)
        planes_value = lambda t: _f(h.from_planes(h.to_planes(t.to(DEV)))).double()
        tag = f"gemm_tn_x3 wide {wide} {M}x{N}x{K} "
        _tn_check(tag + "dy cols", run, dy, x, dy * fr, x, preset, fr, torch.ones(K), 0, X3_TOL, X3_TOL, dyv=planes_value)
        _tn_check(tag + "x cols", run, dy, x, dy, x * fc, preset, torch.ones(N), fc, 1, X3_TOL, X3_TOL, dyv=planes_value)
    finally:
        L.p3_gemm_tn_x3_wide(was)


# ====================================================================================================================== fusion 3 x 3 conv on planes
def test_conv_planes_output_channel_graded():
    """csrc/conv_planes.hip at the smallest shape of tests/test_conv_planes_gpu.py (B, H, W, Ci, Co = 3, 5, 7, 64, 96): the weight planes, bias and residual
    graded per output channel"""
    h = _h()
    B, H, W, Ci, Co = 3, 5, 7, 64, 96
    M = B * H * W
    x, w = _rand(B, H, W, Ci, seed=1), _rand(Co, Ci, 3, 3, seed=2, scale=0.1)
    bias, res = _rand(Co, seed=3), _rand(M, Co, seed=4)
    c = grade(Co)
    xp = h.pad_nhwc_planes(x.reshape(-1, Ci).to(DEV), B, H, W)
    x_own = h.from_planes(xp).cpu().double().view(B, H + 2, W + 2, Ci)[:, 1:-1, 1:-1].permute(0, 3, 1, 2)
    w2 = w.permute(0, 2, 3, 1).reshape(Co, 9 * Ci).contiguous()                # [Co, (ky, kx, ci)]

    def run(wm, b, r):
        wp = h.to_planes(wm.to(DEV), pad=1)
        w_own = h.from_planes(wp).cpu().double().view(Co, 3, 3, Ci).permute(0, 3, 1, 2)
        ref = F.conv2d(x_own, w_own, padding=1).permute(0, 2, 3, 1).reshape(M, Co) + b.double() + r.double()
        out = h.gemm_x3(xp, wp, bias=b.to(DEV), residual=r.to(DEV), conv=(B, H, W, Ci))
        torch.cuda.synchronize()
        return _f(out), ref
    out0, ref0 = run(w2, bias, res)
    outg, ref = run(w2 * c[:, None], bias * c, res * c)
    _both("conv planes 3x5x7 64 -> 96 output channels", outg, out0, c, ref, ref0, 1, X3_TOL)


# ====================================================================================================================== attention
def _heads(t, H):
    B, L, Dm = t.shape
    return t.reshape(B, L, H, Dm // H)


def _scaled(t, f, H):
    """t [B, L, H * hd] times the per-(batch, head) factors f [B or 1, H] -> same shape and dtype"""
    return (_heads(t.float(), H) * f[:, None, :, None]).reshape(t.shape).to(t.dtype)


def _attn_fwd(kind, q, k, v, H, scale, causal):
    h = _h()
    with _scope(ATTN_KINDS[kind][1]):
        o, lse = h.attention(q.to(DEV), k.to(DEV), v.to(DEV), H, scale, causal=causal, need_lse=True)
    torch.cuda.synchronize()
    return o, lse


def _attn_bwd(kind, q, k, v, o, lse, do, H, scale, causal):
    h = _h()
    with _scope(ATTN_KINDS[kind][1]):
        g = h.attention_bwd(q.to(DEV), k.to(DEV), v.to(DEV), o, lse, do.to(DEV), H, scale, causal=causal)
    torch.cuda.synchronize()
    return g


def _attn_ref(q, k, v, do, H, scale, causal):
    """float64 -> (o, lse, dq, dk, dv) from the operands' own (rounded) values"""
    q, k, v = (t.double().requires_grad_(True) for t in (q, k, v))
    o, lse, _ = _attn_ref64(q, k, v, H, scale, causal, None)
    o.backward(do.double())
    return o.detach(), lse.detach(), q.grad, k.grad, v.grad


@pytest.mark.parametrize("Lq,Lk,causal", [(129, 65, False), (129, 129, True), (37, 200, False)])
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("kind", list(ATTN_KINDS))
def test_attention_graded_heads(kind, hd, Lq, Lk, causal):
    """B = 2, H = 3.  (a) q and k of head h times 2^-(3h + 2) and 2^(3h - 3): the product 2^-5 of every head is undone in `scale` - the same bits of o and lse.
    (b) v graded per (batch, head): o carries the factor, lse does not change.  (c) backward with dO graded per (batch, head): dq, dk, dv carry the factor.
    (d) backward after (b): dv does not change, dq and dk carry the factor.  The forward and both backward kernels (dq; dk | dv) add a whole row / column of the
    score matrix in one workgroup, in tile order: fixed.  Per-(batch, head) bounds at ATTN_TOL."""
    dtype = ATTN_KINDS[kind][0]
    tol_o, tol_lse, tol_g = ATTN_TOL[kind]
    B, H = 2, 3
    Dm = H * hd
    scale = 1.0 / math.sqrt(hd)
    q, k, v, do = (_rand(B, L, Dm, seed=s).to(dtype) for s, L in ((1, Lq), (2, Lk), (3, Lk), (4, Lq)))
    BH, HL = (0, 2), (0, 1)                                                    # slices: (batch, head) of [B, L, H, hd] and of lse [B, H, Lq]
    hv = lambda t: _heads(_f(t), H)
    hr = lambda t: _heads(t, H)
    tag = f"attention {kind} hd {hd} ({Lq}, {Lk}){' causal' if causal else ''} "
    ro, rlse, rdq, rdk, rdv = _attn_ref(q, k, v, do, H, scale, causal)
    o0, lse0 = _attn_fwd(kind, q, k, v, H, scale, causal)
    dq0, dk0, dv0 = _attn_bwd(kind, q, k, v, o0, lse0, do, H, scale, causal)
    # (a)
    e = 3.0 * torch.arange(H) + 2.0
    fq, fk = torch.pow(2.0, -e)[None, :], torch.pow(2.0, e - 5.0)[None, :]
    oa, lsea = _attn_fwd(kind, _scaled(q, fq, H), _scaled(k, fk, H), v, H, scale * 32.0, causal)
    _both(tag + "(a) o", hv(oa), hv(o0), None, hr(ro), hr(ro), BH, tol_o)
    _both(tag + "(a) lse", lsea, lse0, None, rlse, rlse, HL, tol_lse)
    # (b)
    f = grade(B * H).view(B, H)
    f4 = f[:, None, :, None]
    vg = _scaled(v, f, H)
    og, lseg = _attn_fwd(kind, q, k, vg, H, scale, causal)
    go, _, gdq, gdk, gdv = _attn_ref(q, k, vg, do, H, scale, causal)
    _both(tag + "(b) o", hv(og), hv(o0), f4, hr(go), hr(ro), BH, tol_o)
    _equal(tag + "(b) lse", lseg, lse0)
    # (c)
    dog = _scaled(do, f, H)
    _, _, cdq, cdk, cdv = _attn_ref(q, k, v, dog, H, scale, causal)
    for nm, got, got0, ref, ref0 in zip(("dq", "dk", "dv"), _attn_bwd(kind, q, k, v, o0, lse0, dog, H, scale, causal), (dq0, dk0, dv0), (cdq, cdk, cdv),
                                        (rdq, rdk, rdv)):
        _both(tag + "(c) " + nm, hv(got), hv(got0), f4, hr(ref), hr(ref0), BH, tol_g)
    # (d)
    ddq, ddk, ddv = _attn_bwd(kind, q, k, vg, og, lseg, do, H, scale, causal)
    _both(tag + "(d) dq", hv(ddq), hv(dq0), f4, hr(gdq), hr(rdq), BH, tol_g)
    _both(tag + "(d) dk", hv(ddk), hv(dk0), f4, hr(gdk), hr(rdk), BH, tol_g)
    _both(tag + "(d) dv", hv(ddv), hv(dv0), None, hr(gdv), hr(rdv), BH, tol_g)


# ====================================================================================================================== LayerNorm
LN_SHAPES = [(65, 256), (65, 384), (3, 768)]
EPS = 1e-6


def _ln_params(cols):
    return 1 + _rand(cols, seed=2, scale=0.1), _rand(cols, seed=3, scale=0.1)


def _ln_fwd(form, x, gamma, beta, eps):
    """-> (y fp32 on the host [for planes: hi + lo], raw planes or None, mean, rstd on the device)"""
    h = _h()
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    if form == "planes":
        yp, mean, rstd = h.layernorm_planes(xd, gd, bd, eps)
        torch.cuda.synchronize()
        return _f(h.from_planes(yp)), (_f(yp.hi[:yp.rows]), _f(yp.lo[:yp.rows])), mean, rstd
    y, mean, rstd = h.layernorm(xd, gd, bd, eps, save_stats=True)
    torch.cuda.synchronize()
    return _f(y), None, mean, rstd


def _ln_bwd(form, dy, x, gamma, mean, rstd):
    """-> dx, dgamma, dbeta (fp32 on the host; planes form: also the planes' value)"""
    h = _h()
    cols = x.shape[1]
    dg, db = torch.zeros(cols, device=DEV), torch.zeros(cols, device=DEV)
    if form == "planes":
        dx, dxp = h.layernorm_bwd_planes(dy.to(DEV), x.to(DEV), gamma.to(DEV), mean, rstd, torch.zeros_like(x).to(DEV), dg, db)
        torch.cuda.synchronize()
        return _f(dx), _f(dg), _f(db), _f(h.from_planes(dxp))
    dx = h.layernorm_bwd(dy.to(DEV), x.to(DEV), gamma.to(DEV), mean, rstd, dgamma=dg, dbeta=db)
    torch.cuda.synchronize()
    return _f(dx), _f(dg), _f(db), None


def _ln_ref(x, gamma, beta, eps, dy):
    xr, gr, br = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    y = F.layer_norm(xr, (x.shape[1],), gr, br, eps)
    y.backward(dy.double())
    return y.detach(), xr.grad, gr.grad, br.grad


@pytest.mark.parametrize("rows,cols", LN_SHAPES)
@pytest.mark.parametrize("form", ["fp32", "planes"])
def test_layernorm_uniform_scaling(det, form, rows, cols):
    """(a) x * 2^-k with eps * 4^-k, k = 0, 7, 20: the same bits of y; mean * 2^-k and rstd * 2^k exactly; backward (dy unchanged): dx * 2^k exactly, the same bits
    of dgamma and dbeta - where their summation order is fixed: one workgroup (3 rows).  At 65 rows three workgroups add their partials with atomics (norm.hip
    ln_bwd_impl sends the partials through the fixed-order slab from 9 workgroups on, at every deterministic level), so there only the existing 1e-5 against float64
    is asserted."""
    det(1)
    one_wg = rows <= 32                          # ln_bwd_impl: 32 rows per workgroup at these widths
    x = _rand(rows, cols, seed=1, scale=2.0) + 0.3
    gamma, beta = _ln_params(cols)
    dy = _rand(rows, cols, seed=4)
    base = None
    _, _, rdg, rdb = _ln_ref(x, gamma, beta, EPS, dy)
    for k in (0, 7, 20):
        s = 2.0 ** -k
        y, raw, mean, rstd = _ln_fwd(form, x * s, gamma, beta, EPS * s * s)
        grads = _ln_bwd(form, dy, x * s, gamma, mean, rstd)
        for nm, got, ref in (("dgamma", grads[1], rdg), ("dbeta", grads[2], rdb)):          # x * s with eps * s^2 has the parameter gradients of x with eps
            e = rel_err(got, ref)
            print(f"[graded] layernorm {form} {rows}x{cols} x * 2^-{k} {nm}: rel_err {e:.3e}, tol {LN_TOL['dparam']:.0e}")
            assert e < LN_TOL["dparam"], (nm, k, e)
        if base is None:
            base = (y, raw, mean, rstd, grads)
            continue
        y0, raw0, mean0, rstd0, grads0 = base
        tag = f"layernorm {form} {rows}x{cols} x * 2^-{k} "
        _equal(tag + "y", y, y0)
        if raw is not None:
            _equal(tag + "y hi", raw[0], raw0[0])
            _equal(tag + "y lo", raw[1], raw0[1])
        _equal(tag + "mean", mean, mean0, s)
        _equal(tag + "rstd", rstd, rstd0, 1.0 / s)
        _equal(tag + "dx", grads[0], grads0[0], 1.0 / s)
        why = None if one_wg else "three workgroups add their partials with atomics: no fixed order"
        _equal(tag + "dgamma", grads[1], grads0[1], skip=why)
        _equal(tag + "dbeta", grads[2], grads0[2], skip=why)
        if grads[3] is not None:
            _equal(tag + "dx planes", grads[3], grads0[3], 1.0 / s)


@pytest.mark.parametrize("rows,cols", LN_SHAPES)
@pytest.mark.parametrize("form", ["fp32", "planes"])
def test_layernorm_row_graded(form, rows, cols):
    """(b) rows of x graded, eps fixed: against float64 F.layer_norm per row.  beta = 0 (a bias would set every small row's yardstick).  Not equivariant: eps
    is an absolute term beside the rows' variances."""
    x0 = _rand(rows, cols, seed=1, scale=2.0) + 0.3
    gamma, _ = _ln_params(cols)
    beta = torch.zeros(cols)
    x = x0 * grade(rows)[:, None]
    ref0 = F.layer_norm(x0.double(), (cols,), gamma.double(), beta.double(), EPS)
    ref = F.layer_norm(x.double(), (cols,), gamma.double(), beta.double(), EPS)
    y, _, mean, rstd = _ln_fwd(form, x, gamma, beta, EPS)
    tag = f"layernorm {form} {rows}x{cols} row-graded "
    _equal(tag + "y", None, None, skip="eps does not scale with the rows")
    _bound(tag + "y", y, ref, ref0, 0, LN_TOL["y_planes" if form == "planes" else "y"])
    xd = x.double()
    _bound(tag + "mean", mean, xd.mean(-1), x0.double().mean(-1), 0, LN_TOL["stat"])               # every row its own slice
    _bound(tag + "rstd", rstd, (xd.var(-1, unbiased=False) + EPS).rsqrt(), torch.ones(1, dtype=torch.float64), 0, LN_TOL["stat"])


def _ln_chain(form, cols):
    """longest chain of fp32 additions behind a row sum in norm.hip: a lane adds the four values of a float4 chunk as a tree (2), its chunks one after the
    other (chunks - 1), then the lanes of the row - a wave (64 lanes: 6 levels) in ln_fwd_kernel, half a wave (32: 5 levels) in ln_fwd_half_planes_kernel.
    256 / 384 / 768 columns: 8 / 9 / 10 for the fp32 form (a balanced tree's ceil(log2 cols)), 8 / 9 / 12 for the planes form."""
    lanes = 32 if form == "planes" else 64
    chunks = -(-(cols // 4) // lanes)
    return max(2 + (chunks - 1) + int(math.log2(lanes)), math.ceil(math.log2(cols)))


@pytest.mark.parametrize("ratio", [30.0, 1e3])
@pytest.mark.parametrize("rows,cols", LN_SHAPES)
@pytest.mark.parametrize("form", ["fp32", "planes"])
def test_layernorm_offset_rows(form, rows, cols, ratio):
    """(c) x = std * randn + mean with mean / std = 30 and 1e3, forward and backward against float64.  Bound: the existing tolerance + delta,
    delta = (chain + 4) * 2^-24 * |mean| / std: the fp32 rounding of the row sum (an addition chain of _ln_chain() links, each rounding a partial sum of size
    <= cols |mean|; + 4 for the division by cols, the rounded reciprocal, x - mean and the product with rstd) is an error of the mean of delta * std, carried into
    (x - mean) * rstd as delta.  7.7e-4 at 384 columns and ratio 1e3; a one-pass variance (E[x^2] - mean^2) is wrong by about 2^-24 ratio^2 = 6e-2 there.
    dx is linear in xhat with coefficients of the size of dx itself: the same bound.  dgamma[c] = sum_r dy[r, c] xhat[r, c] sees the rows' errors added:
    delta * max_c sum_r |dy[r, c]| relative to max|dgamma|.  dbeta does not depend on x."""
    std = 0.5
    x = _rand(rows, cols, seed=1) * std + ratio * std
    gamma, beta = _ln_params(cols)
    dy = _rand(rows, cols, seed=4)
    ry, rdx, rdg, rdb = _ln_ref(x, gamma, beta, EPS, dy)
    delta = (_ln_chain(form, cols) + 4) * 2.0 ** -24 * ratio
    y, _, mean, rstd = _ln_fwd(form, x, gamma, beta, EPS)
    dx, dg, db, dxp = _ln_bwd(form, dy, x, gamma, mean, rstd)
    xd = x.double()
    checks = [("y", y, ry, LN_TOL["y_planes" if form == "planes" else "y"] + delta),
              ("mean", _f(mean), xd.mean(-1), LN_TOL["stat"]),
              ("rstd", _f(rstd), (xd.var(-1, unbiased=False) + EPS).rsqrt(), LN_TOL["stat"]),
              ("dx", dx, rdx, LN_TOL["dx"] + delta),
              ("dgamma", dg, rdg, LN_TOL["dparam"] + delta * float(dy.double().abs().sum(0).max() / rdg.abs().max())),
              ("dbeta", db, rdb, LN_TOL["dparam"])]
    if dxp is not None:
        checks.append(("dx planes", dxp, rdx, LN_TOL["y_planes"] + delta))
    fails = []
    for nm, got, ref, bound in checks:
        e = rel_err(got, ref)
        print(f"[graded] layernorm {form} {rows}x{cols} mean/std {ratio:g} {nm}: rel_err {e:.3e}, bound {bound:.3e}{'   <-- within 3x' if not e < bound / 3 else ''}")
        if not e < bound:
            fails.append((nm, e, bound))
    assert not fails, fails
