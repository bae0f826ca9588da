"""The fp32x3 fusion convolution on the planes GEMM kernels: conv-tap addressing in the two tile kernels of p3_gemm_x3 (forward and input
gradient), the nine taps of the weight gradient as column tiles of one p3_gemm_tn_x3_conv launch, the pad-and-split pass, the column statistics pass and the
autograd node built from them (fusion_layers._FusionConvBN).  References are float64 F.conv2d / its gradients on the PLANES' OWN values (from_planes) at the
1e-5 every planes product of tests/test_x3_gpu.py is held to; every output is a view between guard bands (tests/guard.py)."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.guard import guarded
from tests.helpers import l2_err, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _h():
    import pixelspointspolygons_amd.hip as hip
    return hip


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _image(hip, x):
    """x [B, H, W, C] fp32 (host) -> (zero-bordered Planes with guard rows, the planes' own interior values [B, H, W, C] float64 on the host)"""
    B, H, W, C = x.shape
    pl = hip.pad_nhwc_planes(x.reshape(-1, C).to(DEV), B, H, W)
    own = hip.from_planes(pl).cpu().double().view(B, H + 2, W + 2, C)[:, 1:-1, 1:-1]
    return pl, own


def _border(B, H, W):
    m = torch.zeros(B, H, W, dtype=torch.bool)
    m[:, 0], m[:, -1], m[:, :, 0], m[:, :, -1] = True, True, True, True
    return m.view(-1)


def _names(hip, fn):
    hip.KTIMER.enable()
    try:
        out = fn()
        return out, set(hip.KTIMER.summary())
    finally:
        hip.KTIMER.disable()


# (3, 5, 7): M = 105 < 128 - clamp rows, non-square, ragged N = 96;  (5, 6, 6): M = 180 - a tile boundary inside an image, N = 384 on the big tile;
# (2, 6, 6, 128): K = 1152 - the library's own rule (tile 0) picks the big tile
@pytest.mark.parametrize("B,H,W,Ci,Co", [(3, 5, 7, 64, 96), (5, 6, 6, 64, 384), (2, 6, 6, 128, 384)])
@pytest.mark.parametrize("tile", [0, 1, 2])
def test_conv_forward_and_input_gradient_addressing(B, H, W, Ci, Co, tile):
    hip = _h()
    M = B * H * W
    x, w = _rand(B, H, W, Ci, seed=1), _rand(Co, Ci, 3, 3, seed=2, scale=0.1)
    bias, res = _rand(Co, seed=3), _rand(M, Co, seed=4)
    xp, x_own = _image(hip, x)
    wp = hip.to_planes(w.permute(0, 2, 3, 1).reshape(Co, 9 * Ci).contiguous().to(DEV), pad=1)                     # [Co, (ky, kx, ci)]
    w_own = hip.from_planes(wp).cpu().double().view(Co, 3, 3, Ci).permute(0, 3, 1, 2)
    ref = F.conv2d(x_own.permute(0, 3, 1, 2), w_own, padding=1).permute(0, 2, 3, 1).reshape(M, Co) + bias.double() + res.double()
    out, g = guarded(M, Co, torch.float32, ld=Co + 8, device=DEV)
    _, names = _names(hip, lambda: hip.gemm_x3(xp, wp, bias=bias.to(DEV), residual=res.to(DEV), out=out, conv=(B, H, W, Ci), tile=tile))
    g.check()
    big = (tile == 2 and Co > 128) or (tile == 0 and Co > 256 and 9 * Ci >= 1024)
    assert names == ({"gemm_x3_n384_conv_kernel"} if big else {"gemm_x3_conv_kernel<false>"}), names
    assert rel_err(out.cpu(), ref.float()) < 1e-5
    bd = _border(B, H, W)
    assert rel_err(out.cpu()[bd], ref.float()[bd]) < 1e-5                                 # border pixels of every image: where a wrong shift shows
    # input gradient: the same addressing over the gradient image with the flipped / transposed kernel [Ci, (ky', kx', co)]
    dy = _rand(B, H, W, Co, seed=5)
    dyp, dy_own = _image(hip, dy)
    wfp = hip.to_planes(w.flip(2, 3).permute(1, 2, 3, 0).reshape(Ci, 9 * Co).contiguous().to(DEV), pad=1)
    wf_own = hip.from_planes(wfp).cpu().double().view(Ci, 3, 3, Co)                       # wf[ci, ky', kx', co] = w[co, ci, 2 - ky', 2 - kx']
    w_back = wf_own.flip(1, 2).permute(3, 0, 1, 2)
    ref_dx = torch.nn.grad.conv2d_input((B, Ci, H, W), w_back, dy_own.permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1).reshape(M, Ci)
    dx, g2 = guarded(M, Ci, torch.float32, ld=Ci + 4, device=DEV)
    hip.gemm_x3(dyp, wfp, out=dx, conv=(B, H, W, Co), tile=tile)
    g2.check()
    assert rel_err(dx.cpu(), ref_dx.float()) < 1e-5
    assert rel_err(dx.cpu()[bd], ref_dx.float()[bd]) < 1e-5


def test_conv_refuses_the_a_stationary_kernel_and_bad_channel_counts():
    hip = _h()
    xp, _ = _image(hip, _rand(1, 4, 4, 64, seed=1))
    wp = hip.to_planes(_rand(64, 9 * 64, seed=2).to(DEV), pad=1)
    with pytest.raises(hip.P3Error):
        hip.gemm_x3(xp, wp, conv=(1, 4, 4, 64), tile=3)
    xq, _ = _image(hip, _rand(1, 4, 4, 48, seed=1))                  # 48 channels per tap: a 32-deep slice would straddle two taps
    with pytest.raises(hip.P3Error):
        hip.gemm_x3(xq, hip.to_planes(_rand(64, 9 * 48, seed=2).to(DEV), pad=1), conv=(1, 4, 4, 48))


def test_conv_row0_split_gives_the_bits_of_the_whole_launch():
    """M = 300 whole, and as pixels 0 .. 127 + 128 .. 299 (what the host's ragged-round split does with conv_row0 = head): the image pointer stays, the second
    launch maps its rows from pixel 128 on"""
    hip = _h()
    B, H, W, Ci, Co = 3, 10, 10, 64, 384
    xp, _ = _image(hip, _rand(B, H, W, Ci, seed=1))
    wp = hip.to_planes(_rand(Co, 9 * Ci, seed=2, scale=0.1).to(DEV), pad=1)
    bias = _rand(Co, seed=3).to(DEV)
    whole = hip.gemm_x3(xp, wp, bias=bias, conv=(B, H, W, Ci), tile=1)
    parts, g = guarded(300, Co, torch.float32, device=DEV)
    hip.gemm_x3(xp, wp, bias=bias, out=parts[:128], conv=(B, H, W, Ci), conv_rows=(0, 128), tile=1)
    hip.gemm_x3(xp, wp, bias=bias, out=parts[128:], conv=(B, H, W, Ci), conv_rows=(128, 172), tile=1)
    g.check()
    assert torch.equal(whole, parts)
    # the same split with the head on the big tile: each half against its own kernel run whole
    big = hip.gemm_x3(xp, wp, bias=bias, conv=(B, H, W, Ci), tile=2)
    head = hip.gemm_x3(xp, wp, bias=bias, conv=(B, H, W, Ci), conv_rows=(0, 128), tile=2)
    assert torch.equal(big[:128], head)


@pytest.mark.parametrize("B,H,W", [(2, 6, 6), (5, 6, 6)])            # R = 128 and 320 rows of the zero-bordered row space
@pytest.mark.parametrize("Ci,kernel", [(384, "gemm_tn_x3_wide_kernel<4>/conv"), (128, "gemm_tn_x3_kernel<4>/conv")])
def test_conv_weight_gradient_in_one_launch(B, H, W, Ci, kernel):
    hip = _h()
    N, M, Pw = 128, B * H * W, W + 2
    x, dy = _rand(B, H, W, Ci, seed=1), _rand(B, H, W, N, seed=2)
    xp, x_own = _image(hip, x)
    dyp = hip.pad_nhwc_planes(dy.reshape(M, N).to(DEV), B, H, W, guard=0)
    dy_own = hip.from_planes(dyp).cpu().double().view(B, H + 2, W + 2, N)[:, 1:-1, 1:-1]
    ref = torch.nn.grad.conv2d_weight(x_own.permute(0, 3, 1, 2), (N, Ci, 3, 3), dy_own.permute(0, 3, 1, 2), padding=1)     # [N, Ci, ky, kx]
    ref = ref.permute(0, 2, 3, 1).reshape(N, 9 * Ci)
    out, g = guarded(N, 9 * Ci, torch.float32, ld=9 * Ci + 4, device=DEV, fill=0.0)
    _, names = _names(hip, lambda: hip.gemm_tn_x3_conv(dyp, xp, Pw, out=out))
    g.check(written=False)
    assert names == {kernel}, names
    assert rel_err(out.cpu(), ref.float()) < 1e-5
    again = torch.zeros(N, 9 * Ci, device=DEV)
    hip.gemm_tn_x3_conv(dyp, xp, Pw, out=again)
    assert torch.equal(again, out)                                                        # fixed-order reduce of the split-M partial tiles
    full, guard = xp.buf._base, Pw + 1
    assert full.shape[0] == xp.rows_alloc + 2 * guard
    assert float(full[:guard].float().abs().max()) == 0.0 and float(full[guard + xp.rows:].float().abs().max()) == 0.0       # guard and tail rows still zero
    with pytest.raises(hip.P3Error):                                                      # an image without guard rows is refused, not read out of bounds
        hip.gemm_tn_x3_conv(dyp, hip.pad_nhwc_planes(x.reshape(M, Ci).to(DEV), B, H, W, guard=0), Pw, out=again)


def test_pad_and_split_pass():
    hip = _h()
    B, H, W, C = 3, 5, 7, 72
    M, R = B * H * W, B * (H + 2) * (W + 2)
    x = _rand(M, C, seed=1) * torch.logspace(-6, 6, C)
    src = torch.full((M, C + 8), float("nan"), device=DEV)                # a row stride: the padding columns are never read
    src[:, :C] = x.to(DEV)
    pl = hip.pad_nhwc_planes(src[:, :C], B, H, W)
    full, guard = pl.buf._base, W + 3
    assert pl.rows == R and pl.rows_alloc % 64 == 0 and full.shape == (pl.rows_alloc + 2 * guard, 2 * C)
    assert float(full[:guard].float().abs().max()) == 0.0 and float(full[guard + R:].float().abs().max()) == 0.0             # guard rows and the 64-row tail
    hi = pl.hi[:R].float().cpu().view(B, H + 2, W + 2, C)
    lo = pl.lo[:R].float().cpu().view(B, H + 2, W + 2, C)
    x4 = x.view(B, H, W, C)
    assert torch.equal(hi[:, 1:-1, 1:-1], x4.bfloat16().float())                          # hi = the bf16 rounding of x, lo = the bf16 rounding of the rest
    assert torch.equal(lo[:, 1:-1, 1:-1], (x4 - x4.bfloat16().float()).bfloat16().float())
    for img in (hi, lo):
        inner = img.clone()
        inner[:, 1:-1, 1:-1] = 0
        assert float(inner.abs().max()) == 0.0                                            # border pixels
    # zero columns up to a wider image
    wide = hip.pad_nhwc_planes(src[:, :C], B, H, W, guard=0, cols=128)
    assert wide.cols == 128 and torch.equal(wide.hi[:, :C], pl.hi) and torch.equal(wide.lo[:, :C], pl.lo)
    assert float(wide.buf.float()[:, C:128].abs().max()) == 0.0 and float(wide.buf.float()[:, 128 + C:].abs().max()) == 0.0
    # the fused statistics term: planes(dpre + a + b pre) == to_planes(affine_fix(dpre, pre, a, b)), bit for bit
    dpre, pre, a, b = _rand(M, C, seed=2).to(DEV), _rand(M, C, seed=3).to(DEV), _rand(C, seed=4).to(DEV), _rand(C, seed=5).to(DEV)
    fused = hip.pad_nhwc_planes(dpre, B, H, W, pre=pre, a=a, b=b, guard=0)
    fixed = dpre.clone()
    hip.affine_fix(fixed, pre, a, b)
    two = hip.to_planes(fixed)
    interior = lambda t: t[:R].view(B, H + 2, W + 2, C)[:, 1:-1, 1:-1].reshape(M, C)
    assert torch.equal(interior(fused.hi), two.hi[:M]) and torch.equal(interior(fused.lo), two.lo[:M])
    assert torch.equal(dpre.cpu(), _rand(M, C, seed=2))                                   # the fp32 gradient itself is not written


@pytest.mark.parametrize("M,N", [(1, 8), (777, 384), (5000, 64), (300, 1024)])
def test_col_stats_fixed_order(M, N):
    hip = _h()
    x = _rand(M, N, seed=1) + 0.5
    src = torch.full((M, N + 4), float("nan"), device=DEV)
    src[:, :N] = x.to(DEV)
    out, g = guarded(1, 2 * N, torch.float32, device=DEV)
    hip.col_stats(src[:, :N], out.view(-1))
    g.check()
    ref = torch.cat([x.double().sum(0), (x.double() ** 2).sum(0)])
    assert rel_err(out.view(-1).cpu(), ref.float()) < 1e-5          # fp32 partials of <= 32 .. 64 rows per lane, float64 across workgroups
    again = hip.col_stats(src[:, :N])
    assert torch.equal(again, out.view(-1))


def test_weight_planes_of_both_layouts():
    """the two weight operands of the node: planes of the re-laid-out weight == to_planes of the permuted fp32 weight, bit for bit (optimizer-less: derived
    from the parameter and cached on its version)"""
    hip = _h()
    from pixelspointspolygons_amd import ops
    w = nn.Parameter(_rand(64, 128, 3, 3, seed=1).to(DEV))
    lay = {"khwc": lambda t: t.permute(0, 2, 3, 1).reshape(t.shape[0], -1), "flipT": lambda t: t.flip(2, 3).permute(1, 2, 3, 0).reshape(t.shape[1], -1)}
    with hip.gemm_split(True):
        for key, fn in lay.items():
            hi, lo = ops.derived_planes(w, key, fn)
            want = hip.to_planes(fn(w.detach()).contiguous(), pad=1)
            assert torch.equal(hi, want.hi) and torch.equal(lo, want.lo)
            assert ops.derived_planes(w, key, fn)[0].data_ptr() == hi.data_ptr()             # cached: no second split for the same version
            with torch.no_grad():
                w.mul_(1.5)                                                               # a new version of the parameter: the planes follow, in the same buffer
            hi2, lo2 = ops.derived_planes(w, key, fn)
            want2 = hip.to_planes(fn(w.detach()).contiguous(), pad=1)
            assert torch.equal(hi2, want2.hi) and torch.equal(lo2, want2.lo) and not torch.equal(hi2, want.hi) and hi2.data_ptr() == hi.data_ptr()


class _Stub(nn.Module):
    def __init__(self, D, g):
        super().__init__()
        self.fusion_layer = nn.Sequential(nn.Conv2d(2 * D, D, kernel_size=3, padding=1), nn.BatchNorm2d(D), nn.ReLU(inplace=True))
        self.cd, self.g, self.D = torch.float32, g, D


def _node_run(B, g, D, planes):
    """one forward + backward of the node and of the tokens_assemble node that applies its scale / shift -> dict of host tensors"""
    hip = _h()
    from pixelspointspolygons_amd import fusion_layers as fl
    from pixelspointspolygons_amd.vision_transformer import _Assemble
    torch.manual_seed(0)
    mod = _Stub(D, g).to(DEV).train()
    with torch.no_grad():
        mod.fusion_layer[1].weight.copy_(0.5 + _rand(D, seed=11).abs().to(DEV))
        mod.fusion_layer[1].bias.copy_(_rand(D, seed=12).to(DEV) * 0.3)
    conv, bn = mod.fusion_layer[0], mod.fusion_layer[1]
    canvas = _rand(B, g * g, 2 * D, seed=1).to(DEV).requires_grad_(True)
    cls, pos = torch.zeros(1, 1, D, device=DEV), _rand(1, g * g + 1, D, seed=2).to(DEV) * 0.1
    G = _rand(B, g * g + 1, D, seed=3).to(DEV)
    was = fl.CONV_PLANES[0]
    fl.CONV_PLANES[0] = planes
    try:
        with hip.gemm_split(True):
            hip.KTIMER.enable()
            try:
                pre, scale, shift, mean = fl._FusionConvBN.apply(canvas, conv.weight, conv.bias, bn.weight, bn.bias, mod, B)
                x = _Assemble.apply(pre, cls, pos, scale, shift, B, g * g, D, None, mean)
                (x * G).sum().backward()
                names = set(hip.KTIMER.summary())
            finally:
                hip.KTIMER.disable()
    finally:
        fl.CONV_PLANES[0] = was
    out = dict(pre=pre, scale=scale, shift=shift, x=x, rmean=bn.running_mean, rvar=bn.running_var, dcanvas=canvas.grad, dw=conv.weight.grad,
               dgamma=bn.weight.grad, dbeta=bn.bias.grad)
    state = dict(w=conv.weight, b=conv.bias, gamma=bn.weight, beta=bn.bias, canvas=canvas, pos=pos, G=G)
    return {k: v.detach().cpu().clone() for k, v in out.items()}, {k: v.detach().cpu() for k, v in state.items()}, names


def test_fusion_conv_bn_node_on_planes():
    """_FusionConvBN on a stub module (B = 2, g = 6, D = 64), train mode, inside an fp32x3 scope: against float64 autograd, against fusion_layers.CONV_PLANES off, and twice.
    Tolerance: 2e-5 in the l2 metric - what tests/test_backward_gpu.py holds its fp32x3 BatchNorm node (test_pair_bwd_fused_x3...) to: a split product carries
    2^-17 per term, the BatchNorm statistics and coefficients are fp32 sums reduced in float64; the ReLU decisions of a handful of elements within that error of
    the kink differ, which the l2 metric absorbs."""
    B, g, D = 2, 6, 64
    got, st, names = _node_run(B, g, D, True)
    assert {"gemm_x3_conv_kernel<false>", "pad_nhwc_planes_kernel", "pad_nhwc_planes_kernel<fix>", "col_stats_kernel", "gemm_tn_x3_kernel<4>/conv"} <= names, names
    assert not any(k.startswith("gemm_kernel") or k.startswith("gemm_tn_kernel") for k in names), names            # nothing on the register-staged family
    # float64 reference
    c = st["canvas"].double().view(B, g, g, 2 * D).permute(0, 3, 1, 2).requires_grad_(True)
    w, b = st["w"].double().requires_grad_(True), st["b"].double().requires_grad_(True)
    gamma, beta = st["gamma"].double().requires_grad_(True), st["beta"].double().requires_grad_(True)
    rm, rv = torch.zeros(D, dtype=torch.float64), torch.ones(D, dtype=torch.float64)
    pre = F.conv2d(c, w, b, padding=1)
    y = F.relu(F.batch_norm(pre, rm, rv, gamma, beta, training=True, momentum=0.1, eps=1e-5))
    tok = y.permute(0, 2, 3, 1).reshape(B, g * g, D) + st["pos"].double()[:, 1:]
    (tok * st["G"].double()[:, 1:]).sum().backward()
    pre_tok = pre.detach().permute(0, 2, 3, 1).reshape(B * g * g, D)
    tol = 2e-5
    assert l2_err(got["pre"], pre_tok) < tol
    assert l2_err(got["x"][:, 1:], tok.detach()) < tol
    assert l2_err(got["pre"] * got["scale"] + got["shift"], F.batch_norm(pre.detach(), None, None, gamma.detach(), beta.detach(), training=True)
                  .permute(0, 2, 3, 1).reshape(B * g * g, D)) < tol                      # scale / shift applied
    assert l2_err(got["rmean"], rm) < tol and l2_err(got["rvar"], rv) < tol
    assert l2_err(got["dcanvas"].view(B, g, g, 2 * D), c.grad.permute(0, 2, 3, 1)) < tol
    assert l2_err(got["dw"], w.grad) < tol
    assert l2_err(got["dgamma"], gamma.grad) < tol and l2_err(got["dbeta"], beta.grad) < tol
    # the register-staged path of the parent
    old, _, names0 = _node_run(B, g, D, False)
    assert not any("conv_kernel" in k or "planes" in k for k in names0), names0
    for k in got:
        assert l2_err(got[k], old[k]) < tol, k
    # bit-reproducible
    again, _, _ = _node_run(B, g, D, True)
    for k in got:
        assert torch.equal(got[k], again[k]), k
