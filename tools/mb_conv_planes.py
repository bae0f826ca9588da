"""Microbenchmark of the fp32x3 fusion convolution (768 -> 384 channels, 28 x 28 grid, bench batch 64) on the planes GEMM kernels against the register-staged
forms it replaces, and of the tile / split variants of its two tile-kernel products: python tools/mb_conv_planes.py"""
import sys
import torch
sys.path.insert(0, ".")
from pixelspointspolygons_amd import hip

B, g, D = 64, 28, 384
M, P = B * g * g, g + 2
dev = "cuda"
PEAK = 833.0            # TF: the bf16 MFMA peak over the three MFMAs of a product


def bench(fn, n=10):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


canvas, dpre, pre = torch.randn(M, 2 * D, device=dev), torch.randn(M, D, device=dev), torch.randn(M, D, device=dev)
a, b, bias = torch.randn(D, device=dev), torch.randn(D, device=dev), torch.randn(D, device=dev)
w2, wf = torch.randn(D, 9 * 2 * D, device=dev) * 0.05, torch.randn(2 * D, 9 * D, device=dev) * 0.05
w2p, wfp = hip.to_planes(w2, pad=1), hip.to_planes(wf, pad=1)
cpl = hip.pad_nhwc_planes(canvas, B, g, g)
dpl = hip.pad_nhwc_planes(dpre, B, g, g, guard=0)
out_f, out_x = torch.empty(M, D, device=dev), torch.empty(M, 2 * D, device=dev)
dW = torch.zeros(D, 9 * 2 * D, device=dev)
sums = torch.empty(2 * D, device=dev)
hip.set_deterministic(1)
FL = 2.0 * M * D * 9 * 2 * D


def old_dw():
    dp = hip.pad_nhwc(dpre, D, None, None, 0, D, D, B, g, g).view(B * P * P, D)
    cp = hip.pad_nhwc(canvas, 2 * D, None, None, 0, 2 * D, 2 * D, B, g, g).view(B * P * P, 2 * D)
    R = B * P * P
    for t in range(9):
        s = (t // 3 - 1) * P + (t % 3 - 1)
        r0, r1 = max(0, -s), R - max(0, s)
        hip.gemm_tn(dp[r0:r1], cp[r0 + s:r1 + s], out=dW[:, t * 2 * D:(t + 1) * 2 * D])


fwd = lambda **kw: hip.gemm_x3(cpl, w2p, bias=bias, out=out_f, conv=(B, g, g, 2 * D), **kw)
dx = lambda **kw: hip.gemm_x3(dpl, wfp, out=out_x, conv=(B, g, g, D), **kw)
rows = [
    ("forward  planes, library rule (head 128x384 + rest 128x128)", lambda: fwd(), FL),
    ("forward  planes, 128x384 whole", lambda: fwd(tile=2), FL),
    ("forward  planes, 128x128 whole", lambda: fwd(tile=1), FL),
    ("dX       planes, library rule (head 128x384 + rest 128x128)", lambda: dx(), FL),
    ("dX       planes, 128x384 whole", lambda: dx(tile=2), FL),
    ("dX       planes, 128x128 whole", lambda: dx(tile=1), FL),
    ("dW       planes, one launch (+ reduce)", lambda: hip.gemm_tn_x3_conv(dpl, cpl, P, out=dW), FL),
    ("pad + split canvas [M, 768]", lambda: hip.pad_nhwc_planes(canvas, B, g, g), 0.0),
    ("pad + split dpre + a + b pre [M, 384]", lambda: hip.pad_nhwc_planes(dpre, B, g, g, pre=pre, a=a, b=b, guard=0), 0.0),
    ("column statistics of pre", lambda: hip.col_stats(pre, sums), 0.0),
]
with hip.gemm_split(True):
    rows += [
        ("forward  register-staged implicit GEMM (+ statistics)", lambda: hip.gemm(canvas, w2, bias=bias, a_mode=hip.A_CONV3X3, conv=(B, g, g, 2 * D), lda=2 * D, out_dtype=torch.float32,
                                                                                   colsum=sums[:D], colsumsq=sums[D:], w_planes=(w2p.hi, w2p.lo)), FL),
        ("dX       register-staged implicit GEMM", lambda: hip.gemm(dpre, wf, a_mode=hip.A_CONV3X3, conv=(B, g, g, D), lda=D, out_dtype=torch.float32, w_planes=(wfp.hi, wfp.lo)), FL),
        ("dW       two fp32 pads + nine shifted products (+ reduces)", old_dw, FL),
        ("affine_fix dpre", lambda: hip.affine_fix(dpre, pre, a, b), 0.0),
    ]
    for name, fn, flop in rows:
        us = bench(fn)
        print(f"{name:62s} {us:9.1f} us" + (f" {flop / us / 1e6:7.1f} TF  {flop / us / 1e6 / PEAK:5.2f} of peak" if flop else ""), flush=True)
