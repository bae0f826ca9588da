"""Guard-band tests of the dense kernels (GEMM family, weight gradients, planes kernels, attention, LayerNorm and a few neighbours): every output is a view
into a sentinel-filled buffer (tests/guard.py), every strided input a view into a NaN-filled one, at the smallest shapes that put one row and one 8-column
group past a tile edge.  Each case asserts (1) the kernel the dispatch rule was meant to pick ran, (2) nothing outside the output views changed and every
valid element was written, (3) the views equal a float64 reference computed from the operands' own (rounded) values, at the tolerance the existing test of
that kernel and dtype uses (test_ops_gpu.py, test_x3_gpu.py, test_backward_gpu.py) - quoted beside each table below.

The attention backward, the planes conversions and the elementwise neighbours (affine_fix, colsum, ce_loss_bwd) have one kernel per dtype behind their
entry point and record no name; every other case reads p3_last_kernel() under tracing."""
import contextlib
import math
from ctypes import byref, c_float, c_int, c_int64

import pytest
import torch
import torch.nn.functional as F

from tests.guard import guarded, poisoned
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")


def _h():
    import pixelspointspolygons_amd.hip as h
    return h


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _launch(fn):
    """one launch under kernel tracing -> (its result, the kernel name the library recorded for it: '' where the launch site records none)"""
    L = _h().lib()
    L.p3_trace_kernels(1)                       # also forgets the previous launch's name
    try:
        r = fn()
        return r, L.p3_last_kernel().decode()
    finally:
        L.p3_trace_kernels(0)


def _close(what, got, ref, tol):
    """rel_err(got, ref) < tol, with the measured value printed first (a margin below 3x is marked)"""
    e = rel_err(got.cpu(), ref)
    print(f"[bounds] {what}: rel_err {e:.3e}, tol {tol:.0e}{'   <-- within 3x' if not e < tol / 3 else ''}")
    assert e < tol, (what, e, tol)


def _scope(split):
    return _h().gemm_split(True) if split else contextlib.nullcontext()


def _up8(n):
    return (n + 7) // 8 * 8


def _vec(n, fill=None):
    """guarded float32 vector [n] (column sums, row statistics, parameter gradients)"""
    v, g = guarded(1, n, F32, device=DEV, fill=fill)
    return v[0], g


def _gelu_grad(x):
    x = x.double().clone().requires_grad_(True)
    F.gelu(x).sum().backward()
    return x.grad


# ====================================================================================================================== p3_gemm
# kind -> (operand dtype, output dtype, fp32x3 scope).  Tolerances: bf16 -> bf16 5e-3 (test_gemm_bf16; GELU 6e-3: test_gemm_bf16_tall_tiles), bf16 -> f32 1e-5
# (test_gemm_bf16), f32 2e-6 plain / 3e-6 with an epilogue (test_gemm_f32_exact_path / _epilogues), fp32x3 1e-5 (test_gemm_fp32_operands_as_bf16x3);
# column sums 1e-5 in f32 (test_gemm_f32_epilogues), 2e-3 in bf16 (test_gemm_batchnorm_sums_persistent_path).
KINDS = {"bf16": (BF, BF, False), "bf16_f32": (BF, F32, False), "f32": (F32, F32, False), "x3": (F32, F32, True)}
NAME_T = {BF: "bf16", F32: "float"}


def _gemm_tol(kind, epi):
    if kind == "bf16":
        return 6e-3 if epi.startswith(("gelu", "bwd")) else 5e-3
    if kind == "f32":
        return 2e-6 if epi in ("none", "bias") else 3e-6
    return 1e-5


def _tile_kernel(kind, K, a_mode=0):
    idt, odt, split = KINDS[kind]
    if idt == BF:
        bk = 64 if (K % 64 == 0 and K >= 2048) else 32
    else:
        bk = 17 if (split and K % 32 == 0) else 16
    return f"gemm_kernel<{NAME_T[idt]}, {NAME_T[odt]}, {a_mode}, {bk}, false>"


def _gemm_case(M, N, K, kind, ldc, epi, want, variant=None, tol=None, lda=None):
    """C = epilogue(A W^T) with A and W in NaN-padded rows (row stride K + 8, three NaN rows behind the last), C / aux / the column sums guarded"""
    h = _h()
    idt, odt, split = KINDS[kind]
    tol = _gemm_tol(kind, epi) if tol is None else tol
    a, w, bias = _rand(M, K, seed=1).to(idt), _rand(N, K, seed=2, scale=0.1).to(idt), _rand(N, seed=3)
    pre = a.double() @ w.double().t()
    A = poisoned(a, ld=K + 8 if lda is None else lda, extra_rows=3, device=DEV)
    W = poisoned(w, ld=K + 8 if lda is None else lda, extra_rows=3, device=DEV)
    out, g_out = guarded(M, N, odt, ld=ldc, device=DEV)
    guards, kw, checks = {"out": g_out}, {}, []
    if epi != "none" and not epi.startswith("bwd"):
        kw["bias"] = bias.to(DEV)
        pre = pre + bias.double()
    ref = pre
    if epi.startswith("gelu"):
        aux, guards["aux"] = guarded(M, N, odt, ld=ldc, device=DEV)
        kw.update(act=h.ACT_GELU, aux=aux, aux_grad=epi == "gelu_auxgrad")
        ref = F.gelu(pre)
        checks.append(("aux", aux, _gelu_grad(pre) if epi == "gelu_auxgrad" else pre, tol))
    elif epi == "relu":
        kw["act"] = h.ACT_RELU
        ref = F.relu(pre)
    elif epi in ("res_f32", "res_bf16"):
        r = _rand(M, N, seed=4).to(F32 if epi == "res_f32" else BF)
        kw["residual"] = poisoned(r, ld=_up8(N) + 8, extra_rows=2, device=DEV)        # its own padded row stride
        ref = pre + r.double()
    elif epi == "colsum":
        cs, guards["colsum"] = _vec(N, fill=0.0)
        cq, guards["colsumsq"] = _vec(N, fill=0.0)
        kw.update(colsum=cs, colsumsq=cq)
        stol = 2e-3 if idt == BF else 1e-5
        checks += [("colsum", cs, pre.sum(0), stol), ("colsumsq", cq, (pre * pre).sum(0), stol)]
    elif epi == "drop":
        seed = torch.full((1,), 1234567, dtype=torch.int64, device=DEV)
        kw["drop"] = (seed, 7, 0.25)
    elif epi.startswith("bwd"):
        sv = _rand(M, N, seed=5).to(odt)
        act = h.ACT_GELU if epi == "bwd_gelu" else h.ACT_RELU
        kw["bwd"] = (poisoned(sv, ld=ldc, extra_rows=2, device=DEV), act, 0.5)          # the output's dtype and row stride (the wrapper's contract)
        ref = pre * (_gelu_grad(sv) if epi == "bwd_gelu" else (sv.double() > 0).double()) * 0.5
    with _scope(split):
        _, name = _launch(lambda: h.gemm(A, W, out=out, variant=variant, **kw))
    torch.cuda.synchronize()
    assert name == want, (name, want)
    for k, g in guards.items():
        try:
            g.check()
        except AssertionError as e:
            raise AssertionError(f"{k}: {e}") from None
    tag = f"gemm {kind} {M}x{N}x{K} ldc {ldc} {epi}"
    if epi == "drop":
        o = out.float().cpu()
        keep = h.dropout_apply(torch.ones(M, N, device=DEV), F32, kw["drop"]).cpu() != 0     # the mask is a function of (seed, site, row, column) only
        assert 0.70 < float(keep.float().mean()) < 0.80
        assert bool((o[~keep] == 0).all())
        _close(tag, torch.where(keep, o, torch.zeros(())), torch.where(keep, ref / 0.75, torch.zeros((), dtype=torch.float64)), tol)
    else:
        _close(tag, out.float(), ref, tol)
    for what, t, r, tl in checks:
        _close(f"{tag} {what}", t.float(), r, tl)


@pytest.mark.parametrize("kind", list(KINDS))
def test_gemm_tile_kernel_simple_vector_epilogue(kind):
    """(129, 136, 64): one row and one 8-column group past the 128 x 128 tile, ldc = N + 8 - bias only, whole 8-groups: the one-pass bf16 image / the vector stores"""
    _gemm_case(129, 136, 64, kind, 136 + 8, "bias", _tile_kernel(kind, 64))


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("pad", ["aligned", "odd"])
def test_gemm_tile_kernel_ragged_n(kind, pad):
    """(255, 227, 32): the last 8-group is cut by N.  aligned: ldc = 232 (bf16 out) / 228 (f32 out) keeps the vector epilogue, whose last group must fall back to
    element stores; odd: ldc = 233, the scalar epilogue with padding behind every row"""
    ldc = (232 if KINDS[kind][1] == BF else 228) if pad == "aligned" else 233
    _gemm_case(255, 227, 32, kind, ldc, "bias", _tile_kernel(kind, 32))


@pytest.mark.parametrize("kind", ["f32", "x3"])
def test_gemm_tile_kernel_f32_four_column_tail(kind):
    """(130, 132, 96): N % 8 == 4 - an aligned fp32 row whose last 8-group holds four columns"""
    _gemm_case(130, 132, 96, kind, 136, "bias", _tile_kernel(kind, 96))


@pytest.mark.parametrize("kind", ["bf16", "bf16_f32"])
def test_gemm_tile_kernel_64_deep_slices(kind):
    _gemm_case(129, 136, 2048, kind, 144, "bias", _tile_kernel(kind, 2048))


EPILOGUES = ["gelu_aux", "gelu_auxgrad", "relu", "res_f32", "res_bf16", "colsum", "drop", "bwd_gelu", "bwd_relu"]


@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("kind", ["bf16", "f32"])
def test_gemm_tile_kernel_epilogues_on_the_ragged_shape(kind, epi):
    """every epilogue once on (255, 227, 32) with an aligned padded ldc: the vector path with the last group cut; out, aux and both column-sum vectors guarded"""
    _gemm_case(255, 227, 32, kind, 232, epi, _tile_kernel(kind, 32))


@pytest.mark.parametrize("epi", ["gelu_aux", "res_f32", "colsum"])
@pytest.mark.parametrize("kind", ["bf16_f32", "x3"])
def test_gemm_tile_kernel_epilogues_other_kinds(kind, epi):
    _gemm_case(255, 227, 32, kind, 228, epi, _tile_kernel(kind, 32))


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("conv_pad", [False, True])
def test_gemm_implicit_conv3x3_border_gather(dtype, conv_pad):
    """B = 2, H = 5, W = 7, C = 32 -> N = 40 with NaN bands directly in front of and behind the NHWC buffer and NaN row padding (lda = C + 8): a border tap that read
    row -1 or row H would pick them up.  conv_pad: the source is the zero-bordered [B, H + 2, W + 2, C] image (its border is the library's zero, not poisoned).
    Tolerance: 1e-5 (f32) / 2e-5 (bf16, fp32 out) of test_gemm_conv3x3_implicit."""
    h = _h()
    B, H, W_, C, N = 2, 5, 7, 32, 40
    x = _rand(B, C, H, W_, seed=5).to(dtype)
    wt = _rand(N, C, 3, 3, seed=6, scale=0.05).to(dtype)
    b = _rand(N, seed=7)
    ref = F.conv2d(x.double(), wt.double(), b.double(), padding=1).permute(0, 2, 3, 1).reshape(B * H * W_, N)
    nhwc = x.permute(0, 2, 3, 1).contiguous()
    if conv_pad:
        nhwc = F.pad(nhwc, (0, 0, 1, 1, 1, 1))                               # zero border around every image
    src = poisoned(nhwc.reshape(-1, C), ld=C + 8, front_rows=2 * (W_ + 2), extra_rows=2 * (W_ + 2), device=DEV)
    w2 = poisoned(wt.permute(0, 2, 3, 1).reshape(N, 9 * C).contiguous(), ld=9 * C + 8, extra_rows=3, device=DEV)
    out, g = guarded(B * H * W_, N, F32, ld=N + 8, device=DEV)
    _, name = _launch(lambda: h.gemm(src, w2, bias=b.to(DEV), a_mode=h.A_CONV3X3, conv=(B, H, W_, C), lda=C + 8, out=out, conv_pad=conv_pad))
    torch.cuda.synchronize()
    assert name == f"gemm_kernel<{NAME_T[dtype]}, float, 1, {32 if dtype == BF else 16}, false>", name
    g.check()
    _close(f"conv3x3 {NAME_T[dtype]} pad={conv_pad}", out, ref, 1e-5 if dtype == F32 else 2e-5)


def _pair_operands(Bn, n, K, N, dtype, seed=1):
    U, V = _rand(Bn * n, K, seed=seed, scale=0.7).to(dtype), _rand(Bn * n, K, seed=seed + 1, scale=0.7).to(dtype)
    sc, sh = _rand(K, seed=seed + 2).abs() + 0.5, _rand(K, seed=seed + 3) * 0.2
    w = _rand(N, K, seed=seed + 4, scale=0.08).to(dtype)
    return U, V, sc, sh, w, _rand(N, seed=seed + 5)


def test_gemm_tile_kernel_generated_a_operands():
    """P3_A_AFFINE_RELU and P3_A_PAIR_AFFINE_RELU on the tile kernel (fp32, 3e-6: test_gemm_affine_and_pair_modes): M = 2 * 9 * 9 = 162 pair rows (two row tiles,
    ragged) / 18 rows, N = 40; U and V in NaN-padded rows of one stride"""
    h = _h()
    Bn, n, K, N = 2, 9, 64, 40
    U, V, sc, sh, w, _ = _pair_operands(Bn, n, K, N, F32)
    Ud, Vd = poisoned(U, ld=K + 8, extra_rows=3, device=DEV), poisoned(V, ld=K + 8, extra_rows=3, device=DEV)
    Wd = poisoned(w, ld=K + 8, extra_rows=3, device=DEV)
    pair = (U.double().view(Bn, n, 1, K) + V.double().view(Bn, 1, n, K)).reshape(-1, K)
    out, g = guarded(Bn * n * n, N, F32, ld=N + 4, device=DEV)
    _, name = _launch(lambda: h.gemm(Ud, Wd, a_mode=h.A_PAIR_AFFINE_RELU, M=Bn * n * n, pair_v=Vd, pair_n=n, a_scale=sc.to(DEV), a_shift=sh.to(DEV), out=out))
    torch.cuda.synchronize()
    assert name == "gemm_kernel<float, float, 3, 16, false>", name
    g.check()
    _close("pair affine relu", out, F.relu(pair * sc.double() + sh.double()) @ w.double().t(), 3e-6)
    out2, g2 = guarded(Bn * n, N, F32, ld=N + 4, device=DEV)
    _, name = _launch(lambda: h.gemm(Ud, Wd, a_mode=h.A_AFFINE_RELU, a_scale=sc.to(DEV), a_shift=sh.to(DEV), out=out2))
    torch.cuda.synchronize()
    assert name == "gemm_kernel<float, float, 2, 16, false>", name
    g2.check()
    _close("affine relu", out2, F.relu(U.double() * sc.double() + sh.double()) @ w.double().t(), 3e-6)


@pytest.mark.parametrize("split", [False, True])
def test_rows_gemm_hooks_smallest_shape(split):
    """csrc/rows_gemm.hip / rows_x3.hip at the smallest M they accept (4096; dense strides are part of their rule): conv3 forward 128 -> 64 with the BatchNorm /
    ReLU operand, bias and column sums, and (bf16) the input gradient 64 -> 128 with the BN + ReLU backward epilogue.  Tolerances of
    test_rows_gemm_kernels_of_the_scorenet_conv3 (3e-3, sums 1e-5) and test_rows_x3_kernel_of_the_scorenet_conv3 (2e-5)."""
    h = _h()
    M = 4096
    dtype = F32 if split else BF
    x = _rand(M, 128, seed=1, scale=0.5).to(dtype)
    w = _rand(64, 128, seed=2, scale=0.1).to(dtype)
    bias, sc, sh = _rand(64, seed=3), torch.rand(128, generator=torch.Generator().manual_seed(4)) + 0.5, _rand(128, seed=5, scale=0.1)
    out, g = guarded(M, 64, dtype, device=DEV)
    cs, gcs = _vec(64, fill=0.0)
    cq, gcq = _vec(64, fill=0.0)
    X = poisoned(x, ld=128, extra_rows=32, device=DEV)                  # dense rows: NaN rows behind the last only
    with _scope(split):
        _, name = _launch(lambda: h.gemm(X, w.to(DEV), bias=bias.to(DEV), a_mode=h.A_AFFINE_RELU, a_scale=sc.to(DEV), a_shift=sh.to(DEV), out=out, colsum=cs, colsumsq=cq))
    torch.cuda.synchronize()
    assert name == ("rows_x3_fwd_kernel" if split else "rows_gemm_kernel<128, 64, 0>"), name
    for gg in (g, gcs, gcq):
        gg.check()
    a_ref = torch.relu(torch.addcmul(sh, x.float(), sc))                 # fma like the kernel
    a_ref = (a_ref if split else a_ref.bfloat16()).double()              # bf16: rounded to the MFMA operand
    ref = a_ref @ w.double().t() + bias.double()
    tol, stol = (2e-5, 2e-5) if split else (3e-3, 1e-5)
    _close("rows fwd", out.float(), ref, tol)
    _close("rows fwd colsum", cs, ref.sum(0), stol)
    _close("rows fwd colsumsq", cq, (ref * ref).sum(0), stol)
    if split:
        return
    dy, w3t, H = _rand(M, 64, seed=6, scale=0.5).bfloat16(), _rand(128, 64, seed=7, scale=0.1).bfloat16(), _rand(M, 128, seed=8).bfloat16()
    tab = torch.stack([torch.rand(128, generator=torch.Generator().manual_seed(9)) + 0.5, _rand(128, seed=10, scale=0.3), _rand(128, seed=11, scale=0.1),
                       _rand(128, seed=12, scale=0.1)]).contiguous()
    dx, gdx = guarded(M, 128, BF, device=DEV)
    _, name = _launch(lambda: h.gemm(poisoned(dy, ld=64, extra_rows=32, device=DEV), w3t.to(DEV), out=dx,
                                     bwd=(poisoned(H, ld=128, extra_rows=32, device=DEV), h.ACT_BN_RELU, tab.to(DEV))))
    torch.cuda.synchronize()
    assert name == "rows_gemm_kernel<64, 128, 1>", name
    gdx.check()
    z = H.double() * tab[0].double() + tab[1].double()
    ref = torch.where(z > 0, (dy.double() @ w3t.double().t()) * tab[0].double(), torch.zeros((), dtype=torch.float64)) + tab[2].double() + tab[3].double() * H.double()
    far = z.abs() > 1e-4                                                 # the kernel's fma may decide the ReLU either way at the kink
    zero = torch.zeros((), dtype=torch.float64)
    _close("rows bwd", torch.where(far, dx.float().cpu().double(), zero), torch.where(far, ref, zero), 3e-3)


@pytest.mark.parametrize("split", [False, True])
def test_pair_forward_hooks_smallest_shape(split):
    """csrc/pair_fwd_mma.hip / pair_fwd_x3.hip at the smallest pair grid they accept (B = 1, n = 8: M = 64, K = 256 -> N = 128), output and column sums guarded.
    Tolerances of test_pair_forward_kernel_of_the_scorenet_conv2 (4e-3, sums 1e-3) and its x3 twin (2e-5)."""
    h = _h()
    Bn, n = 1, 8
    dtype = F32 if split else BF
    U, V, sc, sh, w, bias = _pair_operands(Bn, n, 256, 128, dtype, seed=7)
    out, g = guarded(Bn * n * n, 128, dtype, device=DEV)
    sums, gs = _vec(256, fill=0.0)
    Ud, Vd = poisoned(U, ld=256, extra_rows=8, device=DEV), poisoned(V, ld=256, extra_rows=8, device=DEV)
    with _scope(split):
        _, name = _launch(lambda: h.gemm(Ud, w.to(DEV), bias=bias.to(DEV), a_mode=h.A_PAIR_AFFINE_RELU, M=Bn * n * n, pair_v=Vd, pair_n=n, a_scale=sc.to(DEV),
                                         a_shift=sh.to(DEV), out=out, colsum=sums[:128], colsumsq=sums[128:]))
    torch.cuda.synchronize()
    assert name == ("pair_fwd_x3_kernel" if split else "pair_fwd_mma_kernel"), name
    g.check()
    gs.check()
    if split:
        a_ref = torch.relu(torch.addcmul(torch.addcmul(sh, U.view(Bn, n, 1, 256), sc), V.view(Bn, 1, n, 256), sc)).reshape(-1, 256).double()     # fp32, the kernel's order
    else:
        pair = (U.float().view(Bn, n, 1, 256) + V.float().view(Bn, 1, n, 256)).reshape(-1, 256)
        a_ref = torch.relu(pair * sc + sh).bfloat16().double()
    ref = a_ref @ w.double().t() + bias.double()
    tol, stol = (2e-5, 2e-5) if split else (4e-3, 1e-3)
    _close("pair fwd", out.float(), ref, tol)
    _close("pair fwd colsum", sums[:128], ref.sum(0), stol)
    _close("pair fwd colsumsq", sums[128:], (ref * ref).sum(0), stol)


# ------------------------------------------------------------------------------------------------ the M <= 128 one-wave kernel
@pytest.mark.parametrize("K", [32, 1024])
@pytest.mark.parametrize("N,ldc", [(40, 40), (40, 48), (33, 40)])
@pytest.mark.parametrize("M", [1, 33, 128])
def test_gemm_skinny_kernel(M, N, ldc, K):
    """one wave per 32 x 32 block, rows and weight rows clamped at the edge; K = 1024: eight waves split K.  bf16 and fp32 out, with and without a residual (its own
    padded stride).  Tolerances: fp32 out 2e-3, bf16 out 8e-3 (test_skinny_gemm_is_bit_identical_to_the_tiled_kernel)."""
    h = _h()
    a, w, bias = _rand(M, K, seed=11).bfloat16(), _rand(N, K, seed=12, scale=0.2).bfloat16(), _rand(N, seed=13)
    A, W = poisoned(a, ld=K + 8, extra_rows=3, device=DEV), poisoned(w, ld=K + 8, extra_rows=3, device=DEV)
    pre = a.double() @ w.double().t() + bias.double()
    for odt in (BF, F32):
        for res_t in (None, F32, BF):
            r = _rand(M, N, seed=15).to(res_t) if res_t is not None else None
            out, g = guarded(M, N, odt, ld=ldc, device=DEV)
            R = poisoned(r, ld=N + 3, extra_rows=2, device=DEV) if r is not None else None          # an odd stride: the kernel reads residual elements one by one
            _, name = _launch(lambda: h.gemm(A, W, bias=bias.to(DEV), residual=R, out=out))
            torch.cuda.synchronize()
            assert name == f"gemm_skinny_kernel<{8 if K >= 1024 else 1}>", name
            g.check()
            _close(f"skinny {M}x{N}x{K} ldc {ldc} out {NAME_T[odt]} res {res_t}", out.float(), pre + (r.double() if r is not None else 0.0), 8e-3 if odt == BF else 2e-3)


# ------------------------------------------------------------------------------------------------ gemm_dma.hip through variant=
DMA_NAMES = {4: "gemm_dma_kernel<{}, 64, 2>", 6: "gemm_dma_kernel<{}, 32, 2>", 9: "gemm_dma_n384_kernel<{}>"}


@pytest.mark.parametrize("epi,kind", [("bias", "bf16"), ("gelu_aux", "bf16"), ("res_f32", "bf16_f32")])
@pytest.mark.parametrize("M,N,K", [(129, 136, 64), (130, 392, 128)])
@pytest.mark.parametrize("variant", [4, 6, 9])
def test_gemm_lds_dma_kernels(variant, M, N, K, epi, kind):
    """the LDS-DMA kernels asked for by variant= (p3_gemm itself takes them from M = 2048 on): one row past the row tile, one 8-group past the 128- / 384-column
    tile ((130, 392, 128): two column tiles of the 128 x 384 form), padded lda / ldb / ldc.  They add the same MFMA blocks as the register-staged kernel
    (test_gemm_lds_dma_kernels_equal_the_register_staged_kernel), whose tolerances apply."""
    _gemm_case(M, N, K, kind, N + 8, epi, DMA_NAMES[variant].format(NAME_T[KINDS[kind][1]]), variant=variant)


# ====================================================================================================================== weight gradients
def _column_slice(t, extra_rows, dev=DEV):
    """t [M, C] as the column slice [:, 8:8 + C] of a NaN matrix [M + extra_rows, C + 16]"""
    M, C = t.shape
    wide = torch.full((M, C + 16), NAN, dtype=t.dtype)
    wide[:, 8:8 + C] = t
    return poisoned(wide, ld=C + 16, extra_rows=extra_rows, device=dev)[:, 8:8 + C]


def _accumulate_target(N, K, seed=31):
    """a guarded [N, K + 16] matrix preset to finite values; the kernel owns the column slice [:, 8:8 + K] and accumulates into it"""
    preset = _rand(N, K + 16, seed=seed)
    wide, g = guarded(N, K + 16, F32, device=DEV, fill=preset)
    own = torch.zeros(N, K + 16, dtype=torch.bool)
    own[:, 8:8 + K] = True
    return wide[:, 8:8 + K], g, own, preset[:, 8:8 + K].double()


# tolerances: fp32 1e-5 (test_gemm_tn_strided_operand_and_accumulate), bf16 1e-4 (test_gemm_tn_and_colsum: tol * 10), the LDS-DMA kernel 2e-5
# (test_gemm_tn_dma_kernel), fp32x3 1e-5 (test_gemm_tn_fp32_operands_as_bf16x3); column sums 1e-4 (fp32x3: 1e-5) of the same tests
TN_SHAPES = [(70, 136, 72, False),        # M no multiple of the 64- / 16-row step
             (257, 136, 136, False),      # more than one M split, ragged against the 128 x 128 tile
             (64, 128, 128, True),        # the smallest shape p3_gemm_tn_dma_try accepts (bf16) ...
             (72, 128, 128, False)]       # ... and its nearest neighbour it does not (M % 64)


def _gemm_tn_case(M, N, K, kind, dma):
    h = _h()
    idt, _, split = KINDS[kind]
    a, b = _rand(M, N, seed=21).to(idt), _rand(M, K, seed=22).to(idt)
    A, B = _column_slice(a, 64), _column_slice(b, 64)                   # NaN columns on both sides, 64 NaN rows behind row M
    out, g, own, preset = _accumulate_target(N, K)
    cs_preset = _rand(N, seed=32)
    cs, gcs = _vec(N, fill=cs_preset)
    with _scope(split):
        _, name = _launch(lambda: h.gemm_tn(A, B, out=out, colsum_out=cs))
    torch.cuda.synchronize()
    assert name == ("gemm_tn_dma_kernel<4>" if (dma and idt == BF) else f"gemm_tn_kernel<{NAME_T[idt]}, 0>"), name
    g.check(valid=own)
    gcs.check()
    tol = {"f32": 1e-5, "x3": 1e-5, "bf16": 2e-5 if dma else 1e-4}[kind]
    _close(f"gemm_tn {kind} {M}x{N}x{K}", out, preset + a.double().t() @ b.double(), tol)
    _close(f"gemm_tn {kind} {M}x{N}x{K} colsum", cs, cs_preset.double() + a.double().sum(0), 1e-5 if split else 1e-4)


@pytest.mark.parametrize("M,N,K,dma", TN_SHAPES)
@pytest.mark.parametrize("kind", ["bf16", "f32", "x3"])
def test_gemm_tn_accumulates_into_a_column_slice(kind, M, N, K, dma):
    _gemm_tn_case(M, N, K, kind, dma)


@pytest.fixture
def det():
    """set the deterministic level for one test; the previous level comes back afterwards (as in test_glue_kernels_gpu.py)"""
    h = _h()
    prev = h.DETERMINISTIC
    yield h.set_deterministic
    h.set_deterministic(prev)


@pytest.mark.parametrize("M,N,K,dma", [(257, 136, 136, False), (256, 128, 128, True)])
def test_gemm_tn_bf16_deterministic_slabs_and_reduce(det, M, N, K, dma):
    """level 2: the bf16 launch stores its split-M partial tiles in slabs and a reduce kernel adds them into the (strided, preset) slice"""
    det(2)
    _gemm_tn_case(M, N, K, "bf16", dma)


# ====================================================================================================================== planes kernels
def _planes_out(rows, cols, pad_ld=8):
    """a guarded Planes [rows, cols] (row stride 2 * cols + pad_ld, zero tail rows up to the 64-row multiple) -> (Planes, Guard, mask of the rows the kernel owns)"""
    h = _h()
    ra = (rows + 63) // 64 * 64
    buf, g = guarded(ra, 2 * cols, BF, ld=2 * cols + pad_ld, device=DEV)
    own = torch.zeros(ra, 2 * cols, dtype=torch.bool)
    own[:rows] = True
    if ra > rows:
        buf[rows:].zero_()                      # what the library defines as zero: must still be zero afterwards
        g.rearm()
    return h.Planes(buf, rows, cols), g, own


def _planes_in(x, pad=64):
    """fp32 [rows, cols] as Planes whose row padding is NaN (the tail rows stay the library's zero)"""
    h = _h()
    rows, cols = x.shape
    ra = (rows + pad - 1) // pad * pad
    buf = poisoned(torch.zeros(ra, 2 * cols, dtype=BF), ld=2 * cols + 8, device=DEV)
    p = h.Planes(buf, rows, cols)
    h.to_planes(x.to(DEV), out=p)
    return p


def _planes_value(p):
    return (p.hi[:p.rows].float() + p.lo[:p.rows].float()).cpu().double()


X3_NAMES = {1: "gemm_x3_kernel<{}>", 2: "gemm_x3_n384_kernel<false>", 3: "gemm_x3_as_kernel<"}
X3_TILES = [(1, 129, 136, 64), (2, 200, 392, 64), (3, 129, 160, 256)]


@contextlib.contextmanager
def _x3_tile(tile):
    L = _h().lib()
    was = L.p3_gemm_x3_tile(tile)
    try:
        yield
    finally:
        L.p3_gemm_x3_tile(was)


@pytest.mark.parametrize("tile,M,N,K", X3_TILES)
def test_gemm_x3_tiles(tile, M, N, K):
    """p3_gemm_x3 on each of its kernels (128 x 128, 128 x 384, A-stationary), forced by p3_gemm_x3_tile: fp32 out in a padded guarded view, planes out with its
    zero tail, residual / aux / multiplier in padded rows, GELU.  Against float64 of the planes' own values: 1e-5 (fp32 out), 2e-5 (planes out), aux 1e-4
    (test_gemm_x3_plain_and_epilogues / test_gemm_x3_a_stationary_kernel)."""
    h = _h()
    a, w = _rand(M, K, seed=1), _rand(N, K, seed=2, scale=0.1)
    bias, res, mul = _rand(N, seed=3), _rand(M, N, seed=4), _rand(M, N, seed=5)
    ap, wp = _planes_in(a), _planes_in(w, pad=1)
    ref = _planes_value(ap) @ _planes_value(wp).t()

    def named(name, planes):
        want = X3_NAMES[tile].format("true" if planes else "false")
        assert name.startswith(want) if tile == 3 else name == want, (name, want)
    with _x3_tile(tile):
        # bias + residual -> fp32 view
        out, g = guarded(M, N, F32, ld=N + 4, device=DEV)
        R = poisoned(res, ld=N + 8, extra_rows=2, device=DEV)
        _, name = _launch(lambda: h.gemm_x3(ap, wp, bias=bias.to(DEV), residual=R, out=out))
        torch.cuda.synchronize()
        named(name, False)
        g.check()
        _close(f"x3 tile {tile} bias+residual", out, ref + bias.double() + res.double(), 1e-5)
        # bias + GELU -> planes, aux = GELU'
        hp, gp, own = _planes_out(M, N)
        aux, ga = guarded(M, N, F32, ld=N + 12, device=DEV)
        _, name = _launch(lambda: h.gemm_x3(ap, (wp.hi, wp.lo), bias=bias.to(DEV), act=h.ACT_GELU, aux=aux, out=hp))
        torch.cuda.synchronize()
        named(name, True)
        gp.check(valid=own)
        ga.check()
        pre = ref + bias.double()
        _close(f"x3 tile {tile} gelu planes", _planes_value(hp), F.gelu(pre), 2e-5)
        _close(f"x3 tile {tile} gelu' aux", aux, _gelu_grad(pre), 1e-4)
        # multiplier -> planes
        dp, gd, own = _planes_out(M, N, pad_ld=16)
        Mu = poisoned(mul, ld=N + 4, extra_rows=2, device=DEV)
        _, name = _launch(lambda: h.gemm_x3(ap, wp, mul=Mu, out=dp))
        torch.cuda.synchronize()
        named(name, True)
        gd.check(valid=own)
        _close(f"x3 tile {tile} mul planes", _planes_value(dp), ref * mul.double(), 2e-5)


def test_gemm_tn_x3_accumulates_into_a_column_slice():
    """M = 70 rows (planes padded to 128, zero tail), N = 128, K = 256, out a preset column slice of a guarded matrix, the bias column sums guarded; 1e-5
    (test_gemm_tn_x3_weight_gradient)"""
    h = _h()
    M, N, K = 70, 128, 256
    dy, x = _rand(M, N, seed=21), _rand(M, K, seed=22)
    dyp, xp = _planes_in(dy), _planes_in(x)
    out, g, own, preset = _accumulate_target(N, K)
    cs_preset = _rand(N, seed=32)
    cs, gcs = _vec(N, fill=cs_preset)
    _, name = _launch(lambda: h.gemm_tn_x3(dyp, xp, out=out, colsum_out=cs))
    torch.cuda.synchronize()
    assert name == "gemm_tn_x3_kernel<4>", name
    g.check(valid=own)
    gcs.check()
    _close("gemm_tn_x3", out, preset + _planes_value(dyp).t() @ _planes_value(xp), 1e-5)
    _close("gemm_tn_x3 colsum", cs, cs_preset.double() + _planes_value(dyp).sum(0), 1e-5)


# the LDS-DMA weight-gradient kernels keep FOUR step buffers in LDS and three steps in flight (csrc/tn_dma_tile.h): a split with fewer steps than that fills
# less and waits for fewer.  (kernel, N, K, M, steps per split by the host's split plan - one tile: splits = min(256 / tiles, M / (2 * step rows)) -, direct):
# direct = lib().p3_gemm_tn_x3 on raw plane buffers (Planes pads its rows to 64).  128 x 3072 is 8 tiles of 128 x 384: the fewest at which the host picks the
# wide kernel, whose plan counts 32-row steps (M = 32, 64 -> one split) while it runs 16-row ones.
TN_SHORT = [("gemm_tn_dma_kernel<4>", 128, 128, 64, "1", False), ("gemm_tn_dma_kernel<4>", 128, 128, 128, "2", False),
            ("gemm_tn_dma_kernel<4>", 128, 128, 320, "3 + 2", False),                      # two uneven splits of 192 and 128 rows
            ("gemm_tn_x3_kernel<4>", 128, 128, 32, "1", True), ("gemm_tn_x3_kernel<4>", 128, 128, 96, "3", True), ("gemm_tn_x3_kernel<4>", 128, 128, 64, "2", False),
            ("gemm_tn_x3_wide_kernel<4>", 128, 3072, 32, "2", True), ("gemm_tn_x3_wide_kernel<4>", 128, 3072, 64, "4", False)]


@pytest.mark.parametrize("level", [2, None])
@pytest.mark.parametrize("kernel,N,K,M,steps,direct", TN_SHORT)
def test_gemm_tn_lds_dma_pipelines_shorter_than_their_buffers(det, kernel, N, K, M, steps, direct, level):
    """splits of 1 .. 4 steps on the three LDS-DMA weight-gradient kernels, out a preset column slice of a guarded matrix, the bias column sums preset and guarded,
    against float64 of the operands' own values: 2e-5 / column sums 1e-4 (bf16: test_gemm_tn_dma_kernel), 1e-5 both (planes: test_gemm_tn_x3_weight_gradient).
    level 2 and the default level; at level 2 a second launch gives the same bits."""
    h = _h()
    if level is not None:
        det(level)
    bf = kernel == "gemm_tn_dma_kernel<4>"
    a, b = _rand(M, N, seed=21), _rand(M, K, seed=22)
    if bf:
        a, b = a.bfloat16(), b.bfloat16()
        A, B = _column_slice(a, 64), _column_slice(b, 64)
        a64, b64 = a.double(), b.double()
        run = lambda out, cs: h.gemm_tn(A, B, out=out, colsum_out=cs)
    elif direct:
        ah, bh = a.bfloat16(), b.bfloat16()
        al, bl = (a - ah.float()).bfloat16(), (b - bh.float()).bfloat16()
        a64, b64 = ah.double() + al.double(), bh.double() + bl.double()
        P = [poisoned(t, ld=t.shape[1] + 8, extra_rows=64, device=DEV) for t in (ah, al, bh, bl)]          # NaN row padding, 64 NaN rows behind row M

        def run(out, cs):
            slabs, ns = h._tn_slabs(N, K, out)
            h.check(h.lib().p3_gemm_tn_x3(h.ptr(P[0]), h.ptr(P[1]), N + 8, h.ptr(P[2]), h.ptr(P[3]), K + 8, h.ptr(out), out.stride(0), M, N, K, h.ptr(cs),
                                          h.ptr(slabs), ns, h.stream()), "p3_gemm_tn_x3")
    else:
        ap, bp = _planes_in(a), _planes_in(b)
        a64, b64 = _planes_value(ap), _planes_value(bp)
        run = lambda out, cs: h.gemm_tn_x3(ap, bp, out=out, colsum_out=cs)
    cs_preset = _rand(N, seed=32)
    got = []
    for _ in range(2 if level == 2 else 1):
        out, g, own, preset = _accumulate_target(N, K)
        cs, gcs = _vec(N, fill=cs_preset)
        _, name = _launch(lambda: run(out, cs))
        torch.cuda.synchronize()
        assert name == kernel, (name, kernel)
        g.check(valid=own)
        gcs.check()
        got.append((out, cs))
    tag = f"{kernel} {M}x{N}x{K} ({steps} steps) level {level}"
    _close(tag, got[0][0], preset + a64.t() @ b64, 2e-5 if bf else 1e-5)
    _close(tag + " colsum", got[0][1], cs_preset.double() + a64.sum(0), 1e-4 if bf else 1e-5)
    if level == 2:
        assert torch.equal(got[1][0], got[0][0]) and torch.equal(got[1][1], got[0][1])


@pytest.mark.parametrize("rows,cols", [(1, 8), (70, 136), (129, 384)])
def test_planes_conversions_with_strided_source_and_destination(rows, cols):
    """to_planes / to_planes_into / from_planes: NaN-padded fp32 source, guarded padded destinations; the split is exact (hi = bf16(x), lo = bf16(x - hi):
    test_planes_round_trip_carries_16_significant_bits)"""
    h = _h()
    x = _rand(rows, cols, seed=1) * torch.logspace(-3, 3, cols)
    X = poisoned(x, ld=cols + 4, extra_rows=2, device=DEV)
    p, g, own = _planes_out(rows, cols)
    h.to_planes(X, out=p)
    torch.cuda.synchronize()
    g.check(valid=own)
    hi_ref = x.bfloat16()
    lo_ref = (x - hi_ref.float()).bfloat16()
    assert torch.equal(p.hi[:rows].cpu(), hi_ref) and torch.equal(p.lo[:rows].cpu(), lo_ref)
    hi, gh = guarded(rows, cols, BF, ld=cols + 8, device=DEV)
    lo, gl = guarded(rows, cols, BF, ld=cols + 8, device=DEV)
    h.to_planes_into(X, hi, lo)
    torch.cuda.synchronize()
    gh.check()
    gl.check()
    assert torch.equal(hi.cpu(), hi_ref) and torch.equal(lo.cpu(), lo_ref)
    back, gb = guarded(rows, cols, F32, ld=cols + 4, device=DEV)
    h.from_planes(p, out=back)
    torch.cuda.synchronize()
    gb.check()
    assert torch.equal(back.cpu(), hi_ref.float() + lo_ref.float())


# ====================================================================================================================== attention
ATTN_KINDS = {"f32": (F32, False), "bf16": (BF, False), "x3": (F32, True)}
ATTN_T = {"f32": "float", "bf16": "bf16_t", "x3": "f32s"}           # the kernel's operand type as the launch site spells it
# forward: o 1e-5 / 1e-2 (test_attention_forward), lse 1e-5 / 1e-4, fp32x3 1e-4 (test_attention_fp32x3_forward_backward);
# backward 2e-5 / 3e-2 (test_attention_backward), fp32x3 1e-4
ATTN_TOL = {"f32": (1e-5, 1e-5, 2e-5), "bf16": (1e-2, 1e-4, 3e-2), "x3": (1e-4, 1e-4, 1e-4)}
ATTN_SHAPES = [(128, 64, False), (129, 65, False), (127, 63, False), (129, 129, True), (37, 200, False), (1, 1, False)]


def _packed_qkv(B, Lq, Lk, Dm, dtype, seed=1, qscale=1.0):
    """q, k, v as views of ONE [B, L + 3, 3 Dm + 8] buffer: eight NaN padding columns behind every row, three NaN rows between the batches.
    -> (CPU float64 q, k, v from the rounded values; the device views)"""
    Lb, Wd = max(Lq, Lk) + 3, 3 * Dm + 8
    vals = _rand(B, Lb, 3 * Dm, seed=seed)
    vals[..., :Dm] *= qscale
    vals = vals.to(dtype)
    buf = torch.full((B, Lb, Wd), NAN, dtype=dtype)
    buf[:, :Lq, :Dm] = vals[:, :Lq, :Dm]
    buf[:, :Lk, Dm:3 * Dm] = vals[:, :Lk, Dm:]
    d = poisoned(buf.reshape(B * Lb, Wd), ld=Wd, front_rows=2, extra_rows=2, device=DEV).view(B, Lb, Wd)
    cpu = (vals[:, :Lq, :Dm].double(), vals[:, :Lk, Dm:2 * Dm].double(), vals[:, :Lk, 2 * Dm:].double())
    return cpu, (d[:, :Lq, :Dm], d[:, :Lk, Dm:2 * Dm], d[:, :Lk, 2 * Dm:])


def _guarded_blv(B, L, D, dtype, gap=3, padc=8):
    """a guarded [B, L, D] view with padded row stride (D + padc) and batch stride ((L + gap) rows) -> (view, Guard, mask of what the kernel owns)"""
    buf, g = guarded(B * (L + gap), D + padc, dtype, device=DEV)
    own = torch.zeros(B, L + gap, D + padc, dtype=torch.bool)
    own[:, :L, :D] = True
    return buf.view(B, L + gap, D + padc)[:, :L, :D], g, own.view(B * (L + gap), D + padc)


def _attn_ref64(q, k, v, H, scale, causal, kb):
    B, Lq, Dm = q.shape
    Lk, hd = k.shape[1], Dm // H
    sp = lambda t, L: t.reshape(B, L, H, hd).transpose(1, 2)
    s = sp(q, Lq) @ sp(k, Lk).transpose(-1, -2) * scale
    if kb is not None:
        s = s + kb.double().view(B, 1, 1, Lk)
    if causal:
        s = s + torch.full((Lq, Lk), float("-inf"), dtype=torch.float64).triu(1)
    return (torch.softmax(s, -1) @ sp(v, Lk)).transpose(1, 2).reshape(B, Lq, Dm), torch.logsumexp(s, -1), s


def _attn_forward_case(kind, hd, Lq, Lk, causal, bias, qscale=1.0, backward=False):
    h = _h()
    dtype, split = ATTN_KINDS[kind]
    tol_o, tol_lse, tol_g = ATTN_TOL[kind]
    B, H = 2, 2
    Dm = H * hd
    (q, k, v), (qd, kd, vd) = _packed_qkv(B, Lq, Lk, Dm, dtype, qscale=qscale)
    kb = None
    if bias:
        kb = torch.zeros(B, Lk)
        kb[:, Lk // 2:] = 1.0                      # half the keys at +1.0, as the model's PAD bias
    scale = 1.0 / math.sqrt(hd)
    if backward:
        q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    ref, lse_ref, s = _attn_ref64(q, k, v, H, scale, causal, kb)
    o, go, own_o = _guarded_blv(B, Lq, Dm, dtype)
    lse, gl = _vec(B * H * Lq)
    kbd = kb.to(DEV) if kb is not None else None
    with _scope(split):
        _, name = _launch(lambda: h.attention(qd, kd, vd, H, scale, causal=causal, key_bias=kbd, need_lse=True, out=o, lse_out=lse.view(B, H, Lq)))
    torch.cuda.synchronize()
    assert name == f"attn_fwd_kernel<{ATTN_T[kind]}, {hd}, false>", name
    go.check(valid=own_o)
    gl.check()
    tag = f"attention {kind} hd {hd} ({Lq}, {Lk}){' causal' if causal else ''}{' bias' if bias else ''}"
    _close(tag + " o", o.float(), ref.detach(), tol_o)
    _close(tag + " lse", lse.view(B, H, Lq), lse_ref.detach(), tol_lse)
    if not backward:
        return s
    do = _rand(B, Lq, Dm, seed=4).to(dtype)
    ref.backward(do.double())
    dod = torch.full((B, Lq + 3, Dm + 8), NAN, dtype=dtype)                 # dO with O's strides, NaN around it
    dod[:, :Lq, :Dm] = do
    dod = dod.to(DEV)[:, :Lq, :Dm]
    assert dod.stride() == o.stride()
    # dq | dk | dv: views of ONE packed guarded gradient buffer with the strides of q, k, v
    Lb, Wd = max(Lq, Lk) + 3, 3 * Dm + 8
    gbuf, gg = guarded(B * Lb, Wd, dtype, device=DEV)
    g3 = gbuf.view(B, Lb, Wd)
    own = torch.zeros(B, Lb, Wd, dtype=torch.bool)
    own[:, :Lq, :Dm] = True
    own[:, :Lk, Dm:3 * Dm] = True
    dq, dk, dv = g3[:, :Lq, :Dm], g3[:, :Lk, Dm:2 * Dm], g3[:, :Lk, 2 * Dm:3 * Dm]
    with _scope(split):
        h.attention_bwd(qd, kd, vd, o, lse.view(B, H, Lq), dod, H, scale, causal=causal, key_bias=kbd, dq=dq, dk=dk, dv=dv)
    torch.cuda.synchronize()
    gg.check(valid=own.view(B * Lb, Wd))
    go.check(valid=own_o)                           # the backward reads O: it must not have written around it either
    for nm, got, want in (("dq", dq, q.grad), ("dk", dk, k.grad), ("dv", dv, v.grad)):
        _close(f"{tag} {nm}", got.float(), want, tol_g)
    return s


@pytest.mark.parametrize("Lq,Lk,causal", ATTN_SHAPES)
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("kind", list(ATTN_KINDS))
def test_attention_forward_in_guarded_views(kind, hd, Lq, Lk, causal):
    for bias in (False, True):
        _attn_forward_case(kind, hd, Lq, Lk, causal, bias)


LARGE_Q = 18.0        # q ~ N(0, 18^2): the scaled scores ~ N(0, 18^2), the extremes of 2 x 2 x 129 rows x 65 keys lie past +-60


@pytest.mark.parametrize("kind", list(ATTN_KINDS))
def test_attention_forward_large_scores(kind):
    """q scaled so that the scaled scores leave the range where exp() without the row maximum subtracted still works: some row maxima above +60 and some row
    minima below -60 in the float64 reference"""
    s = _attn_forward_case(kind, 32, 129, 65, False, False, qscale=LARGE_Q)
    assert float(s.amax(-1).max()) > 60 and float(s.amin(-1).min()) < -60, (float(s.amax(-1).max()), float(s.amin(-1).min()))


@pytest.mark.parametrize("Lq,Lk,causal", [c for c in ATTN_SHAPES if c[:2] != (1, 1)])
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("kind", list(ATTN_KINDS))
def test_attention_backward_into_a_packed_guarded_gradient(kind, hd, Lq, Lk, causal):
    _attn_forward_case(kind, hd, Lq, Lk, causal, bias=(Lk % 2 == 1), backward=True)


@pytest.mark.parametrize("Lk", [1, 255, 257])
@pytest.mark.parametrize("hd", [32, 64])
def test_attention_decode_kernel_strided_kv(Lk, hd):
    """Lq = 1, bf16, no lse: attn_decode_kernel (p3_attention's rule: not causal, no dropout, Lk <= 8192, v strides % 8); k and v are column slices of a packed
    NaN-padded buffer; 8e-3 (test_decode_attention_one_query_vs_fp32_reference)"""
    h = _h()
    B, H = 3, 2
    Dm = H * hd
    (q, k, v), (qd, kd, vd) = _packed_qkv(B, 1, Lk, Dm, BF, seed=21)
    kb = (torch.rand(B, Lk, generator=torch.Generator().manual_seed(23)) < 0.2).float()
    scale = 1.0 / math.sqrt(hd)
    ref, _, _ = _attn_ref64(q, k, v, H, scale, False, kb)
    o, go, own = _guarded_blv(B, 1, Dm, BF)
    assert vd.stride(1) % 8 == 0 and vd.stride(0) % 8 == 0          # the decode kernel's eligibility rule
    _, name = _launch(lambda: h.attention(qd, kd, vd, H, scale, key_bias=kb.to(DEV), out=o))
    torch.cuda.synchronize()
    assert name == f"attn_decode_kernel<{hd}>", name
    go.check(valid=own)
    _close(f"decode attention hd {hd} Lk {Lk}", o.float(), ref, 8e-3)


def test_attention_dropout_keep_bit_words_are_guarded():
    """the keep-bit words [B * H, ceil(Lk / 32), Lq] the forward publishes: nothing outside them is written, every word is, and the bits of the keys < Lk are the
    mask p3_dropout_apply gives for (seed, site, row, key) (the bits of the last word past Lk are not specified)"""
    h = _h()
    B, H, Lq, Lk, hd = 2, 2, 129, 65, 32
    Dm = H * hd
    _, (qd, kd, vd) = _packed_qkv(B, Lq, Lk, Dm, BF)
    seed = torch.full((1,), 4242, dtype=torch.int64, device=DEV)
    drop = (seed, 9, 0.2)
    nw = (Lk + 31) // 32
    words, gw = guarded(1, B * H * nw * Lq, torch.int32, device=DEV)
    o, go, own = _guarded_blv(B, Lq, Dm, BF)
    _, name = _launch(lambda: h.attention(qd, kd, vd, H, 1.0 / math.sqrt(hd), drop=drop, drop_rows=words[0].view(B * H, nw, Lq), out=o))
    torch.cuda.synchronize()
    assert name == "attn_fwd_kernel<bf16_t, 32, true>", name
    gw.check()
    go.check(valid=own)
    keep = h.dropout_apply(torch.ones(B * H * Lq, Lk, device=DEV), F32, drop).cpu().view(B * H, Lq, Lk) != 0
    wcpu = words[0].view(B * H, nw, Lq).cpu().to(torch.int64) & 0xFFFFFFFF
    keys = torch.arange(Lk)
    got = ((wcpu[:, keys // 32, :] >> (keys % 32).view(1, Lk, 1)) & 1).bool().transpose(1, 2)          # [B * H, Lq, Lk]
    assert torch.equal(got, keep)


# ====================================================================================================================== LayerNorm
LN_ROWS, LN_COLS = [1, 3, 65], [128, 256, 384, 768, 1024]


def _ln_data(rows, cols):
    x = (_rand(rows, cols, seed=1, scale=2.0) + 0.3)
    return x, 1 + _rand(cols, seed=2, scale=0.1), _rand(cols, seed=3, scale=0.1)


@pytest.mark.parametrize("cols", LN_COLS)
@pytest.mark.parametrize("rows", LN_ROWS)
@pytest.mark.parametrize("odt", [F32, BF])
def test_layernorm_forward_strided(odt, rows, cols):
    """x in NaN-padded rows (ldx = cols + 8), y in a guarded padded view, mean / rstd guarded; 2e-6 / 5e-3 for bf16 out (test_layernorm_fwd_bwd), the row
    statistics at 1e-5"""
    h = _h()
    x, gamma, beta = _ln_data(rows, cols)
    X = poisoned(x, ld=cols + 8, extra_rows=4, device=DEV)
    y, gy = guarded(rows, cols, odt, ld=cols + 12, device=DEV)
    mean, gm = _vec(rows)
    rstd, gr = _vec(rows)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    rc, name = _launch(lambda: h.lib().p3_layernorm(h.ptr(X), h.ptr(gd), h.ptr(bd), h.ptr(y), c_int64(rows), c_int(cols), c_int(X.stride(0)), c_int(y.stride(0)),
                                                    c_float(1e-6), c_int(h.F32), c_int(h.dt(y)), h.ptr(mean), h.ptr(rstd), h.stream()))
    h.check(rc, "p3_layernorm")
    torch.cuda.synchronize()
    assert name == "ln_fwd_kernel", name
    for g in (gy, gm, gr):
        g.check()
    xd = x.double()
    _close(f"layernorm {rows}x{cols} {NAME_T[odt]}", y.float(), F.layer_norm(xd, (cols,), gamma.double(), beta.double(), 1e-6), 2e-6 if odt == F32 else 5e-3)
    _close(f"layernorm {rows}x{cols} mean", mean, xd.mean(-1), 1e-5)
    _close(f"layernorm {rows}x{cols} rstd", rstd, (xd.var(-1, unbiased=False) + 1e-6).rsqrt(), 1e-5)
    # the wrapper with out=: the same view, the same bits
    y2, gy2 = guarded(rows, cols, odt, ld=cols + 12, device=DEV)
    h.layernorm(X, gd, bd, 1e-6, out=y2)
    torch.cuda.synchronize()
    gy2.check()
    assert torch.equal(y2, y)


@pytest.mark.parametrize("cols", LN_COLS)
@pytest.mark.parametrize("rows", LN_ROWS)
@pytest.mark.parametrize("form", ["plain", "dres", "want_lo"])
def test_layernorm_backward_guarded(form, rows, cols):
    """dx, its bf16 twin and the preset dgamma / dbeta accumulators guarded (the entry takes dense rows).  plain: fp32 everywhere; dres: a residual gradient added;
    want_lo: bf16 dy, dres and the bf16 twin of dx, at the widths whose kernel writes it.  1e-5 (test_layernorm_fwd_bwd); the twin is bf16(dx) bit for bit."""
    h = _h()
    if form == "want_lo" and cols not in h.LN_TWIN_COLS:
        # at every other width the entry must refuse a twin pointer (test_layernorm_backward_twin_only_at_the_widths_its_kernel_serves covers the wrapper)
        x, gamma, _ = _ln_data(rows, cols)
        z = torch.zeros(rows, cols, device=DEV)
        lo, glo = guarded(rows, cols, BF, device=DEV)
        st, zb, gd = torch.ones(rows, device=DEV), z.bfloat16(), gamma.to(DEV)
        rc = h.lib().p3_layernorm_bwd_lo_drop(h.ptr(zb), h.ptr(z), h.ptr(gd), h.ptr(st), h.ptr(st), h.ptr(None), h.ptr(z), h.ptr(lo), None,
                                              h.ptr(None), h.ptr(None), c_int64(rows), c_int(cols), c_int(h.BF16), c_int(h.F32), c_int(h.F32), h.stream())
        torch.cuda.synchronize()
        assert rc != 0
        glo.check(written=False)                  # refused: nothing written
        return
    x, gamma, beta = _ln_data(rows, cols)
    dy = _rand(rows, cols, seed=4)
    dres = _rand(rows, cols, seed=5) if form != "plain" else None
    if form == "want_lo":
        dy = dy.bfloat16().float()
    xr = x.double().requires_grad_(True)
    gr_, br_ = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    F.layer_norm(xr, (cols,), gr_, br_, 1e-6).backward(dy.double())
    want_dx = xr.grad + (dres.double() if dres is not None else 0.0)
    xd64 = x.double()
    mean, rstd = xd64.mean(-1).float().to(DEV), (xd64.var(-1, unbiased=False) + 1e-6).rsqrt().float().to(DEV)
    dx, gdx = guarded(rows, cols, F32, device=DEV)
    lo, glo = guarded(rows, cols, BF, device=DEV) if form == "want_lo" else (None, None)
    dg_preset, db_preset = _rand(cols, seed=6), _rand(cols, seed=7)
    dg, gdg = _vec(cols, fill=dg_preset)
    db, gdb = _vec(cols, fill=db_preset)
    dyd = (dy.bfloat16() if form == "want_lo" else dy).to(DEV)
    xd, gd, dresd = x.to(DEV), gamma.to(DEV), (dres.to(DEV) if dres is not None else None)
    rc, name = _launch(lambda: h.lib().p3_layernorm_bwd_lo_drop(h.ptr(dyd), h.ptr(xd), h.ptr(gd), h.ptr(mean), h.ptr(rstd), h.ptr(dresd), h.ptr(dx), h.ptr(lo), None,
                                                                h.ptr(dg), h.ptr(db), c_int64(rows), c_int(cols), c_int(h.dt(dyd)), c_int(h.F32), c_int(h.F32), h.stream()))
    h.check(rc, "p3_layernorm_bwd")
    torch.cuda.synchronize()
    assert name == ("ln_bwd_half_kernel" if cols in (256, 384, 768) else "ln_bwd_kernel"), name      # half a wave per row at the ViT widths, a wave elsewhere
    for g in (gdx, gdg, gdb) + ((glo,) if glo is not None else ()):
        g.check()
    tag = f"layernorm_bwd {form} {rows}x{cols}"
    _close(tag + " dx", dx, want_dx, 1e-5)
    _close(tag + " dgamma", dg, dg_preset.double() + gr_.grad, 1e-5)
    _close(tag + " dbeta", db, db_preset.double() + br_.grad, 1e-5)
    if lo is not None:
        assert torch.equal(lo, dx.bfloat16())


@pytest.mark.parametrize("rows,cols", [(1, 384), (65, 256), (65, 768), (3, 128), (65, 1024)])
def test_layernorm_planes_forward_backward_guarded(rows, cols):
    """layernorm_planes (the half-wave kernel at 256 / 384 / 768 columns, the one-wave kernel elsewhere) and layernorm_bwd_planes (256 / 384 / 768): planes in guarded
    padded buffers whose tail rows stay zero, statistics and dx guarded.  3e-5 planes, 1e-5 dx and parameter gradients (test_layernorm_planes_forward_backward)."""
    h = _h()
    x, gamma, beta = _ln_data(rows, cols)
    X = poisoned(x, ld=cols + 4, extra_rows=4, device=DEV)
    yp, gy, own = _planes_out(rows, cols)
    mean, gm = _vec(rows)
    rstd, gr = _vec(rows)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    rc, name = _launch(lambda: h.lib().p3_layernorm_planes(h.ptr(X), h.ptr(gd), h.ptr(bd), h.ptr(yp.hi), h.ptr(yp.lo), c_int64(rows), c_int(cols), c_int(X.stride(0)),
                                                           c_int(yp.ld), c_float(1e-6), h.ptr(mean), h.ptr(rstd), h.stream()))
    h.check(rc, "p3_layernorm_planes")
    torch.cuda.synchronize()
    assert name == ("ln_fwd_half_planes_kernel" if cols in (256, 384, 768) else "ln_fwd_kernel"), name
    gy.check(valid=own)
    gm.check()
    gr.check()
    xr = x.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.layer_norm(xr, (cols,), g64, b64, 1e-6)
    _close(f"layernorm_planes {rows}x{cols}", _planes_value(yp), y.detach(), 3e-5)
    _close(f"layernorm_planes {rows}x{cols} mean", mean, x.double().mean(-1), 1e-5)
    if cols not in (256, 384, 768):
        return
    dy, dres = _rand(rows, cols, seed=34), _rand(rows, cols, seed=35)
    y.backward(dy.double())
    dx, gdx = guarded(rows, cols, F32, device=DEV)
    dxp, gp, own = _planes_out(rows, cols, pad_ld=16)
    dg_preset, db_preset = _rand(cols, seed=6), _rand(cols, seed=7)
    dg, gdg = _vec(cols, fill=dg_preset)
    db, gdb = _vec(cols, fill=db_preset)
    dyd, xd, dresd = dy.to(DEV), x.to(DEV), dres.to(DEV)
    rc, name = _launch(lambda: h.lib().p3_layernorm_bwd_planes(h.ptr(dyd), h.ptr(xd), h.ptr(gd), h.ptr(mean), h.ptr(rstd), h.ptr(dresd), h.ptr(dx), h.ptr(dxp.hi),
                                                               h.ptr(dxp.lo), c_int(dxp.ld), h.ptr(dg), h.ptr(db), c_int64(rows), c_int(cols), h.stream()))
    h.check(rc, "p3_layernorm_bwd_planes")
    torch.cuda.synchronize()
    assert name == "ln_bwd_half_kernel", name
    gdx.check()
    gp.check(valid=own)
    gdg.check()
    gdb.check()
    want = xr.grad + dres.double()
    _close(f"layernorm_bwd_planes {rows}x{cols} dx", dx, want, 1e-5)
    _close(f"layernorm_bwd_planes {rows}x{cols} planes", _planes_value(dxp), want, 3e-5)
    assert torch.equal(dxp.hi[:rows], dx.bfloat16())
    _close(f"layernorm_bwd_planes {rows}x{cols} dgamma", dg, dg_preset.double() + g64.grad, 1e-5)
    _close(f"layernorm_bwd_planes {rows}x{cols} dbeta", db, db_preset.double() + b64.grad, 1e-5)


# ====================================================================================================================== small neighbours
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("R,C", [(1, 8), (70, 136), (129, 256)])
def test_affine_fix_with_a_strided_h(dtype, R, C):
    """dH (dense, in place) += a + b * H with H a NaN-padded strided view (ldh, as ffl.py passes it); the elementwise tolerances of test_glue_kernels_gpu.py:
    1e-5 in fp32, bf16 rounding (2^-8) of the result in bf16"""
    h = _h()
    dH0, H = _rand(R, C, seed=1).to(dtype), _rand(R, C, seed=2).to(dtype)
    a, b = _rand(C, seed=3), _rand(C, seed=4)
    dH, g = guarded(R, C, dtype, device=DEV, fill=dH0)
    Hd = poisoned(H, ld=C + 8, extra_rows=2, device=DEV)
    h.affine_fix(dH, Hd, a.to(DEV), b.to(DEV), ldh=Hd.stride(0))
    torch.cuda.synchronize()
    g.check()
    _close(f"affine_fix {NAME_T[dtype]} {R}x{C}", dH.float(), dH0.double() + a.double() + b.double() * H.double(), 1e-5 if dtype == F32 else 2.0 ** -8)


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("M,N", [(1, 8), (70, 136), (257, 300), (2049, 36), (70, 37)])          # N = 37: the element-wise form (N % 4)
def test_colsum_with_a_strided_x_and_ragged_m(dtype, M, N):
    """hip.colsum over NaN-padded rows with NaN rows behind row M, accumulating into a preset guarded vector; 1e-4 (test_gemm_tn_and_colsum)"""
    h = _h()
    x = _rand(M, N, seed=1).to(dtype)
    X = poisoned(x, ld=N + 8, extra_rows=130, device=DEV)
    preset = _rand(N, seed=2)
    out, g = _vec(N, fill=preset)
    h.colsum(X, out=out)
    torch.cuda.synchronize()
    g.check()
    _close(f"colsum {NAME_T[dtype]} {M}x{N}", out, preset.double() + x.double().sum(0), 1e-4)


def test_batch_sum_of_a_small_batch():
    h = _h()
    x = _rand(3, 5, 28, seed=1)
    got = h.batch_sum(x.to(DEV))
    torch.cuda.synchronize()
    _close("batch_sum", got, x.double().sum(0), 1e-4)


@pytest.mark.parametrize("out_t", [F32, BF])
def test_ce_loss_bwd_pad_columns_and_surroundings(out_t):
    """p3_ce_loss_bwd with vpad > V into a guarded view of row stride vpad + 8: the pad columns [V, vpad) hold zero (the contract test_ce_loss checks on a tight
    buffer), the gradient equals float64 softmax - onehot (1e-5, bf16: its rounding), nothing behind column vpad or around the rows is touched"""
    h = _h()
    R, V, vpad, IGN = 70, 227, 240, 226
    logits = _rand(R, V, seed=232, scale=3.0)
    tgt = torch.randint(0, V, (R,), generator=torch.Generator().manual_seed(231))
    tgt[::5] = IGN
    L_ = poisoned(logits, ld=V + 5, extra_rows=2, device=DEV)
    tgtd = tgt.to(DEV)
    lse, acc = h.ce_loss_fwd(L_, tgtd, IGN)
    gscale = torch.tensor([0.7], device=DEV)
    out, g = guarded(R, vpad, out_t, ld=vpad + 8, device=DEV)
    h.check(h.lib().p3_ce_loss_bwd(h.ptr(L_), c_int(L_.stride(0)), h.ptr(tgtd), c_int(R), c_int(V), c_int(IGN), h.ptr(lse), h.ptr(acc), h.ptr(gscale), h.ptr(out),
                                   c_int(h.dt(out)), c_int(out.stride(0)), c_int(vpad), h.stream()), "p3_ce_loss_bwd")
    torch.cuda.synchronize()
    g.check()
    assert bool((out[:, V:] == 0).all()), "padding columns must be zero"
    valid = tgt != IGN
    Lr = logits.double().requires_grad_(True)
    (0.7 * F.cross_entropy(Lr, tgt, ignore_index=IGN, reduction="mean")).backward()
    _close(f"ce_loss_bwd {NAME_T[out_t]}", out[:, :V].float(), Lr.grad, 1e-5 if out_t == F32 else 2.0 ** -8)
    assert int(valid.sum()) == int(acc[1])


# ====================================================================================================================== refusals
def test_strides_the_kernels_cannot_honour_are_refused_at_the_entry():
    """the 16-byte accesses of the operand loads need aligned rows: a row stride or base that breaks them is refused (P3_EALIGN / P3_ESHAPE -> P3Error) before
    anything is launched - the guarded outputs still hold the sentinel everywhere"""
    h = _h()
    a, w = _rand(33, 32, seed=1).bfloat16(), _rand(40, 32, seed=2).bfloat16()
    out, g = guarded(33, 40, BF, ld=48, device=DEV)
    with pytest.raises(h.P3Error):
        h.gemm(poisoned(a, ld=32 + 4, device=DEV), w.to(DEV), out=out)                        # lda % 8 (bf16)
    a40, w40 = _rand(33, 40, seed=8).bfloat16().to(DEV), _rand(40, 40, seed=9).bfloat16().to(DEV)
    with pytest.raises(h.P3Error):
        h.gemm(a40[:, 4:36], w40[:, 4:36], out=out)                                            # K = 32, aligned strides, bases 8 bytes off
    o32, g32 = guarded(70, 136, F32, ld=136, device=DEV)
    at, bt = _rand(70, 136, seed=3).bfloat16(), _rand(70, 72, seed=4).bfloat16()
    with pytest.raises(h.P3Error):
        h.gemm_tn(poisoned(at, ld=136 + 4, device=DEV), bt.to(DEV), out=o32[:, :72])          # lda % 8 (bf16)
    ap, wp = _planes_in(_rand(33, 64, seed=5)), _planes_in(_rand(40, 64, seed=6), pad=1)
    o3, g3 = guarded(33, 40, F32, ld=42, device=DEV)
    with pytest.raises(h.P3Error):
        h.gemm_x3(ap, wp, out=o3)                                                              # ldc % 4 (fp32 out)
    (_, _, _), (qd, kd, vd) = _packed_qkv(1, 5, 5, 64, BF)
    o, go, own = _guarded_blv(1, 5, 64, BF)
    with pytest.raises(h.P3Error):
        h.attention(qd[:, :, 4:36], kd[:, :, 4:36], vd[:, :, 4:36], 1, 1.0, out=o[:, :, :32])  # q / k / v bases 8 bytes off
    y, gy = guarded(3, 128, F32, ld=130, device=DEV)
    x = _rand(3, 128, seed=7).to(DEV)
    with pytest.raises(h.P3Error):
        h.layernorm(x, torch.ones(128, device=DEV), torch.zeros(128, device=DEV), 1e-6, out=y)   # ldy % 4
    torch.cuda.synchronize()
    for gg in (g, g32, g3, go, gy):
        gg.check(valid=torch.zeros(gg.rows, gg.cols, dtype=torch.bool), written=False)
