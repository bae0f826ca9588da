"""Thin tensor-level bindings of the C-ABI in include/p3hip.h (PyTorch = device memory + streams only).

The library arrives declared from that header (_lib.declare: argtypes and restype of every function), so a call passes plain Python numbers, ptr(tensor),
stream() and byref(descriptor); ctypes converts each to the parameter's C type and refuses what does not fit."""
import ctypes
import math
import os
from ctypes import Structure, byref, c_float, c_int, c_int64, c_void_p

import torch

from ._lib import P3Error, check, lib

F32, BF16, F32X3 = 0, 1, 2
ACT_NONE, ACT_GELU, ACT_RELU, ACT_MUL, ACT_BN_RELU = 0, 1, 2, 3, 4
A_PLAIN, A_CONV3X3, A_AFFINE_RELU, A_PAIR_AFFINE_RELU = 0, 1, 2, 3


class _KernelTimer:
    """Per-kernel timing with HIP events recorded on the launch stream (used by bench.py for the roofline object)."""

    def __init__(self):
        self.on, self.pending = False, []

    def enable(self):
        self.on, self.pending = True, []
        lib().p3_trace_kernels(1)          # p3_gemm records which device kernel it picked (p3_last_kernel)

    def disable(self):
        self.on = False
        lib().p3_trace_kernels(0)

    def begin(self):
        if not self.on:
            return None
        e = torch.cuda.Event(enable_timing=True)
        e.record(torch.cuda.current_stream())
        return e

    def end(self, e0, name, flop=0.0, nbytes=0.0):
        if e0 is None:
            return
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record(torch.cuda.current_stream())
        self.pending.append((name, e0, e1, flop, nbytes))

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, e0, e1, flop, nbytes in self.pending:
            r = out.setdefault(name, {"ms": 0.0, "n": 0, "flop": 0.0, "bytes": 0.0})
            r["ms"] += e0.elapsed_time(e1)
            r["n"] += 1
            r["flop"] += flop
            r["bytes"] += nbytes
        return out


KTIMER = _KernelTimer()
_AMODE_NAMES = {0: "plain", 1: "conv3x3", 2: "affine_relu", 3: "pair_affine_relu", 4: "conv3x3_affine_relu"}


def dt(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise P3Error(f"unsupported dtype {t.dtype}")


# ---- precision scope of the products ('fp32x3', include/p3hip.h P3_F32X3) --------------------------------------------------------------------------
# The library takes the precision of a product PER CALL (the dtype code of the descriptor); here it is a scope that the modules of an 'fp32x3' model open around
# their forward (scope_module) and that every autograd Function of the package re-opens around its backward with the value its forward saw (@precision_scoped),
# so that two models of different precision in one process - and a bf16 model's fp32 side products - never see each other's setting.
_SPLIT = [False]


def split_now():
    return _SPLIT[0]


def dt_mm(t):
    """dtype code of a PRODUCT operand: fp32 tensors inside an 'fp32x3' scope are multiplied as bf16 x 3"""
    c = dt(t)
    return F32X3 if (c == F32 and _SPLIT[0]) else c


class gemm_split:
    """`with hip.gemm_split(True):` fp32 products launched inside the block run as bf16 x 3 (P3_F32X3); the previous setting comes back after it."""

    def __init__(self, on=True):
        self.on = bool(on)

    def __enter__(self):
        self.was, _SPLIT[0] = _SPLIT[0], self.on
        return self

    def __exit__(self, *exc):
        _SPLIT[0] = self.was
        return False


def precision_scoped(cls):
    """class decorator for torch.autograd.Function: the backward runs under the product precision the forward ran under (the autograd engine calls it later,
    from its own thread, possibly between the passes of another model)"""
    fwd, bwd = cls.forward, cls.backward

    def forward(ctx, *a):
        ctx._p3_split = _SPLIT[0]
        return fwd(ctx, *a)

    def backward(ctx, *g):
        was, _SPLIT[0] = _SPLIT[0], ctx._p3_split
        try:
            return bwd(ctx, *g)
        finally:
            _SPLIT[0] = was

    cls.forward, cls.backward = staticmethod(forward), staticmethod(backward)
    return cls


class _ScopedMethod:
    """Instance attribute that shadows a method of a scoped module: calls the CLASS's function on the module under the product precision `split`.  The module
    is held WEAKLY and `__wrapped__` is the unbound function, so module -> attribute -> module is not a reference cycle: `del model` frees the module and the
    arenas its parameters view at once, not at the next cyclic collection.  A deep copy re-binds to the copied module."""

    def __init__(self, module, name, split):
        import functools
        import weakref
        self._ref, self._name, self._split = weakref.ref(module), name, bool(split)
        functools.update_wrapper(self, getattr(type(module), name))

    def __call__(self, *a, **k):
        m = self._ref()
        if m is None:
            raise ReferenceError(f"the module of scoped method {self._name!r} is gone")
        with gemm_split(self._split):
            return getattr(type(m), self._name)(m, *a, **k)

    def __deepcopy__(self, memo):
        m = self._ref()
        twin = memo.get(id(m)) if m is not None else None
        return _ScopedMethod(twin if twin is not None else m, self._name, self._split)


def scope_module(module, split, methods=()):
    """every forward of `module` (and whatever it calls) - and every call of the named methods - runs with the product precision `split`; scopes nest"""
    stack = []
    for name in methods:
        setattr(module, name, _ScopedMethod(module, name, split))

    def pre(_m, _a):
        stack.append(_SPLIT[0])
        _SPLIT[0] = bool(split)

    def post(_m, _a, _o):
        _SPLIT[0] = stack.pop()

    module.register_forward_pre_hook(pre)
    module.register_forward_hook(post, always_call=True)
    module.p3_split = bool(split)
    return module


def tdtype(code):
    return torch.float32 if code == F32 else torch.bfloat16


def ptr(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


# Deterministic reductions (csrc/det_reduce.hip): P3_DETERMINISTIC = 0 off | 1 (default) every fp32 (parity-mode) launch | 2 bf16 too.
# A 128 MB scratch (P3_SCRATCH_MB) for workgroup / tile partials is registered with the library at the first launch of the process (one
# device per process); the GEMM's BatchNorm column sums use it in every dtype (per-tile partials + fixed-order reduce, gemm.hip launch_bk).
DETERMINISTIC = int(os.environ.get("P3_DETERMINISTIC", "1"))
_det_state = {"buf": None}
SIDE_STREAMS = [k for k in ("sn", "dw", "stem") if os.environ.get("P3_SIDE_" + k.upper(), "0") == "1"]     # ops.SIDE: branches enqueued on side streams
SCRATCH_REGIONS = 1 + len(SIDE_STREAMS)
_DET_SCRATCH_BYTES = int(os.environ.get("P3_SCRATCH_MB", "128")) << 20     # per-tile BatchNorm partials of the tall ScoreNet / FFL GEMMs: <= 103 MB


def set_deterministic(level):
    """0: atomics everywhere; 1: fp32 launches reduce workgroup partials in a fixed order (float64); 2: bf16 launches too."""
    global DETERMINISTIC
    DETERMINISTIC = int(level)
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise P3Error("set_deterministic during a hipGraph capture")
    if DETERMINISTIC <= 0:
        check(lib().p3_set_deterministic(None, 0, 0), "p3_set_deterministic")
        _det_state["buf"] = False
        return
    buf = _det_state["buf"]
    if buf is None or buf is False:
        buf = _det_state.get("keep")
        if buf is None:        # one region per launch stream (SCRATCH_REGIONS: 1 + the side streams switched on, ops.SIDE)
            buf = torch.empty(_DET_SCRATCH_BYTES * SCRATCH_REGIONS, dtype=torch.uint8, device="cuda")
            check(lib().p3_scratch_regions(SCRATCH_REGIONS), "p3_scratch_regions")
    _det_state["buf"] = _det_state["keep"] = buf      # never freed: captured hipGraphs hold its address
    check(lib().p3_set_deterministic(ptr(buf), buf.numel(), 1 if DETERMINISTIC >= 2 else 0), "p3_set_deterministic")


def det_on(t):
    """True when launches on tensors of t's dtype take the deterministic path (Python-side workspaces follow the library's rule)."""
    return DETERMINISTIC >= 2 or (DETERMINISTIC == 1 and t.dtype == torch.float32)


_cur_stream = [None]


def register_side_stream(s):
    check(0 if lib().p3_scratch_side_stream(s.cuda_stream) > 0 else -1, "p3_scratch_side_stream")
    _cur_stream[0] = None


def stream():
    """the launch stream (torch's current stream); the library is told whenever it changes so that scratch regions follow the stream"""
    if _det_state["buf"] is None:
        set_deterministic(DETERMINISTIC)
    h = torch.cuda.current_stream().cuda_stream
    if h != _cur_stream[0]:
        _cur_stream[0] = h
        lib().p3_scratch_stream(h)
    return c_void_p(h)


def _dev(t):
    if not t.is_cuda:
        raise P3Error("p3hip ops need device tensors (there is no CPU path)")


class Dropout(Structure):
    """p3_dropout: (device seed pointer, site id, p).  Built from a python triple (seed_tensor int64[1], site, p) by _drop()."""
    _fields_ = [("seed", c_void_p), ("site", ctypes.c_uint), ("p", c_float)]


def _drop(spec):
    d = Dropout()
    if spec is not None and spec[2] > 0.0:
        d.seed, d.site, d.p = spec[0].data_ptr(), int(spec[1]), float(spec[2])
    return d


class GemmDesc(Structure):
    _fields_ = [("M", c_int), ("N", c_int), ("K", c_int), ("lda", c_int), ("ldb", c_int), ("ldc", c_int),
                ("dtype_in", c_int), ("dtype_out", c_int), ("act", c_int), ("a_mode", c_int),
                ("bias", c_void_p), ("residual", c_void_p), ("ldr", c_int), ("dtype_res", c_int), ("aux", c_void_p),
                ("conv_H", c_int), ("conv_W", c_int), ("conv_C", c_int),
                ("a_scale", c_void_p), ("a_shift", c_void_p), ("pair_V", c_void_p), ("pair_n", c_int),
                ("colsum", c_void_p), ("colsumsq", c_void_p), ("drop", Dropout),
                ("bwd_saved", c_void_p), ("bwd_act", c_int), ("bwd_scale", c_float), ("aux_mode", c_int), ("conv_pad", c_int),
                ("bwd_bn", c_void_p), ("w_lo", c_void_p)]


def w_planes_fit(wp, K):
    """can the register-staged fp32x3 GEMM take the weight as these (hi, lo) planes ([N, K] bf16, one row stride % 8, 16-byte aligned, K % 32 == 0)?"""
    wh, wl = wp
    return (wh.dim() == 2 and wh.shape[1] == K and K % 32 == 0 and wh.dtype == torch.bfloat16 and wl.dtype == torch.bfloat16 and wh.shape == wl.shape
            and wh.stride() == wl.stride() and wh.stride(1) == 1 and wh.stride(0) % 8 == 0 and wh.data_ptr() % 16 == 0 and wl.data_ptr() % 16 == 0)


def gemm(a, w, *, bias=None, act=ACT_NONE, residual=None, out=None, out_dtype=None, aux=None, M=None,
         a_mode=A_PLAIN, conv=None, a_scale=None, a_shift=None, pair_v=None, pair_n=0, colsum=None, colsumsq=None,
         lda=None, ldc=None, drop=None, bwd=None, aux_grad=False, conv_pad=False, variant=None, w_planes=None):
    """C[M,N] = drop(act(A'[M,K] @ W[N,K]^T + bias)) + residual.  a: [..., K] (2-D view), w: [N, K].  drop = (seed, site, p).
    variant = 4 | 6 | 9: call that LDS-DMA kernel (p3_gemm_dma, csrc/gemm_dma.hip) directly instead of p3_gemm's own choice (A/B tools, tests).
    w_planes = (hi, lo) bf16 [N, K] views of w's split (fp32x3 scope, plain or 3x3-gathered A): the kernel copies them instead of splitting w per tile."""
    _dev(a)
    wpl = None
    if w is None:                                   # the weight exists as planes only (ops.wpl_T_registered): the caller checked w_planes_fit
        if w_planes is None or not w_planes_fit(w_planes, a.shape[-1]) or dt_mm(a) != F32X3 or a_mode != A_PLAIN:
            raise P3Error("gemm: w = None needs fitting weight planes, a plain A and an fp32x3 scope")
        wpl = w_planes
        N, K = wpl[0].shape
    else:
        N, K = w.shape
        # (planes that are handed in and fit are used)
        if w_planes is not None and dt_mm(a) == F32X3 and a_mode in (A_PLAIN, A_CONV3X3, A_CONV3X3_AFFINE_RELU) and tuple(w_planes[0].shape) == (N, K) \
                and w_planes_fit(w_planes, K):
            wpl = w_planes
    if a_mode in (A_CONV3X3, A_CONV3X3_AFFINE_RELU):
        B, H, W_, C = conv
        M_ = B * H * W_
        lda_ = lda if lda is not None else a.stride(-2)
    elif a_mode == A_PAIR_AFFINE_RELU:
        M_ = M
        lda_ = a.stride(-2)
    else:
        a2 = a.reshape(-1, a.shape[-1]) if a.dim() != 2 else a
        M_ = a2.shape[0] if M is None else M
        lda_ = a2.stride(0) if lda is None else lda
    odt = out_dtype if out_dtype is not None else (out.dtype if out is not None else a.dtype)
    if out is None:
        out = torch.empty((M_, N), dtype=odt, device=a.device)
    d = GemmDesc()
    d.M, d.N, d.K = M_, N, K
    d.lda, d.ldb, d.ldc = lda_, (w.stride(0) if w is not None else wpl[0].stride(0)), (out.stride(-2) if ldc is None else ldc)
    d.dtype_in, d.dtype_out, d.act, d.a_mode = dt_mm(a), dt(out), act, a_mode
    if w is not None and w.dtype != a.dtype:
        raise P3Error("gemm: A and W dtypes differ")
    if wpl is not None:
        d.ldb, d.w_lo = wpl[0].stride(0), wpl[1].data_ptr()
    d.bias = bias.data_ptr() if bias is not None else None
    if residual is not None:
        d.residual, d.ldr, d.dtype_res = residual.data_ptr(), residual.stride(-2), dt(residual)
    if aux is not None:
        d.aux = aux.data_ptr()
        d.aux_mode = 1 if aux_grad else 0          # aux receives act'(pre) instead of the pre-activation
    if conv is not None:
        d.conv_H, d.conv_W, d.conv_C = conv[1], conv[2], conv[3]
        d.conv_pad = 1 if conv_pad else 0
    if a_scale is not None:
        d.a_scale, d.a_shift = a_scale.data_ptr(), a_shift.data_ptr()
    if pair_v is not None:
        d.pair_V, d.pair_n = pair_v.data_ptr(), pair_n
    if colsum is not None:
        d.colsum, d.colsumsq = colsum.data_ptr(), colsumsq.data_ptr()
    d.drop = _drop(drop)
    if bwd is not None:            # (saved tensor [M,N] in the output dtype, act, scale): out *= act'(saved) * scale
        sv, bact, bscale = bwd
        if sv.dtype != out.dtype or sv.stride(-2) != out.stride(-2):
            raise P3Error("gemm: bwd_saved must match the output's dtype and row stride")
        d.bwd_saved, d.bwd_act = sv.data_ptr(), bact
        if bact == ACT_BN_RELU:    # bscale = the [4, N] float table (scale | shift | a | b): the BatchNorm + ReLU backward of the layer in front
            if bscale.dtype != torch.float32 or tuple(bscale.shape) != (4, N) or not bscale.is_contiguous():
                raise P3Error("gemm: ACT_BN_RELU needs a contiguous float32 [4, N] table")
            d.bwd_bn, d.bwd_scale = bscale.data_ptr(), 1.0
        else:
            d.bwd_scale = bscale
    ev = KTIMER.begin()
    if variant is not None:
        check(lib().p3_gemm_dma(ptr(a), ptr(w), ptr(out), byref(d), int(variant), stream()), "p3_gemm_dma")
    else:
        check(lib().p3_gemm(ptr(a), ptr(wpl[0] if wpl is not None else w), ptr(out), byref(d), stream()), "p3_gemm")
    if ev is not None:
        # algorithmic HBM bytes of this launch: A read once (generated A: its sources), W once, C written once, residual / aux /
        # saved-activation streams once each
        esi, eso = a.element_size(), out.element_size()
        if a_mode in (A_CONV3X3, A_CONV3X3_AFFINE_RELU):
            a_bytes = M_ * conv[3] * esi
        elif a_mode == A_PAIR_AFFINE_RELU:
            a_bytes = 2 * (M_ // pair_n) * K * esi
        else:
            a_bytes = M_ * K * esi
        nbytes = a_bytes + N * K * esi + M_ * N * eso
        if residual is not None:
            nbytes += M_ * N * residual.element_size()
        if aux is not None:
            nbytes += M_ * N * eso
        if bwd is not None:
            nbytes += M_ * N * eso
        kname = lib().p3_last_kernel().decode() or f"gemm_kernel<{'bf16' if d.dtype_in == BF16 else 'f32'},{_AMODE_NAMES[a_mode]}>"
        KTIMER.end(ev, kname, 2.0 * M_ * N * K, float(nbytes))     # the name rocprofv3 prints for the kernel p3_gemm picked
    return out


def layernorm(x, gamma, beta, eps, out_dtype=None, save_stats=False, out=None):
    _dev(x)
    cols = x.shape[-1]
    x2 = x.reshape(-1, cols)
    rows = x2.shape[0]
    if out is None:
        out = torch.empty(x.shape, dtype=out_dtype or x.dtype, device=x.device)
    o2 = out.view(-1, cols)
    mean = rstd = None
    if save_stats:
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    check(lib().p3_layernorm(ptr(x2), ptr(gamma), ptr(beta), ptr(o2), rows, cols, x2.stride(0),
                             o2.stride(0), eps, dt(x), dt(out), ptr(mean), ptr(rstd),
                             stream()), "p3_layernorm")
    return (out, mean, rstd) if save_stats else out


# widths served by the half-wave LayerNorm backward kernel, the only one that writes the bf16 twin of dx (norm.hip); any other width gets
# no twin (lo = None) and the consumer casts dx itself - an uninitialised twin must never be registered
LN_TWIN_COLS = (256, 384, 768)


_park = {"buf": None}


def param_reduce_arena(mb=None):
    """register (once per process) the arena deferred parameter-gradient reduces park their partials in (p3_reduce_defer); P3_DEFER_MB, default 192"""
    if _park["buf"] is None:
        mb = int(os.environ.get("P3_DEFER_MB", "192")) if mb is None else mb
        if mb <= 0:
            return False
        _park["buf"] = torch.empty(mb * (1 << 20) // 4, dtype=torch.float32, device="cuda")
        check(lib().p3_reduce_defer(ptr(_park["buf"]), _park["buf"].numel()), "p3_reduce_defer")
    return True


_tn_park = {"buf": None}


def tn_defer_arena(mb=None):
    """register (once per process) the arena the deterministic weight-gradient GEMMs park their split-M partial tiles in (p3_tn_defer); P3_TN_DEFER_MB, default 4096 (r06: the 128 x 384 weight-gradient tile runs 21 - 28 splits per launch: 2 GB of partial tiles per backward pass of the 12 blocks)"""
    if _tn_park["buf"] is None:
        mb = int(os.environ.get("P3_TN_DEFER_MB", "4096")) if mb is None else mb
        if mb <= 0:
            _tn_park["buf"] = False
            return False
        _tn_park["buf"] = torch.empty(mb * (1 << 20) // 4, dtype=torch.float32, device="cuda")
        check(lib().p3_tn_defer(ptr(_tn_park["buf"]), _tn_park["buf"].numel()), "p3_tn_defer")
    return _tn_park["buf"] is not False


def tn_defer_release():
    """unregister and free the parking arena of the weight-gradient GEMMs (FlatAdamW.close(), ops.reset_process_state()): partial tiles still parked are dropped;
    the next optimizer - or the first parking launch - registers a new one"""
    buf = _tn_park["buf"]
    if buf is not None and buf is not False:
        lib().p3_tn_drop()
        check(lib().p3_tn_defer(ptr(None), 0), "p3_tn_defer")
    _tn_park["buf"] = None


class tn_parking:
    """`with hip.tn_parking(on):` weight-gradient launches inside may leave their split-M partial tiles parked for reduce_flush() (their outputs must be
    accumulation targets that stay valid and unread until then: views of the optimizer's gradient arena)"""

    def __init__(self, on):
        self.on = bool(on) and DETERMINISTIC >= 1 and tn_defer_arena()
        # r06: the launch's bias-gradient column sums (colsum_out = a view of the gradient arena) park with the deferred parameter reduces (p3_reduce_park) - one
        # det_reduce launch of ~6 us less per Linear and train step
        self.on_colsum = self.on and param_reduce_arena()

    def __enter__(self):
        if self.on:
            lib().p3_tn_defer_enable(1)
        if self.on_colsum:
            lib().p3_reduce_defer_enable(1)
        return self

    def __exit__(self, *exc):
        if self.on:
            lib().p3_tn_defer_enable(0)
        if self.on_colsum:
            lib().p3_reduce_defer_enable(0)
        return False


def reduce_pending():
    return int(lib().p3_reduce_pending()) + int(lib().p3_tn_pending())


def reduce_flush():
    check(lib().p3_reduce_flush(stream()), "p3_reduce_flush")
    if lib().p3_tn_pending():
        check(lib().p3_tn_flush(stream()), "p3_tn_flush")


def reduce_drop():
    return int(lib().p3_reduce_drop()) + int(lib().p3_tn_drop())


def layernorm_bwd(dy, x, gamma, mean, rstd, dx_dtype=None, dgamma=None, dbeta=None, dres=None, want_lo=False, lo_drop=None, park=False):
    """dres: gradient that reaches x through a residual connection (same dtype as dx); summed into dx in the same pass.
    want_lo: also return a bf16 copy of an fp32 dx written by the same kernel -> (dx, dx_lo).
    lo_drop = (seed, site, p): the bf16 copy carries that dropout site's mask and 1/(1-p) (see p3_layernorm_bwd_lo_drop).
    park: dgamma / dbeta are accumulation targets that stay valid until reduce_flush() (gradient arena views): the kernel's partials may be parked
    and added by ONE launch at the end of the backward pass (p3_reduce_defer) instead of by a reduce launch of their own."""
    cols = x.shape[-1]
    dy2, x2 = dy.reshape(-1, cols).contiguous(), x.reshape(-1, cols).contiguous()
    rows = x2.shape[0]
    dx = torch.empty(x.shape, dtype=dx_dtype or x.dtype, device=x.device)
    if dres is not None:
        dres = dres.contiguous()
        if dres.dtype != dx.dtype:
            raise P3Error("layernorm_bwd: dres dtype must equal the dx dtype")
    lo = None
    if want_lo and dx.dtype == torch.float32 and cols in LN_TWIN_COLS:
        lo = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    if lo_drop is not None and lo is None:
        raise P3Error("layernorm_bwd: lo_drop needs the bf16 copy (want_lo, fp32 dx, 256 / 384 / 768 columns)")
    dspec = _drop(lo_drop)
    park = park and dgamma is not None and param_reduce_arena()
    if park:
        lib().p3_reduce_defer_enable(1)
    try:
        check(lib().p3_layernorm_bwd_lo_drop(ptr(dy2), ptr(x2), ptr(gamma), ptr(mean), ptr(rstd), ptr(dres), ptr(dx), ptr(lo),
                                             byref(dspec) if lo_drop is not None else None, ptr(dgamma), ptr(dbeta),
                                             rows, cols, dt(dy2), dt(x2), dt(dx), stream()),
              "p3_layernorm_bwd")
    finally:
        if park:
            lib().p3_reduce_defer_enable(0)
    return (dx, lo) if want_lo else dx


class AttnDesc(Structure):
    _fields_ = [("B", c_int), ("H", c_int), ("Lq", c_int), ("Lk", c_int), ("head_dim", c_int),
                ("q_bs", c_int64), ("k_bs", c_int64), ("v_bs", c_int64), ("o_bs", c_int64),
                ("q_rs", c_int), ("k_rs", c_int), ("v_rs", c_int), ("o_rs", c_int),
                ("scale", c_float), ("causal", c_int), ("key_bias", c_void_p), ("dtype", c_int), ("lse", c_void_p),
                ("drop", Dropout), ("drop_rows", c_void_p), ("grad_planes", c_int), ("g_rs", c_int), ("g_bs", c_int64), ("g_lo", c_int64),
                ("o_planes", c_void_p), ("op_rs", c_int), ("op_bs", c_int64), ("op_lo", c_int64)]


def _attn_desc(q, k, v, o, heads, scale, causal, key_bias, lse, drop=None, drop_rows=None):
    B, Lq, Dm = q.shape
    Lk = k.shape[1]
    d = AttnDesc()
    d.B, d.H, d.Lq, d.Lk, d.head_dim = B, heads, Lq, Lk, Dm // heads
    d.q_bs, d.k_bs, d.v_bs, d.o_bs = q.stride(0), k.stride(0), v.stride(0), o.stride(0)
    d.q_rs, d.k_rs, d.v_rs, d.o_rs = q.stride(1), k.stride(1), v.stride(1), o.stride(1)
    d.scale, d.causal, d.dtype = scale, int(causal), dt_mm(q)
    d.key_bias = key_bias.data_ptr() if key_bias is not None else None
    d.lse = lse.data_ptr() if lse is not None else None
    d.drop = _drop(drop)
    d.drop_rows = drop_rows.data_ptr() if drop_rows is not None else None
    return d


def attention(q, k, v, heads, scale, causal=False, key_bias=None, need_lse=False, drop=None, drop_rows=None, out_planes=None, out=None, lse_out=None):
    """q [B,Lq,H*D], k/v [B,Lk,H*D] (arbitrary batch/row strides, unit inner stride) -> o [B,Lq,H*D].
    out: the tensor that receives o (q's shape and dtype, unit inner stride, batch and row strides free: a view of a larger buffer); default a new dense one.
    lse_out (with need_lse): the contiguous float32 [B, heads, Lq] tensor that receives the log-sum-exp rows.
    out_planes (fp32x3 scope): a Planes [B * Lq, H*D] that receives the output as planes too (the output projection's operand), written by the same launch."""
    _dev(q)
    for t in (q, k, v):
        if t.stride(2) != 1:
            raise P3Error("attention: inner stride must be 1")
    if out is None:
        o = torch.empty((q.shape[0], q.shape[1], q.shape[2]), dtype=q.dtype, device=q.device)
    else:
        if out.shape != q.shape or out.dtype != q.dtype or out.device != q.device or out.stride(2) != 1:
            raise P3Error("attention: out must have q's shape, dtype and device and unit inner stride")
        o = out
    lse = None
    if need_lse:
        lse = lse_out if lse_out is not None else torch.empty((q.shape[0], heads, q.shape[1]), dtype=torch.float32, device=q.device)
        if tuple(lse.shape) != (q.shape[0], heads, q.shape[1]) or lse.dtype != torch.float32 or not lse.is_contiguous():
            raise P3Error("attention: lse_out must be a contiguous float32 [B, heads, Lq] tensor")
    d = _attn_desc(q, k, v, o, heads, scale, causal, key_bias, lse, drop, drop_rows)
    if out_planes is not None:
        op = out_planes
        if op.rows != q.shape[0] * q.shape[1] or op.cols != q.shape[2] or not split_now():
            raise P3Error("attention: out_planes must be [B * Lq, H * D] and the call must run in an fp32x3 scope")
        d.o_planes, d.op_rs, d.op_bs, d.op_lo = op.hi.data_ptr(), op.ld, q.shape[1] * op.ld, op.cols
    ev = KTIMER.begin()
    check(lib().p3_attention(ptr(q), ptr(k), ptr(v), ptr(o), byref(d), stream()), "p3_attention")
    KTIMER.end(ev, f"attn_fwd_kernel<{'bf16' if d.dtype == BF16 else 'f32'},{d.head_dim}>",
               4.0 * d.B * d.H * d.Lq * d.Lk * d.head_dim * (0.5 if causal else 1.0))
    return (o, lse) if need_lse else o


# ------------------------------------------------------------------------------------------ pillar stem
class PillarDesc(Structure):
    _fields_ = [("B", c_int), ("total_points", c_int64), ("nx", c_int), ("ny", c_int), ("vx", c_float), ("vy", c_float),
                ("vz", c_float), ("zmax", c_float), ("max_points", c_int), ("max_voxels", c_int), ("C", c_int),
                ("training", c_int), ("bn_eps", c_float), ("bn_momentum", c_float), ("dtype", c_int), ("out_ld", c_int),
                ("out_col_off", c_int), ("no_backward", c_int)]


_ws_cache = {}
_ws_retired = []     # superseded buffers: a captured hipGraph may still hold their addresses, so they are never handed back


def workspace(nbytes, device, tag="default"):
    """Grow-only scratch buffer per (device, tag): avoids allocator traffic inside the step / graph capture.  A buffer that has to
    grow is replaced, and the old one is kept alive for the life of the process (a graph captured at the smaller size replays into
    it; freeing it would let the caching allocator hand that memory to other tensors).  Growing DURING a capture would allocate
    from the graph's private pool and leave eager callers with a pointer the graph owns: refused."""
    key = (str(device), tag, torch.cuda.current_stream().cuda_stream if SCRATCH_REGIONS > 1 else 0)     # a side stream's launches get buffers of their own
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise P3Error(f"workspace '{tag}' must grow from {buf.numel()} to {nbytes} bytes while a hipGraph is being captured: run the "
                          "largest shape once eagerly before capturing")
        if buf is not None:
            _ws_retired.append(buf)
        buf = torch.empty(int(nbytes * 1.25) + 256, dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def pillar_stem(values, offsets, w1, bn1, w2, bn2, out, *, B, grid, voxel, zmax, max_points, max_voxels, training,
                col_off=0, total_points=None, keep_workspace=False, sync=None, phases=None):
    """bn1 / bn2 = (gamma, beta, running_mean, running_var) fp32 tensors.  out: [B, ny*nx, ld] token-major canvas.
    keep_workspace: run in a workspace of its own and return (out, workspace, desc) for p3_pillar_stem_bwd.
    sync: callable(*tensors) all-reducing statistic buffers in place (SyncBatchNorm) or None.
    phases: bit mask for p3_pillar_stem_phased (1 = pillarize + layer-0 sums only: what PointPillarsEncoder.voxelize runs)."""
    _dev(values)
    d = PillarDesc()
    d.B = B
    d.total_points = values.shape[0] if total_points is None else total_points
    d.nx, d.ny = grid
    d.vx, d.vy, d.vz = voxel
    d.zmax = zmax
    d.max_points, d.max_voxels, d.C = max_points, max_voxels, w2.shape[0]
    d.training, d.bn_eps, d.bn_momentum = int(training), 1e-3, 0.01
    d.dtype, d.out_ld, d.out_col_off = dt_mm(out), out.stride(-2), col_off
    d.no_backward = int(not keep_workspace)      # a workspace nobody keeps cannot feed p3_pillar_stem_bwd
    if w2.dtype != out.dtype:
        raise P3Error("pillar_stem: w2 dtype must equal the canvas dtype")
    L = lib()
    nbytes = L.p3_pillar_stem_workspace_bytes(byref(d))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=values.device) if keep_workspace else workspace(nbytes, values.device, "pillar")
    args = (ptr(values), ptr(offsets), ptr(w1), ptr(bn1[0]), ptr(bn1[1]), ptr(bn1[2]), ptr(bn1[3]), ptr(w2),
            ptr(bn2[0]), ptr(bn2[1]), ptr(bn2[2]), ptr(bn2[3]), ptr(out), ptr(ws), byref(d))
    if phases is not None:
        check(L.p3_pillar_stem_phased(*args, int(phases), stream()), "p3_pillar_stem")
    elif sync is None or not training:
        check(L.p3_pillar_stem(*args, stream()), "p3_pillar_stem")
    else:   # SyncBatchNorm: all-reduce the pillar count / BatchNorm sums between the phases
        sec = _pillar_sections(ws, d)
        check(L.p3_pillar_stem_phased(*args, 1, stream()), "p3_pillar_stem")
        sync(sec["totals"], sec["sums1"])
        check(L.p3_pillar_stem_phased(*args, 2, stream()), "p3_pillar_stem")
        sync(sec["sums2"])
        check(L.p3_pillar_stem_phased(*args, 4, stream()), "p3_pillar_stem")
    return (out, ws, d) if keep_workspace else out


# the sections of a stem workspace in the order p3_pillar_stem_layout returns their byte offsets (include/p3hip.h)
_PILLAR_SECTIONS = ("sorted", "vox_xy", "vox_start", "vox_cnt", "vox_row", "nvox", "X2", "H2", "hmax", "hmin", "F8", "row_vox", "row_w",
                    "totals", "sums1", "sums2", "acc1", "acc1_stat")


def _pillar_layout(d):
    """section name -> byte offset in a stem workspace (p3_pillar_stem_layout)"""
    off = (c_int64 * len(_PILLAR_SECTIONS))()
    check(lib().p3_pillar_stem_layout(byref(d), off), "p3_pillar_stem_layout")
    return dict(zip(_PILLAR_SECTIONS, off))


def _pillar_views(ws, d, sizes, dtypes=None):
    """{name: view of `ws`} for sizes = {name: elements of 4 bytes}; int32 unless dtypes names another type"""
    off = _pillar_layout(d)
    return {k: ws[off[k]:off[k] + 4 * n].view((dtypes or {}).get(k, torch.int32)) for k, n in sizes.items()}


def _pillar_sections(ws, d):
    f32 = torch.float32
    return _pillar_views(ws, d, dict(totals=1, sums1=64, sums2=2 * d.C, acc1_stat=64), dict(sums1=f32, sums2=f32, acc1_stat=f32))


def pillar_tables(ws, d):
    """The integer outputs of the pillar sort (Open3D `PointPillars.voxelize`, pointpillars_o3d.py:92) as int32 views of a stem workspace:
    sorted [total_points] global point ids grouped by pillar (ascending id inside a pillar), and per pillar slot b * max_voxels + s
    (s = rank of the kept pillar in ascending hash order): vox_xy (cy * nx + cx, bit 30 = the scatter skips it because the top-z pillar
    of the same (x, y) overwrites it), vox_start (first position in `sorted`), vox_cnt (= num_points, capped), vox_row; nvox [B]."""
    nv = d.B * d.max_voxels
    return _pillar_views(ws, d, dict(sorted=max(int(d.total_points), 1), vox_xy=nv, vox_start=nv, vox_cnt=nv, vox_row=nv, nvox=d.B))


def pillar_stem_bwd(dcanvas, w1, g1, w2t, g2, ws, d, sync=None):
    """-> (dw1 [32,8], dg1, db1, dw2 [C,64], dg2, db2) fp32; consumes the forward's workspace.  sync: SyncBatchNorm all-reduce."""
    dev, C = dcanvas.device, d.C
    f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    dw1, dg1, db1, dw2, dgb2 = f(32, 8), f(32), f(32), f(C, 64), f(2 * C)
    db2, dg2 = dgb2[:C], dgb2[C:]
    if dt(dcanvas) != (F32 if d.dtype == F32X3 else d.dtype):
        raise P3Error("pillar_stem_bwd: canvas gradient dtype differs from the forward's")
    args = (ptr(dcanvas), dcanvas.stride(-2), ptr(w1), ptr(g1), ptr(w2t), ptr(g2), ptr(ws), byref(d), ptr(dw1),
            ptr(dg1), ptr(db1), ptr(dw2), ptr(dg2), ptr(db2))
    L = lib()
    if sync is None or not d.training:
        check(L.p3_pillar_stem_bwd(*args, stream()), "p3_pillar_stem_bwd")
    else:
        check(L.p3_pillar_stem_bwd_phased(*args, ptr(None), ptr(None), 1, stream()), "p3_pillar_stem_bwd")
        stat2 = dgb2.clone()
        sync(stat2)
        check(L.p3_pillar_stem_bwd_phased(*args, ptr(stat2), ptr(None), 2, stream()), "p3_pillar_stem_bwd")
        stat1 = _pillar_sections(ws, d)["acc1_stat"].clone()
        sync(stat1)
        check(L.p3_pillar_stem_bwd_phased(*args, ptr(stat2), ptr(stat1), 4, stream()), "p3_pillar_stem_bwd")
    return dw1, dg1, db1, dw2, dg2, db2


# ------------------------------------------------------------------------------------------ glue ops
def patchify(img, P, dtype):
    _dev(img)
    B, Cin, H, W = img.shape
    out = torch.empty((B * (H // P) * (W // P), Cin * P * P), dtype=dtype, device=img.device)
    check(lib().p3_patchify(ptr(img), ptr(out), B, Cin, H, W, P, dt(out), stream()), "p3_patchify")
    return out


def patchify_ld(img, P, dtype, ldk):
    """patchify with rows of leading dimension ldk >= Cin*P*P; the pad columns are zeros"""
    _dev(img)
    B, Cin, H, W = img.shape
    out = torch.empty((B * (H // P) * (W // P), ldk), dtype=dtype, device=img.device)
    check(lib().p3_patchify_ld(ptr(img), ptr(out), B, Cin, H, W, P, ldk, dt(out), stream()), "p3_patchify_ld")
    return out


def bicubic_taps(n_in, n_out, scale=None):
    """[n_out, n_in] float64 tap table of torch's 1-D bicubic resampling (A = -0.75, align_corners=False, no antialias, border indices clamped):
    out[o] = sum_i taps[o, i] * in[i].  `scale`: the scale_factor handed to F.interpolate (source coordinate = (o + 0.5) / scale - 0.5);
    None: the `size=` form (source coordinate = (o + 0.5) * n_in / n_out - 0.5).  Host arithmetic only."""
    A = -0.75
    ratio = (1.0 / scale) if scale is not None else n_in / n_out
    taps = torch.zeros((n_out, n_in), dtype=torch.float64)
    for o in range(n_out):
        src = ratio * (o + 0.5) - 0.5
        i0 = math.floor(src)
        t = src - i0
        coef = (((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A,
                ((A + 2) * t - (A + 3)) * t * t + 1,
                ((A + 2) * (1 - t) - (A + 3)) * (1 - t) * (1 - t) + 1,
                ((A * (2 - t) - 5 * A) * (2 - t) + 8 * A) * (2 - t) - 4 * A)
        for k, c in enumerate(coef):
            taps[o, min(max(i0 - 1 + k, 0), n_in - 1)] += c
    return taps


def posembed_resample(table, wy, wx, n_in, n_out):
    """table [1 + n_in^2, D] fp32 -> [1 + n_out^2, D]; wy / wx: device fp32 [n_out, n_in] tap tables (bicubic_taps)"""
    _dev(table)
    D = table.shape[-1]
    if table.dtype != torch.float32 or table.shape[0] != 1 + n_in * n_in or tuple(wy.shape) != (n_out, n_in) or tuple(wx.shape) != (n_out, n_in):
        raise P3Error("posembed_resample: fp32 table [1 + n_in^2, D] and tap tables [n_out, n_in] expected")
    out = torch.empty((1 + n_out * n_out, D), dtype=torch.float32, device=table.device)
    check(lib().p3_posembed_resample(ptr(table.contiguous()), ptr(wy), ptr(wx), ptr(out), n_in, n_out, D, stream()), "p3_posembed_resample")
    return out


def posembed_resample_bwd(dout, wy, wx, n_in, n_out):
    _dev(dout)
    D = dout.shape[-1]
    if dout.dtype != torch.float32 or dout.shape[0] != 1 + n_out * n_out or tuple(wy.shape) != (n_out, n_in) or tuple(wx.shape) != (n_out, n_in):
        raise P3Error("posembed_resample_bwd: fp32 gradient [1 + n_out^2, D] and tap tables [n_out, n_in] expected")
    dtable = torch.empty((1 + n_in * n_in, D), dtype=torch.float32, device=dout.device)
    check(lib().p3_posembed_resample_bwd(ptr(dout.contiguous()), ptr(wy), ptr(wx), ptr(dtable), n_in, n_out, D, stream()), "p3_posembed_resample_bwd")
    return dtable


def layerscale_fold(gamma, W, b=None):
    """-> (gamma[:, None] * W, gamma * b) fp32"""
    _dev(W)
    N, K = W.shape
    if W.dtype != torch.float32 or gamma.dtype != torch.float32 or gamma.numel() != N or (b is not None and b.numel() != N):
        raise P3Error("layerscale_fold: fp32 W [N, K], gamma [N] (and b [N]) expected")
    Wf = torch.empty((N, K), dtype=torch.float32, device=W.device)
    bf = torch.empty(N, dtype=torch.float32, device=W.device) if b is not None else None
    check(lib().p3_layerscale_fold(ptr(gamma.contiguous()), ptr(W.contiguous()), ptr(b), ptr(Wf), ptr(bf), N, K, stream()), "p3_layerscale_fold")
    return Wf, bf


def layerscale_fold_bwd(gamma, W, b, dWf, dbf):
    """-> (dW, db, dgamma) from the gradients of the folded weight / bias"""
    _dev(W)
    N, K = W.shape
    if dWf.dtype != torch.float32 or tuple(dWf.shape) != (N, K) or (b is not None and (dbf is None or dbf.dtype != torch.float32 or dbf.numel() != N)):
        raise P3Error("layerscale_fold_bwd: fp32 dW' [N, K] (and db' [N]) expected")
    dW = torch.empty((N, K), dtype=torch.float32, device=W.device)
    db = torch.empty(N, dtype=torch.float32, device=W.device) if b is not None else None
    dgamma = torch.empty(N, dtype=torch.float32, device=W.device)
    check(lib().p3_layerscale_fold_bwd(ptr(gamma.contiguous()), ptr(W.contiguous()), ptr(b), ptr(dWf.contiguous()),
                                       ptr(dbf.contiguous() if dbf is not None else None), ptr(dW), ptr(db), ptr(dgamma), N, K, stream()),
          "p3_layerscale_fold_bwd")
    return dW, db, dgamma


def tokens_assemble(src, cls, pos, B, np_, D, scale=None, shift=None, src_ld=None):
    x = torch.empty((B, np_ + 1, D), dtype=torch.float32, device=src.device)
    check(lib().p3_tokens_assemble(ptr(src), src.stride(-2) if src_ld is None else src_ld, dt(src), ptr(scale),
                                   ptr(shift), ptr(cls), ptr(pos), ptr(x), B, np_, D, stream()),
          "p3_tokens_assemble")
    return x


def pool_pos(y, pos, Dout, out_dtype, want_nopos=False):
    B, L, Din = y.shape
    out = torch.empty((B, L - 1, Dout), dtype=out_dtype, device=y.device)
    nop = torch.empty_like(out) if want_nopos else None
    check(lib().p3_pool_pos(ptr(y), dt(y), ptr(pos), ptr(out), ptr(nop), dt(out), B, L - 1, Din, Dout, stream()), "p3_pool_pos")
    return (out, nop) if want_nopos else out


def embed_tokens(tokens, emb, pos, pad_idx, dtype):
    B, L = tokens.shape
    D = emb.shape[1]
    x = torch.empty((B, L, D), dtype=dtype, device=tokens.device)
    kb = torch.empty((B, L), dtype=torch.float32, device=tokens.device)
    check(lib().p3_embed_tokens(ptr(tokens), ptr(emb), ptr(pos), ptr(x), ptr(kb), B, L, D, pad_idx, dt(x), stream()), "p3_embed_tokens")
    return x, kb


def pair_mean(feats, N):
    B, L, D = feats.shape
    out = torch.empty((B, N, D), dtype=feats.dtype, device=feats.device)
    check(lib().p3_pair_mean(ptr(feats), ptr(out), B, L, N, D, dt(feats), stream()), "p3_pair_mean")
    return out


def pair_stats(U, V, B, N, sums):
    check(lib().p3_pair_stats(ptr(U), ptr(V), B, N, U.shape[-1], dt(U), ptr(sums), stream()), "p3_pair_stats")


def bn_finalize(sums, count, gamma, beta, rmean, rvar, eps, momentum, training, save=False):
    C = gamma.shape[0]
    scale = torch.empty(C, dtype=torch.float32, device=gamma.device)
    shift = torch.empty_like(scale)
    sm = torch.empty_like(scale) if save else None
    sr = torch.empty_like(scale) if save else None
    check(lib().p3_bn_finalize(ptr(sums), C, count, ptr(gamma), ptr(beta), ptr(rmean), ptr(rvar), eps,
                               momentum, int(training), ptr(scale), ptr(shift), ptr(sm), ptr(sr), stream()),
          "p3_bn_finalize")
    return (scale, shift, sm, sr) if save else (scale, shift)


def score_out(H3, scale, shift, w4, b4, out, B, N, transpose_acc):
    check(lib().p3_score_out(ptr(H3), dt(H3), ptr(scale), ptr(shift), ptr(w4), ptr(b4), ptr(out), B, N, H3.shape[-1], int(transpose_acc), stream()), "p3_score_out")
    return out


def sinkhorn(scores, alpha, iters, want_perm=True, want_z=False, want_hist=False):
    B, m, n = scores.shape
    dev = scores.device
    perm = torch.empty((B, m, n), dtype=torch.float32, device=dev) if want_perm else None
    z = torch.empty((B, m + 1, n + 1), dtype=torch.float32, device=dev) if want_z else None
    hist = torch.empty((B, iters, m + n + 2), dtype=torch.float32, device=dev) if want_hist else None
    check(lib().p3_sinkhorn(ptr(scores), ptr(alpha), B, m, n, iters, ptr(perm), ptr(z), ptr(hist), stream()), "p3_sinkhorn")
    return perm, z, hist


def argmax(x):
    rows, cols = x.shape
    out = torch.empty(rows, dtype=torch.int64, device=x.device)
    check(lib().p3_argmax(ptr(x), ptr(out), rows, cols, x.stride(0), stream()), "p3_argmax")
    return out


class DecodeLayerDesc(Structure):
    _fields_ = [("B", c_int), ("t", c_int), ("steps", c_int), ("Lmem", c_int), ("D", c_int), ("H", c_int), ("FF", c_int),
                ("x_in", c_void_p), ("x_in_stride", c_int64), ("x_out", c_void_p), ("x_out_stride", c_int64),
                ("kv_self", c_void_p), ("kv_mem", c_void_p), ("key_bias", c_void_p), ("key_bias_stride", c_int64),
                ("w_in", c_void_p), ("b_in", c_void_p), ("w_so", c_void_p), ("b_so", c_void_p), ("w_q", c_void_p), ("b_q", c_void_p),
                ("w_co", c_void_p), ("b_co", c_void_p), ("w1", c_void_p), ("b1", c_void_p), ("w2", c_void_p), ("b2", c_void_p),
                ("g1", c_void_p), ("be1", c_void_p), ("g2", c_void_p), ("be2", c_void_p), ("g3", c_void_p), ("be3", c_void_p),
                ("eps", c_float), ("scale", c_float), ("cluster", c_int), ("exch", c_void_p), ("sync", c_void_p), ("err", c_void_p), ("fp32", c_int)]


_cu_count = {}


def coresident_workgroups(device, per_cu):
    """workgroups of a launch that can be resident at once: per_cu x the device's CU count (queried, not assumed)."""
    key = str(device)
    if key not in _cu_count:
        _cu_count[key] = torch.cuda.get_device_properties(device).multi_processor_count
    return per_cu * _cu_count[key]


def decode_layer_scratch(B, device):
    """(exch fp32 [B, 3, 4, 256], sync int32 [B, 2] zeroed ONCE, err int32 [1]) for the 4-workgroup cluster form of p3_decode_layer."""
    exch = torch.empty(B * 3 * 4 * 256 + 64, dtype=torch.float32, device=device)      # + 64: phase timestamps of the -DDL_TIMING build
    return exch, torch.zeros((B, 2), dtype=torch.int32, device=device), torch.zeros(1, dtype=torch.int32, device=device)


def decode_layer(x_in, x_out, kv_self, kv_mem, key_bias, t, heads, w, eps, scratch=None):
    """One decoder layer on the new position t of every sample (p3_decode_layer).  x_in / x_out: [B, D] rows (any row stride), bf16 or
    fp32 - activations, caches and weight matrices share that one dtype; kv_self [B, steps, 3D] (row t written), kv_mem [B, Lmem, 2D],
    key_bias [B, >= t+1] fp32 or None; `w`: dict of the layer's tensors - weights w_in, w_so, w_q, w_co, w1, w2 (row-major [out, in]) and
    fp32 b_in, b_so, b_q, b_co, b1, b2, g1, be1, g2, be2, g3, be3."""
    _dev(x_in)
    B, D = x_in.shape
    edt = x_in.dtype
    if edt not in (torch.bfloat16, torch.float32):
        raise P3Error("decode_layer: bf16 or fp32 activations")
    for name in ("w_in", "w_so", "w_q", "w_co", "w1", "w2"):
        if w[name].dtype != edt or not w[name].is_contiguous():
            raise P3Error(f"decode_layer: {name} must be a contiguous matrix of the activations' dtype ({edt})")
    if x_out.dtype != edt or kv_self.dtype != edt or kv_mem.dtype != edt:
        raise P3Error("decode_layer: activations and caches must share one dtype")
    if not (kv_self.is_contiguous() and kv_mem.is_contiguous()) or x_in.stride(1) != 1 or x_out.stride(1) != 1:
        raise P3Error("decode_layer: caches must be contiguous, activation rows dense")
    d = DecodeLayerDesc()
    d.B, d.t, d.steps, d.Lmem, d.D, d.H, d.FF = B, int(t), kv_self.shape[1], kv_mem.shape[1], D, heads, w["w1"].shape[0]
    d.x_in, d.x_in_stride, d.x_out, d.x_out_stride = x_in.data_ptr(), x_in.stride(0), x_out.data_ptr(), x_out.stride(0)
    d.kv_self, d.kv_mem = kv_self.data_ptr(), kv_mem.data_ptr()
    if key_bias is not None:
        d.key_bias, d.key_bias_stride = key_bias.data_ptr(), key_bias.stride(0)
    for name in ("w_in", "b_in", "w_so", "b_so", "w_q", "b_q", "w_co", "b_co", "w1", "b1", "w2", "b2", "g1", "be1", "g2", "be2", "g3", "be3"):
        setattr(d, name, w[name].data_ptr())
    d.eps, d.scale, d.fp32 = float(eps), 1.0 / math.sqrt(D // heads), int(edt == torch.float32)
    # 4 workgroups per sample while the whole launch is co-resident: 2 workgroups fit a CU (60 KB LDS, 512 threads), the CU count comes
    # from the device (256 on a full MI355X, fewer on a partition); incl. the padding to groups of 8 samples
    if scratch is not None and ((B + 7) // 8) * 8 * 4 <= coresident_workgroups(x_in.device, 2):
        d.cluster, d.exch, d.sync, d.err = 4, scratch[0].data_ptr(), scratch[1].data_ptr(), scratch[2].data_ptr()
    else:
        d.cluster = 1
    check(lib().p3_decode_layer(byref(d), stream()), "p3_decode_layer")
    return x_out


def assignment(scores, maximize=True, want_perm=True):
    """scipy.optimize.linear_sum_assignment per tile on the device -> (col4row int32 [B,N], perm fp32 [B,N,N] | None, status int32 [B])."""
    B, N, N2 = scores.shape
    if N != N2:
        raise P3Error(f"p3_assignment: square score matrices only, got {tuple(scores.shape)}")
    sc = scores.contiguous().float()
    col = torch.empty((B, N), dtype=torch.int32, device=sc.device)
    perm = torch.empty((B, N, N), dtype=torch.float32, device=sc.device) if want_perm else None
    status = torch.empty(B, dtype=torch.int32, device=sc.device)
    check(lib().p3_assignment(ptr(sc), B, N, 1 if maximize else 0, ptr(col), ptr(perm), ptr(status), stream()), "p3_assignment")
    return col, perm, status


def image_prepare(src_u8, group=None, sub=(0.0, 0.0, 0.0), mul=(1.0 / 255.0,) * 3, out=None):
    """u8 [B,H,W,C] -> f32 [B,C,H,W] = ToTensorV2(Normalize(D4_group(img)));  group int32 [B] (0..7) or None."""
    _dev(src_u8)
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 4:
        raise P3Error(f"image_prepare: expected uint8 [B,H,W,C], got {src_u8.dtype} {tuple(src_u8.shape)}")
    B, H, W, C = src_u8.shape
    src = src_u8.contiguous()
    if out is None:
        out = torch.empty((B, C, H, W), dtype=torch.float32, device=src.device)
    subc = (c_float * 4)(*([float(v) for v in sub] + [0.0] * 4)[:4])
    mulc = (c_float * 4)(*([float(v) for v in mul] + [1.0] * 4)[:4])
    check(lib().p3_image_prepare(ptr(src), ptr(group), ptr(out), B, H, W, C, subc, mulc, stream()), "p3_image_prepare")
    return out


def ffl_targets_prepare(gt_u8=None, angle_u8=None, distances=None, sizes=None, group=None):
    """FFL ground-truth masks of a batch -> dict of fp32 NCHW tensors (gt_polygons_image, gt_crossfield_angle, distances, sizes)."""
    ref = next(t for t in (gt_u8, angle_u8, distances, sizes) if t is not None)
    _dev(ref)
    B, H, W = ref.shape[0], ref.shape[1], ref.shape[2]
    dev = ref.device
    if gt_u8 is not None and (gt_u8.dtype != torch.uint8 or tuple(gt_u8.shape) != (B, H, W, 3)):
        raise P3Error(f"ffl_targets_prepare: gt_polygons_image must be uint8 [B,H,W,3], got {gt_u8.dtype} {tuple(gt_u8.shape)}")
    if angle_u8 is not None and (angle_u8.dtype != torch.uint8 or tuple(angle_u8.shape) != (B, H, W)):
        raise P3Error(f"ffl_targets_prepare: gt_crossfield_angle must be uint8 [B,H,W], got {angle_u8.dtype} {tuple(angle_u8.shape)}")
    c = lambda t: t.contiguous() if t is not None else None
    gt_u8, angle_u8 = c(gt_u8), c(angle_u8)
    distances = c(distances.float()) if distances is not None else None
    sizes = c(sizes.float()) if sizes is not None else None
    mk = lambda t, ch: torch.empty((B, ch, H, W), dtype=torch.float32, device=dev) if t is not None else None
    o_gt, o_an, o_di, o_si = mk(gt_u8, 3), mk(angle_u8, 1), mk(distances, 1), mk(sizes, 1)
    check(lib().p3_ffl_targets_prepare(ptr(gt_u8), ptr(angle_u8), ptr(distances), ptr(sizes), ptr(group), B, H, W, ptr(o_gt),
                                       ptr(o_an), ptr(o_di), ptr(o_si), stream()), "p3_ffl_targets_prepare")
    out = {"gt_polygons_image": o_gt, "gt_crossfield_angle": o_an, "distances": o_di, "sizes": o_si}
    return {k: v for k, v in out.items() if v is not None}


def points_d4_(values, offsets, group, cx, cy):
    """in-place D4 of a jagged point list (values [T,3] f32, offsets int64 [B+1]) around (cx, cy); group int32 [B]."""
    _dev(values)
    if values.dtype != torch.float32 or not values.is_contiguous() or values.shape[-1] != 3:
        raise P3Error("points_d4_: values must be contiguous float32 [T, 3]")
    check(lib().p3_points_d4(ptr(values), ptr(offsets), ptr(group), offsets.numel() - 1, values.shape[0], cx, cy, stream()), "p3_points_d4")
    return values


def ffl_loss(seg, crossfield, gt_polygons_image, gt_crossfield_angle, coef, bce_coef, dice_coef, need_grad=True, seg_weights=None):
    """fused FFL loss: -> (losses fp32 [6] = five raw losses + total, dseg | None, dcrossfield | None)."""
    _dev(seg)
    B, _, H, W = seg.shape
    ts = [t.contiguous().float() for t in (seg, crossfield, gt_polygons_image, gt_crossfield_angle)]
    if ts[0].shape != (B, 1, H, W) or ts[1].shape != (B, 4, H, W) or ts[2].shape != (B, 3, H, W) or ts[3].numel() != B * H * W:
        raise P3Error(f"ffl_loss: shapes seg {tuple(seg.shape)} crossfield {tuple(crossfield.shape)} gt {tuple(gt_polygons_image.shape)} "
                      f"angle {tuple(gt_crossfield_angle.shape)}")
    ws = workspace(int(lib().p3_ffl_loss_workspace_bytes(B, H, W)), seg.device, "ffl_loss")
    losses = torch.empty(6, dtype=torch.float32, device=seg.device)
    dseg = torch.empty_like(ts[0]) if need_grad else None
    dcf = torch.empty_like(ts[1]) if need_grad else None
    cc = (c_float * 5)(*[float(v) for v in coef])
    sw = seg_weights.contiguous().float() if seg_weights is not None else None
    if sw is not None and sw.numel() != B * H * W:
        raise P3Error(f"ffl_loss: seg_weights must hold one weight per pixel of the seg channel, got {tuple(seg_weights.shape)}")
    check(lib().p3_ffl_loss(ptr(ts[0]), ptr(ts[1]), ptr(ts[2]), ptr(ts[3]), ptr(sw), B, H, W, cc,
                            bce_coef, dice_coef, ptr(losses), ptr(dseg), ptr(dcf), ptr(ws), stream()), "p3_ffl_loss")
    return losses, dseg, dcf


def afm(lines, shape_info, height, width):
    """attraction field map of line segments (HiSup afm op): -> (afmap f32 [B,2,H,W], aflabel i32 [B,1,H,W])."""
    _dev(shape_info)
    si = shape_info.to(torch.int32).contiguous()
    ln = lines.float().contiguous() if lines is not None and lines.numel() else None
    B = si.shape[0]
    afmap = torch.empty((B, 2, height, width), dtype=torch.float32, device=si.device)
    lab = torch.empty((B, 1, height, width), dtype=torch.int32, device=si.device)
    check(lib().p3_afm(ptr(ln), ptr(si), B, height, width, ptr(afmap), ptr(lab), stream()), "p3_afm")
    return afmap, lab


# ------------------------------------------------------------------------------------------ HiSup inference after the heads
HISUP_MAX_HW = 1 << 22
HISUP_TOPK = 300


def _logit_map(t, n, shape, what):
    """a logit map with n channels -> (tensor kept alive, B, H, W, (batch, channel, pixel) strides in elements).  Either NCHW fp32
    [B, n, H, W] or token-major fp32 rows [B*H*W, ld >= n] (a predictor's output, hisup.HiSupHeads._predictor) with shape = (B, H, W)."""
    _dev(t)
    if t.dtype != torch.float32:
        raise P3Error(f"{what}: fp32 logits expected, got {t.dtype}")
    if t.dim() == 4:
        B, C, H, W = t.shape
        if C != n:
            raise P3Error(f"{what}: {n} channels expected, got {C}")
        t = t.contiguous()
        st = (C * H * W, H * W, 1)
    elif t.dim() == 2 and shape is not None:
        B, H, W = shape
        if t.shape[0] != B * H * W or t.shape[1] < n or t.stride(1) != 1:
            raise P3Error(f"{what}: token-major rows [{B * H * W}, >= {n}] expected, got {tuple(t.shape)}")
        st = (H * W * t.stride(0), 1, t.stride(0))
    else:
        raise P3Error(f"{what}: NCHW [B, {n}, H, W] or token-major rows with shape=(B, H, W) expected, got {tuple(t.shape)}")
    if B < 1 or H < 1 or W < 1 or H * W > HISUP_MAX_HW:
        raise P3Error(f"{what}: H * W = {H * W} is beyond the {HISUP_MAX_HW} pixels per map the kernel supports (or an empty map)")
    return t, B, H, W, st


def hisup_junctions(jloc, joff, scale_x=1.0, scale_y=1.0, shape=None):
    """p3_hisup_junctions: -> (juncs f32 [B,600,2] (x, y), scores f32 [B,600], index i32 [B,600], counts i32 [B,2] = (n_class2, n_class1)).
    Class 2 first, then class 1; inside a class descending score, equal scores by ascending flat index.  No host synchronisation."""
    jl, B, H, W, sl = _logit_map(jloc, 3, shape, "hisup_junctions(jloc)")
    jo, B2, H2, W2, so = _logit_map(joff, 2, shape, "hisup_junctions(joff)")
    if (B, H, W) != (B2, H2, W2):
        raise P3Error(f"hisup_junctions: jloc is {(B, H, W)}, joff is {(B2, H2, W2)}")
    dev = jl.device
    juncs = torch.empty((B, 2 * HISUP_TOPK, 2), dtype=torch.float32, device=dev)
    scores = torch.empty((B, 2 * HISUP_TOPK), dtype=torch.float32, device=dev)
    index = torch.empty((B, 2 * HISUP_TOPK), dtype=torch.int32, device=dev)
    counts = torch.empty((B, 2), dtype=torch.int32, device=dev)
    ws = workspace(int(lib().p3_hisup_junctions_workspace_bytes(B, H, W)), dev, "hisup_junctions")
    check(lib().p3_hisup_junctions(ptr(jl), sl[0], sl[1], sl[2], ptr(jo), so[0], so[1], so[2],
                                   B, H, W, scale_x, scale_y, ptr(juncs), ptr(scores), ptr(index), ptr(counts),
                                   ptr(ws), stream()), "p3_hisup_junctions")
    return juncs, scores, index, counts


def _outputs(stage, dev, spec, out=None):
    """the output tensors of a *_device binding -> dict.  spec: (name, shape, dtype) per output, in the order of the C arguments.  out: None, or a dict with
    the caller's own tensors for any of the names (buffers kept across batches or a graph capture, guard-band views in the tests); the rest is allocated.
    A given tensor must lie on dev, be contiguous, have exactly that dtype and exactly prod(shape) elements; it is viewed to shape, so [n, 1] stands for [n]."""
    given, res = dict(out or {}), {}
    for name, shape, dtype in spec:
        t = given.pop(name, None)
        if t is None:
            res[name] = torch.empty(shape, dtype=dtype, device=dev)
            continue
        if t.device != torch.device(dev) or t.dtype != dtype or t.numel() != math.prod(shape) or not t.is_contiguous():
            raise P3Error(f"{stage}: out['{name}'] must be a contiguous {dtype} tensor of {math.prod(shape)} elements on {dev}, got {t.dtype} "
                          f"{tuple(t.shape)} with strides {t.stride()} on {t.device}")
        res[name] = t.view(shape)
    if given:
        raise P3Error(f"{stage}: out has no {sorted(given)}; its outputs are {[name for name, _, _ in spec]}")
    return res


def _read_back(out, who, errors, narrow):
    """the one device-to-host copy of a checking form: counts and status together.  errors: (status bits, message or function of the counts -> message) in the
    order they are looked at, the first set one raises; narrow: output name -> the index of the count it is cut to.  counts becomes the tuple of ints."""
    *counts, status = torch.cat([out["counts"], out["status"]]).tolist()
    for bits, msg in errors:
        if status & bits:
            raise P3Error(f"{who}: {msg(*counts) if callable(msg) else msg}")
    for k, i in narrow.items():
        out[k] = out[k][:counts[i]]
    out["counts"] = tuple(counts)
    return out


def hisup_regions_device(remask, max_regions=1024, shape=None, out=None):
    """p3_hisup_regions without any synchronisation: -> dict(mask f32 [B,H,W], labels i32 [B,H,W], n_regions i32 [B], area i32 [B,R],
    bbox i32 [B,R,4] = (min_row, min_col, max_row + 1, max_col + 1), score f32 [B,R], status i32 [B] = 1 where n_regions > R = max_regions).
    out: the caller's own tensors for any of these (`_outputs`)."""
    rm, B, H, W, st = _logit_map(remask, 2, shape, "hisup_regions(remask)")
    R = int(max_regions)
    if R < 1:
        raise P3Error(f"hisup_regions: max_regions = {max_regions}")
    dev, f32, i32 = rm.device, torch.float32, torch.int32
    out = _outputs("hisup_regions", dev, (("mask", (B, H, W), f32), ("labels", (B, H, W), i32), ("n_regions", (B,), i32), ("area", (B, R), i32),
                                          ("bbox", (B, R, 4), i32), ("score", (B, R), f32), ("status", (B,), i32)), out)
    ws = workspace(int(lib().p3_hisup_regions_workspace_bytes(B, H, W, R)), dev, "hisup_regions")
    check(lib().p3_hisup_regions(ptr(rm), st[0], st[1], st[2], B, H, W, R, ptr(out["mask"]), ptr(out["labels"]), ptr(out["n_regions"]), ptr(out["area"]),
                                 ptr(out["bbox"]), ptr(out["score"]), ptr(out["status"]), ptr(ws), stream()), "p3_hisup_regions")
    return out


def hisup_regions(remask, max_regions=1024, shape=None):
    """the checking form of hisup_regions_device: reads the status words on the host and raises when an image has more regions than max_regions"""
    out = hisup_regions_device(remask, max_regions, shape)
    if bool(out["status"].any()):
        raise P3Error(f"hisup_regions: an image has more than max_regions = {max_regions} regions (n_regions = {out['n_regions'].tolist()})")
    return out


def hisup_val_loss(jloc, joff, mask, afm_pred, remask, t_jloc, t_joff, t_mask, t_afm):
    """p3_hisup_val_loss: -> fp32 [5] = loss_jloc, loss_joff, loss_mask, loss_afm, loss_remask (un-weighted, model_hisup.py:241-245)"""
    _dev(jloc)
    B, C, H, W = jloc.shape
    want = ((jloc, 3), (joff, 2), (mask, 2), (afm_pred, 2), (remask, 2), (t_jloc, 1), (t_joff, 2), (t_mask, 1), (t_afm, 2))
    for i, (t, n) in enumerate(want):
        _dev(t)
        if tuple(t.shape) != (B, n, H, W):
            raise P3Error(f"hisup_val_loss: argument {i} must be {(B, n, H, W)}, got {tuple(t.shape)}")
    if H * W > HISUP_MAX_HW:
        raise P3Error(f"hisup_val_loss: H * W = {H * W} is beyond the {HISUP_MAX_HW} pixels per map the kernel supports")
    f = [t.contiguous().float() for t in (jloc, joff, mask, afm_pred, remask)]
    tj = t_jloc.contiguous().to(torch.int64)
    tt = [t.contiguous().float() for t in (t_joff, t_mask, t_afm)]
    losses = torch.empty(5, dtype=torch.float32, device=jloc.device)
    ws = workspace(int(lib().p3_hisup_val_loss_workspace_bytes(B, H, W)), jloc.device, "hisup_val_loss")
    check(lib().p3_hisup_val_loss(ptr(f[0]), ptr(f[1]), ptr(f[2]), ptr(f[3]), ptr(f[4]), ptr(tj), ptr(tt[0]), ptr(tt[1]), ptr(tt[2]), B,
                                  H, W, ptr(losses), ptr(ws), stream()), "p3_hisup_val_loss")
    return losses


def hisup_train_loss(jloc, joff, mask, afm_pred, remask, t_jloc, t_joff, t_mask, t_afm, weights, need_grad=True, shape=None, grads=None):
    """p3_hisup_train_loss: the five HiSup training losses (model_hisup.py:302-306) and the gradients of their weighted total, in one call
    -> (losses fp32 [6] = loss_jloc, loss_joff, loss_mask, loss_afm, loss_remask (un-weighted), total = sum weights[k] * loss_k,
        [d total / d jloc, d joff, d mask, d afm, d remask] | None).
    Each prediction is NCHW fp32 or token-major fp32 rows [B*H*W, >= n] with shape = (B, H, W) (`_logit_map`), in any mix; its gradient has the same
    layout (for rows: an [R, n] view with the prediction's row stride).  grads: the five output tensors, given by the caller (same layouts and strides);
    only their valid channels are written.  need_grad=False computes the values alone - the same values, bit for bit.  No host synchronisation."""
    names = ("jloc", "joff", "mask", "afm", "remask")
    preds = (jloc, joff, mask, afm_pred, remask)
    bhw = [(t.shape[0], t.shape[2], t.shape[3]) if t.dim() == 4 else (tuple(int(v) for v in shape) if shape is not None else None) for t in preds]
    B, H, W = bhw[0] if bhw[0] is not None and len(bhw[0]) == 3 else (0, 0, 0)
    for k, v in zip(names, bhw):                         # shapes first, devices second: a shape error reads as one on any tensor
        if v != (B, H, W) or B < 1:
            raise P3Error(f"hisup_train_loss: the five maps must share one (B, H, W); jloc is {bhw[0]}, {k} is {v}")
    want = ((t_jloc, 1), (t_joff, 2), (t_mask, 1), (t_afm, 2))
    for i, (t, n) in enumerate(want):
        if tuple(t.shape) != (B, n, H, W):
            raise P3Error(f"hisup_train_loss: target {i} must be {(B, n, H, W)}, got {tuple(t.shape)}")
    if H * W > HISUP_MAX_HW:
        raise P3Error(f"hisup_train_loss: H * W = {H * W} is beyond the {HISUP_MAX_HW} pixels per map the kernel supports")
    if len(weights) != 5:
        raise P3Error(f"hisup_train_loss: five loss weights expected, got {len(weights)}")
    maps = [_logit_map(t, n, shape, f"hisup_train_loss({k})") for t, n, k in zip(preds, (3, 2, 2, 2, 2), names)]
    dev = maps[0][0].device
    for t, _ in want:
        _dev(t)
    tj = t_jloc.contiguous().to(torch.int64)
    tt = [t.contiguous().float() for t in (t_joff, t_mask, t_afm)]
    out = None
    if need_grad:
        out = []
        for i, (k, (t, _, _, _, st)) in enumerate(zip(names, maps)):
            n = 3 if i == 0 else 2
            if grads is None:
                g = torch.empty_like(t) if t.dim() == 4 else torch.empty((t.shape[0], st[2]), dtype=torch.float32, device=dev)[:, :n]
            else:
                g = grads[i]
                if g.dim() == 4 and not g.is_contiguous():
                    raise P3Error(f"hisup_train_loss: the gradient of {k} must be contiguous")
                gm = _logit_map(g, n, shape, f"hisup_train_loss(d {k})")
                if g.dim() != t.dim() or gm[1:] != (B, H, W, st):
                    raise P3Error(f"hisup_train_loss: the gradient of {k} needs the layout and strides of its prediction {st}, got {gm[4]}")
                g = g if g.dim() == 4 else g[:, :n]
            out.append(g)
    elif grads is not None:
        raise P3Error("hisup_train_loss: grads given with need_grad=False")
    losses = torch.empty(6, dtype=torch.float32, device=dev)
    ws = workspace(int(lib().p3_hisup_train_loss_workspace_bytes(B, H, W)), dev, "hisup_train_loss")
    cw = (c_float * 5)(*[float(v) for v in weights])
    s = [m[4] for m in maps]
    gp = out if out is not None else [None] * 5
    check(lib().p3_hisup_train_loss(ptr(maps[0][0]), s[0][0], s[0][1], s[0][2], ptr(maps[1][0]), s[1][0], s[1][1], s[1][2],
                                    ptr(maps[2][0]), s[2][0], s[2][1], s[2][2], ptr(maps[3][0]), s[3][0], s[3][1], s[3][2],
                                    ptr(maps[4][0]), s[4][0], s[4][1], s[4][2], ptr(tj), ptr(tt[0]), ptr(tt[1]), ptr(tt[2]), B, H, W, cw,
                                    ptr(losses), ptr(gp[0]), ptr(gp[1]), ptr(gp[2]), ptr(gp[3]), ptr(gp[4]), ptr(ws), stream()),
          "p3_hisup_train_loss")
    return losses, out


HISUP_MAX_EDGE = 32766     # csrc/hisup_polygon.hip: ring coordinates are packed into 16 bits each


def hisup_polygons_capacity(B, H, W, max_regions):
    """the max_vertices that can never overflow (include/p3hip.h, the ring bound of p3_hisup_polygons)"""
    return B * (2 * (H * (W + 1) + W * (H + 1)) + 9 * min(max_regions, ((H + 1) // 2) * ((W + 1) // 2)))


def hisup_polygons_device(labels, n_regions, bbox, juncs, junc_counts, max_vertices=None, force_fallback=False, out=None):
    """p3_hisup_polygons (models/hisup/polygon.py `get_poly_crowdai`, outer polygons only) without any synchronisation.
    labels i32 [B,H,W], n_regions i32 [B], bbox i32 [B,R,4] as hisup_regions_device returns them, juncs f32 [B,600,2], junc_counts i32 [B,2] as
    hisup_junctions returns them.  -> dict(pos f32 [max_vertices,2] (x, y), src i32 [max_vertices] (ring or junction index), poly_slice i64 [B,R,2],
    poly_flags i32 [B,R] (bit 0 junction polygon, bit 1 the region has holes - their rings are NOT built -, bit 2 no polygon), hole_pixels i32 [B,R],
    n_vertices i32 [B], counts i32 [2] = (vertices, longest polygon), status i32 [1] (bit 0: max_vertices was too small; the counts are the true totals
    then, pos / src are not written)).  The default max_vertices cannot overflow but is large: 12 bytes of output and 12 of workspace per vertex, about
    2 x 41 MB at B = 16, 224 x 224, where real outputs have a few thousand vertices; a caller that holds many batches passes its own max_vertices and
    checks status.  out: the caller's own tensors for any of the outputs (`_outputs`); they have to fit max_vertices, they do not define it."""
    if labels.dim() != 3 or labels.dtype != torch.int32 or min(labels.shape) < 1:
        raise P3Error(f"hisup_polygons: labels int32 [B, H, W] expected, got {labels.dtype} {tuple(labels.shape)}")
    B, H, W = labels.shape
    if bbox.dim() != 3 or bbox.shape[0] != B or bbox.shape[2] != 4 or bbox.shape[1] < 1 or bbox.dtype != torch.int32 or tuple(n_regions.shape) != (B,) \
            or n_regions.dtype != torch.int32:
        raise P3Error(f"hisup_polygons: n_regions int32 [{B}] and bbox int32 [{B}, R, 4] expected, got {tuple(n_regions.shape)}, {tuple(bbox.shape)}")
    if tuple(juncs.shape) != (B, 2 * HISUP_TOPK, 2) or juncs.dtype != torch.float32 or tuple(junc_counts.shape) != (B, 2) or junc_counts.dtype != torch.int32:
        raise P3Error(f"hisup_polygons: juncs float32 [{B}, {2 * HISUP_TOPK}, 2] and junc_counts int32 [{B}, 2] expected, got {tuple(juncs.shape)}, "
                      f"{tuple(junc_counts.shape)}")
    if H > HISUP_MAX_EDGE or W > HISUP_MAX_EDGE or H * W > HISUP_MAX_HW:
        raise P3Error(f"hisup_polygons: {H} x {W} is beyond the {HISUP_MAX_EDGE} pixels per edge / {HISUP_MAX_HW} pixels per map the kernel supports")
    R = bbox.shape[1]
    nv = hisup_polygons_capacity(B, H, W, R) if max_vertices is None else int(max_vertices)
    if nv < 1 or nv >= 1 << 31:
        raise P3Error(f"hisup_polygons: max_vertices = {nv}")
    for t in (labels, n_regions, bbox, juncs, junc_counts):
        _dev(t)
    dev, i32 = labels.device, torch.int32
    out = _outputs("hisup_polygons", dev, (("pos", (nv, 2), torch.float32), ("src", (nv,), i32), ("poly_slice", (B, R, 2), torch.int64), ("poly_flags", (B, R), i32),
                                           ("hole_pixels", (B, R), i32), ("n_vertices", (B,), i32), ("counts", (2,), i32), ("status", (1,), i32)), out)
    lab, nr, bb, jc, cn = labels.contiguous(), n_regions.contiguous(), bbox.contiguous(), juncs.contiguous(), junc_counts.contiguous()
    ws = workspace(int(lib().p3_hisup_polygons_workspace_bytes(B, H, W, R, nv)), dev, "hisup_polygons")
    check(lib().p3_hisup_polygons(ptr(lab), ptr(nr), ptr(bb), ptr(jc), ptr(cn), B, H, W, R, nv, int(bool(force_fallback)),
                                  ptr(out["pos"]), ptr(out["src"]), ptr(out["poly_slice"]), ptr(out["poly_flags"]), ptr(out["hole_pixels"]),
                                  ptr(out["n_vertices"]), ptr(out["counts"]), ptr(out["status"]), ptr(ws), stream()), "p3_hisup_polygons")
    return out


def hisup_polygons(labels, n_regions, bbox, juncs, junc_counts, max_vertices=None, force_fallback=False):
    """the checking form of hisup_polygons_device: reads counts and status once (the only read-back), raises when max_vertices was too small and narrows
    pos / src to the vertices found; counts = (vertices, longest polygon) as Python ints."""
    return hisup_polygons_checked(hisup_polygons_device(labels, n_regions, bbox, juncs, junc_counts, max_vertices, force_fallback))


def hisup_polygons_checked(out, who="hisup_polygons"):
    """the one read-back of counts and status of a hisup_polygons_device result: raises on any status bit, narrows pos / src, counts as Python ints"""
    return _read_back(out, who, ((1, lambda V, _: f"{V} vertices do not fit max_vertices = {out['pos'].shape[0]}"),
                                 (4, "P3_HISUP_POLY_STOP is set: the run was cut short for a measurement and has no result"),
                                 (2, "a region's ring is longer than the bound the workspace is sized for (include/p3hip.h)")), dict(pos=0, src=0))


def hisup_polygon_rings_capacity(B, H, W, max_regions):
    """(max_vertices, max_rings, max_ring_vertices) that can never overflow (include/p3hip.h, the ring bounds of p3_hisup_polygons_rings)"""
    q = (H * W) // 50
    return hisup_polygons_capacity(B, H, W, max_regions), max(1, B * q), max(1, B * (2 * (H * (W - 1) + W * (H - 1)) + 17 * q))


def hisup_polygon_rings_device(labels, n_regions, bbox, juncs, junc_counts, max_vertices=None, max_rings=None, max_ring_vertices=None, force_fallback=False,
                               out=None):
    """p3_hisup_polygons_rings (models/hisup/polygon.py `get_poly_crowdai` with its hole branch `inn_c_to_poly_coco`) without any
    synchronisation.  Inputs and the first seven outputs as hisup_polygons_device, with the same bits.  Further outputs, rings in (image, label, hole) order:
    ring_pos f32 [max_ring_vertices,2], ring_src i32 [max_ring_vertices], ring_slice i64 [max_rings,2], ring_region i32 [max_rings] (b R + l - 1),
    ring_flags i32 [max_rings] (bit 0 junction ring, bit 2 nothing kept), ring_area2 i32 [max_rings] (twice the area of the hole border), region_rings
    i32 [B,R,2], n_holes i32 [B,R], ring_counts i32 [3] = (rings, ring vertices, longest ring); status i32 [1]: bits 0 to 2 as hisup_polygons_device, bit 3
    max_rings was too small, bit 4 max_ring_vertices was too small (the counts are the true totals then).  The default capacities cannot overflow.
    out: the caller's own tensors for any of the outputs (`_outputs`)."""
    if labels.dim() != 3 or labels.dtype != torch.int32 or min(labels.shape) < 1:
        raise P3Error(f"hisup_polygon_rings: labels int32 [B, H, W] expected, got {labels.dtype} {tuple(labels.shape)}")
    B, H, W = labels.shape
    if bbox.dim() != 3 or bbox.shape[0] != B or bbox.shape[2] != 4 or bbox.shape[1] < 1 or bbox.dtype != torch.int32 or tuple(n_regions.shape) != (B,) \
            or n_regions.dtype != torch.int32:
        raise P3Error(f"hisup_polygon_rings: n_regions int32 [{B}] and bbox int32 [{B}, R, 4] expected, got {tuple(n_regions.shape)}, {tuple(bbox.shape)}")
    if tuple(juncs.shape) != (B, 2 * HISUP_TOPK, 2) or juncs.dtype != torch.float32 or tuple(junc_counts.shape) != (B, 2) or junc_counts.dtype != torch.int32:
        raise P3Error(f"hisup_polygon_rings: juncs float32 [{B}, {2 * HISUP_TOPK}, 2] and junc_counts int32 [{B}, 2] expected, got {tuple(juncs.shape)}, "
                      f"{tuple(junc_counts.shape)}")
    if H > HISUP_MAX_EDGE or W > HISUP_MAX_EDGE or H * W > HISUP_MAX_HW:
        raise P3Error(f"hisup_polygon_rings: {H} x {W} is beyond the {HISUP_MAX_EDGE} pixels per edge / {HISUP_MAX_HW} pixels per map the kernel supports")
    R = bbox.shape[1]
    cap = hisup_polygon_rings_capacity(B, H, W, R)
    nv, nr_, nrv = (c if v is None else int(v) for c, v in zip(cap, (max_vertices, max_rings, max_ring_vertices)))
    for k, v in (("max_vertices", nv), ("max_rings", nr_), ("max_ring_vertices", nrv)):
        if v < 1 or v >= 1 << 31:
            raise P3Error(f"hisup_polygon_rings: {k} = {v}")
    for t in (labels, n_regions, bbox, juncs, junc_counts):
        _dev(t)
    dev, i32, f32, i64 = labels.device, torch.int32, torch.float32, torch.int64
    out = _outputs("hisup_polygon_rings", dev, (("pos", (nv, 2), f32), ("src", (nv,), i32), ("poly_slice", (B, R, 2), i64), ("poly_flags", (B, R), i32),
                                                ("hole_pixels", (B, R), i32), ("n_vertices", (B,), i32), ("counts", (2,), i32), ("ring_pos", (nrv, 2), f32),
                                                ("ring_src", (nrv,), i32), ("ring_slice", (nr_, 2), i64), ("ring_region", (nr_,), i32),
                                                ("ring_flags", (nr_,), i32), ("ring_area2", (nr_,), i32), ("region_rings", (B, R, 2), i32),
                                                ("n_holes", (B, R), i32), ("ring_counts", (3,), i32), ("status", (1,), i32)), out)
    lab, nr, bb, jc, cn = labels.contiguous(), n_regions.contiguous(), bbox.contiguous(), juncs.contiguous(), junc_counts.contiguous()
    ws = workspace(int(lib().p3_hisup_polygons_rings_workspace_bytes(B, H, W, R, nv, nr_, nrv)), dev, "hisup_polygon_rings")
    check(lib().p3_hisup_polygons_rings(ptr(lab), ptr(nr), ptr(bb), ptr(jc), ptr(cn), B, H, W, R, nv, nr_, nrv, int(bool(force_fallback)),
                                        *(ptr(out[k]) for k in ("pos", "src", "poly_slice", "poly_flags", "hole_pixels", "n_vertices", "counts", "ring_pos",
                                                                "ring_src", "ring_slice", "ring_region", "ring_flags", "ring_area2", "region_rings", "n_holes",
                                                                "ring_counts", "status")), ptr(ws), stream()), "p3_hisup_polygons_rings")
    return out


def hisup_polygon_rings(labels, n_regions, bbox, juncs, junc_counts, max_vertices=None, max_rings=None, max_ring_vertices=None, force_fallback=False):
    """the checking form of hisup_polygon_rings_device: reads the counts and status once (the only read-back), raises on any status bit and narrows pos / src
    to the vertices, ring_pos / ring_src to the ring vertices and the per-ring outputs to the rings found; counts = (vertices, longest polygon) and
    ring_counts = (rings, ring vertices, longest ring) as Python ints."""
    return hisup_polygon_rings_checked(hisup_polygon_rings_device(labels, n_regions, bbox, juncs, junc_counts, max_vertices, max_rings, max_ring_vertices,
                                                                  force_fallback))


def hisup_polygon_rings_checked(out, who="hisup_polygon_rings"):
    """the one read-back of counts, ring_counts and status of a hisup_polygon_rings_device result"""
    res = dict(out)
    res["counts"] = torch.cat([out["counts"], out["ring_counts"]])
    res = _read_back(res, who, ((1, lambda V, *_: f"{V} vertices do not fit max_vertices = {out['pos'].shape[0]}"),
                                (8, lambda V, L, Q, *_: f"{Q} rings do not fit max_rings = {out['ring_region'].shape[0]}"),
                                (16, lambda V, L, Q, RV, _: f"{RV} ring vertices do not fit max_ring_vertices = {out['ring_pos'].shape[0]}"),
                                (4, "P3_HISUP_POLY_STOP is set: the run was cut short for a measurement and has no result"),
                                (2, "a ring is longer than the bound the workspace is sized for (include/p3hip.h)")),
                     dict(pos=0, src=0, ring_pos=3, ring_src=3, ring_slice=2, ring_region=2, ring_flags=2, ring_area2=2))
    res["counts"], res["ring_counts"] = res["counts"][:2], res["counts"][2:]
    return res


# ------------------------------------------------------------------------------------------ FFL active-contour polygon optimiser
ACM_LDS_CAP = 4096          # csrc/acm.hip: vertices of one polygon that fit the one-launch LDS path


def _ffl_maps(who, indicator, c0c2):
    """indicator [B,H,W] or seg [B,C,H,W] (channel 0 is taken) and c0c2 [B,4,H,W] -> contiguous fp32 copies and (B, H, W)"""
    if indicator.dim() == 4:
        indicator = indicator[:, 0]
    if indicator.dim() != 3 or c0c2.dim() != 4 or c0c2.shape[1] != 4 or (c0c2.shape[0],) + tuple(c0c2.shape[2:]) != tuple(indicator.shape):
        raise P3Error(f"{who}: indicator [B, H, W] and c0c2 [B, 4, H, W] expected, got {tuple(indicator.shape)}, {tuple(c0c2.shape)}")
    return indicator.contiguous().float(), c0c2.contiguous().float(), tuple(indicator.shape)


def acm_optimize(pos, poly_slice, batch, is_endpoint, indicator, c0c2, data_coef, length_coef, crossfield_coef, data_level=0.5, poly_lr=0.01,
                 warmup_iters=100, warmup_factor=0.1, first_iter=0, steps=500, losses=False, force_fallback=False, max_len=None):
    """p3_acm_optimize (predict/ffl/polygonize_acm.py:77-220): `steps` SGD iterations first_iter .. first_iter + steps - 1 on pos fp32 [N,2] (row, col), IN PLACE.
    poly_slice [P,2]; batch [N] is the tensorpoly's per-node image index (a polygon's image is that of its first vertex); is_endpoint [N].
    indicator [B,H,W] or seg [B,C,H,W] (channel 0 is taken), c0c2 [B,4,H,W]; bf16 / strided maps are copied to contiguous fp32.
    max_len: longest polygon if the caller knows it (else read from poly_slice: one host synchronisation).  max_len=0 ("unknown", what the raw C entry
    takes) is for tests only: it sizes the per-step fallback grid for a polygon of all N vertices, thousands of workgroups that return at once.  -> pos, or (pos, losses fp32 [P,3] = (align,
    level, length) per polygon at the last step, before its update) with losses=True."""
    for t in (pos, poly_slice, batch, is_endpoint, indicator, c0c2):
        _dev(t)
    if pos.dtype != torch.float32 or pos.dim() != 2 or pos.shape[1] != 2 or not pos.is_contiguous():
        raise P3Error(f"acm_optimize: pos must be contiguous float32 [N, 2] (it is updated in place), got {pos.dtype} {tuple(pos.shape)}")
    N, P = pos.shape[0], poly_slice.shape[0]
    if poly_slice.dim() != 2 or poly_slice.shape[1] != 2 or batch.shape[0] != N or is_endpoint.shape[0] != N:
        raise P3Error(f"acm_optimize: poly_slice [P, 2], batch [N], is_endpoint [N] expected, got {tuple(poly_slice.shape)}, {tuple(batch.shape)}, {tuple(is_endpoint.shape)}")
    ind, cf, (B, H, W) = _ffl_maps("acm_optimize", indicator, c0c2)
    out = torch.zeros((P, 3), dtype=torch.float32, device=pos.device) if losses else None          # zeros: a polygon longer than a wrong max_len is skipped, row and all
    if P == 0 or N == 0 or steps == 0:
        return (pos, out) if losses else pos
    sl = poly_slice.to(torch.int32).contiguous()
    pb = batch.index_select(0, poly_slice[:, 0].clamp(0, N - 1).long()).to(torch.int32).contiguous()          # image of a polygon = image of its first vertex
    ep = is_endpoint.to(torch.uint8).contiguous()
    if max_len is None:
        max_len = int((poly_slice[:, 1] - poly_slice[:, 0]).max())
    ws = None
    if force_fallback or max_len > ACM_LDS_CAP or max_len <= 0:
        ws = workspace(int(lib().p3_acm_workspace_bytes(N)), pos.device, "acm")
    check(lib().p3_acm_optimize(ptr(pos), N, ptr(sl), ptr(pb), P, ptr(ep), ptr(ind), ptr(cf), B, H, W, data_coef,
                                length_coef, crossfield_coef, data_level, poly_lr, int(warmup_iters),
                                warmup_factor, int(first_iter), int(steps), int(max_len), int(bool(force_fallback)),
                                ptr(out), ptr(ws), stream()), "p3_acm_optimize")
    return (pos, out) if losses else pos


# ------------------------------------------------------------------------------------------ FFL initial contours (marching squares)
def init_contours_device(indicator, level=0.5, max_vertices=None, max_contours=None, out=None):
    """p3_init_contours (predict/ffl/polygonize_utils.py:15-44: find_contours(indicator, level, fully_connected='low', positive_orientation='high') per image)
    without any synchronisation.  indicator fp32 [B,H,W] with any strides (seg[:, 0] is not copied), or [B,C,H,W] (channel 0 is taken).
    -> dict(pos f32 [max_vertices,2] (row, col), poly_slice i64 [max_contours,2], poly_batch i32 [max_contours], batch i64 [max_vertices], is_endpoint u8
    [max_vertices], counts i32 [3] = (N, P, longest contour), n_contours i32 [B], n_vertices i32 [B], status i32 [1] = 1 when N > max_vertices or P > max_contours;
    counts are the true totals then, and nothing is written past the capacities).  The default capacities B (H (W-1) + (H-1) W) and half of that cannot overflow.
    out: the caller's own tensors for any of the outputs (`_outputs`); they have to fit the capacities, they do not define them."""
    _dev(indicator)
    if indicator.dim() == 4:
        indicator = indicator[:, 0]
    if indicator.dim() != 3 or indicator.shape[0] < 1 or indicator.shape[1] < 1 or indicator.shape[2] < 1:
        raise P3Error(f"init_contours: indicator [B, H, W] or seg [B, C, H, W] expected, got {tuple(indicator.shape)}")
    if indicator.dtype != torch.float32:
        indicator = indicator.float()
    B, H, W = indicator.shape
    bound = B * (H * (W - 1) + (H - 1) * W)
    nv = max(bound, 1) if max_vertices is None else int(max_vertices)
    nc = max(bound // 2, 1) if max_contours is None else int(max_contours)
    if nv < 1 or nc < 1:
        raise P3Error(f"init_contours: max_vertices = {max_vertices}, max_contours = {max_contours}")
    dev, i32, i64 = indicator.device, torch.int32, torch.int64
    out = _outputs("init_contours", dev, (("pos", (nv, 2), torch.float32), ("poly_slice", (nc, 2), i64), ("poly_batch", (nc,), i32), ("batch", (nv,), i64),
                                          ("is_endpoint", (nv,), torch.uint8), ("counts", (3,), i32), ("n_contours", (B,), i32), ("n_vertices", (B,), i32),
                                          ("status", (1,), i32)), out)
    ws = workspace(int(lib().p3_init_contours_workspace_bytes(B, H, W)), dev, "init_contours")
    sb, sr, sc = indicator.stride()
    check(lib().p3_init_contours(ptr(indicator), sb, sr, sc, B, H, W, float(level), nv,
                                 nc, ptr(out["pos"]), ptr(out["poly_slice"]), ptr(out["poly_batch"]), ptr(out["batch"]), ptr(out["is_endpoint"]),
                                 ptr(out["counts"]), ptr(out["n_contours"]), ptr(out["n_vertices"]), ptr(out["status"]), ptr(ws), stream()), "p3_init_contours")
    return out


def init_contours(indicator, level=0.5, max_vertices=None, max_contours=None):
    """the checking form of init_contours_device: reads counts and status once (the only read-back), raises when a capacity was too small and narrows every
    array to what was found: pos [N,2], poly_slice [P,2], poly_batch [P], batch [N], is_endpoint [N]; counts = (N, P, longest) as Python ints."""
    out = init_contours_device(indicator, level, max_vertices, max_contours)
    fit = lambda N, P, _: f"{N} vertices in {P} contours do not fit max_vertices = {out['pos'].shape[0]}, max_contours = {out['poly_slice'].shape[0]}"
    return _read_back(out, "init_contours", ((-1, fit),), dict(pos=0, batch=0, is_endpoint=0, poly_slice=1, poly_batch=1))          # -1: any status bit


# ------------------------------------------------------------------------------------------ FFL corner-aware contour simplification
CS_LDS_CAP = 4096          # csrc/corner_split.hip: explicit points of one polyline that run in LDS


def corner_split_device(pos, index, poly_slice, closed, poly_batch, c0c2, tol_pre, tol, max_len=None, force_fallback=False, max_vertices=None,
                        max_pieces=None, stage_flags=False, out=None):
    """p3_corner_split (the array half of FFL's post_process: approximate_polygon, detect_corners, split_polylines_corner, simplify per piece; DESIGN.md
    section 14) without any synchronisation.  pos fp32 [N,2] (row, col); index int64 [K] or None; poly_slice [P,2] into index (into pos without index);
    closed [P] (the first point is appended once more); poly_batch [P] the image of each polyline; c0c2 [B,4,H,W].  tol_pre: stage A (ACM: min(1,
    tolerance); ASM: 0), tol: stage D.  max_len: longest poly_slice row if the caller knows it, None / <= 0: unknown.
    -> dict(out_pos f32 [max_vertices,2], out_src i32 [max_vertices], piece_slice i64 [max_pieces,2], piece_poly i32 [max_pieces], piece_batch i32
    [max_pieces], counts i32 [3] = (vertices, pieces, longest piece), status i32 [1] (bit 0: a capacity was too small; counts are the true totals then and
    nothing is written past the capacities), stage_flags u8 [(K or N) + P] with stage_flags=True).  The default capacities 2 E and E for E = (K or N) + P
    explicit points cannot overflow.  out: the caller's own tensors for any of the outputs (`_outputs`); they have to fit the capacities."""
    for t in (pos, poly_slice, closed, poly_batch, c0c2) + (() if index is None else (index,)):
        _dev(t)
    if pos.dtype != torch.float32 or pos.dim() != 2 or pos.shape[1] != 2:
        raise P3Error(f"corner_split: pos must be float32 [N, 2], got {pos.dtype} {tuple(pos.shape)}")
    N, P = pos.shape[0], poly_slice.shape[0]
    if poly_slice.dim() != 2 or poly_slice.shape[1] != 2 or closed.shape[0] != P or poly_batch.shape[0] != P or (index is not None and index.dim() != 1):
        raise P3Error(f"corner_split: poly_slice [P, 2], closed [P], poly_batch [P], index [K] expected, got {tuple(poly_slice.shape)}, {tuple(closed.shape)}, "
                      f"{tuple(poly_batch.shape)}")
    if c0c2.dim() != 4 or c0c2.shape[1] != 4 or min(c0c2.shape) < 1:
        raise P3Error(f"corner_split: c0c2 [B, 4, H, W] expected, got {tuple(c0c2.shape)}")
    B, _, H, W = c0c2.shape
    K = 0 if index is None else index.shape[0]
    E = (N if index is None else K) + P
    nv = max(2 * E, 1) if max_vertices is None else int(max_vertices)
    nq = max(E, 1) if max_pieces is None else int(max_pieces)
    if nv < 1 or nq < 1:
        raise P3Error(f"corner_split: max_vertices = {max_vertices}, max_pieces = {max_pieces}")
    dev, i32 = pos.device, torch.int32
    flags = (("stage_flags", (max(E, 1),), torch.uint8),) if stage_flags else ()
    out = _outputs("corner_split", dev, (("out_pos", (nv, 2), torch.float32), ("out_src", (nv,), i32), ("piece_slice", (nq, 2), torch.int64), ("piece_poly", (nq,), i32),
                                         ("piece_batch", (nq,), i32)) + flags + (("counts", (3,), i32), ("status", (1,), i32)), out)
    # converted copies stay referenced until the launch is queued
    p32, cf = pos.contiguous(), c0c2.contiguous().float()
    idx = None if index is None else index.to(torch.int64).contiguous()
    sl, cl, pb = poly_slice.to(torch.int64).contiguous(), closed.to(torch.uint8).contiguous(), poly_batch.to(torch.int32).contiguous()
    ws = workspace(int(lib().p3_corner_split_workspace_bytes(E, P)), dev, "corner_split")
    check(lib().p3_corner_split(ptr(p32), N, ptr(idx), K, ptr(sl), ptr(cl), ptr(pb), P, ptr(cf), B, H, W,
                                float(tol_pre), float(tol), int(max_len or 0), int(bool(force_fallback)),
                                nv, nq, ptr(out["out_pos"]), ptr(out["out_src"]), ptr(out["piece_slice"]), ptr(out["piece_poly"]),
                                ptr(out["piece_batch"]), ptr(out.get("stage_flags")), ptr(out["counts"]), ptr(out["status"]), ptr(ws), stream()),
          "p3_corner_split")
    return out


def corner_split(pos, index, poly_slice, closed, poly_batch, c0c2, tol_pre, tol, max_len=None, force_fallback=False, max_vertices=None, max_pieces=None,
                 stage_flags=False):
    """the checking form of corner_split_device: reads counts and status once (the only read-back), raises when a capacity was too small and narrows the
    outputs to what was found: out_pos [V,2], out_src [V], piece_slice [Q,2], piece_poly [Q], piece_batch [Q]; counts = (V, Q, longest piece) as ints."""
    out = corner_split_device(pos, index, poly_slice, closed, poly_batch, c0c2, tol_pre, tol, max_len, force_fallback, max_vertices, max_pieces, stage_flags)
    fit = lambda V, Q, _: f"{V} vertices in {Q} pieces do not fit max_vertices = {out['out_pos'].shape[0]}, max_pieces = {out['piece_slice'].shape[0]}"
    return _read_back(out, "corner_split", ((1, fit), (2, "the rows of poly_slice overlap: they hold more explicit points than index / pos has entries")),
                      dict(out_pos=0, out_src=0, piece_slice=1, piece_poly=1, piece_batch=1))


# ------------------------------------------------------------------------------------------ FFL polygons: planar faces, area and probability filters
def ffl_polygons_capacity(V, B):
    """(max_polygons, max_rings, max_vertices) that cannot overflow for V piece vertices in B images: an image of n piece vertices has at most n segments and
    n + 4 border edges (the four sides, cut once per vertex on them), E = 2 V + 4 B edges in all; every ring has 3 half-edges at least, so there are at
    most 2 E / 3 <= E rings and polygons, and the closed rings hold at most 2 E + 2 E / 3 <= 3 E vertices."""
    E = 2 * int(V) + 4 * int(B)
    return E, E, 3 * E


def ffl_polygons_device(out_pos, piece_slice, piece_batch, indicator, min_area, seg_threshold, max_polygons=None, max_rings=None, max_vertices=None,
                        force_fallback=False, out=None):
    """p3_ffl_polygons (the planar-graph half of FFL's shapely_postprocess: unary_union, polygonize_full, the area and probability filters; DESIGN.md
    section 19) without any synchronisation.  out_pos fp32 [V,2] (row, col), piece_slice [Q,2], piece_batch [Q]: the pieces as corner_split leaves them;
    indicator [B,H,W].
    -> dict(ring_pos f32 [max_vertices,2] (row, col; closed rings), ring_slice i64 [max_rings,2], poly_rings i64 [max_polygons,2] (the rings of a polygon,
    shell first), poly_batch i32, poly_area f32, poly_prob f32, poly_flags i32 [max_polygons] (bit 0: not min_area < area, bit 1: not seg_threshold <
    prob), image_status i32 [B] (bit 0 not planar as given, bit 1 a coordinate is not finite, bit 2 a ring of area 0: the image gives no polygon),
    counts i32 [3] = (polygons, rings, vertices), status i32 [1] (bit 0: a capacity was too small; counts are the true totals then and nothing is written
    past the capacities; bit 1: a piece with piece_batch outside [0, B) or a slice outside out_pos was left out)).  The default capacities
    (ffl_polygons_capacity) cannot overflow.  out: the caller's own tensors for any of the outputs (`_outputs`); they have to fit the capacities."""
    for t in (out_pos, piece_slice, piece_batch, indicator):
        _dev(t)
    if out_pos.dtype != torch.float32 or out_pos.dim() != 2 or out_pos.shape[1] != 2:
        raise P3Error(f"ffl_polygons: out_pos must be float32 [V, 2], got {out_pos.dtype} {tuple(out_pos.shape)}")
    V, Q = out_pos.shape[0], piece_slice.shape[0]
    if piece_slice.dim() != 2 or piece_slice.shape[1] != 2 or piece_batch.dim() != 1 or piece_batch.shape[0] != Q or piece_slice.dtype.is_floating_point \
            or piece_batch.dtype.is_floating_point:
        raise P3Error(f"ffl_polygons: integer piece_slice [Q, 2] and piece_batch [Q] expected, got {piece_slice.dtype} {tuple(piece_slice.shape)}, "
                      f"{piece_batch.dtype} {tuple(piece_batch.shape)}")
    if indicator.dim() != 3 or indicator.shape[0] < 1 or min(indicator.shape[1:]) < 2 or not indicator.dtype.is_floating_point:
        raise P3Error(f"ffl_polygons: a floating-point indicator [B, H, W] with B >= 1 and H, W >= 2 expected, got {indicator.dtype} {tuple(indicator.shape)}")
    B, H, W = indicator.shape
    cap = ffl_polygons_capacity(V, B)
    npoly, nr, nv = (c if m is None else int(m) for c, m in zip(cap, (max_polygons, max_rings, max_vertices)))
    if npoly < 1 or nr < 1 or nv < 1:
        raise P3Error(f"ffl_polygons: max_polygons = {max_polygons}, max_rings = {max_rings}, max_vertices = {max_vertices}")
    dev, f32, i32, i64 = out_pos.device, torch.float32, torch.int32, torch.int64
    out = _outputs("ffl_polygons", dev, (("ring_pos", (nv, 2), f32), ("ring_slice", (nr, 2), i64), ("poly_rings", (npoly, 2), i64), ("poly_batch", (npoly,), i32),
                                         ("poly_area", (npoly,), f32), ("poly_prob", (npoly,), f32), ("poly_flags", (npoly,), i32), ("image_status", (B,), i32),
                                         ("counts", (3,), i32), ("status", (1,), i32)), out)
    # converted copies stay referenced until the launch is queued
    p32, ind = out_pos.contiguous(), indicator.contiguous().float()
    sl, pb = piece_slice.to(i64).contiguous(), piece_batch.to(i32).contiguous()
    ws = workspace(int(lib().p3_ffl_polygons_workspace_bytes(V, B)), dev, "ffl_polygons")
    check(lib().p3_ffl_polygons(ptr(p32), V, ptr(sl), ptr(pb), Q, ptr(ind), B, H, W, float(min_area), float(seg_threshold), int(bool(force_fallback)),
                                npoly, nr, nv, ptr(out["ring_pos"]), ptr(out["ring_slice"]), ptr(out["poly_rings"]), ptr(out["poly_batch"]),
                                ptr(out["poly_area"]), ptr(out["poly_prob"]), ptr(out["poly_flags"]), ptr(out["image_status"]), ptr(out["counts"]),
                                ptr(out["status"]), ptr(ws), stream()), "p3_ffl_polygons")
    return out


def ffl_polygons(out_pos, piece_slice, piece_batch, indicator, min_area, seg_threshold, max_polygons=None, max_rings=None, max_vertices=None,
                 force_fallback=False):
    """the checking form of ffl_polygons_device: reads counts and status once (the only read-back), raises when a capacity was too small or a piece was
    malformed and narrows the outputs to what was found; counts = (polygons, rings, vertices) as ints."""
    out = ffl_polygons_device(out_pos, piece_slice, piece_batch, indicator, min_area, seg_threshold, max_polygons, max_rings, max_vertices, force_fallback)
    fit = lambda P, R, Vn: (f"{P} polygons of {R} rings and {Vn} vertices do not fit max_polygons = {out['poly_rings'].shape[0]}, max_rings = "
                            f"{out['ring_slice'].shape[0]}, max_vertices = {out['ring_pos'].shape[0]}")
    return _read_back(out, "ffl_polygons", ((1, fit), (2, "a piece has piece_batch outside [0, B) or a piece_slice row outside out_pos")),
                      dict(ring_pos=2, ring_slice=1, poly_rings=0, poly_batch=0, poly_area=0, poly_prob=0, poly_flags=0))


# ------------------------------------------------------------------------------------------ polygon metrics: IoU / C-IoU / NR, POLIS, chamfer, Hausdorff
PM_IOU, PM_POLIS, PM_SAMPLES = 1, 2, 4          # include/p3hip.h P3_PM_*
PM_MAX_HW = 1 << 18        # csrc/poly_metrics.hip: pixels of one image whose two bit-packed masks are held in LDS
PM_EDGE_CHUNK = 32         # edges of a ring staged through LDS at a time
PM_TILE = 1024             # samples of a ring in LDS at a time


def _ring_set(who, name, pos, ring_slice, ring_image):
    for t in (pos, ring_slice, ring_image):
        _dev(t)
    if pos.dtype != torch.float32 or pos.dim() != 2 or pos.shape[1] != 2:
        raise P3Error(f"{who}: {name} pos must be float32 [V, 2], got {pos.dtype} {tuple(pos.shape)}")
    R = ring_slice.shape[0]
    if ring_slice.dim() != 2 or ring_slice.shape[1] != 2 or ring_image.dim() != 1 or ring_image.shape[0] != R or ring_slice.dtype.is_floating_point \
            or ring_image.dtype.is_floating_point:
        raise P3Error(f"{who}: integer {name} ring_slice [R, 2] and ring_image [R] expected, got {ring_slice.dtype} {tuple(ring_slice.shape)}, "
                      f"{ring_image.dtype} {tuple(ring_image.shape)}")
    # converted copies stay referenced until the launch is queued
    return pos.contiguous(), ring_slice.to(torch.int64).contiguous(), ring_image.to(torch.int32).contiguous()


def polygon_metrics_workspace_bytes(R_gt, R_dt, B):
    """bytes of workspace p3_polygon_metrics takes for R_gt ground-truth rings and R_dt predicted rings in B images: 24 bytes of state, vertex count, first vertex
    and 32 of box per ring, each section rounded up to 256"""
    return int(lib().p3_polygon_metrics_workspace_bytes(int(R_gt), int(R_dt), int(B)))


def polygon_metrics_device(gt_pos, gt_slice, gt_image, dt_pos, dt_slice, dt_image, batch_size, height, width, modes=PM_IOU | PM_POLIS | PM_SAMPLES, out=None):
    """p3_polygon_metrics (IoU / C-IoU / NR of the rasterised ring sets, POLIS, chamfer and Hausdorff of the matched pairs; include/p3hip.h, DESIGN.md
    section 21) without any synchronisation.  A ring set: pos fp32 [V,2] (x, y), ring_slice [R,2], ring_image [R] non-decreasing; open exterior rings.
    gt_*: the ground truth, dt_*: the predictions.  modes: PM_IOU | PM_POLIS | PM_SAMPLES; the figures of a mode that is off are NaN (image_iou and image_nr, the pair_* and image_* of POLIS, of chamfer and
    Hausdorff; image_counts 0), match, image_valid and invalid_rings are always computed.
    -> dict(metrics f64 [6] = (IoU, C-IoU, NR, POLIS, chamfer, hausdorff), image_iou, image_nr, image_polis, image_chamfer, image_hausdorff f64 [B],
    image_valid i32 [B], image_counts i32 [B,2] = (I, U), match i32 [R_gt] (index into the predictions, -1: no counted pair), pair_polis, pair_chamfer,
    pair_hausdorff f64 [R_gt] (NaN where match is -1), invalid_rings i32 [B,2] = (gt, dt), status i32 [1] (bit 0: an invalid ring - fewer than 3 vertices, a
    coordinate not finite or beyond +-32768; bit 1: a ring with ring_image outside [0, B) or a slice outside pos was left out)).
    out: the caller's own tensors for any of the outputs (`_outputs`)."""
    gp, gs, gi = _ring_set("polygon_metrics", "gt", gt_pos, gt_slice, gt_image)
    dp, ds, di = _ring_set("polygon_metrics", "dt", dt_pos, dt_slice, dt_image)
    B, H, W, modes = int(batch_size), int(height), int(width), int(modes)
    if B < 1 or H < 1 or W < 1 or H * W > PM_MAX_HW:
        raise P3Error(f"polygon_metrics: batch_size, height, width >= 1 and height * width <= {PM_MAX_HW} expected, got {B}, {H}, {W}")
    if modes < 1 or modes & ~(PM_IOU | PM_POLIS | PM_SAMPLES):
        raise P3Error(f"polygon_metrics: modes = {modes} is not a non-empty set of PM_IOU | PM_POLIS | PM_SAMPLES")
    Rg, Rd = gs.shape[0], ds.shape[0]
    dev, f64, i32 = gp.device, torch.float64, torch.int32
    out = _outputs("polygon_metrics", dev, (("metrics", (6,), f64), ("image_iou", (B,), f64), ("image_nr", (B,), f64), ("image_polis", (B,), f64),
                                            ("image_chamfer", (B,), f64), ("image_hausdorff", (B,), f64), ("image_valid", (B,), i32),
                                            ("image_counts", (B, 2), i32), ("match", (Rg,), i32), ("pair_polis", (Rg,), f64), ("pair_chamfer", (Rg,), f64),
                                            ("pair_hausdorff", (Rg,), f64), ("invalid_rings", (B, 2), i32), ("status", (1,), i32)), out)
    ws = workspace(polygon_metrics_workspace_bytes(Rg, Rd, B), dev, "polygon_metrics")
    o = lambda k: ptr(out[k] if out[k].numel() else None)
    check(lib().p3_polygon_metrics(ptr(gp if Rg else None), gp.shape[0], ptr(gs if Rg else None), ptr(gi if Rg else None), Rg,
                                   ptr(dp if Rd else None), dp.shape[0], ptr(ds if Rd else None), ptr(di if Rd else None), Rd, B, H, W, modes,
                                   o("metrics"), o("image_iou"), o("image_nr"), o("image_polis"), o("image_chamfer"), o("image_hausdorff"), o("image_valid"),
                                   o("image_counts"), o("match"), o("pair_polis"), o("pair_chamfer"), o("pair_hausdorff"), o("invalid_rings"), o("status"),
                                   ptr(ws), stream()), "p3_polygon_metrics")
    return out


# ------------------------------------------------------------------------------------------ COCO AP / AR on instance masks and on their boundaries
COCO_SEGM, COCO_BOUNDARY = 1, 2          # include/p3hip.h P3_COCO_*
COCO_KEEP = 100            # csrc/coco_metrics.hip: predictions of an image that take part (maxDets[-1])
COCO_IOU_LDS = 2048        # pair IoUs of an image, both types, that the match kernel stages in LDS


def _ring_field(who, name, t, R, dev):
    """the optional fp32 [R] field of a ring set (score, area) -> contiguous tensor or None"""
    if t is None:
        return None
    _dev(t)
    if t.dtype != torch.float32 or t.dim() != 1 or t.shape[0] != R or t.device != dev:
        raise P3Error(f"{who}: {name} must be float32 [{R}] on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t.contiguous()


def _coco_sizes(B, H, W, types):
    if B < 1 or H < 1 or W < 1 or H * W > PM_MAX_HW:
        raise P3Error(f"coco_metrics: batch_size, height, width >= 1 and height * width <= {PM_MAX_HW} expected, got {B}, {H}, {W}")
    if types < 1 or types & ~(COCO_SEGM | COCO_BOUNDARY):
        raise P3Error(f"coco_metrics: iou_types = {types} is not a non-empty set of COCO_SEGM | COCO_BOUNDARY")


def coco_metrics_workspace_bytes(R_gt, R_dt, B, height, width, iou_types=COCO_SEGM | COCO_BOUNDARY):
    """bytes of workspace p3_coco_metrics takes: per ring the 56 bytes of p3_polygon_metrics, 16 of pixel box, 1 of flags and one slab of height *
    ceil(width / 32) words (three with COCO_BOUNDARY); 400 B of kept lists, 1600 R_gt of pair IoUs, 12 R_dt of ranks and 240 x 13 R_dt of series; each
    section rounded up to 256"""
    return int(lib().p3_coco_metrics_workspace_bytes(int(R_gt), int(R_dt), int(B), int(height), int(width), int(iou_types)))


def coco_metrics_device(gt_pos, gt_slice, gt_image, dt_pos, dt_slice, dt_image, batch_size, height, width, iou_types=COCO_SEGM | COCO_BOUNDARY, dt_score=None,
                        gt_area=None, out=None):
    """p3_coco_metrics (COCO AP / AR on instance masks and on their boundaries; include/p3hip.h) without any synchronisation.  Ring
    sets as for polygon_metrics_device; dt_score fp32 [R_dt] (None: every score 1.0), gt_area fp32 [R_gt] (None: the ring's own pixel count).
    -> dict(stats f64 [2,12], precision f64 [2,10,101,4,3], recall f64 [2,10,4,3], gt_area_px, dt_area_px, gt_boundary_px, dt_boundary_px i32 [R],
    dt_rank i32 [R_dt], pair_inter i32 [2, 100 R_gt], dt_match i32 [2,4,10,R_dt], dt_ignore u8 [2,4,10,R_dt], gt_match i32 [2,4,10,R_gt], status i32 [1]);
    row 0 is segm, row 1 boundary, a type that is off gives NaN.  out: the caller's own tensors for any of the outputs (`_outputs`)."""
    gp, gs, gi = _ring_set("coco_metrics", "gt", gt_pos, gt_slice, gt_image)
    dp, ds, di = _ring_set("coco_metrics", "dt", dt_pos, dt_slice, dt_image)
    B, H, W, types = int(batch_size), int(height), int(width), int(iou_types)
    _coco_sizes(B, H, W, types)
    Rg, Rd = gs.shape[0], ds.shape[0]
    dev, f64, i32 = gp.device, torch.float64, torch.int32
    score, area = _ring_field("coco_metrics", "dt_score", dt_score, Rd, dev), _ring_field("coco_metrics", "gt_area", gt_area, Rg, dev)
    out = _outputs("coco_metrics", dev, (("stats", (2, 12), f64), ("precision", (2, 10, 101, 4, 3), f64), ("recall", (2, 10, 4, 3), f64),
                                         ("gt_area_px", (Rg,), i32), ("dt_area_px", (Rd,), i32), ("gt_boundary_px", (Rg,), i32), ("dt_boundary_px", (Rd,), i32),
                                         ("dt_rank", (Rd,), i32), ("pair_inter", (2, COCO_KEEP * Rg), i32), ("dt_match", (2, 4, 10, Rd), i32),
                                         ("dt_ignore", (2, 4, 10, Rd), torch.uint8), ("gt_match", (2, 4, 10, Rg), i32), ("status", (1,), i32)), out)
    ws = workspace(coco_metrics_workspace_bytes(Rg, Rd, B, H, W, types), dev, "coco_metrics")
    o = lambda k: ptr(out[k] if out[k].numel() else None)
    check(lib().p3_coco_metrics(ptr(gp if Rg else None), gp.shape[0], ptr(gs if Rg else None), ptr(gi if Rg else None), ptr(area if Rg else None), Rg,
                                ptr(dp if Rd else None), dp.shape[0], ptr(ds if Rd else None), ptr(di if Rd else None), ptr(score if Rd else None), Rd,
                                B, H, W, types, o("stats"), o("precision"), o("recall"), o("gt_area_px"), o("dt_area_px"), o("gt_boundary_px"),
                                o("dt_boundary_px"), o("dt_rank"), o("pair_inter"), o("dt_match"), o("dt_ignore"), o("gt_match"), o("status"), ptr(ws),
                                stream()), "p3_coco_metrics")
    return out


# ------------------------------------------------------------------------------------------ max tangent angle error (MTA)
MTA_COUNTED, MTA_INVALID, MTA_EMPTY, MTA_BELOW_PRECISION, MTA_NO_EDGE = 0, 1, 2, 3, 4          # include/p3hip.h P3_MTA_*: ring_state
MTA_MIN_SPACING = 1.0 / 64          # csrc/mta_metrics.hip: a smaller sampling_spacing is refused, which bounds the samples of a ring


def max_tangent_angle_workspace_bytes(R_gt, R_dt, B):
    """bytes of workspace p3_max_tangent_angle takes: the ring records of p3_polygon_metrics (24 bytes of state, vertex count, first vertex and 32 of box
    per ring, each section rounded up to 256) and nothing else: masks, samples and projected points live in LDS"""
    return int(lib().p3_max_tangent_angle_workspace_bytes(int(R_gt), int(R_dt), int(B)))


def max_tangent_angle_device(gt_pos, gt_slice, gt_image, dt_pos, dt_slice, dt_image, batch_size, height, width, sampling_spacing=2.0, min_precision=0.5,
                             max_stretch=2.0, out=None):
    """p3_max_tangent_angle (the mean max tangent angle error of eval/angle_eval.py; include/p3hip.h) without any synchronisation.
    Ring sets as for polygon_metrics_device: gt_* the ground truth, dt_* the predictions.  sampling_spacing >= MTA_MIN_SPACING = 1 / 64.
    -> dict(mta f64 [1] in degrees (NaN when nothing is counted), counted i32 [1], ring_angle (radians), ring_cos f64 [R_dt] (NaN unless the ring is
    counted), ring_state i32 [R_dt] (MTA_COUNTED, MTA_INVALID: invalid or left out, MTA_EMPTY: no pixel, MTA_BELOW_PRECISION, MTA_NO_EDGE), ring_px i32
    [R_dt,2] = (A, I), image_overlap_px i32 [B], invalid_rings i32 [B,2] = (gt, dt), status i32 [1] (bits 0 and 1 as for polygon_metrics_device; bit 2:
    predictions of an image overlap, which the reference would have merged)).  out: the caller's own tensors for any of the outputs (`_outputs`)."""
    gp, gs, gi = _ring_set("max_tangent_angle", "gt", gt_pos, gt_slice, gt_image)
    dp, ds, di = _ring_set("max_tangent_angle", "dt", dt_pos, dt_slice, dt_image)
    B, H, W = int(batch_size), int(height), int(width)
    spacing, precision, stretch = float(sampling_spacing), float(min_precision), float(max_stretch)
    if B < 1 or H < 1 or W < 1 or H * W > PM_MAX_HW:
        raise P3Error(f"max_tangent_angle: batch_size, height, width >= 1 and height * width <= {PM_MAX_HW} expected, got {B}, {H}, {W}")
    if not (MTA_MIN_SPACING <= spacing < math.inf and 0.0 <= precision < 1.0 and 1.0 < stretch < math.inf):
        raise P3Error(f"max_tangent_angle: finite sampling_spacing >= 1 / 64, min_precision in [0, 1) and finite max_stretch > 1 expected, got {spacing}, "
                      f"{precision}, {stretch}")
    Rg, Rd = gs.shape[0], ds.shape[0]
    dev, f64, i32 = gp.device, torch.float64, torch.int32
    out = _outputs("max_tangent_angle", dev, (("mta", (1,), f64), ("counted", (1,), i32), ("ring_angle", (Rd,), f64), ("ring_cos", (Rd,), f64),
                                              ("ring_state", (Rd,), i32), ("ring_px", (Rd, 2), i32), ("image_overlap_px", (B,), i32),
                                              ("invalid_rings", (B, 2), i32), ("status", (1,), i32)), out)
    ws = workspace(max_tangent_angle_workspace_bytes(Rg, Rd, B), dev, "max_tangent_angle")
    o = lambda k: ptr(out[k] if out[k].numel() else None)
    check(lib().p3_max_tangent_angle(ptr(gp if Rg else None), gp.shape[0], ptr(gs if Rg else None), ptr(gi if Rg else None), Rg,
                                     ptr(dp if Rd else None), dp.shape[0], ptr(ds if Rd else None), ptr(di if Rd else None), Rd, B, H, W, spacing, precision,
                                     stretch, o("mta"), o("counted"), o("ring_angle"), o("ring_cos"), o("ring_state"), o("ring_px"), o("image_overlap_px"),
                                     o("invalid_rings"), o("status"), ptr(ws), stream()), "p3_max_tangent_angle")
    return out


# ------------------------------------------------------------------------------------------ mask / topology metrics, subset IoU, annotation counts
MM_TOPDIG, MM_SUBSET, MM_STATS = 1, 2, 4          # include/p3hip.h P3_MM_*
MM_MAX_THICKNESS = 64      # csrc/mask_metrics.hip: the largest buffer_thickness


def mask_metrics_workspace_bytes(R_gt, R_dt, B):
    """bytes of workspace p3_mask_metrics takes: the ring records of p3_polygon_metrics (24 bytes of state, vertex count, first vertex and 32 of box per
    ring) and 32 bytes of counts per image, each section rounded up to 256; the masks live in LDS"""
    return int(lib().p3_mask_metrics_workspace_bytes(int(R_gt), int(R_dt), int(B)))


def mask_metrics_device(gt_pos, gt_slice, gt_image, dt_pos, dt_slice, dt_image, batch_size, height, width, buffer_thickness=5,
                        modes=MM_TOPDIG | MM_SUBSET | MM_STATS, out=None):
    """p3_mask_metrics (the reference's modes topdig, subset_iou and stats; include/p3hip.h) without any synchronisation.  Ring sets
    as for polygon_metrics_device: gt_* the ground truth, dt_* the predictions.  buffer_thickness in [1, MM_MAX_THICKNESS]: the width of the stroked
    outlines (the reference: 5).  modes: MM_TOPDIG | MM_SUBSET | MM_STATS; a mode that is off leaves NaN in its floating-point outputs and 0 in its
    integer ones.
    -> dict(metrics f64 [9] = (IoU_, P-Acc, F1-Score, IoU-Topo, P-Acc-Topo, F1-Score-Topo, sIoU, sC-IoU, sNR), stats i64 [7] = (images, images with gt
    rings, images with predictions, gt rings, predictions, gt vertices, prediction vertices), image_conf i32 [B,2,4] = (filled, stroked) x (TP, FP, FN,
    TN), image_scores f64 [B,6] in the order of metrics[0..5], image_nr f64 [B], image_subset i32 [B], invalid_rings i32 [B,2] = (gt, dt), status i32 [1]
    (bits 0 and 1 as for polygon_metrics_device)).  out: the caller's own tensors for any of the outputs (`_outputs`)."""
    gp, gs, gi = _ring_set("mask_metrics", "gt", gt_pos, gt_slice, gt_image)
    dp, ds, di = _ring_set("mask_metrics", "dt", dt_pos, dt_slice, dt_image)
    B, H, W, T, modes = int(batch_size), int(height), int(width), int(buffer_thickness), int(modes)
    if B < 1 or H < 1 or W < 1 or H * W > PM_MAX_HW:
        raise P3Error(f"mask_metrics: batch_size, height, width >= 1 and height * width <= {PM_MAX_HW} expected, got {B}, {H}, {W}")
    if not 1 <= T <= MM_MAX_THICKNESS:
        raise P3Error(f"mask_metrics: buffer_thickness in [1, {MM_MAX_THICKNESS}] expected, got {buffer_thickness}")
    if modes < 1 or modes & ~(MM_TOPDIG | MM_SUBSET | MM_STATS):
        raise P3Error(f"mask_metrics: modes = {modes} is not a non-empty set of MM_TOPDIG | MM_SUBSET | MM_STATS")
    Rg, Rd = gs.shape[0], ds.shape[0]
    dev, f64, i32 = gp.device, torch.float64, torch.int32
    out = _outputs("mask_metrics", dev, (("metrics", (9,), f64), ("stats", (7,), torch.int64), ("image_conf", (B, 2, 4), i32), ("image_scores", (B, 6), f64),
                                         ("image_nr", (B,), f64), ("image_subset", (B,), i32), ("invalid_rings", (B, 2), i32), ("status", (1,), i32)), out)
    ws = workspace(mask_metrics_workspace_bytes(Rg, Rd, B), dev, "mask_metrics")
    o = lambda k: ptr(out[k])
    check(lib().p3_mask_metrics(ptr(gp if Rg else None), gp.shape[0], ptr(gs if Rg else None), ptr(gi if Rg else None), Rg,
                                ptr(dp if Rd else None), dp.shape[0], ptr(ds if Rd else None), ptr(di if Rd else None), Rd, B, H, W, T, modes,
                                o("metrics"), o("stats"), o("image_conf"), o("image_scores"), o("image_nr"), o("image_subset"), o("invalid_rings"),
                                o("status"), ptr(ws), stream()), "p3_mask_metrics")
    return out


# ------------------------------------------------------------------------------------------ FFL active-skeleton optimiser
ASM_LDS_CAP = 4096         # csrc/asm.hip: nodes of one connected component that fit the one-launch LDS path
FFL_POLY_LDS_CAP = 1024    # csrc/ffl_polygons.hip: edge slots of one image (its segments + its segment ends on the border + 4) that run in LDS
ASM_MAX_KNOTS = 8


def _asm_knots(knots):
    """[step_thresholds, data, length, crossfield] -> (ctypes double [4 * nk], nk)"""
    rows = [[float(v) for v in r] for r in knots]
    nk = len(rows[0]) if rows else 0
    if len(rows) != 4 or any(len(r) != nk for r in rows) or not 2 <= nk <= ASM_MAX_KNOTS:
        raise P3Error(f"asm: knots must be [step_thresholds, data, length, crossfield] with 2 .. {ASM_MAX_KNOTS} entries each")
    return (ctypes.c_double * (4 * nk))(*[v for r in rows for v in r]), nk


def asm_schedule(iter_num, knots, lr=0.1, gamma=0.995):
    """p3_asm_schedule (host only, needs no device): the (data, length, crossfield, lr) floats the kernel uses at iteration iter_num, as Python floats"""
    arr, nk = _asm_knots(knots)
    out = (ctypes.c_double * 4)()
    check(lib().p3_asm_schedule(int(iter_num), arr, nk, lr, gamma, out), "p3_asm_schedule")
    return tuple(out)


def asm_optimize(pos, sq, plan, is_tip, batch, indicator, c0c2, knots, data_level=0.5, lr=0.1, gamma=0.995, first_iter=0, steps=300, grad_out=None,
                 losses=False, force_fallback=False):
    """p3_asm_optimize (predict/ffl/polygonize_asm.py:133-421): `steps` RMSprop iterations first_iter .. first_iter + steps - 1 on pos fp32 [N,2] (row, col),
    IN PLACE, with the state sq fp32 [N,2] (zeros on a first call) read and written.  plan: polygonize_asm.AsmPlan on the device (components, occurrence
    lists and neighbour indices derived from path_index / path_delim, built once per skeleton on the host) or its device-built twin (asm_plan below).  is_tip [N] (degrees == 1), batch [N].
    indicator [B,H,W] or seg [B,C,H,W] (channel 0 is taken), c0c2 [B,4,H,W]; bf16 / strided maps are copied to contiguous fp32.
    knots: [step_thresholds, data, length, crossfield] of loss_params.coefs.  grad_out: None or contiguous fp32 [N,2], receives the gradient of the last
    executed step.  Reads nothing back.  -> pos, or (pos, losses fp32 [C,3] = (align, level, length) per component at the last step, before its update)."""
    for t in (pos, sq, is_tip, batch, indicator, c0c2) + tuple(getattr(plan, k) for k in ("comp_ptr", "cn_node", "cn_occ", "slot_nb")):
        _dev(t)
    for name, t in (("pos", pos), ("sq", sq), ("grad_out", grad_out)):
        if t is not None and (not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 2 or not t.is_contiguous() or t.shape[0] != pos.shape[0]):
            raise P3Error(f"asm_optimize: {name} must be a contiguous float32 [N, 2] device tensor (it is written in place), got {t.dtype} {tuple(t.shape)}")
    N, C, CN, S = pos.shape[0], plan.comp_ptr.shape[0] - 1, plan.cn_node.shape[0], plan.slot_nb.shape[0]
    if is_tip.shape[0] != N or batch.shape[0] != N or plan.cn_occ.shape[0] != CN + 1 or plan.slot_nb.dim() != 2 or plan.slot_nb.shape[1] != 2 or C < 0:
        raise P3Error(f"asm_optimize: is_tip [N], batch [N] and a plan with cn_occ [CN+1], slot_nb [S,2] expected, got {tuple(is_tip.shape)}, {tuple(batch.shape)}, "
                      f"{tuple(plan.cn_occ.shape)}, {tuple(plan.slot_nb.shape)}")
    ind, cf, (B, H, W) = _ffl_maps("asm_optimize", indicator, c0c2)
    arr, nk = _asm_knots(knots)
    out = torch.zeros((max(C, 0), 3), dtype=torch.float32, device=pos.device) if losses else None
    if C <= 0 or N == 0 or steps == 0:
        return (pos, out) if losses else pos
    i32 = lambda t: t.to(torch.int32).contiguous()
    # converted copies stay referenced until the launch is queued: a temporary freed while the argument list is built is handed to the next conversion
    comp_ptr, cn_node, cn_occ, slot_nb = (i32(getattr(plan, k)) for k in ("comp_ptr", "cn_node", "cn_occ", "slot_nb"))
    tip8, batch32 = is_tip.to(torch.uint8).contiguous(), i32(batch)
    ws = None
    if force_fallback or plan.max_comp > ASM_LDS_CAP or plan.max_comp <= 0:
        ws = workspace(int(lib().p3_asm_workspace_bytes(N, CN)), pos.device, "asm")
    check(lib().p3_asm_optimize(ptr(pos), ptr(sq), N, ptr(comp_ptr), C, ptr(cn_node), ptr(cn_occ), CN,
                                ptr(slot_nb), S, ptr(tip8), ptr(batch32), ptr(ind), ptr(cf), B,
                                H, W, data_level, arr, nk, lr, gamma, int(first_iter),
                                int(steps), int(plan.max_comp), int(bool(force_fallback)), ptr(grad_out), ptr(out), ptr(ws), stream()),
          "p3_asm_optimize")
    return (pos, out) if losses else pos


# ------------------------------------------------------------------------------------------ FFL active-skeleton initialisation (marching squares) and plan
def skeleton_from_contours_device(pos, poly_slice, poly_batch, is_endpoint, batch_size, min_area=None, max_nodes=None, max_slots=None, max_paths=None,
                                  out=None):
    """p3_skeleton_from_contours (the conversion half of get_marching_squares_skeleton, predict/ffl/polygonize_asm.py:581-638, plus
    skeletons_to_tensorskeleton) without any synchronisation.  The contour container as init_contours leaves it: pos fp32 [N,2], poly_slice [P,2],
    poly_batch [P], is_endpoint [N].  min_area None keeps every contour, a number keeps those with at least 3 vertices and a larger shoelace area.
    -> dict(pos f32 [max_nodes,2], degrees i64 [max_nodes], path_index i64 [max_slots], path_delim i64 [max_paths+1], batch i64 [max_nodes], batch_delim i64
    [B+1], counts i32 [4] = (nodes, slots, paths, nodes of the longest kept path), status i32 [1] (bit 0: a capacity was too small; counts are the true totals
    then and nothing is written past the capacities)).  The default capacities N, N + P and P cannot overflow.  out: the caller's own tensors for any of the outputs (`_outputs`)."""
    for t in (pos, poly_slice, poly_batch, is_endpoint):
        _dev(t)
    if pos.dtype != torch.float32 or pos.dim() != 2 or pos.shape[1] != 2:
        raise P3Error(f"skeleton_from_contours: pos must be float32 [N, 2], got {pos.dtype} {tuple(pos.shape)}")
    N, P, B = pos.shape[0], poly_slice.shape[0], int(batch_size)
    if poly_slice.dim() != 2 or poly_slice.shape[1] != 2 or poly_batch.shape[0] != P or is_endpoint.shape[0] != N or B < 1:
        raise P3Error(f"skeleton_from_contours: poly_slice [P, 2], poly_batch [P], is_endpoint [N] and batch_size >= 1 expected, got {tuple(poly_slice.shape)}, "
                      f"{tuple(poly_batch.shape)}, {tuple(is_endpoint.shape)}, {batch_size}")
    nn = max(N, 1) if max_nodes is None else int(max_nodes)
    ns = max(N + P, 1) if max_slots is None else int(max_slots)
    npth = max(P, 1) if max_paths is None else int(max_paths)
    if nn < 1 or ns < 1 or npth < 1:
        raise P3Error(f"skeleton_from_contours: max_nodes = {max_nodes}, max_slots = {max_slots}, max_paths = {max_paths}")
    dev, i32, i64 = pos.device, torch.int32, torch.int64
    out = _outputs("skeleton_from_contours", dev, (("pos", (nn, 2), torch.float32), ("degrees", (nn,), i64), ("path_index", (ns,), i64), ("path_delim", (npth + 1,), i64),
                                                   ("batch", (nn,), i64), ("batch_delim", (B + 1,), i64), ("counts", (4,), i32), ("status", (1,), i32)), out)
    # converted copies stay referenced until the launch is queued
    p32, sl = pos.contiguous(), poly_slice.to(torch.int64).contiguous()
    pb, ep = poly_batch.to(torch.int32).contiguous(), is_endpoint.to(torch.uint8).contiguous()
    ws = workspace(int(lib().p3_skeleton_from_contours_workspace_bytes(P)), dev, "skeleton_from_contours") if P else None
    check(lib().p3_skeleton_from_contours(ptr(p32), N, ptr(sl), ptr(pb), ptr(ep), P, B, int(min_area is not None),
                                          0.0 if min_area is None else float(min_area), nn, ns, npth, ptr(out["pos"]), ptr(out["degrees"]),
                                          ptr(out["path_index"]), ptr(out["path_delim"]), ptr(out["batch"]), ptr(out["batch_delim"]), ptr(out["counts"]),
                                          ptr(out["status"]), ptr(ws), stream()), "p3_skeleton_from_contours")
    return out


def skeleton_from_contours(pos, poly_slice, poly_batch, is_endpoint, batch_size, min_area=None, max_nodes=None, max_slots=None, max_paths=None):
    """the checking form of skeleton_from_contours_device: reads counts and status once (the only read-back), raises when a capacity was too small and
    narrows the arrays: pos [N',2], degrees [N'], path_index [M'], path_delim [P'+1] ([0] without a path), batch [N']; counts = (N', M', P', longest)."""
    out = skeleton_from_contours_device(pos, poly_slice, poly_batch, is_endpoint, batch_size, min_area, max_nodes, max_slots, max_paths)
    fit = lambda N, M, P, _: (f"{N} nodes, {M} slots and {P} paths do not fit max_nodes = {out['pos'].shape[0]}, max_slots = {out['path_index'].shape[0]}, "
                              f"max_paths = {out['path_delim'].shape[0] - 1}")
    P = _read_back(out, "skeleton_from_contours", ((1, fit),), dict(pos=0, degrees=0, batch=0, path_index=1))["counts"][2]
    out["path_delim"] = out["path_delim"][:P + 1] if P else torch.zeros(1, dtype=torch.int64, device=pos.device)          # nothing was written without a path
    return out


def asm_plan_device(path_index, path_delim, num_nodes, out=None):
    """p3_asm_plan without any synchronisation: path_index [M], path_delim [paths + 1] and the node count -> dict of the six int32 arrays of
    polygonize_asm.AsmPlan at their largest sizes (comp_ptr [N+1] with C + 1 entries used, cn_node [N], cn_occ [N+1], slot_nb [M,2], node_local [N], slot_k
    [M]), counts i32 [2] = (C, nodes of the largest component) and status i32 [1] (bit 1: a node id outside [0, N); the arrays are no plan then).
    out: the caller's own tensors for any of the outputs (`_outputs`)."""
    for t in (path_index, path_delim):
        _dev(t)
    if path_index.dim() != 1 or path_delim.dim() != 1 or int(num_nodes) < 0:
        raise P3Error(f"asm_plan: path_index [M], path_delim [P+1] and num_nodes >= 0 expected, got {tuple(path_index.shape)}, {tuple(path_delim.shape)}, {num_nodes}")
    N, M, D = int(num_nodes), path_index.shape[0], path_delim.shape[0]
    dev, i32 = path_index.device, torch.int32
    out = _outputs("asm_plan", dev, (("comp_ptr", (N + 1,), i32), ("cn_node", (N,), i32), ("cn_occ", (N + 1,), i32), ("slot_nb", (M, 2), i32), ("node_local", (N,), i32),
                                     ("slot_k", (M,), i32), ("counts", (2,), i32), ("status", (1,), i32)), out)
    idx, delim = path_index.to(torch.int64).contiguous(), path_delim.to(torch.int64).contiguous()
    ws = workspace(int(lib().p3_asm_plan_workspace_bytes(N, M)), dev, "asm_plan") if N else None
    check(lib().p3_asm_plan(ptr(idx), M, ptr(delim), D, N, ptr(out["comp_ptr"]), ptr(out["cn_node"]), ptr(out["cn_occ"]), ptr(out["slot_nb"]),
                            ptr(out["node_local"]), ptr(out["slot_k"]), ptr(out["counts"]), ptr(out["status"]), ptr(ws), stream()), "p3_asm_plan")
    return out


def asm_plan(path_index, path_delim, num_nodes):
    """the checking form of asm_plan_device: reads counts and status once (the only read-back), raises on a node id outside [0, N), narrows comp_ptr to
    [C+1]; counts = (C, max_comp) as Python ints."""
    out = asm_plan_device(path_index, path_delim, num_nodes)
    C = _read_back(out, "asm_plan", ((2, f"path_index holds node ids outside [0, {int(num_nodes)})"),), {})["counts"][0]
    out["comp_ptr"] = out["comp_ptr"][:C + 1]
    return out


# ------------------------------------------------------------------------------------------ FFL active-skeleton initialisation from the segmentation map
SKELETON_THIN_MAX_SIDE = 508          # csrc/skeleton_thin.hip: H + 4 and W + 4 <= 512, two bit planes of the padded image in 64 KB of LDS


def skeleton_from_seg_capacity(B, H, W):
    """(max_nodes, max_slots, max_paths) that cannot overflow: N <= B H W; a node has at most 4 links (a diagonal link needs both 4-neighbours beside it
    empty), so links <= 2 N; every link lies on exactly one path and a path has one slot more than links: P <= links and M = links + P <= 4 N."""
    n = max(int(B) * int(H) * int(W), 1)
    return n, 4 * n, 2 * n


def skeleton_from_seg_device(seg, level=0.5, max_nodes=None, max_slots=None, max_paths=None, out=None):
    """p3_skeleton_from_seg (init_method "skeleton_device", DESIGN.md section 20: edge mask, closing, Zhang-Suen thinning, link graph, maximal degree-2 paths)
    without any synchronisation.  seg fp32 [B,C,H,W]: channel 0 the interior probability, channel 1 (when C >= 2) the edge probability; batch and channel
    strides are taken as they are (a channel slice of a wider tensor is not copied), rows must be contiguous or the map is copied.  H, W <= 508.
    -> dict(pos f32 [max_nodes,2] (row, col), degrees i64 [max_nodes], path_index i64 [max_slots], path_delim i64 [max_paths+1], batch i64 [max_nodes],
    batch_delim i64 [B+1], counts i32 [4] = (nodes, slots, paths, nodes of the longest path), status i32 [1] (bit 0: a capacity was too small; counts are
    the true totals then and nothing is written past the capacities)).  The default capacities (skeleton_from_seg_capacity) cannot overflow.
    out: the caller's own tensors for any of the outputs (`_outputs`)."""
    _dev(seg)
    if seg.dim() != 4 or seg.shape[1] < 1 or seg.shape[2] < 1 or seg.shape[3] < 1:
        raise P3Error(f"skeleton_from_seg: seg [B, C, H, W] with C, H, W >= 1 expected, got {tuple(seg.shape)}")
    B, C, H, W = seg.shape
    if max(H, W) > SKELETON_THIN_MAX_SIDE:
        raise P3Error(f"skeleton_from_seg: H and W must not exceed {SKELETON_THIN_MAX_SIDE}, got {H} x {W}")
    cap = skeleton_from_seg_capacity(B, H, W)
    nn, ns, npth = (c if m is None else int(m) for c, m in zip(cap, (max_nodes, max_slots, max_paths)))
    if nn < 1 or ns < 1 or npth < 1:
        raise P3Error(f"skeleton_from_seg: max_nodes = {max_nodes}, max_slots = {max_slots}, max_paths = {max_paths}")
    dev, i32, i64 = seg.device, torch.int32, torch.int64
    out = _outputs("skeleton_from_seg", dev, (("pos", (nn, 2), torch.float32), ("degrees", (nn,), i64), ("path_index", (ns,), i64), ("path_delim", (npth + 1,), i64),
                                              ("batch", (nn,), i64), ("batch_delim", (B + 1,), i64), ("counts", (4,), i32), ("status", (1,), i32)), out)
    # a converted copy stays referenced until the launch is queued
    s32 = seg if seg.dtype == torch.float32 else seg.float()
    if s32.stride(3) != 1 or s32.stride(2) != W or min(s32.stride(0), s32.stride(1)) < 0:
        s32 = s32.contiguous()
    ws = workspace(int(lib().p3_skeleton_from_seg_workspace_bytes(B, H, W)), dev, "skeleton_from_seg") if B else None
    check(lib().p3_skeleton_from_seg(ptr(s32), B, C, H, W, s32.stride(0), s32.stride(1), float(level), nn, ns, npth, ptr(out["pos"]), ptr(out["degrees"]),
                                     ptr(out["path_index"]), ptr(out["path_delim"]), ptr(out["batch"]), ptr(out["batch_delim"]), ptr(out["counts"]),
                                     ptr(out["status"]), ptr(ws), stream()), "p3_skeleton_from_seg")
    return out


def skeleton_from_seg(seg, level=0.5, max_nodes=None, max_slots=None, max_paths=None):
    """the checking form of skeleton_from_seg_device: reads counts and status once (the only read-back), raises when a capacity was too small and narrows
    the arrays: pos [N,2], degrees [N], path_index [M], path_delim [P+1] ([0] without a path), batch [N]; counts = (N, M, P, longest)."""
    out = skeleton_from_seg_device(seg, level, max_nodes, max_slots, max_paths)
    fit = lambda N, M, P, _: (f"{N} nodes, {M} slots and {P} paths do not fit max_nodes = {out['pos'].shape[0]}, max_slots = {out['path_index'].shape[0]}, "
                              f"max_paths = {out['path_delim'].shape[0] - 1}")
    P = _read_back(out, "skeleton_from_seg", ((1, fit),), dict(pos=0, degrees=0, batch=0, path_index=1))["counts"][2]
    out["path_delim"] = out["path_delim"][:P + 1] if P else torch.zeros(1, dtype=torch.int64, device=seg.device)          # nothing was written without a path
    return out


def cast(a, dtype):
    out = torch.empty(a.shape, dtype=dtype, device=a.device)
    check(lib().p3_cast(ptr(a.contiguous()), dt(a), ptr(out), dt(out), a.numel(), stream()), "p3_cast")
    return out


def add_pos(x, pos):
    B, L, D = x.shape
    out = torch.empty_like(x)
    check(lib().p3_add_pos(ptr(x), ptr(pos), ptr(out), B, L, D, dt(x), stream()), "p3_add_pos")
    return out


# ------------------------------------------------------------------------------------------ backward / training ops
def attention_bwd(q, k, v, o, lse, do, heads, scale, causal=False, key_bias=None, dq=None, dk=None, dv=None, drop=None, drop_rows=None, grad_planes=None):
    """dq/dk/dv get the same batch/row strides as q/k/v (pass views of a packed buffer to get a packed gradient).
    grad_planes (fp32x3 self-attention on a packed qkv [B, L, 3D]): a Planes [B * L, 3D] that receives the packed gradient (dq | dk | dv) as planes - the operand
    of the qkv projection's backward GEMMs - instead of fp32 tensors; returns it."""
    if grad_planes is not None:
        B, L, D = q.shape
        gp = grad_planes
        if gp.cols != 3 * D or gp.rows != B * L or not split_now():
            raise P3Error("attention_bwd: grad_planes must be [B * L, 3D] and the call must run in an fp32x3 scope")
        if do.stride() != o.stride():
            raise P3Error("attention_bwd: dO strides must equal O strides")
        d = _attn_desc(q, k, v, o, heads, scale, causal, key_bias, None, drop, drop_rows)
        d.grad_planes, d.g_rs, d.g_bs, d.g_lo = 1, gp.ld, L * gp.ld, gp.cols
        delta = torch.empty((B, heads, L), dtype=torch.float32, device=q.device)
        base, es = gp.hi.data_ptr(), 2
        check(lib().p3_attention_bwd(ptr(q), ptr(k), ptr(v), ptr(o), ptr(do), ptr(lse), base, base + D * es, base + 2 * D * es,
                                     ptr(delta), byref(d), stream()), "p3_attention_bwd")
        return gp
    dq = torch.empty_like(q) if dq is None else dq
    dk = torch.empty_like(k) if dk is None else dk
    dv = torch.empty_like(v) if dv is None else dv
    for a, b_ in ((q, dq), (k, dk), (v, dv)):
        if a.stride() != b_.stride():
            raise P3Error("attention_bwd: gradient strides must equal input strides")
    if do.stride() != o.stride():
        raise P3Error("attention_bwd: dO strides must equal O strides")
    d = _attn_desc(q, k, v, o, heads, scale, causal, key_bias, None, drop, drop_rows)
    delta = torch.empty((q.shape[0], heads, q.shape[1]), dtype=torch.float32, device=q.device)
    check(lib().p3_attention_bwd(ptr(q), ptr(k), ptr(v), ptr(o), ptr(do), ptr(lse), ptr(dq), ptr(dk), ptr(dv), ptr(delta), byref(d),
                                 stream()), "p3_attention_bwd")
    return dq, dk, dv


def _tn_slabs(N, K, a):
    """(scratch, max slabs) for the split-M partial tiles of the weight-gradient GEMM: stored + summed in split order by tn_reduce_kernel
    instead of fp32 atomics - in deterministic launches (hip.det_on) only: elsewhere the atomics were faster (r02 A/B: 43.3 ms with atomics, 43.7 - 48 with slabs)."""
    if det_on(a):
        ns = max(8, min(512, (64 << 20) // (N * K * 4)))         # <= 64 MB of slabs, at least 8
        return workspace(ns * N * K * 4 + 16, a.device, "tn_slabs"), ns
    return None, 0


def gemm_tn(a, b, out=None, colsum_out=None):
    """out[N,K] (+)= a[M,N]^T @ b[M,K]  (fp32 out; zero-filled when not given); colsum_out[N] += column sums of a (bias gradient)."""
    M, N = a.shape
    K = b.shape[1]
    if out is None:
        out = torch.zeros((N, K), dtype=torch.float32, device=a.device)
    slabs, ns = _tn_slabs(N, K, a)
    ev = KTIMER.begin()
    if ev is not None:
        lib().p3_trace_kernels(1)                        # forget the previous launch's name: an untraced kernel must not inherit it
    check(lib().p3_gemm_tn_ex(ptr(a), ptr(b), ptr(out), M, N, K, a.stride(0), b.stride(0),
                              out.stride(0), dt_mm(a), 0, ptr(None), ptr(None), ptr(None), 0, ptr(colsum_out),
                              ptr(slabs), ns, stream()), "p3_gemm_tn")
    if ev is not None:                                          # operands once, the fp32 output tile once (split-M partials are not algorithmic)
        kname = lib().p3_last_kernel().decode() or f"gemm_tn_kernel<{'bf16' if dt(a) == BF16 else 'float'}, 0>"
        KTIMER.end(ev, kname, 2.0 * M * N * K, float(M * (N + K) * a.element_size() + N * K * 4))
    return out


def colsum(x, out=None):
    M, N = x.shape
    if out is None:
        out = torch.zeros(N, dtype=torch.float32, device=x.device)
    check(lib().p3_colsum(ptr(x), ptr(out), M, N, x.stride(0), dt(x), stream()), "p3_colsum")
    return out


def batch_sum(x):
    """sum over the leading dim of a contiguous [B, ...] tensor -> fp32 [...]."""
    B = x.shape[0]
    return colsum(x.reshape(B, -1)).view(x.shape[1:])


def act_bwd(dy, saved, act, out_dtype, scale=1.0):
    out = torch.empty(dy.shape, dtype=out_dtype, device=dy.device)
    dyc, sc = dy.contiguous(), saved.contiguous()
    check(lib().p3_act_bwd(ptr(dyc), dt(dyc), ptr(sc), dt(sc), ptr(out), dt(out), dy.numel(), act, scale, stream()), "p3_act_bwd")
    return out


def embed_tokens_bwd(dx, tokens, emb_shape, pos_shape):
    B, L, D = dx.shape
    demb = torch.zeros(emb_shape, dtype=torch.float32, device=dx.device)
    dpos = torch.zeros(pos_shape, dtype=torch.float32, device=dx.device)
    check(lib().p3_embed_tokens_bwd_v(ptr(dx), dt(dx), ptr(tokens), ptr(demb), B, L, D, emb_shape[0], stream()), "p3_embed_tokens_bwd_v")
    colsum(dx.reshape(B, L * D), out=dpos.reshape(-1)[:L * D])          # dpos[t] = sum over the batch: column sums, no atomics
    return demb, dpos


def tokens_assemble_bwd(dx, tok, scale, shift, B, np_, D, src_ld, mean=None):
    dsrc = torch.empty((B * np_, D), dtype=tok.dtype, device=dx.device)
    dscale = torch.zeros(D, dtype=torch.float32, device=dx.device) if scale is not None else None
    dshift = torch.zeros(D, dtype=torch.float32, device=dx.device) if scale is not None else None
    check(lib().p3_tokens_assemble_bwd(ptr(dx.contiguous()), ptr(tok), tok.stride(-2) if src_ld is None else src_ld, dt(tok),
                                       ptr(scale), ptr(shift), ptr(mean), ptr(dsrc), ptr(dscale), ptr(dshift), B, np_, D, stream()),
          "p3_tokens_assemble_bwd")
    return dsrc, dscale, dshift


def pool_pos_bwd(dout, yshape, ydtype):
    B, L, Din = yshape
    dy = torch.empty(yshape, dtype=ydtype, device=dout.device)
    check(lib().p3_pool_pos_bwd(ptr(dout), dt(dout), ptr(dy), dt(dy), B, L - 1, Din, dout.shape[-1], stream()), "p3_pool_pos_bwd")
    return dy


def pair_mean_bwd(dF, B, L, N, D, dtype, accumulate_into=None):
    out = accumulate_into if accumulate_into is not None else torch.empty((B, L, D), dtype=dtype, device=dF.device)
    check(lib().p3_pair_mean_bwd(ptr(dF.contiguous()), ptr(out), dt(out), B, L, N, D, int(accumulate_into is not None), stream()), "p3_pair_mean_bwd")
    return out


def sinkhorn_bwd(scores, alpha, perm, hist, dperm, iters):
    B, m, n = scores.shape
    dscores = torch.empty_like(scores)
    dalpha = torch.zeros(1, dtype=torch.float32, device=scores.device)
    ws = workspace(int(lib().p3_sinkhorn_bwd_workspace_bytes(B, m, n, iters)), scores.device, "sinkhorn_bwd")
    check(lib().p3_sinkhorn_bwd(ptr(scores), ptr(alpha), B, m, n, iters, ptr(perm), ptr(hist), ptr(dperm),
                                ptr(dscores), ptr(dalpha), ptr(ws), stream()), "p3_sinkhorn_bwd")
    return dscores, dalpha


def ce_loss_fwd(logits2d, targets, ignore_index):
    R, V = logits2d.shape
    lse = torch.empty(R, dtype=torch.float32, device=logits2d.device)
    acc = torch.zeros(2, dtype=torch.float32, device=logits2d.device)
    check(lib().p3_ce_loss_fwd(ptr(logits2d), logits2d.stride(0), ptr(targets), R, V, ignore_index, ptr(lse), ptr(acc), stream()), "p3_ce_loss_fwd")
    return lse, acc


def ce_loss_bwd(logits2d, targets, ignore_index, lse, acc, gscale, out_dtype=torch.float32, vpad=None):
    R, V = logits2d.shape
    vpad = vpad or V
    out = torch.empty((R, vpad), dtype=out_dtype, device=logits2d.device)
    check(lib().p3_ce_loss_bwd(ptr(logits2d), logits2d.stride(0), ptr(targets), R, V, ignore_index, ptr(lse),
                               ptr(acc), ptr(gscale), ptr(out), dt(out), vpad, vpad, stream()), "p3_ce_loss_bwd")
    return out


def bce_loss_fwd(p, y):
    acc = torch.zeros(1, dtype=torch.float32, device=p.device)
    check(lib().p3_bce_loss_fwd(ptr(p), ptr(y), p.numel(), ptr(acc), stream()), "p3_bce_loss_fwd")
    return acc


def bce_loss_bwd(p, y, gscale):
    dp = torch.empty_like(p)
    check(lib().p3_bce_loss_bwd(ptr(p), ptr(y), p.numel(), ptr(gscale), ptr(dp), stream()), "p3_bce_loss_bwd")
    return dp


def adamw_schedule(step, hyper, base_lr, kind, warmup, total, beta1, beta2):
    check(lib().p3_adamw_schedule(ptr(step), ptr(hyper), base_lr, kind, warmup, total, beta1, beta2, stream()), "p3_adamw_schedule")


def adamw_schedule_dev(step, hyper, sched, beta1, beta2):
    check(lib().p3_adamw_schedule_dev(ptr(step), ptr(hyper), ptr(sched), beta1, beta2, stream()), "p3_adamw_schedule_dev")


def adamw(params, grads, m, v, hyper, beta1, beta2, eps, wd, grad_scale=1.0, shadow=None):
    check(lib().p3_adamw(ptr(params), ptr(grads), ptr(m), ptr(v), params.numel(), ptr(hyper), beta1, beta2, eps, wd, grad_scale, ptr(shadow), stream()), "p3_adamw")


# ------------------------------------------------------------------------------------------ ScoreNet backward
A_AFFINE_MASK2 = 5


def bn_sums_from_g(G, W, scale, shift, mean, dW, acc):
    """see p3_bn_sums_from_g: G [N, 2K] fp32 from gemm_tn_ex(..., A_AFFINE_MASK2); dW [N, K] and acc [2K] are accumulated into"""
    N, K = W.shape
    check(lib().p3_bn_sums_from_g(ptr(G), G.stride(0), ptr(W), ptr(scale), ptr(shift), ptr(mean), ptr(dW), ptr(acc), N, K, stream()), "p3_bn_sums_from_g")


def gemm_tn_ex(a, b, out, b_mode, b_scale, b_shift, pair_v=None, pair_n=0, M=None):
    M_ = a.shape[0] if M is None else M
    N, K = a.shape[1], b.shape[1]
    if tuple(out.shape) != (N, K * (2 if b_mode == A_AFFINE_MASK2 else 1)) or out.dtype != torch.float32:
        raise P3Error(f"gemm_tn_ex: out must be float32 [{N}, {K * (2 if b_mode == A_AFFINE_MASK2 else 1)}], got {out.dtype} {tuple(out.shape)}")
    slabs, ns = _tn_slabs(N, K * (2 if b_mode == A_AFFINE_MASK2 else 1), a)
    check(lib().p3_gemm_tn_ex(ptr(a), ptr(b), ptr(out), M_, N, K, a.stride(0), b.stride(0),
                              out.stride(0), dt_mm(a), b_mode, ptr(b_scale), ptr(b_shift), ptr(pair_v), pair_n,
                              ptr(None), ptr(slabs), ns, stream()), "p3_gemm_tn_ex")
    return out


def row_affine_bwd(H, scale, shift, mean, acc, *, dA=None, dS=None, w4=None, N=0, transpose=False, out=None, store=True, fix=None):
    """store=False: sums only (pass 1 of the train-mode two-pass form); fix=(a, b): write dz*scale + a + b*H (pass 2, acc may be None)."""
    R, C = H.shape
    if store:
        out = out if out is not None else torch.empty_like(H)
    else:
        out = None
    fa, fb = fix if fix is not None else (None, None)
    check(lib().p3_row_affine_bwd2(ptr(dA), ptr(dS), ptr(H), ptr(scale), ptr(shift), ptr(mean), ptr(w4), ptr(out), ptr(acc), ptr(fa), ptr(fb),
                                   R, C, N, int(transpose), dt(H), stream()), "p3_row_affine_bwd")
    return out


def bn_bwd_coeffs(dscale, dshift, gamma, mean, rstd, count, training, acc=None):
    """acc = (dgamma, dbeta) fp32 [C] accumulators (the parameters' .grad views): += instead of fresh tensors (returned as None)."""
    C = gamma.shape[0]
    o = torch.empty((4, C), dtype=torch.float32, device=gamma.device)
    dg, db = (acc[0], acc[1]) if acc is not None else (o[0], o[1])
    check(lib().p3_bn_bwd_coeffs(ptr(dscale), ptr(dshift), ptr(gamma), ptr(mean), ptr(rstd), count,
                                 int(bool(training)) | (2 if acc is not None else 0), C,
                                 ptr(dg), ptr(db), ptr(o[2]), ptr(o[3]), stream()), "p3_bn_bwd_coeffs")
    return (None, None, o[2], o[3]) if acc is not None else (o[0], o[1], o[2], o[3])


def affine_fix(dH, H, a, b, ldh=None):
    """dH [R, C] (dense) += a + b * H;  H may be a strided view (row stride ldh)."""
    R, C = dH.shape
    check(lib().p3_affine_fix_ld(ptr(dH), ptr(H), ldh if ldh is not None else H.stride(0), ptr(a), ptr(b), R, C, dt(dH), stream()), "p3_affine_fix")
    return dH


def pair_bwd(dA, U, V, scale, shift, mean, B, N, acc):
    C = U.shape[1]
    dU = torch.empty((B * N, C), dtype=torch.float32, device=U.device)
    dV = torch.zeros((B * N, C), dtype=torch.float32, device=U.device)
    L = lib()
    # dV partials through a scratch slab instead of global atomics: the bf16 form always, the fp32 one in deterministic launches
    if dt(U) == BF16 or (dt(U) == F32 and det_on(U)):
        ws = workspace(L.p3_pair_bwd_workspace_bytes_dt(B, N, C, dt(U)), U.device, "pair_bwd")
        check(L.p3_pair_bwd_ws(ptr(dA), ptr(U), ptr(V), ptr(scale), ptr(shift), ptr(mean), ptr(dU), ptr(dV), ptr(acc), B, N, C,
                               dt(U), ptr(ws), stream()), "p3_pair_bwd_ws")
    else:
        check(L.p3_pair_bwd(ptr(dA), ptr(U), ptr(V), ptr(scale), ptr(shift), ptr(mean), ptr(dU), ptr(dV), ptr(acc), B, N, C, dt(U), stream()), "p3_pair_bwd")
    return dU, dV


def pair_bwd_fused(dH2, w2t, U, V, scale, shift, mean, B, N, acc):
    """conv2's input gradient + pair_bwd in one launch: dA2 = dH2 @ w2t^T never touches memory.  -> (dU, dV) fp32 [B N, 256].
    bf16 operands (csrc/pair_bwd_mma.hip), or fp32 operands inside a gemm_split scope (fp32x3: csrc/pair_bwd_x3.hip)."""
    x3 = dt(dH2) == F32 and split_now()
    want = F32 if x3 else BF16
    if any(dt(t) != want for t in (dH2, w2t, U, V)) or w2t.shape != (256, 128) or not all(t.is_contiguous() for t in (dH2, w2t, U, V)) or dH2.shape[1] != 128:
        raise P3Error("pair_bwd_fused: bf16 (or fp32 under gemm_split), contiguous dH2 [B N N, 128], w2t [256, 128], U / V [B N, 256]")
    dU = torch.empty((B * N, 256), dtype=torch.float32, device=U.device)
    dV = torch.zeros((B * N, 256), dtype=torch.float32, device=U.device)
    L = lib()
    ws = workspace(L.p3_pair_bwd_fused_workspace_bytes(B, N), U.device, "pair_bwd")
    if x3:
        check(L.p3_pair_bwd_fused_x3(ptr(dH2), ptr(w2t), ptr(U), ptr(V), ptr(scale), ptr(shift), ptr(mean), ptr(dU), ptr(dV), ptr(acc), B, N,
                                     ptr(ws), stream()), "p3_pair_bwd_fused_x3")
        return dU, dV
    check(L.p3_pair_bwd_fused(ptr(dH2), ptr(w2t), ptr(U), ptr(V), ptr(scale), ptr(shift), ptr(mean), ptr(dU), ptr(dV), ptr(acc), B, N,
                              ptr(ws), stream()), "p3_pair_bwd_fused")
    return dU, dV


def pair_stats_bwd(U, V, a, b, dU, dV, B, N):
    check(lib().p3_pair_stats_bwd(ptr(U), ptr(V), ptr(a), ptr(b), ptr(dU), ptr(dV), B, N, U.shape[1], dt(U), stream()), "p3_pair_stats_bwd")


# ------------------------------------------------------------------------------------------ FFL / *CNN tails
A_CONV3X3_AFFINE_RELU = 4


def upsample_bilinear(tokens, B, h, w, H, W, out, tok_off=1):
    """tokens [B, tok_off + h*w, C] -> out [B, H, W, ld] (writes channels 0..C-1)."""
    C = tokens.shape[-1]
    check(lib().p3_upsample_bilinear(ptr(tokens), dt(tokens), ptr(out), dt(out), B, h, w, C, H,
                                     W, out.stride(-2), tok_off, tokens.shape[1], stream()), "p3_upsample_bilinear")
    return out


def head1x1(X, ld, scale, shift, W, bias, act, post_mul, B, HW, copy_dst=None, copy_ld=0):
    n_out = W.shape[0]
    out = torch.empty((B, n_out, HW), dtype=torch.float32, device=X.device)
    check(lib().p3_head1x1(ptr(X), ld, dt(X), ptr(scale), ptr(shift), ptr(W), ptr(bias), n_out, act, post_mul,
                           ptr(out), ptr(copy_dst), copy_ld, B * HW, HW, stream()), "p3_head1x1")
    return out


def nhwc_to_nchw(X, ld, scale, shift, B, C, HW):
    out = torch.empty((B, C, HW), dtype=torch.float32, device=X.device)
    check(lib().p3_nhwc_to_nchw(ptr(X), ld, dt(X), ptr(scale), ptr(shift), ptr(out), B, C, HW, stream()), "p3_nhwc_to_nchw")
    return out


# ------------------------------------------------------------------------------------------ dropout
def rng_advance(seed):
    check(lib().p3_rng_advance(ptr(seed), stream()), "p3_rng_advance")


def dropout_apply(x, out_dtype, drop, out=None):
    """out = keep ? x / (1 - p) : 0 with the counter-based mask of (seed, site); element = (flat row, last-dim column) of x."""
    xc = x.contiguous()
    out = torch.empty(xc.shape, dtype=out_dtype, device=x.device) if out is None else out
    d = _drop(drop)
    check(lib().p3_dropout_apply(ptr(xc), dt(xc), ptr(out), dt(out), xc.numel(), xc.shape[-1], byref(d), stream()), "p3_dropout_apply")
    return out


# ------------------------------------------------------------------------------------------ FFL / *CNN tail backward
def head1x1_bwd(H, scale, shift, mean, W, out_nchw, dout_nchw, act, post_mul, B, HW):
    """-> (dHd [R,256] = dy*scale in H's dtype, acc fp32 [512 + n_out*256 + n_out] = dscale(centred) | dshift | dW | db)."""
    n_out = W.shape[0]
    R = B * HW
    dHd = torch.empty((R, 256), dtype=H.dtype, device=H.device)
    acc = torch.zeros(512 + n_out * 256 + n_out, dtype=torch.float32, device=H.device)
    check(lib().p3_head1x1_bwd(ptr(H), dt(H), ptr(scale), ptr(shift), ptr(mean), ptr(W), n_out, ptr(out_nchw), ptr(dout_nchw),
                               act, post_mul, ptr(dHd), ptr(acc), R, HW, stream()), "p3_head1x1_bwd")
    return dHd, acc


def affine_relu_bwd256(dA, H, ldh, scale, shift, mean, R, out=None):
    out = dA if out is None else out
    acc = torch.zeros(512, dtype=torch.float32, device=dA.device)
    check(lib().p3_affine_relu_bwd256(ptr(dA), ptr(H), ldh, dt(dA), ptr(scale), ptr(shift), ptr(mean), ptr(out), ptr(acc), R, stream()), "p3_affine_relu_bwd256")
    return out, acc


def pad_nhwc(src, ld_src, scale, shift, c_aff, C, Cp, B, H, W, out=None):
    """-> zero-bordered [B, H+2, W+2, Cp] copy (channels < c_aff through relu(x*scale + shift) when scale is given)."""
    if out is None:
        out = torch.empty((B, H + 2, W + 2, Cp), dtype=src.dtype, device=src.device)
    check(lib().p3_pad_nhwc(ptr(src), ld_src, dt(src), ptr(scale), ptr(shift), c_aff, C, Cp, ptr(out), B, H, W, stream()), "p3_pad_nhwc")
    return out


# ------------------------------------------------------------------------------------------ HiSup head set
def nchw_to_nhwc(x, dtype, ld=None):
    """fp32 [B, C, H, W] -> token-major [B*H*W, ld] in `dtype` (columns >= C zero)."""
    _dev(x)
    B, C, H, W = x.shape
    ld = ld or C
    out = torch.zeros((B * H * W, ld), dtype=dtype, device=x.device) if ld != C else torch.empty((B * H * W, ld), dtype=dtype, device=x.device)
    check(lib().p3_nchw_to_nhwc(ptr(x.contiguous().float()), ptr(out), ld, dt(out), B, C, H * W, stream()), "p3_nchw_to_nhwc")
    return out


def eca_gate(a1, aff1, a2, aff2, conv_w, B, HW, C):
    """sigmoid(conv1d_k(mean_hw(relu(bn(a1)) + relu(bn(a2))))) -> fp32 [B, C]; aff = (scale, shift) of the producing BatchNorm."""
    pooled = torch.empty((B, C), dtype=torch.float32, device=a1.device)
    gate = torch.empty_like(pooled)
    w = conv_w.detach().reshape(-1).float().contiguous()
    check(lib().p3_eca_gate(ptr(a1), a1.stride(0), ptr(aff1[0]), ptr(aff1[1]), ptr(a2), a2.stride(0), ptr(aff2[0]), ptr(aff2[1]), ptr(w),
                            w.numel(), ptr(pooled), ptr(gate), B, HW, C, dt(a1), stream()), "p3_eca_gate")
    return gate


def affine_relu_mix(out, a, aff_a, HW, C, gate=None, b=None, aff_b=None):
    """out[:, :C] = f(a) * gate[b(r)] + g(b): f / g = relu(x*scale + shift) when aff is given, identity otherwise (see p3_affine_relu_mix)."""
    R = a.shape[0]
    sa, ha = aff_a if aff_a is not None else (None, None)
    sb, hb = aff_b if aff_b is not None else (None, None)
    check(lib().p3_affine_relu_mix(ptr(out), out.stride(0), ptr(a), a.stride(0), ptr(sa), ptr(ha), ptr(gate), ptr(b),
                                   b.stride(0) if b is not None else 0, ptr(sb), ptr(hb), R, C, HW, dt(a),
                                   stream()), "p3_affine_relu_mix")
    return out


def upsample_bilinear_bwd(dUp, B, h, w, H, W, tok_off=1):
    """dUp [B, H, W, C] -> dtokens [B, tok_off + h*w, C] (rows before tok_off are zero)."""
    C = dUp.shape[-1]
    tmp = torch.empty((B, H, w, C), dtype=torch.float32, device=dUp.device)
    dtok = torch.zeros((B, tok_off + h * w, C), dtype=dUp.dtype, device=dUp.device)
    check(lib().p3_upsample_bilinear_bwd(ptr(dUp), dt(dUp), ptr(tmp), ptr(dtok), B, h, w, C, H, W, tok_off, tok_off + h * w, stream()), "p3_upsample_bilinear_bwd")
    return dtok


def transpose_many(src, dst, table, n_entries, total_tiles):
    check(lib().p3_transpose_many(ptr(src), ptr(dst), ptr(table), n_entries, total_tiles, stream()), "p3_transpose_many")


def attention_mask_words(B, heads, Lq, Lk, device):
    """keep-bit words the attention forward publishes for its backward (p3_attn_desc.drop_rows)."""
    return torch.empty((B * heads, (Lk + 31) // 32, Lq), dtype=torch.int32, device=device)     # [b*H + h][key word][q]


# ------------------------------------------------------------------------------------------ planes (fp32x3 ViT block; include/p3hip.h p3_gemm_x3)
class Planes:
    """An fp32-valued [rows, cols] matrix stored as hi = bf16(x) and lo = bf16(x - hi): two bf16 views with one row stride (the two halves of one
    [rows_alloc, 2 * cols] buffer).  rows_alloc rounds the row count up (64: the weight-gradient kernel walks whole 64-row steps); the tail rows are zero."""
    __slots__ = ("buf", "hi", "lo", "rows", "cols")

    def __init__(self, buf, rows, cols):
        self.buf, self.rows, self.cols = buf, rows, cols
        self.hi, self.lo = buf[:, :cols], buf[:, cols:]

    @staticmethod
    def empty(rows, cols, device, pad=64):
        ra = (rows + pad - 1) // pad * pad
        buf = torch.empty((ra, 2 * cols), dtype=torch.bfloat16, device=device)
        if ra > rows:
            buf[rows:].zero_()
        return Planes(buf, rows, cols)

    def narrow(self, cols):
        """the first `cols` columns as Planes over the same buffer (same rows and row stride)"""
        p = Planes.__new__(Planes)
        p.buf, p.rows, p.cols = self.buf, self.rows, cols
        p.hi, p.lo = self.hi[:, :cols], self.lo[:, :cols]
        return p

    @property
    def ld(self):
        return self.buf.stride(0)

    @property
    def rows_alloc(self):
        return self.buf.shape[0]


def to_planes(x, out=None, pad=64):
    """fp32 [rows, cols] (row stride free) -> Planes"""
    _dev(x)
    rows, cols = x.shape
    if out is None:
        out = Planes.empty(rows, cols, x.device, pad)
    check(lib().p3_to_planes(ptr(x), x.stride(0), ptr(out.hi), ptr(out.lo), out.ld, rows, cols, stream()), "p3_to_planes")
    return out


def to_planes_into(x, hi, lo):
    """fp32 [rows, cols] -> the given bf16 hi / lo matrices (same shape, one row stride)"""
    rows, cols = x.shape
    check(lib().p3_to_planes(ptr(x), x.stride(0), ptr(hi), ptr(lo), hi.stride(0), rows, cols, stream()), "p3_to_planes")


def from_planes(p, out=None):
    if out is None:
        out = torch.empty((p.rows, p.cols), dtype=torch.float32, device=p.buf.device)
    check(lib().p3_from_planes(ptr(p.hi), ptr(p.lo), p.ld, ptr(out), out.stride(0), p.rows, p.cols, stream()), "p3_from_planes")
    return out


class GemmX3Desc(Structure):
    _fields_ = [("M", c_int), ("N", c_int), ("K", c_int),
                ("a_hi", c_void_p), ("a_lo", c_void_p), ("lda", c_int),
                ("w_hi", c_void_p), ("w_lo", c_void_p), ("ldb", c_int),
                ("c", c_void_p), ("c_lo", c_void_p), ("ldc", c_int),
                ("bias", c_void_p), ("residual", c_void_p), ("ldr", c_int), ("act", c_int),
                ("aux", c_void_p), ("ldaux", c_int), ("mul", c_void_p), ("ldmul", c_int),
                ("tile", c_int),
                ("conv_B", c_int), ("conv_H", c_int), ("conv_W", c_int), ("conv_ci", c_int), ("conv_row0", c_int)]


_x3_cus = {}


def x3_cus(device):
    """CUs of the device the launch goes to (the 128 x 384 tile runs one workgroup per CU): queried once per device, 256 on MI355X"""
    idx = torch.device(device).index
    idx = torch.cuda.current_device() if idx is None else idx
    if idx not in _x3_cus:
        _x3_cus[idx] = int(torch.cuda.get_device_properties(idx).multi_processor_count)
    return _x3_cus[idx]


X3_RAGGED_SPLIT = [True]               # A/B switch of the ragged-round rule below


def x3_conv_row(m, H, W):
    """row of the zero-bordered image [B, H+2, W+2] that output pixel m of the unpadded [B, H, W] grid reads its centre tap from (csrc/gemm_x3.hip x3_conv_row)"""
    b, r = divmod(m, H * W)
    y, x = divmod(r, W)
    return (b * (H + 2) + y + 1) * (W + 2) + x + 1


def gemm_x3(a, w, *, bias=None, act=ACT_NONE, residual=None, aux=None, mul=None, out=None, out_planes=False, conv=None, conv_rows=None, tile=0,
            ragged=None):
    """C = epilogue((a_hi + a_lo) (w_hi + w_lo)^T).  a: Planes [M, K]; w: (hi, lo) bf16 [N, K] tensors (or Planes); out: fp32 [M, N] tensor or Planes
    (out_planes=True allocates one).
    conv = (B, H, W, Ci): 3 x 3 convolution - a is the zero-bordered planes image [B (H+2) (W+2), Ci] (pad_nhwc_planes), w is [N, (ky, kx, ci)], the output rows
    are the B H W interior pixels (conv_rows = (first, count): only these output pixels; out, residual, ... start at pixel `first`).  tile: 0 the library's rule, 1 / 2 force a tile kernel for this call; ragged: False keeps the launch whole (measurement)."""
    M, K = a.rows, a.cols
    if conv is not None:
        cB, cH, cW, cCi = conv
        if a.rows != cB * (cH + 2) * (cW + 2) or a.cols != cCi:
            raise P3Error("gemm_x3: conv needs the zero-bordered image [B (H+2) (W+2), Ci] as a")
        row0, M = (0, cB * cH * cW) if conv_rows is None else conv_rows
        K = 9 * cCi
        if row0 < 0 or M <= 0 or row0 + M > cB * cH * cW:
            raise P3Error("gemm_x3: conv_rows outside the B H W output pixels")
    w_hi, w_lo = (w.hi, w.lo) if isinstance(w, Planes) else w
    N = w_hi.shape[0]
    if w_hi.shape[1] != K or w_hi.stride(0) != w_lo.stride(0):
        raise P3Error("gemm_x3: weight planes must be [N, K] with one row stride")
    d = GemmX3Desc()
    d.M, d.N, d.K = M, N, K
    d.a_hi, d.a_lo, d.lda = a.hi.data_ptr(), a.lo.data_ptr(), a.ld
    d.w_hi, d.w_lo, d.ldb = w_hi.data_ptr(), w_lo.data_ptr(), w_hi.stride(0)
    if out is None:
        out = Planes.empty(M, N, a.buf.device) if out_planes else torch.empty((M, N), dtype=torch.float32, device=a.buf.device)
    if isinstance(out, Planes):
        d.c, d.c_lo, d.ldc = out.hi.data_ptr(), out.lo.data_ptr(), out.ld
    else:
        if out.dtype != torch.float32:
            raise P3Error("gemm_x3: out must be float32 or Planes")
        d.c, d.c_lo, d.ldc = out.data_ptr(), None, out.stride(-2)
    d.bias = bias.data_ptr() if bias is not None else None
    if residual is not None:
        d.residual, d.ldr = residual.data_ptr(), residual.stride(-2)
    d.act = act
    d.tile = tile
    if conv is not None:
        d.conv_B, d.conv_H, d.conv_W, d.conv_ci, d.conv_row0 = cB, cH, cW, cCi, row0
    if aux is not None:
        d.aux, d.ldaux = aux.data_ptr(), aux.stride(-2)
    if mul is not None:
        d.mul, d.ldmul = mul.data_ptr(), mul.stride(-2)
    def launch(dd, rows):
        ev = KTIMER.begin()
        check(lib().p3_gemm_x3(byref(dd), stream()), "p3_gemm_x3")
        if ev is not None:
            a_rows = rows if conv is None else a.rows * rows / M          # conv: the image is read once (nine taps of it from L2), not K / Ci times
            nbytes = 4.0 * (a_rows * a.cols + N * K + rows * N) + (4.0 * rows * N if residual is not None else 0) + (4.0 * rows * N if aux is not None else 0) \
                + (4.0 * rows * N if mul is not None else 0)
            KTIMER.end(ev, lib().p3_last_kernel().decode() or "gemm_x3_kernel", 2.0 * rows * N * K, nbytes)

    # A ragged last round of the 128 x 384 tile (csrc/gemm_x3.hip picks it for N > 256, K >= 1024; one workgroup per CU): M = 50 240 is 393 row tiles = a full round
    # of 256 and a round of 137 with 119 CUs idle - two round times for 1.5 rounds of work.  Whole rounds go to the big tile, the remainder to the 128 x 128 tile
    # (two workgroups per CU: 137 x 3 = 411 small tiles are ONE round of 512 slots at a third of the work each), back to back on the same stream.
    # conv: the forward of the fusion convolution (N = 384, K = 6912) stays WHOLE on the 128 x 384 tile - 746 us against 830 us split (its 136 x 3 remainder
    # tiles walk 216 slices each, longer than the half round they save) and 768 us on the small tile; its input gradient (N = 768, K = 3456: two column tiles, a
    # round is cus // 2 row tiles, 392 = 3 rounds + 8) takes the split - 688 us against 737 whole / 741 on the small tile (tools/mb_conv_planes.py,
    # profiles/fusion_conv_planes_mb.txt)
    tm = (M + 127) // 128
    cus = x3_cus(a.buf.device)
    if conv is not None and 384 < N <= 768:
        cus //= 2
    rem = tm % cus
    split_ok = X3_RAGGED_SPLIT[0] if ragged is None else ragged
    if split_ok and tile == 0 and ((conv is None and 256 < N <= 384) or (conv is not None and 384 < N <= 768)) and K >= 1024 and tm > cus \
            and 0 < rem <= (3 * cus) // 4:
        head = (tm - rem) * 128
        d2 = GemmX3Desc()
        ctypes.memmove(byref(d2), byref(d), ctypes.sizeof(d))
        d.M, d2.M = head, M - head
        if conv is not None:
            d2.conv_row0 = row0 + head           # the image stays where it is: the kernel maps its output rows from pixel `head` on
        else:
            d2.a_hi, d2.a_lo = d.a_hi + head * d.lda * 2, d.a_lo + head * d.lda * 2
        esz = 2 if isinstance(out, Planes) else 4
        d2.c = d.c + head * d.ldc * esz
        if isinstance(out, Planes):
            d2.c_lo = d.c_lo + head * d.ldc * esz
        if residual is not None:
            d2.residual = d.residual + head * d.ldr * 4
        if aux is not None:
            d2.aux = d.aux + head * d.ldaux * 4
        if mul is not None:
            d2.mul = d.mul + head * d.ldmul * 4
        d.tile, d2.tile = 2, 1               # per call (p3_gemm_x3_desc.tile): no process-wide state is touched
        launch(d, head)
        launch(d2, M - head)
        return out
    launch(d, M)
    return out


def gemm_tn_x3(a, b, out=None, colsum_out=None):
    """out[N, K] (+)= (a_hi + a_lo)[M, N]^T (b_hi + b_lo)[M, K]; a, b: Planes with the same (64-padded, zero-tailed) row count; fp32 out, zero-filled when not given"""
    if a.rows_alloc != b.rows_alloc:
        raise P3Error("gemm_tn_x3: operands must share the padded row count")
    M, N, K = a.rows_alloc, a.cols, b.cols
    if out is None:
        out = torch.zeros((N, K), dtype=torch.float32, device=a.buf.device)
    slabs, ns = _tn_slabs(N, K, out)
    ev = KTIMER.begin()
    check(lib().p3_gemm_tn_x3(ptr(a.hi), ptr(a.lo), a.ld, ptr(b.hi), ptr(b.lo), b.ld, ptr(out), out.stride(0), M, N, K,
                              ptr(colsum_out), ptr(slabs), ns, stream()), "p3_gemm_tn_x3")
    if ev is not None:
        KTIMER.end(ev, lib().p3_last_kernel().decode() or "gemm_tn_x3_kernel<4>", 2.0 * a.rows * N * K, float(4 * a.rows * (N + K) + N * K * 4))
    return out


def pad_nhwc_planes(src, B, H, W, pre=None, a=None, b=None, guard=None, cols=None):
    """fp32 token-major map [B*H*W, C] (row stride free) -> Planes of the zero-bordered image [B (H+2) (W+2), C]: a view into a buffer that also holds `guard`
    zero rows (default W + 3: one padded row + 1, what the shifted rows of gemm_tn_x3_conv reach) in front of and behind the 64-padded rows - written in the same
    pass.  pre, a, b: the value split is src + a + b * pre (affine_fix's arithmetic; src itself is not written).  cols >= C: zero columns up to
    that width (Planes.narrow gives the C-column view back)."""
    _dev(src)
    M, C = src.shape
    if M != B * H * W:
        raise P3Error("pad_nhwc_planes: src must be [B*H*W, C]")
    guard = W + 3 if guard is None else guard
    R = B * (H + 2) * (W + 2)
    Ra = (R + 63) // 64 * 64
    Cp = C if cols is None else cols
    full = torch.empty((Ra + 2 * guard, 2 * Cp), dtype=torch.bfloat16, device=src.device)
    out = Planes(full[guard:guard + Ra], R, Cp)
    ev = KTIMER.begin()
    check(lib().p3_pad_nhwc_planes(ptr(src), src.stride(0), ptr(pre), pre.stride(0) if pre is not None else 0, ptr(a), ptr(b), ptr(out.hi), ptr(out.lo), out.ld,
                                   B, H, W, C, Cp, guard, Ra, stream()), "p3_pad_nhwc_planes")
    if ev is not None:
        KTIMER.end(ev, "pad_nhwc_planes_kernel<fix>" if pre is not None else "pad_nhwc_planes_kernel", (2.0 if pre is not None else 0.0) * M * C,
                   4.0 * M * C * (2 if pre is not None else 1) + 4.0 * (Ra + 2 * guard) * Cp)
    return out


def gemm_tn_x3_conv(a, b, Pw, out=None):
    """weight gradient of a 3 x 3 convolution in one launch: out[N, 9 Ci] (+)= sum over the nine taps of a^T (b shifted by the tap's row offset).  a: Planes of the
    zero-bordered output gradient [R, N]; b: Planes of the zero-bordered input image [R, Ci] from pad_nhwc_planes with its default guard rows (the kernel reads
    Pw + 1 rows in front of and behind b); Pw = W + 2.  fp32 out, zero-filled when not given."""
    if a.rows_alloc != b.rows_alloc:
        raise P3Error("gemm_tn_x3_conv: operands must share the padded row count")
    base = b.buf._base if b.buf._base is not None else b.buf
    lead = (b.buf.data_ptr() - base.data_ptr()) // (base.stride(0) * 2)
    if base.stride(0) != b.ld or lead < Pw + 1 or base.shape[0] - lead - b.rows_alloc < Pw + 1:
        raise P3Error("gemm_tn_x3_conv: b needs Pw + 1 guard rows in front of and behind it (pad_nhwc_planes)")
    M, N, Ci = a.rows_alloc, a.cols, b.cols
    if out is None:
        out = torch.zeros((N, 9 * Ci), dtype=torch.float32, device=a.buf.device)
    slabs, ns = _tn_slabs(N, 9 * Ci, out)
    ev = KTIMER.begin()
    check(lib().p3_gemm_tn_x3_conv(ptr(a.hi), ptr(a.lo), a.ld, ptr(b.hi), ptr(b.lo), b.ld, ptr(out), out.stride(0), M, N, Ci, Pw, ptr(slabs), ns, stream()),
          "p3_gemm_tn_x3_conv")
    if ev is not None:
        KTIMER.end(ev, (lib().p3_last_kernel().decode() or "gemm_tn_x3_wide_kernel<4>") + "/conv", 2.0 * a.rows * N * 9 * Ci, float(4 * a.rows * (N + Ci) + N * 9 * Ci * 4))
    return out


def col_stats(x, sums=None):
    """[column sums | column sums of squares] of fp32 x [M, N] -> fp32 [2 N]; fixed summation order (the same bits on every run)"""
    _dev(x)
    M, N = x.shape
    if sums is None:
        sums = torch.empty(2 * N, dtype=torch.float32, device=x.device)
    nfl = 1024 * 2 * N
    ws = workspace(nfl * 4, x.device, "col_stats")
    ev = KTIMER.begin()
    check(lib().p3_col_stats(ptr(x), x.stride(0), M, N, ptr(sums), ptr(ws), nfl, stream()), "p3_col_stats")
    if ev is not None:
        KTIMER.end(ev, "col_stats_kernel", 3.0 * M * N, 4.0 * M * N)
    return sums


def layernorm_planes(x, gamma, beta, eps, out=None, save_stats=True):
    """LayerNorm of the fp32 rows of x [rows, cols] written as Planes (+ mean, rstd)"""
    rows, cols = x.shape
    if out is None:
        out = Planes.empty(rows, cols, x.device)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device) if save_stats else None
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device) if save_stats else None
    check(lib().p3_layernorm_planes(ptr(x), ptr(gamma), ptr(beta), ptr(out.hi), ptr(out.lo), rows, cols, x.stride(0), out.ld, eps,
                                    ptr(mean), ptr(rstd), stream()), "p3_layernorm_planes")
    return out, mean, rstd


def layernorm_bwd_planes(dy, x, gamma, mean, rstd, dres, dgamma, dbeta, out=None, park=False):
    """dx (fp32) = LayerNorm backward (+ dres); the same values also as Planes; dgamma / dbeta are accumulated into"""
    rows, cols = x.shape
    dx = torch.empty_like(x)
    if out is None:
        out = Planes.empty(rows, cols, x.device)
    L = lib()
    park = park and dgamma is not None and param_reduce_arena()
    if park:
        L.p3_reduce_defer_enable(1)
    try:
        check(L.p3_layernorm_bwd_planes(ptr(dy), ptr(x), ptr(gamma), ptr(mean), ptr(rstd), ptr(dres), ptr(dx), ptr(out.hi), ptr(out.lo), out.ld,
                                        ptr(dgamma), ptr(dbeta), rows, cols, stream()), "p3_layernorm_bwd_planes")
    finally:
        if park:
            L.p3_reduce_defer_enable(0)
    return dx, out
