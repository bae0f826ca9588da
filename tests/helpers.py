"""Shared helpers for the parity tests (oracle side only: fixtures + tolerances)."""
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    z = np.load(os.path.join(GOLD, name), allow_pickle=False)
    data, weights = {}, {}
    for k in z.files:
        t = torch.from_numpy(z[k])
        if k.startswith("w::"):
            weights[k[3:]] = t
        else:
            data[k] = t
    return data, weights


# Margin audit ("audit every test ... for margin < 3x of its tolerance"): P3_TOL_AUDIT=k multiplies every measured error by k, so
# one run of the suite without -x lists exactly the comparisons whose margin is below k (profiles/r03_margin_audit.txt).  Default 1.
AUDIT = float(os.environ.get("P3_TOL_AUDIT", "1"))


def rel_err(a, b):
    """max |a-b| / max|b|  (the 'within 1e-3 rel' metric of BASELINE.json north_star)."""
    a, b = a.double(), b.double()
    return AUDIT * float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def l2_err(a, b, floor=0.0):
    """||a-b|| / max(||b||, floor): robust to the isolated ReLU-mask flips that dominate max-abs metrics of gradients."""
    a, b = a.double(), b.double()
    return AUDIT * float((a - b).norm() / max(float(b.norm()), floor, 1e-30))


def _slices(t, dim):
    """t as [slices, elements]: one row per index of `dim` (an int or a tuple of dims)"""
    dims = (dim,) if isinstance(dim, int) else tuple(dim)
    dims = tuple(d % t.dim() for d in dims)
    rest = [d for d in range(t.dim()) if d not in dims]
    n = 1
    for d in dims:
        n *= t.shape[d]
    return t.permute(*dims, *rest).reshape(n, -1)


def block_err(got, ref, dim):
    """rel_err per slice along `dim`: max over the slices of max|got - ref| / max|ref| inside the slice.  The largest entry of the tensor no longer sets the
    yardstick of a small row, column or head.  A slice whose reference is all zero must be zero exactly (anything else counts as infinite)."""
    g, r = _slices(got.double(), dim), _slices(ref.double(), dim)
    d, m = (g - r).abs().amax(1), r.abs().amax(1)
    e = torch.where(m > 0, d / m.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
    return AUDIT * float(e.max())


def spread(ref0, dim):
    """max|ref0| / min over the slices of max|slice|, from the float64 reference of the UNGRADED problem: a slice's own maximum is smaller than the tensor's by at
    most this factor, so a per-tensor tolerance t becomes the per-slice tolerance t * spread - the only widening a per-slice bound gets"""
    m = _slices(ref0.double(), dim).abs().amax(1)
    return float(m.max() / m.min())


def elem_err(got, ref, floor=1e-2):
    """max |a-b| / max(|b|, floor * max|b|): element-wise relative error with the denominator floored at 1 % of the largest entry (the figure bench.py prints as
    logits_rel_elementwise)"""
    a, b = got.double(), ref.double()
    return AUDIT * float(((a - b).abs() / b.abs().clamp_min(floor * float(b.abs().max()))).max())


def grade(n, step=3, period=12):
    """factors 2^-(step * (i mod period)), i < n, float32 (smallest 2^-33 by default).  Multiplying by them is exact in fp32 and bf16 and commutes with
    round-to-nearest-even and with the hi / lo plane split; row and column grading together stay above 2^-66, so the lo planes stay normal numbers."""
    return torch.pow(2.0, -(step * (torch.arange(n) % period)).double()).float()
