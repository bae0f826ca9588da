"""What the graded-input metrics of tests/helpers.py can and cannot see, shown on a CPU emulation of the fp32x3 product (hi hi + hi lo + lo hi on bf16 planes,
fp32 accumulation) at (129, 136, 64) with rows and / or columns scaled by 2^-(3 (i mod 12)):

  * the correct product is bit-equal to the ungraded product times the factors (the property tests/test_graded_accuracy_gpu.py asserts of the kernels);
  * a planted magnitude-dependent defect - the lo plane of A dropped wherever |a| < 2^-12 - passes the per-tensor rel_err < 1e-5 of the suite
    and fails the per-row block_err < 1e-5 * spread."""
import pytest
import torch

from tests.helpers import block_err, elem_err, grade, rel_err, spread

M, N, K = 129, 136, 64
TOL = 1e-5                    # the planes kernels' tolerance (test_gemm_fp32_operands_as_bf16x3)


def _planes(x):
    hi = x.bfloat16().float()
    return hi, (x - hi).bfloat16().float()


def _x3(a, w, broken=False):
    ah, al = _planes(a)
    wh, wl = _planes(w)
    if broken:
        al = torch.where(a.abs() < 2.0 ** -12, torch.zeros_like(al), al)           # the planted defect
    return ah @ wh.t() + ah @ wl.t() + al @ wh.t()


@pytest.fixture(scope="module")
def problem():
    g = torch.Generator().manual_seed(0)
    a0, w0 = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.1
    return a0, w0, _x3(a0, w0), a0.double() @ w0.double().t()


def _graded(a0, w0, how):
    r, c = grade(M)[:, None], grade(N)[:, None]
    if how == "rows":
        return a0 * r, w0, r
    if how == "cols":
        return a0, w0 * c, c.t()
    return a0 * r, w0 * c, r * c.t()


def test_grade_factors():
    f = grade(40)
    assert f.dtype == torch.float32 and float(f.min()) == 2.0 ** -33 and float(f.max()) == 1.0
    assert torch.equal(f[:12], f[12:24]) and float(f[1]) == 0.125
    x = torch.randn(40, generator=torch.Generator().manual_seed(1))
    assert torch.equal((x * f).bfloat16().float(), x.bfloat16().float() * f)       # commutes with the rounding ...
    h0, l0 = _planes(x)
    h1, l1 = _planes(x * f)
    assert torch.equal(h1, h0 * f) and torch.equal(l1, l0 * f)                     # ... and with the plane split
    assert float(l1[l1 != 0].abs().min()) > 2.0 ** -126                            # lo planes stay normal


@pytest.mark.parametrize("how", ["rows", "cols", "both"])
def test_correct_product_is_bit_equivariant(problem, how):
    a0, w0, c0, _ = problem
    a, w, s = _graded(a0, w0, how)
    assert torch.equal(_x3(a, w), c0 * s)


def test_planted_defect_passes_rel_err_and_fails_block_err(problem):
    a0, w0, c0, ref0 = problem
    a, w, s = _graded(a0, w0, "rows")
    ref = a.double() @ w.double().t()
    rho = spread(ref0, 0)
    good, bad = _x3(a, w), _x3(a, w, broken=True)
    print(f"spread {rho:.2f}; correct: rel_err {rel_err(good, ref):.2e} block_err {block_err(good, ref, 0):.2e}; "
          f"defect: rel_err {rel_err(bad, ref):.2e} block_err {block_err(bad, ref, 0):.2e}; bound {TOL * rho:.2e}")
    assert rho < 4
    assert rel_err(good, ref) < TOL and block_err(good, ref, 0) < TOL * rho
    assert rel_err(bad, ref) < TOL                        # today's metric does not see the defect ...
    assert not block_err(bad, ref, 0) < TOL * rho         # ... the per-row one does
    assert block_err(bad, ref, 0) > 1e-3


def test_block_err_and_elem_err_definitions():
    ref = torch.tensor([[4.0, -2.0], [0.0, 0.0], [1e-6, 2e-6]], dtype=torch.float64)
    got = ref.clone()
    assert block_err(got, ref, 0) == 0.0
    got[2, 1] = 3e-6
    assert block_err(got, ref, 0) == pytest.approx(0.5) and rel_err(got, ref) < 1e-6
    assert block_err(got, ref, 1) == pytest.approx(1e-6 / 2.0)
    got[1, 0] = 1e-30                                     # an all-zero slice must be zero exactly
    assert block_err(got, ref, 0) == float("inf")
    assert spread(torch.tensor([[4.0, 1.0], [0.5, -2.0]]), 0) == 2.0
    r = torch.tensor([100.0, 1.0, 0.01])
    assert elem_err(r + torch.tensor([0.0, 0.01, 0.01]), r) == pytest.approx(0.01)          # the floor (1.0) divides the error of the smallest entry
    t = torch.zeros(2, 3, 4, 5)
    t[1, :, 2] = 1.0
    assert block_err(t, t, (0, 2)) == 0.0 and block_err(t * 2, t, (0, 2)) == pytest.approx(1.0)
