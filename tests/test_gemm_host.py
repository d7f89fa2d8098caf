"""The GEMM comparator (util.gemm_err) and proof that it bites: at every case of the tables in gemm_cases.py, at that case's own
tolerance, five deliberately wrong references are told apart from a correct fp32 result.  CPU only."""
import pytest
import torch

import gemm_cases as G
from util import gemm_err, gemm_tol


def test_tables_cover_the_required_values():
    nt = G.NT_CASES
    assert {c.m for c in nt} >= {1, 7, 127, 128, 129, 1023, 1024, 1030, 16400}
    assert {c.n for c in nt} == {4, 15, 32, 36, 64, 68, 128, 132, 252} and {c.k for c in nt} == {32, 96, 512}
    tile = lambda n: 0 if n <= 32 else (1 if n <= 64 else 2)
    for t in range(3):
        mine = [c for c in nt if tile(c.n) == t]
        assert any(c.m < 1024 for c in mine) and any(c.m >= 1024 for c in mine)
        assert {c.variant for c in mine} == {"plain", "bias", "bias_relu", "res", "acc", "all", "aslice"}, t
    assert {c.n for c in G.NN_CASES} == {4, 64, 68, 256}
    assert {(c.m, c.n) for c in G.TN_CASES if c.k == 40} == {(m, n) for m in (4, 64, 132) for n in (4, 64, 132)}
    assert {c.k for c in G.TN_CASES if (c.m, c.n, c.variant) == (128, 128, "plain")} == {1, 31, 32, 33, 1000, 1024, 1056}
    assert len({str(c) for c in G.ALL_CASES}) == len(G.ALL_CASES)


def test_gemm_err_is_per_element_relative_and_exact_at_zero_scale():
    ref = torch.tensor([[1000.0, 1e-3]], dtype=torch.float64)
    scale = ref.abs()
    out = ref.clone(); out[0, 1] += 1e-6              # 1e-3 relative in the small element; 1e-9 of the row's maximum
    assert abs(gemm_err(out, ref, scale) - 1e-3) < 1e-9
    ref0 = torch.zeros(1, 2, dtype=torch.float64)
    assert gemm_err(ref0, ref0, ref0) == 0.0
    assert gemm_err(torch.tensor([[0.0, 1e-30]]), ref0, ref0) == float("inf")
    assert gemm_err(torch.tensor([[float("nan"), 0.0]]), ref0, torch.ones(1, 2)) == float("inf")


@pytest.mark.parametrize("case", G.ALL_CASES, ids=str)
def test_wrong_references_fail_at_the_case_tolerance(case):
    x = G.make_inputs(case)
    ref, scale = G.evaluate(x, torch.float64), G.scale64(x)
    out32 = G.evaluate(x, torch.float32)              # stands in for a correct kernel
    r32 = gemm_err(out32, ref, scale)
    tol = gemm_tol(r32)
    assert 0 < r32 <= 16 * 2.0 ** -24, f"{case}: CPU fp32 error {r32:.3e}"
    applied = 0
    for wrong in G.WRONG:
        bad = G.evaluate(x, torch.float64, wrong)
        if bad is None:             # the case has no such argument
            continue
        applied += 1
        err = gemm_err(out32, bad, scale)
        assert err > tol, f"{case}: wrong reference '{wrong}' passes, err {err:.3e} <= tol {tol:.3e} (r32 {r32:.3e})"
    assert applied >= 2
