"""The plain GEMM entry points (csrc/gemm.hip: dcn_gemm_nt / _nn / _tn / _nt_batched) against the fp64 product of the same fp32
operands: every tile, pipe and argument, at the cases of gemm_cases.py and at each case's own tolerance (util.gemm_tol of the CPU
fp32 error of the same case, computed at run time).  Every output is a view of a wider sentinel-filled buffer whose other rows and
columns must come back bitwise untouched.  test_gemm_host.py shows that the comparator bites at exactly these cases."""
import functools

import pytest
import torch

import gemm_cases as G
from util import gemm_err, gemm_tol, rand, tuning

pytestmark = pytest.mark.gpu

SENTINEL = -777.25


@functools.lru_cache(maxsize=None)
def _reference(case):
    """(inputs, fp64 result, fp64 scale, tolerance) of a case: computed once on the CPU, shared by the runs of the case, never written"""
    x = G.make_inputs(case)
    ref, scale = G.evaluate(x, torch.float64), G.scale64(x)
    r32 = gemm_err(G.evaluate(x, torch.float32), ref, scale)
    return x, ref, scale, r32


def _ld4(n):
    return (n + 3) // 4 * 4 + 8


def _out_view(dev, m, n, c_old=None, batch=None):
    """An (m, n) view (per batch item) of a wider, taller sentinel-filled buffer, holding c_old where the case accumulates"""
    shape = (m + 2, _ld4(n)) if batch is None else (batch, m + 2, _ld4(n))
    buf = torch.full(shape, SENTINEL, dtype=torch.float32, device=dev)
    out = buf[..., :m, :n]
    if c_old is not None:
        out.copy_(c_old)
    return buf, out


def _untouched(buf, m, n):
    keep = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    keep[..., :m, :n] = False
    rest = buf[keep]
    return bool((rest.view(torch.int32) == torch.tensor(SENTINEL).view(torch.int32).item()).all())


def _column_slice(t, off, extra, fill_seed):
    """t (rows, c) as columns [off, off + c) of a wider matrix of other finite values: the row stride exceeds c"""
    rows, c = t.shape
    wide = rand(rows, c + extra, seed=fill_seed).to(t.device)
    wide[:, off:off + c] = t
    return wide[:, off:off + c]


def _pipe(case, precision0=False):
    if precision0:
        return "fp32"
    if case.kind in ("nt", "nn"):
        return "split" if case.m >= 1024 and case.n > 64 else "fp32"
    if case.kind == "tn":
        return "split" if case.m >= 128 and case.n >= 128 and case.k >= 1024 else "fp32"
    return "fp32"


def _check(case, out, buf, precision0=False):
    x, ref, scale, r32 = _reference(case)
    got = out.detach().cpu()
    if case.kind != "ntb":
        got = got.unsqueeze(0)
    err, tol = gemm_err(got, ref, scale), gemm_tol(r32)
    print(f"GEMMERR {_pipe(case, precision0)} {case}{' precision0' if precision0 else ''} err {err:.3e} r32 {r32:.3e} "
          f"ratio {err / max(r32, 2.0 ** -24):.2f}")
    assert _untouched(buf, case.m, case.n), f"{case}: wrote outside its (M, N) view"
    assert err <= tol, f"{case}: err {err:.3e} > tol {tol:.3e} (CPU fp32 {r32:.3e})"


def _run_nt(case, dev):
    from dcnet_amd import ops
    x = _reference(case)[0]
    a, b = x["a"][0].to(dev), x["b"][0].to(dev)
    if case.variant == "aslice":
        a = _column_slice(a, 16, 32, G.seed_of(case) + 5)
        assert a.stride(0) > case.k
    bias = None if x["bias"] is None else x["bias"].to(dev)
    res = None
    if x["res"] is not None:                 # its own row stride, different from the output's
        res = _column_slice(x["res"].to(dev), 0, 13, G.seed_of(case) + 6)
    buf, out = _out_view(dev, case.m, case.n, x["c_old"])
    assert res is None or res.stride(0) != out.stride(0)
    ops.gemm_nt(a, b, bias, ops.ACT_LEAKY if x["act"] else ops.ACT_NONE, residual=res, out=out, accumulate=x["c_old"] is not None)
    return out, buf


@pytest.mark.parametrize("case", G.NT_CASES, ids=str)
def test_gemm_nt(dev, case):
    """C (+)= act(A . B^T + bias) + residual, the formula of the csrc/gemm.hip comment; ACT_LEAKY has slope 0 on this entry"""
    _check(case, *_run_nt(case, dev))


@pytest.mark.parametrize("case", [c for c in G.NT_CASES if c.m >= 1024], ids=str)
def test_gemm_nt_fp32_pipe_on_the_split_shapes(dev, case):
    with tuning({"precision": 0}):
        out, buf = _run_nt(case, dev)
    _check(case, out, buf, precision0=True)


@pytest.mark.parametrize("case", G.NN_CASES, ids=str)
def test_gemm_nn(dev, case):
    from dcnet_amd import ops
    x = _reference(case)[0]
    s = G.seed_of(case)
    kv = case.kvalid or case.k
    a = rand(case.m, case.k, seed=s + 7).to(dev)              # columns >= kvalid: other finite values, multiplied by rows read as zero
    a[:, :kv] = x["a"][0].to(dev)
    b = torch.full((case.k, case.n), 1000.0, device=dev)      # rows >= kvalid must not be read
    b[:kv] = x["b"][0].t().to(dev)
    if case.variant in ("bslice", "kvacc"):
        b = _column_slice(b, 32, 64, s + 8)
        assert b.stride(0) > case.n
    buf, out = _out_view(dev, case.m, case.n, x["c_old"])
    ops.gemm_nn(a, b, out=out, accumulate=x["c_old"] is not None, kvalid=case.kvalid)
    _check(case, out, buf)


@pytest.mark.parametrize("case", G.TN_CASES, ids=str)
def test_gemm_tn(dev, case):
    from dcnet_amd import ops
    x = _reference(case)[0]
    s = G.seed_of(case)
    # [K][M], [K][N]; freshly allocated, so that a single row (K = 1) still carries its row stride
    a = torch.empty(case.k, case.m, device=dev).copy_(x["a"][0].t())
    b = torch.empty(case.k, case.n, device=dev).copy_(x["b"][0].t())
    if case.variant == "slices":
        a, b = _column_slice(a, 8, 16, s + 7), _column_slice(b, 4, 12, s + 8)
        assert a.stride(0) > case.m and b.stride(0) > case.n
    buf, out = _out_view(dev, case.m, case.n, x["c_old"])
    ops.gemm_tn(a, b, out=out, accumulate=x["c_old"] is not None)
    _check(case, out, buf)


@pytest.mark.parametrize("case", G.NTB_CASES, ids=str)
def test_gemm_nt_batched(dev, case):
    from dcnet_amd import ops
    x = _reference(case)[0]
    pairs = torch.stack([x["a"], x["b"]], 1).to(dev)           # (batch, 2, M, K): both operands strided selections of one tensor
    a, b = pairs[:, 0], pairs[:, 1]
    assert not a.is_contiguous() or case.batch == 1
    buf, out = _out_view(dev, case.m, case.n, batch=case.batch)
    ops.gemm_nt_batched(a, b, out=out)
    _check(case, out, buf)


def _rejected(dev, call, m, n, batch=None):
    from dcnet_amd import ops
    buf, out = _out_view(dev, m, n, batch=batch)
    with pytest.raises(ops.DcnError):
        call(out)
    torch.cuda.synchronize()
    assert bool((buf.view(torch.int32) == torch.tensor(SENTINEL).view(torch.int32).item()).all()), "a rejected call wrote its output"


def test_rejections_leave_the_output_untouched(dev):
    from dcnet_amd import ops
    r = lambda *s: rand(*s, seed=5).to(dev)
    _rejected(dev, lambda o: ops.gemm_nt(r(8, 40), r(8, 40), out=o), 8, 8)                          # K = 40
    off = r(8 * 32 + 1)[1:].view(8, 32)                                                          # a view offset by one float
    _rejected(dev, lambda o: ops.gemm_nt(off, r(8, 32), out=o), 8, 8)
    _rejected(dev, lambda o: ops.gemm_nt(r(8, 32), off, out=o), 8, 8)
    _rejected(dev, lambda o: ops.gemm_nn(off, r(32, 8), out=o), 8, 8)
    _rejected(dev, lambda o: ops.gemm_nt(r(8, 34)[:, :32], r(8, 32), out=o), 8, 8)                  # lda = 34
    _rejected(dev, lambda o: ops.gemm_nn(r(8, 32), r(32, 6), out=o), 8, 6)                          # N = 6 (NN)
    _rejected(dev, lambda o: ops.gemm_tn(r(32, 6), r(32, 8), out=o), 6, 8)                          # M = 6 (TN)
    narrow = lambda o: ops.gemm_nt_batched(r(2, 8, 32), r(2, 8, 32), out=torch.as_strided(o, (2, 8, 8), (o.stride(0), 4, 1)))
    _rejected(dev, narrow, 8, 8, batch=2)                                                        # ldc = 4 < N = 8
