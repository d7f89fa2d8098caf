"""The kernels of csrc/sample.hip (the two correspondence-sampling heads and the device sampler), each through its dcnet_amd.ops wrapper
(or lib() where the wrapper computes its own inputs or cannot express the case) against the references of tests/sample_ref.py over the
case tables of tests/sample_cases.py.  Selections, gathers, the arg-max, the sampler's tables and the pure fp32 sums are compared bit
for bit; the normalisations, the conv map and the two projected gradients per element in fp64, relative to what was summed into the
element.  test_sample_ref_host.py shows on the CPU that these inputs tell twenty-four wrong variants from the right answer.  Every
kernel is launched twice and must repeat itself bitwise; calls with bad arguments must raise before anything is launched."""
import pytest
import torch

import sample_cases as SC
import sample_ref as SR
from dcnet_amd import ops
from dcnet_amd.lib import lib

pytestmark = pytest.mark.gpu
U = SR.U
F32 = SR.F32


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(xs, ys):
    return all(x.shape == y.shape and torch.equal(_bits(x), _bits(y)) for x, y in zip(xs, ys))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check(kernel, name, got, ref, ref32):
    """Every (value, scale) key of the reference per element against its scale, exact where the scale is 0.  Prints one SAMPLEFIG line per
    key and fails after all of them."""
    bad = []
    for k, r in ref.items():
        if not isinstance(r, tuple) or k not in got:
            continue
        r32, ex32 = SR.err_units(ref32[k][0], r[0], r[1])
        assert ex32, (kernel, name, k)
        err, exact = SR.err_units(got[k].cpu(), r[0], r[1])
        print(f"SAMPLEFIG {kernel} {name} {k}: err {err / U:.2f} u, r32 {r32 / U:.2f} u, ratio {err / max(r32, U):.2f}, exact {exact}")
        if not exact or not err <= SC.sample_tol(r32):
            bad.append((k, err / U, r32 / U, exact))
    assert not bad, (kernel, name, bad)


# ---- K9 forward: selection and gathers, exact -----------------------------------------------------------------------------------------
def _k9_fwd(case, dev):
    """lib().k9_fwd on the case's constructed cmap.  Empty tensors (neg_n == 0) have no address: one-element stand-ins are passed."""
    i = SC.k9_inputs(case)
    k, m = case.top_k, case.neg_n
    index = torch.full((case.pairs, k), -7, dtype=torch.int64, device=dev); neg_idx = torch.full((case.pairs, k, max(m, 1)), -7, dtype=torch.int64, device=dev)
    fill = float("nan")                                         # a row the kernel leaves out stays NaN and fails the comparison
    frame = torch.full((case.pairs, k, case.e), fill, device=dev); corr = torch.full_like(frame, fill)
    negf = torch.full((case.pairs, k, max(m, 1), case.e), fill, device=dev)
    cm, fv = i.cmap.to(dev), i.fv.to(dev)
    raw = (i.raw if m else torch.zeros(case.pairs, k, 1, dtype=torch.int64)).to(dev)
    lib().k9_fwd(cm.data_ptr(), fv.data_ptr(), raw.data_ptr(), case.pairs, case.hw, case.e, k, m, index.data_ptr(),
                 neg_idx.data_ptr(), frame.data_ptr(), corr.data_ptr(), negf.data_ptr(), _stream())
    return dict(index=index, neg_idx=neg_idx[:, :, :m], frame=frame, corr=corr, negf=negf[:, :, :m])


@pytest.mark.parametrize("case", SC.K9_CASES, ids=str)
def test_k9_select_and_gather_edges(dev, case):
    ref = SC.k9_refs(case)
    got = _k9_fwd(case, dev)
    for k in ("index", "neg_idx", "frame", "corr", "negf"):
        assert _same([got[k]], [ref[k]]), (str(case), k, got["index"].cpu().tolist() if k == "index" else None, ref["index"].tolist() if k == "index" else None)
    again = _k9_fwd(case, dev)
    assert _same(list(again.values()), list(got.values()))


# ---- K9 backward: fp32 sums in list order, exact -------------------------------------------------------------------------------------
def _k9_bwd(case, dev):
    i = SC.k9_bwd_inputs(case)
    d = lambda t: t.to(dev)
    if case.neg_n:
        return ops.k9_bwd(d(i.index), d(i.neg_idx), d(i.d_frame), d(i.d_corr), d(i.d_neg), case.hw)
    dfv = torch.full((2 * case.pairs, case.hw, case.e), float("nan"), device=dev)          # the wrapper has no address for empty lists
    one_i = torch.zeros(1, dtype=torch.int64, device=dev); one_f = torch.zeros(1, device=dev)
    index, d_frame, d_corr = d(i.index), d(i.d_frame), d(i.d_corr)
    lib().k9_bwd(index.data_ptr(), one_i.data_ptr(), d_frame.data_ptr(), d_corr.data_ptr(), one_f.data_ptr(), case.pairs, case.hw, case.e,
                 case.top_k, 0, dfv.data_ptr(), _stream())
    return dfv


@pytest.mark.parametrize("case", SC.KB_CASES, ids=str)
def test_k9_bwd_sums_keep_list_order(dev, case):
    i = SC.k9_bwd_inputs(case)
    r64, r32 = SR.k9_bwd(i.index, i.neg_idx, i.d_frame, i.d_corr, i.d_neg, case.hw)
    got = _k9_bwd(case, dev)
    print(f"SAMPLEFIG k9_bwd {case}: max |got - fp64| {float((got.cpu().double() - r64).abs().max()):.3e}, bitwise {_same([got], [r32])}")
    assert _same([got], [r32])
    assert _same([_k9_bwd(case, dev)], [got])


# ---- colnorm forward / backward ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.CN_CASES, ids=str)
def test_colnorm_edges(dev, case):
    i = SC.colnorm_inputs(case)
    v, dq = i.v.to(dev), i.dq.to(dev)
    extra = None if i.extra is None else i.extra.to(dev)
    vit, cn = ops.colnorm_fwd(v)
    dv = ops.colnorm_bwd(vit, cn, dq, extra, case.n_extra)
    fwd = (vit.cpu(), cn.cpu())
    ref, ref32 = SC.colnorm_refs(case, fwd=fwd), SC.colnorm_refs(case, F32, fwd=fwd)
    _check("colnorm", case, dict(vit=vit, cnorm=cn, dv=dv), ref, ref32)
    if case.zero:
        assert bool((vit[0, :, 1] == 0).all()) and float(cn[0, 1]) == 0.0
        g = i.dq[0, :, 1] + (i.extra[:, 1] if i.extra is not None and case.n_extra == 0 else 0.0)
        assert float((dv[0, :, 1].cpu().double() - g.double() / 1e-12).abs().max()) <= 4 * U * 1e12 * float(g.abs().max())   # g / eps
    vit2, cn2 = ops.colnorm_fwd(v)
    assert _same([vit2, cn2, ops.colnorm_bwd(vit, cn, dq, extra, case.n_extra)], [vit, cn, dv])


# ---- lagnorm ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.LN_CASES, ids=str)
def test_lagnorm_edges(dev, case):
    ctx = SC.lagnorm_inputs(case).ctx.to(dev)
    lag, ln = ops.lagnorm_fwd(ctx)
    _check("lagnorm_fwd", case, dict(lag=lag, lnorm=ln), SC.lagnorm_refs(case), SC.lagnorm_refs(case, F32))
    assert bool(torch.isfinite(lag).all()) and bool(torch.isfinite(ln).all())            # an odd channel (1e30) read would overflow the sum
    if case.zero:
        assert bool((lag[0, :, 1] == 0).all()) and float(ln[0, 1]) == 0.0
    assert _same(ops.lagnorm_fwd(ctx), (lag, ln))


# ---- crossmap ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.CM_CASES, ids=str)
def test_crossmap_edges(dev, case):
    i = SC.crossmap_inputs(case)
    lag, vit, w, b = i.lag.to(dev), i.vit.to(dev), i.w.to(dev), i.b.to(dev)
    cols, lv = ops.crossmap(lag, vit, w, b, want_map=True)
    ref, ref32 = SC.crossmap_refs(case), SC.crossmap_refs(case, F32)
    _check("crossmap", case, dict(lvmap=lv), ref, ref32)
    assert torch.equal(cols.cpu(), ref["cols"]), (str(case), int((cols.cpu() != ref["cols"]).sum()))       # every column: none is excluded
    if case.plant == "tie":
        assert _same([lv[:, SC.TIE_A]], [lv[:, SC.TIE_B]])
    if case.plant == "zero":
        assert _same([lv], [torch.full_like(lv, 0.25)]) and bool((cols == 0).all())
    cols2, lv2 = ops.crossmap(lag, vit, w, b, want_map=True)
    assert _same([cols2, lv2, ops.crossmap(lag, vit, w, b)[0]], [cols, lv, cols])


# ---- k14_gather, k14_negscatter, k14_dlag -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.GA_CASES, ids=str)
def test_k14_gather_edges(dev, case):
    i = SC.gather_inputs(case)
    run = lambda: ops.k14_gather(i.lag.to(dev), i.vit.to(dev), i.cols.to(dev), i.neg.to(dev))
    lag_pos, neg_cross = run()
    ref = SC.gather_refs(case)
    assert _same([lag_pos, neg_cross], [ref["lag_pos"], ref["neg_cross"]])
    assert _same(run(), [lag_pos, neg_cross])


@pytest.mark.parametrize("case", SC.NS_CASES, ids=str)
def test_k14_negscatter_adds_in_source_order(dev, case):
    i = SC.negscatter_inputs(case)
    run = lambda: ops.k14_negscatter(i.d_neg.to(dev), i.off.to(dev), i.src.to(dev), i.hw)
    got = run()
    r64, r32 = SR.k14_negscatter(i.d_neg, i.off, i.src, i.hw)
    print(f"SAMPLEFIG k14_negscatter {case}: max |got - fp64| {float((got.cpu().double() - r64).abs().max()):.3e}, bitwise {_same([got], [r32])}")
    assert _same([got], [r32])
    assert bool((got[0] == 0).all()) and bool((got[-1] == 0).all()) and not bool(torch.signbit(got[0]).any())
    assert _same([run()], [got])


@pytest.mark.parametrize("case", SC.DL_CASES, ids=str)
def test_k14_dlag_edges(dev, case):
    i = SC.dlag_inputs(case)
    run = lambda: ops.k14_dlag(i.lag.to(dev), i.lnorm.to(dev), i.cols.to(dev), i.d_k.to(dev))
    dctx = run()
    _check("k14_dlag", case, dict(dctx=dctx), SC.dlag_refs(case), SC.dlag_refs(case, F32))
    odd = dctx[:, :, 1::2]
    assert bool((odd == 0).all()) and not bool(torch.signbit(odd).any())                  # +0, bit for bit
    assert _same([run()], [dctx])


# ---- the device sampler: every draw predicted bit for bit ----------------------------------------------------------------------------------
def _sample(case, dev):
    n, hw = case.n, case.hw
    k9 = torch.full((n // 2, case.top_k, case.neg_n), -1, dtype=torch.int64, device=dev)
    k14 = torch.full((n, hw, case.neg_c), -1, dtype=torch.int64, device=dev)
    off = torch.full((hw + 1,), -1, dtype=torch.int32, device=dev); src = torch.full((n * hw * case.neg_c,), -1, dtype=torch.int32, device=dev)
    ws = torch.zeros(int(lib().device_sample_ws(hw)), dtype=torch.int32, device=dev)
    state = torch.tensor([case.seed, case.step], dtype=torch.int64, device=dev)
    out = {}
    for s in range(case.steps):
        lib().device_sample(state.data_ptr(), n, case.top_k, hw, case.neg_n, case.neg_c, k9.data_ptr(), k14.data_ptr(), off.data_ptr(),
                            src.data_ptr(), ws.data_ptr(), _stream())
        out.update({f"k9@{s}": k9.cpu(), f"k14@{s}": k14.cpu(), f"csr_off@{s}": off.cpu(), f"csr_src@{s}": src.cpu()})
    return out, state.cpu().tolist()


@pytest.mark.parametrize("case", SC.SP_CASES, ids=str)
def test_device_sampler_draws_are_the_predicted_ones(dev, case):
    ref = SC.sampler_refs(case)
    got, state = _sample(case, dev)
    for k, r in ref.items():
        assert torch.equal(got[k], r), (str(case), k)
    assert state == [case.seed, case.step + case.steps]
    again, state2 = _sample(case, dev)
    assert _same(list(again.values()), list(got.values())) and state2 == state


# ---- argument rejections: every one returns before a kernel starts -------------------------------------------------------------------------
def test_bad_arguments_raise_and_leave_the_outputs_alone(dev):
    S = -12345.0
    f = lambda *s: torch.full(s, S, device=dev)
    l = lambda *s: torch.full(s, -12345, dtype=torch.int64, device=dev)
    z = lambda *s: torch.zeros(*s, device=dev)
    untouched = lambda *ts: all(bool((t == -12345).all()) for t in ts)
    # crossmap: L = 33 > CM_MAXL; E = 6; one position past the 64 KiB of LDS
    for L, hw, e in ((33, 4, 4), (4, 4, 6), (32, 414, 4)):
        lag, vit, w, b = z(1, L, e), z(1, hw, e), z(L, L, 3), z(L)
        cols, lv = l(1, hw), f(1, L, hw)
        with pytest.raises(ops.DcnError, match="crossmap"):
            lib().crossmap(lag.data_ptr(), vit.data_ptr(), w.data_ptr(), b.data_ptr(), 1, L, hw, e, cols.data_ptr(), lv.data_ptr(), _stream())
        assert untouched(cols, lv), (L, hw, e)
    # k9_fwd: top_k = 65 > SK_MAXK; top_k = HW^2 + 1; neg_n = HW
    for hw, top_k, neg_n in ((9, 65, 1), (2, 5, 1), (4, 4, 4)):
        e = 4
        cm, fv, raw = z(1, hw * hw), z(2, hw, e), torch.zeros(1, top_k, neg_n, dtype=torch.int64, device=dev)
        index, neg_idx, fr, co, ng = l(1, top_k), l(1, top_k, neg_n), f(1, top_k, e), f(1, top_k, e), f(1, top_k, neg_n, e)
        with pytest.raises(ops.DcnError, match="k9_fwd"):
            lib().k9_fwd(cm.data_ptr(), fv.data_ptr(), raw.data_ptr(), 1, hw, e, top_k, neg_n, index.data_ptr(), neg_idx.data_ptr(),
                         fr.data_ptr(), co.data_ptr(), ng.data_ptr(), _stream())
        assert untouched(index, neg_idx, fr, co, ng), (hw, top_k, neg_n)
    # k9_bwd: 1024 list entries need more than 64 KiB of LDS; empty or negative lists
    for top_k, neg_n in ((64, 15), (0, 1), (-1, 1), (4, -1)):
        hw, e, k, m = 4, 4, max(top_k, 1), max(neg_n, 1)
        index, neg_idx = torch.zeros(1, k, dtype=torch.int64, device=dev), torch.zeros(1, k, m, dtype=torch.int64, device=dev)
        dfv = f(2, hw, e)
        with pytest.raises(ops.DcnError, match="k9_bwd"):
            lib().k9_bwd(index.data_ptr(), neg_idx.data_ptr(), z(1, k, e).data_ptr(), z(1, k, e).data_ptr(), z(1, k, m, e).data_ptr(), 1, hw, e,
                         top_k, neg_n, dfv.data_ptr(), _stream())
        assert untouched(dfv), (top_k, neg_n)
    # k14_dlag: (2 * 8176 + 33) * 4 bytes are four more than 64 KiB
    hw, e = 8176, 4
    dctx = f(1, 2, 2 * e)
    with pytest.raises(ops.DcnError, match="k14_dlag"):
        lib().k14_dlag(z(1, 2, e).data_ptr(), z(1, e).data_ptr(), torch.zeros(1, hw, dtype=torch.int64, device=dev).data_ptr(),
                       z(1, hw, e).data_ptr(), 1, 2, hw, e, dctx.data_ptr(), _stream())
    assert untouched(dctx)
    # device_sample: odd n; more than 16 negatives; neg_n = hw
    for n, hw, neg_n in ((3, 20, 2), (2, 20, 17), (2, 5, 5)):
        top_k, neg_c = 2, 2
        k9, k14 = l(max(n // 2, 1), top_k, neg_n), l(n, hw, neg_c)
        off = torch.full((hw + 1,), -12345, dtype=torch.int32, device=dev); src = torch.full((n * hw * neg_c,), -12345, dtype=torch.int32, device=dev)
        ws = torch.full((hw,), -12345, dtype=torch.int32, device=dev)
        state = torch.tensor([5, 9], dtype=torch.int64, device=dev)
        with pytest.raises(ops.DcnError, match="device_sample"):
            lib().device_sample(state.data_ptr(), n, top_k, hw, neg_n, neg_c, k9.data_ptr(), k14.data_ptr(), off.data_ptr(), src.data_ptr(),
                                ws.data_ptr(), _stream())
        assert untouched(k9, k14, off, src, ws) and state.cpu().tolist() == [5, 9], (n, hw, neg_n)
