"""The thirteen kernels of the cross-scale head tail (csrc/head.hip, csrc/locmod.hip; pad_rows and colsum with them), each through its
dcnet_amd.ops wrapper against the fp64 stage reference of tests/head_ref.py over the case tables of tests/head_cases.py, per element and
relative to what was summed into the element: P from 3 to 8192 around every stride of the kernels, B = 1, ld = 15 and mixed, non-square
scales, ties of the minimum and maximum across lanes, waves, trips and scales, a constant loc_map, a zero-objectness image, dead rows,
zero-variance channels, exact zeros at the ReLU mask, every set of missing output gradients, the strided dMp view, and the updated
running statistics relative to their update term.  test_head_ref_host.py shows on the CPU that these inputs tell seventeen wrong
variants from the right answer.  Each backward kernel is given the device's own forward outputs, as in the model."""
import types

import pytest
import torch

import head_cases as HC
import head_ref as HR
from dcnet_amd import ops

pytestmark = pytest.mark.gpu
U = HR.U
F32 = HR.F32


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int64) if t.dtype == torch.float64 else t)


def _same(xs, ys):
    return all((x is None and y is None) or torch.equal(_bits(x), _bits(y)) for x, y in zip(xs, ys))


def _check(kernel, name, got, ref, ref32):
    """got: key -> device tensor.  Every key of the reference that the kernel produced, per element against its scale; exact where the
    scale is 0.  Prints one HEADFIG line per key and fails after all of them."""
    bad = []
    for k, r in ref.items():
        if k in HC.GUARD_KEYS or k not in got:
            continue
        r32, ex32 = HR.err_units(ref32[k][0], r[0], r[1])
        assert ex32, (kernel, name, k)
        err, exact = HR.err_units(got[k].cpu(), r[0], r[1])
        print(f"HEADFIG {kernel} {name} {k}: err {err / U:.2f} u, r32 {r32 / U:.2f} u, ratio {err / max(r32, U):.2f}, exact {exact}")
        if not exact or not err <= HC.head_tol(r32):
            bad.append((k, err / U, r32 / U, exact))
    assert not bad, (kernel, name, bad)


def _check64(kernel, name, key, got, ref, scale):
    """An fp64 output (the moments) against fp64 sums, in units of 2**-53 of the scale."""
    err, exact = HR.err_units(got.cpu(), ref, scale)
    print(f"HEADFIG {kernel} {name} {key}: err {err / HR.U64:.2f} u64")
    assert exact and err <= HC.MOM_MARGIN * HR.U64, (kernel, name, key, err / HR.U64)


def _bn(n, rm, rv, dev):
    bn = torch.nn.BatchNorm1d(n).to(dev)
    with torch.no_grad():
        bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    return bn


# ---- the kernels over three scales --------------------------------------------------------------------------------------------------
def _tail_forward(case, dev, rows=None):
    """head_obj and head_final_fwd on the case's inputs (rows: a slice of the batch)."""
    i = HC.tail_inputs(case)
    sl = rows or slice(None)
    logits = [t[sl].to(dev) for t in i.logits]; sims = [t[sl].to(dev) for t in i.sims]
    only, obj_map, objn, X = ops.head_obj(logits, sims, i.e8.to(dev))
    outbox, loc, mm = ops.head_final_fwd(logits, sims, i.loc_map[sl].to(dev))
    return types.SimpleNamespace(logits=logits, sims=sims, only=only, obj_map=obj_map, objn=objn, X=X, outbox=outbox, loc=loc, mm=mm)


def _flat_outputs(f):
    return [*f.only, f.obj_map, f.objn, f.X, *f.outbox, *f.loc, f.mm]


@pytest.mark.parametrize("case", HC.TAIL_CASES, ids=str)
def test_tail_forward_edges(dev, case):
    i = HC.tail_inputs(case)
    f = _tail_forward(case, dev)
    ref, ref32 = HC.tail_forward_refs(case), HC.tail_forward_refs(case, F32)
    got = dict(obj_map=f.obj_map, objn=f.objn, X=f.X, **{f"only{s}": f.only[s] for s in range(3)})
    _check("head_obj", case, got, ref["obj"], ref32["obj"])
    assert bool((f.X[:, i.P:] == 0).all())
    if case.plant == "sim0":
        assert float(f.objn[0]) == 0.0 and bool((f.obj_map[0] == 0).all()) and bool((f.X[:8] == 0).all())
    got = dict(mm=f.mm[:, :2], **{f"outbox{s}": f.outbox[s] for s in range(3)}, **{f"loc{s}": f.loc[s] for s in range(3)})
    _check("head_final_fwd", case, got, ref["final"], ref32["final"])
    idx = f.mm[:, 2:].contiguous().view(torch.int32).cpu().long()
    assert torch.equal(idx[:, 0], ref["final"]["imn"]) and torch.equal(idx[:, 1], ref["final"]["imx"]), (idx, ref["final"]["imn"])
    # a second call is the first; a batch is its images one at a time
    assert _same(_flat_outputs(_tail_forward(case, dev)), _flat_outputs(f))
    for b in range(case.B):
        one = _tail_forward(case, dev, slice(b, b + 1))
        assert _same(_flat_outputs(one), [*[t[b:b + 1] for t in f.only], f.obj_map[b:b + 1], f.objn[b:b + 1], f.X[8 * b:8 * b + 8],
                                          *[t[b:b + 1] for t in f.outbox], *[t[b:b + 1] for t in f.loc], f.mm[b:b + 1]]), b


def _tail_backward(case, which, f, dev, rows=None):
    i = HC.tail_inputs(case)
    sl = rows or slice(None)
    cut = lambda ts: [None if t is None else t[sl].to(dev) for t in ts]
    d_outbox, d_loc, d_only, dobj = HC.grad_args(case, which)
    d_outbox, d_loc, d_only = cut(d_outbox), cut(d_loc), cut(d_only)
    dloc_map = ops.head_dloc(f.logits, f.sims, f.loc, d_outbox, d_loc, f.mm)
    dlogits, dsim = ops.head_dlogits(f.logits, f.sims, f.loc, f.only, d_outbox, d_only, f.obj_map, f.objn, None if dobj is None else dobj[sl].to(dev))
    return dloc_map, dlogits, dsim


@pytest.mark.parametrize("which", HC.GRAD_SETS)
@pytest.mark.parametrize("case", HC.TAIL_CASES, ids=str)
def test_tail_backward_edges(dev, case, which):
    i = HC.tail_inputs(case)
    f = _tail_forward(case, dev)
    c = lambda t: t.cpu()
    idx = f.mm[:, 2:].contiguous().view(torch.int32).cpu().long()
    fwd = types.SimpleNamespace(loc=[c(t).reshape(case.B, -1) for t in f.loc], mm=c(f.mm[:, :2]), imn=idx[:, 0], imx=idx[:, 1],
                                only=[c(t).reshape(case.B, -1) for t in f.only], obj_map=c(f.obj_map), objn=c(f.objn))
    ref, ref32 = HC.tail_backward_refs(case, which, fwd), HC.tail_backward_refs(case, which, fwd, F32)
    dloc_map, dlogits, dsim = _tail_backward(case, which, f, dev)
    name = f"{case} {which}"
    _check("head_dloc", name, dict(dloc_map=dloc_map), ref["dloc"], ref32["dloc"])
    got = dict(**{f"dlogits{s}": dlogits[s] for s in range(3)}, **{f"dsim{s}": dsim[s] for s in range(3)})
    _check("head_dlogits", name, got, ref["dlogits"], ref32["dlogits"])
    assert all(bool((dlogits[s][..., 15:] == 0).all()) for s in range(3))
    again = _tail_backward(case, which, f, dev)
    assert _same([again[0], *again[1], *again[2]], [dloc_map, *dlogits, *dsim])
    if which == "all":
        dobj, de8 = ops.head_fold(i.dX.to(dev), i.e8.to(dev), f.obj_map)
        _check("head_fold", case, dict(dobj_map=dobj, dE8x=de8), ref["fold"], ref32["fold"])
        assert _same(ops.head_fold(i.dX.to(dev), i.e8.to(dev), f.obj_map), (dobj, de8))
        for b in range(case.B):
            one = _tail_backward(case, which, _tail_forward(case, dev, slice(b, b + 1)), dev, slice(b, b + 1))
            assert _same([one[0], *one[1], *one[2]], [dloc_map[b:b + 1], *[t[b:b + 1] for t in dlogits], *[t[b:b + 1] for t in dsim]]), b
            assert _same([ops.head_fold(i.dX[8 * b:8 * b + 8].to(dev), i.e8.to(dev), f.obj_map[b:b + 1])[0]], [dobj[b:b + 1]]), b


def test_bad_geometry_and_channel_counts_raise(dev):
    z = lambda *s: torch.zeros(*s, device=dev)
    for what, scales in HC.BAD_GEOMETRY.items():
        logits = [z(1, h, w, ld) for h, w, ld in scales]; sims = [z(1, h * w) for h, w, _ in scales]
        P = sum(h * w for h, w, _ in scales)
        with pytest.raises(ops.DcnError, match="head_obj"):
            ops.head_obj(logits, sims, z(P, 8))
        if what == "ld = 14":
            with pytest.raises(ops.DcnError, match="head_final_fwd"):
                ops.head_final_fwd(logits, sims, z(1, P))
            loc = [z(1, h, w) for h, w, _ in scales]
            with pytest.raises(ops.DcnError, match="head_dloc"):
                ops.head_dloc(logits, sims, loc, [None] * 3, loc, z(1, 4))
            with pytest.raises(ops.DcnError, match="head_dlogits"):
                ops.head_dlogits(logits, sims, loc, loc, [None] * 3, [None] * 3, z(1, P), z(1), None)
    bn = torch.nn.BatchNorm1d(256).to(dev)
    mom = torch.zeros(72, dtype=torch.float64, device=dev)
    with pytest.raises(ops.DcnError, match="locbn_fwd"):
        ops.locbn_fwd(z(1, 8, 256), mom, z(256), z(256), z(256), bn, True, 8)
    with pytest.raises(ops.DcnError, match="locbn_bwd"):
        ops.locbn_bwd(z(1, 8, 256), mom, z(256), z(256), z(256), z(3, 256), z(1, 8, 256), z(256), True, 8)
    with pytest.raises(ops.DcnError, match="locmod_fwd"):
        ops.locmod_fwd(z(4, 8), z(1, 8, 256), z(256), z(1, 256))
    with pytest.raises(ops.DcnError, match="locmod_bwd"):
        ops.locmod_bwd(z(4, 8), z(1, 8, 256), z(256), z(1, 256), z(1, 4))


# ---- location embedding ----------------------------------------------------------------------------------------------------------
def _locemb_forward(case, dev):
    i = HC.locemb_inputs(case)
    bn = _bn(8, i.rm, i.rv, dev)
    d = lambda t: t.to(dev)
    e8, xh, stat, mom = ops.locemb_fwd(d(i.coord), d(i.W), d(i.b), d(i.gamma), d(i.beta), bn, case.training, i.count)
    return e8, xh, stat, mom, bn.running_mean.clone(), bn.running_var.clone()


@pytest.mark.parametrize("case", HC.LOCEMB_CASES, ids=str)
def test_locemb_edges(dev, case):
    i = HC.locemb_inputs(case)
    e8, xh, stat, mom, rm, rv = _locemb_forward(case, dev)
    ref, ref32 = HC.locemb_refs(case)["locemb_fwd"], HC.locemb_refs(case, None, F32)["locemb_fwd"]
    _check("locemb_fwd", case, dict(E8=e8, xh=xh, stat=stat, rm=rm, rv=rv), ref, ref32)
    if not case.training:
        assert _same([rm, rv], [i.rm, i.rv])
    m64, s64 = HR.moments_exact(e8.cpu())
    _check64("locemb_fwd", case, "mom", mom, m64, s64)
    if case.plant == "const":
        assert bool((xh[:, HC.CONST_CH] == 0).all()) and bool((e8[:, HC.CONST_CH] == 0).all())
    if case.plant == "deadrow":
        assert bool((e8[i.dead] == 0).all())
    assert _same(_locemb_forward(case, dev), (e8, xh, stat, mom, rm, rv))
    if not case.bwd:
        return
    d = lambda t: None if t is None else t.to(dev)
    for args in ("full", "dEa"):
        fwd = (xh.cpu(), stat.cpu())
        rb, rb32 = HC.locemb_refs(case, fwd, args=args)["locemb_bwd"], HC.locemb_refs(case, fwd, F32, args=args)["locemb_bwd"]
        y, s = rb["y"]
        assert not bool(((y.abs() <= 0.5 * HC.GUARD * s) & (s > 0)).any())            # the device's own x-hat is clear of the band as well
        dEb, dmom = (i.dEb, i.dmom if case.training else None) if args == "full" else (None, None)
        run = lambda: ops.locemb_bwd(d(i.coord), d(i.W), d(i.gamma), d(i.beta), d(HC.locemb_bwd_xh(case, xh.cpu())), stat, d(i.dEa), d(dEb),
                                     d(dmom), case.training)
        grads = run()
        _check("locemb_bwd", f"{case} {args}", dict(grads=grads), rb, rb32)
        assert _same([run()], [grads])


# ---- BatchNorm1d(512) from the moments -------------------------------------------------------------------------------------------------
def _locbn_forward(case, dev):
    i = HC.locbn_inputs(case)
    bn = _bn(512, i.rm, i.rv, dev)
    d = lambda t: t.to(dev)
    Mp, bp, saved = ops.locbn_fwd(d(i.M), d(i.mom), d(i.b), d(i.gamma), d(i.beta), bn, case.training, i.count)
    return Mp, bp, saved, bn.running_mean.clone(), bn.running_var.clone()


@pytest.mark.parametrize("case", HC.LOCBN_CASES, ids=str)
def test_locbn_edges(dev, case):
    i = HC.locbn_inputs(case)
    Mp, bp, saved, rm, rv = _locbn_forward(case, dev)
    refs, refs32 = HC.locbn_refs(case, saved.cpu()), HC.locbn_refs(case, saved.cpu(), F32)
    _check("locbn_fwd", case, dict(Mp=Mp, bp=bp, saved=saved, rm=rm, rv=rv), refs["locbn_fwd"], refs32["locbn_fwd"])
    if not case.training:
        assert _same([rm, rv], [i.rm, i.rv])
    assert _same(_locbn_forward(case, dev), (Mp, bp, saved, rm, rv))
    d = lambda t: t.to(dev)
    dsum = d(i.dsum)
    run = lambda dMp: ops.locbn_bwd(d(i.M), d(i.mom), d(i.b), d(i.gamma), d(i.rm), saved, dMp, d(i.dbp), case.training, i.count)
    view = dsum[:, :8]
    assert view.stride(0) == 10 * 512 and not view.is_contiguous() or case.B == 1
    dM, out, dmom = run(view)
    _check("locbn_bwd", case, dict(dM=dM, out=out), refs["locbn_bwd"], refs32["locbn_bwd"])
    if case.training:
        _check64("locbn_bwd", case, "dmom", dmom, *refs["locbn_bwd"]["dmom"])
    # the strided view of dsum and a contiguous copy give bitwise the same; a second call is the first
    assert _same(run(view.contiguous()), (dM, out, dmom)) and _same(run(view), (dM, out, dmom))


# ---- location module core ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", HC.LOCMOD_CASES, ids=str)
def test_locmod_edges(dev, case):
    i = HC.locmod_inputs(case)
    d = lambda t: t.to(dev)
    E, Mp, bp, q, dloc = d(i.E), d(i.Mp), d(i.bp), d(i.q), d(i.dloc)
    refs, refs32 = HC.locmod_refs(case), HC.locmod_refs(case, F32)
    loc = ops.locmod_fwd(E, Mp, bp, q)
    _check("locmod_fwd", case, dict(loc=loc), refs["locmod_fwd"], refs32["locmod_fwd"])
    if case.plant == "dead":
        assert bool((loc[0] == 0).all()) and bool((loc[:, 0] == 0).all()) and bool((loc[:, case.P - 1] == 0).all())
    assert _same([ops.locmod_fwd(E, Mp, bp, q)], [loc])
    for n in range(case.n):
        assert _same([ops.locmod_fwd(E, Mp[n:n + 1].contiguous(), bp, q[n:n + 1].contiguous())], [loc[n:n + 1]]), n
    if not case.bwd:
        return
    dE, dsum = ops.locmod_bwd(E, Mp, bp, q, dloc)
    _check("locmod_bwd", case, dict(dE_part=dE, dsum=dsum), refs["locmod_bwd"], refs32["locmod_bwd"])
    assert _same(ops.locmod_bwd(E, Mp, bp, q, dloc), (dE, dsum))
    for n in range(case.n):
        one = ops.locmod_bwd(E, Mp[n:n + 1].contiguous(), bp, q[n:n + 1].contiguous(), dloc[n:n + 1].contiguous())
        assert _same(one, (dE[n:n + 1], dsum[n:n + 1])), n


# ---- copies and column sums ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,cols_out", [(5, 257, 288), (3, 288, 257), (2, 8161, 8192), (512, 3, 32)])
def test_pad_rows_is_an_exact_copy_with_a_zero_tail(dev, rows, cols, cols_out):
    src = torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows + cols))
    got = ops.pad_rows(src.to(dev), cols_out)
    ref = HR.pad_rows(src, cols_out)["out"][0]
    assert torch.equal(got.cpu().double(), ref)


@pytest.mark.parametrize("rows,cols,stride", [(1, 512, 512), (5, 512, 10 * 512), (11, 512, 10 * 512), (3, 8 * 257, 8 * 257), (2, 8 * 1025, 8 * 1025)])
def test_colsum_of_strided_rows(dev, rows, cols, stride):
    """The two uses in HeadTail.backward: dbp = colsum(dsum[:, 8]) (row stride 10 * 512) and dE_a = colsum(dE_part.view(B, P * 8))."""
    base = torch.randn(rows, stride, generator=torch.Generator().manual_seed(rows + cols))
    view = base.to(dev)[:, stride - cols:]
    got = ops.colsum(view)
    ref, ref32 = HR.colsum(base[:, stride - cols:]), HR.colsum(base[:, stride - cols:], F32)
    _check("colsum", f"{rows}x{cols}/{stride}", dict(out=got), ref, ref32)
    assert _same([ops.colsum(view)], [got])


# ---- the autograd function with missing output gradients ----------------------------------------------------------------------------------
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_head_tail_backward_with_none_is_backward_with_zeros(dev, training):
    """HeadTail.backward given None for an output gradient (NULL pointers in head_dloc / head_dlogits) is bitwise the backward given a
    zero tensor in its place, at P = 1025 (a second trip of the 1024-thread loops)."""
    from dcnet_amd.functions import HeadTail
    case = next(c for c in HC.TAIL_CASES if c.plant == "tie-trip")
    i = HC.tail_inputs(case)
    B, P = case.B, i.P
    g = torch.Generator().manual_seed(77)
    rn = lambda *s: torch.randn(*s, generator=g)
    leaf = lambda t: t.to(dev).requires_grad_(True)
    logits = [leaf(t) for t in i.logits]; sims = [leaf(t.view(B, h, w)) for t, (h, w, _) in zip(i.sims, case.scales)]
    q = leaf(torch.nn.functional.normalize(rn(B, 512), dim=1)); coord = (2 * torch.rand(P, 8, generator=g) - 1).to(dev)
    prm = [leaf(t) for t in (rn(8, 8) * 0.6, rn(8) * 0.1, 1 + 0.2 * rn(8), 0.3 * rn(8), rn(512, P) / P ** 0.5, rn(512) * 0.1, 1 + 0.2 * rn(512),
                             0.2 * rn(512))]
    bn_le = _bn(8, rn(8) * 0.2, torch.rand(8, generator=g) + 0.5, dev); bn_lt = _bn(512, rn(512) * 0.02, torch.rand(512, generator=g) * 0.01 + 0.005, dev)
    res = HeadTail.apply(*logits, *sims, q, coord, *prm, bn_le, bn_lt, training)
    node = res[0].grad_fn
    d_out = [t.view_as(r).to(dev) for t, r in zip(i.d_outbox, res[0:3])]; d_loc = [t.view_as(r).to(dev) for t, r in zip(i.d_loc, res[3:6])]
    zeros = lambda rs: [torch.zeros_like(r) for r in rs]
    for with_none, with_zero in (((*d_out, None, None, None, None, None, None), (*d_out, *zeros(res[3:6]), *zeros(res[6:9]))),
                                 ((*d_out, *d_loc, None, None, None), (*d_out, *d_loc, *zeros(res[6:9]))),
                                 ((d_out[0], None, d_out[2], *d_loc, None, None, None), (d_out[0], torch.zeros_like(res[1]), d_out[2], *d_loc,
                                                                                        *zeros(res[6:9])))):
        a = HeadTail.backward(node, *with_none); b = HeadTail.backward(node, *with_zero)
        assert len(a) == len(b) == 19
        for n, (x, y) in enumerate(zip(a, b)):
            assert (x is None and y is None) or torch.equal(x, y), n
        assert all(bool(torch.isfinite(x).all()) for x in a if x is not None)
