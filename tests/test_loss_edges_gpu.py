"""The kernels of csrc/loss.hip (target assignment, the dense losses forward and backward, the InfoNCE rows forward and backward, the
evaluation decode, box IoU), each through its dcnet_amd.ops entry point against the references of tests/loss_ref.py over the case tables
of tests/loss_cases.py.  Integers (target_i, the dense target's positions, the decode's cellinfo) and every element the reference marks
with scale 0 are compared bit for bit; everything else per element in fp64, relative to what was summed into the element, at
LOSS_MARGIN * max(r32, 2**-24).  test_loss_ref_host.py shows on the CPU that these inputs tell twenty-nine wrong variants from the right
answer.  The outputs of dense_loss_bwd, contrastive_bwd, decode_boxes and target_dense are views inside larger buffers, prefilled with NaN
(0x7fffffff for integers): every element must be written and nothing around them.  Every kernel is launched twice and must repeat itself
bitwise; calls whose shapes do not agree with `size` and `n` must raise before anything is launched."""
import math
import types

import pytest
import torch

import loss_cases as LC
import loss_ref as LR
from dcnet_amd import losses, ops
from dcnet_amd.lib import lib

pytestmark = pytest.mark.gpu
U = LR.U
F32 = LR.F32
PAD = 64                                                        # elements around a guarded view (a multiple of the 16-byte vectors)
IFILL = 0x7FFFFFFF


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(xs, ys):
    return all(x.shape == y.shape and torch.equal(_bits(x), _bits(y)) for x, y in zip(xs, ys))


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """Contiguous views of the given shapes, each inside a buffer of its own with PAD elements on both sides, all prefilled."""

    def __init__(self, dev, shapes, dtype=torch.float32, fill=float("nan")):
        self.fill, self.bufs, self.views = fill, [], []
        for shape in shapes:
            n = math.prod(shape)
            buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=dev)
            self.bufs.append(buf); self.views.append(buf[PAD:PAD + n].view(shape))

    def surroundings_untouched(self):
        same = (lambda t: torch.isnan(t).all()) if isinstance(self.fill, float) and math.isnan(self.fill) else (lambda t: (t == self.fill).all())
        return all(bool(same(b[:PAD])) and bool(same(b[-PAD:])) for b in self.bufs)

    def untouched(self):
        same = (lambda t: torch.isnan(t).all()) if isinstance(self.fill, float) and math.isnan(self.fill) else (lambda t: (t == self.fill).all())
        return all(bool(same(b)) for b in self.bufs)


def _check(kernel, name, got, ref, ref32):
    """Every (value, scale) key of the reference per element against its scale, exact where the scale is 0.  Prints one LOSSFIG line per
    key and fails after all of them."""
    bad = []
    for k, r in ref.items():
        if not isinstance(r, tuple) or k not in got:
            continue
        r32, ex32 = LR.err_units(ref32[k][0], r[0], r[1])
        assert ex32, (kernel, name, k)
        err, exact = LR.err_units(got[k].cpu(), r[0], r[1])
        print(f"LOSSFIG {kernel} {name} {k}: err {err / U:.2f} u, r32 {r32 / U:.2f} u, ratio {err / max(r32, U):.2f}, exact {exact}")
        if not exact or not err <= LC.loss_tol(r32):
            bad.append((k, err / U, r32 / U, exact))
    assert not bad, (kernel, name, bad)


# ---- target, target_dense ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LC.TG_CASES, ids=str)
def test_target_edges(dev, case):
    i = LC.target_inputs(case)
    bbox, anchors = i.bbox.to(dev), i.anchors.to(dev)
    ti, tf = ops.build_target(bbox, anchors, case.size)
    ref, ref32 = LC.target_refs(case), LC.target_refs(case, F32)
    assert torch.equal(ti.cpu(), ref["ti"]), (str(case), (ti.cpu() != ref["ti"]).nonzero().tolist())      # every sample: none is excluded
    _check("target", case, dict(tf=tf), ref, ref32)
    for n, kind in enumerate(i.kinds):
        if kind == "boundary":
            assert tf[n, :2].tolist() == [0.0, 0.0]
    assert _same(ops.build_target(bbox, anchors, case.size), (ti, tf))
    # the dense form of the device's own compact targets: a numpy scatter, bit for bit, zeros included
    G = LR.grids(case.size)
    rbox, rctr = LR.target_dense(ti.cpu(), tf.cpu(), case.size)
    box, ctr = ops.target_dense(ti, tf, case.size)
    assert _same(box + ctr, rbox + rctr)
    shapes = [(case.n, 3, 5, g, g) for g in G] + [(case.n, 5, g, g) for g in G]
    for prefill in (0.0, float("nan")):                          # pre-zeroed, as the kernel expects; then NaN: exactly the positive cells are written
        gd = Guarded(dev, shapes)
        for v in gd.views:
            v.fill_(prefill)
        ops.target_dense(ti, tf, case.size, out=(gd.views[:3], gd.views[3:]))
        assert gd.surroundings_untouched()
        if prefill == 0.0:
            assert _same(gd.views, rbox + rctr)
        else:
            mbox, mctr = LR.target_dense(ti.cpu(), torch.ones(case.n, 4), case.size)
            for got, want, mask in zip(gd.views, rbox + rctr, mbox + mctr):
                got = got.cpu()
                assert torch.equal(torch.isnan(got), mask == 0) and _same([got[mask != 0]], [want[mask != 0]])


# ---- dense losses -----------------------------------------------------------------------------------------------------------------------
def _dense_shapes(case):
    G, n = LR.grids(case.size), case.n
    return [(n, 15, g, g) for g in G] + [(n, g, g) for g in G] * 3


def _dense_bwd(dev, case, d, lse, gup):
    gd = Guarded(dev, _dense_shapes(case))
    v = gd.views
    out = ops.dense_loss_bwd(d.outbox, d.sim, d.negsim, d.loc, d.ti, d.tf, lse, torch.tensor(gup, dtype=F32, device=dev), case.size,
                             out=(v[0:3], v[3:6], v[6:9], v[9:12]))
    assert gd.surroundings_untouched()
    return out


@pytest.mark.parametrize("case", LC.DN_CASES, ids=str)
def test_dense_loss_edges(dev, case):
    i = LC.dense_inputs(case)
    to = lambda ts: [t.to(dev) for t in ts]
    d = types.SimpleNamespace(outbox=to(i.outbox), sim=to(i.sim), negsim=to(i.negsim), loc=to(i.loc), ti=i.ti.to(dev), tf=i.tf.to(dev))
    out, lse, vals = ops.dense_loss_fwd(d.outbox, d.sim, d.negsim, d.loc, d.ti, d.tf, case.size, want_vals=True)
    got = dict(out=out, lse=lse, vals=vals)
    grads = []
    for k, gup in enumerate(LC.GUPS):
        g = _dense_bwd(dev, case, d, lse, gup)
        grads.append(g)
        for key, ts in zip(("d_outbox", "d_sim", "d_negsim", "d_loc"), g):
            got.update({f"{key}@{k}[{s}]": ts[s] for s in range(3)})
    ref, ref32 = LC.dense_refs(case, lse=lse.cpu()), LC.dense_refs(case, F32, lse=lse.cpu())
    assert set(got) == set(ref)                                  # lse, vals, out and the twelve gradient tensors of each upstream set
    _check("dense", case, got, ref, ref32)
    assert float(vals[:, 7].abs().max()) == 0.0
    if case.regime == "equal":                                   # lse = c + log(3P), log(P)
        P = LR.offsets(case.size)[1]
        c = torch.stack([i.outbox[0][:, 4, 0, 0], i.loc[0][:, 0, 0]], 1).double()
        assert float((lse.cpu().double() - c - torch.tensor([math.log(3 * P), math.log(P)])).abs().max()) <= 4 * U * (float(c.abs().max()) + math.log(3 * P))
    if case.sat == 90:                                           # expf overflows: p is exactly 0 or 1, its derivative exactly 0
        for n in range(case.n):
            bn, gi, gj, _ = i.ti[n].tolist()
            for g in grads:
                assert g[0][bn // 3][n, (bn % 3) * 5:(bn % 3) * 5 + 2, gj, gi].tolist() == [0.0, 0.0]
    # an upstream gradient of zero gives zeros, all of them
    zero = _dense_bwd(dev, case, d, lse, (0.0, 0.0, 0.0))
    assert all(bool((t == 0).all()) for ts in zero for t in ts)
    # repeatable, and the default allocations give the same bits as the supplied views
    out2, lse2 = ops.dense_loss_fwd(d.outbox, d.sim, d.negsim, d.loc, d.ti, d.tf, case.size)
    plain = ops.dense_loss_bwd(d.outbox, d.sim, d.negsim, d.loc, d.ti, d.tf, lse, torch.tensor(LC.GUPS[0], dtype=F32, device=dev), case.size)
    assert _same([out2, lse2], [out, lse]) and _same([t for ts in plain for t in ts], [t for ts in grads[0] for t in ts])


# ---- InfoNCE rows -----------------------------------------------------------------------------------------------------------------------
def _contrastive_bwd(dev, q, pos, neg, gup):
    gd = Guarded(dev, [tuple(q.shape), tuple(pos.shape), tuple(neg.shape)])
    out = ops.contrastive_bwd(q, pos, neg, LC.T32, torch.tensor([gup], dtype=F32, device=dev), out=tuple(gd.views))
    assert gd.surroundings_untouched()
    return out


@pytest.mark.parametrize("case", LC.CT_CASES, ids=str)
def test_contrastive_edges(dev, case):
    i = LC.contrastive_inputs(case)
    q, pos, neg = i.q.to(dev), i.pos.to(dev), i.neg.to(dev)
    loss = ops.contrastive_fwd(q, pos, neg, LC.T32)
    got = dict(loss=loss)
    first = None
    for k, gup in enumerate(LC.CT_GUPS):
        g = _contrastive_bwd(dev, q, pos, neg, gup)
        first = first or g
        got.update({f"dq@{k}": g[0], f"dpos@{k}": g[1], f"dneg@{k}": g[2]})
    ref, ref32 = LC.contrastive_refs(case), LC.contrastive_refs(case, F32)
    assert set(got) == set(ref)
    _check("contrastive", case, got, ref, ref32)
    assert all(bool(torch.isfinite(t).all()) for t in got.values())                       # zero rows included: the clamp is a constant
    assert _same([ops.contrastive_fwd(q, pos, neg, LC.T32)], [loss])
    assert _same(ops.contrastive_bwd(q, pos, neg, LC.T32, torch.tensor([LC.CT_GUPS[0]], dtype=F32, device=dev)), first)


class _Stacked(list):
    """A list that carries the (n, K, ...) tensor it was unbound from, as the model's output lists do."""
    stacked = None


@pytest.mark.parametrize("which", ["interframe", "crossmodal"])
def test_contrastive_list_entry_points(dev, which):
    """losses.interframe_contrastive_loss / crossmodal_contrastive_loss on plain lists of K = 3 tensors at n = 2, c = 8: the fp64 reference on
    the stacked rows, and bit for bit the call on lists that carry `.stacked`."""
    K, n, c, m = 3, 2, 8, 5
    g = torch.Generator().manual_seed(31600 + (which == "crossmodal"))
    qs = [torch.randn(n, c, generator=g) for _ in range(K)]
    ks = [torch.randn(*((n, c) if which == "interframe" else (n, 1, c)), generator=g) for _ in range(K)]
    ns = [torch.randn(n, m, c, generator=g) for _ in range(K)]
    fn = losses.interframe_contrastive_loss if which == "interframe" else losses.crossmodal_contrastive_loss
    leaves = [[t.to(dev).requires_grad_(True) for t in ts] for ts in (qs, ks, ns)]
    loss = fn(*leaves)
    loss.backward()
    rows = lambda ts, tail: torch.stack(ts, 1).reshape(n * K, *tail)
    q, pos, neg = rows(qs, (c,)), rows(ks, (c,)), rows(ns, (m, c))
    t32 = float(torch.tensor(0.07, dtype=F32))
    one = torch.tensor([1.0], dtype=F32)
    ref = {**{"loss": LR.contrastive_fwd(q, pos, neg, t32)["loss"]}, **LR.contrastive_bwd(q, pos, neg, t32, one)}
    ref32 = {**{"loss": LR.contrastive_fwd(q, pos, neg, t32, F32)["loss"]}, **LR.contrastive_bwd(q, pos, neg, t32, one, F32)}
    grad = lambda ts, tail: torch.stack([t.grad for t in ts], 1).reshape(n * K, *tail)
    got = dict(loss=loss.detach(), dq=grad(leaves[0], (c,)), dpos=grad(leaves[1], (c,)), dneg=grad(leaves[2], (m, c)))
    _check("contrastive-lists", which, got, ref, ref32)
    carried = [_Stacked([t.to(dev).requires_grad_(True) for t in ts]) for ts in (qs, ks, ns)]
    for lst in carried:
        lst.stacked = torch.stack([t.detach() for t in lst], 1).requires_grad_(True)
    loss2 = fn(*carried)
    loss2.backward()
    assert _same([loss2.detach()], [loss.detach()])
    for lst, ts in zip(carried, leaves):
        assert _same([lst.stacked.grad], [torch.stack([t.grad for t in ts], 1)])


# ---- evaluation decode -------------------------------------------------------------------------------------------------------------------
def _decode(dev, case):
    i = LC.decode_inputs(case)
    fb = Guarded(dev, [(case.n, 4)]); ib = Guarded(dev, [(case.n, 3)], torch.int32, IFILL)
    outbox = [o.to(dev) for o in i.outbox]
    boxes, cells = ops.decode_boxes(outbox, i.anchors.to(dev), case.size, want_cells=True, out=(fb.views[0], ib.views[0]))
    assert fb.surroundings_untouched() and ib.surroundings_untouched()
    assert bool((cells != IFILL).all())
    return outbox, boxes, cells


@pytest.mark.parametrize("case", LC.DC_CASES, ids=str)
def test_decode_edges(dev, case):
    outbox, boxes, cells = _decode(dev, case)
    ref, ref32 = LC.decode_refs(case), LC.decode_refs(case, F32)
    assert torch.equal(cells.cpu(), ref["cellinfo"]), (str(case), cells.cpu().tolist(), ref["cellinfo"].tolist())
    _check("decode", case, dict(boxes=boxes), ref, ref32)
    anchors = LC.decode_inputs(case).anchors.to(dev)
    plain = ops.decode_boxes(outbox, anchors, case.size)
    b2, c2 = ops.decode_boxes(outbox, anchors, case.size, want_cells=True)
    assert _same([plain, b2, c2], [boxes, boxes, cells])


@pytest.mark.parametrize("case", LC.DECODE_NONFINITE, ids=str)
def test_decode_index_stays_in_range_on_non_finite_confidences(dev, case):
    """Every confidence -inf gives index 0; a NaN gives the first NaN, as torch.max does.  Only cellinfo is specified."""
    _, _, cells = _decode(dev, case)
    assert torch.equal(cells.cpu(), LC.decode_refs(case)["cellinfo"]), (str(case), cells.cpu().tolist())


# ---- box IoU -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LC.BI_CASES, ids=str)
def test_box_iou_edges(dev, case):
    i = LC.box_iou_inputs(case)
    b1, b2 = i.b1.to(dev), i.b2.to(dev)
    iou = ops.box_iou(b1, b2)
    _check("box_iou", case, dict(iou=iou), LC.box_iou_refs(case), LC.box_iou_refs(case, F32))
    assert _same([ops.box_iou(b1, b2)], [iou])


# ---- argument rejections: every one raises before a kernel starts ---------------------------------------------------------------------------
def test_rejections(dev):
    f = lambda *s: torch.zeros(*s, device=dev)
    maps = lambda n, size, lead=(): [f(n, *lead, g, g) for g in LR.grids(size)]
    ti, tf = torch.zeros(2, 4, dtype=torch.int32, device=dev), f(2, 4)
    anchors = LR.scaled_anchors(256).to(dev)
    ob, sim = maps(2, 256, (15,)), maps(2, 256)
    lse, g3, g1 = f(2, 2), f(3), f(1)

    def bad(match, fn, *a, **k):
        with pytest.raises(ValueError, match=match):
            fn(*a, **k)

    # build_target
    bad("bbox", ops.build_target, f(2, 5), anchors, 256)
    bad("bbox", ops.build_target, f(2, 4).double(), anchors, 256)
    bad("bbox", ops.build_target, f(2, 4).cpu(), anchors, 256)
    bad("anchors", ops.build_target, f(2, 4), f(9, 2), 256)
    bad("size", ops.build_target, f(2, 4), anchors, 100)
    bad("size", ops.build_target, f(2, 4), anchors, 0)
    # target_dense
    bad("target_i", ops.target_dense, ti.long(), tf, 256)
    bad("target_f", ops.target_dense, ti, f(2, 3), 256)
    bad("target_f", ops.target_dense, ti, f(3, 4), 256)
    bad("size", ops.target_dense, ti, tf, 48)
    gd = Guarded(dev, [(2, 3, 5, g, g) for g in LR.grids(256)] + [(2, 5, g, g) for g in LR.grids(256)])
    bad("out", ops.target_dense, ti, tf, 416, out=(gd.views[:3], gd.views[3:]))                 # buffers of 256 at size 416
    bad("out", ops.target_dense, ti, tf, 256, out=(gd.views[:3], gd.views[:3]))
    assert gd.untouched()
    # dense_loss_fwd / bwd: maps built for 256 at size 416, a channel dimension too many, a list of two, n of the targets
    for fn, tail in ((ops.dense_loss_fwd, ()), (ops.dense_loss_bwd, (lse, g3))):
        bad("outbox", fn, ob, sim, sim, sim, ti, tf, *tail, 416)
        bad("outbox", fn, maps(2, 256, (3, 5)), sim, sim, sim, ti, tf, *tail, 256)
        bad("sim", fn, ob, maps(2, 256, (1,)), sim, sim, ti, tf, *tail, 256)
        bad("negsim", fn, ob, sim, sim[:2], sim, ti, tf, *tail, 256)
        bad("loc", fn, ob, sim, sim, maps(3, 256), ti, tf, *tail, 256)
        bad("loc", fn, ob, sim, sim, [t.double() for t in sim], ti, tf, *tail, 256)
        bad("target_i", fn, ob, sim, sim, sim, ti[:1].long(), tf, *tail, 256)
        bad("outbox", fn, ob, sim, sim, sim, ti[:1], tf[:1], *tail, 256)
        bad("size", fn, ob, sim, sim, sim, ti, tf, *tail, 250)
    gd = Guarded(dev, [(2, 15, g, g) for g in LR.grids(256)] + [(2, g, g) for g in LR.grids(256)] * 3)
    v = gd.views
    good_out = (v[0:3], v[3:6], v[6:9], v[9:12])
    bad("lse", ops.dense_loss_bwd, ob, sim, sim, sim, ti, tf, f(2), g3, 256, out=good_out)
    bad("gout", ops.dense_loss_bwd, ob, sim, sim, sim, ti, tf, lse, g1, 256, out=good_out)
    bad("d_sim", ops.dense_loss_bwd, ob, sim, sim, sim, ti, tf, lse, g3, 256, out=(v[0:3], v[0:3], v[6:9], v[9:12]))
    bad("outbox", ops.dense_loss_bwd, maps(2, 416, (15,)), maps(2, 416), maps(2, 416), maps(2, 416), ti, tf, lse, g3, 256, out=good_out)
    assert gd.untouched()
    # contrastive: pos against q, neg against both, a gradient of the wrong length, strides
    q, pos, neg = f(4, 8), f(4, 8), f(4, 5, 8)
    for fn, tail in ((ops.contrastive_fwd, ()), (ops.contrastive_bwd, (g1,))):
        bad("pos", fn, q, f(3, 8), neg, 0.07, *tail)
        bad("pos", fn, q, f(4, 12), neg, 0.07, *tail)
        bad("neg", fn, q, pos, f(4, 5, 12), 0.07, *tail)
        bad("neg", fn, q, pos, f(3, 5, 8), 0.07, *tail)
        bad("neg", fn, q, pos, f(4, 40), 0.07, *tail)
        bad("neg", fn, q, pos, f(4, 0, 8), 0.07, *tail)
        bad(" q", fn, f(4, 16)[:, ::2], pos, neg, 0.07, *tail)
        bad(" q", fn, q.double(), pos, neg, 0.07, *tail)
    gd = Guarded(dev, [(4, 8), (4, 8), (4, 5, 8)])
    bad("gout", ops.contrastive_bwd, q, pos, neg, 0.07, f(2), out=tuple(gd.views))
    bad("dneg", ops.contrastive_bwd, q, pos, neg, 0.07, g1, out=(gd.views[0], gd.views[1], gd.views[0]))
    # the C entry's own limits: E % 4, E > 1024, M > 16 return before launching
    for e, m in ((6, 5), (1028, 5), (8, 17)):
        gd2 = Guarded(dev, [(4, e), (4, e), (4, m, e)])
        with pytest.raises(ops.DcnError, match="contrastive_bwd"):
            ops.contrastive_bwd(f(4, e), f(4, e), f(4, m, e), 0.07, g1, out=tuple(gd2.views))
        assert gd2.untouched()
        with pytest.raises(ops.DcnError, match="contrastive_fwd"):
            ops.contrastive_fwd(f(4, e), f(4, e), f(4, m, e), 0.07)
    assert gd.untouched()
    # decode_boxes
    fb = Guarded(dev, [(2, 4)]); ib = Guarded(dev, [(2, 3)], torch.int32, IFILL)
    bad("outbox", ops.decode_boxes, ob, anchors, 416, out=(fb.views[0], ib.views[0]))
    bad("outbox", ops.decode_boxes, ob[:2], anchors, 256)
    bad("outbox", ops.decode_boxes, maps(2, 256, (3, 5)), anchors, 256)
    bad("anchors", ops.decode_boxes, ob, f(3, 3), 256)
    bad("size", ops.decode_boxes, ob, anchors, 260)
    bad("boxes", ops.decode_boxes, ob, anchors, 256, out=(f(2, 3), None))
    bad("cells", ops.decode_boxes, ob, anchors, 256, want_cells=True, out=(fb.views[0], ib.views[0].long()))
    assert fb.untouched() and ib.untouched()
    # box_iou
    bad("box2", ops.box_iou, f(4, 4), f(3, 4))
    bad("box2", ops.box_iou, f(3, 4), f(4, 4))
    bad("box1", ops.box_iou, f(4, 5), f(4, 5))
    bad("box2", ops.box_iou, f(4, 4), f(4, 4).double())
    # the C entries on a size that is no multiple of 32: nothing is launched, the outputs keep their prefill
    o3 = Guarded(dev, [(3,), (2, 2), (2, 8)])
    ptrs = lambda ts: ops._ptrs(ts)
    with pytest.raises(ops.DcnError, match="dense_loss_fwd"):
        lib().dense_loss_fwd(ptrs(ob), ptrs(sim), ptrs(sim), ptrs(sim), ti.data_ptr(), tf.data_ptr(), 250, 2, o3.views[2].data_ptr(),
                             o3.views[1].data_ptr(), o3.views[0].data_ptr(), _stream())
    gd = Guarded(dev, [(2, 15, g, g) for g in LR.grids(256)] + [(2, g, g) for g in LR.grids(256)] * 3)
    v = gd.views
    with pytest.raises(ops.DcnError, match="dense_loss_bwd"):
        lib().dense_loss_bwd(ptrs(ob), ptrs(sim), ptrs(sim), ptrs(sim), ti.data_ptr(), tf.data_ptr(), lse.data_ptr(), g3.data_ptr(), 250, 2,
                             ptrs(v[0:3]), ptrs(v[3:6]), ptrs(v[6:9]), ptrs(v[9:12]), _stream())
    ti_o = Guarded(dev, [(2, 4)], torch.int32, IFILL); tf_o = Guarded(dev, [(2, 4)])
    with pytest.raises(ops.DcnError, match="build_target"):
        lib().build_target(f(2, 4).data_ptr(), anchors.data_ptr(), 250, 2, ti_o.views[0].data_ptr(), tf_o.views[0].data_ptr(), _stream())
    td = Guarded(dev, [(2, 3, 5, g, g) for g in LR.grids(256)] + [(2, 5, g, g) for g in LR.grids(256)])
    with pytest.raises(ops.DcnError, match="target_dense"):
        lib().target_dense(ti.data_ptr(), tf.data_ptr(), 250, 2, ptrs(td.views[:3]), ptrs(td.views[3:]), _stream())
    with pytest.raises(ops.DcnError, match="decode_boxes"):
        lib().decode_boxes(ptrs(ob), anchors.data_ptr(), 250, 2, fb.views[0].data_ptr(), ib.views[0].data_ptr(), _stream())
    torch.cuda.synchronize()
    assert o3.untouched() and gd.untouched() and ti_o.untouched() and tf_o.untouched() and td.untouched() and fb.untouched() and ib.untouched()
