"""The references of the loss kernels (tests/loss_ref.py) and the shared case tables (tests/loss_cases.py), on the CPU: the references
agree in fp64 with oracle/train_oracle.py and oracle/dcnet_oracle.py (values, and gradients through autograd), every case tells exactly
the wrong variants it claims from the right answer (by more than the largest tolerance the margin cap allows, or in an exact output),
every variant is claimed by a case, the tables hold the shapes and the planted edges they are there for, and no decision of the
reference (best anchor, cell, hinge, arg-max) sits inside the guard band except the planted exact ones, so that the GPU tests on the same
inputs (test_loss_edges_gpu.py) can tell a subtly wrong kernel from a right one.  The last test keeps the reason for this suite on
record: a backward kernel without the softmax part of d(outbox) is all but invisible to the criterion of test_losses_gpu.py.  No GPU."""
import contextlib
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_cases as LC
import loss_ref as LR

F64, F32 = LR.F64, LR.F32


@contextlib.contextmanager
def _default_f64():
    """The oracle allocates with the default dtype: run it in fp64 throughout."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(F64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def _units(got, ref):
    e, exact = LR.err_units(got, ref[0], ref[1])
    return e if exact else float("inf")


# ---- the references against the oracle, in fp64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [32, 256, 416, 608])
def test_anchor_table_is_the_packages(size):
    from dcnet_amd import losses
    assert torch.equal(LR.scaled_anchors(size), losses.scaled_anchors(size, "cpu"))
    assert LR.ANCHORS[::-1] == losses.ANCHORS_FULL


@pytest.mark.parametrize("case", LC.TG_CASES, ids=str)
def test_target_reference_matches_oracle(case):
    """The oracle divides by the unrounded anchors and adds 1e-16 where the kernel holds floats: 2**-22 of the scale covers both."""
    from oracle import train_oracle as TO
    i = LC.target_inputs(case)
    ref = LC.target_refs(case)
    with _default_f64():
        box, gi, gj, bn, ctr = TO.build_target(torch.clamp(i.bbox.double(), 0, case.size - 1), case.size)
    ti = ref["ti"]
    assert ti[:, 0].tolist() == bn and ti[:, 1].tolist() == [int(x) for x in gi] and ti[:, 2].tolist() == [int(x) for x in gj]
    off, _ = LR.offsets(case.size)
    G = LR.grids(case.size)
    tf = torch.stack([box[b // 3][n, b % 3, :4, int(gj[n]), int(gi[n])] for n, b in enumerate(bn)])
    assert ti[:, 3].tolist() == [off[b // 3] + int(gj[n]) * G[b // 3] + int(gi[n]) for n, b in enumerate(bn)]
    assert _units(tf, ref["tf"]) <= 2.0 ** -22
    # the dense tensors: the reference scatter of the fp32 targets is the oracle's, rounded
    dbox, dctr = LR.target_dense(ti, ref["tf"][0].to(F32), case.size)
    for s in range(3):
        assert dbox[s].dtype == F32 and torch.equal(dbox[s][:, :, 4].double(), box[s][:, :, 4]) and torch.equal(dctr[s][:, 4].double(), ctr[s][:, 4])
        assert float((dbox[s].double() - box[s]).abs().max()) <= 1e-5 and float((dctr[s].double() - ctr[s]).abs().max()) <= 1e-5


@pytest.mark.parametrize("case", LC.DN_CASES, ids=str)
def test_dense_reference_matches_oracle_and_autograd(case):
    from oracle import train_oracle as TO
    i = LC.dense_inputs(case)
    n, size = case.n, case.size
    args = (i.outbox, i.sim, i.negsim, i.loc, i.ti, i.tf)
    f = LR.dense_fwd(*args, size, margin=0.1)
    with _default_f64():
        box, ctr = LR.target_dense(i.ti, i.tf, size)
        box, ctr = [b.double() for b in box], [c.double() for c in ctr]
        leaf = lambda ts: [t.double().requires_grad_(True) for t in ts]
        ob, sim, neg, loc = leaf(i.outbox), leaf(i.sim), leaf(i.negsim), leaf(i.loc)
        pred5 = [p.view(n, 3, 5, p.shape[2], p.shape[3]) for p in ob]
        gi, gj, bn = i.ti[:, 1].long(), i.ti[:, 2].long(), i.ti[:, 0].tolist()
        parts = torch.stack([TO.yolo_loss(pred5, box, gi, gj, bn), TO.rank_loss(sim, neg, ctr), TO.loc_loss(loc, ctr)])
        assert _units(parts.detach(), f["out"]) <= 1e-12, (parts, f["out"][0])
        for gup in LC.GUPS:
            for t in ob + sim + neg + loc:
                t.grad = None
            gu = torch.tensor(gup, dtype=F64)
            (parts * gu).sum().backward(retain_graph=True)
            b = LC.flatten(LR.dense_bwd(*args, f["lse"][0], gu, size, margin=0.1))
            for key, ts in (("d_outbox", ob), ("d_sim", sim), ("d_negsim", neg), ("d_loc", loc)):
                for s in range(3):
                    grad = ts[s].grad if ts[s].grad is not None else torch.zeros_like(ts[s])
                    assert _units(grad, b[f"{key}[{s}]"]) <= 1e-11, (key, s, gup)


@pytest.mark.parametrize("case", LC.CT_CASES, ids=str)
def test_contrastive_reference_matches_oracle_and_autograd(case):
    from oracle import train_oracle as TO
    i = LC.contrastive_inputs(case)
    with _default_f64():
        q, pos, neg = (t.double().requires_grad_(True) for t in (i.q, i.pos, i.neg))
        loss = TO._contrastive(F.normalize(q, dim=1), F.normalize(pos, dim=1), F.normalize(neg.permute(0, 2, 1), dim=1), LC.T32)
        ref = LR.contrastive_fwd(i.q, i.pos, i.neg, LC.T32)
        assert _units(loss.detach(), ref["loss"]) <= 1e-12
        if "Z" in case.plant or "z" in case.plant:
            return                                              # the oracle's norm has no gradient at 0; the clamp is tested on the device
        (loss * 100.0).backward()
        b = LR.contrastive_bwd(i.q, i.pos, i.neg, LC.T32, torch.tensor([100.0], dtype=F64))
        assert _units(q.grad, b["dq"]) <= 1e-11 and _units(pos.grad, b["dpos"]) <= 1e-11 and _units(neg.grad, b["dneg"]) <= 1e-11


def test_contrastive_clamp_is_a_constant_in_the_gradient():
    """With a zero q row every cosine is 0 whatever the other rows are: the loss is log(1 + M), and the reference's gradients are those of
    the loss with the clamped norm held at 1e-12f (finite, checked against a difference quotient of that very function)."""
    case = next(c for c in LC.CT_CASES if c.name == "R4-E252-M10")
    i = LC.contrastive_inputs(case)
    r = case.plant.index("Z")
    rows = LR.contrastive_fwd(i.q, i.pos, i.neg, LC.T32)["rows"][0]
    assert abs(float(rows[r]) - math.log(1 + case.m)) <= 1e-12
    b = LR.contrastive_bwd(i.q, i.pos, i.neg, LC.T32, torch.tensor([1.0], dtype=F64))
    assert bool(torch.isfinite(b["dq"][0]).all()) and float(b["dq"][0][r].abs().max()) > 1e6 and bool((b["dpos"][0][r] == 0).all())
    h = 1e-18
    q2 = i.q.double().clone(); q2[r, 3] += h
    d = (LR.contrastive_fwd(q2, i.pos, i.neg, LC.T32)["loss"][0] - LR.contrastive_fwd(i.q, i.pos, i.neg, LC.T32)["loss"][0]) / h
    assert abs(float(d) - float(b["dq"][0][r, 3])) <= 1e-4 * abs(float(d))


@pytest.mark.parametrize("case", [c for c in LC.DC_CASES if c.plant == "max"], ids=str)
def test_decode_reference_matches_oracle(case):
    from oracle import dcnet_oracle as O
    i = LC.decode_inputs(case)
    ref = LC.decode_refs(case)
    with _default_f64():
        boxes = O.decode_boxes([o.double() for o in i.outbox], case.size)
    assert _units(boxes, ref["boxes"]) <= 2.0 ** -22             # the oracle's anchors are not rounded to float


@pytest.mark.parametrize("case", LC.DECODE_NONFINITE + [c for c in LC.DC_CASES if c.plant in LC.DC_TIES], ids=str)
def test_decode_reference_orders_ties_and_non_finite_values_as_torch_max(case):
    i = LC.decode_inputs(case)
    conf = torch.cat([o.view(case.n, 3, 5, -1)[:, :, 4].reshape(case.n, -1) for o in i.outbox], 1)
    cells = LC.decode_refs(case)["cellinfo"]
    loc = conf.max(1)[1].tolist()
    for n in range(case.n):
        j = LR.first_max(conf[n].numpy())
        s, ch, cell = LC.conf_index(case.size, j)
        g = LR.grids(case.size)[s]
        assert cells[n].tolist() == [s * 3 + ch // 5, cell % g, cell // g]
        if i.expect is not None:
            assert j == i.expect[n]
        ties = LC.tie_indices(case, n)
        if ties:
            assert j == min(ties) and bool((conf[n, ties] == conf[n].max()).all()) and int((conf[n] == conf[n].max()).sum()) == len(ties)
        if case.plant == "all_equal":
            assert j == 0
        if case in LC.DECODE_NONFINITE:
            assert loc[n] == j                                  # torch.max itself: all -inf -> 0, a NaN -> the first NaN


@pytest.mark.parametrize("case", LC.BI_CASES, ids=str)
def test_box_iou_reference_matches_oracle(case):
    from oracle import dcnet_oracle as O
    i = LC.box_iou_inputs(case)
    ref = LC.box_iou_refs(case)
    assert _units(O.bbox_iou_xyxy(i.b1.double(), i.b2.double()), ref["iou"]) <= 1e-12


# ---- every wrong variant is caught by the cases that claim it ---------------------------------------------------------------------------
def _told(refs_of, case, letters):
    """The letters of the variants that change an exact output of refs_of(case, dt, var) or move an fp64 one past 8 max(r32, 2**-24)."""
    ref = refs_of(case, F64, {})
    r32 = LC.worst(ref, refs_of(case, F32, {}))
    assert all(v < float("inf") for v in r32.values()), [k for k, v in r32.items() if v == float("inf")]
    told = ""
    for letter in letters:
        w = LC.worst(ref, refs_of(case, F64, LC.VARIANTS[letter]))
        if any(not w[k] <= LC.cap_tol(r32[k]) for k in w):
            told += letter
    return "".join(sorted(told))


STAGES = dict(target=(LC.TG_CASES, LC.target_refs), dense=(LC.DN_CASES, LC.dense_refs), contrastive=(LC.CT_CASES, LC.contrastive_refs),
              decode=(LC.DC_CASES, LC.decode_refs), box_iou=(LC.BI_CASES, LC.box_iou_refs))


@pytest.mark.parametrize("stage,case", [(s, c) for s, (table, _) in STAGES.items() for c in table], ids=lambda v: str(v))
def test_cases_tell_their_variants(stage, case):
    assert _told(STAGES[stage][1], case, LC.STAGE_VARIANTS[stage]) == "".join(sorted(case.covers))


def test_every_variant_is_covered_by_a_named_case():
    assert set("".join(LC.STAGE_VARIANTS.values())) == set(LC.VARIANTS) and len(LC.VARIANTS) == 29
    for stage, (table, _) in STAGES.items():
        assert set("".join(c.covers for c in table)) == set(LC.STAGE_VARIANTS[stage]), stage
    big = [c for c in LC.DN_CASES if c.regime == "big"]
    assert big and all("h" in c.covers for c in big)            # only logits near +-90 overflow a sum of raw exponentials
    assert all("o" in c.covers for c in LC.DN_CASES if c.collide) and all("x" in c.covers for c in LC.DC_CASES if c.plant in LC.DC_TIES)
    assert all(("t" in c.covers) == (c.e > 768) for c in LC.CT_CASES)
    assert all(("r" in c.covers) == ("Z" in c.plant[:c.rows] or "z" in c.plant[:c.rows]) for c in LC.CT_CASES)


def test_the_tables_hold_the_required_shapes():
    T = LC.TG_CASES
    assert {c.size for c in T} == {32, 256, 416, 608} and {c.n for c in T} == {1, 63, 64, 65, 130}
    assert LR.grids(32) == [1, 2, 4]
    D = LC.DN_CASES
    assert {c.size for c in D} == {32, 64, 96, 256, 416} and sum(c.size == 416 for c in D) == 1 and {c.n for c in D} == {1, 2, 3, 5, 8}
    assert [LR.offsets(s)[1] for s in (32, 64, 96, 256, 416)] == [21, 84, 189, 1344, 3549]
    assert {c.regime for c in D} == {"randn", "big", "dominant", "equal"} and {c.sat for c in D} == {0, 30, 90}
    assert any(c.n % 2 == 1 and c.n > 1 for c in D) and any(c.n == 1 for c in D) and any(c.collide and c.n > 2 for c in D)
    assert LC.GUPS[0] == (1.0, 100.0, 1.0) and LC.GUPS[1] == (0.37, -2.5, 0.0)
    C = LC.CT_CASES
    assert {c.e for c in C} == {4, 8, 252, 256, 260, 512, 764, 768, 772, 1020, 1024} and {c.m for c in C} == {1, 5, 10, 16}
    assert {c.rows for c in C} == {1, 3, 4, 5, 1027} and all(c.rows <= 5 or (c.e, c.m) == (4, 1) for c in C)
    assert set("".join(c.plant[:c.rows] for c in C)) == set("INSZz-") and LC.CT_GUPS == (1.0, 100.0)
    Dc = LC.DC_CASES
    assert {c.size for c in Dc} == {32, 96, 256} and {c.n for c in Dc} == {1, 3, 9} and {c.plant for c in Dc} == {"max", *LC.DC_TIES}
    assert {c.plant for c in LC.DECODE_NONFINITE} == {"all_ninf", "one_nan", "nan_inf", "all_nan"}
    assert {c.n for c in LC.BI_CASES} == {1, 64, 65}
    big = next(c for c in LC.BI_CASES if c.n == 64)
    iou = LC.box_iou_refs(big)["iou"][0]
    assert abs(float(iou[0]) - 1) < 1e-12 and 0 < float(iou[1]) < 1 and iou[2:7].tolist() == [0.0] * 5 and bool((iou[7:] > 0).any())


# ---- the planted edges are where the tables say ----------------------------------------------------------------------------------------------
def test_target_tables_plant_their_edges():
    seen_bn, kinds = set(), set()
    for c in LC.TG_CASES:
        i = LC.target_inputs(c)
        r = LC.target_refs(c)
        ti, tf = r["ti"], r["tf"][0]
        G = torch.tensor(LR.grids(c.size))[ti[:, 0].long() // 3]
        assert bool((ti[:, 1] >= 0).all()) and bool((ti[:, 1] < G).all()) and bool((ti[:, 2] >= 0).all()) and bool((ti[:, 2] < G).all())
        seen_bn |= set(ti[:, 0].tolist()); kinds |= set(i.kinds)
        for n, kind in enumerate(i.kinds):
            if kind in LC.TG_EXACT_IOU:
                assert int(ti[n, 0]) == 0 and float(tf[n, 2 if kind != "zero_h" else 3]) == math.log(LR.EPS16_F)
                assert int(LC.target_refs(c, F64, dict(last_max=True))["ti"][n, 0]) == 8
            if kind == "boundary":
                assert float(tf[n, 0]) == 0.0 and float(tf[n, 1]) == 0.0
                assert bool((LC.target_refs(c, F32)["tf"][0][n, :2] == 0).all())       # exact in fp32 too
            if kind == "point":
                assert ti[n, 1:3].tolist() == [int(G[n]) - 1] * 2
            if kind == "far_edge":
                assert float(i.bbox[n, 2]) == c.size - 1 and int(ti[n, 1]) < int(G[n])
            if kind == "outside":
                assert float(i.bbox[n].min()) < 0 and float(i.bbox[n].max()) > c.size - 1
    assert seen_bn == set(range(9))
    assert kinds == {"anchor", "whole", "zero_w", "zero_h", "point", "outside", "far_edge", "boundary", "random"}
    c256 = next(c for c in LC.TG_CASES if c.size == 256 and c.n == 64)
    i = LC.target_inputs(c256)
    assert {int(LC.target_refs(c256)["ti"][n, 0]) // 3 for n, k in enumerate(i.kinds) if k == "boundary"} == {0, 1, 2}


def test_dense_tables_plant_their_edges():
    anchors, corners, combos, finest = set(), set(), set(), 0
    for c in LC.DN_CASES:
        i = LC.dense_inputs(c)
        n = c.n
        G = LR.grids(c.size)
        f = LR.dense_fwd(i.outbox, i.sim, i.negsim, i.loc, i.ti, i.tf, c.size)
        for k in range(n):
            bn, gi, gj, cell = i.ti[k].tolist()
            g = G[bn // 3]
            anchors.add(bn); finest += bn // 3 == 2
            if gi in (0, g - 1) and gj in (0, g - 1) and g > 1:
                corners.add((bn // 3, gi == 0, gj == 0))
            a1, a2 = LR._hinges(i.sim, i.negsim, i.ti, c.size, F64)[:2]
            combos.add((bool(a1[k] > 0), bool(a2[k] > 0)))
        cells = i.ti[:, 3].tolist()
        if c.collide:
            assert cells[0] == cells[n - 1] and (n == 2 or True)
        if c.collide and n > 2:
            assert any(cells[k] == cells[n - 1 - k] and k != n - 1 - k for k in range(n))
        if c.regime != "equal":
            conf = LR._conf(i.outbox, F64); loc = LR._flat(i.loc, F64)
            for x in (conf, loc):
                assert all(len(set(row.tolist())) == row.numel() for row in x)
        if c.regime == "big":
            assert float(LR._conf(i.outbox, F64).max()) > 89.0 and float(LR._conf(i.outbox, F64).abs().min()) >= 80.0
            assert not bool(torch.isfinite(LR.dense_fwd(i.outbox, i.sim, i.negsim, i.loc, i.ti, i.tf, c.size, F64, no_max=True)["lse"][0]).all())
        if c.regime == "equal":
            conf = LR._conf(i.outbox, F64)
            assert float((f["lse"][0][:, 0] - (conf[:, 0] + math.log(conf.shape[1]))).abs().max()) <= 1e-12
        if c.sat:
            t = LR._coords(i.outbox, i.ti, c.size, F32)
            assert bool((t[:, :2].abs() == c.sat).all())
            p = LR._sig(t[:, :2])
            assert c.sat != 90 or bool(((p == 0) | (p == 1)).all())              # expf overflows: exactly 0 or 1 in fp32
    assert anchors == set(range(9)) and finest >= 4
    assert corners == {(s, a, b) for s in range(3) for a in (True, False) for b in (True, False)}
    assert combos == {(True, True), (True, False), (False, True), (False, False)}


def test_decode_tables_plant_the_maximum_everywhere():
    seen, corners = set(), set()
    for c in LC.DC_CASES:
        if c.plant != "max":
            continue
        cells = LC.decode_refs(c)["cellinfo"]
        for sa, gi, gj in cells.tolist():
            g = LR.grids(c.size)[sa // 3]
            seen.add(sa)
            assert gi in (0, g - 1) and gj in (0, g - 1)
            corners.add((gi == 0, gj == 0))
    assert seen == set(range(9)) and len(corners) == 4
    thread = next(c for c in LC.DC_CASES if c.plant == "tie_thread")
    assert all(b - a == 256 for a, b in (LC.tie_indices(thread, n) for n in range(3)))
    lanes = next(c for c in LC.DC_CASES if c.plant == "tie_lanes")
    assert all(a // 64 == b // 64 and a // 256 == b // 256 for a, b in (LC.tie_indices(lanes, n) for n in range(3)))
    waves = next(c for c in LC.DC_CASES if c.plant == "tie_waves")
    assert len({(j % 256) // 64 for j in LC.tie_indices(waves, 0)}) == 3 and len({j // 256 for j in LC.tie_indices(waves, 0)}) == 1
    scales = next(c for c in LC.DC_CASES if c.plant == "tie_scales")
    assert all(LC.conf_index(scales.size, a)[0] != LC.conf_index(scales.size, b)[0] for a, b in (LC.tie_indices(scales, n) for n in range(3)))


# ---- the guard band, on the reference alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LC.TG_CASES, ids=str)
def test_no_target_decision_is_inside_the_guard_band(case):
    i = LC.target_inputs(case)
    gap, frac = LC.target_guard(case)
    for n, kind in enumerate(i.kinds):
        if kind in LC.TG_EXACT_IOU:
            assert float(gap[n]) == 0.0
        else:
            assert float(gap[n]) > LC.GUARD, (n, kind, float(gap[n]))
        if kind in LC.TG_EXACT_FRAC:
            assert bool((frac[n] == 0).all())
        else:
            assert bool((frac[n] > LC.GUARD).all()), (n, kind, frac[n].tolist())


@pytest.mark.parametrize("case", LC.DN_CASES, ids=str)
def test_no_hinge_is_inside_the_guard_band(case):
    h = LC.dense_guard(case)
    assert bool((h > LC.GUARD).all()) and bool((h > 0.01).all())          # planted at least 0.5 from the kink: never an argument of 0


@pytest.mark.parametrize("case", LC.DC_CASES, ids=str)
def test_no_decode_maximum_is_inside_the_guard_band(case):
    gap = LC.decode_gap(case)
    if case.plant in LC.DC_TIES:
        assert bool((gap == 0).all())
    else:
        assert bool((gap > LC.GUARD).all())


# ---- why this suite exists ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,n,seed,blind", [(256, 4, 0, ()), (416, 6, 1, (0,)), (256, 2, 2, (0,)), (416, 16, 3, (0, 1))])
def test_dropped_softmax_gradient_passes_the_old_criterion_and_fails_the_new(size, n, seed, blind):
    """Variant (n), a backward kernel that drops the softmax part of d(outbox), on the very inputs of
    test_losses_gpu.py::test_total_loss_and_gradients_match_oracle_on_device, against that test's criterion
    |err| < 2e-4 * max|grad of the tensor| + 1e-7.  In every scale that holds a positive cell at least 98.9 % of the non-zero
    gradient entries lie below that tolerance, the variant differs from the right gradient by more than it in at most 6 elements, and
    in the scales `blind` in none: there the old criterion passes a kernel that writes zeros.  The per-element criterion of this suite
    fails the variant in every scale."""
    from test_losses_gpu import _fake_outputs
    from dcnet_amd.utils.synth import synth_boxes
    out = _fake_outputs(n, size, seed)
    bbox = synth_boxes(n, size, seed=seed).float()
    tr = LR.target(bbox, LR.scaled_anchors(size), size)
    ti, tf = tr["ti"], tr["tf"][0].to(F32)
    fa = out["flang_attn"]
    neg = [torch.sum(fa.flip(0) * cf[:, :512], dim=1) for cf in out["corr_feat"]]
    args = (out["outbox"], out["sim_score"], neg, out["loc_score"], ti, tf)
    lse = LR.dense_fwd(*args, size)["lse"][0].to(F32)
    gup = torch.tensor(LC.GUPS[0], dtype=F32)
    right, r32, wrong = (LR.dense_bwd(*args, lse, gup, size, dt, **var)["d_outbox"] for dt, var in ((F64, {}), (F32, {}), (F64, dict(no_softmax=True))))
    with_positive = set((ti[:, 0] // 3).tolist())
    passed = []
    for s in range(3):
        g, err = right[s][0], (wrong[s][0] - right[s][0]).abs()
        old_tol = 2e-4 * max(float(g.abs().max()), 1e-6) + 1e-7
        if s in with_positive:
            nz = g != 0
            assert float((g.abs()[nz] < old_tol).sum()) >= 0.989 * int(nz.sum()) and int((err >= old_tol).sum()) <= 6
            if float(err.max()) < old_tol:
                passed.append(s)
        yard = LR.err_units(r32[s][0], *right[s])[0]
        assert not _units(wrong[s][0], right[s]) <= LC.cap_tol(yard)
    assert tuple(passed) == blind
