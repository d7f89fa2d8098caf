"""The fp64 stage references of the cross-scale head tail (tests/head_ref.py) and the shared case tables (tests/head_cases.py), on the
CPU: every case tells the wrong variants it claims to cover from the right answer by more than the largest tolerance the margin cap
allows, no backward case has a ReLU pre-activation or a runner-up extreme within the guard band, and the stage references, composed in
order, reproduce the P x P reference form of test_tail_gpu.py and the fp64 autograd gradients of their own composition, so that the GPU
tests on the same inputs (test_head_edges_gpu.py) can tell a subtly wrong kernel from a right one.  No GPU."""
import pytest
import torch

import head_cases as HC
import head_ref as HR
from test_tail_gpu import _ref_head_tail

F64, F32 = HR.F64, HR.F32


# ---- every wrong variant is caught by the cases that claim it ---------------------------------------------------------------------------
def _told(refs_of, case, letters):
    """The letters of the variants that move some output of the composition refs_of(case, dt, var) past 8 max(r32, 2**-24) scale."""
    ref = refs_of(case, F64, {})
    r32 = HC.worst(ref, refs_of(case, F32, {}))
    assert all(v < float("inf") for v in r32.values()), [k for k, v in r32.items() if v == float("inf")]
    told = ""
    for letter in letters:
        var = HC.VARIANTS[letter]
        if not any(st in var for st in ref):
            continue
        w = HC.worst(ref, refs_of(case, F64, var))
        if any(w[k] > HC.cap_tol(r32[k]) for k in w):
            told += letter
    return "".join(sorted(told))


def _tail_refs(case, dt, var):
    out = HC.tail_forward_refs(case, dt, var)
    out.update(HC.tail_backward_refs(case, "all", None, dt, var))
    return out


ALL = "".join(sorted(HC.VARIANTS))


@pytest.mark.parametrize("case", HC.TAIL_CASES, ids=str)
def test_tail_cases_tell_their_variants(case):
    assert _told(_tail_refs, case, ALL) == "".join(sorted(case.covers))


@pytest.mark.parametrize("case", HC.LOCEMB_CASES, ids=str)
def test_locemb_cases_tell_their_variants(case):
    assert _told(lambda c, dt, var: HC.locemb_refs(c, None, dt, var), case, ALL) == "".join(sorted(case.covers))


@pytest.mark.parametrize("case", HC.LOCBN_CASES, ids=str)
def test_locbn_cases_tell_their_variants(case):
    assert _told(lambda c, dt, var: HC.locbn_refs(c, None, dt, var), case, ALL) == "".join(sorted(case.covers))


@pytest.mark.parametrize("case", HC.LOCMOD_CASES, ids=str)
def test_locmod_cases_tell_their_variants(case):
    assert _told(HC.locmod_refs, case, ALL) == "".join(sorted(case.covers))


def test_every_variant_is_covered_by_a_named_case():
    covered = set("".join(c.covers for t in (HC.TAIL_CASES, HC.LOCEMB_CASES, HC.LOCBN_CASES, HC.LOCMOD_CASES) for c in t))
    assert covered == set(HC.VARIANTS)
    # each mechanism of the ReLU mask and of the running statistics in both modules that have it
    assert any("l" in c.covers for c in HC.LOCEMB_CASES) and any("l" in c.covers for c in HC.LOCMOD_CASES)


def test_the_tables_hold_the_required_shapes():
    geo = {HC.geometry(c)[1] for c in HC.TAIL_CASES}
    assert geo == {3, 255, 256, 257, 1023, 1024, 1025, 2049, 8161, 8192}
    assert max(HC.geometry(c)[2] for c in HC.TAIL_CASES) == 8192 and HC.geometry(HC.TAIL_CASES[-2])[1:] == (8161, 8192)
    assert {c.B for c in HC.TAIL_CASES} == {1, 2, 5}
    lds = {tuple(ld for _, _, ld in c.scales) for c in HC.TAIL_CASES}
    assert (15, 15, 15) in lds and (32, 32, 32) in lds and any(len(set(l)) == 3 for l in lds)
    assert any(h != w for c in HC.TAIL_CASES for h, w, _ in c.scales)
    assert {c.plant for c in HC.TAIL_CASES} == {"-", "sim0", "const"} | set(HC.TIES)
    assert {c.P for c in HC.LOCMOD_CASES} == {1, 15, 16, 17, 63, 64, 65, 130, 3549} and {c.n for c in HC.LOCMOD_CASES if c.bwd} == {1, 3}
    assert all(c.n * c.P * 512 <= 1.3e5 for c in HC.LOCMOD_CASES if c.bwd)
    assert {c.training for c in HC.LOCEMB_CASES} == {True, False} == {c.training for c in HC.LOCBN_CASES}
    bad = HC.BAD_GEOMETRY["Ppad > 8192"]
    assert (sum(h * w for h, w, _ in bad) + 31) // 32 * 32 > 8192


# ---- guard bands -----------------------------------------------------------------------------------------------------------------------
def _band(v, s):
    """Elements of a pre-activation inside the guard band; a planted exact zero (every term of it is 0: scale 0) is exact in fp32 too."""
    return (v.abs() <= HC.GUARD * s) & (s > 0)


@pytest.mark.parametrize("case", [c for c in HC.LOCEMB_CASES if c.bwd], ids=str)
def test_locemb_backward_masks_are_clear_of_the_band(case):
    y, s = HC.locemb_refs(case)["locemb_bwd"]["y"]
    assert not bool(_band(y, s).any()), _band(y, s).nonzero()[:4]
    planted = int((s == 0).sum())
    assert planted == (case.P if case.plant == "const" else 0)
    if case.plant == "deadrow":
        assert bool((y[HC.locemb_inputs(case).dead] < 0).all())
        assert bool((HC.locemb_refs(case)["locemb_fwd"]["E8"][0][HC.locemb_inputs(case).dead] == 0).all())


@pytest.mark.parametrize("case", [c for c in HC.LOCMOD_CASES if c.bwd], ids=str)
def test_locmod_backward_masks_are_clear_of_the_band(case):
    v, s = HC.locmod_refs(case)["locmod_bwd"]["v"]
    assert not bool(_band(v, s).any()), _band(v, s).nonzero()[:4]
    assert int((s == 0).sum()) == (case.n * len(HC.ZERO_CH) if case.plant == "zero" else 0)
    dead = (v <= 0).all(2)
    if case.plant == "dead":
        assert bool(dead[0].all()) and bool(dead[:, 0].all()) and bool(dead[:, case.P - 1].all()) and not bool(dead.all())
    else:
        assert not bool(dead.any())


@pytest.mark.parametrize("case", HC.TAIL_CASES, ids=str)
def test_loc_map_extremes_are_planted_ties_or_clear_of_the_band(case):
    x = HC.tail_inputs(case).loc_map.double()
    mn, mx, imn, imx = HR.minmax_index(x)
    _, _, lmn, lmx = HR.minmax_index(x, "last")
    for b in range(case.B):
        vals = torch.unique(x[b])                                         # ascending
        n_mn, n_mx = int((x[b] == mn[b]).sum()), int((x[b] == mx[b]).sum())
        if case.plant == "const" and b == 0:
            assert vals.numel() == 1 and int(imn[b]) == int(imx[b]) == 0 and int(lmn[b]) == x.shape[1] - 1
            continue
        if case.plant in HC.TIES:
            (a0, a1), (b0, b1) = HC.TIES[case.plant]
            assert (int(imn[b]), int(lmn[b]), int(imx[b]), int(lmx[b])) == (a0, a1, b0, b1)
            assert n_mn == 2 and n_mx == len({b0, b1})
        else:
            assert n_mn == 1 and n_mx == 1
        assert float(vals[1] - vals[0]) > HC.GUARD * float(vals[1].abs() + vals[0].abs())
        assert float(vals[-1] - vals[-2]) > HC.GUARD * float(vals[-1].abs() + vals[-2].abs())


def test_planted_inputs_are_what_they_claim():
    c = next(c for c in HC.TAIL_CASES if c.plant == "sim0")
    r = HC.tail_forward_refs(c)["obj"]
    assert float(r["objn"][0][0]) == 0.0 and float(r["objn"][1][0]) == 0.0 and bool((r["X"][0].view(c.B, 8, -1)[0] == 0).all())
    assert float(r["objn"][0][1]) > 0.0
    c = next(c for c in HC.LOCEMB_CASES if c.plant == "const")
    i = HC.locemb_inputs(c)
    assert float(i.coord[:, HC.CONST_COL].std()) == 0.0
    ce = i.coord @ i.W.t() + i.b
    assert float(ce[:, HC.CONST_CH].std()) == 0.0                          # identical in fp32: the device's variance is the clamp's 0
    for c in HC.LOCBN_CASES:
        if c.plant == "zerocol":
            assert bool((HC.locbn_inputs(c).M[:, :, HC.ZERO_COL] == 0).all())
            if c.training:
                assert abs(float(HC.locbn_refs(c)["locbn_fwd"]["saved"][0][0, HC.ZERO_COL]) - HC.EPS ** -0.5) < 1e-9     # var == 0


@pytest.mark.parametrize("table,refs,stage", [(HC.LOCEMB_CASES, HC.locemb_refs, "locemb_fwd"), (HC.LOCBN_CASES, HC.locbn_refs, "locbn_fwd")],
                         ids=["locemb", "locbn"])
def test_running_statistics_are_judged_relative_to_the_update(table, refs, stage):
    """The retained part (1 - momentum) * old is at most the update wherever the update is not a zero-variance channel's, so the scale
    |retained| + |update| of the comparison is within a factor of two of the update term."""
    for case in (c for c in table if c.training):
        i = (HC.locemb_inputs if stage == "locemb_fwd" else HC.locbn_inputs)(case)
        r = refs(case)[stage]
        for key, old in (("rm", i.rm), ("rv", i.rv)):
            retained = ((1.0 - HC.MOMENTUM) * old.double()).abs()
            update = (r[key][0] - (1.0 - HC.MOMENTUM) * old.double()).abs()
            live = update > 1e-12
            assert int((~live).sum()) <= 1 and bool((retained[live] <= update[live]).all()), (case, key)
            if key == "rv":
                assert bool((r[key][1][live] <= 2.0 * update[live] * (1 + 1e-9)).all()), (case, key)


# ---- the stage references, composed, are the reference model -------------------------------------------------------------------------------
GRIDS = ((2, 3), (3, 4), (4, 5))


def _small(training, seed=5):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    B = 2
    P = sum(h * w for h, w in GRIDS)
    prm = dict(w_le=rn(8, 8) * 0.6, b_le=rn(8) * 0.1, g_le=1 + 0.2 * rn(8), be_le=0.3 * rn(8), w_lt=rn(512, P) / P ** 0.5, b_lt=rn(512) * 0.1,
               g_lt=1 + 0.2 * rn(512), be_lt=0.2 * rn(512))
    st = dict(rm_le=rn(8) * 0.2, rv_le=torch.rand(8, generator=g, dtype=F64) + 0.5, rm_lt=rn(512) * 0.02,
              rv_lt=torch.rand(512, generator=g, dtype=F64) * 0.01 + 0.005)
    logits = [rn(B, h, w, 17) for h, w in GRIDS]                          # NHWC, two pad channels
    sim = [rn(B, h, w) * 0.5 for h, w in GRIDS]
    q = torch.nn.functional.normalize(rn(B, 512), dim=1)
    coord = 2 * torch.rand(P, 8, generator=g, dtype=F64) - 1
    gout = [rn(B, 15, h * w) for h, w in GRIDS]; gloc = [rn(B, h * w) for h, w in GRIDS]; gonly = [rn(B, h * w) for h, w in GRIDS]
    return B, P, prm, st, logits, sim, q, coord, gout, gloc, gonly


def _compose_forward(B, P, p, st, logits, sim, q, coord, training):
    cnt = B * P
    le = HR.locemb_fwd(coord, p["w_le"], p["b_le"], p["g_le"], p["be_le"], st["rm_le"], st["rv_le"], training, cnt, 0.1, 1e-5)
    e8 = le["E8"][0]
    mom = HR.moments(e8)[0]
    ho = HR.head_obj(logits, [s.reshape(B, -1) for s in sim], e8)
    X = ho["X"][0]
    wp = HR.pad_rows(p["w_lt"], X.shape[1])["out"][0]
    M = (X @ wp.t()).view(B, 8, 512)
    bn = HR.locbn_fwd(M, mom, p["b_lt"], p["g_lt"], p["be_lt"], st["rm_lt"], st["rv_lt"], training, cnt, 0.1, 1e-5)
    loc_map = HR.locmod_fwd(e8, bn["Mp"][0], bn["bp"][0], q)["loc"][0]
    fin = HR.head_final_fwd(logits, [s.reshape(B, -1) for s in sim], loc_map)
    return dict(le=le, e8=e8, mom=mom, ho=ho, X=X, wp=wp, M=M, bn=bn, loc_map=loc_map, fin=fin)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_composed_stage_references_are_the_reference_form(training):
    B, P, prm, st, logits, sim, q, coord, gout, gloc, gonly = _small(training)
    leaf = lambda t: t.clone().requires_grad_(True)
    p = {k: leaf(v) for k, v in prm.items()}; lg = [leaf(t) for t in logits]; sg = [leaf(t) for t in sim]; qg = leaf(q)
    f = _compose_forward(B, P, p, st, lg, sg, qg, coord, training)
    # forward against the P x P form (its BatchNorm calls update the running statistics in place)
    st2 = {k: v.clone() for k, v in st.items()}
    ro, rl, rn_ = _ref_head_tail([t[..., :15].permute(0, 3, 1, 2).contiguous() for t in logits], sim, q, coord, prm, st2, training)
    close = lambda a, b: float((a.detach().reshape(-1) - b.detach().reshape(-1)).abs().max()) <= 1e-10 * max(1.0, float(b.abs().max()))
    for s in range(3):
        assert close(f["fin"][f"outbox{s}"][0], ro[s]) and close(f["fin"][f"loc{s}"][0], rl[s]) and close(f["ho"][f"only{s}"][0], rn_[s]), s
    if training:
        assert close(f["le"]["rm"][0], st2["rm_le"]) and close(f["le"]["rv"][0], st2["rv_le"])
        assert close(f["bn"]["rm"][0], st2["rm_lt"]) and close(f["bn"]["rv"][0], st2["rv_lt"])
    # gradients: fp64 autograd of the composed forward against the composed backward references
    loss = sum((f["fin"][f"outbox{s}"][0] * gout[s]).sum() + (f["fin"][f"loc{s}"][0] * gloc[s]).sum() + (f["ho"][f"only{s}"][0] * gonly[s]).sum()
               for s in range(3))
    leaves = lg + sg + [qg] + [p[k] for k in ("w_le", "b_le", "g_le", "be_le", "w_lt", "b_lt", "g_lt", "be_lt")]
    auto = torch.autograd.grad(loss, leaves, allow_unused=True)
    d = lambda t: t.detach()
    sims2 = [d(s).reshape(B, -1) for s in sim]
    fin, ho, bn, le = f["fin"], f["ho"], f["bn"], f["le"]
    loc = [d(fin[f"loc{s}"][0]) for s in range(3)]; only = [d(ho[f"only{s}"][0]) for s in range(3)]
    dloc_map = HR.head_dloc(logits, sims2, loc, gout, gloc, d(fin["mm"][0]), fin["imn"], fin["imx"])["dloc_map"][0]
    lb = HR.locmod_bwd(d(f["e8"]), d(bn["Mp"][0]), d(bn["bp"][0]), q, dloc_map)
    dE_a = lb["dE_part"][0].sum(0); dsum = lb["dsum"][0]
    bb = HR.locbn_bwd(d(f["M"]), d(f["mom"]), prm["b_lt"], prm["g_lt"], st["rm_lt"], d(bn["saved"][0]), dsum[:, :8], dsum[:, 8].sum(0), training,
                      B * P)
    dM2 = bb["dM"][0].reshape(B * 8, 512)
    dX = dM2 @ d(f["wp"]); dw_lt = (dM2.t() @ d(f["X"]))[:, :P]
    fo = HR.head_fold(dX, d(f["e8"]), d(ho["obj_map"][0]))
    dl = HR.head_dlogits(logits, sims2, loc, only, gout, gonly, d(ho["obj_map"][0]), d(ho["objn"][0]), fo["dobj_map"][0])
    g88 = HR.locemb_bwd(coord, prm["w_le"], prm["g_le"], prm["be_le"], d(le["xh"][0]), d(le["stat"][0]), dE_a, fo["dE8x"][0],
                        bb["dmom"][0] if training else None, training)["grads"][0]
    mine = [dl[f"dlogits{s}"][0].view_as(logits[s]) for s in range(3)] + [dl[f"dsim{s}"][0].view_as(sim[s]) for s in range(3)] + [dsum[:, 9]] \
        + [g88[:64].view(8, 8), g88[64:72], g88[72:80], g88[80:88], dw_lt, bb["out"][0][2], bb["out"][0][0], bb["out"][0][1]]
    for n, (a, b) in enumerate(zip(mine, auto)):
        b = torch.zeros_like(a) if b is None else b
        assert float((a - b).abs().max()) <= 1e-9 * max(1e-3, float(b.abs().max())), (n, float((a - b).abs().max()), float(b.abs().max()))
