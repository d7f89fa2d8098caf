"""The references of the correspondence-sampling kernels (tests/sample_ref.py) and the shared case tables (tests/sample_cases.py), on the
CPU: the Philox rounds reproduce the published known-answer vectors, the reference draws obey the sampler's rules, the reference CSR is
the host library's, every case tells exactly the wrong variants it claims from the right answer (by more than the largest tolerance the
margin cap allows, or in an exact output), no crossmap column sits inside the guard band except the planted ties, the selection agrees
with torch.topk, and the K14 references, composed, reproduce the torch restatement of test_tail_gpu.py and its fp64 autograd gradients,
so that the GPU tests on the same inputs (test_sample_edges_gpu.py) can tell a subtly wrong kernel from a right one.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sample_cases as SC
import sample_ref as SR

F64, F32 = SR.F64, SR.F32


# ---- the sampler ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,out", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, out):
    """Random123 kat_vectors, philox4x32 with 10 rounds."""
    assert SR.philox4x32_10(ctr, key) == out


@pytest.mark.parametrize("case", SC.SP_CASES, ids=str)
def test_reference_draws_obey_the_rules(case):
    r = SC.sampler_refs(case)
    n, hw = case.n, case.hw
    for s in range(case.steps):
        k9, k14 = r[f"k9@{s}"].numpy(), r[f"k14@{s}"].numpy()
        assert k9.shape == (n // 2, case.top_k, case.neg_n) and k9.min() >= 0 and k9.max() < hw - 1
        assert k14.shape == (n, hw, case.neg_c) and k14.min() >= 0 and k14.max() < hw
        for t in (k9, k14):
            st = np.sort(t, -1)
            assert (st[..., 1:] != st[..., :-1]).all()
        assert (k14[n - 1] != np.arange(hw)[:, None]).all()
    if case.steps > 1:
        assert not torch.equal(r["k14@0"], r["k14@1"])


def test_draws_fill_small_populations_and_split_the_streams():
    assert SR.draw(1, 1, 5, 0, 0) == [0]
    assert sorted(SR.draw(16, 16, 77, 7, 3)) == list(range(16))
    assert SR.draw(64, 5, 1, 2, 3) != SR.draw(64, 5, 1, 2, 0x80000000 + 3)
    assert SR.draw(64, 5, 1, 2 ** 32 + 2, 3) != SR.draw(64, 5, 1, 2, 3) == SR.draw(64, 5, 1, 2 ** 32 + 2, 3, step_lo=True)
    assert SR.draw(64, 5, 2 ** 32 + 1, 2, 3) != SR.draw(64, 5, 1, 2, 3)


@pytest.mark.parametrize("case", SC.SP_CASES, ids=str)
def test_reference_csr_is_the_host_librarys(case):
    from dcnet_amd.lib import lib
    r = SC.sampler_refs(case)
    k14 = np.ascontiguousarray(r["k14@0"].numpy())
    off = np.zeros(case.hw + 1, np.int32); src = np.zeros(k14.size, np.int32)
    lib().mt_sample_crossmodal_csr(k14.ctypes.data, case.n, case.hw, case.neg_c, off.ctypes.data, src.ctypes.data)
    assert np.array_equal(off, r["csr_off@0"].numpy()) and np.array_equal(src, r["csr_src@0"].numpy())


# ---- every wrong variant is caught by the cases that claim it ---------------------------------------------------------------------------
def _told(refs_of, case, letters):
    """The letters of the variants that change an exact output of refs_of(case, dt, var) or move an fp64 one past 8 max(r32, 2**-24)."""
    ref = refs_of(case, F64, {})
    r32 = SC.worst(ref, refs_of(case, F32, {}))
    assert all(v < float("inf") for v in r32.values()), [k for k, v in r32.items() if v == float("inf")]
    told = ""
    for letter in letters:
        w = SC.worst(ref, refs_of(case, F64, SC.VARIANTS[letter]))
        if any(not w[k] <= SC.cap_tol(r32[k]) for k in w):
            told += letter
    return "".join(sorted(told))


STAGES = dict(k9=(SC.K9_CASES, SC.k9_refs), colnorm=(SC.CN_CASES, SC.colnorm_refs), lagnorm=(SC.LN_CASES, SC.lagnorm_refs),
              crossmap=(SC.CM_CASES, SC.crossmap_refs), gather=(SC.GA_CASES, SC.gather_refs), dlag=(SC.DL_CASES, SC.dlag_refs),
              sampler=(SC.SP_CASES, SC.sampler_refs))


@pytest.mark.parametrize("stage,case", [(s, c) for s, (table, _) in STAGES.items() for c in table], ids=lambda v: str(v))
def test_cases_tell_their_variants(stage, case):
    assert _told(STAGES[stage][1], case, SC.STAGE_VARIANTS[stage]) == "".join(sorted(case.covers))


def test_every_variant_is_covered_by_a_named_case():
    assert set("".join(SC.STAGE_VARIANTS.values())) == set(SC.VARIANTS)
    for stage, (table, _) in STAGES.items():
        assert set("".join(c.covers for c in table)) == set(SC.STAGE_VARIANTS[stage]), stage
    assert any("j" in c.covers for c in SC.CN_CASES) and any("j" in c.covers for c in SC.LN_CASES) and any("j" in c.covers for c in SC.DL_CASES)
    assert any("h" in c.covers for c in SC.CN_CASES) and any("h" in c.covers for c in SC.LN_CASES)


def test_the_tables_hold_the_required_shapes():
    K = SC.K9_CASES
    assert {c.hw for c in K} >= {2, 32, 33, 46} and {c.e for c in K} == {4, 260, 512} and {c.top_k for c in K} >= {1, 4, 30, 64}
    assert any(c.top_k == c.hw * c.hw for c in K) and any(c.pairs == 3 for c in K)
    assert {0, 1} <= {c.neg_n for c in K} and any(c.neg_n == c.hw - 1 for c in K)
    assert {c.hw for c in SC.CN_CASES} == {1, 3, 4, 5, 28, 29, 32, 33, 36, 37, 61} and {c.e for c in SC.CN_CASES} == {4, 64, 68, 100}
    assert {c.n for c in SC.CN_CASES} == {1, 3} and {c.extra for c in SC.CN_CASES} == {True, False}
    assert {(c.n_extra == 0, c.n) for c in SC.CN_CASES if c.extra} == {(True, 1), (True, 3), (False, 3)}
    assert {c.L for c in SC.LN_CASES} == {1, 20, 32} and {c.e for c in SC.LN_CASES} == {4, 256, 300}
    assert {(c.L, c.hw, c.e) for c in SC.CM_CASES if c.plant == "-"} == {(1, 1, 4), (3, 2, 8), (20, 64, 260), (20, 30, 1024), (5, 9, 1028),
                                                                         (2, 5, 2048), (4, 1030, 8), (32, 413, 4)}
    assert (32 * 415 + 32 * 32 * 3 + 32) * 4 == 64 * 1024
    assert {(c.n, c.hw) for c in SC.GA_CASES} == {(1, 1), (3, 5), (2, 7)} and {c.neg_n for c in SC.GA_CASES} == {1, 5}
    assert {c.L for c in SC.DL_CASES} == {1, 32} and {c.hw for c in SC.DL_CASES} == {1, 9, 40} and {c.e for c in SC.DL_CASES} == {4, 100, 130}
    big = next(c for c in SC.DL_CASES if c.hw == 40)
    assert {0, 7, 8, 9} <= set(np.bincount(SC.dlag_inputs(big).cols[0].numpy(), minlength=32).tolist())
    assert {c.hw for c in SC.KB_CASES} == {1, 16, 17} and all(c.e == 516 for c in SC.KB_CASES) and any(c.neg_n == 0 for c in SC.KB_CASES)
    assert max(c.top_k * (1 + c.neg_n) for c in SC.KB_CASES) == 960 and (960 * 17 + 16) * 4 == 65344
    assert {(c.n, c.hw, c.top_k, c.neg_n, c.neg_c) for c in SC.SP_CASES} == {(2, 2, 1, 1, 1), (2, 17, 3, 16, 16), (4, 65, 5, 10, 5),
                                                                            (4, 64, 30, 10, 5), (6, 13, 2, 3, 2), (2, 131, 1, 1, 1)}
    assert any(c.step + c.steps > 2 ** 32 and c.steps == 3 for c in SC.SP_CASES) and sum(c.seed >> 32 != 0 for c in SC.SP_CASES) >= 3


def test_k9_raw_positions_hit_their_edges():
    """Over the table: raw == k, k == 0, k == HW-1 and raw == HW-2 each occur with a negative drawn, and a tie plateau is cut inside
    a thread's segment."""
    seen = set()
    for c in SC.K9_CASES:
        if not c.neg_n:
            continue
        i = SC.k9_inputs(c); k = (SC.k9_refs(c)["index"] % c.hw).unsqueeze(2).expand_as(i.raw)
        assert int(i.raw.min()) >= 0 and int(i.raw.max()) <= c.hw - 2
        seen |= {n for n, m in (("raw==k", i.raw == k), ("k==0", k == 0), ("k==HW-1", k == c.hw - 1), ("raw==HW-2", i.raw == c.hw - 2),
                                ("raw==k-1", i.raw == k - 1)) if bool(m.any())}
    assert seen == {"raw==k", "k==0", "k==HW-1", "raw==HW-2", "raw==k-1"}
    span = next(c for c in SC.K9_CASES if c.kind == "plateau_span")
    assert SC.k9_refs(span)["index"][0, -7:].tolist() == list(range(50, 57))
    inseg = next(c for c in SC.K9_CASES if c.kind == "plateau_in")
    assert SC.k9_refs(inseg)["index"][0, -1].item() == 301
    zeros = next(c for c in SC.K9_CASES if c.kind == "signed_zero")
    x = SC.k9_inputs(zeros).cmap[0]
    assert SC.k9_refs(zeros)["index"][0, -1].item() == 10 and bool(torch.signbit(x[10])) and not bool(torch.signbit(x[20]))
    low = next(c for c in SC.K9_CASES if c.kind == "lowbyte0")
    x = SC.k9_inputs(low).cmap[0]
    assert int(x[SC.k9_refs(low)["index"][0, -1]].view(torch.int32)) & 0xFF == 0
    b16 = SC.k9_inputs(next(c for c in SC.K9_CASES if c.kind == "bits16")).cmap.view(torch.int32)
    assert int(b16.min()) >> 16 == int(b16.max()) >> 16


@pytest.mark.parametrize("case", SC.K9_CASES, ids=str)
def test_selection_agrees_with_torch_topk(case):
    i = SC.k9_inputs(case)
    index = SC.k9_refs(case)["index"]
    tv, ti = i.cmap.topk(case.top_k, dim=1, largest=True, sorted=True)
    assert bool((torch.gather(i.cmap, 1, index) == tv).all())
    for b in range(case.pairs):
        head = i.cmap[b].sort(descending=True)[0][:case.top_k + 1]
        if bool((head[1:] != head[:-1]).all()):
            assert torch.equal(index[b], ti[b])


# ---- the guard band of the arg-max ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.CM_CASES, ids=str)
def test_no_crossmap_column_is_inside_the_guard_band(case):
    gap = SC.crossmap_gap(case)
    cols = SC.crossmap_refs(case)["cols"]
    if case.plant == "zero":
        assert bool((gap == 0).all()) and bool((cols == 0).all())
        return
    if case.plant == "tie":
        tied = gap == 0
        assert bool(tied.any()) and bool((cols[tied] == SC.TIE_A).all()) and bool((SC.crossmap_refs(case, F64, dict(last_max=True))["cols"][tied] == SC.TIE_B).all())
        gap = gap[~tied]
    print(f"{case}: smallest top-2 gap {float(gap.min()) / SC.GUARD:.1f} GUARD" if gap.numel() else f"{case}: every column tied")
    assert bool((gap > SC.GUARD).all())


# ---- the pure sums ------------------------------------------------------------------------------------------------------------------------
def test_sequential_fp32_sums_are_within_their_bound_of_the_fp64_sums():
    """A sum of m terms added one at a time in fp32 is within (m - 1) 2**-24 of the sum of the absolute terms."""
    for c in SC.KB_CASES:
        i = SC.k9_bwd_inputs(c)
        r64, r32 = SR.k9_bwd(i.index, i.neg_idx, i.d_frame, i.d_corr, i.d_neg, c.hw)
        m = c.top_k * (1 + c.neg_n)
        assert float((r32.double() - r64).abs().max()) <= m * SR.U * float(torch.cat([i.d_frame.flatten(), i.d_neg.flatten()]).abs().max()) * m
    for c in SC.NS_CASES:
        i = SC.negscatter_inputs(c)
        r64, r32 = SR.k14_negscatter(i.d_neg, i.off, i.src, i.hw)
        assert bool((r64[0] == 0).all()) and bool((r64[-1] == 0).all()) and torch.equal(r64[1], i.d_neg[i.src[0]].double())
        assert float((r32.double() - r64).abs().max()) <= 17 * SR.U * 17 * float(i.d_neg.abs().max())
        assert sorted(i.src.tolist()) == list(range(i.d_neg.shape[0]))
    for c in SC.DL_CASES:
        i = SC.dlag_inputs(c)
        r64, r32 = SR.k14_word_sums(i.cols, i.d_k, c.L)
        assert float((r32.double() - r64).abs().max()) <= c.hw * SR.U * c.hw * float(i.d_k.abs().max())
        assert float((r64 - SR.k14_dlag(torch.zeros_like(i.lag), torch.ones_like(i.lnorm), i.cols, i.d_k)["dctx"][0][:, :, 0::2]).abs().max()) <= 1e-12


# ---- the composed K14 reference against stock torch ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hw,L,e", [(3, 25, 6, 32), (1, 7, 3, 8)])
def test_composed_k14_reference_matches_torch_and_autograd(n, hw, L, e):
    g = torch.Generator().manual_seed(n * 3 + hw)
    neg_n = 5
    fv = F.normalize(torch.randn(n, hw, e, generator=g), dim=2)
    ctx = torch.randn(n, L, 2 * e, generator=g)
    cw = torch.randn(L, L, 3, generator=g) * 0.2; cb = torch.randn(L, generator=g) * 0.1
    neg = torch.randint(0, hw, (n, hw, neg_n), generator=g)
    # the restatement of test_crossmodal_sampling_matches_torch
    fd, cd = fv.double().requires_grad_(True), ctx.double().requires_grad_(True)
    r_vit = F.normalize(fd.permute(0, 2, 1), dim=2).permute(0, 2, 1)
    r_lag = F.normalize(cd[:, :, 0::2], dim=1)
    lv = F.conv1d(torch.bmm(r_lag, r_vit.transpose(1, 2)), cw.double(), cb.double(), padding=1)
    cols = lv.argmax(1)
    ar = torch.arange(n)
    r_lp = r_lag[ar.unsqueeze(1), cols].unsqueeze(2); r_nc = r_vit[n - 1][neg]
    # the stage references, composed in the order of CrossModalSample
    cn = SR.colnorm_fwd(fv); ln = SR.lagnorm_fwd(ctx)
    vit, lag = cn["vit"][0], ln["lag"][0]
    cm = SR.crossmap(lag, vit, cw, cb)
    ga = SR.k14_gather(lag, vit, cm["cols"], neg)
    close = lambda a, b, tol: float((a.detach() - b.detach()).abs().max()) <= tol
    assert close(vit, r_vit, 1e-10) and close(lag, r_lag, 1e-10) and close(cm["lvmap"][0], lv, 1e-10)
    assert torch.equal(cm["cols"], cols) and close(ga["lag_pos"], r_lp, 1e-10) and close(ga["neg_cross"], r_nc, 1e-10)
    g1, g2, g3 = (torch.randn(t.shape, generator=g).double() for t in (r_vit, r_lp, r_nc))
    ((r_vit * g1).sum() + (r_lp * g2).sum() + (r_nc * g3).sum()).backward()
    off, src = SR.csr(neg.numpy(), hw)
    extra = SR.k14_negscatter(g3, torch.from_numpy(off), torch.from_numpy(src), hw)[0]
    dv = SR.colnorm_bwd(vit, cn["cnorm"][0], g1, extra, n - 1)["dv"][0]
    dctx = SR.k14_dlag(lag, ln["lnorm"][0], cm["cols"], g2)["dctx"][0]
    assert close(dv, fd.grad, 1e-9) and close(dctx, cd.grad, 1e-9)
