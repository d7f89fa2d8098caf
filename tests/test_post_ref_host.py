"""The fp64 / exact reference of the post-processing kernels (tests/post_ref.py) and the shared case tables (tests/post_cases.py), on the
CPU: the reference reproduces the fixtures captured from the original code, agrees with the stock-torch restatement where nothing is tied,
and every case of the tables tells the wrong variants it claims to cover from the right answer, so that the GPU tests on the same inputs
(test_post_edges_gpu.py) can tell a subtly wrong kernel from a right one.  No GPU."""
import os

import numpy as np
import pytest
import torch

import post_cases as PC
import post_ref as PR
import post_torch as PT
from dcnet_amd.utils.synth import synth_head_outputs

GOLD = os.path.join(os.path.dirname(__file__), "golden")
U = PR.U


def box_err(boxes, ref):
    return float((np.abs(np.asarray(boxes, np.float64) - ref.boxes) / ref.scale).max())


# ---- the fixtures of the original code ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [256, 416])
def test_reference_reproduces_the_fixtures(size):
    g = np.load(os.path.join(GOLD, f"post_S{size}.npz"))
    E, topk, n_items, nk = int(g["E"]), int(g["topk"]), int(g["n_items"]), int(g["num_frame_k"])
    refs = []
    for it in range(n_items):
        pred, feat = synth_head_outputs(size, E, 1000 * size + it)
        ratio, dw, dh, H, W = g[f"meta{it}"]
        f32 = lambda v: np.array([v], np.float32)
        r = PR.topk_ref([p.numpy() for p in pred], [f.numpy() for f in feat], size, topk, f32(ratio), f32(dw), f32(dh), np.array([[H, W]], np.int64))
        assert np.array_equal(r.cells[0], g[f"cells{it}"]) and np.array_equal(r.scores[0], g[f"scores{it}"])
        # the fixture's boxes went through eight fp32 roundings (exp, 1 + e, the quotient, + cell | exp, * anchor | the two differences,
        # / ratio; the products with the power-of-two stride and the halving are exact), each at most 2^-24 of the coordinate's scale
        err = np.abs(g[f"boxes{it}"][:, 0].astype(np.float64) - r.boxes[0]) / r.scale[0]
        print(f"S{size} item {it}: box err {err.max() / U:.2f} u")
        assert err.max() <= 8 * U
        refs.append(r)
    c = nk // 2
    for it in range(n_items):
        if f"fuse_idx{it}" not in g:
            continue
        inv = list(g[f"fuse_invalid{it}"])
        src = [it if frm in inv else it + o for o, frm in zip(range(-c, c + 1), range(nk))]
        valid = np.array([[frm not in inv for frm in range(nk)]])
        f = PR.fusion_ref(refs[it].feats, np.stack([refs[j].feats[0] for j in src])[None], np.stack([refs[j].scores[0] for j in src])[None], valid)
        assert not f.ambiguous.any()
        assert int(f.best[0]) == int(g[f"fuse_idx{it}"])
        # unit-norm rows: the E roundings of an fp32 similarity add up like a random walk, sqrt(E) 2^-24 sum |c r| <= sqrt(E) 2^-24 (E 2^-24
        # is the worst case no real sum attains); that moves a softmax weight by the same share of itself, twice (numerator and
        # denominator); exp, the quotient and the fused sum add eight roundings
        err = np.abs(g[f"fuse_scores{it}"].astype(np.float64) - f.fused[0]) / f.scale[0]
        print(f"S{size} item {it}: fused err {err.max() / U:.2f} u")
        assert err.max() <= (2 * E ** 0.5 + 8) * U


# ---- the stock-torch restatement --------------------------------------------------------------------------------------------------
def _torch_topk(case):
    ob, cf, size, k, ratio, dw, dh, hw = PC.topk_args(case)
    t = torch.from_numpy
    return PT.topk_candidates_torch([t(o) for o in ob], [t(np.ascontiguousarray(c)) for c in cf], size, k, t(ratio), t(dw), t(dh), t(hw))


@pytest.mark.parametrize("case", [c for c in PC.TOPK_CASES if c.kind in ("randn", "neg")], ids=str)
def test_reference_agrees_with_torch_on_tie_free_maps(case):
    ref = PC.topk_reference(case)
    boxes, score, feats, cells = _torch_topk(case)
    assert np.array_equal(cells.numpy(), ref.cells) and np.array_equal(score.numpy(), ref.scores) and np.array_equal(feats.numpy(), ref.feats)
    assert box_err(boxes.numpy(), ref) <= 16 * U              # (fp32 against fp64: the eight roundings above, twice over for a vendor exp)


@pytest.mark.parametrize("case", [c for c in PC.FUSION_CASES if c.plant == "-" and c.E > 1], ids=str)
def test_fusion_reference_agrees_with_torch(case):
    center, ref_, score, valid = PC.fusion_inputs(case)
    r = PC.fusion_reference(case)
    t = torch.from_numpy
    best, fused = PT.temporal_fusion_torch(t(center).double(), t(ref_).double(), t(score).double(), None if valid is None else t(valid))
    clean = ~(r.ambiguous | r.tied).any(-1)
    err = np.abs(fused.numpy() - r.fused)[clean]
    assert clean.any() and (err <= 1e-12 * np.maximum(r.scale[clean], 1e-300)).all()        # fp64 against fp64
    if clean.all() and case.valid != "all":
        assert np.array_equal(best.numpy(), r.best)


# ---- the tables ---------------------------------------------------------------------------------------------------------------------
def test_tables_cover_the_required_values():
    T, F, Bk = PC.TOPK_CASES, PC.FUSION_CASES, PC.BANK_CASES
    assert {c.size for c in T} == {32, 64, 256, 352} and {1, 5, 17, 64} <= {c.k for c in T} and {1, 40, 64, 96, 512} == {c.E for c in T}
    assert any(c.size == 32 and c.k == 63 for c in T)
    assert {c.kind for c in T} == {"randn", "neg", "quant", "equal", "planted"} and {c.layout for c in T} == {"nchw", "nhwc", "slice"}
    for size in (32, 64, 256, 352):                 # every size meets ties at the threshold
        assert {c.kind for c in T if c.size == size} & {"quant", "equal", "planted"}
    assert {c.R for c in F} == {1, 2, 4, 5, 32} and {c.K for c in F} == {1, 2, 5, 64} and {c.E for c in F} == {1, 40, 64, 512, 2048, 2112}
    assert {65, 130} <= {c.B for c in F} and {c.regime for c in F} == {"unit", "norm3", "sat"}
    assert {c.valid for c in F} == {"none", "some", "all"} and {c.plant for c in F} == {"-", "tie", "dup"}
    assert {c.n for c in Bk} == {1, 2, 9, 65} and any(c.n < c.R and c.n == 2 for c in Bk) and any(c.R % 2 == 0 for c in Bk)
    assert any(c.E > 2048 for c in Bk) and any(c.K == 64 for c in Bk) and any(c.K == 1 for c in Bk)
    for c in F:                                     # a case stays under a few MB
        assert c.B * c.R * c.K * c.E * 4 <= 4 << 20
    for v in PC.TOPK_VARIANTS:
        assert sum(v in c.covers for c in T) >= 2, v
    for v in PC.FUSION_VARIANTS:
        assert sum(v in c.covers for c in F + Bk) >= 2, v
    assert all(set(c.covers) <= set(PC.TOPK_VARIANTS) for c in T) and all(set(c.covers) <= set(PC.FUSION_VARIANTS) for c in F + Bk)
    assert not any(set(c.covers) & set("ij") for c in F)       # (the window is gathered by the bank form only)


@pytest.mark.parametrize("case", PC.TOPK_CASES, ids=str)
def test_topk_case_properties(case):
    ob, cf, size, k, ratio, dw, dh, hw = PC.topk_args(case)
    ref = PC.topk_reference(case)
    n = 3 * sum(g * g for g in PR.grids_of(size))
    for b in range(case.B):
        conf = PR.flat_conf(ob, b)
        assert conf.shape == (n,) and not np.isnan(conf).any() and not (np.signbit(conf) & (conf == 0)).any()
        # the general selection (threshold, ties, ranking) with the right rules is the stable sort
        assert np.array_equal(PR.select(conf, k), ref.idx[b]) and np.array_equal(ref.idx[b], PR.stable_order(conf)[:k])
        assert np.all(ref.scores[b][:-1] >= ref.scores[b][1:])
        thr = ref.scores[b, -1]
        slots = int((ref.scores[b] == thr).sum()); copies = int((conf == thr).sum())
        if case.kind == "equal":
            assert ref.idx[b].tolist() == list(range(k))
        if case.kind == "neg":
            assert (ref.scores[b] < 0).all()
        if case.kind == "planted":
            pos = PC.planted_positions(size)
            assert (conf[pos] == thr).all() and copies == len(pos) + 1 > slots == min(k, 3)
            seg = -(-n // PR.THREADS)
            assert pos[0] % seg == seg - 1 and pos[1] == pos[0] + 1 and pos[2] == n - 1
            assert [PR.unflatten(p, size)[0] for p in pos[3:]] == [0, 1, 2]
        if case.kind == "quant" and k < n:
            assert copies > slots
            if n > 1024:
                assert copies >= 24 and {PR.unflatten(int(i), size)[0] for i in np.nonzero(conf == thr)[0]} == {0, 1, 2}
    # the clamp clip: each of the four clamps engages for a selected candidate
    b = case.B - 1
    H, W = (float(v) for v in hw[b])
    raw, sc = ref.raw[b], ref.scale[b] * PC.ENGAGE
    assert (raw[:, 0] < -sc[:, 0]).any() and (raw[:, 1] < -sc[:, 1]).any() and (raw[:, 2] > W + sc[:, 2]).any() and (raw[:, 3] > H + sc[:, 3]).any()
    assert H >= 1 and W >= 1


def _topk_changed(ref, w):
    return (not np.array_equal(w.cells, ref.cells)) or (not np.array_equal(w.scores, ref.scores)) or box_err(w.boxes, ref) > PC.ENGAGE


def _fusion_changed(ref, w):
    """A wrong variant changes the answer: a fused score that the GPU test checks (no ambiguous triple) moves by far more than any
    tolerance (2^-12 of its scale against at most 8 max(r32, 2^-24)), or the winner moves."""
    clean = ~ref.ambiguous.any(-1)
    moved = np.abs(w.fused - ref.fused) > PC.ENGAGE * np.maximum(ref.scale, w.scale)
    return bool((moved & clean).any()) or not np.array_equal(w.best, ref.best)


@pytest.mark.parametrize("case", PC.TOPK_CASES, ids=str)
def test_topk_cases_tell_the_wrong_variants(case):
    ref = PC.topk_reference(case)
    assert not _topk_changed(ref, PR.topk_ref(*PC.topk_args(case)))
    for v in case.covers:
        assert _topk_changed(ref, PR.topk_ref(*PC.topk_args(case), **PC.TOPK_VARIANTS[v])), v


@pytest.mark.parametrize("case", PC.FUSION_CASES, ids=str)
def test_fusion_cases_tell_the_wrong_variants(case):
    ref = PC.fusion_reference(case)
    assert ref.ambiguous.mean() <= PC.AMBIGUITY_CAP
    assert not _fusion_changed(ref, PR.fusion_ref(*PC.fusion_inputs(case)))
    for v in case.covers:
        assert _fusion_changed(ref, PR.fusion_ref(*PC.fusion_inputs(case), **PC.FUSION_VARIANTS[v])), v
    if case.valid == "all":
        assert (ref.fused == 0).all() and (ref.scale == 0).all() and (ref.best == 0).all()
    if case.regime == "sat":
        assert ref.exact.any()
    if case.plant != "-":
        assert ref.tied.any()


@pytest.mark.parametrize("case", PC.BANK_CASES, ids=str)
def test_bank_cases_tell_the_wrong_variants(case):
    ref = PC.bank_reference(case)
    assert ref.ambiguous.mean() <= PC.AMBIGUITY_CAP
    feats, scores = PC.bank_inputs(case)
    assert not _fusion_changed(ref, PR.fusion_bank_ref(feats, scores, case.R))
    for v in case.covers:
        assert _fusion_changed(ref, PR.fusion_bank_ref(feats, scores, case.R, **PC.FUSION_VARIANTS[v])), v
    # the window of the bank form: a missing neighbour is the centre's own entry, invalid; the centre itself is always there
    src, valid = PR.bank_window(case.n, case.R)
    assert valid[:, case.R // 2].all() and (src[~valid] == np.nonzero(~valid)[0]).all()
    if case.n < case.R:
        assert not valid.all(1).any()
    if case.n == 1:
        assert valid.sum() == 1


def test_exact_entries_are_what_they_claim():
    """An entry the reference calls exact: its leading frame's weight is 1 to within 2^-180 in fp64, and the claimed value is that
    frame's referred score (first maximum), or 0 if the frame is invalid."""
    seen = 0
    for case in PC.FUSION_CASES:
        r = PC.fusion_reference(case)
        _, _, score, valid = PC.fusion_inputs(case)
        for b, c in zip(*np.nonzero(r.exact)):
            lead = int(r.sim[b, c].max(-1).argmax())
            ok = valid is None or bool(valid[b, lead])
            assert r.exact_value[b, c] == (score[b, lead, int(r.sim[b, c, lead].argmax())] if ok else 0)
            assert abs(r.fused[b, c] - float(r.exact_value[b, c])) <= 2.0 ** -180
            seen += 1
    assert seen > 20
