"""The post-processing kernels at their edges (csrc/post.hip: post_topk, post_fusion, post_argmax; csrc/video.hip: post_fusion_bank,
bank_argmax) against the exact / fp64 reference of tests/post_ref.py over the case tables of tests/post_cases.py: threshold ties that
straddle thread segments and scales, negative keys, n < 1024, a ragged last segment, k = 1 and k = 3 P, every clamp; the unstaged
E > 2048, even R, R = 1 and 32, K = 1 and 64, E = 1, n < R, all-invalid windows, exact ties of the per-frame maximum and of the fused
scores, and more than 64 windows.  test_post_ref_host.py shows on the CPU that these inputs tell twelve wrong variants from the right
answer."""
import numpy as np
import pytest
import torch

import post_cases as PC
import post_ref as PR
import post_torch as PT
from dcnet_amd import ops
from dcnet_amd import postprocess as PP

pytestmark = pytest.mark.gpu
U = PR.U


def _bits(t):
    a = t.detach().cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(xs, ys):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(xs, ys))


# ---- top-k --------------------------------------------------------------------------------------------------------------------------
def _topk_r32(case, ref):
    """The fp32 yardstick: tests/post_torch.py on the CPU, on the same box channels and letterbox meta.  Its confidence channel is replaced
    by a tie-free map whose top-k is the reference's selection in the reference's order (the boxes do not depend on the confidences), so
    that torch.topk's own tie order does not enter."""
    ob, cf, size, k, ratio, dw, dh, hw = PC.topk_args(case)
    ob = [o.copy() for o in ob]
    n = 3 * sum(g * g for g in PR.grids_of(size))
    for b in range(case.B):
        flat = np.full(n, -1.0, np.float32)
        flat[ref.idx[b]] = np.arange(k, 0, -1, dtype=np.float32)
        PC._set_flat_conf(ob, b, flat)
    t = torch.from_numpy
    boxes, _, _, cells = PT.topk_candidates_torch([t(o) for o in ob], [t(np.ascontiguousarray(c)) for c in cf], size, k, t(ratio), t(dw), t(dh),
                                                  t(hw))
    assert np.array_equal(cells.numpy(), ref.cells)
    return float((np.abs(boxes.numpy().astype(np.float64) - ref.boxes) / ref.scale).max())


@pytest.mark.parametrize("case", PC.TOPK_CASES, ids=str)
def test_topk_edges(dev, case):
    i = PC.topk_inputs(case)
    ref = PC.topk_reference(case)
    t = lambda a: torch.from_numpy(a).to(dev)
    outbox = [t(o) for o in i.outbox]
    corr = [PC.feature_view(t(f), case.layout, case.E) for f in i.feat_base]
    assert all(c.stride() == tuple(s // 4 for s in PC.feature_view(f, case.layout, case.E).strides) for c, f in zip(corr, i.feat_base))
    ratio, dw, dh, hw = t(i.ratio), t(i.dw), t(i.dh), t(i.frame_hw)
    out = PP.topk_candidates(outbox, corr, case.size, case.k, ratio, dw, dh, hw)
    boxes, score, feat, cells = out
    # the selection is integer work: every slot, the tied ones included, is the reference's
    assert np.array_equal(cells.cpu().numpy(), ref.cells)
    assert np.array_equal(_bits(score), ref.scores.view(np.uint32)) and np.array_equal(_bits(feat), ref.feats.view(np.uint32))
    # a batch is its clips one at a time; a second call is the first
    for b in range(case.B):
        one = PP.topk_candidates([o[b:b + 1] for o in outbox], [c[b:b + 1] for c in corr], case.size, case.k, ratio[b:b + 1], dw[b:b + 1],
                                 dh[b:b + 1], hw[b:b + 1])
        assert _same(one, [x[b:b + 1] for x in out]), b
    assert _same(PP.topk_candidates(outbox, corr, case.size, case.k, ratio, dw, dh, hw), out)
    # boxes per coordinate against fp64
    r32 = _topk_r32(case, ref)
    tol = PC.post_tol(r32)
    got = boxes.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    err = float((np.abs(got - ref.boxes) / ref.scale).max())
    print(f"POSTFIG topk {case}: err {err / U:.2f} u, r32 {r32 / U:.2f} u, ratio {err / max(r32, U):.2f}")
    assert err <= tol, (err, tol)
    # a coordinate past its clamp by more than the tolerance is exactly the clamp value
    H = i.frame_hw[:, 0].astype(np.float64)[:, None]; W = i.frame_hw[:, 1].astype(np.float64)[:, None]
    lim = tol * ref.scale
    engaged = 0
    for c, bound, past in ((0, 0.0, ref.raw[..., 0] < -lim[..., 0]), (1, 0.0, ref.raw[..., 1] < -lim[..., 1]),
                           (2, W, ref.raw[..., 2] > W + lim[..., 2]), (3, H, ref.raw[..., 3] > H + lim[..., 3])):
        assert past[case.B - 1].any(), c
        assert np.array_equal(got[..., c][past], np.broadcast_to(bound, past.shape)[past]), c
        engaged += int(past.sum())
    assert engaged >= 4


def test_topk_argument_checks(dev):
    z = lambda g: torch.zeros(1, 15, g, g, device=dev)
    f = lambda g: torch.zeros(1, 8, g, g, device=dev)
    one = torch.ones(1, device=dev); zero = torch.zeros(1, device=dev); hw = torch.full((1, 2), 32, device=dev)
    with pytest.raises(Exception, match="post_topk"):
        PP.topk_candidates([z(8), z(16), z(32)], [f(8), f(16), f(32)], 256, 65, one, zero, zero, hw)
    with pytest.raises(Exception, match="post_topk"):                     # top_k > 3 P = 63
        PP.topk_candidates([z(1), z(2), z(4)], [f(1), f(2), f(4)], 32, 64, one, zero, zero, hw)
    PP.topk_candidates([z(1), z(2), z(4)], [f(1), f(2), f(4)], 32, 63, one, zero, zero, hw)


# ---- fusion -------------------------------------------------------------------------------------------------------------------------
def _check_fusion(name, kernel, best, fused, r, center, ref_feat, ref_score, valid):
    """best (B,), fused (B,K) of a kernel against the reference r of the same (gathered) inputs."""
    got32 = fused.cpu().numpy(); got = got32.astype(np.float64); best = best.cpu().numpy()
    assert np.isfinite(got).all()
    t = torch.from_numpy
    _, f32 = PT.temporal_fusion_torch(t(center), t(ref_feat), t(ref_score), None if valid is None else t(valid))
    amb = r.ambiguous.any(-1)
    checked = ~amb & ~r.exact
    zero = r.scale == 0
    safe = np.where(zero, 1.0, r.scale)
    plain = checked & ~zero & ~r.tied.any(-1)                              # (torch may break an exact tie its own way)
    r32 = float((np.abs(f32.numpy().astype(np.float64) - r.fused) / safe)[plain].max()) if plain.any() else 0.0
    tol = PC.post_tol(r32)
    # exact entries (one frame leads by more than 128: its referred score, or 0 if it is invalid) and entries without a valid frame
    assert np.array_equal(got32[r.exact & ~amb].view(np.uint32), r.exact_value[r.exact & ~amb].view(np.uint32))
    assert (got32[zero & checked] == 0).all()
    err = float((np.abs(got - r.fused) / safe)[checked & ~zero].max()) if (checked & ~zero).any() else 0.0
    print(f"POSTFIG {kernel} {name}: err {err / U:.2f} u, r32 {r32 / U:.2f} u, ratio {err / max(r32, U):.2f}, "
          f"checked {int((checked & ~zero).sum())}, exact {int(r.exact.sum())}, ambiguous {int(amb.sum())}")
    assert err <= tol, (err, tol)
    # the winner: the first maximum of the kernel's own fused scores (exact duplicates give the lowest index), and the reference's
    # wherever the fp64 gap exceeds the tolerance; elsewhere one of those within it
    assert np.array_equal(best, got32.argmax(1))
    lim = np.where(r.exact, 0.0, tol * r.scale)
    f64 = np.where(r.exact, r.exact_value.astype(np.float64), r.fused)
    for b in range(got.shape[0]):
        top = int(f64[b].argmax())
        allowed = (f64[b] + lim[b] >= f64[b, top] - lim[b, top]) | amb[b]
        assert allowed[best[b]], (b, best[b], top)
        same_row = [c for c in range(int(best[b])) if np.array_equal(center[b, c], center[b, best[b]])]
        assert not same_row, (b, best[b], same_row)


@pytest.mark.parametrize("case", PC.FUSION_CASES, ids=str)
def test_fusion_edges(dev, case):
    center, ref_feat, score, valid = PC.fusion_inputs(case)
    r = PC.fusion_reference(case)
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    args = (t(center), t(ref_feat), t(score), t(valid))
    best, fused = PP.temporal_fusion(*args)
    _check_fusion(str(case), "fusion", best, fused, r, center, ref_feat, score, valid)
    if case.valid == "all":
        assert (fused == 0).all() and (best == 0).all()
    assert _same(PP.temporal_fusion(*args), (best, fused))


@pytest.mark.parametrize("case", PC.BANK_CASES, ids=str)
def test_bank_fusion_edges(dev, case):
    feats, scores = PC.bank_inputs(case)
    r = PC.bank_reference(case)
    src, valid = PR.bank_window(case.n, case.R)
    t = lambda a: torch.from_numpy(a).to(dev)
    best, fused = ops.post_fusion_bank(t(feats), t(scores), case.R)
    _check_fusion(str(case), "fusion_bank", best, fused, r, feats, feats[src], scores[src], valid)
    # bitwise the pair kernel on the gathered tensor: even R, n < R and n = 1 included
    pair = PP.temporal_fusion(t(feats), t(np.ascontiguousarray(feats[src])), t(np.ascontiguousarray(scores[src])), t(valid))
    assert _same(pair, (best, fused))
    assert _same(ops.post_fusion_bank(t(feats), t(scores), case.R), (best, fused))


def test_fusion_argument_checks(dev):
    z = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(Exception, match="post_fusion"):
        PP.temporal_fusion(z(1, 65, 8), z(1, 2, 65, 8), z(1, 2, 65))
    with pytest.raises(Exception, match="post_fusion"):
        PP.temporal_fusion(z(1, 2, 8), z(1, 33, 2, 8), z(1, 33, 2))
    with pytest.raises(Exception, match="post_fusion_bank"):
        ops.post_fusion_bank(z(3, 65, 8), z(3, 65), 3)
    with pytest.raises(Exception, match="post_fusion_bank"):
        ops.post_fusion_bank(z(3, 2, 8), z(3, 2), 33)
