"""GPU: tube linking (dcnet_amd/csrc/tube.hip, postprocess.nms_keep / link_tubes, VideoGrounder(link=...)) against the fp64 numpy
reference of tests/tube_ref.py.  The inputs and what makes them decisive (margins, planted optima, wrong variants that fail these
criteria) are checked on the CPU by tests/test_tube_host.py.

Tolerances (u = 2^-24, the unit roundoff of fp32; unit-norm features, scores in (0,1), IoU in [0,1]):
  W      an fp32 dot product of E terms in any order is within (E - 1 + small) u sum|a_e b_e| of the exact one, the IoU takes at most
         8 roundings of values <= 1, the two products and the sum of the terms 2 more relative ones:
         |W - W64| <= u (8 w_iou + (E + 8) w_feat sum|a_e b_e| + 2 |W64|) per element.
  path   with M = 1 + w_iou + w_feat every delta is at most n M; a step rounds one add of W, one add of the unary score (2 u n M) and
         reads a W that is off by eps_W = the bound above at sum|a_e b_e| = 1, |W64| <= M.  So every delta_t, and the value the device
         assigns to any path, is within n (2 u n M + eps_W) of its fp64 value: ``score`` is that close to the fp64 optimum, and
         the fp64 value of the returned path is within twice that of the optimum."""
import numpy as np
import pytest
import torch

import tube_ref as R

pytestmark = pytest.mark.gpu


def _up(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _link(c, dev, keep=True, w=(1.0, 1.0), feats=True):
    from dcnet_amd import postprocess
    return postprocess.link_tubes(_up(c["boxes"], dev), _up(c["unary"], dev), _up(c["feats"], dev) if feats else None,
                                  _up(c["keep"], dev) if keep else None, w[0], w[1])


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", R.THRS)
@pytest.mark.parametrize("B,k", R.NMS_SHAPES)
def test_nms_equals_the_reference_exactly(dev, B, k, thr):
    """Every within-frame IoU is 1e-4 away from the threshold and the fp32 IoU is within 1e-6 of the fp64 one: the mask is exact.
    The last two rows are zero-area boxes (all kept) and a row with inverted boxes.  Written into a view of a larger buffer."""
    from dcnet_amd import ops, postprocess
    boxes = R.nms_case(B, k)
    want = torch.from_numpy(R.nms_batch(boxes, thr).astype(np.uint8))
    n = boxes.shape[0]
    buf = torch.full((n + 5, k), 0xAB, dtype=torch.uint8, device=dev)
    out = ops.post_nms(_up(boxes, dev), thr, out=buf[2:2 + n])
    assert out.data_ptr() == buf[2:].data_ptr()
    assert torch.equal(buf[2:2 + n].cpu(), want)
    assert bool((buf[:2] == 0xAB).all()) and bool((buf[2 + n:] == 0xAB).all())
    got = postprocess.nms_keep(_up(boxes, dev), thr)
    assert got.dtype == torch.bool and torch.equal(got.cpu(), want.bool())
    assert bool(got[:, 0].all()) and bool(got[B].all())


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w_iou,w_feat", R.TRANS_WEIGHTS)
@pytest.mark.parametrize("Q,n,k,E", R.TRANS_SHAPES)
def test_transitions_against_fp64(dev, Q, n, k, E, w_iou, w_feat):
    from dcnet_amd import ops
    c = R.gen_batch([5000 + 10 * n + q for q in range(Q)], n, k, E)
    use_feats = w_feat > 0
    boxes, feats = _up(c["boxes"], dev), _up(c["feats"], dev) if use_feats else None
    W = torch.full((Q, n, k, k), float("nan"), device=dev)
    ops.tube_transitions(boxes, feats, 0, n, w_iou, w_feat, W)
    assert bool(torch.isnan(W[:, 0]).all()), "the row of frame 0 is not written"
    W = W.cpu().numpy().astype(np.float64)
    worst = 0.0
    for q in range(Q):
        W64, S = R.transitions(c["boxes"][q], c["feats"][q] if use_feats else None, w_iou, w_feat)
        bound = R.w_bound(W64, S, E, w_iou, w_feat)
        err = np.abs(W[q, 1:] - W64[1:])
        worst = max(worst, float((err / bound[1:]).max()))
        assert np.all(err <= bound[1:]), (q, float(err.max()), float(bound[1:].min()))
    print(f"transitions {(Q, n, k, E)} w=({w_iou},{w_feat}): worst error / bound = {worst:.3f}")
    # a sub-range lands at the front of its workspace and equals the rows of the full run bit for bit
    if n >= 4:
        part = ops.tube_transitions(boxes, feats, 2, 4, w_iou, w_feat)
        full = ops.tube_transitions(boxes, feats, 0, n, w_iou, w_feat)
        assert part.shape == (Q, 2, k, k) and torch.equal(part, full[:, 2:4])


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_keep", [False, True])
@pytest.mark.parametrize("Q,n,k,E", R.PATH_SHAPES)
def test_path_value_against_the_fp64_optimum(dev, Q, n, k, E, with_keep):
    c = R.path_case(Q, n, k, E)
    path, score, tube_boxes = _link(c, dev, keep=with_keep)
    assert path.shape == (Q, n) and path.dtype == torch.int64 and score.shape == (Q,) and tube_boxes.shape == (Q, n, 4)
    path, score = path.cpu().numpy(), score.cpu().numpy().astype(np.float64)
    slack = R.path_slack(n, E, 1.0, 1.0)
    for q in range(Q):
        assert path[q].min() >= 0 and path[q].max() < k
        keep = c["keep"][q] if with_keep else None
        if with_keep:
            assert keep[np.arange(n), path[q]].all(), "a suppressed candidate on the path"
        W64, _ = R.transitions(c["boxes"][q], c["feats"][q], 1.0, 1.0)
        _, opt, _ = R.viterbi(c["unary"][q], W64, keep)
        val = R.path_value(path[q], c["unary"][q], W64)
        print(f"path {(Q, n, k, E)} keep={with_keep} q={q}: optimum - value = {opt - val:.3e} (slack {slack:.3e}), "
              f"|score - optimum| = {abs(score[q] - opt):.3e}")
        assert val >= opt - slack
        assert abs(score[q] - opt) <= slack / 2
        assert np.array_equal(tube_boxes[q].cpu().numpy(), c["boxes"][q][np.arange(n), path[q]])


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def test_exact_paths_brute_force_batch(dev):
    c = R.brute_cases()
    path, score, _ = _link(c, dev)
    assert np.array_equal(path.cpu().numpy(), c["best"])
    assert np.all(np.abs(score.cpu().numpy() - c["value"]) <= R.path_slack(R.BRUTE_SHAPE[0], R.BRUTE_SHAPE[2], 1.0, 1.0) / 2)


@pytest.mark.parametrize("i", range(len(R.PLANTED)))
def test_exact_paths_planted_tracks(dev, i):
    v = R.planted_case(i)
    c = {key: v[key][None] for key in ("boxes", "unary", "feats")}
    path, _, tube_boxes = _link(c, dev, keep=False)
    assert np.array_equal(path[0].cpu().numpy(), v["slots"])
    assert np.array_equal(tube_boxes[0].cpu().numpy(), v["boxes"][np.arange(len(v["slots"])), v["slots"]])


def test_exact_ties_resolve_to_the_lowest_index(dev):
    """Candidates 5 ... 9 are bit-for-bit copies of 0 ... 4: equal inputs give equal bits at every step, so the lowest-index rule
    never lets a copy onto the path, and path and score are those of the five originals alone."""
    c = {key: v[None] for key, v in R.tie_case().items()}
    path, score, _ = _link(c, dev, keep=False)
    assert int(path.max()) < 5
    half = {key: v[:, :, :5] for key, v in c.items()}
    path5, score5, _ = _link(half, dev, keep=False)
    assert torch.equal(path, path5) and torch.equal(score, score5)
    W64, _ = R.transitions(half["boxes"][0], half["feats"][0], 1.0, 1.0)
    assert np.array_equal(path5[0].cpu().numpy(), R.viterbi(half["unary"][0], W64)[0])


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def test_ranges_do_not_change_the_result(dev, monkeypatch):
    from dcnet_amd import ops
    Q, n, k, E = R.PATH_SHAPES[1]
    c = R.path_case(Q, n, k, E)
    assert ops.tube_ranges(Q, n, k) == [(0, n)]
    path, score, _ = _link(c, dev)
    for per in (1, 3):
        monkeypatch.setattr(ops, "TUBE_WS_BYTES", per * Q * k * k * 4)
        assert [t1 - t0 for t0, t1 in ops.tube_ranges(Q, n, k)] == [per] * (n // per) + ([n % per] if n % per else [])
        p2, s2, _ = _link(c, dev)
        assert torch.equal(p2, path) and torch.equal(s2, score), per


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def test_queries_are_independent(dev):
    Q, n, k, E = 3, 9, 20, 64
    c = R.gen_batch([6100, 6200, 6300], n, k, E)
    c["keep"] = R.nms_batch(c["boxes"], 0.6)
    perm = [2, 0, 1]
    path, score, tube_boxes = _link(c, dev)
    p2, s2, b2 = _link({key: v[perm] for key, v in c.items()}, dev)
    assert torch.equal(p2, path[perm]) and torch.equal(s2, score[perm]) and torch.equal(b2, tube_boxes[perm])
    assert len({tuple(r) for r in path.cpu().tolist()}) > 1


def test_precision_mode_does_not_change_the_tube(dev):
    from dcnet_amd import ops
    c = R.path_case(*R.PATH_SHAPES[2])
    path, score, _ = _link(c, dev)
    try:
        ops.set_precision("bf16s")
        p2, s2, _ = _link(c, dev)
    finally:
        ops.set_precision("fp32")
    assert torch.equal(p2, path) and torch.equal(s2, score)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", ["replicate", "valid"])
def test_video_grounder_link(dev, border):
    from dcnet_amd import postprocess
    from dcnet_amd import video as V
    from dcnet_amd.utils.synth import synth_inputs
    from test_video_gpu import _model
    m = _model(256)
    image, word_id, _ = synth_inputs(12, 256, n_queries=2, seed=91)
    image, word_id = image.to(dev), word_id.to(dev)
    base = V.VideoGrounder(m, n_frame=5, border=border, topk=5).run(image, word_id)
    cfg = V.TubeLink()
    res = V.VideoGrounder(m, n_frame=5, border=border, topk=5, link=cfg).run(image, word_id)
    n = res.centres.numel()
    assert base.cand_keep is None and base.tube is None and base.tube_score is None and base.tube_boxes is None
    for f in ("centres", "boxes", "cand_boxes", "cand_scores", "cand_feats", "best", "fused", "fused_boxes"):
        assert torch.equal(getattr(res, f), getattr(base, f)), f
    for f in ("outbox", "sim", "loc", "only_obj"):
        for q in range(2):
            for s in range(3):
                assert torch.equal(getattr(res, f)[q][s], getattr(base, f)[q][s]), (f, q, s)
    for s in range(3):
        assert torch.equal(res.corr_feat[s], base.corr_feat[s])
    assert res.cand_keep.shape == (2, n, 5) and res.cand_keep.dtype == torch.bool
    assert torch.equal(res.cand_keep, postprocess.nms_keep(res.cand_boxes.reshape(2 * n, 5, 4), cfg.nms_iou).view(2, n, 5))
    path, score, tb = postprocess.link_tubes(res.cand_boxes, res.cand_scores, res.cand_feats, res.cand_keep, cfg.iou_weight, cfg.feat_weight)
    assert res.tube.shape == (2, n) and res.tube_score.shape == (2,) and res.tube_boxes.shape == (2, n, 4)
    assert torch.equal(res.tube, path) and torch.equal(res.tube_score, score) and torch.equal(res.tube_boxes, tb)
    assert bool(torch.gather(res.cand_keep, 2, res.tube[:, :, None]).all())
    # the fused scores as the unary term, no NMS, no appearance term: the same entry with other arguments
    cfg2 = V.TubeLink(iou_weight=2.0, feat_weight=0.0, nms_iou=None, unary="fused")
    res2 = V.VideoGrounder(m, n_frame=5, border=border, topk=5, link=cfg2).run(image, word_id)
    assert bool(res2.cand_keep.all())
    path2, score2, _ = postprocess.link_tubes(res2.cand_boxes, res2.fused, None, None, 2.0, 0.0)
    assert torch.equal(res2.tube, path2) and torch.equal(res2.tube_score, score2)


# ---- 8 ------------------------------------------------------------------------------------------------------------------------
def test_rejections(dev):
    from dcnet_amd import ops, postprocess
    from dcnet_amd import video as V
    from test_video_gpu import _model
    z = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(RuntimeError, match="HIP kernels only"):
        postprocess.link_tubes(torch.zeros(1, 3, 5, 4), torch.zeros(1, 3, 5), torch.zeros(1, 3, 5, 8))
    with pytest.raises(RuntimeError, match="HIP kernels only"):
        postprocess.link_tubes(z(1, 3, 5, 4), z(1, 3, 5), torch.zeros(1, 3, 5, 8))
    with pytest.raises(RuntimeError, match="HIP kernels only"):
        postprocess.nms_keep(torch.zeros(3, 5, 4), 0.5)
    with pytest.raises(ValueError, match="k <= 64"):
        postprocess.nms_keep(z(3, 65, 4), 0.5)
    with pytest.raises(ValueError, match="k <= 64"):
        postprocess.link_tubes(z(1, 3, 65, 4), z(1, 3, 65), z(1, 3, 65, 8))
    with pytest.raises(ValueError, match="boxes must be"):
        postprocess.link_tubes(z(3, 5, 4), z(3, 5), z(3, 5, 8))
    with pytest.raises(ValueError, match="boxes must be"):
        postprocess.nms_keep(z(3, 5, 5), 0.5)
    with pytest.raises(ValueError, match="unary must be"):
        postprocess.link_tubes(z(1, 3, 5, 4), z(1, 3, 4), z(1, 3, 5, 8))
    with pytest.raises(ValueError, match="feats must be"):
        postprocess.link_tubes(z(1, 3, 5, 4), z(1, 3, 5), z(1, 2, 5, 8))
    with pytest.raises(ValueError, match="keep must be"):
        postprocess.link_tubes(z(1, 3, 5, 4), z(1, 3, 5), z(1, 3, 5, 8), keep=z(1, 3, 5))
    with pytest.raises(ValueError, match="keep must be"):
        postprocess.link_tubes(z(1, 3, 5, 4), z(1, 3, 5), z(1, 3, 5, 8), keep=torch.ones(1, 3, 4, dtype=torch.bool, device=dev))
    with pytest.raises(ValueError, match="feats is None"):
        postprocess.link_tubes(z(1, 3, 5, 4), z(1, 3, 5), None, None, 1.0, 0.5)
    with pytest.raises(ValueError, match="weights"):
        postprocess.link_tubes(z(1, 3, 5, 4), z(1, 3, 5), z(1, 3, 5, 8), None, -1.0, 1.0)
    with pytest.raises(ValueError, match="out must be uint8"):
        ops.post_nms(z(3, 5, 4), 0.5, out=torch.zeros(3, 5, dtype=torch.bool, device=dev))
    with pytest.raises(ValueError, match="topk"):
        V.VideoGrounder(_model(256), n_frame=5, link=V.TubeLink())
    with pytest.raises(TypeError, match="TubeLink"):
        V.VideoGrounder(_model(256), n_frame=5, topk=5, link=True)
    with pytest.raises(ValueError, match="without link"):
        V.VideoGrounder(_model(256), n_frame=5, topk=5).link(None)
    # feats=None with feat_weight = 0 is the IoU-only tube, not an error
    path, score, _ = postprocess.link_tubes(z(1, 3, 5, 4), z(1, 3, 5), None, None, 1.0, 0.0)
    assert path.tolist() == [[0, 0, 0]] and float(score[0]) == 0.0
