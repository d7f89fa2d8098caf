"""CPU: the fp64 reference of tube linking (tests/tube_ref.py) against brute force and its own definitions, the inputs that
tests/test_tube_gpu.py relies on (planted optima, margins), four wrong variants that must fail that file's criteria on its inputs,
the workspace range planner and the argument validation of the Python API."""
import numpy as np
import pytest
import torch

import tube_ref as R


def test_dp_equals_brute_force():
    c = R.brute_cases()
    assert c["boxes"].shape == (8,) + R.BRUTE_SHAPE[:2] + (4,)
    print("brute-force margins", np.round(c["margin"], 3))
    assert c["margin"].min() >= R.BRUTE_MARGIN
    assert not c["keep"][1::2].all(), "the odd cases are meant to run under a keep mask that suppresses something"
    for q in range(8):
        W, _ = R.transitions(c["boxes"][q], c["feats"][q], 1.0, 1.0)
        path, score, _ = R.viterbi(c["unary"][q], W, c["keep"][q])
        assert np.array_equal(path, c["best"][q]), q
        assert abs(score - c["value"][q]) < 1e-12 and abs(R.path_value(path, c["unary"][q], W) - score) < 1e-12
        assert c["keep"][q][np.arange(len(path)), path].all()


@pytest.mark.parametrize("thr", R.THRS)
@pytest.mark.parametrize("B,k", R.NMS_SHAPES)
def test_nms_reference_properties(B, k, thr):
    boxes = R.nms_case(B, k)
    suppressed = 0
    for b in boxes:
        keep = R.nms(b, thr)
        m = R.iou(b[:, None, :], b[None, :, :])
        assert keep[0]
        kept = np.nonzero(keep)[0]
        off = m[np.ix_(kept, kept)][~np.eye(len(kept), dtype=bool)]
        assert np.all(off <= thr)
        for i in np.nonzero(~keep)[0]:
            assert np.any(m[kept[kept < i], i] > thr), i
        suppressed += int((~keep).sum())
        assert np.all(np.abs(m[~np.eye(k, dtype=bool)] - thr) >= 1e-4)            # the margin that makes fp32 NMS exact
    assert R.nms(boxes[B], thr).all(), "zero-area boxes overlap nothing"
    if k >= 5:
        assert suppressed > 0, "a case that suppresses nothing tests nothing"


@pytest.mark.parametrize("i", range(len(R.PLANTED)))
def test_planted_tracks_are_the_optimum(i):
    v = R.planted_case(i)
    W, _ = R.transitions(v["boxes"], v["feats"], 1.0, 1.0)
    path, score, _ = R.viterbi(v["unary"], W)
    assert np.array_equal(path, v["slots"])
    margin = R.single_frame_margin(v["slots"], v["unary"], W)
    print("planted", R.PLANTED[i], "single-frame margin", round(margin, 3), "redraws", v["redraws"])
    assert margin >= R.PLANTED_MARGIN
    assert len(set(v["slots"].tolist())) > 1, "a track that never changes its slot tests no back-pointer"


def test_fp32_inputs_are_what_the_generator_says():
    v = R.planted_case(1)
    assert v["boxes"].dtype == v["unary"].dtype == v["feats"].dtype == np.float32
    assert np.all(np.diff(v["unary"], axis=1) <= 0) and v["unary"].min() > 0 and v["unary"].max() < 1
    assert np.allclose(np.linalg.norm(v["feats"].astype(np.float64), axis=-1), 1, atol=1e-6)
    assert np.array_equal(R.gen_video(4000, 40, 20, 96)["boxes"], v["boxes"])       # seeded


# ---- wrong variants: each must fail a criterion of tests/test_tube_gpu.py on that file's inputs ---------------------------------
def _paths(case, q, **kw):
    W, _ = R.transitions(case["boxes"][q], case["feats"][q], 1.0, 1.0)
    return R.viterbi(case["unary"][q], W, case.get("keep", [None] * 99)[q], **kw), W


def test_wrong_variant_last_maximum_fails_the_tie_criterion():
    c = R.tie_case()
    W, _ = R.transitions(c["boxes"], c["feats"], 1.0, 1.0)
    right, _, _ = R.viterbi(c["unary"], W)
    wrong, _, _ = R.viterbi(c["unary"], W, tie="last")
    assert right.max() < 5                       # the criterion: only the first copy of a candidate appears
    assert wrong.max() >= 5


def test_wrong_variant_keep_ignored_fails_the_path_criteria():
    failed = 0
    for shape in R.PATH_SHAPES[1:]:
        c = R.path_case(*shape)
        for q in range(shape[0]):
            (path, _, _), W = _paths(c, q, use_keep=False)
            failed += int(not c["keep"][q][np.arange(len(path)), path].all())    # the criterion: no suppressed candidate on the path
    assert failed == sum(s[0] for s in R.PATH_SHAPES[1:])


def test_wrong_variant_backpointer_row_off_by_one_fails_the_exact_paths():
    c = R.brute_cases()
    wrong = sum(int(not np.array_equal(_paths(c, q, bp_shift=1)[0][0], c["best"][q])) for q in range(8))
    assert wrong > 0
    for i in range(len(R.PLANTED)):
        v = R.planted_case(i)
        W, _ = R.transitions(v["boxes"], v["feats"], 1.0, 1.0)
        assert not np.array_equal(R.viterbi(v["unary"], W, bp_shift=1)[0], v["slots"])


def test_wrong_variant_nms_against_suppressed_fails_the_exact_mask():
    differs = 0
    for B, k in R.NMS_SHAPES:
        for thr in R.THRS:
            boxes = R.nms_case(B, k)
            differs += int(not np.array_equal(R.nms_batch(boxes, thr), R.nms_batch(boxes, thr, against_suppressed=True)))
    assert differs > 0


def test_path_slack_is_small_against_the_margins():
    """The slack the GPU test grants the path value is far below the margins that make the exact-path cases unambiguous."""
    for (n, k, E), _ in R.PLANTED:
        assert R.path_slack(n, E, 1.0, 1.0) < R.PLANTED_MARGIN / 10
    assert R.path_slack(R.BRUTE_SHAPE[0], R.BRUTE_SHAPE[2], 1.0, 1.0) < R.BRUTE_MARGIN / 10


# ---- the range planner ----------------------------------------------------------------------------------------------------------
def test_range_planner():
    from dcnet_amd import ops
    for q, n, k, ws in [(1, 1, 5, 1), (2, 33, 5, 2 * 25 * 4), (2, 33, 5, 3 * 2 * 25 * 4), (2, 33, 5, 3 * 2 * 25 * 4 + 199), (1, 40, 64, 64 << 20),
                        (4, 1024, 64, 64 << 20), (3, 7, 20, 0)]:
        got = ops.tube_ranges(q, n, k, ws)
        assert got == R.ranges(q, n, k, ws)
        per = max(1, ws // (q * k * k * 4))
        assert got[0][0] == 0 and got[-1][1] == n and all(a[1] == b[0] for a, b in zip(got, got[1:]))
        assert all(0 < t1 - t0 <= per for t0, t1 in got) and all(t1 - t0 == per for t0, t1 in got[:-1])
        assert per == 1 or q * per * k * k * 4 <= ws
    assert ops.tube_ranges(4, 1024, 64, 64 << 20) == [(0, 1024)]
    assert ops.tube_ranges(2, 33, 5, None) == [(0, 33)] and ops.TUBE_WS_BYTES == 64 << 20
    assert [t1 - t0 for t0, t1 in ops.tube_ranges(2, 7, 5, 3 * 200)] == [3, 3, 1]
    with pytest.raises(ValueError):
        ops.tube_ranges(0, 5, 5)


# ---- argument validation that needs no GPU --------------------------------------------------------------------------------------
def test_python_api_rejects_cpu_tensors_and_bad_settings():
    from dcnet_amd import postprocess
    from dcnet_amd import video as V
    with pytest.raises(RuntimeError, match="HIP kernels only"):
        postprocess.nms_keep(torch.zeros(2, 5, 4), 0.5)
    with pytest.raises(RuntimeError, match="HIP kernels only"):
        postprocess.link_tubes(torch.zeros(1, 3, 5, 4), torch.zeros(1, 3, 5))
    with pytest.raises(ValueError, match="unary"):
        V.TubeLink(unary="best")
    with pytest.raises(ValueError, match="weights"):
        V.TubeLink(iou_weight=-1.0)
    with pytest.raises(ValueError, match="nms_iou"):
        V.TubeLink(nms_iou=1.5)
    cfg = V.TubeLink()
    assert (cfg.iou_weight, cfg.feat_weight, cfg.nms_iou, cfg.unary) == (1.0, 1.0, 0.6, "score")
    r = V.VideoResult(centres=torch.arange(2), outbox=[[torch.zeros(1)] * 3], sim=[[torch.zeros(1)] * 3], loc=[[torch.zeros(1)] * 3],
                      corr_feat=[torch.zeros(1)] * 3, only_obj=[[torch.zeros(1)] * 3], boxes=torch.zeros(1, 2, 4))
    assert r.cand_keep is None and r.tube is None and r.tube_score is None and r.tube_boxes is None
    r.cand_boxes, r.cand_scores, r.cand_feats = torch.zeros(1, 2, 3, 4), torch.zeros(1, 2, 3), torch.zeros(1, 2, 3, 8)
    r.cand_keep = torch.ones(1, 2, 3, dtype=torch.bool)
    both = V.VideoResult.cat([r, r])
    assert both.cand_keep.shape == (1, 4, 3) and both.cand_keep.dtype == torch.bool and both.tube is None
