"""CPU: the streaming rule of tests/tube_stream_ref.py on tube_ref's fp64 transitions cast to fp32 — what it
guarantees, that the inputs of tests/test_tube_stream_gpu.py are decisive (every wrong variant fails that file's criteria on that
file's own inputs), and the host logic of dcnet_amd.video's streams (release counts, argument checks)."""
import types

import numpy as np
import pytest

import tube_ref as R
import tube_stream_ref as S


@pytest.fixture(scope="module")
def cases():
    """(name, n, E, [(unary, W32, W64, keep) per query]) of every generated case."""
    out = []
    for name, c in S.gen_cases():
        Q, n, k = c["unary"].shape
        per_q = []
        for q in range(Q):
            W64 = R.transitions(c["boxes"][q], c["feats"][q], 1.0, 1.0)[0]
            per_q.append((c["unary"][q], W64.astype(np.float32), W64, None if c["keep"] is None else c["keep"][q]))
        out.append((name, n, c["feats"].shape[-1], per_q))
    return out


def _big_keep(cases):
    return next(x for x in cases if x[0] == f"{S.BIG}+keep")


def test_no_early_commit_is_the_offline_optimum(cases):
    """lag >= n: nothing is committed before the end, and fp32 chooses the path fp64 chooses."""
    for name, n, E, per_q in cases:
        for unary, W32, W64, keep in per_q:
            want, opt, _ = R.viterbi(unary, W64, keep)
            for lag in (n, 64):
                path, forced, score = S.stream_viterbi(unary, W32, keep, lag)
                assert forced == 0 and np.array_equal(path, want), (name, lag)
                assert abs(float(score) - opt) <= R.path_slack(n, E, 1.0, 1.0) / 2, (name, lag)


def test_lag_8_is_exact_on_the_generated_cases(cases):
    for name, n, E, per_q in cases:
        for unary, W32, W64, keep in per_q:
            path, forced, score = S.stream_viterbi(unary, W32, keep, 8)
            full, _, full_score = S.stream_viterbi(unary, W32, keep, 64)
            assert forced == 0, name
            assert np.array_equal(path, R.viterbi(unary, W64, keep)[0]) and score == full_score, name


def test_lag_1_forces_commits_and_stays_a_valid_path(cases):
    name, n, E, per_q = _big_keep(cases)
    unary, W32, W64, keep = per_q[0]
    path, forced, score = S.stream_viterbi(unary, W32, keep, 1)
    off = R.viterbi(unary, W64, keep)[0]
    differ = int((path != off).sum())
    val = R.path_value(path, unary, W32.astype(np.float64))
    print(f"lag 1 on {name}: forced {forced}, {differ} frames differ from the offline path, |value - score| = {abs(val - float(score)):.3e}")
    assert forced > 0 and differ > 0
    assert keep[np.arange(n), path].all(), "a suppressed candidate on the path"
    assert abs(val - float(score)) <= R.path_slack(n, E, 1.0, 1.0)


def test_twin():
    c = S.twin()
    off = R.viterbi(c["unary"], c["W"].astype(np.float64))[0]
    assert np.array_equal(off, np.ones(16, np.int64))
    for lag in (1, 3, 8):
        path, forced, score = S.stream_viterbi(c["unary"], c["W"], None, lag)
        assert forced == 1 and np.array_equal(path, np.zeros(16, np.int64)) and float(score) == 16.0, lag
    path, forced, score = S.stream_viterbi(c["unary"], c["W"], None, 15)
    assert forced == 1 and np.array_equal(path, off) and float(score) == 16.5


def test_dead_lane():
    c = S.dead_lane()
    path, forced, _ = S.stream_viterbi(c["unary"], c["W"], c["keep"], 2)
    assert forced == 0 and np.array_equal(path, np.zeros(8, np.int64))
    assert S.stream_viterbi(c["unary"], c["W"], c["keep"], 2, count_dead=True)[1] == 1


# ---- every wrong variant fails the GPU file's criteria (exact equality with the reference; value == score) on its inputs -------
def test_wrong_no_pruning(cases):
    c = S.twin()
    for lag in (1, 3, 8):
        path, _, score = S.stream_viterbi(c["unary"], c["W"], None, lag, prune=False)
        assert R.path_value(path, c["unary"], c["W"].astype(np.float64)) != float(score), lag
    name, n, E, per_q = next(x for x in cases if x[0] == f"{S.GEN_SHAPES[1]}+keep")
    unary, W32, W64, keep = per_q[0]
    path, forced, score = S.stream_viterbi(unary, W32, keep, 1, prune=False)
    assert forced > 0
    assert abs(R.path_value(path, unary, W32.astype(np.float64)) - float(score)) > R.path_slack(n, E, 1.0, 1.0)
    assert not np.array_equal(path, S.stream_viterbi(unary, W32, keep, 1)[0])


def test_wrong_last_arg_max(cases):
    name, n, E, per_q = next(x for x in cases if x[0] == "tie")
    unary, W32, _, keep = per_q[0]
    for lag in S.LAGS:
        assert not np.array_equal(S.stream_viterbi(unary, W32, keep, lag, tie="last")[0], S.stream_viterbi(unary, W32, keep, lag)[0]), lag
    c = S.twin()
    for lag in (1, 2, 8):
        assert not np.array_equal(S.stream_viterbi(c["unary"], c["W"], None, lag, tie="last")[0], S.stream_viterbi(c["unary"], c["W"], None, lag)[0])


def test_wrong_ancestor_depth(cases):
    for name, n, E, per_q in cases:
        for unary, W32, _, keep in per_q:
            for lag in (1, 2, 8):
                assert not np.array_equal(S.stream_viterbi(unary, W32, keep, lag, depth_shift=1)[0],
                                          S.stream_viterbi(unary, W32, keep, lag)[0]), (name, lag)


def test_wrong_dead_lanes_counted():
    c = S.dead_lane()
    assert S.stream_viterbi(c["unary"], c["W"], c["keep"], 2, count_dead=True)[1] != S.stream_viterbi(c["unary"], c["W"], c["keep"], 2)[1]


# ---- host logic of dcnet_amd.video -------------------------------------------------------------------------------------------------
def test_release_counts():
    from dcnet_amd import video as V
    assert [V.fuse_delay(K) for K in (2, 3, 4, 5)] == [0, 1, 1, 2]
    # unary "score": the recursion takes every arrival, frames below arrived - lag are out
    assert V.stream_counts(10, 5, 8, False) == (8, 10, 2)
    assert V.stream_counts(7, 5, 8, False) == (5, 7, 0)
    # unary "fused": the recursion trails by the fusion delay
    assert V.stream_counts(10, 5, 8, True) == (8, 8, 0)
    assert V.stream_counts(13, 5, 8, True) == (11, 11, 3)
    assert V.stream_counts(1, 5, 1, True) == (0, 0, 0)
    assert V.stream_counts(13, 5, 8, True, flushed=True) == (13, 13, 13)
    for K in (2, 3, 5):
        for lag in (1, 8):
            for fused in (False, True):
                prev = (0, 0, 0)
                for N in range(1, 30):
                    cur = V.stream_counts(N, K, lag, fused)
                    assert all(0 <= c - p <= 1 for c, p in zip(cur, prev)) and cur[2] <= cur[1] <= N and cur[0] <= N
                    prev = cur


def test_argument_validation():
    import torch
    from dcnet_amd import video as V
    for lag in (0, 65, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="lag"):
            V.TubeStream(V.TubeLink(), 5, lag)
    with pytest.raises(TypeError, match="TubeLink"):
        V.TubeStream(None, 5, 8)
    with pytest.raises(ValueError, match="n_frame"):
        V.TubeStream(V.TubeLink(), 1, 8)
    with pytest.raises(ValueError, match="n_frame"):
        V.FuseStream(33)
    ts = V.TubeStream(V.TubeLink(), 5, 64)
    assert ts.state_bytes() == 0 and ts.push(None) is None and ts.flush() is None

    def part(Q, m, k, E=8, keep=True, cands=True):
        z = torch.zeros
        return types.SimpleNamespace(centres=torch.arange(m), cand_boxes=z(Q, m, k, 4) if cands else None, cand_scores=z(Q, m, k) if cands else None,
                                     cand_feats=z(Q, m, k, E) if cands else None, cand_keep=torch.ones(Q, m, k, dtype=torch.bool) if keep else None)

    with pytest.raises(ValueError, match="no candidates"):
        V._check_stream_part(part(2, 3, 5, cands=False), None, "t", False)
    with pytest.raises(ValueError, match="cand_keep is None"):
        V._check_stream_part(part(2, 3, 5, keep=False), None, "t", True)
    with pytest.raises(ValueError, match="began with Q = 2, k = 5"):
        V._check_stream_part(part(2, 3, 4), (2, 5), "t", True)
    with pytest.raises(ValueError, match="began with Q = 2, k = 5"):
        V._check_stream_part(part(1, 3, 5), (2, 5), "t", True)
    with pytest.raises(ValueError, match="CUDA"):                            # (the last check: a matching CPU part gets this far)
        V._check_stream_part(part(2, 3, 5), (2, 5), "t", True)
    with pytest.raises(ValueError, match="CUDA"):
        V.FuseStream(5).push(part(2, 3, 5))
    with pytest.raises(ValueError, match="CUDA"):
        ts.push(part(2, 3, 5))
