"""CPU: the host logic of dcnet_amd/video.py — the window rule against the reference's own windows (tests/golden/video_windows.json,
written by tools/make_video_goldens.py from ``getChunk``), the pair planner against brute-force enumeration, argument errors."""
import json
import os
from collections import Counter

import pytest
import torch

from util import GOLD, build_product, synth_sd

KS = (2, 3, 5, 8)


def _cases():
    with open(os.path.join(GOLD, "video_windows.json")) as f:
        return json.load(f)["cases"]


def test_fixture_covers_the_grid():
    got = {(c["frames"], c["n_frame"]) for c in _cases()}
    assert got == {(F, K) for F in (2, 5, 6, 8, 12) for K in KS}
    assert sum(len(c["windows"]) for c in _cases()) > 40


def test_window_rule_reproduces_the_reference_windows():
    from dcnet_amd import video as V
    assert V.window_offsets(2) == [-1, 0] and V.window_offsets(3) == [-1, 0, 1]
    assert V.window_offsets(5) == [-2, -1, 0, 1, 2] and V.window_offsets(8) == [-4, -3, -2, -1, 0, 1, 2, 3]
    for c in _cases():
        F, K = c["frames"], c["n_frame"]
        ref = V.reference_centres(F, K)
        assert [[i + o for o in V.window_offsets(K)] for i in ref] == c["windows"], (F, K)
        assert [V.window_frames(i, F, K, "valid") for i in ref] == c["windows"], (F, K)
        assert all(w[K // 2] == i for i, w in zip(ref, c["windows"]))                      # centre slot K // 2
        # "valid" = the reference's set plus the one centre it drops although its window fits
        valid = V.centres(F, K, "valid")
        dropped = F - (K + 1) // 2
        if dropped >= K // 2:
            assert valid == ref + [dropped], (F, K)
            assert V.window_frames(dropped, F, K)[-1] == F - 1
        else:
            assert valid == ref == [], (F, K)
        assert V.centres(F, K, "replicate") == list(range(F))
    assert V.reference_centres(8, 5) == [2, 3, 4] and V.centres(8, 5) == [2, 3, 4, 5]


def _brute(V, F, K, border):
    out = Counter()
    for i in V.centres(F, K, border):
        for o in V.window_offsets(K):
            if o:
                j = i + o
                out[(i, min(max(j, 0), F - 1) if border == "replicate" else j)] += 1
    return out


@pytest.mark.parametrize("border", ["valid", "replicate"])
@pytest.mark.parametrize("K", KS)
def test_pair_plan_equals_brute_force(K, border):
    from dcnet_amd import video as V
    for F in range(1, 13):
        want = _brute(V, F, K, border)
        assert sum(want.values()) == (K - 1) * len(V.centres(F, K, border))
        for chunk in (1, 3, F):
            got, aff = Counter(), Counter()
            for f0 in range(0, F, chunk):
                plan = V.pair_plan(f0, min(F, f0 + chunk), K, border, total=F)
                for i, j, w in plan.contributions():
                    got[(i, j)] += w
                for ab in plan.affinities():
                    aff[ab] += 1
                for d, a0, n, fwd, bwd in plan.runs:
                    assert 0 < d <= K // 2 and n > 0 and a0 >= 0 and a0 + d + n <= F and (fwd or bwd)
                    assert fwd <= (d in V.window_offsets(K)) and bwd <= (-d in V.window_offsets(K))
                    assert f0 <= a0 + d and a0 + d + n <= min(F, f0 + chunk)          # the later frame is one of the new ones
                for a, b, w_ab, w_ba in plan.border:
                    assert 0 <= a <= b < F and b - a <= K // 2 and border == "replicate" and (w_ab or w_ba)
            assert got == want, (F, K, border, chunk)
            assert all(v == 1 for (a, b), v in aff.items() if a != b), (F, K, border, chunk)      # no affinity twice
            # every centre's weights sum to K - 1 (the mean is over K - 1 attended features, duplicates counted)
            per = Counter()
            for (i, _), w in got.items():
                per[i] += w
            assert all(v == K - 1 for v in per.values())
        if K % 2 == 0 and border == "valid" and F > K:
            # even K: the distance K / 2 has one direction only
            assert all(not fwd for d, _, _, fwd, _ in V.pair_plan(0, F, K, border, total=F).runs if d == K // 2)


@pytest.mark.parametrize("border", ["valid", "replicate"])
@pytest.mark.parametrize("K", KS)
def test_streamed_plan_without_a_known_length(K, border):
    """Frame by frame with the length unknown, plus flush_plan: restricted to the centres that exist in the end, the same multiset."""
    from dcnet_amd import video as V
    for F in range(1, 13):
        got = Counter()
        for f0 in range(F):
            for i, j, w in V.pair_plan(f0, f0 + 1, K, border).contributions():
                got[(i, j)] += w
        for i, j, w in V.flush_plan(F, K, border).contributions():
            got[(i, j)] += w
        cs = set(V.centres(F, K, border))
        assert Counter({k: v for k, v in got.items() if k[0] in cs}) == _brute(V, F, K, border), (F, K, border)
        if border == "valid":
            assert V.flush_plan(F, K, border).affinities() == []


def test_argument_errors_name_the_argument():
    from dcnet_amd import video as V
    for fn in (lambda: V.window_offsets(1), lambda: V.centres(8, 1), lambda: V.pair_plan(0, 4, 0), lambda: V.reference_centres(8, True)):
        with pytest.raises(ValueError, match="n_frame"):
            fn()
    with pytest.raises(ValueError, match="border"):
        V.centres(8, 5, "reflect")
    with pytest.raises(ValueError, match="border"):
        V.pair_plan(0, 4, 5, "wrap")
    m = build_product(256, synth_sd(256), torch.device("cpu"))
    with pytest.raises(ValueError, match="train mode"):
        V.VideoGrounder(m.train(), n_frame=5)
    m.eval()
    with pytest.raises(ValueError, match="n_frame"):
        V.VideoGrounder(m, n_frame=1)
    with pytest.raises(ValueError, match="border"):
        V.VideoGrounder(m, border="mirror")
    with pytest.raises(ValueError, match="chunk"):
        V.VideoGrounder(m, chunk=0)
    with pytest.raises(ValueError, match="topk"):
        V.VideoGrounder(m, topk=65)
    with pytest.raises(ValueError, match="topk"):
        V.VideoGrounder(m, n_frame=33, topk=5)
    with pytest.raises(TypeError, match="model"):
        V.VideoGrounder(torch.nn.Linear(2, 2))
    vg = V.VideoGrounder(m, n_frame=5)
    with pytest.raises(ValueError, match="image"):
        vg.run(torch.zeros(8, 3, 256, 256), torch.ones(1, 20, dtype=torch.long))
    with pytest.raises(ValueError, match="word_id"):
        vg.reset(torch.ones(1, 20, dtype=torch.long))
    with pytest.raises(RuntimeError, match="reset"):
        vg.push(torch.zeros(1, 3, 256, 256))
    m.train()
    with pytest.raises(ValueError, match="train mode"):
        vg.reset(torch.ones(1, 20, dtype=torch.long))

