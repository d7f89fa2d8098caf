"""GPU: streaming tube linking and fusion (dcnet_amd/csrc/tube.hip tube_stream_step / _flush, ops.tube_stream_*, video.FuseStream /
TubeStream, VideoGrounder.tube_stream) against tests/tube_stream_ref.py.  What makes the inputs decisive is checked on the CPU by
tests/test_tube_stream_host.py.

No tolerance anywhere.  The reference runs in fp32 on the transition scores READ BACK from the device, and a delta update is two single
fp32 additions on either side (no multiply: nothing to contract, no order to choose), so delta and with it every arg-max, commit,
forced count and the score are equal bit for bit.  Where no commit was forced no delta was altered, so the streamed track is that of
``postprocess.link_tubes``; the streamed fusion runs the kernel of ``ops.post_fusion_bank`` on the same window contents."""
import numpy as np
import pytest
import torch

import tube_stream_ref as S

pytestmark = pytest.mark.gpu


def _up(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _device_w(c, dev):
    """The device's own transition scores of a generated batch, (Q,n,k,k); the row of frame 0 (never written, never read) zeroed."""
    from dcnet_amd import ops
    Q, n, k = c["unary"].shape
    W = torch.zeros((Q, n, k, k), device=dev)
    return ops.tube_transitions(_up(c["boxes"], dev), _up(c["feats"], dev), 0, n, 1.0, 1.0, W)


def _stream(W, unary, keep, lag, sizes):
    """The entry points over pushes of the given sizes: (path (Q,n) = commits + tail, forced (Q,), score (Q,), commit (Q,n))."""
    from dcnet_amd import ops
    Q, n, k = unary.shape
    dev = unary.device
    delta = torch.full((Q, k), float("nan"), device=dev)                  # unread at t0 = 0
    surv = torch.full((Q, lag, k), 0xAB, dtype=torch.uint8, device=dev)   # likewise
    forced = torch.zeros(Q, dtype=torch.int32, device=dev)
    commits, t = [], 0
    for m in sizes:
        commits.append(ops.tube_stream_step(W[:, t:t + m].contiguous(), unary[:, t:t + m].contiguous(),
                                            None if keep is None else keep[:, t:t + m].contiguous(), t, lag, delta, surv, forced))
        t += m
    assert t == n
    commit = torch.cat(commits, dim=1)
    tail, score = ops.tube_stream_flush(delta, surv, n, lag)
    assert tail.shape == (Q, min(lag, n)) and bool((commit[:, :min(lag, n)] == -1).all())
    return torch.cat([commit[:, lag:], tail], dim=1), forced, score, commit


def _sizes(n, per):
    return [per] * (n // per) + ([n % per] if n % per else [])


def _check_against_ref(W, unary, keep, lag, sizes):
    path, forced, score, _ = _stream(W, unary, keep, lag, sizes)
    Wn, un = W.cpu().numpy(), unary.cpu().numpy()
    kn = None if keep is None else keep.cpu().numpy().astype(bool)
    refs = []
    for q in range(unary.shape[0]):
        rp, rf, rs = S.stream_viterbi(un[q], Wn[q], None if kn is None else kn[q], lag)
        assert np.array_equal(path[q].cpu().numpy(), rp), (q, lag)
        assert int(forced[q]) == rf and float(score[q]) == float(rs), (q, lag, int(forced[q]), rf)
        refs.append((rp, rf, rs))
    return path, forced, score, refs


@pytest.fixture(scope="module")
def gen(dev):
    """name -> (W, unary, keep or None, boxes) on the device, for every generated case (computed once, never modified)."""
    out = {}
    for name, c in S.gen_cases():
        out[name] = (_device_w(c, dev), _up(c["unary"], dev), None if c["keep"] is None else _up(c["keep"].astype(np.uint8), dev),
                     _up(c["boxes"], dev), _up(c["feats"], dev))
    return out


def _hand(c, dev):
    return _up(c["W"][None], dev), _up(c["unary"][None], dev), None if c["keep"] is None else _up(c["keep"][None].astype(np.uint8), dev)


# ---- 1: the entry points against the reference on the device's own W ------------------------------------------------------------
@pytest.mark.parametrize("lag", S.LAGS)
def test_entry_points_equal_the_reference_exactly(dev, gen, lag):
    for name, (W, unary, keep, _, _) in gen.items():
        n = unary.shape[1]
        _, forced, _, refs = _check_against_ref(W, unary, keep, lag, _sizes(n, 6))
        if lag == 1 and name == f"{S.BIG}+keep":
            print(f"lag 1 on {name}: forced {int(forced[0])}")
            assert int(forced[0]) > 0
    for c in (S.twin(), S.dead_lane()):
        W, unary, keep = _hand(c, dev)
        _check_against_ref(W, unary, keep, lag, _sizes(unary.shape[1], 6))


def test_hand_cases(dev):
    W, unary, keep = _hand(S.twin(), dev)
    for lag, want in ((1, 0), (3, 0), (8, 0), (15, 1)):
        path, forced, score, _ = _stream(W, unary, keep, lag, [16])
        assert int(forced[0]) == 1 and path[0].tolist() == [want] * 16 and float(score[0]) == 16.0 + 0.5 * want, lag
    W, unary, keep = _hand(S.dead_lane(), dev)
    path, forced, _, _ = _stream(W, unary, keep, 2, [8])
    assert int(forced[0]) == 0 and path[0].tolist() == [0] * 8


# ---- 2: exactness ---------------------------------------------------------------------------------------------------------------
def _part(boxes, unary, feats, keep, lo, hi):
    from dcnet_amd.video import VideoResult
    Q, _, k = unary.shape
    kp = torch.ones((Q, hi - lo, k), dtype=torch.bool, device=unary.device) if keep is None else keep[:, lo:hi].bool()
    return VideoResult(centres=torch.arange(lo, hi, device=unary.device), outbox=[], sim=[], loc=[], corr_feat=[], only_obj=[],
                       boxes=boxes[:, lo:hi, 0], cand_boxes=boxes[:, lo:hi], cand_scores=unary[:, lo:hi], cand_feats=feats[:, lo:hi],
                       cand_keep=kp)


def _tube_stream(boxes, unary, feats, keep, lag, per, n_frame=5):
    from dcnet_amd import video as V
    n = unary.shape[1]
    ts = V.TubeStream(V.TubeLink(nms_iou=None), n_frame, lag)
    chunks, lo = [], 0
    for m in _sizes(n, per):
        chunks.append(ts.push(_part(boxes, unary, feats, keep, lo, lo + m)))
        lo += m
        assert sum(c.centres.numel() for c in chunks if c is not None) == V.stream_counts(lo, n_frame, lag, False)[2]
    chunks.append(ts.flush())
    chunks = [c for c in chunks if c is not None]
    assert all(c.tube_score is None for c in chunks[:-1])
    cat = lambda f, d: torch.cat([getattr(c, f) for c in chunks], dim=d)
    return cat("centres", 0), cat("tube", 1), cat("tube_boxes", 1), chunks[-1].tube_score, ts.forced


def test_without_a_forced_commit_the_stream_is_link_tubes(dev, gen):
    from dcnet_amd import postprocess
    for name, (W, unary, keep, boxes, feats) in gen.items():
        Q, n, k = unary.shape
        refs = [S.stream_viterbi(unary[q].cpu().numpy(), W[q].cpu().numpy(), None if keep is None else keep[q].cpu().numpy().astype(bool), 8)
                for q in range(Q)]
        assert all(r[1] == 0 for r in refs), name
        cen, tube, tb, score, forced = _tube_stream(boxes, unary, feats, keep, 8, 5)
        path, want_score, want_boxes = postprocess.link_tubes(boxes, unary, feats, keep, 1.0, 1.0)
        assert int(forced.sum()) == 0 and cen.tolist() == list(range(n)), name
        assert torch.equal(tube, path) and torch.equal(score, want_score) and torch.equal(tb, want_boxes), name


# ---- 3: chunk invariance ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,lag", [(f"{S.GEN_SHAPES[0]}", 1), (f"{S.GEN_SHAPES[0]}", 8), (f"{S.BIG}+keep", 1)])
def test_pushes_do_not_change_the_result(dev, gen, name, lag):
    W, unary, keep, _, _ = gen[name]
    n = unary.shape[1]
    base = _stream(W, unary, keep, lag, [n])
    for per in (1, 3, 7):
        got = _stream(W, unary, keep, lag, _sizes(n, per))
        for a, b in zip(got, base):
            assert torch.equal(a, b), per


# ---- 4: edges ---------------------------------------------------------------------------------------------------------------------
def test_edges(dev, gen):
    W, unary, keep, _, _ = gen[f"{S.GEN_SHAPES[1]}+keep"]                  # (1,40,20,96)
    # one frame
    path, _, score, _ = _check_against_ref(W[:, :1], unary[:, :1].contiguous(), keep[:, :1].contiguous(), 8, [1])
    assert path.shape == (1, 1) and float(score[0]) == float(unary[0, 0, 0])              # (scores sorted descending, candidate 0 kept)
    # n < lag: every commit entry is -1, the flush hands out the whole path
    path, forced, score, commit = _stream(W[:, :5].contiguous(), unary[:, :5].contiguous(), keep[:, :5].contiguous(), 8, [2, 3])
    assert bool((commit == -1).all()) and path.shape == (1, 5)
    _check_against_ref(W[:, :5].contiguous(), unary[:, :5].contiguous(), keep[:, :5].contiguous(), 8, [2, 3])
    # k = 1
    _check_against_ref(W[:, :, :1, :1].contiguous(), unary[:, :, :1].contiguous(), None, 2, _sizes(40, 7))
    # k = 64, and lag = 64 with n = 48
    W, unary, keep, _, _ = gen[f"{S.BIG}+keep"]
    _check_against_ref(W, unary, keep, 64, _sizes(48, 5))
    _check_against_ref(W, unary, None, 63, [48])
    _check_against_ref(W, unary, keep, 5, _sizes(48, 5))


def test_queries_are_independent(dev):
    c = S.gen_batch([6100, 6200, 6300], 9, 20, 64)
    c["keep"] = S.nms_batch(c["boxes"], 0.6)
    W, unary, keep = _device_w(c, dev), _up(c["unary"], dev), _up(c["keep"].astype(np.uint8), dev)
    perm = [2, 0, 1]
    for lag in (1, 4):
        path, forced, score, _ = _check_against_ref(W, unary, keep, lag, [4, 5])
        p2, f2, s2, _ = _stream(W[perm].contiguous(), unary[perm].contiguous(), keep[perm].contiguous(), lag, [4, 5])
        assert torch.equal(p2, path[perm]) and torch.equal(f2, forced[perm]) and torch.equal(s2, score[perm])
        for q in range(3):                                                 # each query on its own
            p1, f1, s1, _ = _stream(W[q:q + 1].contiguous(), unary[q:q + 1].contiguous(), keep[q:q + 1].contiguous(), lag, [9])
            assert torch.equal(p1[0], path[q]) and int(f1[0]) == int(forced[q]) and float(s1[0]) == float(score[q])
    assert len({tuple(r) for r in path.cpu().tolist()}) > 1


# ---- 5: FuseStream ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_frame", [2, 3, 5])
def test_fuse_stream_is_post_fusion_bank_on_the_whole_run(dev, n_frame):
    from dcnet_amd import ops
    from dcnet_amd import video as V
    Q, n, k, E = 2, 12, 5, 64
    c = S.gen_batch([8100, 8200], n, k, E)
    boxes, unary, feats = _up(c["boxes"], dev), _up(c["unary"], dev), _up(c["feats"], dev)
    best, fused = zip(*[ops.post_fusion_bank(feats[q].contiguous(), unary[q].contiguous(), n_frame) for q in range(Q)])
    best, fused = torch.stack(best), torch.stack(fused)
    fb = torch.gather(boxes, 2, best[:, :, None, None].expand(-1, -1, 1, 4))[:, :, 0]
    for per in (1, 4, n):
        fs = V.FuseStream(n_frame)
        chunks, lo = [], 0
        for m in _sizes(n, per):
            chunks.append(fs.push(_part(boxes, unary, feats, None, lo, lo + m)))
            lo += m
            assert sum(ch.centres.numel() for ch in chunks if ch is not None) == V.stream_counts(lo, n_frame, 1, False)[0]
        chunks.append(fs.flush())
        chunks = [ch for ch in chunks if ch is not None]
        assert torch.cat([ch.centres for ch in chunks]).tolist() == list(range(n))
        assert torch.equal(torch.cat([ch.best for ch in chunks], 1), best), (n_frame, per)
        assert torch.equal(torch.cat([ch.fused for ch in chunks], 1), fused), (n_frame, per)
        assert torch.equal(torch.cat([ch.fused_boxes for ch in chunks], 1), fb), (n_frame, per)
        assert fs.state_bytes() == 0 and fs.flush() is None


# ---- 6: VideoGrounder ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unary", ["score", "fused"])
@pytest.mark.parametrize("border", ["replicate", "valid"])
def test_video_grounder_tube_stream(dev, border, unary):
    from dcnet_amd import ops
    from dcnet_amd import video as V
    from dcnet_amd.utils.synth import synth_inputs
    from test_video_gpu import _model
    m = _model(256)
    image, word_id, _ = synth_inputs(12, 256, n_queries=2, seed=91)
    image, word_id = image.to(dev), word_id.to(dev)
    cfg = V.TubeLink(unary=unary)
    vg = V.VideoGrounder(m, n_frame=5, border=border, chunk=4, topk=5, link=cfg)
    res = vg.run(image, word_id)
    vg.reset(word_id, total=12)
    ts = vg.tube_stream(lag=8)
    chunks, state = [], []
    for i0 in range(0, 12, 4):
        chunks.append(ts.push(vg.push(image[i0:i0 + 4])))
        state.append(ts.state_bytes())
    last = vg.flush()
    if last is not None:
        chunks.append(ts.push(last))
        state.append(ts.state_bytes())
    assert state[2] == state[-1] > 0
    chunks.append(ts.flush())
    chunks = [c for c in chunks if c is not None]
    fz = [c.fused for c in chunks if c.fused is not None]
    assert torch.equal(torch.cat([f.centres for f in fz]), res.centres)
    for f in ("best", "fused", "fused_boxes"):
        assert torch.equal(torch.cat([getattr(c, f) for c in fz], 1), getattr(res, f)), f
    assert torch.equal(torch.cat([c.centres for c in chunks]), res.centres)
    tube, tb, score = torch.cat([c.tube for c in chunks], 1), torch.cat([c.tube_boxes for c in chunks], 1), chunks[-1].tube_score
    if int(ts.forced.sum()) == 0:
        assert torch.equal(tube, res.tube) and torch.equal(tb, res.tube_boxes) and torch.equal(score, res.tube_score)
    else:
        n = res.centres.numel()
        W = torch.zeros((2, n, 5, 5), device=dev)
        ops.tube_transitions(res.cand_boxes.contiguous(), res.cand_feats.contiguous(), 0, n, cfg.iou_weight, cfg.feat_weight, W)
        un = (res.cand_scores if unary == "score" else res.fused).cpu().numpy()
        for q in range(2):
            rp, rf, rs = S.stream_viterbi(un[q], W[q].cpu().numpy(), res.cand_keep[q].cpu().numpy(), 8)
            assert np.array_equal(tube[q].cpu().numpy(), rp) and int(ts.forced[q]) == rf and float(score[q]) == float(rs)
        assert torch.equal(tb, torch.gather(res.cand_boxes, 2, tube[:, :, None, None].expand(-1, -1, 1, 4))[:, :, 0])


# ---- 7: rejections ------------------------------------------------------------------------------------------------------------------
def test_rejections(dev, gen):
    from dcnet_amd import ops
    from dcnet_amd import video as V
    from dcnet_amd.lib import DcnError, lib
    from test_video_gpu import _model
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    state = lambda lag: (z(1, 5), z(1, lag, 5, dt=torch.uint8), z(1, dt=torch.int32))
    for lag in (0, 65):
        with pytest.raises(ValueError, match="lag"):
            ops.tube_stream_step(z(1, 3, 5, 5), z(1, 3, 5), None, 0, lag, *state(max(lag, 1)))
        with pytest.raises(ValueError, match="lag"):
            ops.tube_stream_flush(z(1, 5), z(1, max(lag, 1), 5, dt=torch.uint8), 3, lag)
        with pytest.raises(ValueError, match="lag"):
            V.TubeStream(V.TubeLink(), 5, lag)
        with pytest.raises(DcnError, match="lag"):                         # the C entry points check for themselves
            d, s, f = state(4)
            lib().tube_stream_step(z(1, 3, 5, 5).data_ptr(), z(1, 3, 5).data_ptr(), 0, 1, 3, 5, 0, lag, d.data_ptr(), s.data_ptr(),
                                   z(1, 3, dt=torch.int64).data_ptr(), f.data_ptr(), 0)
        with pytest.raises(DcnError, match="lag"):
            lib().tube_stream_flush(z(1, 5).data_ptr(), z(1, 4, 5, dt=torch.uint8).data_ptr(), 1, 5, 3, lag, z(1, 3, dt=torch.int64).data_ptr(),
                                    z(1).data_ptr(), 0)
    with pytest.raises(ValueError, match="k <= 64"):
        ops.tube_stream_step(z(1, 3, 65, 65), z(1, 3, 65), None, 0, 4, z(1, 65), z(1, 4, 65, dt=torch.uint8), z(1, dt=torch.int32))
    with pytest.raises(ValueError, match="W must be"):
        ops.tube_stream_step(z(1, 2, 5, 5), z(1, 3, 5), None, 0, 4, *state(4))
    with pytest.raises(ValueError, match="surv must be"):
        ops.tube_stream_step(z(1, 3, 5, 5), z(1, 3, 5), None, 0, 4, z(1, 5), z(1, 3, 5, dt=torch.uint8), z(1, dt=torch.int32))
    with pytest.raises(ValueError, match="forced must be"):
        ops.tube_stream_step(z(1, 3, 5, 5), z(1, 3, 5), None, 0, 4, z(1, 5), z(1, 4, 5, dt=torch.uint8), z(1))
    with pytest.raises(ValueError, match="keep must be"):
        ops.tube_stream_step(z(1, 3, 5, 5), z(1, 3, 5), z(1, 3, 5), 0, 4, *state(4))
    with pytest.raises(ValueError, match="CUDA"):
        ops.tube_stream_step(torch.zeros(1, 3, 5, 5), z(1, 3, 5), None, 0, 4, *state(4))
    with pytest.raises(ValueError, match="CUDA"):
        ops.tube_stream_flush(torch.zeros(1, 5), z(1, 4, 5, dt=torch.uint8), 3, 4)
    with pytest.raises(ValueError, match="without link"):
        V.VideoGrounder(_model(256), n_frame=5, topk=5).tube_stream()
    W, unary, keep, boxes, feats = gen[f"{S.GEN_SHAPES[0]}"]
    ts = V.TubeStream(V.TubeLink(), 5, 8)
    good = _part(boxes, unary, feats, keep, 0, 3)
    bare = _part(boxes, unary, feats, keep, 3, 6)
    bare.cand_boxes = bare.cand_scores = bare.cand_feats = None
    with pytest.raises(ValueError, match="no candidates"):
        ts.push(bare)
    nokeep = _part(boxes, unary, feats, keep, 3, 6)
    nokeep.cand_keep = None
    with pytest.raises(ValueError, match="cand_keep is None"):
        ts.push(nokeep)
    ts.push(good)
    with pytest.raises(ValueError, match="began with Q = 2, k = 5"):
        ts.push(_part(boxes[:, :, :4], unary[:, :, :4], feats[:, :, :4], None, 3, 6))
    with pytest.raises(ValueError, match="began with Q = 2, k = 5"):
        ts.push(_part(boxes[:1], unary[:1], feats[:1], None, 3, 6))
    cpu = _part(boxes.cpu(), unary.cpu(), feats.cpu(), None, 3, 6)
    with pytest.raises(ValueError, match="CUDA"):
        ts.push(cpu)
    assert ts.push(_part(boxes, unary, feats, keep, 3, 6)).tube.shape == (2, 0) and ts.flush().tube.shape == (2, 6)   # the stream survived
