"""Tube linking: the four entries of csrc/tube.hip against the same computation in stock torch ops, and its share of a video run
(a tool, not bench.py).

    python tools/bench_tube.py                  # (Q,n,k,E) = (1,1024,20,512) and (4,1024,64,512); 64 frames x 416^2 with / without link
    python tools/bench_tube.py --no-video       # the entries and the torch arms only
    python tools/bench_tube.py --stream [--frames 256]    # streaming: dcn_tube_stream_step against dcn_tube_forward, a TubeStream push,
                                                          # and a video pushed through a TubeStream against VideoGrounder.run

Per shape, device-event medians (``--warmup`` 5, ``--repeat`` 20) of ``dcn_post_nms``, ``dcn_tube_transitions``, ``dcn_tube_forward``,
``dcn_tube_backtrack`` and of ``postprocess.link_tubes`` as a whole.  Arm "torch": the same NMS, transitions (one batched matmul),
Viterbi recursion and walk in stock torch ops on the device — the recursion and the walk are a loop over the frames whatever one does.
Arm "torch_per_frame": the transitions inside that loop as well, one frame pair at a time (what a streaming caller would write).
Then ``VideoGrounder.run`` with ``topk`` and with / without ``link``, alternated, host clock around a synchronise.  One JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(1, 1024, 20, 512), (4, 1024, 64, 512)]


def _events(fn, warmup, repeat):
    """median ms of fn() by device events"""
    ts = []
    for it in range(warmup + repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        if it >= warmup:
            ts.append(a.elapsed_time(b))
    return round(float(np.median(ts)), 4)


# ---- the stock-torch arms -------------------------------------------------------------------------------------------------------
def t_iou(a, b):
    iw = (torch.minimum(a[..., 2], b[..., 2]) - torch.maximum(a[..., 0], b[..., 0])).clamp_min(0)
    ih = (torch.minimum(a[..., 3], b[..., 3]) - torch.maximum(a[..., 1], b[..., 1])).clamp_min(0)
    inter = iw * ih
    aa = (a[..., 2] - a[..., 0]).clamp_min(0) * (a[..., 3] - a[..., 1]).clamp_min(0)
    ab = (b[..., 2] - b[..., 0]).clamp_min(0) * (b[..., 3] - b[..., 1]).clamp_min(0)
    return inter / (aa + ab - inter + 1e-16)


def t_nms(boxes, thr):
    """boxes (B,k,4): k rounds, every centre at once"""
    B, k = boxes.shape[:2]
    over = t_iou(boxes[:, :, None], boxes[:, None, :]) > thr
    keep = torch.ones((B, k), dtype=torch.bool, device=boxes.device)
    later = torch.arange(k, device=boxes.device)
    for i in range(k - 1):
        keep &= ~(over[:, i] & keep[:, i:i + 1] & (later > i)[None])
    return keep


def t_transitions(boxes, feats, t0, t1):
    """W of frames t0 <= t < t1 (t0 >= 1): (Q, t1-t0, k, k)"""
    return t_iou(boxes[:, t0 - 1:t1 - 1, :, None], boxes[:, t0:t1, None, :]) + feats[:, t0 - 1:t1 - 1] @ feats[:, t0:t1].transpose(-1, -2)


def t_forward(W, unary, keep, per_frame=None):
    """W (Q,n-1,k,k) for frames 1 ... n-1, or None with per_frame = (boxes, feats): the transitions inside the loop"""
    Q, n, k = unary.shape
    ninf = torch.full((), float("-inf"), device=unary.device)
    delta = torch.where(keep[:, 0], unary[:, 0], ninf)
    bp = torch.zeros((Q, n, k), dtype=torch.int64, device=unary.device)
    for t in range(1, n):
        Wt = W[:, t - 1] if per_frame is None else t_transitions(per_frame[0], per_frame[1], t, t + 1)[:, 0]
        best, bp[:, t] = (delta[:, :, None] + Wt).max(dim=1)           # (torch.max hands out an arg-max, not promised to be the first)
        delta = torch.where(keep[:, t], unary[:, t] + best, ninf)
    return delta, bp


def t_backtrack(delta, bp):
    Q, n, k = bp.shape
    path = torch.empty((Q, n), dtype=torch.int64, device=bp.device)
    score, path[:, n - 1] = delta.max(dim=1)
    for t in range(n - 1, 0, -1):
        path[:, t - 1] = bp[:, t].gather(1, path[:, t:t + 1])[:, 0]
    return path, score


# ---- measurements ---------------------------------------------------------------------------------------------------------------
def bench_shape(Q, n, k, E, a, dev):
    import tube_ref as R
    from dcnet_amd import ops, postprocess
    c = R.gen_batch([31 * n + k + q for q in range(Q)], n, k, E)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    boxes, unary, feats = up(c["boxes"]), up(c["unary"]), up(c["feats"])
    keep8 = ops.post_nms(boxes.view(Q * n, k, 4), 0.6).view(Q, n, k)
    keep = keep8.view(torch.bool)
    assert ops.tube_ranges(Q, n, k) == [(0, n)], "the default workspace holds these shapes in one range"
    W = ops.tube_transitions(boxes, feats, 0, n, 1.0, 1.0)
    delta = torch.empty((Q, k), device=dev); backptr = torch.empty((Q, n, k), dtype=torch.uint8, device=dev)
    ops.tube_forward(W, unary, keep8, delta, 0, n, backptr)
    ev = lambda fn: _events(fn, a.warmup, a.repeat)
    hip = {"nms": ev(lambda: ops.post_nms(boxes.view(Q * n, k, 4), 0.6, out=keep8.view(Q * n, k))),
           "transitions": ev(lambda: ops.tube_transitions(boxes, feats, 0, n, 1.0, 1.0, W)),
           "forward": ev(lambda: ops.tube_forward(W, unary, keep8, delta, 0, n, backptr)),
           "backtrack": ev(lambda: ops.tube_backtrack(backptr, delta)),
           "link_tubes": ev(lambda: postprocess.link_tubes(boxes, unary, feats, keep, 1.0, 1.0))}
    hip["forward_us_per_step"] = round(hip["forward"] * 1e3 / (n - 1), 4)
    path, score, _ = postprocess.link_tubes(boxes, unary, feats, keep, 1.0, 1.0)
    # the torch arms; their results are compared so that the two sides time the same computation
    Wt = t_transitions(boxes, feats, 1, n)
    dt, bpt = t_forward(Wt, unary, keep)
    pt, st = t_backtrack(dt, bpt)
    same = {"keep": bool(torch.equal(t_nms(boxes.view(Q * n, k, 4), 0.6).view(Q, n, k), keep)), "path": bool(torch.equal(pt, path)),
            "score_maxdiff": float((st - score).abs().max())}
    tor = {"nms": ev(lambda: t_nms(boxes.view(Q * n, k, 4), 0.6)), "transitions": ev(lambda: t_transitions(boxes, feats, 1, n)),
           "forward": ev(lambda: t_forward(Wt, unary, keep)), "backtrack": ev(lambda: t_backtrack(dt, bpt))}
    tor["sum"] = round(sum(tor.values()), 4)
    per = {"forward_with_transitions": ev(lambda: t_forward(None, unary, keep, per_frame=(boxes, feats)))}
    per["sum"] = round(per["forward_with_transitions"] + tor["nms"] + tor["backtrack"], 4)
    return {"shape": [Q, n, k, E], "hip_ms": hip, "torch_ms": tor, "torch_per_frame_ms": per, "torch_agrees": same,
            "kept_per_centre": round(float(keep.float().sum(-1).mean()), 2)}


def bench_video(a, dev):
    from bench_video import build_model
    from dcnet_amd.utils.synth import synth_inputs
    from dcnet_amd.video import TubeLink, VideoGrounder
    m = build_model(a.size, dev)
    image, word_id, _ = synth_inputs(a.frames, a.size, n_queries=1, seed=1)
    image, word_id = image.to(dev), word_id.to(dev)
    arms = {"topk": VideoGrounder(m, n_frame=5, topk=a.topk), "topk_link": VideoGrounder(m, n_frame=5, topk=a.topk, link=TubeLink())}
    times = {name: [] for name in arms}
    for it in range(2 + 10):
        for name, vg in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vg.run(image, word_id)
            torch.cuda.synchronize()
            if it >= 2:
                times[name].append((time.perf_counter() - t0) * 1e3)
    med = {name: round(float(np.median(v)), 3) for name, v in times.items()}
    spread = {name: round(float(np.max(v) - np.min(v)), 3) for name, v in times.items()}
    return {"frames": a.frames, "size": a.size, "topk": a.topk, "run_ms": med, "run_spread_ms": spread,
            "link_share": round((med["topk_link"] - med["topk"]) / med["topk_link"], 4)}


# ---- streaming -------------------------------------------------------------------------------------------------
def _events_alt(fns, warmup, repeat):
    """median ms of every fn of the dict by device events, the arms alternated within each repetition"""
    ts = {name: [] for name in fns}
    for it in range(warmup + repeat):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            b.synchronize()
            if it >= warmup:
                ts[name].append(a.elapsed_time(b))
    return {name: round(float(np.median(v)), 4) for name, v in ts.items()}


def bench_stream_shape(Q, n, k, E, a, dev, push=32):
    """dcn_tube_stream_step (lags 8 and 64, pushes of ``push`` centres) against dcn_tube_forward (one launch, and the same pushes) on
    the same W; then a whole TubeStream.push of ``push`` centres (fusion, transitions, step, the host side's copies)."""
    import tube_ref as R
    from dcnet_amd import ops
    from dcnet_amd import video as V
    c = R.gen_batch([31 * n + k + q for q in range(Q)], n, k, E)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    boxes, unary, feats = up(c["boxes"]), up(c["unary"]), up(c["feats"])
    keep8 = ops.post_nms(boxes.view(Q * n, k, 4), 0.6).view(Q, n, k)
    W = ops.tube_transitions(boxes, feats, 0, n, 1.0, 1.0, torch.zeros((Q, n, k, k), device=dev))
    cuts = [(t, min(n, t + push)) for t in range(0, n, push)]
    Wp, up_, kp = ([x[:, t0:t1].contiguous() for t0, t1 in cuts] for x in (W, unary, keep8))
    delta = torch.empty((Q, k), device=dev); backptr = torch.empty((Q, n, k), dtype=torch.uint8, device=dev)
    forced = torch.zeros(Q, dtype=torch.int32, device=dev)
    surv = {lag: torch.zeros((Q, lag, k), dtype=torch.uint8, device=dev) for lag in (8, 64)}
    commit = torch.empty((Q, push), dtype=torch.int64, device=dev)

    def fwd_pushes():
        for (t0, t1), w in zip(cuts, Wp):
            ops.tube_forward(w, unary, keep8, delta, t0, t1, backptr)

    def stream(lag):
        for (t0, t1), w, u, kk in zip(cuts, Wp, up_, kp):
            ops.tube_stream_step(w, u, kk, t0, lag, delta, surv[lag], forced, commit[:, :t1 - t0] if t1 - t0 == push else None)

    forced.zero_(); stream(8); f8 = forced.tolist()
    forced.zero_(); stream(64); f64 = forced.tolist()
    ms = _events_alt({"forward": lambda: ops.tube_forward(W, unary, keep8, delta, 0, n, backptr), "forward_pushes": fwd_pushes,
                      "stream_lag8": lambda: stream(8), "stream_lag64": lambda: stream(64)}, a.warmup, a.repeat)
    us = {name: round(v * 1e3 / (n - 1), 4) for name, v in ms.items()}
    # one whole push of the Python front end, steady state (the stream is ``push`` centres past its start)
    part = lambda lo: V.VideoResult(centres=torch.arange(lo, lo + push, device=dev), outbox=[], sim=[], loc=[], corr_feat=[], only_obj=[],
                                    boxes=boxes[:, lo:lo + push, 0], cand_boxes=boxes[:, lo:lo + push], cand_scores=unary[:, lo:lo + push],
                                    cand_feats=feats[:, lo:lo + push], cand_keep=keep8[:, lo:lo + push])
    pushes = {}
    for lag in (8, 64):
        for un in ("score", "fused"):
            ts = V.TubeStream(V.TubeLink(unary=un), 5, lag)
            ts.push(part(0)); ts.push(part(push))
            lo = [2 * push]

            def one(ts=ts, lo=lo):
                ts.push(part(lo[0]))
                lo[0] = (lo[0] + push) % (n - push)                         # (any centres will do: the cost does not depend on them)
            pushes[f"lag{lag}_{un}"] = _events(one, a.warmup, a.repeat)
            pushes[f"lag{lag}_{un}_state_bytes"] = ts.state_bytes()
    return {"shape": [Q, n, k, E], "push": push, "ms": ms, "us_per_step": us,
            "commit_overhead_us_per_step": {"lag8": round(us["stream_lag8"] - us["forward_pushes"], 4),
                                            "lag64": round(us["stream_lag64"] - us["forward_pushes"], 4)},
            "forced": {"lag8": f8, "lag64": f64}, "tube_stream_push_ms": pushes}


def bench_stream_video(a, dev):
    """VideoGrounder.run with link against the same frames pushed through a TubeStream (no part kept): wall time around a synchronise,
    peak memory, the stream's state; and the device time of TubeStream.push against that of VideoGrounder.push, per push."""
    from bench_video import build_model
    from dcnet_amd.utils.synth import synth_inputs
    from dcnet_amd.video import TubeLink, VideoGrounder
    m = build_model(a.size, dev)
    image, word_id, _ = synth_inputs(a.frames, a.size, n_queries=1, seed=1)
    image, word_id = image.to(dev), word_id.to(dev)
    vg = VideoGrounder(m, n_frame=5, topk=a.topk, link=TubeLink(), chunk=32)
    shares = []

    def streamed(lag=16, timed=False):
        vg.reset(word_id, total=a.frames)
        ts = vg.tube_stream(lag)
        state = 0
        for i0 in range(0, a.frames, 32):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record(); part = vg.push(image[i0:i0 + 32]); e[1].record(); ts.push(part); e[2].record()
            del part
            state = max(state, ts.state_bytes())
            if timed and i0 >= 32:
                e[2].synchronize()
                shares.append((e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])))
        ts.push(vg.flush())
        return ts.flush(), state, ts.forced

    arms = {"run": lambda: vg.run(image, word_id), "streamed": streamed}
    times, peak = {name: [] for name in arms}, {}
    for it in range(2 + 6):
        for name, fn in arms.items():
            torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if it >= 2:
                times[name].append((time.perf_counter() - t0) * 1e3)
            peak[name] = torch.cuda.max_memory_allocated()
            del out
    _, state, forced = streamed(timed=True)
    ground, link = (float(np.median([s[i] for s in shares])) for i in range(2))
    return {"frames": a.frames, "size": a.size, "topk": a.topk, "lag": 16,
            "wall_ms": {name: round(float(np.median(v)), 3) for name, v in times.items()},
            "wall_spread_ms": {name: round(float(np.max(v) - np.min(v)), 3) for name, v in times.items()},
            "peak_bytes": peak, "state_bytes": state, "forced": forced.tolist(),
            "push32_ms": {"grounder": round(ground, 3), "tube_stream": round(link, 3), "share": round(link / (ground + link), 4)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stream", action="store_true", help="the streaming entries and front end (DESIGN.md section 14) instead")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--topk", type=int, default=20)
    ap.add_argument("--no-video", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.stream:
        res = {"stream_entries": [bench_stream_shape(*s, a, dev) for s in SHAPES]}
        if not a.no_video:
            res["stream_video"] = bench_stream_video(a, dev)
        print(json.dumps(res))
        return
    res = {"entries": [bench_shape(*s, a, dev) for s in SHAPES]}
    if not a.no_video:
        res["video"] = bench_video(a, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
