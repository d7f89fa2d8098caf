"""Clip preprocessing (csrc/prep.hip dcn_clip_prep) on one GPU: device time per batch, fraction of the HBM roofline on the
algorithmic bytes, the pinned host-to-device copy of the raw bytes, and the host time of the draws + geometry and of packing.

    python tools/bench_prep.py [--iters 20] [--warmup 3] [--json out.json]

Algorithmic bytes = source frames read once + fp32 output written + the uint8 RGBx letterbox intermediate written and read
once (two launches).  Device times are HIP events around the call on a warm, otherwise idle GPU; medians over --iters.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dcnet_amd import prep            # noqa: E402
from dcnet_amd.lib import lib         # noqa: E402

HBM_PEAK = 8.0e12                     # MI355X HBM3E peak (MI355X_MICROARCH.md); ~6.3e12 achievable by a streaming copy

CASES = [("B8_T8_1280x720_to_416", 8, 8, (720, 1280), 416), ("B32_T8_1280x720_to_416", 32, 8, (720, 1280), 416),
         ("B8_T8_500x375_to_608", 8, 8, (375, 500), 608)]


def _events(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def bench_case(name, B, T, hw, S, augment, iters, warmup):
    rs = np.random.RandomState(0)
    h, w = hw
    frames = [[rs.randint(0, 256, size=(h, w, 3), dtype=np.uint8) for _ in range(T)] for _ in range(B)]
    boxes = [[[100, 80, 600, 500]] * T for _ in range(B)]
    phrases = [["the dog on the left"] * T for _ in range(B)]
    n = B * T
    t0 = time.perf_counter()
    for _ in range(5):
        plan = prep.plan_batch(frames, boxes, phrases, S, augment, rng=random.Random(1))
    host_plan_ms = (time.perf_counter() - t0) / 5 * 1e3
    pinned = torch.empty(plan.src_bytes, dtype=torch.uint8).pin_memory()
    pv = pinned.numpy()
    t0 = time.perf_counter()
    for _ in range(3):
        i = 0
        for clip in frames:
            for f in clip:
                off = int(plan.jobs[i]["src_off"])
                pv[off:off + f.size] = f.reshape(-1)
                i += 1
    host_pack_ms = (time.perf_counter() - t0) / 3 * 1e3
    dev = torch.device("cuda:0")
    src = torch.empty(plan.src_bytes, dtype=torch.uint8, device=dev)
    h2d_ms = _events(lambda: src.copy_(pinned, non_blocking=True), iters, warmup)
    jobs_dev = torch.from_numpy(plan.jobs.view(np.uint8).copy()).to(dev)
    out = torch.empty((n, 3, S, S), dtype=torch.float32, device=dev)
    ws = torch.empty(int(lib().clip_prep_ws(n, S)), dtype=torch.uint8, device=dev)
    L = lib()
    s = torch.cuda.current_stream().cuda_stream
    call = lambda: L.clip_prep(src.data_ptr(), plan.src_bytes, jobs_dev.data_ptr(), plan.jobs.ctypes.data, n, S, ws.data_ptr(),
                               out.data_ptr(), None, s)
    dev_ms = _events(call, iters, warmup)
    src_b = sum(f.size for c in frames for f in c)
    alg = src_b + out.numel() * 4 + 2 * n * S * S * 4
    # end to end through prepare_clips (host plan + pack + staged copy + kernels), per call, host-synchronised
    prep.prepare_clips(frames, boxes, phrases, S, augment, rng=random.Random(2))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(3):
        prep.prepare_clips(frames, boxes, phrases, S, augment, rng=random.Random(3 + k))
    torch.cuda.synchronize()
    e2e_ms = (time.perf_counter() - t0) / 3 * 1e3
    return {"case": name, "augment": augment, "frames": n, "size": S, "device_ms": round(dev_ms, 4),
            "alg_MB": round(alg / 1e6, 1), "alg_TBps": round(alg / dev_ms / 1e9, 3), "frac_hbm_peak": round(alg / dev_ms / 1e9 / (HBM_PEAK / 1e12), 3),
            "h2d_ms": round(h2d_ms, 3), "h2d_GBps": round(src_b / h2d_ms / 1e6, 1), "host_plan_ms": round(host_plan_ms, 2),
            "host_pack_ms": round(host_pack_ms, 2), "prepare_clips_ms": round(e2e_ms, 2)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="first case only, training mode (for a profiler run)")
    ap.add_argument("--json", default="")
    a = ap.parse_args(argv)
    rows = []
    for name, B, T, hw, S in CASES[:1] if a.quick else CASES:
        for augment in ((True,) if a.quick else (True, False)):
            r = bench_case(name, B, T, hw, S, augment, a.iters, a.warmup)
            print(json.dumps(r), flush=True)
            rows.append(r)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
