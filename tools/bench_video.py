"""Whole-video grounding against what a user does today, in one process (a tool, not bench.py).

    python tools/bench_video.py                    # F = 64 frames, 416x416, n_frame = 5, one query, fp32, forward only
    python tools/bench_video.py --baseline-only    # arm (b) alone: runs on a tree without dcnet_amd.video as well
    python tools/bench_video.py --frames 32 --size 608 --n-frame 16 --windows 4      # BASELINE configs[3]'s geometry
    python tools/bench_video.py --precision bf16s  # both arms on bf16 storage, plus arm (c): VideoGrounder in fp32 on its own model

Arm (a): ``VideoGrounder.run`` on the whole video.  Arm (b): the same "valid" centres as explicit windows through
``model(windows, word_id, None, n_frame)`` in batches of ``--windows`` windows — every frame is encoded once per window it appears
in.  Both arms alternate in one process; medians of ``--repeat`` runs after ``--warmup``; frames/s = frames of the VIDEO per second
(both arms answer the same centres).  Prints one JSON line.
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


def build_model(size, dev):
    from dcnet_amd.model import grounding_model
    from dcnet_amd.utils.synth import apply_bn_calibration, synth_state_dict
    gold = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gold, "state_dict_keys_256.json")) as f:
        shapes = {k: tuple(v) for k, v in json.load(f).items()}
    shapes["loc_text_embedding.0.weight"] = (512, sum((size // 32 * 2 ** i) ** 2 for i in range(3)))
    sd = apply_bn_calibration(synth_state_dict(shapes, 0), os.path.join(gold, "bn_calib.npz"))
    m = grounding_model(corpus=list(range(1000)), light=False, emb_size=512, coordmap=True, dataset="vid", img_size=size,
                        config_path=os.path.join(ROOT, "model", "yolov3.cfg"), weights_path=None)
    m.load_state_dict(sd, strict=True)
    return m.to(dev).eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--n-frame", type=int, default=5)
    ap.add_argument("--windows", type=int, default=12, help="windows per call of the windowed arm")
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--precision", default="fp32", choices=("fp32", "bf16s"),
                    help="ops.set_precision mode of both arms; bf16s adds a third arm, VideoGrounder in fp32 on a model of its own")
    a = ap.parse_args()
    from dcnet_amd import ops
    ops.set_precision(a.precision)                   # (before the model is built)
    try:
        run(a)
    finally:
        ops.set_precision("fp32")


def run(a):
    from dcnet_amd import ops
    from dcnet_amd.utils.synth import synth_inputs
    dev = torch.device("cuda:0")
    m = build_model(a.size, dev)
    image, word_id, _ = synth_inputs(a.frames, a.size, n_queries=1, seed=1)
    image, word_id = image.to(dev), word_id.to(dev)
    K, F = a.n_frame, a.frames
    cs = list(range(K // 2, F - (K + 1) // 2 + 1))
    idx = torch.tensor([[i + o for o in range(-(K // 2), (K + 1) // 2)] for i in cs], device=dev)

    def windowed():
        out = []
        with torch.no_grad():
            for w0 in range(0, len(cs), a.windows):
                sel = idx[w0:w0 + a.windows]
                clips = image[sel.reshape(-1)]                       # (the gather is part of what a user pays today)
                out.append(m(clips, word_id.expand(sel.shape[0], -1).contiguous(), None, K)[0][0])
        return out

    arms = {"windowed": windowed}
    if not a.baseline_only:
        from dcnet_amd.video import VideoGrounder
        vg = VideoGrounder(m, n_frame=K, border="valid", chunk=a.chunk)
        arms["video"] = lambda: vg.run(image, word_id)
        bank = {"video": vg.bank_bytes_per_frame(a.size)}
        if a.precision != "fp32":
            ops.set_precision("fp32")
            try:
                vg32 = VideoGrounder(build_model(a.size, dev), n_frame=K, border="valid", chunk=a.chunk)
                bank["video_fp32"] = vg32.bank_bytes_per_frame(a.size)
            finally:
                ops.set_precision(a.precision)

            def video_fp32():
                ops.set_precision("fp32")
                try:
                    return vg32.run(image, word_id)
                finally:
                    ops.set_precision(a.precision)
            arms["video_fp32"] = video_fp32
    times = {k: [] for k in arms}
    peak = {}
    for it in range(a.warmup + a.repeat):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times[name].append(time.perf_counter() - t0)
            peak[name] = torch.cuda.max_memory_allocated() / 2 ** 30
    res = {"frames": F, "size": a.size, "n_frame": K, "centres": len(cs), "windows_per_call": a.windows, "chunk": a.chunk,
           "precision": a.precision}
    for name in arms:
        t = float(np.median(times[name]))
        res[name] = {"ms": round(t * 1e3, 2), "frames_per_s": round(F / t, 1), "peak_gib": round(peak[name], 2)}
        if not a.baseline_only and name in bank:
            res[name]["bank_bytes_per_frame"] = bank[name]
    if "video" in res:
        res["speedup"] = round(res["windowed"]["ms"] / res["video"]["ms"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
