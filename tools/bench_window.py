"""Timing of window training (the n_frame model in train mode: functions.CoAttentionWindow on csrc/coattn_center.hip, losses.window_loss,
graph.GraphedTrainStep(..., n_frame=K)), every measurement in a child process of its own, the children run in interleaved rounds, medians
reported, the device's clock printed with every figure:

    python tools/bench_window.py [--against DIR] [--rounds 3] [--modes fp32,bf16s] [--json out.json]

The window model at --size 416 --clips 8 --n-frame 5, in fp32 and in bf16 storage: ms per step (wall clock around --iters steps,
host-synchronised at both ends) and torch.cuda.max_memory_allocated (the peak of the whole child: warm-up — and, for the replayed step,
its eager warm-up steps and the capture's private pool — included).  The arms:

    eager             forward + the three dense losses + backward, eagerly, no optimiser (gradients dropped before every backward)
    eager@other       the same on another checkout of the project (``--against DIR``: the parent commit, built there)
    step              the replayed training step (RMSprop); this tree only — the parent has no captured window step

The eager arm spells its loss out with what both trees have (losses.neg_sim_score, losses.dense_losses: the body of losses.window_loss),
so the two trees run the same script.  Two conditions are reported per mode: ``eager`` is not slower than the other tree beyond that
tree's own run-to-run spread (median - other's median <= max - min of the other's runs), and it holds less memory.

A child measures one arm in one tree and prints one JSON line; nothing here runs without a GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _clock(torch):
    """MHz: the device's current shader clock where the runtime reports it, and its maximum"""
    khz = getattr(torch.cuda.get_device_properties(0), "clock_rate", None)          # (not every torch build exposes it)
    out = {"max_mhz": None if khz is None else round(khz / 1e3)}
    try:
        out["now_mhz"] = int(torch.cuda.clock_rate())
    except Exception:
        out["now_mhz"] = None
    return out


def child(root, size, clips, n_frame, iters, warmup, mode, arm):
    import torch
    from dcnet_amd import losses, ops
    from dcnet_amd.model import grounding_model
    from dcnet_amd.parallel import freeze_gradless
    from dcnet_amd.train import make_optimizer
    from dcnet_amd.utils.synth import synth_boxes, synth_inputs
    dev = torch.device("cuda:0")
    ops.set_precision(mode)
    image, word_id, word_mask = (t.to(dev) for t in synth_inputs(clips * n_frame, size, n_queries=clips, seed=100))
    bbox = synth_boxes(clips, size, seed=100).to(dev)
    random.seed(13)
    torch.manual_seed(1234)
    m = grounding_model(corpus=list(range(1000)), light=False, emb_size=512, coordmap=True, bert_model="bert-base-uncased", dataset="vid",
                        img_size=size, config_path=os.path.join(root, "model", "yolov3.cfg"), weights_path=None).to(dev)
    m.train(); freeze_gradless(m)
    if arm == "step":
        from dcnet_amd.graph import GraphedTrainStep
        step = GraphedTrainStep(m, make_optimizer(m, 1e-4), image, word_id, word_mask, bbox, size, warmup=max(1, warmup), n_frame=n_frame)
        last = lambda: step.loss
    else:
        box = {}

        def step():
            pred, sim, loc, corr_feat, flang_attn = m(image, word_id, word_mask, n_frame)
            yolo, rank, locl = losses.dense_losses(pred, sim, losses.neg_sim_score(corr_feat, flang_attn), loc, bbox, size)
            for p_ in m.parameters():
                p_.grad = None
            box["loss"] = yolo + 100 * rank + locl
            box["loss"].backward()

        last = lambda: box["loss"].detach()
    for _ in range(max(1, warmup)):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        step()
    torch.cuda.synchronize()
    return {"ms": round((time.perf_counter() - t0) / iters * 1e3, 3), "iters": iters,
            "max_memory_allocated_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 3), "loss": float(last()),
            "geometry": f"{clips} clips x n_frame {n_frame} at {size}x{size}", "clock": _clock(torch)}


def _spawn(root, what, args):
    """One measurement in a fresh process whose dcnet_amd is the one of ``root``.  Returns its JSON line as a dict."""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--root", root, "--size", str(args.size), "--clips", str(args.clips),
           "--n-frame", str(args.n_frame), "--iters", str(args.iters), "--warmup", str(args.warmup)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout, cwd=root)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def summarise(runs: dict) -> dict:
    """{arm: [child results]} of one mode -> medians, the other tree's spread and the two conditions (None where there is no other tree)."""
    out = {k: {"median_ms": round(statistics.median(r["ms"] for r in v), 3), "runs_ms": [r["ms"] for r in v],
               "max_memory_allocated_gb": max(r["max_memory_allocated_gb"] for r in v)}
           for k, v in runs.items() if v}
    other = out.get("eager@other")
    if other is not None:
        spread = max(other["runs_ms"]) - min(other["runs_ms"])
        out["other_spread_ms"] = round(spread, 3)
        out["eager_not_slower_than_other"] = out["eager"]["median_ms"] - other["median_ms"] <= spread
        out["eager_holds_less_memory"] = out["eager"]["max_memory_allocated_gb"] < other["max_memory_allocated_gb"]
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--against", default="", metavar="DIR", help="also the eager arm on this checkout of the project, alternating")
    ap.add_argument("--modes", default="fp32,bf16s")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--n-frame", type=int, default=5)
    ap.add_argument("--child-timeout", type=int, default=600)
    ap.add_argument("--json", default="")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.child:
        sys.path.insert(0, args.root)
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_window: no GPU (nothing here is measured on a CPU)")
        mode, arm = args.child.split(":")
        print(json.dumps(child(args.root, args.size, args.clips, args.n_frame, args.iters, args.warmup, mode, arm)), flush=True)
        return
    report = {}
    for mode in [m_ for m_ in args.modes.split(",") if m_]:
        arms = [("eager", ROOT)] + ([("eager@other", os.path.abspath(args.against))] if args.against else []) + [("step", ROOT)]
        runs = {k: [] for k, _ in arms}
        for _ in range(args.rounds):
            for k, root in arms:
                runs[k].append(_spawn(root, f"{mode}:{k.split('@')[0]}", args))
                print(json.dumps({"mode": mode, "arm": k, **runs[k][-1]}), flush=True)
        report[mode] = summarise(runs)
    print(json.dumps(report), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(report, fh, indent=1)


if __name__ == "__main__":
    main()
