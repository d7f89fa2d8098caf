"""Timing of the frozen-BatchNorm paths (csrc/frozen_bn.h, grounding_model.freeze_batchnorm), every measurement in a child process of its
own, the children run in interleaved rounds, medians reported, the device's clock printed with every figure:

    python tools/bench_frozen.py --eval [--against DIR] [--rounds 3]      # (a)
    python tools/bench_frozen.py --steps [--rounds 2]                      # (b)
    python tools/bench_frozen.py --eval --steps --json out.json

(a) ``model.eval()`` with gradients on, fp32, forward + backward of a linear objective over outbox and sim_score at 8 x 416^2 (HIP events
    around the pair, warm, median over --iters).  ``--against DIR``: the same measurement on another checkout of the project (the parent
    commit, built: ``python -m dcnet_amd.build`` there), alternating with this one, ``--rounds`` runs each.  The condition reported:
    this tree's median is no more than the other's median plus the spread (max - min) of the other's runs.
(b) The replayed training step (graph.GraphedTrainStep, RMSprop) at BASELINE configs[1] — 8 clips x T 8 at 416 x 416 — with BatchNorm
    frozen nowhere, in the backbone, everywhere (gamma and beta training), in fp32 and in bf16 storage: ms per step (wall clock around
    --iters replays, host-synchronised at both ends) and torch.cuda.max_memory_allocated.  Reported, not judged.

A child measures one configuration in one tree and prints one JSON line; nothing here runs without a GPU.
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


def _model(root, size, dev):
    import torch
    from dcnet_amd.model import grounding_model
    torch.manual_seed(1234)
    return grounding_model(corpus=list(range(1000)), light=False, emb_size=512, coordmap=True, bert_model="bert-base-uncased", dataset="vid",
                           img_size=size, config_path=os.path.join(root, "model", "yolov3.cfg"), weights_path=None).to(dev)


def child_eval(root, size, n, iters, warmup):
    import torch
    from dcnet_amd.utils.synth import synth_inputs
    dev = torch.device("cuda:0")
    m = _model(root, size, dev).eval()
    image, word_id, word_mask = (t.to(dev) for t in synth_inputs(n, size, seed=100))
    gs = None
    ms = []
    for it in range(warmup + iters):
        m.zero_grad(set_to_none=True)
        random.seed(5)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        outbox, sim, _, _ = m(image, word_id, word_mask)
        if gs is None:
            g = torch.Generator(device=dev).manual_seed(9)
            gs = [torch.randn(o.shape, device=dev, generator=g) for o in list(outbox) + list(sim)]
        sum((o * g_).sum() for o, g_ in zip(list(outbox) + list(sim), gs)).backward()
        b.record(); b.synchronize()
        if it >= warmup:
            ms.append(a.elapsed_time(b))
    return {"ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "iters": iters,
            "geometry": f"{n} x {size}x{size}", "clock": _clock(torch)}


def child_step(root, size, clips, iters, warmup, mode, scope):
    import torch
    from dcnet_amd import ops
    from dcnet_amd.graph import GraphedTrainStep
    from dcnet_amd.parallel import freeze_gradless
    from dcnet_amd.train import make_optimizer
    from dcnet_amd.utils.synth import synth_boxes, synth_inputs
    dev = torch.device("cuda:0")
    n = clips * 8
    ops.set_precision(mode)
    image, word_id, word_mask = (t.to(dev) for t in synth_inputs(n, size, seed=100))
    bbox = synth_boxes(n, size, seed=100).to(dev)
    random.seed(13)
    m = _model(root, size, dev)
    m.train(); freeze_gradless(m)
    if scope != "none":
        m.freeze_batchnorm(scope)
    step = GraphedTrainStep(m, make_optimizer(m, 1e-4), image, word_id, word_mask, bbox, size, warmup=max(1, warmup))
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        step()
    torch.cuda.synchronize()
    return {"ms": round((time.perf_counter() - t0) / iters * 1e3, 3), "iters": iters, "max_memory_allocated_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
            "loss": float(step.loss), "geometry": f"{clips} clips x T 8 at {size}x{size}", "clock": _clock(torch)}


def _spawn(root, what, args, limit):
    """One measurement in a fresh process whose dcnet_amd is the one of ``root``.  Returns its JSON line as a dict."""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--root", root, "--size", str(args.size), "--clips", str(args.clips),
           "--iters", str(args.iters), "--warmup", str(args.warmup)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, cwd=root)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--eval", action="store_true", help="(a) fp32 eval forward + backward")
    ap.add_argument("--against", default="", metavar="DIR", help="(a) also on this checkout of the project, alternating")
    ap.add_argument("--steps", action="store_true", help="(b) the replayed training step, --freeze-bn none / backbone / all, fp32 and bf16s")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--child-timeout", type=int, default=600)
    ap.add_argument("--json", default="")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.child:
        sys.path.insert(0, args.root)
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_frozen: no GPU (nothing here is measured on a CPU)")
        if args.child == "eval":
            res = child_eval(args.root, args.size, args.clips, args.iters, args.warmup)
        else:
            mode, scope = args.child.split(":")
            res = child_step(args.root, args.size, args.clips, args.iters, args.warmup, mode, scope)
        print(json.dumps(res), flush=True)
        return
    report = {}
    if args.eval:
        trees = {"this": ROOT}
        if args.against:
            trees["other"] = os.path.abspath(args.against)
        runs = {k: [] for k in trees}
        for _ in range(args.rounds):
            for k, root in trees.items():
                runs[k].append(_spawn(root, "eval", args, args.child_timeout))
                print(json.dumps({"eval": k, **runs[k][-1]}), flush=True)
        ev = {k: {"median_ms": round(statistics.median(r["ms"] for r in v), 3), "runs_ms": [r["ms"] for r in v]} for k, v in runs.items()}
        if "other" in ev:
            spread = max(ev["other"]["runs_ms"]) - min(ev["other"]["runs_ms"])
            ev["other_spread_ms"] = round(spread, 3)
            ev["not_slower_than_other"] = ev["this"]["median_ms"] <= ev["other"]["median_ms"] + spread
        report["eval_fwd_bwd"] = ev
    if args.steps:
        keys = [f"{mode}:{scope}" for mode in ("fp32", "bf16s") for scope in ("none", "backbone", "all")]
        runs = {k: [] for k in keys}
        for _ in range(args.rounds):
            for k in keys:
                runs[k].append(_spawn(ROOT, k, args, args.child_timeout))
                print(json.dumps({"step": k, **runs[k][-1]}), flush=True)
        report["replayed_step"] = {k: {"median_ms": round(statistics.median(r["ms"] for r in v), 3), "runs_ms": [r["ms"] for r in v],
                                       "max_memory_allocated_gb": max(r["max_memory_allocated_gb"] for r in v)} for k, v in runs.items()}
    print(json.dumps(report), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(report, fh, indent=1)


if __name__ == "__main__":
    main()
