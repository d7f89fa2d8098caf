"""The fused Adam / SGD steps (csrc/optim.hip) against torch's foreach steps, on the trained parameter shapes of the real model
(synthetic weights, random gradients), alternating in one process:

    python tools/bench_optim.py [--iters 20] [--warmup 3] [--step] [--clip | --ema | --accum K] [--json out.json]

Per optimiser one JSON line: ms per step of ``torch.optim.{Adam,SGD}(foreach=True)`` and of ``dcnet_amd.optim.{Adam,SGD}`` (HIP events
around ``step()`` on a warm, otherwise idle GPU; medians over --iters, the two sides measured in turns), the bytes a step has to move
(Adam 16 B read + 12 B written per value, SGD 12 B + 8 B) and the fraction of the HBM peak the fused step reaches on them.

``--step`` adds the whole training step at configs[1]'s geometry (8 clips x T 8 at 416x416): the eager ``train_step`` with
``torch.optim.Adam`` — what Adam training had to run before the fused class could be captured — against the replayed hipGraph with
the fused Adam (wall clock per step over --step-iters steps, host-synchronised at both ends).

``--clip`` times global-norm gradient clipping instead: per optimiser (RMSprop, Adam, SGD) four steps on the same shapes, measured in
turns in one process — (a) the fused step, (b) the fused step with ``max_grad_norm`` (dcn_grad_sumsq + dcn_grad_clip_coef + the clipped
update), (c) torch's foreach step, (d) ``torch.nn.utils.clip_grad_norm_(foreach=True)`` + torch's foreach step — and reports b - a
against d - c and against the HBM time of one read of the gradients, which is all the extra pass has to move.  With ``--step`` as
well: the replayed RMSprop training step at configs[1]'s geometry with and without clipping, two graphs alive in one process,
measured in alternating blocks.

``--ema`` times the weight EMA instead (``dcnet_amd.optim.WeightEMA``) on the model's own tensors — every floating-point entry of its
``state_dict()``: one update (dcn_ema_prepare + dcn_ema_update, 12 B per value), ``torch._foreach_lerp_`` on the same tensors, one
``rmsprop_kernel`` step over tensors of the same shapes (20 B per value) and one ``swap()`` (16 B per value), measured in turns in one
process, in --rounds rounds of --iters; per side the median of the round medians, the achieved GB/s and fraction of the HBM peak,
and the spread of the round medians.  The EMA pass and RMSprop are both pure streaming passes over the same tensor list, so the
figure to read is ``ema_frac_minus_rmsprop_frac`` against ``frac_round_spread``.  With ``--step`` as well: the replayed RMSprop
training step at configs[1]'s geometry without and with an attached EMA, two graphs alive in one process, alternating blocks.

``--accum K`` times the gradient-accumulation pass instead (dcn_grad_accumulate) on the model's trained tensors: the pass in its first
(8 B per value), middle and boundary phase (12 B), ``torch._foreach_add_`` on the same tensors (12 B) and dcn_ema_update on the same
tensors (the file's other 12 B pass), measured in turns in one process, --rounds rounds of --iters; ms, TB/s and the spread of the
round medians per side.  With ``--step`` as well: the replayed RMSprop training step at configs[1]'s geometry with ``accum_steps=1``
and with ``accum_steps=K`` (ms per micro-step), two graphs alive in one process, alternating blocks.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import random
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dcnet_amd import optim            # noqa: E402

HBM_PEAK = 8.0e12                      # MI355X HBM3E peak (MI355X_MICROARCH.md); ~6.3e12 achievable by a streaming copy
BYTES_PER_VALUE = {"adam": 28, "sgd": 20}


def build_model(size, dev):
    from dcnet_amd.model import grounding_model
    from dcnet_amd.parallel import freeze_gradless
    torch.manual_seed(1234)
    model = grounding_model(corpus=list(range(1000)), light=False, emb_size=512, coordmap=True, bert_model="bert-base-uncased",
                            dataset="vid", img_size=size, config_path=os.path.join(ROOT, "model", "yolov3.cfg"), weights_path=None).to(dev)
    model.train(); freeze_gradless(model)
    return model


def _make(name, params, fused, **clip):
    if name == "rmsprop":
        return optim.RMSprop(params, lr=1e-4, weight_decay=5e-4, **clip) if fused else torch.optim.RMSprop(params, lr=1e-4, weight_decay=5e-4, foreach=True)
    if clip:
        return optim.Adam(params, lr=1e-4, weight_decay=5e-4, **clip) if name == "adam" else optim.SGD(params, lr=1e-4, momentum=0.99, **clip)
    if name == "adam":
        return optim.Adam(params, lr=1e-4, weight_decay=5e-4) if fused else torch.optim.Adam(params, lr=1e-4, weight_decay=5e-4, foreach=True)
    return optim.SGD(params, lr=1e-4, momentum=0.99) if fused else torch.optim.SGD(params, lr=1e-4, momentum=0.99, foreach=True)


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    b.synchronize()
    return a.elapsed_time(b)


def bench_steps(name, shapes, dev, iters, warmup):
    g = torch.Generator(device=dev).manual_seed(0)
    sides = {}
    for fused in (False, True):
        ps = [torch.nn.Parameter(torch.randn(s, device=dev, generator=g) * 0.05) for s in shapes]
        for p in ps:
            p.grad = torch.randn(p.shape, device=dev, generator=g) * 1e-3
        sides[fused] = _make(name, ps, fused)
    for _ in range(warmup):
        for o in sides.values():
            o.step()
    torch.cuda.synchronize()
    ts = {False: [], True: []}
    for _ in range(iters):
        for fused, o in sides.items():
            ts[fused].append(_timed(o.step))
    n = sum(int(torch.Size(s).numel()) for s in shapes)
    t_ms, f_ms = statistics.median(ts[False]), statistics.median(ts[True])
    alg = n * BYTES_PER_VALUE[name]
    return {"optimizer": name, "tensors": len(shapes), "values_M": round(n / 1e6, 2), "alg_GB": round(alg / 1e9, 3),
            "torch_foreach_ms": round(t_ms, 4), "fused_ms": round(f_ms, 4), "speedup": round(t_ms / f_ms, 2),
            "fused_TBps": round(alg / f_ms / 1e9, 3), "frac_hbm_peak": round(alg / f_ms / 1e9 / (HBM_PEAK / 1e12), 3)}


def bench_clip(name, shapes, dev, iters, warmup, max_norm=1.0):
    """(a) fused, (b) fused + max_grad_norm, (c) torch foreach, (d) torch clip_grad_norm_(foreach=True) + foreach step; gradients
    randn * 1e-3 (norm ~ 1e-3 * sqrt(values) = 8.6 at 74 M values), so ``max_norm`` = 1 clips.  (d) scales its gradients in place, so
    from its second step on its coefficient is ~1; its launches and bytes are the same either way."""
    g = torch.Generator(device=dev).manual_seed(0)
    sides = {}
    for key, fused, clip in (("a", True, {}), ("b", True, {"max_grad_norm": max_norm}), ("c", False, {}), ("d", False, {})):
        ps = [torch.nn.Parameter(torch.randn(s, device=dev, generator=g) * 0.05) for s in shapes]
        for p in ps:
            p.grad = torch.randn(p.shape, device=dev, generator=g) * 1e-3
        o = _make(name, ps, fused, **clip)
        if key == "d":
            def run(o=o, ps=ps):
                torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=True)
                o.step()
            sides[key] = run
        else:
            sides[key] = o.step
        if key == "b":
            clipped = o
    for _ in range(warmup):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    norm = float(clipped.grad_norm)
    ts = {k: [] for k in sides}
    for _ in range(iters):
        for k, fn in sides.items():
            ts[k].append(_timed(fn))
    n = sum(int(torch.Size(s).numel()) for s in shapes)
    ms = {k: statistics.median(v) for k, v in ts.items()}
    read_ms = n * 4 / HBM_PEAK * 1e3
    return {"optimizer": name, "clip": True, "tensors": len(shapes), "values_M": round(n / 1e6, 2), "grad_norm": round(norm, 4), "max_norm": max_norm,
            "a_fused_ms": round(ms["a"], 4), "b_fused_clip_ms": round(ms["b"], 4), "c_torch_foreach_ms": round(ms["c"], 4),
            "d_torch_clip_foreach_ms": round(ms["d"], 4), "b_minus_a_ms": round(ms["b"] - ms["a"], 4), "d_minus_c_ms": round(ms["d"] - ms["c"], 4),
            "grad_read_hbm_peak_ms": round(read_ms, 4), "b_minus_a_over_grad_read": round((ms["b"] - ms["a"]) / read_ms, 2),
            "spread_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ts.items()}}


def bench_train_step_clip(dev, size, clips, iters, warmup, max_norm=1.0, rounds=3):
    """The replayed RMSprop training step without and with ``max_grad_norm``: two models, two graphs, alternating blocks of ``iters``
    steps (wall clock per step, host-synchronised at both ends of a block); per side the median over the blocks."""
    from dcnet_amd.graph import GraphedTrainStep
    from dcnet_amd.train import make_optimizer
    from dcnet_amd.utils.synth import synth_boxes, synth_inputs
    n = clips * 8
    image, word_id, word_mask = (t.to(dev) for t in synth_inputs(n, size, seed=100))
    bbox = synth_boxes(n, size, seed=100).to(dev)
    steps = {}
    for key, clip in (("plain", {}), ("clipped", {"max_grad_norm": max_norm})):
        random.seed(13)
        model = build_model(size, dev)
        steps[key] = GraphedTrainStep(model, make_optimizer(model, 1e-4, "rmsprop", **clip), image, word_id, word_mask, bbox, size, warmup=max(1, warmup))
        for _ in range(warmup):
            steps[key]()
    torch.cuda.synchronize()
    blocks = {k: [] for k in steps}
    for _ in range(rounds):
        for key, step in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                step()
            torch.cuda.synchronize()
            blocks[key].append((time.perf_counter() - t0) / iters * 1e3)
    return {"geometry": f"{clips} clips x T 8 at {size}x{size}", "steps_per_block": iters, "blocks": rounds, "max_norm": max_norm,
            "grad_norm_last": round(float(steps["clipped"].grad_norm), 4),
            "replayed_rmsprop_ms": round(statistics.median(blocks["plain"]), 3), "replayed_rmsprop_clip_ms": round(statistics.median(blocks["clipped"]), 3),
            "blocks_ms": {k: [round(x, 3) for x in v] for k, v in blocks.items()}}


def bench_ema(dev, size, iters, warmup, rounds=3):
    """(a) WeightEMA.update, (b) torch._foreach_lerp_ on the same tensors, (c) the fused RMSprop step over tensors of the same shapes,
    (d) WeightEMA.swap — HIP events around each, the four measured in turns; ``rounds`` rounds of ``iters``."""
    model = build_model(size, dev)
    ema = optim.WeightEMA(model, decay=0.9999, tau=2000.0)
    src = list(ema._src)
    g = torch.Generator(device=dev).manual_seed(0)
    with torch.no_grad():
        for v in src:                        # the weights have moved since the shadows were taken
            v.add_(torch.randn(v.shape, device=dev, generator=g) * 1e-3)
    lerp_shadow = [v.clone() for v in ema._shadow]
    ps = [torch.nn.Parameter(v.clone()) for v in src]
    for p in ps:
        p.grad = torch.randn(p.shape, device=dev, generator=g) * 1e-3
    rms = optim.RMSprop(ps, lr=1e-4, weight_decay=5e-4)
    sides = {"ema": ema.update, "foreach_lerp": lambda: torch._foreach_lerp_(lerp_shadow, src, 1e-4), "rmsprop": rms.step, "swap": ema.swap}
    bytes_per_value = {"ema": 12, "foreach_lerp": 12, "rmsprop": 20, "swap": 16}
    for _ in range(warmup):
        for k, fn in sides.items():
            fn()
            if k == "swap":
                fn()
    torch.cuda.synchronize()
    n = sum(v.numel() for v in src)
    meds = {k: [] for k in sides}
    lo, hi = {k: math.inf for k in sides}, {k: 0.0 for k in sides}
    for _ in range(rounds):
        ts = {k: [] for k in sides}
        for _ in range(iters):
            for k, fn in sides.items():
                ts[k].append(_timed(fn))
                if k == "swap":
                    ts[k].append(_timed(fn))         # ... and back: the next update sees the model the right way round
        for k, v in ts.items():
            meds[k].append(statistics.median(v)); lo[k] = min(lo[k], min(v)); hi[k] = max(hi[k], max(v))
    assert not ema.swapped
    ms = {k: statistics.median(v) for k, v in meds.items()}
    frac = {k: n * bytes_per_value[k] / ms[k] / 1e9 / (HBM_PEAK / 1e12) for k in sides}
    frac_rounds = {k: [n * bytes_per_value[k] / m / 1e9 / (HBM_PEAK / 1e12) for m in meds[k]] for k in sides}
    spread = max(max(v) - min(v) for k, v in frac_rounds.items() if k in ("ema", "rmsprop"))
    out = {"ema": True, "tensors": len(src), "values_M": round(n / 1e6, 2), "rounds": rounds, "iters": iters, "updates": ema.updates()}
    for k in sides:
        out[k + "_ms"] = round(ms[k], 4)
        out[k + "_GBps"] = round(n * bytes_per_value[k] / ms[k] / 1e6, 1)
        out[k + "_frac_hbm_peak"] = round(frac[k], 3)
    out["ema_frac_minus_rmsprop_frac"] = round(frac["ema"] - frac["rmsprop"], 3)
    out["frac_round_spread"] = round(spread, 3)
    out["round_medians_ms"] = {k: [round(x, 4) for x in v] for k, v in meds.items()}
    out["spread_ms"] = {k: [round(lo[k], 4), round(hi[k], 4)] for k in sides}
    return out


def bench_train_step_ema(dev, size, clips, iters, warmup, rounds=3):
    """The replayed RMSprop training step without and with an attached ``WeightEMA``: two models, two graphs, alternating blocks of
    ``iters`` steps (wall clock per step, host-synchronised at both ends of a block); per side the median over the blocks."""
    from dcnet_amd.graph import GraphedTrainStep
    from dcnet_amd.train import make_optimizer
    from dcnet_amd.utils.synth import synth_boxes, synth_inputs
    n = clips * 8
    image, word_id, word_mask = (t.to(dev) for t in synth_inputs(n, size, seed=100))
    bbox = synth_boxes(n, size, seed=100).to(dev)
    steps, emas = {}, {}
    for key in ("plain", "ema"):
        random.seed(13)
        model = build_model(size, dev)
        opt = make_optimizer(model, 1e-4, "rmsprop")
        if key == "ema":
            emas[key] = optim.WeightEMA(model)
            opt.attach_ema(emas[key])                # before the capture
        steps[key] = GraphedTrainStep(model, opt, image, word_id, word_mask, bbox, size, warmup=max(1, warmup))
        for _ in range(warmup):
            steps[key]()
    torch.cuda.synchronize()
    blocks = {k: [] for k in steps}
    for _ in range(rounds):
        for key, step in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                step()
            torch.cuda.synchronize()
            blocks[key].append((time.perf_counter() - t0) / iters * 1e3)
    med = {k: statistics.median(v) for k, v in blocks.items()}
    return {"geometry": f"{clips} clips x T 8 at {size}x{size}", "steps_per_block": iters, "blocks": rounds, "ema_updates": emas["ema"].updates(),
            "replayed_rmsprop_ms": round(med["plain"], 3), "replayed_rmsprop_ema_ms": round(med["ema"], 3),
            "ema_minus_plain_ms": round(med["ema"] - med["plain"], 3),
            "block_spread_ms": round(max(max(v) - min(v) for v in blocks.values()), 3),
            "blocks_ms": {k: [round(x, 3) for x in v] for k, v in blocks.items()}}


def bench_accum(dev, size, k, iters, warmup, rounds=3):
    """The accumulation pass by phase (the phase word of a block of its own is set by hand: no prepare launch moves it), against
    torch._foreach_add_ and dcn_ema_update over the same tensors — HIP events around each, measured in turns."""
    import ctypes
    from dcnet_amd.lib import lib
    L = lib()
    model = build_model(size, dev)
    shapes = [tuple(p.shape) for p in model.parameters() if p.requires_grad]
    del model
    torch.cuda.empty_cache()
    g = torch.Generator(device=dev).manual_seed(0)
    draw = lambda scale: [torch.randn(s, device=dev, generator=g) * scale for s in shapes]
    grads, acc, acc_t, shadow, src = draw(1e-3), draw(1e-3), draw(1e-3), draw(0.05), draw(0.05)
    n_t = len(shapes)
    ptrs = lambda ts: (ctypes.c_void_p * n_t)(*[t.data_ptr() for t in ts])
    numel = (ctypes.c_int64 * n_t)(*[t.numel() for t in grads])
    p_acc, p_g, p_sh, p_src = ptrs(acc), ptrs(grads), ptrs(shadow), ptrs(src)
    inv_k = torch.tensor([1.0 / k], dtype=torch.float32).view(torch.int32).item()
    blocks = {ph: torch.tensor([0, code, inv_k, 0], dtype=torch.int32, device=dev) for ph, code in (("first", 0), ("middle", 1), ("boundary", 2))}
    w = torch.full((1,), 1e-4, dtype=torch.float32, device=dev)
    stream = lambda: torch.cuda.current_stream().cuda_stream
    sides = {"accum_" + ph: (lambda b=b: L.grad_accumulate(p_acc, p_g, numel, n_t, b.data_ptr(), stream())) for ph, b in blocks.items()}
    sides["foreach_add"] = lambda: torch._foreach_add_(acc_t, grads)
    sides["ema"] = lambda: L.ema_update(p_sh, p_src, numel, n_t, w.data_ptr(), 0, stream())
    bytes_per_value = {"accum_first": 8, "accum_middle": 12, "accum_boundary": 12, "foreach_add": 12, "ema": 12}
    for _ in range(warmup):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    n = sum(t.numel() for t in grads)
    meds = {s_: [] for s_ in sides}
    lo, hi = {s_: math.inf for s_ in sides}, {s_: 0.0 for s_ in sides}
    for _ in range(rounds):
        ts = {s_: [] for s_ in sides}
        for _ in range(iters):
            for s_, fn in sides.items():
                ts[s_].append(_timed(fn))
        for s_, v in ts.items():
            meds[s_].append(statistics.median(v)); lo[s_] = min(lo[s_], min(v)); hi[s_] = max(hi[s_], max(v))
    ms = {s_: statistics.median(v) for s_, v in meds.items()}
    out = {"accum": k, "tensors": n_t, "values_M": round(n / 1e6, 2), "rounds": rounds, "iters": iters}
    for s_ in sides:
        out[s_ + "_ms"] = round(ms[s_], 4)
        out[s_ + "_TBps"] = round(n * bytes_per_value[s_] / ms[s_] / 1e9, 3)
    out["ema_round_spread_ms"] = round(max(meds["ema"]) - min(meds["ema"]), 4)
    out["middle_minus_ema_ms"] = round(ms["accum_middle"] - ms["ema"], 4)
    out["boundary_minus_ema_ms"] = round(ms["accum_boundary"] - ms["ema"], 4)
    out["round_medians_ms"] = {s_: [round(x, 4) for x in v] for s_, v in meds.items()}
    out["spread_ms"] = {s_: [round(lo[s_], 4), round(hi[s_], 4)] for s_ in sides}
    return out


def bench_train_step_accum(dev, size, clips, iters, warmup, k, rounds=3):
    """The replayed RMSprop training step with ``accum_steps=1`` and with ``accum_steps=k``: two models, two graphs, alternating blocks
    of ``iters`` micro-steps (``iters`` rounded up to whole windows; wall clock per micro-step, host-synchronised at both ends of a
    block); per side the median over the blocks."""
    from dcnet_amd.graph import GraphedTrainStep
    from dcnet_amd.train import make_optimizer
    from dcnet_amd.utils.synth import synth_boxes, synth_inputs
    n = clips * 8
    iters = -(-iters // k) * k
    image, word_id, word_mask = (t.to(dev) for t in synth_inputs(n, size, seed=100))
    bbox = synth_boxes(n, size, seed=100).to(dev)
    steps = {}
    for key, kk in (("accum1", 1), (f"accum{k}", k)):
        random.seed(13)
        model = build_model(size, dev)
        steps[key] = GraphedTrainStep(model, make_optimizer(model, 1e-4, "rmsprop", accum_steps=kk), image, word_id, word_mask, bbox, size,
                                      warmup=max(1, warmup))
        for _ in range(warmup):
            steps[key]()
    torch.cuda.synchronize()
    blocks = {k_: [] for k_ in steps}
    for _ in range(rounds):
        for key, step in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                step()
            torch.cuda.synchronize()
            blocks[key].append((time.perf_counter() - t0) / iters * 1e3)
    med = {k_: statistics.median(v) for k_, v in blocks.items()}
    return {"geometry": f"{clips} clips x T 8 at {size}x{size}", "micro_steps_per_block": iters, "blocks": rounds, "accum": k,
            "replayed_rmsprop_ms": round(med["accum1"], 3), f"replayed_rmsprop_accum{k}_ms_per_micro_step": round(med[f"accum{k}"], 3),
            "accum_minus_plain_ms": round(med[f"accum{k}"] - med["accum1"], 3),
            "block_spread_ms": {k_: round(max(v) - min(v), 3) for k_, v in blocks.items()},
            "window_position": steps[f"accum{k}"].window_position, "loss": float(steps["accum1"].loss),
            "blocks_ms": {k_: [round(x, 3) for x in v] for k_, v in blocks.items()}}


def bench_train_step(dev, size, clips, iters, warmup):
    from dcnet_amd.graph import GraphedTrainStep
    from dcnet_amd.train import make_optimizer, train_step
    from dcnet_amd.utils.synth import synth_boxes, synth_inputs
    n = clips * 8
    image, word_id, word_mask = (t.to(dev) for t in synth_inputs(n, size, seed=100))
    bbox = synth_boxes(n, size, seed=100).to(dev)
    out = {"geometry": f"{clips} clips x T 8 at {size}x{size}", "steps": iters}
    random.seed(13)
    model = build_model(size, dev)
    opt = make_optimizer(model, 1e-4, "adam", fused=False)
    for _ in range(warmup):
        train_step(model, opt, image, word_id, word_mask, bbox, size)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        train_step(model, opt, image, word_id, word_mask, bbox, size)
    torch.cuda.synchronize()
    out["eager_torch_adam_ms"] = round((time.perf_counter() - t0) / iters * 1e3, 2)
    del model, opt
    torch.cuda.empty_cache()
    random.seed(13)
    model = build_model(size, dev)
    step = GraphedTrainStep(model, make_optimizer(model, 1e-4, "adam"), image, word_id, word_mask, bbox, size, warmup=max(1, warmup))
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        step()
    torch.cuda.synchronize()
    out["replayed_fused_adam_ms"] = round((time.perf_counter() - t0) / iters * 1e3, 2)
    out["loss"] = float(step.loss)
    return out


def arg_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--step", action="store_true", help="also time the whole step: eager torch Adam against the replayed fused Adam")
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--step-iters", type=int, default=10)
    ap.add_argument("--clip", action="store_true", help="time gradient clipping: fused / fused + clip / torch foreach / torch clip + foreach")
    ap.add_argument("--ema", action="store_true", help="time the weight EMA: update / torch._foreach_lerp_ / rmsprop_kernel / swap on the model's tensors")
    ap.add_argument("--rounds", type=int, default=3, help="--ema, --accum: rounds of --iters (the spread of their medians is reported)")
    ap.add_argument("--accum", type=int, default=0, metavar="K",
                    help="time the gradient-accumulation pass (first / middle / boundary) against torch._foreach_add_ and dcn_ema_update; with --step "
                         "the replayed step with accum_steps=1 and accum_steps=K")
    ap.add_argument("--json", default="")
    return ap


def main(argv=None):
    ap = arg_parser()
    a = ap.parse_args(argv)
    if (a.ema + a.clip + (a.accum != 0)) > 1:
        ap.error("--ema, --clip and --accum are separate measurements")
    if a.accum < 0 or a.accum == 1:
        ap.error("--accum K: K >= 2")
    dev = torch.device("cuda:0")
    if a.accum:
        rows = [bench_accum(dev, a.size, a.accum, a.iters, a.warmup, a.rounds)]
        print(json.dumps(rows[-1]), flush=True)
        torch.cuda.empty_cache()
        if a.step:
            rows.append(bench_train_step_accum(dev, a.size, a.clips, a.step_iters, a.warmup, a.accum, a.rounds))
            print(json.dumps(rows[-1]), flush=True)
        if a.json:
            with open(a.json, "w") as fh:
                json.dump(rows, fh, indent=1)
        return
    if a.ema:
        rows = [bench_ema(dev, a.size, a.iters, a.warmup, a.rounds)]
        print(json.dumps(rows[-1]), flush=True)
        torch.cuda.empty_cache()
        if a.step:
            rows.append(bench_train_step_ema(dev, a.size, a.clips, a.step_iters, a.warmup, a.rounds))
            print(json.dumps(rows[-1]), flush=True)
        if a.json:
            with open(a.json, "w") as fh:
                json.dump(rows, fh, indent=1)
        return
    model = build_model(a.size, dev)
    shapes = [tuple(p.shape) for p in model.parameters() if p.requires_grad]
    del model
    torch.cuda.empty_cache()
    rows = []
    for name in (("rmsprop", "adam", "sgd") if a.clip else ("adam", "sgd")):
        rows.append(bench_clip(name, shapes, dev, a.iters, a.warmup) if a.clip else bench_steps(name, shapes, dev, a.iters, a.warmup))
        print(json.dumps(rows[-1]), flush=True)
        torch.cuda.empty_cache()
    if a.step and a.clip:
        rows.append(bench_train_step_clip(dev, a.size, a.clips, a.step_iters, a.warmup))
        print(json.dumps(rows[-1]), flush=True)
    elif a.step:
        rows.append(bench_train_step(dev, a.size, a.clips, a.step_iters, a.warmup))
        print(json.dumps(rows[-1]), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
