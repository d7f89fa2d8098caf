#!/usr/bin/env python
"""Which C entry points does a step call, in which order, with which arguments?

Wraps every entry of dcnet_amd.lib.SIGNATURES after the library has loaded and writes one line per call: the entry point and its
arguments, pointers reduced to null / ptr and the trailing stream handle to its order of first appearance (s0, s1, ...).  Two trees
that launch the same kernels in the same order on the same streams write identical files — the check for a change that moves Python
around and must not move a launch (`diff -r` of two output directories).  What the files do not show: wait_stream / wait_event edges.

One run = one eager training step (forward, losses.total_loss, backward) and one torch.no_grad() eval forward of a freshly seeded
model.  Runs: the default switches and one run per ``--switches`` item (NAME=VALUE, a module attribute of dcnet_amd.ops;
WGRAD_DIRECT=True is set around the step as graph.GraphedTrainStep sets it).  The sampler's worker thread calls the library too, so
calls are kept per calling thread and written thread after thread.

    python tools/abi_trace.py --precision bf16s --out traces/            # -> traces/bf16s_default.txt, traces/bf16s_BN_TAP=False.txt, ...

Needs only dcnet_amd.lib and the model: the same file runs in another checkout of this repository.
"""
from __future__ import annotations

import argparse
import ast
import ctypes
import os
import random
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEFAULT_SWITCHES = "WGRAD_AFTER_DGRAD=False;WGRAD_HELD=False;BN_TAP=False;PRE_ACT=False;WGRAD_DIRECT=True"
# entry points whose last pointer is not a stream
NO_STREAM = {"dcn_stream_destroy", "dcn_stream_priority_range", "dcn_prof_collect", "dcn_prof_records", "dcn_tuning_info",
             "dcn_mt_sample_interframe", "dcn_mt_sample_crossmodal", "dcn_mt_sample_crossmodal_csr", "dcn_mt_sample_step"}


def _address(a) -> int:
    if a is None:
        return 0
    if isinstance(a, int):
        return a
    if isinstance(a, (bytes, str)):
        return 1
    v = getattr(a, "value", a)          # c_void_p(...).value; byref() objects have none and are never null
    return 1 if v is a else (v or 0)


def call_line(name: str, argtypes, args, streams: dict) -> str:
    """One call as text.  A function of (argtypes, args) alone, but for ``streams`` (handle -> ordinal), which it extends when the
    call's trailing stream handle has not been seen before."""
    stream_at = len(argtypes) - 1 if (argtypes and argtypes[-1] is ctypes.c_void_p and name not in NO_STREAM) else -1
    out = []
    for i, (t, a) in enumerate(zip(argtypes, args)):
        if t is ctypes.c_void_p:
            if i == stream_at:
                out.append("s%d" % streams.setdefault(_address(a), len(streams)))
            else:
                out.append("ptr" if _address(a) else "null")
        elif t is ctypes.c_float:
            out.append(repr(float(a)))
        elif t is ctypes.c_char_p:
            out.append(repr(a))
        else:
            out.append(repr(int(getattr(a, "value", a))))
    return "%s(%s)" % (name, ", ".join(out))


class Tracer:
    """Wraps the attributes of the loaded library object; ``lines()`` is the text of everything called since ``reset()``."""

    def __init__(self):
        from dcnet_amd.lib import SIGNATURES, lib
        self._lock = threading.Lock()
        self.reset()
        L = lib()
        for name, (_, argtypes) in SIGNATURES.items():
            setattr(L, name[4:], self._wrap(name, list(argtypes), getattr(L, name[4:])))

    def reset(self):
        with self._lock:
            self.threads = {}          # thread id -> (lines, streams), in order of first call

    def _wrap(self, name, argtypes, fn):
        def call(*a):
            with self._lock:
                lines, streams = self.threads.setdefault(threading.get_ident(), ([], {}))
                lines.append(call_line(name, argtypes, a, streams))
            return fn(*a)
        return call

    def lines(self):
        with self._lock:
            out = []
            for k, (lines, _) in enumerate(self.threads.values()):
                out.append("# thread %d: %d calls" % (k, len(lines)))
                out += lines
            return out


def one_run(tracer, precision: str, size: int, frames: int, switch, out_path: str):
    import torch
    from dcnet_amd import losses, ops
    from dcnet_amd.model import grounding_model
    from dcnet_amd.parallel import freeze_gradless
    from dcnet_amd.utils.synth import synth_boxes, synth_inputs
    dev = torch.device("cuda:0")
    ops.set_precision(precision)
    torch.manual_seed(1234)            # as bench.py seeds
    model = grounding_model(corpus=list(range(1000)), light=False, emb_size=512, coordmap=True, bert_model="bert-base-uncased",
                            dataset="vid", img_size=size, config_path=os.path.join(ROOT, "model", "yolov3.cfg"), weights_path=None).to(dev)
    model.train()
    model.sampler_seed = 0x5DC0E7A1
    freeze_gradless(model)
    image, word_id, word_mask = (t.to(dev) for t in synth_inputs(frames, size, seed=100))
    bbox = synth_boxes(frames, size, seed=100).to(dev)
    random.seed(13)
    name, value = switch if switch else (None, None)
    direct = name == "WGRAD_DIRECT"
    before = getattr(ops, name) if name else None
    torch.cuda.synchronize()
    tracer.reset()
    try:
        if name:
            setattr(ops, name, value)
        if direct:
            ops.reset_held_wgrads()
        out = model(image, word_id, word_mask)
        loss, _ = losses.total_loss(out, bbox, size)
        loss.backward()
        if direct:
            ops.finish_wgrads(dev)
        torch.cuda.synchronize()
        model.eval()
        with torch.no_grad():
            model(image, word_id, word_mask)
        torch.cuda.synchronize()
    finally:
        if name:
            setattr(ops, name, before)
    lines = tracer.lines()
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("%s: %d lines, loss %r" % (out_path, len(lines), float(loss)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--frames", type=int, default=2, help="images of the step (one clip)")
    ap.add_argument("--switches", default=DEFAULT_SWITCHES, help="';'-separated ops.NAME=VALUE runs behind the default one")
    ap.add_argument("--out", required=True, help="directory of the trace files")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    import torch  # noqa: F401  (before the library loads: both must end up on the HIP runtime torch brings, as in every other entry point)
    tracer = Tracer()
    runs = [None] + [(kv.split("=")[0], ast.literal_eval(kv.split("=", 1)[1])) for kv in args.switches.split(";") if kv]
    for sw in runs:
        tag = "default" if sw is None else "%s=%s" % sw
        one_run(tracer, args.precision, args.size, args.frames, sw, os.path.join(args.out, "%s_%s.txt" % (args.precision, tag)))


if __name__ == "__main__":
    main()
