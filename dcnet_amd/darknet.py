"""Darknet-53 / YOLOv3 visual backbone on the HIP conv engine.

Mirrors the reference's model/darknet.py surface — ``parse_model_config``, ``create_modules``,
``Darknet(config_path, img_size, obj_out)`` with ``.module_list`` (same sub-module names, hence the
same 438 state_dict keys), ``.forward(x)`` returning the three taps, ``.load_weights`` /
``.save_weights`` (darknet binary) — but executes a static layer plan with hand-written kernels:

  * the graph is compiled once into a plan (dead YOLO heads removed: F7 of SURVEY.md; every
    shortcut fused into the producing conv; upsample fused with the route concat);
  * the whole backbone is ONE autograd node (``_DarknetFn``) whose backward is scheduled by hand:
    BN+LeakyReLU backward, weight gradient, data gradient per layer, gradients of tensors with two
    consumers accumulated inside the data-gradient kernel (no autograd add nodes);
  * eval mode folds BatchNorm into the conv epilogue: one kernel per layer.

Reference: model/darknet.py:99-116 (cfg parser), :162-237 (module factory), :391-431 (forward),
:433-513 (weights io); graph: model/yolov3.cfg.
"""
from __future__ import annotations

import os
from typing import Dict, List, NamedTuple, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn

from . import convblock, ops

# ----------------------------------------------------------------------------------------------------
# cfg handling
# ----------------------------------------------------------------------------------------------------

def parse_model_config(path: str) -> List[dict]:
    """darknet .cfg -> list of block dicts (first block is [net]).  Same contract as the
    reference parser (model/darknet.py:99-116): '#' lines dropped, values kept as strings,
    ``batch_normalize`` defaults to 0 for (yolo)convolutional blocks."""
    blocks: List[dict] = []
    with open(path, "r") as fh:
        for raw in fh:
            line = raw.strip()
            if not line or line.startswith("#"):
                continue
            if line.startswith("["):
                blocks.append({"type": line[1:-1].rstrip()})
                if blocks[-1]["type"] in ("convolutional", "yoloconvolutional"):
                    blocks[-1]["batch_normalize"] = 0
            else:
                key, value = line.split("=", 1)
                blocks[-1][key.strip()] = value.strip()
    return blocks


_ANCHORS = "10,13,  16,30,  33,23,  30,61,  62,45,  59,119,  116,90,  156,198,  373,326"


def yolov3_blocks(width: int = 416, height: int = 416) -> List[dict]:
    """The YOLOv3 graph DCNet uses, built from the network's regular structure (52-conv
    Darknet-53 trunk, then three neck/head groups with ``yoloconvolutional`` taps).  Produces
    the same block list as parsing the reference's model/yolov3.cfg."""
    blocks: List[dict] = [dict(type="net", batch="1", subdivisions="1", width=str(width), height=str(height),
                               channels="3", momentum="0.9", decay="0.0005")]

    def conv(filters, size, stride=1, bn=1, act="leaky", kind="convolutional"):
        b = {"type": kind, "batch_normalize": bn} if bn else {"type": kind, "batch_normalize": 0}
        if bn:
            b["batch_normalize"] = "1"
        b.update(filters=str(filters), size=str(size), stride=str(stride), pad="1", activation=act)
        blocks.append(b)

    def shortcut():
        blocks.append({"type": "shortcut", "from": "-3", "activation": "linear"})

    conv(32, 3)
    for filters, reps in ((64, 1), (128, 2), (256, 8), (512, 8), (1024, 4)):
        conv(filters, 3, 2)
        for _ in range(reps):
            conv(filters // 2, 1); conv(filters, 3); shortcut()
    for mask, (filters, lateral) in zip(("6,7,8", "3,4,5", "0,1,2"), ((512, None), (256, 61), (128, 36))):
        if lateral is not None:
            blocks.append({"type": "route", "layers": "-4"})
            conv(filters, 1)
            blocks.append({"type": "upsample", "stride": "2"})
            blocks.append({"type": "route", "layers": f"-1, {lateral}"})
        for _ in range(2):
            conv(filters, 1); conv(filters * 2, 3)
        conv(filters, 1, kind="yoloconvolutional")
        conv(filters * 2, 3)
        conv(255, 1, bn=0, act="linear")
        blocks.append({"type": "yolo", "mask": mask, "anchors": _ANCHORS, "classes": "80", "num": "9",
                       "jitter": ".3", "ignore_thresh": ".7", "truth_thresh": "1", "random": "1"})
    return blocks


def write_cfg(path: str, blocks: Optional[Sequence[dict]] = None) -> None:
    blocks = yolov3_blocks() if blocks is None else blocks
    with open(path, "w") as fh:
        for b in blocks:
            fh.write(f"[{b['type']}]\n")
            for k, v in b.items():
                if k != "type" and not (k == "batch_normalize" and str(v) == "0"):
                    fh.write(f"{k}={v}\n")
            fh.write("\n")


class EmptyLayer(nn.Module):
    """Placeholder for route / shortcut slots (model/darknet.py:239-243)."""


class MyUpsample2(nn.Module):
    """Nearest x2 (model/darknet.py:158-160); only a slot marker here — the plan fuses it."""
    def forward(self, x):
        return x[:, :, :, None, :, None].expand(-1, -1, -1, 2, -1, 2).reshape(x.size(0), x.size(1), x.size(2) * 2, x.size(3) * 2)


class YOLOLayer(nn.Module):
    """Detection layer slot (model/darknet.py:245-375).  DCNet discards its output
    (obj_out=False), so it is never executed; it has no parameters."""
    def __init__(self, anchors, num_classes, img_dim):
        super().__init__()
        self.anchors, self.num_classes, self.image_dim = anchors, num_classes, img_dim


def create_modules(module_defs: List[dict]):
    """Parameter containers with the reference's names (model/darknet.py:162-237):
    ``conv_%d`` (bias only when there is no BN), ``batch_norm_%d``, ``leaky_%d``."""
    hyper = module_defs.pop(0)
    filters_out = [int(hyper["channels"])]
    module_list = nn.ModuleList()
    for i, d in enumerate(module_defs):
        seq = nn.Sequential()
        t = d["type"]
        if t in ("convolutional", "yoloconvolutional"):
            bn = int(d["batch_normalize"]); filters = int(d["filters"]); k = int(d["size"])
            pad = (k - 1) // 2 if int(d["pad"]) else 0
            seq.add_module(f"conv_{i}", nn.Conv2d(filters_out[-1], filters, k, int(d["stride"]), pad, bias=not bn))
            if bn:
                seq.add_module(f"batch_norm_{i}", nn.BatchNorm2d(filters))
            if d["activation"] == "leaky":
                seq.add_module(f"leaky_{i}", nn.LeakyReLU(0.1))
        elif t == "upsample":
            assert int(d["stride"]) == 2
            seq.add_module(f"upsample_{i}", MyUpsample2())
            filters = filters_out[-1]
        elif t == "route":
            layers = [int(x) for x in d["layers"].split(",")]
            filters = sum(filters_out[1:][l] if l >= 0 else filters_out[l] for l in layers)
            seq.add_module(f"route_{i}", EmptyLayer())
        elif t == "shortcut":
            filters = filters_out[int(d["from"])]
            seq.add_module(f"shortcut_{i}", EmptyLayer())
        elif t == "yolo":
            idx = [int(x) for x in d["mask"].split(",")]
            a = [int(x) for x in d["anchors"].split(",")]
            a = [(a[j], a[j + 1]) for j in range(0, len(a), 2)]
            seq.add_module(f"yolo_{i}", YOLOLayer([a[j] for j in idx], int(d["classes"]), 256))
            filters = filters_out[-1]
        else:
            raise ValueError(f"unsupported cfg block type {t!r}")
        module_list.append(seq)
        filters_out.append(filters)
    return hyper, module_list


# ----------------------------------------------------------------------------------------------------
# plan
# ----------------------------------------------------------------------------------------------------

class _ConvOp:
    __slots__ = ("slot", "src", "dst", "res", "cin", "cout", "k", "stride", "bn", "leaky")


class _UpCatOp:
    __slots__ = ("dst", "up_src", "lat_src", "c_up", "c_lat")


class _AliasOp:
    __slots__ = ("dst", "src")


def build_plan(module_defs: List[dict], in_channels: int = 3):
    """Compile the slot list into executable ops.  Returns (ops, tap_slots, channels_per_slot)."""
    n = len(module_defs)
    ch: List[int] = []
    prev = in_channels
    for i, d in enumerate(module_defs):
        t = d["type"]
        if t in ("convolutional", "yoloconvolutional"):
            prev = int(d["filters"])
        elif t == "route":
            ls = [int(x) for x in d["layers"].split(",")]
            prev = sum(ch[l if l >= 0 else i + l] for l in ls)
        elif t == "shortcut":
            prev = ch[i + int(d["from"])]
        ch.append(prev)
    # liveness: what can reach a tap (input of each yoloconvolutional)
    taps = [i - 1 for i, d in enumerate(module_defs) if d["type"] == "yoloconvolutional"]
    live = [False] * n
    stack = list(taps)
    while stack:
        i = stack.pop()
        if i < 0 or live[i]:
            continue
        live[i] = True
        d = module_defs[i]; t = d["type"]
        if t in ("convolutional", "yoloconvolutional", "upsample"):
            stack.append(i - 1)
        elif t == "shortcut":
            stack += [i - 1, i + int(d["from"])]
        elif t == "route":
            stack += [l if l >= 0 else i + l for l in (int(x) for x in d["layers"].split(","))]
    consumers: Dict[int, List[int]] = {i: [] for i in range(-1, n)}
    for i, d in enumerate(module_defs):
        if not live[i]:
            continue
        t = d["type"]
        if t in ("convolutional", "yoloconvolutional", "upsample"):
            consumers[i - 1].append(i)
        elif t == "shortcut":
            consumers[i - 1].append(i); consumers[i + int(d["from"])].append(i)
        elif t == "route":
            for l in (int(x) for x in d["layers"].split(",")):
                consumers[l if l >= 0 else i + l].append(i)
    plan = []
    fused_shortcuts = set(); fused_upsamples = set()
    for i, d in enumerate(module_defs):
        if not live[i]:
            continue
        t = d["type"]
        if t in ("convolutional", "yoloconvolutional"):
            op = _ConvOp()
            op.slot = i; op.src = i - 1; op.dst = i; op.res = None
            op.cin = in_channels if i == 0 else ch[i - 1]; op.cout = int(d["filters"])
            op.k = int(d["size"]); op.stride = int(d["stride"])
            op.bn = bool(int(d["batch_normalize"])); op.leaky = d["activation"] == "leaky"
            nxt = module_defs[i + 1] if i + 1 < n else None
            if (nxt is not None and nxt["type"] == "shortcut" and live[i + 1] and consumers[i] == [i + 1]
                    and i not in taps):
                op.dst = i + 1; op.res = i + 1 + int(nxt["from"])
                fused_shortcuts.add(i + 1)
            plan.append(op)
        elif t == "shortcut":
            if i not in fused_shortcuts:
                raise NotImplementedError("unfused shortcut (pattern not present in YOLOv3)")
        elif t == "upsample":
            nxt = module_defs[i + 1]
            ok = nxt["type"] == "route" and consumers[i] == [i + 1]
            ls = [int(x) for x in nxt["layers"].split(",")] if ok else []
            if not (ok and len(ls) == 2 and ls[0] == -1):
                raise NotImplementedError("upsample not followed by route(-1, k)")
            fused_upsamples.add(i + 1)
            op = _UpCatOp()
            op.dst = i + 1; op.up_src = i - 1; op.lat_src = ls[1] if ls[1] >= 0 else i + 1 + ls[1]
            op.c_up = ch[i - 1]; op.c_lat = ch[op.lat_src]
            plan.append(op)
        elif t == "route":
            if i in fused_upsamples:
                continue
            ls = [int(x) for x in d["layers"].split(",")]
            if len(ls) != 1:
                raise NotImplementedError("route concat without upsample")
            op = _AliasOp(); op.dst = i; op.src = ls[0] if ls[0] >= 0 else i + ls[0]
            plan.append(op)
    return plan, taps, ch


# ----------------------------------------------------------------------------------------------------
# what the backward has to compute (requires_grad decides the work)
# ----------------------------------------------------------------------------------------------------

class ConvNeeds(NamedTuple):
    """One conv op's share of the backward.  want_w: its weight gradient; want_affine: the gradient of gamma / beta (or of the conv
    bias); want_dx: its data gradient; want_res: its output gradient is also the shortcut source's; live: the layer has a backward
    pass of its own and keeps a record for it (any trainable parameter, or a gradient that goes through it to a trainable one)."""
    want_w: bool
    want_affine: bool
    want_dx: bool
    want_res: bool
    live: bool


class BackwardNeeds(NamedTuple):
    """conv: {slot: ConvNeeds}; tensor: {tensor slot: is its gradient computed}; live: the slots that keep a record."""
    conv: Dict[int, ConvNeeds]
    tensor: Dict[int, bool]
    live: frozenset


def all_trainable(plan) -> frozenset:
    """Every (slot, key) of the plan's convolutions: key "w", and "gamma" / "beta" (BatchNorm) or "b" (biased convolution)."""
    return frozenset((op.slot, k_) for op in plan if isinstance(op, _ConvOp) for k_ in (("w", "gamma", "beta") if op.bn else ("w", "b")))


def backward_needs(plan, trainable) -> BackwardNeeds:
    """Pure function of the plan and the set of trainable (slot, key) pairs (all_trainable: the keys).  The gradient of a tensor is
    computed only if its producer, or a producer upstream of it, has a trainable parameter; the image (tensor -1) never has one.  With
    everything trainable that is the schedule there always was: every layer live, every gradient wanted, no data gradient for the stem."""
    trainable = frozenset(trainable)
    tensor: Dict[int, bool] = {-1: False}
    conv: Dict[int, ConvNeeds] = {}
    for op in plan:          # (plan order is topological: inputs come first)
        if isinstance(op, _ConvOp):
            want_w = (op.slot, "w") in trainable
            want_affine = any((op.slot, k_) in trainable for k_ in ("gamma", "beta", "b"))
            want_dx = tensor[op.src]
            want_res = op.res is not None and tensor[op.res]
            live = want_w or want_affine or want_dx
            conv[op.slot] = ConvNeeds(want_w, want_affine, want_dx, want_res, live)
            tensor[op.dst] = live or want_res
        elif isinstance(op, _UpCatOp):
            tensor[op.dst] = tensor[op.up_src] or tensor[op.lat_src]
        else:
            tensor[op.dst] = tensor[op.src]
    return BackwardNeeds(conv, tensor, frozenset(s_ for s_, c_ in conv.items() if c_.live))


# ----------------------------------------------------------------------------------------------------
# execution
# ----------------------------------------------------------------------------------------------------

def _inputs(op):
    return (op.src, op.res) if isinstance(op, _ConvOp) else (op.up_src, op.lat_src) if isinstance(op, _UpCatOp) else (op.src,)


def _cpad(c: int) -> int:
    return 4 if c <= 4 else ops.pad32(c)


def _b16_diag_layer(diag, op, p, x, res, w, bank, act, out, amx):
    """Experiments (ops.B16_DIAG, tools/precision_criterion.py --backbone): which part of the bf16-storage backbone costs the box
    criterion, in eval mode.  "layers": predicate on the conv slot — True = this layer on bf16 tensors, False = on fp32 tensors at fp32
    accuracy; "res32": the shortcut sums are kept in fp32 (the convolutions read a bf16 copy).
    Returns (x, res, done): done = the layer's output is in ``out``; else the bf16 operands the ordinary path goes on with."""
    fold = (p["gamma"], p["beta"], p["rm"], p["rv"], 1e-5)
    if not diag.get("layers", lambda s_: True)(op.slot):
        ops.set_precision(diag.get("arith", "fp32"))      # ("bf16": fp32 TENSORS, operands rounded to bf16 in the loaders)
        try:
            ss = ops.bn_fold(*fold) if op.bn else (None, p["b"])
            # (no abs-max words: the launch takes the bf16 three-piece split — fp32 accuracy all the same)
            o, _ = ops.conv2d_fwd(ops.to_f32(x), w, op.k, op.stride, ss[0], ss[1], act, 0.1,
                                  residual=None if res is None else ops.to_f32(diag.get("_r32", {}).get(op.res, res)))
        finally:
            ops.set_precision("bf16s")
        if res is not None and diag.get("res32"):
            diag.setdefault("_r32", {})[op.dst] = o
        out[op.dst] = o; amx[op.dst] = None
        return x, res, True
    x = ops.to_b16(x)
    if res is not None and diag.get("res32"):
        o32, _ = convblock.conv_forward(x, op.k, op.stride, op.cout, bank=bank, fold=fold, act=act, slope=0.1, out_f32=True)
        r32 = diag.setdefault("_r32", {})
        o32 = o32 + (r32[op.res] if op.res in r32 else ops.to_f32(res))
        r32[op.dst] = o32
        out[op.dst] = ops.to_b16(o32); amx[op.dst] = None
        return x, res, True
    return x, (None if res is None else ops.to_b16(res)), False


def _run_forward(plan, taps, x_nhwc, P, training: bool, save: Optional[dict], banks=None, taps_b16: bool = False, live=None,
                 backward: Optional[bool] = None):
    """P[slot] = dict(w=OIHW weight, b=conv bias|None, gamma, beta, rm, rv).  Returns tap tensors.
    banks (ops.FilterBanks, refreshed by the caller): the filter banks of all slots in their GEMM forms.
    Two things that used to be one: ``backward`` — the forward takes the kernels of a pass that a backward may follow (PreAct
    hand-over, the activation kept apart from the shortcut add; default: ``save is not None``) — and ``live`` — the slots that keep a
    record in ``save`` (backward_needs; default: all).  A layer outside ``live`` runs the same kernels and keeps nothing; a tensor is
    dropped behind its last reader, so what no record holds is gone by then."""
    if backward is None:
        backward = save is not None
    out: Dict[int, torch.Tensor] = {-1: x_nhwc}
    # abs-max word of every activation (ops.amax_*): written by the kernel that produces the tensor, read by the GEMMs
    # that consume it (forward here, weight gradient in the backward) to pick their power-of-two operand scales
    am = ops.use_amax()
    # bf16 storage (ops.set_precision("bf16s")): every activation / raw conv output behind the stem is a bf16 tensor; the three taps are
    # cast to fp32 for the head (and their gradients back to bf16 in _run_backward)
    s16 = ops.storage_b16()
    amx: Dict[int, Optional[torch.Tensor]] = {-1: None}
    # outputs with exactly ONE reader, a train-mode conv + BatchNorm whose kernels can apply the activation while loading
    # (ops.pre_supported): they are handed on as ops.PreAct — no scale_act pass, no activation tensor
    readers: Dict[int, list] = {}
    f8_left: Dict[int, int] = {}          # fp8 storage: e4m3 readers of a tensor still to come (its attached copy is dropped after the last)
    last_reader: Dict[int, int] = {}
    for i_op, op in enumerate(plan):
        for s_ in _inputs(op):
            if s_ is not None:
                readers.setdefault(s_, []).append(op)
                last_reader[s_] = i_op

    def sole_pre_reader(op, x):
        """the only reader of op's output, when that is a train-mode conv + BatchNorm whose kernels take the raw tensor"""
        rd = readers.get(op.dst, [])
        if not (am and ops.PRE_ACT and training and backward and len(rd) == 1 and op.dst not in taps and op.res is None):
            return False
        nx = rd[0]
        ho, wo = ops.conv_out_hw(x.shape[1], x.shape[2], op.k, op.stride)
        return (isinstance(nx, _ConvOp) and nx.bn and nx.src == op.dst and nx.res != op.dst
                and ops.pre_supported(x.shape[0], ho, wo, nx.cin, nx.cout, nx.k, nx.stride))

    # the last layer of the persistent one-workgroup-per-CU kernels (csrc/nconv.hip: the 32 <-> 64 channel 3x3 layers): an event behind
    # it lets other streams start their LDS-heavy work (the persistent BiLSTM) where it no longer takes CUs from those launches
    early = [i for i, op in enumerate(plan) if isinstance(op, _ConvOp) and op.k == 3 and op.cin == 32 and op.cout == 64]
    early_at = early[-1] if early else -1
    early_event = None
    for i_op, op in enumerate(plan):
        if i_op == early_at + 1 and early_at >= 0:
            early_event = torch.cuda.Event(); early_event.record()
        if isinstance(op, _ConvOp):
            p = P[op.slot]
            x = out[op.src]; ax = amx.get(op.src)
            bank = banks.get(op.slot, p["w"]) if banks is not None else None
            if bank is not None and getattr(banks, "pending", None) is not None:
                torch.cuda.current_stream().wait_stream(banks.pending)      # the refresh launched by Darknet._filter_banks
                banks.pending = None
            if bank is not None:       # prepared for the whole network in one go (no per-layer transpose / abs-max / pre-split)
                w, aw, wsp, w16 = bank["ohwi"], (bank["amax"] if am else None), bank["split"], bank["b16"]
            else:
                w = ops.weight_to_ohwi(p["w"]); wsp = w16 = None
                aw = ops.absmax(p["w"]) if (am and op.cin > 4) else None
            ao = ops.amax_slot(x.device) if am else None
            res = out[op.res] if op.res is not None else None
            act = ops.ACT_LEAKY if op.leaky else ops.ACT_NONE
            if s16 and ops.B16_DIAG is not None and not training and op.cin > 4:
                x, res, done = _b16_diag_layer(ops.B16_DIAG, op, p, x, res, w, bank, act, out, amx)
                if done:
                    continue
            # "fp8s": a layer that reads its input as e4m3 operands tells conv_forward when it is the last such reader of that tensor
            last8 = (s16 and x.dtype == torch.bfloat16 and ops.f8_takes(op.cin, op.cout, op.k)
                     and convblock.last_q8_reader(f8_left, op.src, sum(1 for r_ in readers.get(op.src, []) if isinstance(r_, _ConvOp)
                                                                      and ops.f8_takes(r_.cin, r_.cout, r_.k))))

            def conv(**kw):
                return convblock.conv_forward(x, op.k, op.stride, op.cout, w=w, bank=bank, amax_x=ax, amax_w=aw, w_split=wsp, w_b16=w16,
                                              drop_q8=last8, **kw)

            if op.bn and training:
                # (the conv hands out the abs-max of its raw output with its store: the bound of an unwritten activation starts from it)
                ay = ops.amax_slot(x.device) if (not isinstance(x, ops.PreAct) and sole_pre_reader(op, x)) else None
                y, stats = conv(want_stats=True, amax_out=ay)
                # "fp8s": a reader that takes e4m3 operands gets its copy from the BatchNorm pass (no quantisation pass of its own)
                q_ = ops.storage_f8() and any(isinstance(r_, _ConvOp) and r_.src == op.dst and ops.f8_takes(r_.cin, r_.cout, r_.k)
                                              for r_ in readers.get(op.dst, []))
                mi, o, ao = convblock.train_bn_forward(y, stats, p["gamma"], p["beta"], 1e-5, p["momentum"], p["rm"], p["rv"], act, 0.1,
                                                       residual=res, amax_out=ao, amax_y=ay, out_b16=s16, quant=q_)    # (s16: the stem's fp32 raw output -> bf16)
                if save is not None and (live is None or op.slot in live):
                    save[op.slot] = convblock.SavedLayer(x, y, w, bank, ax, aw, mi=mi)
            else:
                fold, shift = ((p["gamma"], p["beta"], p["rm"], p["rv"], 1e-5), None) if op.bn else (None, p["b"])
                if not backward:      # inference: one kernel per layer, shortcut fused in the epilogue
                    o, _ = conv(fold=fold, shift=shift, act=act, slope=0.1, residual=res, amax_out=ao)
                else:                 # frozen-BN fine-tuning: keep the pre-shortcut activation for act'
                    a, ss = conv(fold=fold, shift=shift, act=act, slope=0.1, amax_out=ao if res is None else None)
                    o = a if res is None else ops.scale_act(a, None, None, ops.ACT_NONE, 0.0, residual=res, amax_out=ao)
                    if save is not None and (live is None or op.slot in live):
                        save[op.slot] = convblock.SavedLayer(x, a, w, bank, ax, aw, scale=None if ss is None else ss[0])
            if s16:
                o = ops.to_b16(o)          # (the stem in inference: its fused epilogue wrote fp32)
            out[op.dst] = o; amx[op.dst] = ao
        elif isinstance(op, _UpCatOp):
            up, lat = out[op.up_src], out[op.lat_src]
            if up.dtype != lat.dtype:              # (mixed-precision experiments only)
                up = ops.to_b16(up) if lat.dtype == torch.bfloat16 else ops.to_f32(up)
            n, h, w_, _ = lat.shape
            buf = torch.empty((n, h, w_, op.c_up + op.c_lat), dtype=lat.dtype, device=lat.device)
            ops.upsample2_into(up, buf[..., :op.c_up])
            ops.copy_slice(lat, buf[..., op.c_up:])
            out[op.dst] = buf
            # the concat holds exactly the values of its two sources: its abs-max is the larger of theirs
            amx[op.dst] = ops.absmax(lat, ops.absmax(up)) if am else None
        else:
            out[op.dst] = out[op.src]; amx[op.dst] = amx.get(op.src)
        x = res = None
        for s_ in _inputs(op):       # behind its last reader a tensor belongs to the records that kept it (the taps: to the caller)
            if s_ is not None and s_ >= 0 and last_reader[s_] == i_op and s_ not in taps:
                out.pop(s_, None)
    # (taps_b16: the caller's first kernels read bf16 — grounding_model's mapping convolutions — so the taps stay as they are)
    return [ops.to_f32(out[t]) if (s16 and not taps_b16) else out[t] for t in taps], [amx.get(t) for t in taps], early_event


def _run_backward(plan, taps, grads_taps, P, save, training: bool, sink=None, bucket_bytes: int = 0, trainable=None):
    """Hand-scheduled reverse sweep.  Returns {slot: dict(w=, b=, gamma=, beta=)} parameter grads.
    sink (optional): called with [(slot, key, tensor), ...] every time ``bucket_bytes`` of parameter gradients are final —
    the data-parallel reducer starts their all-reduce while the sweep continues (parallel.OverlappedGradReducer).
    trainable: the (slot, key) pairs that want a gradient (default: all).  backward_needs turns it into the launches that are made:
    nothing is computed for a frozen parameter, no gradient is formed (added, copied, upsampled, quantised) for a tensor that has no
    trainable parameter upstream, and the sink sees the trainable gradients only."""
    trainable = all_trainable(plan) if trainable is None else frozenset(trainable)
    needs = backward_needs(plan, trainable)
    pending: list = []
    pending_bytes = 0
    g: Dict[int, Optional[torch.Tensor]] = {}
    s16 = ops.storage_b16()

    def add(slot, t):
        cur = g.get(slot)
        if cur is None:
            if not t.is_contiguous():
                buf = torch.empty(t.shape, dtype=t.dtype, device=t.device)
                ops.copy_slice(t, buf)
                t = buf
            g[slot] = t
        else:
            ops.copy_slice(t, cur, accumulate=True)

    for t, gt in zip(taps, grads_taps):
        if gt is not None and needs.tensor[t]:
            g0 = gt.clone(memory_format=torch.contiguous_format)      # never accumulate into autograd's tensor
            add(t, ops.to_b16(g0) if s16 else g0)
    pg: Dict[int, dict] = {}
    # BatchNorm taps: the data gradient that completes the gradient of a conv + BN + activation output (= the FIRST consumer of that
    # output in plan order, processed last) can form the partial sums that layer's BatchNorm backward starts with (ops.conv2d_bwd_data)
    producer = {op.dst: op for op in plan if isinstance(op, _ConvOp)}
    first_use: Dict[int, int] = {}
    for i, op in enumerate(plan):
        for s_ in _inputs(op):
            if s_ is not None:
                first_use.setdefault(s_, i)
    index_of = {id(op): i for i, op in enumerate(plan)}
    tapped: Dict[int, torch.Tensor] = {}
    held = None          # (gradient dict, slot, ops.HeldWgrad): the weight gradient of the layer before, launched behind this layer's passes

    def release():
        nonlocal held, pending_bytes
        ops.release_held_wgrads()        # (ops.WGRAD_DIRECT: the head's last block)
        if held is not None:
            d_, slot_, hw_ = held
            held = None
            d_["w"] = hw_.issue()
            if sink is not None:
                pending.append((slot_, "w", d_["w"])); pending_bytes += d_["w"].numel() * 4

    def keep(d_):
        """a kernel that forms gamma's and beta's sums forms both: the frozen one of the two is dropped here"""
        for k_ in d_:
            if (op.slot, k_) not in trainable:
                d_[k_] = None
        return d_

    def finished(slot, d):
        """the gradients of a layer are final (a held weight gradient follows through release): to the reducer's sink, bucket by bucket"""
        nonlocal pending, pending_bytes
        pg[slot] = d
        if sink is not None:
            for k_, t_ in d.items():
                if t_ is not None and (slot, k_) in trainable:
                    pending.append((slot, k_, t_)); pending_bytes += t_.numel() * 4
            if pending_bytes >= bucket_bytes:
                sink(pending); pending = []; pending_bytes = 0

    for op in reversed(plan):
        dout = g.pop(op.dst, None)
        if dout is None:
            continue
        if isinstance(op, _AliasOp):
            if needs.tensor[op.src]:
                add(op.src, dout)
        elif isinstance(op, _UpCatOp):
            n, h2, w2, _ = dout.shape
            cur = g.get(op.up_src)
            if not needs.tensor[op.up_src]:
                pass
            elif cur is None:
                cur = torch.empty((n, h2 // 2, w2 // 2, op.c_up), dtype=dout.dtype, device=dout.device)
                ops.upsample2_bwd(dout[..., :op.c_up], cur, False)
                g[op.up_src] = cur
            else:
                ops.upsample2_bwd(dout[..., :op.c_up], cur, True)
            if needs.tensor[op.lat_src]:
                add(op.lat_src, dout[..., op.c_up:])
        else:
            nd = needs.conv[op.slot]
            if not nd.live:            # (nothing trainable in or below this layer: its output gradient is the shortcut source's, no more)
                if nd.want_res:
                    add(op.res, dout)
                continue
            p = P[op.slot]
            rec = save.pop(op.slot)
            x, y = rec.x, rec.y
            act = ops.ACT_LEAKY if op.leaky else ops.ACT_NONE
            # the stem: nothing but its weight gradient reads dy, so dy is formed inside that kernel and never written
            # (a frozen stem weight: the generic BatchNorm backward forms gamma's and beta's gradients, no weight-gradient kernel runs)
            stem_fused = (op.bn and training and not nd.want_dx and nd.want_w and ops.STEM_FUSED_BWD and torch.is_tensor(x) and x.shape[3] == 4 and op.cout == 32
                          and op.k == 3 and op.stride == 1 and op.res is None and torch.is_tensor(y) and y.is_contiguous() and x.shape[2] >= 32)
            if s16 and torch.is_tensor(x) and x.dtype == torch.float32 and dout.dtype == torch.bfloat16 and not stem_fused:
                dout = ops.to_f32(dout)           # bf16 storage: the 3-channel stem's generic kernels stay fp32 (its fused backward reads bf16 itself)
            shape = tuple(p["w"].shape)
            d = {}
            ady = ops.amax_slot(dout.device) if ops.use_amax() else None
            if stem_fused:
                dw, d["gamma"], d["beta"] = ops.stem_bwd_weight_bn(x, y, dout, rec.mi[0], rec.mi[1], p["gamma"], p["beta"], act, 0.1,
                                                                   part=tapped.pop(op.slot, None))
                d["w"] = ops.weight_grad_to_oihw(dw, shape)
                finished(op.slot, keep(d))
                continue
            if op.bn and training:
                dy, d["gamma"], d["beta"] = ops.bn_act_bwd(y, dout, rec.mi[0], rec.mi[1], p["gamma"], p["beta"], act, 0.1, amax_out=ady,
                                                           part=tapped.pop(op.slot, None),
                                                           quant=nd.want_dx and ops.f8_takes(op.cout, op.cin, op.k))      # ("fp8s": dy's e4m3 copy for the data gradient)
            else:
                # frozen statistics: y holds act(scale*conv+shift) before the shortcut add
                if rec.scale is not None:       # folded BN: z = scale*conv + shift
                    dy, dgamma, d["beta"] = convblock.frozen_bn_backward(y, dout, rec.scale, p["gamma"], p["beta"], act, 0.1,
                                                                         want_sums=nd.want_affine)
                    d["gamma"] = dgamma          # (behind beta: the order in which the reducer's sink sees them)
                else:
                    dy = ops.act_bwd(y, dout, 0.1) if op.leaky else dout
                    if p["b"] is not None and nd.want_affine:
                        d["b"] = dy.reshape(-1, op.cout).sum(0)
                ady = None            # (frozen-BN path: the GEMMs below compute the abs-max of dy themselves)
            if nd.want_res:
                add(op.res, dout)
            release()                  # (behind this layer's BatchNorm passes: the main chain stays the first dependent of the data gradient before)

            def dgrad():
                if not nd.want_dx:
                    return
                cur = g.get(op.src)
                b16 = s16 and dy.dtype == torch.bfloat16
                prev = producer.get(op.src)
                tap = None
                if prev is not None and prev.bn and first_use.get(op.src) == index_of[id(op)]:
                    tap = convblock.bn_tap_for(b16, training, x.shape[3], op.k, op.stride, save.get(prev.slot), P[prev.slot]["gamma"],
                                               P[prev.slot]["beta"], ops.ACT_LEAKY if prev.leaky else ops.ACT_NONE, 0.1)
                fb = rec.bank              # the banks of this step (ops.FilterBanks; None: transposed per launch)
                dx, part = convblock.conv_dgrad(dy, x.shape, op.k, op.stride, w=rec.w, bank=fb, out=cur, accumulate=cur is not None, tap=tap,
                                                amax_dy=ady, amax_w=rec.aw, wt_ready=fb and (fb["t"], fb["tsplit"]), wt_b16=fb and fb["tb16"])
                if part is not None:
                    tapped[prev.slot] = part
                if cur is None:
                    g[op.src] = dx

            # (a frozen weight: the data gradient alone, nothing is handed to the side stream or held)
            _, dw = convblock.schedule_wgrad(x, dy, op.k, op.stride, shape, dgrad, amax_x=rec.ax, amax_dy=ady, may_hold=True, want_w=nd.want_w)
            if isinstance(dw, ops.HeldWgrad):      # launched behind the next layer's BatchNorm passes (release)
                held = (d, op.slot, dw)
            else:
                d["w"] = dw
            finished(op.slot, keep(d))
    release()
    if sink is not None and pending:
        sink(pending)
    if pg:
        ops.join_side(next(iter(P.values()))["w"].device)
    return pg


class _DarknetFn(torch.autograd.Function):
    """The whole backbone as one autograd node.  Flat parameter order per conv slot:
    weight, (bias | gamma, beta)."""

    @staticmethod
    def forward(ctx, net: "Darknet", training: bool, image: torch.Tensor, *flat):
        plan, taps = net._plan, net._taps
        P = net._param_table(flat, ctx.needs_input_grad[3:])
        x = ops.nchw_to_nhwc(image.contiguous(), 4)
        # (needs_input_grad speaks about the parameters, not about the caller's grad mode: under torch.no_grad() — inference — nothing is
        #  saved and every layer is ONE kernel with BatchNorm, activation and shortcut in its epilogue; forward_nhwc notes the mode, since
        #  inside a Function's forward grad mode is always off)
        # requires_grad decides the work (backward_needs): the layers that keep a record are those with a trainable parameter in or
        # below them.  With no trainable parameter at all autograd sees no node here, and nothing is kept.
        trainable = frozenset((slot, k_) for slot, d_ in P.items() for k_, on_ in d_["train"].items() if on_)
        live = backward_needs(plan, trainable).live
        grad_on = bool(net.__dict__.get("_grad_on", True))
        need_grad = bool(live) and grad_on
        ctx.no_backward_reason = None if need_grad else "nothing was saved: the forward ran with gradients off (or no parameter requires one)"
        if ops.storage_f8() and not training and need_grad:
            need_grad = False          # fp8 storage has no frozen-BatchNorm backward: inference only with running statistics (backward() says so)
            ctx.no_backward_reason = ("fp8 storage has no backward with BatchNorm on its running statistics (eval mode, freeze_batchnorm): "
                                      "fp32 and bf16 storage (\"bf16s\") have it")
        save = {} if need_grad else None
        # the kernels of the forward do not depend on what is frozen: batch statistics take the training forward whenever the caller
        # has gradients on; running statistics with no backward to come (nothing trainable, or fp8 storage) take the inference forward
        outs, tap_amax, net._early_event = _run_forward(plan, taps, x, P, training, save, net._filter_banks(P),
                                                        taps_b16=bool(net.__dict__.get("_taps_b16")), live=live,
                                                        backward=need_grad or (training and grad_on))
        net._tap_amax = tap_amax              # abs-max words of the three taps (read by the head's first convolutions)
        net.__dict__["saved_slots"] = frozenset(save) if save is not None else frozenset()
        if save is not None:
            for rec in save.values():
                rec.unlink_outputs(outs)          # (outputs go through save_for_backward)
            ctx.save_for_backward(*outs)
        ctx.net, ctx.training, ctx.save, ctx.nflat = net, training, save, len(flat)
        ctx.P, ctx.trainable = P, trainable
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        net = ctx.net
        if ctx.save is None:
            why = getattr(ctx, "no_backward_reason", None) or ("this node's saved tensors were consumed by an earlier backward "
                                                               "(one backward per forward; retain_graph is not supported)")
            raise (NotImplementedError if "fp8 storage" in why else RuntimeError)("dcnet_amd.Darknet: " + why)
        outs = ctx.saved_tensors
        save = ctx.save
        ctx.save = None
        for rec in save.values():
            rec.link_outputs(outs)
        red = net.__dict__.get("_grad_reducer")       # parallel.OverlappedGradReducer (data-parallel runs), else None
        sink = None
        if red is not None:
            pmap = net._slot_params()
            sink = lambda items: red.push([(pmap[(slot, key)], t) for slot, key, t in items if (slot, key) in pmap])
        pg = _run_backward(net._plan, net._taps, grads, ctx.P, save, ctx.training, sink, red.bucket_bytes if red is not None else 0,
                           trainable=ctx.trainable)
        if red is not None:
            red.join_backward()                        # the averaged gradients are complete before autograd sees them
        flat_grads: List[Optional[torch.Tensor]] = []
        for op in net._conv_ops:
            d = pg.get(op.slot, {})
            flat_grads.append(d.get("w"))
            if op.bn:
                flat_grads += [d.get("gamma"), d.get("beta")]
            else:
                flat_grads.append(d.get("b"))
        return (None, None, None) + tuple(flat_grads)


class Darknet(nn.Module):
    """YOLOv3 backbone (drop-in for model/darknet.py:377-431).  ``forward`` returns the list of
    taps [1024@S/32, 512@S/16, 256@S/8] in NCHW like the reference; ``forward_nhwc`` hands the
    NHWC tensors to the rest of this package without a layout round trip."""

    def __init__(self, config_path: str = "./model/yolov3.cfg", img_size: int = 416, obj_out: bool = False):
        super().__init__()
        if obj_out:
            raise NotImplementedError("obj_out=True (YOLO detection output) is outside the DCNet hot path")
        self.config_path = config_path
        self.obj_out = obj_out
        if config_path and os.path.exists(config_path):
            self.module_defs = parse_model_config(config_path)
        else:
            self.module_defs = yolov3_blocks()
        self.hyperparams, self.module_list = create_modules(self.module_defs)
        self.img_size = img_size
        self.seen = 0
        self.header_info = np.array([0, 0, 0, self.seen, 0], dtype=np.int32)
        self._plan, self._taps, self._ch = build_plan(self.module_defs, int(self.hyperparams["channels"]))
        self._conv_ops = [op for op in self._plan if isinstance(op, _ConvOp)]
        self.saved_slots = frozenset()       # the slots whose layers kept a record for the backward in the last forward

    # -- parameter plumbing -------------------------------------------------------------------
    def _flat_params(self) -> List[torch.Tensor]:
        flat = []
        for op in self._conv_ops:
            seq = self.module_list[op.slot]
            conv = seq[0]
            flat.append(conv.weight)
            if op.bn:
                flat += [seq[1].weight, seq[1].bias]
            else:
                flat.append(conv.bias)
        return flat

    def _param_table(self, flat, needs=None):
        """needs (optional): per entry of ``flat``, does it need a gradient (default: all do)."""
        P = {}
        it = iter(flat)
        nd = iter(needs if needs is not None else [True] * len(flat))
        for op in self._conv_ops:
            seq = self.module_list[op.slot]
            d = dict(w=next(it).detach(), b=None, gamma=None, beta=None, rm=None, rv=None, momentum=0.1, affine_grad=True)
            d["train"] = {"w": bool(next(nd))}          # which of the layer's parameters want a gradient (backward_needs)
            if op.bn:
                bn = seq[1]
                d["gamma"], d["beta"] = next(it).detach(), next(it).detach()
                d["train"]["gamma"], d["train"]["beta"] = bool(next(nd)), bool(next(nd))
                d["affine_grad"] = d["train"]["gamma"] | d["train"]["beta"]      # (frozen statistics: False = no partial sums in the backward)
                d["rm"], d["rv"], d["momentum"] = bn.running_mean, bn.running_var, bn.momentum
            else:
                d["b"] = next(it).detach()
                d["train"]["b"] = bool(next(nd))
            P[op.slot] = d
        return P

    def trainable_keys(self) -> frozenset:
        """The (slot, key) pairs of the live convolutions whose parameter has ``requires_grad`` now (the argument of backward_needs)."""
        return frozenset(k_ for k_, p_ in self._slot_params().items() if p_.requires_grad)

    def backward_needs(self) -> BackwardNeeds:
        """What a backward through this module would launch with the parameters' ``requires_grad`` as it stands (darknet.backward_needs).
        After a forward ``saved_slots`` holds the slots that kept a record for it: ``backward_needs().live`` with gradients on."""
        return backward_needs(self._plan, self.trainable_keys())

    def _slot_params(self):
        """{(slot, "w" | "gamma" | "beta" | "b"): parameter} of the live convolutions."""
        out = {}
        for op in self._conv_ops:
            seq = self.module_list[op.slot]
            out[(op.slot, "w")] = seq[0].weight
            if op.bn:
                out[(op.slot, "gamma")] = seq[1].weight; out[(op.slot, "beta")] = seq[1].bias
            elif seq[0].bias is not None:
                out[(op.slot, "b")] = seq[0].bias
        return out

    def _filter_banks(self, P):
        """All filter banks of the backbone in their GEMM forms, refreshed once per forward (ops.FilterBanks: three launches
        instead of ~5 small kernels per layer; the banks of a step serve its backward too)."""
        if not ops.FILTER_BANKS:
            return None
        fb = convblock.cached_filter_banks(self.__dict__, "_fbanks", {slot: d["w"] for slot, d in P.items()})
        # the refresh (0.6 ms of kernels) runs on a stream of its own, beside the image transpose and the stem, which do not read
        # the banks; _run_forward joins it in front of the first convolution that does
        main = torch.cuda.current_stream()
        prep = self.__dict__.get("_prep_stream")
        if prep is None or prep.device != main.device:
            prep = torch.cuda.Stream(device=main.device)
            self.__dict__["_prep_stream"] = prep
        prep.wait_stream(main)                        # (the parameters' last writer and the banks' last readers are on `main`)
        with torch.cuda.stream(prep):
            fb.refresh()
        fb.pending = prep
        return fb

    def forward_nhwc(self, x: torch.Tensor, taps_b16: bool = False) -> List[torch.Tensor]:
        """taps_b16 (bf16-storage mode only): hand the three taps out as the bf16 tensors they are instead of casting them to fp32."""
        self.__dict__["_taps_b16"] = bool(taps_b16) and ops.storage_b16()
        self.__dict__["_grad_on"] = torch.is_grad_enabled()
        if not x.is_cuda:
            raise RuntimeError("dcnet_amd.Darknet runs on an MI355X only: move the model and inputs to cuda "
                               "(there is no CPU path; the CPU restatement lives in oracle/ for tests)")
        training = self.training and not self.__dict__.get("_bn_frozen", False)      # (the BatchNorm mode is all that `training` means here)
        if training:
            torch._foreach_add_([self.module_list[op.slot][1].num_batches_tracked for op in self._conv_ops if op.bn], 1)
        return list(_DarknetFn.apply(self, training, x, *self._flat_params()))

    def freeze_batchnorm(self, frozen: bool = True) -> None:
        """Hold every BatchNorm of the backbone at its running statistics whatever ``.training`` says (grounding_model.freeze_batchnorm):
        the forward normalises with them and leaves them and num_batches_tracked alone, the backward is the frozen one, and the
        nn.BatchNorm2d modules report ``.training == False``.  Survives train() / eval()."""
        self.__dict__["_bn_frozen"] = bool(frozen)
        self.train(self.training)

    def train(self, mode: bool = True):
        super().train(mode)
        if self.__dict__.get("_bn_frozen", False):
            for m in self.modules():
                if isinstance(m, nn.modules.batchnorm._BatchNorm):
                    m.training = False
        return self

    def forward(self, x, targets=None):
        if targets is not None:
            raise NotImplementedError("YOLO detection training (targets=...) is outside the DCNet hot path")
        return [t.permute(0, 3, 1, 2) for t in self.forward_nhwc(x)]

    # -- darknet binary weights (model/darknet.py:433-513) -----------------------------------
    def load_weights(self, weights_path: str) -> None:
        """[5 x int32 header] then per conv slot: (bn.bias, bn.weight, running_mean, running_var | conv.bias),
        conv.weight — for EVERY conv slot incl. the dead YOLO heads (file compatibility)."""
        with open(weights_path, "rb") as fp:
            header = np.fromfile(fp, dtype=np.int32, count=5)
            weights = np.fromfile(fp, dtype=np.float32)
        self.header_info = header
        self.seen = int(header[3])
        ptr = 0

        def take(t: torch.Tensor):
            nonlocal ptr
            n = t.numel()
            if ptr + n > weights.size:
                raise ValueError(f"{weights_path}: truncated weights file")
            t.data.copy_(torch.from_numpy(weights[ptr:ptr + n]).view_as(t))
            ptr += n

        for d, seq in zip(self.module_defs, self.module_list):
            if d["type"] in ("convolutional", "yoloconvolutional"):
                conv = seq[0]
                if int(d["batch_normalize"]):
                    bn = seq[1]
                    take(bn.bias); take(bn.weight); take(bn.running_mean); take(bn.running_var)
                else:
                    take(conv.bias)
                take(conv.weight)

    def save_weights(self, path: str, cutoff: int = -1, reference_layout: bool = False) -> None:
        """Writes every conv slot, i.e. the format ``load_weights`` (here and in the reference, model/darknet.py:433-483)
        reads.  The reference's own writer (model/darknet.py:490-513) skips the three ``yoloconvolutional`` slots, so its
        files cannot be read back by its loader; ``reference_layout=True`` reproduces that file byte for byte
        (pinned by oracle/make_format_goldens.py)."""
        hdr = np.array(self.header_info, dtype=np.int32).copy()
        hdr[3] = self.seen
        defs = self.module_defs if cutoff == -1 else self.module_defs[:cutoff]
        if reference_layout and cutoff == -1:
            defs = self.module_defs[:-1]                     # the reference slices [:cutoff] with cutoff = -1 (:498)
        kinds = ("convolutional",) if reference_layout else ("convolutional", "yoloconvolutional")
        with open(path, "wb") as fp:
            hdr.tofile(fp)
            for d, seq in zip(defs, self.module_list):
                if d["type"] in kinds:
                    conv = seq[0]
                    if int(d["batch_normalize"]):
                        bn = seq[1]
                        for t in (bn.bias, bn.weight, bn.running_mean, bn.running_var):
                            t.detach().cpu().numpy().astype(np.float32).tofile(fp)
                    else:
                        conv.bias.detach().cpu().numpy().astype(np.float32).tofile(fp)
                    conv.weight.detach().cpu().numpy().astype(np.float32).tofile(fp)
