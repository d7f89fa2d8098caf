"""Training / evaluation harness around the hot path — the pieces of train_DCNet.py that a caller needs
to drive ``grounding_model`` without the reference's data pipeline:

  * ``make_optimizer``      RMSprop with the reference's two parameter groups, or its Adam / SGD (train_DCNet.py:519-534), or AdamW
  * ``adjust_learning_rate`` polynomial decay (train_DCNet.py:241-253)
  * ``train_step``          forward + five losses + backward + step, no host sync inside
  * ``evaluate``            eval forward + box decode + Acc@0.5 / mean IoU (train_DCNet.py:764-816)
  * ``save_checkpoint`` / ``load_checkpoint`` / ``load_pretrain``   the reference's ``.pth.tar`` dict
    (train_DCNet.py:255-263, 485-514) including the ``module.`` key prefix left by DDP wrappers

``--ema-decay D`` / ``--ema-tau T`` keep an exponential moving average of the weights inside the fused step (``dcnet_amd.optim.WeightEMA``);
the closing evaluation then reports the raw and the averaged weights.

``--n-frame K`` trains the window model the inference path evaluates (``forward(image, word_id, word_mask, K)``, ``losses.window_loss``).

``python -m dcnet_amd.train --steps 20`` (``--freeze-bn backbone|all``: BatchNorm on its running statistics; ``--freeze-weights backbone|K``:
the backbone, or its modules 0..K, not trained and without a backward) runs a short synthetic-data training loop on one GPU; with ``--raw-frames`` every step's
``image`` / ``bbox`` come from synthetic uint8 frames of mixed sizes (1280x720 and 500x375) through the on-device clip
preprocessing (``dcnet_amd.prep.prepare_clips``: flip, HSV, letterbox, affine, normalisation), as real decoded frames would.
"""
from __future__ import annotations

import argparse
import os
import random
import shutil
from typing import Dict, Iterable, Optional, Tuple

import torch

from . import losses, ops


def make_optimizer(model, lr: float = 1e-4, optimizer: str = "RMSprop", fused: bool = True, max_grad_norm: Optional[float] = None,
                   skip_nonfinite: bool = False, accum_steps: int = 1):
    """The optimiser the reference builds for ``--optimizer`` (train_DCNet.py:519-534).  ``model`` may be DDP-wrapped.

    ``"RMSprop"`` (the default): two groups, everything except the backbone at ``lr``, the Darknet backbone at ``lr / 10``; weight
    decay 5e-4.  ``"adam"``: one group over all parameters, weight decay 5e-4.  ``"sgd"``: one group, momentum 0.99.  ``"adamw"`` (not
    in the reference; what fine-tuning recipes pair with a weight EMA): one group, decoupled weight decay 1e-2.  All are
    the fused classes of ``dcnet_amd.optim`` (torch's update as one HIP pass, torch's ``state_dict`` layout, and the protocol
    ``graph.GraphedTrainStep`` captures); ``fused=False`` returns the ``torch.optim`` classes for Adam, AdamW and SGD instead.

    Every parameter is listed, in ``model.parameters()`` order, whether or not it is trainable — the reference's RMSprop
    groups hold [93, 222] tensors including the dead YOLO heads and ``feature_map`` — so that the ``optimizer`` entry
    of a ``.pth.tar`` checkpoint moves between the reference and this harness in both directions even after
    ``parallel.freeze_gradless`` has run.  Parameters without a gradient are skipped by the step, as in torch.

    ``max_grad_norm`` / ``skip_nonfinite``: the fused classes' global-norm gradient clipping and non-finite skip, computed on the
    device inside the step (``dcnet_amd.optim``; the reference has neither).  One norm over all groups.  In a data-parallel run the
    optimiser steps after the gradient all-reduce, so every rank clips by the same norm of the same averaged gradient.  torch's
    classes have no such step: with ``fused=False`` call ``dcnet_amd.optim.clip_grad_norm_`` before ``step()`` yourself.

    ``accum_steps = K``: the fused classes' gradient accumulation — every K-th ``step()`` updates, with the mean gradient of the K
    calls (``dcnet_amd.optim``; 4 B per trained parameter).  It raises the effective batch of the update only: BatchNorm's statistics,
    the sampling heads' draws and the contrastive losses' negatives stay per micro-batch.  Fused classes only."""
    from . import optim
    core = model.module if hasattr(model, "module") else model
    name = optimizer.lower()
    clip = dict(max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite, accum_steps=accum_steps)
    if isinstance(accum_steps, bool) or not isinstance(accum_steps, int) or accum_steps < 1:
        raise ValueError(f"make_optimizer: accum_steps must be an integer >= 1, not {accum_steps!r}")
    if not fused and accum_steps != 1:
        raise ValueError("make_optimizer: accum_steps belongs to the fused optimisers (fused=False: scale the loss by 1 / K and step "
                         "every K-th backward yourself)")
    if not fused and (max_grad_norm is not None or skip_nonfinite):
        raise ValueError("make_optimizer: max_grad_norm / skip_nonfinite belong to the fused optimisers; with fused=False call "
                         "dcnet_amd.optim.clip_grad_norm_(model.parameters(), max_norm) before optimizer.step()")
    if name == "adam":
        return optim.Adam(list(core.parameters()), lr=lr, weight_decay=0.0005, **clip) if fused else \
            torch.optim.Adam(list(core.parameters()), lr=lr, weight_decay=0.0005)
    if name == "adamw":
        return optim.AdamW(list(core.parameters()), lr=lr, weight_decay=0.01, **clip) if fused else \
            torch.optim.AdamW(list(core.parameters()), lr=lr, weight_decay=0.01)
    if name == "sgd":
        return optim.SGD(list(core.parameters()), lr=lr, momentum=0.99, **clip) if fused else \
            torch.optim.SGD(list(core.parameters()), lr=lr, momentum=0.99)
    visu = list(core.visumodel.parameters())
    ids = {id(p) for p in visu}
    rest = [p for p in core.parameters() if id(p) not in ids]
    return optim.RMSprop([{"params": rest}, {"params": visu, "lr": lr / 10.}], lr=lr, weight_decay=0.0005, **clip)


def lr_poly(base_lr: float, it: int, max_iter: int, power: float) -> float:
    return base_lr * ((1 - float(it) / max_iter) ** power)                      # train_DCNet.py:241-242


def adjust_learning_rate(optimizer, i_iter: int, base_lr: float, nb_epoch: int, power: float = 0.9) -> float:
    """train_DCNet.py:244-253: group 0 at the polynomial rate, group 1 (backbone) at a tenth of it."""
    lr = lr_poly(base_lr, i_iter, nb_epoch, power) if power != 0. else base_lr
    optimizer.param_groups[0]["lr"] = lr
    if len(optimizer.param_groups) > 1:
        optimizer.param_groups[1]["lr"] = lr / 10
    return lr


def train_step(model, optimizer, image, word_id, word_mask, bbox, size: int, n_frame: Optional[int] = None):
    """One optimisation step (train_DCNet.py:580-646).  Returns (loss, dict of the five parts) as device
    tensors — reading them is the caller's (only) synchronisation point.
    ``n_frame = K``: a step of the window model — ``image`` (B * K, 3, S, S), ``word_id`` (B, L), ``bbox`` (B, 4) the boxes of the centre
    frames — with ``losses.window_loss`` (three parts: no sampling heads, no contrastive terms)."""
    model.train()
    if n_frame is None:
        out = model(image, word_id, word_mask)
        loss, parts = losses.total_loss(out, bbox, size)
    else:
        out = model(image, word_id, word_mask, n_frame)
        loss, parts = losses.window_loss(out, bbox, size)
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    optimizer.step()
    return loss.detach(), {k: v.detach() for k, v in parts.items()}


@torch.no_grad()
def evaluate(model, image, word_id, word_mask, bbox, size: int, n_frame: Optional[int] = None):
    """Eval forward, decode the arg-max box, IoU against ``bbox`` (xyxy pixels).  Returns
    (acc@0.5, mean IoU, boxes) as tensors (train_DCNet.py:764-816 / test_DCNet.py:373-470)."""
    model.eval()
    if n_frame is None:
        outbox = model(image, word_id, word_mask)[0]
    else:
        outbox = model(image, word_id, word_mask, n_frame)[0]
    boxes = losses.decode_boxes(list(outbox), size)
    iou = losses.bbox_iou(boxes, torch.clamp(bbox, min=0, max=size - 1))
    ops.check_bilstm(image.device)              # (evaluation results are read by the host anyway: one device synchronisation)
    return (iou > 0.5).float().mean(), iou.mean(), boxes


# ---- checkpoints ------------------------------------------------------------------------------------
def _strip_module(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    return {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}


def save_checkpoint(state: dict, is_best: bool, filename: str, directory: str = "./saved_models") -> str:
    """Writes ``<dir>/<filename>_checkpoint.pth.tar`` (+ ``_model_best`` copy), train_DCNet.py:255-263.
    ``state`` = {'epoch', 'state_dict', 'best_loss', 'optimizer'}, and optionally ``'ema'``: a ``dcnet_amd.optim.WeightEMA``'s
    ``state_dict()`` (its shadows and update count), which ``load_checkpoint(..., ema=ema)`` restores."""
    for t_ in state.get("state_dict", {}).values():
        if torch.is_tensor(t_) and t_.is_cuda:
            ops.check_bilstm(t_.device)         # (host-synchronising anyway: nothing is written after a timed-out BiLSTM hand-off)
            break
    os.makedirs(directory, exist_ok=True)
    ckpt = os.path.join(directory, f"{filename}_checkpoint.pth.tar")
    torch.save(state, ckpt)
    if is_best:
        shutil.copyfile(ckpt, os.path.join(directory, f"{filename}_model_best.pth.tar"))
    return ckpt


def load_checkpoint(model, path: str, optimizer=None, map_location="cpu", ema=None) -> Tuple[int, float]:
    """``--resume`` (train_DCNet.py:500-514): strict load of model (+ optimizer).  Accepts checkpoints saved
    from a DDP/DataParallel wrapper (``module.`` prefix) into a bare model and vice versa.  ``ema``: a ``dcnet_amd.optim.WeightEMA``
    that takes the checkpoint's ``"ema"`` entry (in place: its shadows and step word keep their addresses); ``KeyError`` if the
    checkpoint has none.  Without ``ema`` the entry is ignored, and a checkpoint without one loads as it always did."""
    ck = torch.load(path, map_location=map_location, weights_only=False)
    core = model.module if hasattr(model, "module") else model
    core.load_state_dict(_strip_module(ck["state_dict"]), strict=True)
    if optimizer is not None and "optimizer" in ck:
        optimizer.load_state_dict(ck["optimizer"])
    if ema is not None:
        if "ema" not in ck:
            raise KeyError(f"load_checkpoint: {path} has no 'ema' entry to restore the WeightEMA from")
        ema.load_state_dict(ck["ema"])
    return int(ck.get("epoch", 0)), float(ck.get("best_loss", float("inf")))


def load_pretrain(model, path: str, map_location="cpu") -> int:
    """``--pretrain`` (train_DCNet.py:485-499): load the intersection of keys with matching shapes.
    Returns the number of tensors taken."""
    ck = torch.load(path, map_location=map_location, weights_only=False)
    src = _strip_module(ck["state_dict"] if "state_dict" in ck else ck)
    core = model.module if hasattr(model, "module") else model
    own = core.state_dict()
    take = {k: v for k, v in src.items() if k in own and tuple(v.shape) == tuple(own[k].shape)}
    own.update(take)
    core.load_state_dict(own, strict=True)
    return len(take)


def arg_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="short synthetic-data training run of the HIP-backed DCNet")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--clips", type=int, default=2)
    ap.add_argument("--frames", type=int, default=None, help="frames per clip (default 2; with --n-frame K: K)")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--n-frame", type=int, default=None, metavar="K",
                    help="train the window model (forward(image, word_id, word_mask, K): the centre frame of every clip against its K - 1 "
                         "neighbours, one query and one box per clip, losses.window_loss); every clip is ONE window: --frames is then exactly K "
                         "(its default; any other value is an error)")
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--optimizer", choices=["rmsprop", "adam", "sgd", "adamw"], default="rmsprop", help="train_DCNet.py's --optimizer, and adamw")
    ap.add_argument("--raw-frames", action="store_true", help="feed uint8 frames through dcnet_amd.prep every step")
    ap.add_argument("--clip-grad-norm", type=float, default=None, metavar="X", help="clip the global gradient norm to X inside the fused step")
    ap.add_argument("--skip-nonfinite", action="store_true", help="a step whose gradient norm is inf or NaN updates nothing")
    ap.add_argument("--accum-steps", type=int, default=1, metavar="K",
                    help="accumulate gradients over K steps inside the fused step: --steps counts micro-steps, every K-th one updates, the schedule advances per update")
    ap.add_argument("--ema-decay", type=float, default=None, metavar="D",
                    help="keep an exponential moving average of the weights inside the fused step (dcnet_amd.optim.WeightEMA) and evaluate it too")
    ap.add_argument("--ema-tau", type=float, default=None, metavar="T", help="warm-up constant of the average: decay * (1 - exp(-t / T)); 0: none (default 2000)")
    ap.add_argument("--freeze-bn", choices=["none", "backbone", "all"], default="none",
                    help="hold BatchNorm at its running statistics while training (grounding_model.freeze_batchnorm): the backbone's, or every one")
    ap.add_argument("--freeze-bn-stats-only", action="store_true",
                    help="with --freeze-bn: freeze the statistics only, gamma and beta keep training (train_affine=True; default: they are frozen too)")
    ap.add_argument("--freeze-weights", type=freeze_weights_scope, default=None, metavar="{none,backbone,K}",
                    help="stop training the backbone (grounding_model.freeze_weights): all of it, or its modules 0..K (74: the Darknet-53 feature "
                         "extractor, the neck keeps training); frozen layers cost no backward and keep nothing for one.  Usually with --freeze-bn backbone")
    return ap


def freeze_weights_scope(text: str):
    """--freeze-weights: "none" -> None, "backbone", or an integer module index (the scope argument of grounding_model.freeze_weights)."""
    if text == "none":
        return None
    if text == "backbone":
        return text
    try:
        k = int(text)
    except ValueError:
        k = -1
    if k < 0:
        raise argparse.ArgumentTypeError(f"{text!r}: expected none, backbone or a module index >= 0")
    return k


def freeze_bn_args(args) -> Optional[dict]:
    """The freeze_batchnorm() arguments that --freeze-bn / --freeze-bn-stats-only ask for (None: leave BatchNorm alone)."""
    if args.freeze_bn == "none":
        return None
    return dict(scope=args.freeze_bn, train_affine=bool(args.freeze_bn_stats_only))


def ema_args(args) -> Optional[dict]:
    """The WeightEMA arguments that --ema-decay / --ema-tau ask for (None: no average; either flag alone takes the other's default)."""
    if args.ema_decay is None and args.ema_tau is None:
        return None
    return dict(decay=0.9999 if args.ema_decay is None else args.ema_decay, tau=2000.0 if args.ema_tau is None else args.ema_tau)


def main(argv: Optional[Iterable[str]] = None) -> None:
    ap = arg_parser()
    args = ap.parse_args(argv)
    K = args.n_frame
    if args.frames is None:
        args.frames = 2 if K is None else K
    if K is not None and (K < 2 or args.frames != K):
        ap.error(f"--n-frame {K}: needs K >= 2 and --frames {K} (every clip is one window of exactly K frames)")
    from .model import grounding_model
    from .parallel import freeze_gradless
    from .utils.synth import synth_boxes, synth_inputs
    dev = torch.device("cuda:0")
    torch.manual_seed(0); random.seed(0)
    model = grounding_model(corpus=list(range(1000)), emb_size=512, img_size=args.size, config_path="", weights_path=None).to(dev)
    freeze_gradless(model)
    fz = freeze_bn_args(args)
    if fz is not None:
        model.freeze_batchnorm(**fz)
    if args.freeze_weights is not None:
        model.freeze_weights(args.freeze_weights)
    opt = make_optimizer(model, args.lr, args.optimizer, max_grad_norm=args.clip_grad_norm, skip_nonfinite=args.skip_nonfinite,
                         accum_steps=args.accum_steps)
    ema = None
    if ema_args(args) is not None:
        from .optim import WeightEMA
        ema = WeightEMA(model, **ema_args(args))
        opt.attach_ema(ema)
    n = args.clips * args.frames
    # (the window model: one query and one box — the centre frame's — per clip)
    image, word_id, word_mask = (t.to(dev) for t in synth_inputs(n, args.size, n_queries=None if K is None else args.clips, seed=1))
    bbox = synth_boxes(n if K is None else args.clips, args.size, seed=1).to(dev)
    if args.raw_frames:
        import numpy as np
        from .prep import prepare_clips
        rs = np.random.RandomState(1)
        frames = [[rs.randint(0, 256, size=((720, 1280, 3) if (c + t) % 2 == 0 else (375, 500, 3)), dtype=np.uint8)
                   for t in range(args.frames)] for c in range(args.clips)]
        src_boxes = [[[60, 40, 300, 330]] * args.frames for _ in range(args.clips)]
        phrases = [["the object on the left"] * args.frames for _ in range(args.clips)]
        prep_rng = random.Random(1)               # the pipeline's own draws: Python's global stream stays the model's
    for it in range(args.steps):
        # the schedule is in units of updates: micro-step `it` belongs to update it // K of ceil(steps / K)
        adjust_learning_rate(opt, it // args.accum_steps, args.lr, -(-args.steps // args.accum_steps), 0.9)
        if args.raw_frames:
            res = prepare_clips(frames, src_boxes, phrases, args.size, True, rng=prep_rng, out=image)
            bbox.copy_(res.bbox if K is None else res.bbox.view(args.clips, K, 4)[:, K // 2])
        loss, parts = train_step(model, opt, image, word_id, word_mask, bbox, args.size, n_frame=K)
        if it % 5 == 0 or it == args.steps - 1:
            print(f"step {it:3d} loss {float(loss):9.4f}  " + " ".join(f"{k} {float(v):.4f}" for k, v in parts.items()))
    acc, miou, _ = evaluate(model, image, word_id, word_mask, bbox, args.size, n_frame=K)
    line = f"Acc@0.5 {float(acc):.3f}  mIoU {float(miou):.3f} (on the training clips)"
    if opt.grad_norm is not None:
        line += f"  last gradient norm {float(opt.grad_norm):.4g}  skipped steps {opt.skipped_steps()}"
    print(line)
    if ema is not None:
        with ema.applied():
            acc, miou, _ = evaluate(model, image, word_id, word_mask, bbox, args.size, n_frame=K)
        print(f"Acc@0.5 {float(acc):.3f}  mIoU {float(miou):.3f} (averaged weights: decay {ema.decay:g}, tau {ema.tau:g}, {ema.updates()} updates)")


if __name__ == "__main__":
    main()
