"""The conv + BatchNorm + activation block of the backbone (darknet) and of the head (functions), forward and backward, in every
storage mode: fp32 tensors, bf16 storage ("bf16s"), fp8 operand storage on top of it ("fp8s").

The callers own their graphs (the layer plan, the autograd contexts, the streams they join); which kernel a pass takes and in which
order a block launches its passes is decided here and only here.  Every switch (ops.WGRAD_*, ops.BN_TAP*, ops.PRE_ACT, the precision
mode) is read from ``ops`` when a function runs.
"""
from __future__ import annotations

import torch

from . import ops


def conv_forward(x, ksize, stride, cout, w=None, bank=None, scale=None, shift=None, act=ops.ACT_NONE, slope=0.0, residual=None, out=None,
                 want_stats=False, accumulate=False, out_f32=False, fold=None, amax_x=None, amax_w=None, amax_out=None, w_split=None,
                 w_b16=None, drop_q8=False):
    """One forward convolution with its epilogue.  Returns (y, stats): the [rows][2][Cout] partial sums with ``want_stats``, the folded
    (scale, shift) rows with ``fold``, else None.

    x fp32 (or an ops.PreAct): ``w`` the OHWI bank with its abs-max word ``amax_w`` and, from an ops.FilterBanks entry, its prepared forms
    ``w_split`` / ``w_b16``.  x bf16 (bf16 storage): ``bank`` holds the bf16 bank "b16" — a FilterBanks entry, or a dict made for one
    launch — and the layer runs on e4m3 operands where ops.f8_takes says so: the copy of x its producer wrote beside it (ops.quant_of;
    ``drop_q8``: this is its last reader) and the bank's "q8" form, else a quantisation pass each.  y is bf16, fp32 with ``out_f32``.
    fold = (gamma, beta, running_mean, running_var, eps): frozen BatchNorm as the epilogue's scale and shift (folded here, behind the
    operands' own passes)."""
    b16 = not isinstance(x, ops.PreAct) and x.dtype == torch.bfloat16
    if b16 and bank is None:
        raise RuntimeError("bf16 storage needs the prepared filter banks (ops.FILTER_BANKS) for every layer behind the stem")
    use8 = b16 and ops.f8_takes(x.shape[3], cout, ksize)          # "fp8s": this layer's forward on e4m3 operands
    if use8:
        x8, xs = ops.quant_of(x)
        # the copy rides on the tensor, which the backward keeps (its weight gradient reads the bf16 values): drop it once
        # the last e4m3 reader has it (round-5 advice: ~0.3 GB of dead bytes at 64 images otherwise)
        if drop_q8 and hasattr(x, "_dcn_q8"):
            del x._dcn_q8
        w8, ws = ops.bank_q8(bank, "q8", bank["b16"], cout)          # (made once per step by FilterBanks.refresh)
    ss = ops.bn_fold(*fold) if fold is not None else None
    if ss is not None:
        scale, shift = ss[0], ss[1]
    if use8:
        y, stats = ops.conv2d_fwd_f8(x8, xs, w8.view(-1), ws, cout, ksize, stride, scale, shift, act, slope, residual=residual,
                                     want_stats=want_stats, out_f32=out_f32)
    elif b16:
        y, stats = ops.conv2d_fwd_b16(x, bank["b16"], cout, ksize, stride, scale, shift, act, slope, residual=residual, out=out,
                                      want_stats=want_stats, accumulate=accumulate, out_f32=out_f32)
    else:
        y, stats = ops.conv2d_fwd(x, w, ksize, stride, scale, shift, act, slope, residual=residual, out=out, want_stats=want_stats,
                                  accumulate=accumulate, amax_x=amax_x, amax_w=amax_w, amax_out=amax_out, w_split_ready=w_split, w_b16=w_b16)
    return y, (stats if want_stats else ss)


def last_q8_reader(left: dict, key, n_readers: int) -> bool:
    """fp8 storage: count one e4m3 reader of tensor ``key`` (of ``n_readers`` in the plan); True for the last (conv_forward's drop_q8)."""
    left[key] = left.get(key, n_readers) - 1
    return left[key] <= 0


def train_bn_forward(y, stats, gamma, beta, eps, momentum, running_mean, running_var, act, slope, bn=None, residual=None, amax_out=None,
                     amax_y=None, out_b16=False, out_f32=False, quant=False):
    """Train-mode BatchNorm + activation behind a convolution's raw output y and its partial sums.  Returns (mi, out, amax_out):
    mi = rows mean, invstd, scale, shift.  ``bn``: the module whose num_batches_tracked advances (the backbone advances all of its
    at once).  amax_y (the abs-max word the convolution wrote with y): the sole reader forms the activation while loading — out is an
    ops.PreAct, its word a bound derived from amax_y.  Else one ops.scale_act pass (out_b16 / out_f32 / quant: as there)."""
    mi = ops.bn_finalize(stats, y.numel() // y.shape[-1], gamma, beta, eps, momentum, running_mean, running_var)
    if bn is not None:
        ops.bump_batches(bn)
    if amax_y is not None and y.is_contiguous():
        amax_out = ops.bn_act_amax_bound(amax_y, mi[2], mi[3], slope)
        out = ops.PreAct(y, mi[2], mi[3], act, slope)
        if ops.PRE_ACT == "check":        # (tests: the activation written out, read with the same abs-max word)
            out = out.materialise()
        return mi, out, amax_out
    out = ops.scale_act(y, mi[2], mi[3], act, slope, residual=residual, amax_out=amax_out, out_b16=out_b16, out_f32=out_f32, quant=quant)
    return mi, out, amax_out


def frozen_bn_backward(y, dout, scale, gamma, beta, act, slope, want_sums=True):
    """Backward of out = act(scale*conv + shift) with BatchNorm folded from running statistics; y holds the activation (before a
    shortcut add), fp32 or — bf16 storage — bf16.  Returns (dconv, dgamma, dbeta), the last two None without ``want_sums`` (gamma and
    beta frozen).  One pass of csrc/frozen_bn.h."""
    return ops.frozen_bn_act_bwd(y, dout, scale, gamma, beta, act, slope, want_sums=want_sums)


def bn_tap_for(b16: bool, training: bool, cin: int, ksize: int, stride: int, prev, gamma, beta, act, slope):
    """The ``tap`` argument of conv_dgrad, or None.  prev: the SavedLayer of the conv + train-mode BatchNorm + activation layer whose
    output this data gradient completes the gradient of (None when there is no such layer); gamma, beta, act, slope are that layer's.
    The two storage modes admit different launches:"""
    if not (ops.BN_TAP and training and prev is not None):
        return None
    trunk = ops.BN_TAP_TRUNK
    if b16:
        # bf16 storage: every stride-1 layer, the tapped raw output a bf16 tensor
        ok = trunk and stride == 1 and torch.is_tensor(prev.y) and prev.y.dtype == torch.bfloat16
    else:
        # fp32: the register-bank kernel of the stride-2 layer behind the stem; every stride-1 layer on conv1.hip / conv3.hip
        # (BN_TAP_TRUNK 2: the 3x3 ones only, any other number: the 1x1 ones only)
        ok = ((cin == 32 and stride == 2 and ksize == 3)
              or (trunk and stride == 1 and cin >= 64 and (trunk is True or trunk == 1 or (trunk == 2) == (ksize == 3)))) and torch.is_tensor(prev.y)
    if not (ok and prev.y.is_contiguous()):
        return None
    return dict(y=prev.y, mean=prev.mi[0], invstd=prev.mi[1], gamma=gamma, beta=beta, act=act, slope=slope)


def conv_dgrad(dy, in_shape, ksize, stride, w=None, bank=None, out=None, accumulate=False, tap=None, out_f32=False, amax_dy=None,
               amax_w=None, wt_ready=None, wt_b16=None):
    """The data gradient of a convolution whose input had ``in_shape`` (N,H,W,Cin).  Returns (dx, partials): the partial sums of the
    tapped BatchNorm backward (bn_tap_for) when the launch formed them, else None.
    dy fp32: ``w`` the OHWI bank, ``amax_*`` the operands' words, ``wt_ready`` / ``wt_b16`` the transposed forms of a FilterBanks entry.
    dy bf16: ``bank`` holds the transposed bf16 bank "tb16" (and, "fp8s", its e4m3 form "tq8"); dx is bf16, fp32 with ``out_f32``."""
    hw, cin = (in_shape[1], in_shape[2]), in_shape[3]
    if dy.dtype == torch.bfloat16:
        if ops.f8_takes(dy.shape[3], cin, ksize) and dy.is_contiguous():      # "fp8s": the data gradient on e4m3 operands
            dy8, dys = ops.quant_of(dy)
            wt8, wts = ops.bank_q8(bank, "tq8", bank["tb16"], cin)
            res = ops.conv2d_bwd_data_f8(dy8, dys, wt8.view(-1), wts, hw, cin, ksize, stride, out=out, accumulate=accumulate, tap=tap,
                                         out_f32=out_f32)
        else:
            res = ops.conv2d_bwd_data_b16(dy, bank["tb16"], hw, cin, ksize, stride, out=out, accumulate=accumulate, tap=tap, out_f32=out_f32)
    else:
        res = ops.conv2d_bwd_data(dy, w, hw, ksize, stride, out=out, accumulate=accumulate, amax_dy=amax_dy, amax_w=amax_w,
                                  wt_ready=wt_ready, wt_b16=wt_b16, tap=tap)
    return res if tap is not None else (res, None)


def schedule_wgrad(x, dy, ksize, stride, wshape, dgrad, amax_x=None, amax_dy=None, after=None, may_hold=False, direct_into=None,
                   want_w=True):
    """Launch a layer's two gradients in the order of the schedule: ``dgrad()`` launches the data gradient on the current stream, the
    weight gradient of (x, dy) goes to the side stream (ops.WGRAD_SIDE off: the current one).  Returns (dgrad(), dw): dw the OIHW
    gradient — the caller joins the side stream (ops.join_side) before it is read —, but
      * direct_into = the parameter (ops.WGRAD_DIRECT, the head's blocks): what the block before held goes out first, this block's
        gradient is held, to be added to ``.grad`` on the side stream behind the next block's passes; dw is None;
      * after False (the blocks that never had another order): the weight gradient first, beside its own data gradient;
      * after None = ops.WGRAD_AFTER_DGRAD: queued behind the data gradient, beside the next layer's BatchNorm passes — with
        may_hold (the backbone) and ops.WGRAD_HELD as an ops.HeldWgrad the caller issues behind the next layer's passes;
      * want_w False (the weight is frozen): no weight gradient at all, dw is None and nothing is held or handed to the side stream —
        what the block before held still goes out at the place it would have (ops.WGRAD_DIRECT)."""
    if not want_w:
        if ops.WGRAD_DIRECT:
            ops.release_held_wgrads()
        return dgrad(), None
    if direct_into is not None:
        ops.release_held_wgrads()
        dx = dgrad()
        ops.hold_wgrad_into(direct_into, x, dy, ksize, stride, wshape, amax_x=amax_x, amax_dy=amax_dy)
        return dx, None
    if not (ops.WGRAD_AFTER_DGRAD if after is None else after):
        dw = ops.wgrad_on_side(x, dy, ksize, stride, wshape, amax_x=amax_x, amax_dy=amax_dy)     # overlaps with the data gradient below
        return dgrad(), dw
    dx = dgrad()
    if may_hold and ops.WGRAD_SIDE and ops.WGRAD_HELD:
        return dx, ops.HeldWgrad(x, dy, ksize, stride, wshape, amax_x=amax_x, amax_dy=amax_dy)
    return dx, ops.wgrad_on_side(x, dy, ksize, stride, wshape, amax_x=amax_x, amax_dy=amax_dy)


def direct_wgrad_param(weight, training: bool = True):
    """The parameter a head block adds its weight gradient to itself (ops.WGRAD_DIRECT, see there), else None."""
    return weight if (ops.WGRAD_DIRECT and ops.WGRAD_SIDE and training and isinstance(weight, torch.nn.Parameter)
                      and weight.requires_grad) else None


class SavedLayer:
    """What a backbone conv layer keeps for its backward: its input x (tensor or ops.PreAct), the tensor y its BatchNorm backward reads
    (train mode: the raw convolution output, with ``mi`` = rows mean, invstd, scale, shift; frozen statistics: the activation before
    the shortcut add, with ``scale`` = the folded BatchNorm scale or None for a biased convolution), the OHWI bank ``w`` with the
    abs-max words of x and w, and this step's FilterBanks entry ``bank`` (None: per-launch preparation)."""
    __slots__ = ("x", "y", "mi", "scale", "w", "bank", "ax", "aw")

    def __init__(self, x, y, w, bank, ax, aw, mi=None, scale=None):
        self.x, self.y, self.mi, self.scale, self.w, self.bank, self.ax, self.aw = x, y, mi, scale, w, bank, ax, aw

    def unlink_outputs(self, outs) -> None:
        """An autograd node must reach its own outputs through save_for_backward only (an attribute reference is a ctx <-> output
        cycle that pins the whole activation set until the GC runs): replace such an x by its position in ``outs``."""
        for k, o in enumerate(outs):
            if self.x is o:
                self.x = ("tap", k)

    def link_outputs(self, outs) -> None:
        if isinstance(self.x, tuple):
            self.x = outs[self.x[1]]


def cached_filter_banks(holder: dict, key: str, weights: dict):
    """The ops.FilterBanks table of ``weights`` ({index: OIHW tensor}) kept in ``holder[key]``.  The job table holds raw parameter
    addresses, so it is rebuilt when a parameter moved.  The caller refreshes it (once per forward, on the stream of its choice)."""
    if holder.get(key) is None or not holder[key].valid_for(weights):
        holder[key] = ops.FilterBanks(weights, next(iter(weights.values())).device)
    return holder[key]
