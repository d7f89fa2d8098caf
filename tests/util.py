"""Shared helpers for the parity tests (test infrastructure; may import oracle/)."""
import contextlib
import json
import os
import random

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def num_pos(size):
    return sum((size // 32 * 2 ** i) ** 2 for i in range(3))


def ref_shapes(size=256):
    """The reference's 597 state_dict keys/shapes (captured from the real reference at 256x256);
    only loc_text_embedding.0.weight depends on the image size (P = num_pos)."""
    with open(os.path.join(GOLD, "state_dict_keys_256.json")) as f:
        shapes = {k: tuple(v) for k, v in json.load(f).items()}
    shapes["loc_text_embedding.0.weight"] = (512, num_pos(size))
    return shapes


def synth_sd(size=256, seed=0):
    from dcnet_amd.utils.synth import apply_bn_calibration, synth_state_dict
    return apply_bn_calibration(synth_state_dict(ref_shapes(size), seed), os.path.join(GOLD, "bn_calib.npz"))


def new_product(size, test_model=False):
    """The drop-in grounding model as the reference's scripts construct it, parameters as initialised (no state dict)."""
    if test_model:
        from model.test_DCNet_model import grounding_model
    else:
        from model.DCNet_model import grounding_model
    return grounding_model(corpus=list(range(1000)), light=False, emb_size=512, coordmap=True,
                           bert_model="bert-base-uncased", dataset="vid", img_size=size,
                           config_path=os.path.join(ROOT, "model", "yolov3.cfg"), weights_path=None)


def build_product(size, sd, dev, test_model=False):
    m = new_product(size, test_model)
    m.load_state_dict(sd, strict=True)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0           # parity runs use p = 0 on both sides
    return m.to(dev)


def maxdiff(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


@contextlib.contextmanager
def tuning(knobs=None):
    """``with tuning({"Nconv": 0}) as tune:`` sets dcn_set_tuning knobs; ``tune({...})`` sets more inside the block.  On exit every knob
    has the value it had on entry again, read through dcn_tuning_info: no test needs to know a default."""
    from dcnet_amd.lib import lib, tuning as read

    def tune(kv):
        for k, v in kv.items():
            lib().set_tuning(k.encode(), v)

    before = {k: v["value"] for k, v in read().items()}
    try:
        tune(knobs or {})
        yield tune
    finally:
        for _ in range(2):          # ("precision" drives "wsplit" as well: the second pass puts back what the first pass's setters moved)
            tune({k: before[k] for k, v in read().items() if v["value"] != before[k]})


def rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def close(a, b, tol, name=""):
    """max |a - b| <= tol * max(1, |b|max) in fp64; the operands may live on different devices"""
    a = a.detach().double(); b = b.detach().double().to(a.device)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    ref = max(1.0, float(b.abs().max()))
    err = float((a - b).abs().max())
    assert err <= tol * ref, f"{name}: max err {err:.3e} vs tol {tol * ref:.3e}"


def gemm_err(out, ref64, scale64):
    """max_ij |out - ref64| / scale64 in fp64, where scale64 = |A|.|B|^T + |bias| + |residual| + |C_old| is what the rounding errors
    of element ij are proportional to: one wrong element of a small-magnitude row counts as much as one of a large row.  An element
    whose scale is 0 has nothing to round and must be exactly 0 (inf otherwise)."""
    out = out.detach().double().cpu(); ref64 = ref64.detach().double().cpu(); scale64 = scale64.detach().double().cpu()
    assert out.shape == ref64.shape == scale64.shape, (out.shape, ref64.shape, scale64.shape)
    if not bool(torch.isfinite(out).all()):
        return float("inf")
    d = (out - ref64).abs()
    zero = scale64 == 0
    if bool((d[zero] != 0).any()):
        return float("inf")
    return float((d / scale64.masked_fill(zero, 1.0)).max())


# A case's tolerance is GEMM_MARGIN * max(r32, 2**-24), r32 = gemm_err of torch's CPU fp32 evaluation of the same case (an independent
# fp32 implementation, computed at run time).  A differently ordered fp32 accumulation and the three-piece bf16 split each cost a small
# multiple of that figure.  Measured worst err / max(r32, 2**-24) on an MI355X over the tables of gemm_cases.py:
#   fp32 MFMA pipe (every tile, every entry point, "precision" 0 included): 4.40 (dcn_gemm_tn 132 x 64 at K = 1000; NT 3.37, NN 2.94)
#   bf16 three-piece split (NT / NN 128x128 from 1024 rows, TN 128x128 from K = 1024): 3.98 (dcn_gemm_tn 128 x 128 at K = 1056; NT 2.42)
# The margin started at 4; the long-K weight-gradient form exceeds that with a correct kernel (one fp32 accumulator over all of K against
# the CPU's blocked sum, whose own error is 1.0-1.3 units there), so it is 6, below the 8 at which it would be capped.
# test_gemm_host.py holds every case to this margin: five wrong references must fail at each.
GEMM_MARGIN = 6.0


def gemm_tol(r32):
    return GEMM_MARGIN * max(r32, 2.0 ** -24)


def prof_launches(tag=None):
    """launches booked under a profiling tag (all 64 tags as a list without one) since dcn_prof_enable(1) (csrc/prof.h)"""
    import ctypes
    from dcnet_amd.lib import lib
    c = (ctypes.c_int64 * 64)(); m = (ctypes.c_double * 64)(); wk = (ctypes.c_double * 64)()
    lib().prof_collect(ctypes.addressof(c), ctypes.addressof(m), ctypes.addressof(wk), 0)
    return list(c) if tag is None else c[tag]


def prof_counts(fn):
    """(fn(), launches per profiling tag while it ran)"""
    from dcnet_amd.lib import lib
    lib().prof_enable(1)
    try:
        out = fn()
    finally:
        lib().prof_enable(0)
    return out, prof_launches()


def conv_by_taps(x, w, k, stride, dy=None, dtype=torch.float64, chunk=None):
    """Reference convolution that shares nothing with the library: x (N,H,W,Ci) and w (Co,k,k,Ci) NHWC / OHWI on any device,
    'same' padding (k - 1) // 2, evaluated in ``dtype`` by torch.matmul one tap at a time on shifted slices of the padded input.
    Returns y (N,Ho,Wo,Co) and, with dy (N,Ho,Wo,Co), dx (N,H,W,Ci) and dw (Co,k,k,Ci); with ``chunk`` (a slice of output-pixel
    rows) also the part of dw those rows contribute (what zeroing them in the input would remove)."""
    n, h, wd, ci = x.shape
    co = w.shape[0]
    pad = (k - 1) // 2
    ho, wo = (h + 2 * pad - k) // stride + 1, (wd + 2 * pad - k) // stride + 1
    xp = torch.nn.functional.pad(x.to(dtype), (0, 0, pad, pad, pad, pad))
    wt = w.to(dtype)
    y = torch.zeros(n * ho * wo, co, dtype=dtype, device=x.device)
    dyf = None if dy is None else dy.to(dtype).reshape(-1, co)
    dxp = None if dy is None else torch.zeros_like(xp)
    dw = None if dy is None else torch.zeros(co, k, k, ci, dtype=dtype, device=x.device)
    dwc = None if (dy is None or chunk is None) else torch.zeros_like(dw)
    for r in range(k):
        for s in range(k):
            sl = (slice(None), slice(r, r + stride * (ho - 1) + 1, stride), slice(s, s + stride * (wo - 1) + 1, stride))
            xs = xp[sl].reshape(-1, ci)
            y += xs @ wt[:, r, s, :].t()
            if dy is not None:
                dxp[sl] += (dyf @ wt[:, r, s, :]).view(n, ho, wo, ci)
                dw[:, r, s, :] = dyf.t() @ xs
                if dwc is not None:
                    dwc[:, r, s, :] = dyf[chunk].t() @ xs[chunk]
            del xs
    y = y.view(n, ho, wo, co)
    if dy is None:
        return y
    dx = dxp[:, pad:pad + h, pad:pad + wd, :]
    return (y, dx, dw) if dwc is None else (y, dx, dw, dwc)
