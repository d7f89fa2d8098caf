"""Case tables for the kernels of dcnet_amd/csrc/loss.hip, shared by tests/test_loss_ref_host.py (CPU: the cases tell the wrong variants
of tests/loss_ref.py apart) and tests/test_loss_edges_gpu.py (the kernels against the references on the same inputs).  Every generator is
seeded from the case's position in its table (or from _RESEED), so a case is the same tensor everywhere.  Inputs are finite, except in
DECODE_NONFINITE.  `covers` names the variants (letters of loss_ref.py) a case tells from the right answer; the host test asserts exactly
that set.

Tolerance: LOSS_MARGIN * max(r32, 2**-24) per unit of the reference's scale, r32 = the same error figure of loss_ref.py evaluated in fp32
on the CPU (never the kernel).  Worst err / max(r32, 2**-24) measured on an MI355X over these tables, with the case where it occurred:

    target        tf       1.17 (S32-N63: err 1.19 u, r32 1.02 u)
    dense fwd     lse      1.49 (S416-N2-randn: 1.63 u, 1.09 u)      vals 1.59 (S256-N8-randn: 1.59 u, 0.97 u)
                  out      0.79 (S256-N8-randn: 0.79 u, 0.47 u)
    dense bwd     d_outbox 1.00 (S32-N8-big, upstream 0, scale 0: 1.24 u, 1.24 u)      d_loc 1.00 (S256-N3-dominant, scale 2: 1.00 u, 1.00 u)
                  d_sim    0.64 (S256-N3-dominant: 0.64 u, 0.64 u)   d_negsim 0.64 (S96-N3-big: 0.64 u, 0.64 u)
    contrastive   loss     0.10 (R3-E1024-M16: 0.10 u, 0.37 u)       dq   1.73 (R1027-E4-M1, upstream 100: 1.73 u, 0.66 u)
                  dpos     1.12 (R1027-E4-M1, upstream 100: 2.68 u, 2.40 u)            dneg 0.87 (R4-E252-M10: 0.87 u, 0.84 u)
      on lists    loss     0.02      dq 0.17      dpos 1.32 (interframe: 2.23 u, 1.69 u)      dneg 0.62
    decode        boxes    1.00 (S32-N9-max: 1.17 u, 1.17 u)
    box_iou       iou      0.38 (N64: 0.38 u, 0.38 u)

(u = 2**-24 of the element's scale).  Twice the worst, 1.73, is 3.46, and LOSS_MARGIN, the next integer above, is 4 (cap: the project's 8).
The yardstick uses torch's own fp32 sums; restating it in the kernels' summation order was not needed.  Everything else in the tables
is compared bit for bit: target_i, the dense target (zeros included), cellinfo, and every element whose scale is 0.

GUARD = 2**-18 of the quantity's own scale is the band a decision must clear for fp32 and fp64 to agree on it: the top-2 anchor IoUs,
the distance of gx, gy to an integer, the hinge arguments, the top-2 confidences of the decode.  Planted exact cases (zero-size boxes
whose nine IoUs are all 0, centres on a cell boundary at size 256, the decode's exact ties) are exempt: they are exact in fp32 too.  The
host test enforces the band on the reference alone; seeds that violate it are replaced through _RESEED.  No element and no case is ever
excluded from a comparison.  A hinge argument of exactly 0 is not planted: the kernel's `> 0` and torch's clamp give different
(sub)gradients there, which is unspecified.
"""
import functools
import math
import types
from typing import NamedTuple

import numpy as np
import torch

import loss_ref as LR

F64, F32 = LR.F64, LR.F32
LOSS_MARGIN_CAP = 8.0                        # the project's POST_MARGIN_CAP / HEAD_MARGIN_CAP / SAMPLE_MARGIN_CAP
LOSS_MARGIN = 4.0
assert LOSS_MARGIN <= LOSS_MARGIN_CAP
GUARD = 2.0 ** -18
T32 = float(np.float32(0.07))                # the temperature as the C entry receives it


def loss_tol(r32):
    return LOSS_MARGIN * max(r32, LR.U)


def cap_tol(r32):
    return LOSS_MARGIN_CAP * max(r32, LR.U)


VARIANTS = {
    "a": dict(last_max=True), "b": dict(round_g=True), "c": dict(no_clamp=True), "d": dict(fwd_table=True), "e": dict(cell_swap=True),
    "f": dict(tw_scale0=True),
    "g": dict(conf_sca=True), "h": dict(no_max=True), "i": dict(partner_next=True), "j": dict(neg_partner=True), "k": dict(rank_n=True),
    "l": dict(no_wcoord=True), "m": dict(sig_tw=True),
    "n": dict(no_softmax=True), "o": dict(store_o=True), "p": dict(swap_up=True), "q": dict(no_dsig=True),
    "r": dict(no_eps=True), "s": dict(times_t=True), "t": dict(cut768=True), "u": dict(stride_m1=True), "v": dict(mean_all=True),
    "w": dict(no_proj=True),
    "x": dict(last_max=True), "y": dict(swap_wh=True), "z": dict(stride0=True), "A": dict(full_ext=True),
    "B": dict(no_inter=True), "C": dict(no_clamp=True),
}
STAGE_VARIANTS = dict(target="abcdef", dense="ghijklmnopq", contrastive="rstuvw", decode="xyzA", box_iou="BC")
FWD_KW = ("conf_sca", "no_max", "partner_next", "neg_partner", "rank_n", "no_wcoord", "sig_tw")
BWD_KW = ("no_softmax", "store_o", "swap_up", "no_dsig", "partner_next", "neg_partner")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _seed(case, table, reseed, base):
    return reseed.get(case.name, base + table.index(case))


def _rn(g, *s):
    return torch.randn(*s, generator=g)


def _ru(g, *s):
    return torch.rand(*s, generator=g)


def _pick(var, names):
    return {k: v for k, v in var.items() if k in names}


_RESEED = dict(target={}, dense={}, contrastive={}, decode={}, box_iou={})


def flatten(ref):
    """key -> (value, scale) or exact tensor, with the per-scale lists spread out as key[s]."""
    out = {}
    for k, r in ref.items():
        if isinstance(r, list):
            for s, x in enumerate(r):
                out[f"{k}[{s}]"] = x
        else:
            out[k] = r
    return out


def worst(ref, other):
    """key -> error of `other` against `ref`: per unit of the scale for (value, scale) entries (inf if an exact element differs), 0 / inf
    for exact entries."""
    out = {}
    for k, r in ref.items():
        if isinstance(r, tuple):
            e, exact = LR.err_units(other[k][0], r[0], r[1])
            out[k] = e if exact else float("inf")
        else:
            out[k] = 0.0 if torch.equal(torch.as_tensor(r), torch.as_tensor(other[k])) else float("inf")
    return out


# ---- target / target_dense ---------------------------------------------------------------------------------------------------------------
class TG(NamedTuple):
    name: str
    size: int
    n: int
    first: int              # the planted box the table starts from (the planted boxes, in turn, then random ones)
    covers: str

    def __str__(self):
        return self.name


TG_CASES = [
    TG("S32-N1-point", 32, 1, 12, "ab"),
    TG("S32-N63", 32, 63, 0, "abcdef"),
    TG("S256-N1-boundary", 256, 1, 18, "def"),
    TG("S256-N64", 256, 64, 0, "abcdef"),
    TG("S256-N65", 256, 65, 5, "abcdef"),
    TG("S416-N1-whole", 416, 1, 9, "d"),
    TG("S416-N130", 416, 130, 0, "abcdef"),
    TG("S608-N65", 608, 65, 0, "abcdef"),
    TG("S608-N1-outside", 608, 1, 13, "cd"),
]
TG_EXACT_IOU = ("zero_w", "zero_h", "point")                     # every IoU is 0: an exact nine-way tie
TG_EXACT_FRAC = ("boundary",)                                    # gx, gy integers, exactly


def planted_boxes(size, g):
    """(kind, box) in a fixed order: nine anchor-sized boxes (indices 0-8), the whole image (9), zero width, zero height, a point at the
    far corner (10-12), coordinates outside the image (13, 14), x2 = y2 = size - 1 (15), and at size 256 three integer boxes whose centre
    lies on a cell boundary of the scale they are assigned to (16-18)."""
    S = float(size)
    out = []
    for aw, ah in LR.ANCHORS[::-1]:
        w, h = aw * S / 416.0, ah * S / 416.0
        x = float(_ru(g, 1)) * (S - 1 - w); y = float(_ru(g, 1)) * (S - 1 - h)
        out.append(("anchor", [x, y, x + w, y + h]))
    out.append(("whole", [0.0, 0.0, S - 1, S - 1]))
    out.append(("zero_w", [0.3 * S + 0.37, 0.2 * S + 0.21, 0.3 * S + 0.37, 0.7 * S + 0.13]))
    out.append(("zero_h", [0.1 * S + 0.41, 0.6 * S + 0.29, 0.5 * S + 0.33, 0.6 * S + 0.29]))
    out.append(("point", [S - 1, S - 1, S - 1, S - 1]))
    out.append(("outside", [-20.0, -5.5, S + 30.0, S + 3.0]))
    out.append(("outside", [-10.25, 0.4 * S + 0.3, 0.45 * S + 0.2, S + 10.0]))
    out.append(("far_edge", [S - 1 - 0.31 * S, S - 1 - 0.27 * S, S - 1, S - 1]))
    if size == 256:
        # (x1 + x2) / 2 a multiple of the stride (32, 16, 8) of the scale whose anchor the box matches best
        out.append(("boundary", [24.0, 32.0, 104.0, 96.0]))      # 80 x 64: scale 0 (71 x 55), centre (64, 64)
        out.append(("boundary", [28.0, 20.0, 68.0, 44.0]))       # 40 x 24: scale 1 (38 x 28), centre (48, 32)
        out.append(("boundary", [36.0, 60.0, 44.0, 68.0]))       # 8 x 8: scale 2 (6 x 8), centre (40, 64)
    return out


@functools.lru_cache(maxsize=None)
def target_inputs(case):
    g = _gen(_seed(case, TG_CASES, _RESEED["target"], 30100))
    S = float(case.size)
    planted = planted_boxes(case.size, g)
    kinds, boxes = [], []
    for i in range(case.n):
        j = case.first + i
        if j < len(planted):
            kinds.append(planted[j][0]); boxes.append(planted[j][1])
        else:
            w, h = S * math.exp(float(_rn(g, 1)) * 0.8 - 1.6), S * math.exp(float(_rn(g, 1)) * 0.8 - 1.6)
            x, y = float(_ru(g, 1)) * 0.8 * S, float(_ru(g, 1)) * 0.8 * S          # inside: the clamped box keeps an extent
            kinds.append("random"); boxes.append([x, y, x + w, y + h])
    return types.SimpleNamespace(bbox=torch.tensor(boxes, dtype=F64).to(F32).contiguous(), anchors=LR.scaled_anchors(case.size), kinds=kinds)


@functools.lru_cache(maxsize=None)
def _target_refs(case, dt, var):
    i = target_inputs(case)
    return LR.target(i.bbox, i.anchors, case.size, dt, **dict(var))


def target_refs(case, dt=F64, var={}):
    r = _target_refs(case, dt, tuple(sorted(var.items())))
    return dict(ti=r["ti"], tf=r["tf"])


def target_guard(case):
    r = _target_refs(case, F64, ())
    return r["iou_gap"], r["frac"]


# ---- dense losses ------------------------------------------------------------------------------------------------------------------------
class DN(NamedTuple):
    name: str
    size: int
    n: int
    first: int              # offset into the pool of corner boxes
    regime: str             # "randn", "big" (|logit| in [80, 96]), "dominant" (one logit 60 above the rest), "equal" (all logits equal)
    sat: int                # 0, or 30 / 90: the x, y logits of the positive cell are +-sat
    collide: bool           # sample N-1 gets the box of sample 0
    covers: str

    def __str__(self):
        return self.name


DN_CASES = [
    DN("S32-N1-randn", 32, 1, 0, "randn", 0, False, "jklmnopq"),
    DN("S32-N8-big", 32, 8, 3, "big", 0, False, "hjklmnopq"),
    DN("S32-N2-equal", 32, 2, 20, "equal", 90, False, "jklmnpq"),
    DN("S64-N5-dominant", 64, 5, 8, "dominant", 0, False, "gijklmnopq"),
    DN("S64-N2-sat30", 64, 2, 30, "randn", 30, False, "gjklmnpq"),
    DN("S64-N8-collide", 64, 8, 14, "randn", 0, True, "gijklmnopq"),
    DN("S96-N3-big", 96, 3, 0, "big", 90, False, "ghjklmnopq"),
    DN("S96-N5-collide", 96, 5, 22, "randn", 0, True, "gijklmnopq"),
    DN("S256-N8-randn", 256, 8, 27, "randn", 0, False, "gijklmnpq"),
    DN("S256-N3-dominant", 256, 3, 33, "dominant", 30, False, "gijklmnopq"),
    DN("S256-N2-collide", 256, 2, 5, "equal", 0, True, "jklmnopq"),
    DN("S416-N2-randn", 416, 2, 26, "randn", 0, False, "gjklmnpq"),
]
GUPS = ((1.0, 100.0, 1.0), (0.37, -2.5, 0.0))                    # total_loss's weights; a sign, a fraction and a zero


def corner_boxes(size):
    """36 boxes: for each of the nine anchors (largest first), a box of its size pushed into each corner of the image in turn.  At the
    small sizes they land in the corner cells of their scale."""
    S = float(size)
    out = []
    for aw, ah in LR.ANCHORS[::-1]:
        w, h = aw * S / 416.0, ah * S / 416.0
        for cx, cy in ((0, 0), (1, 0), (0, 1), (1, 1)):
            x, y = cx * (S - 1 - w), cy * (S - 1 - h)
            out.append([x + 0.013 * (1 - 2 * cx), y + 0.011 * (1 - 2 * cy), x + w + 0.013 * (1 - 2 * cx), y + h + 0.011 * (1 - 2 * cy)])
    return out


def _logits(g, regime, n, count):
    """(n, count) logits, pairwise distinct within a sample (a shuffled grid, not draws that may collide in fp32) except in "equal"."""
    if regime == "equal":
        return (_rn(g, n, 1) * 3.0).expand(n, count).clone()
    lo, hi = (80.0, 96.0) if regime == "big" else (-3.0, 3.0)
    x = torch.stack([torch.linspace(lo, hi, count)[torch.randperm(count, generator=g)] for _ in range(n)])
    if regime == "big":
        x = x * (1.0 - 2.0 * (_ru(g, n, count) < 0.5).float())
        x[x.abs() == 96.0] = 96.0                                   # one logit past the overflow of a raw expf, at least
        return x
    x = x * (0.5 + _ru(g, n, 1))
    if regime == "dominant":
        for i in range(n):
            x[i, int(torch.randint(0, count, (1,), generator=g))] = float(x[i].max()) + 60.0
    return x


@functools.lru_cache(maxsize=None)
def dense_inputs(case):
    g = _gen(_seed(case, DN_CASES, _RESEED["dense"], 30400))
    n, size = case.n, case.size
    G, (off, P) = LR.grids(size), LR.offsets(size)
    pool = corner_boxes(size)
    boxes = [pool[(case.first + i) % len(pool)] for i in range(n)]
    if case.collide:
        boxes[n - 1] = boxes[0]
    bbox = torch.tensor(boxes, dtype=F64).to(F32)
    tr = LR.target(bbox, LR.scaled_anchors(size), size)
    ti, tf = tr["ti"], tr["tf"][0].to(F32)
    outbox = [_rn(g, n, 15, x, x) for x in G]
    conf = _logits(g, case.regime, n, 3 * P)
    c0 = 0
    for s, x in enumerate(G):
        outbox[s].view(n, 3, 5, x * x)[:, :, 4] = conf[:, c0:c0 + 3 * x * x].reshape(n, 3, x * x); c0 += 3 * x * x
    lc = _logits(g, case.regime, n, P)
    loc = [lc[:, off[s]:off[s] + x * x].reshape(n, x, x).contiguous() for s, x in enumerate(G)]
    sim = _rn(g, n, P); neg = _rn(g, n, P)
    cell = ti[:, 3].long()
    for i in range(n):
        c, co = int(cell[i]), int(cell[n - 1 - i])
        combo = (i + _seed(case, DN_CASES, {}, 0)) % 4             # hinge 1 on / off, hinge 2 on / off
        pp = float(sim[i, c])
        neg[i, c] = pp - 0.1 + (0.5 if combo & 1 else -0.5) * (1.0 + float(_ru(g, 1)))
        if co != c:
            sim[i, co] = pp - 0.1 + (0.5 if combo & 2 else -0.5) * (1.0 + float(_ru(g, 1)))
        if case.sat:
            s_, a_, gi_, gj_ = int(ti[i, 0]) // 3, int(ti[i, 0]) % 3, int(ti[i, 1]), int(ti[i, 2])
            outbox[s_][i, a_ * 5 + 0, gj_, gi_] = float(case.sat) * (1 if i % 2 == 0 else -1)
            outbox[s_][i, a_ * 5 + 1, gj_, gi_] = float(case.sat) * (-1 if (i // 2) % 2 == 0 else 1)
    split = lambda t: [t[:, off[s]:off[s] + x * x].reshape(n, x, x).contiguous() for s, x in enumerate(G)]
    return types.SimpleNamespace(outbox=[o.contiguous() for o in outbox], sim=split(sim), negsim=split(neg), loc=loc, ti=ti.contiguous(),
                                 tf=tf.contiguous(), bbox=bbox)


def dense_refs(case, dt=F64, var={}, lse=None):
    """Forward, and backward for each of GUPS on `lse` (N,2) float32: the device's own in the GPU test, the fp32-rounded reference
    otherwise."""
    i = dense_inputs(case)
    args = (i.outbox, i.sim, i.negsim, i.loc, i.ti, i.tf)
    f = LR.dense_fwd(*args, case.size, dt, **_pick(var, FWD_KW))
    out = dict(lse=f["lse"], vals=f["vals"], out=f["out"])
    if lse is None:
        lse = LR.dense_fwd(*args, case.size, F64)["lse"][0].to(F32)
    for k, gup in enumerate(GUPS):
        b = LR.dense_bwd(*args, lse, torch.tensor(gup, dtype=F32), case.size, dt, **_pick(var, BWD_KW))
        out.update({f"{key}@{k}": v for key, v in b.items()})
    return flatten(out)


def dense_guard(case):
    i = dense_inputs(case)
    return LR.dense_fwd(i.outbox, i.sim, i.negsim, i.loc, i.ti, i.tf, case.size)["hinge"]


# ---- InfoNCE rows ------------------------------------------------------------------------------------------------------------------------
class CT(NamedTuple):
    name: str
    rows: int
    e: int
    m: int
    plant: str              # per row, from row 0: I pos = q and every negative = pos; N pos = -q; S |q| = 1e-3, |pos| = 1e3, a negative 1e3;
    covers: str             # Z q = 0; z negative 0 = 0; - nothing

    def __str__(self):
        return self.name


CT_CASES = [
    CT("R1-E4-M1", 1, 4, 1, "-", "svw"),
    CT("R1027-E4-M1", 1027, 4, 1, "INSZz", "rsuvw"),
    CT("R3-E8-M5", 3, 8, 5, "IN-", "suvw"),
    CT("R4-E252-M10", 4, 252, 10, "SZz-", "rsuvw"),
    CT("R5-E256-M16", 5, 256, 16, "-----", "suvw"),
    CT("R3-E260-M1", 3, 260, 1, "z-I", "rsuvw"),
    CT("R4-E512-M5", 4, 512, 5, "NS--", "suvw"),
    CT("R5-E764-M10", 5, 764, 10, "-Z-I-", "rsuvw"),
    CT("R3-E768-M16", 3, 768, 16, "---", "suvw"),
    CT("R4-E772-M5", 4, 772, 5, "--S-", "stuvw"),
    CT("R5-E1020-M10", 5, 1020, 10, "I-z--", "rstuvw"),
    CT("R3-E1024-M16", 3, 1024, 16, "NZ-", "rstuvw"),
    CT("R1-E1024-M1", 1, 1024, 1, "-", "stvw"),
]
CT_GUPS = (1.0, 100.0)


@functools.lru_cache(maxsize=None)
def contrastive_inputs(case):
    g = _gen(_seed(case, CT_CASES, _RESEED["contrastive"], 30700))
    R, E, M = case.rows, case.e, case.m
    q, pos, neg = _rn(g, R, E), _rn(g, R, E), _rn(g, R, M, E)
    pos = 0.6 * q + 0.8 * pos                                       # a positive that is one: cos about 0.6
    for r, code in enumerate(case.plant[:R]):
        if code == "I":
            pos[r] = q[r]; neg[r] = pos[r]
        elif code == "N":
            pos[r] = -q[r]
        elif code == "S":
            q[r] *= 1e-3 / float(q[r].norm()); pos[r] *= 1e3 / float(pos[r].norm()); neg[r, 0] *= 1e3 / float(neg[r, 0].norm())
        elif code == "Z":
            q[r] = 0.0
        elif code == "z":
            neg[r, 0] = 0.0
    return types.SimpleNamespace(q=q.contiguous(), pos=pos.contiguous(), neg=neg.contiguous())


def contrastive_refs(case, dt=F64, var={}):
    i = contrastive_inputs(case)
    out = dict(loss=LR.contrastive_fwd(i.q, i.pos, i.neg, T32, dt, **var)["loss"])
    for k, gup in enumerate(CT_GUPS):
        b = LR.contrastive_bwd(i.q, i.pos, i.neg, T32, torch.tensor([gup], dtype=F32), dt, **var)
        out.update({f"{key}@{k}": v for key, v in b.items()})
    return out


# ---- evaluation decode -------------------------------------------------------------------------------------------------------------------
class DC(NamedTuple):
    name: str
    size: int
    n: int
    plant: str              # "max": the maximum planted in scale, anchor (n % 9) and a corner cell in turn;  the ties, see decode_inputs
    covers: str

    def __str__(self):
        return self.name


DC_CASES = [
    DC("S32-N1-max", 32, 1, "max", "Ay"),
    DC("S32-N9-max", 32, 9, "max", "Ayz"),
    DC("S96-N9-max", 96, 9, "max", "Ayz"),
    DC("S256-N3-max", 256, 3, "max", "Ayz"),
    DC("S256-N9-max", 256, 9, "max", "Ayz"),
    DC("S96-N3-tie-thread", 96, 3, "tie_thread", "Axyz"),
    DC("S32-N3-tie-lanes", 32, 3, "tie_lanes", "Axyz"),
    DC("S96-N1-tie-waves", 96, 1, "tie_waves", "Axyz"),
    DC("S256-N3-tie-scales", 256, 3, "tie_scales", "Axyz"),
    DC("S32-N3-all-equal", 32, 3, "all_equal", "Axy"),
    DC("S256-N1-all-equal", 256, 1, "all_equal", "Axy"),
]
DC_TIES = ("tie_thread", "tie_lanes", "tie_waves", "tie_scales", "all_equal")
DECODE_NONFINITE = [                                              # cellinfo only; never run against a kernel without the sentinel fix
    DC("S32-N3-all-ninf", 32, 3, "all_ninf", ""),
    DC("S96-N3-one-nan", 96, 3, "one_nan", ""),
    DC("S96-N3-nan-inf", 96, 3, "nan_inf", ""),
    DC("S256-N1-all-nan", 256, 1, "all_nan", ""),
]


def conf_index(size, j):
    """(scale, channel, cell) of the j-th confidence in the concatenated order scale, anchor, cell."""
    for s, g in enumerate(LR.grids(size)):
        if j < 3 * g * g:
            return s, (j // (g * g)) * 5 + 4, j % (g * g)
        j -= 3 * g * g
    raise IndexError(j)


def _set_conf(outbox, size, n, j, v):
    s, ch, cell = conf_index(size, j)
    outbox[s].view(outbox[s].shape[0], 15, -1)[n, ch, cell] = v


def tie_indices(case, n):
    """The concatenated indices that hold the planted maximum of sample n; the first must win."""
    G, (off, P) = LR.grids(case.size), LR.offsets(case.size)
    if case.plant == "tie_thread":
        j = (5, 255, 3 * P - 257)[n % 3]; return [j, j + 256]
    if case.plant == "tie_lanes":
        j = (0, 17, 3 * P - 2)[n % 3]; return [j, j + 1]
    if case.plant == "tie_waves":
        return [70, 70 + 64, 70 + 128]
    if case.plant == "tie_scales":
        return [(3 * off[1] - 1, 3 * off[1]), (7, 3 * off[2] + 9), (3 * off[1] + 4, 3 * P - 1)][n % 3]
    return []


@functools.lru_cache(maxsize=None)
def decode_inputs(case):
    table = DC_CASES if case in DC_CASES else DECODE_NONFINITE
    g = _gen(_seed(case, table, _RESEED["decode"], 31000 if table is DC_CASES else 31100))
    n, size = case.n, case.size
    G, (off, P) = LR.grids(size), LR.offsets(size)
    outbox = [_rn(g, n, 15, x, x) for x in G]
    expect = None
    if case.plant == "max":
        for i in range(n):
            bn = (i + n) % 9
            s, a, x = bn // 3, bn % 3, G[bn // 3]
            gi, gj = ((0, 0), (x - 1, 0), (0, x - 1), (x - 1, x - 1))[i % 4]
            outbox[s][i, a * 5 + 4, gj, gi] = 6.0 + float(_ru(g, 1))
    elif case.plant == "all_equal":
        for o in outbox:
            o[:, 4::5] = 0.75
    elif case.plant in DC_TIES:
        for i in range(n):
            for j in tie_indices(case, i):
                _set_conf(outbox, size, i, j, 7.5)
    elif case.plant == "all_ninf":
        for o in outbox:
            o[:, 4::5] = float("-inf")
        expect = [0] * n
    elif case.plant == "one_nan":
        expect = [(300, 0, 3 * P - 1)[i % 3] for i in range(n)]
        for i in range(n):
            _set_conf(outbox, size, i, expect[i], float("nan"))
    elif case.plant == "nan_inf":                                  # +inf before and after the NaNs: the first NaN wins all the same
        expect = [(40, 301, 3 * off[2] + 5)[i % 3] for i in range(n)]
        for i in range(n):
            _set_conf(outbox, size, i, 3, float("inf")); _set_conf(outbox, size, i, 3 * P - 2, float("inf"))
            _set_conf(outbox, size, i, expect[i], float("nan")); _set_conf(outbox, size, i, expect[i] + 256, float("nan"))
    elif case.plant == "all_nan":
        for o in outbox:
            o[:, 4::5] = float("nan")
        expect = [0] * n
    else:
        raise KeyError(case.plant)
    return types.SimpleNamespace(outbox=[o.contiguous() for o in outbox], anchors=LR.scaled_anchors(size), expect=expect)


@functools.lru_cache(maxsize=None)
def _decode_refs(case, dt, var):
    i = decode_inputs(case)
    return LR.decode(i.outbox, i.anchors, case.size, dt, **dict(var))


def decode_refs(case, dt=F64, var={}):
    r = _decode_refs(case, dt, tuple(sorted(var.items())))
    return dict(cellinfo=r["cellinfo"], boxes=r["boxes"])


def decode_gap(case):
    return _decode_refs(case, F64, ())["gap"]


# ---- box IoU -----------------------------------------------------------------------------------------------------------------------------
class BI(NamedTuple):
    name: str
    n: int
    first: int
    covers: str

    def __str__(self):
        return self.name


BI_CASES = [BI("N1-nested", 1, 1, "B"), BI("N1-disjoint2", 1, 3, "C"), BI("N64", 64, 0, "BC"), BI("N65", 65, 0, "BC")]
BI_KINDS = ("identical", "nested", "disjoint1", "disjoint2", "touching", "zero_zero", "zero_in")


@functools.lru_cache(maxsize=None)
def box_iou_inputs(case):
    g = _gen(_seed(case, BI_CASES, _RESEED["box_iou"], 31300))
    planted = [([10.3, 20.7, 110.9, 95.2], [10.3, 20.7, 110.9, 95.2]),              # identical
               ([5.5, 6.25, 200.1, 180.3], [50.2, 60.4, 90.8, 100.6]),              # nested
               ([10.1, 10.2, 50.3, 50.4], [70.5, 20.6, 120.7, 45.8]),               # disjoint in x only
               ([10.1, 10.2, 50.3, 50.4], [70.5, 80.6, 120.7, 145.8]),              # disjoint in both axes
               ([10.0, 10.0, 50.0, 50.0], [50.0, 20.0, 90.0, 45.0]),                # touching along an edge
               ([30.5, 40.5, 30.5, 40.5], [30.5, 40.5, 30.5, 40.5]),                # zero area against zero area
               ([30.5, 40.5, 30.5, 90.5], [10.0, 10.0, 100.0, 100.0])]              # zero width inside a box
    b1, b2 = [], []
    for i in range(case.n):
        j = case.first + i
        if j < len(planted):
            b1.append(planted[j][0]); b2.append(planted[j][1])
        else:
            a = _ru(g, 2) * 150.0; b = a + (_ru(g, 2) - 0.5) * 60.0
            wa, wb = 20.0 + _ru(g, 2) * 80.0, 20.0 + _ru(g, 2) * 80.0
            b1.append(torch.cat([a, a + wa]).tolist()); b2.append(torch.cat([b, b + wb]).tolist())
    return types.SimpleNamespace(b1=torch.tensor(b1, dtype=F64).to(F32).contiguous(), b2=torch.tensor(b2, dtype=F64).to(F32).contiguous())


def box_iou_refs(case, dt=F64, var={}):
    i = box_iou_inputs(case)
    return LR.box_iou(i.b1, i.b2, dt, **var)
