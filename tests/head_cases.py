"""Case tables and seeded generators for the kernels of the cross-scale head tail (csrc/head.hip, csrc/locmod.hip), shared by
test_head_ref_host.py (CPU: the cases tell the wrong variants of head_ref.py from the right answer, and no deciding quantity of a
backward sits within rounding of its threshold) and test_head_edges_gpu.py (every kernel against its fp64 reference).  Each entry is
the smallest shape at which the named mechanism can still go wrong.  Inputs are computed once per case and must not be modified.

Tolerance: HEAD_MARGIN * max(r32, 2**-24) per unit of the reference's scale, r32 = the same error figure of head_ref.py evaluated in
fp32 on the CPU at run time (the scheme of post_cases.py).  Measured worst err / max(r32, 2**-24) per kernel on an MI355X over the
tables below (HEADFIG lines of test_head_edges_gpu.py):
  locemb_fwd_kernel       2.00 (P3-B2-train rv: 3.77 against 1.89 units of 2**-24 of the update-sized scale; E8, x-hat, stat below 1.5)
  locemb_bwd_kernel       1.36 (P3-B2-train, dEa alone)
  head_obj_kernel         1.32 (P255-B5-mixed X, at the floor; 1.20 at P1023 with a yardstick of its own)
  locbn_fwd_kernel        1.00    locbn_bwd_kernel     1.00 (both compute in fp64: the fp32 stores are all that rounds)
  locmod_fwd_kernel       0.26    locmod_bwd + reduce  1.05 (P64-n3-zero dsum)
  head_final_fwd_kernel   1.23 (P1023-B2-ld32-tielane outbox0, at the floor; 1.14 at P8161)
  head_dloc_kernel        1.05    head_fold_kernel     1.03    head_dlogits_kernel  1.39 (P256-B1-ld32 all, dsim2)
  colsum_kernel           1.00    pad_rows_kernel      exact
The margin is the next integer above twice the worst of them, below the 8 at which it would be capped.
The fp64 moments (mom, dmom) are compared at MOM_MARGIN * 2**-53 per unit of their scale.  Measured worst: mom 1.96 (P1025-B5-train; 1.74 at
P = 8192) against the correctly rounded sums of head_ref.moments_exact; dmom 3.62 (B1-P3-train, 0.15 and less from P = 257 on) against
plain float64 sums.  MOM_MARGIN is the next integer above twice the worst.

Guard band.  A backward that depends on a ReLU mask agrees between the fp32 kernel and the fp64 reference only if no pre-activation
sits within rounding of zero: GUARD = 2**-18 of the pre-activation's own sum of absolute terms (64 fp32 roundings of it).  The host
test asserts that no element of a backward case is inside the band except the planted exact zeros, which are exact in fp32 too, and
that apart from planted ties the runner-up minimum and maximum of every loc_map are further than the band from the extremes.  Seeds
that put an element inside the band are replaced through the _RESEED tables; no element is ever excluded from a comparison.
"""
import collections
import functools
import types

import torch

import head_ref as HR

HEAD_MARGIN_CAP = 8.0                        # the project's POST_MARGIN_CAP
HEAD_MARGIN = 5.0
MOM_MARGIN = 8.0
assert HEAD_MARGIN <= HEAD_MARGIN_CAP
GUARD = 2.0 ** -18
MOMENTUM = 0.10000000149011612               # float32(0.1), float32(1e-5): what the kernels receive
EPS = 9.999999747378752e-06


def head_tol(r32):
    return HEAD_MARGIN * max(r32, HR.U)


def cap_tol(r32):
    return HEAD_MARGIN_CAP * max(r32, HR.U)


def _seed(case, table, reseed, base):
    return reseed.get(case.name, base + 31 * table.index(case))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def _rand(g, *shape):
    return torch.rand(*shape, generator=g)


def e8_rows(g, P):
    """Rows like the location embedding's: non-negative, unit norm, about half of the entries exactly 0."""
    z = torch.relu(_randn(g, P, 8)); z[:, 0] += 0.1
    return (z / z.norm(dim=1, keepdim=True)).float()


# ---- the kernels over three scales --------------------------------------------------------------------------------------------------
# scales: (H, W, ld) per scale, coarsest first; P = sum H W; head_obj pads to Ppad = 32 ceil(P / 32) <= 8192.
#   P = 3 one position per scale; 255 / 256 / 257 around the 256-thread stride of locemb and head_obj; 1023 / 1024 / 1025 / 2049 around
#   the 1024-thread trips of head_final_fwd, block_minmax and head_dloc; 8161 (Ppad = 8192) and 8192 fill head_obj's register bank.
# plant:  sim0       image 0 has sim == 0 everywhere: objn == 0, the 1e-12 clamp, obj_map == X == 0
#         tie-lane   exact ties of min and max in two lanes of one wave          tie-wave   in two waves of the first trip
#         tie-trip   at p and p + 1024 (one thread, two trips)                   tie-scale  in two different scales
#         const      image 0 has a constant loc_map (min == max, argmin == argmax == 0, the 1e-6 alone is the denominator)
# covers: the wrong variants of head_ref.py (letters of VARIANTS below) that change this case's answer by more than the largest tolerance the
# margin cap allows.  (f), the missing 1e-6, is 1e-6 / (max - min) of a value: past eight roundings only where the range is small (P = 3)
# or zero ("const").
TailCase = collections.namedtuple("TailCase", "name B scales plant covers")
TailCase.__str__ = lambda c: c.name
TAIL_CASES = [TailCase(*c) for c in (
    ("P3-B2-ld15", 2, ((1, 1, 15), (1, 1, 15), (1, 1, 15)), "-", "fhijkmop"),
    ("P255-B5-mixed", 5, ((3, 5, 15), (6, 8, 32), (12, 16, 16)), "-", "hijkmopq"),
    ("P256-B1-ld32", 1, ((1, 16, 32), (6, 8, 32), (12, 16, 32)), "-", "hijkmoq"),
    ("P257-B2-ld15-sim0", 2, ((1, 17, 15), (6, 8, 15), (12, 16, 15)), "sim0", "hijkmop"),
    ("P1023-B2-ld32-tielane", 2, ((3, 11, 32), (6, 30, 32), (27, 30, 32)), "tie-lane", "ghijkmopq"),
    ("P1024-B2-mixed-tiewave", 2, ((2, 17, 32), (6, 30, 15), (27, 30, 17)), "tie-wave", "ghijkmoq"),
    ("P1025-B5-ld15-tietrip", 5, ((5, 7, 15), (6, 30, 15), (27, 30, 15)), "tie-trip", "ghijkmop"),
    ("P2049-B2-ld32-tiescale", 2, ((3, 43, 32), (16, 40, 32), (32, 40, 32)), "tie-scale", "ghijkmopq"),
    ("P8161-B2-mixed-const", 2, ((13, 37, 15), (32, 48, 32), (64, 96, 20)), "const", "fghijkmopq"),
    ("P8192-B2-ld15", 2, ((16, 32, 15), (32, 48, 15), (64, 96, 15)), "-", "hijkmo"),
)]
# the tie positions of each plant: (minimum at, maximum at), first occurrence first
TIES = {"tie-lane": ((5, 9), (17, 40)), "tie-wave": ((70, 700), (3, 1000)), "tie-trip": ((0, 1024), (1, 1)),
        "tie-scale": ((100, 1500), (50, 400))}
# which output gradients reach the backward: all nine; training (only_obj is not in the loss); d_outbox alone (an eval-mode backward);
# one scale's d_outbox missing; and everything but no dobj_map
GRAD_SETS = ("all", "train", "outbox", "scale1-null", "no-dobj")
_TAIL_RESEED = {}


def geometry(case):
    hws = [h * w for h, w, _ in case.scales]
    P = sum(hws)
    return hws, P, (P + 31) // 32 * 32


@functools.lru_cache(maxsize=None)
def tail_inputs(case):
    g = _gen(_seed(case, TAIL_CASES, _TAIL_RESEED, 9100))
    B = case.B
    hws, P, Ppad = geometry(case)
    ns = types.SimpleNamespace(hws=hws, P=P, Ppad=Ppad)
    ns.logits = [_randn(g, B, h, w, ld) for h, w, ld in case.scales]                 # the pad channels hold data too: never read
    ns.sims = [0.5 * _randn(g, B, h * w) for h, w, _ in case.scales]
    if case.plant == "sim0":
        for s in ns.sims:
            s[0] = 0.0
    ns.e8 = e8_rows(g, P)
    x = _randn(g, B, P)
    if case.plant in TIES:
        (a0, a1), (b0, b1) = TIES[case.plant]
        x = x.clamp(-3.0, 3.0)
        x[:, a0] = -3.5; x[:, a1] = -3.5; x[:, b0] = 3.25; x[:, b1] = 3.25
    elif case.plant == "const":
        x[0] = 0.375
    ns.loc_map = x
    ns.d_outbox = [_randn(g, B, 15, hw) for hw in hws]
    ns.d_loc = [_randn(g, B, hw) for hw in hws]
    ns.d_only = [_randn(g, B, hw) for hw in hws]
    ns.dX = _randn(g, B * 8, Ppad)
    ns.dobj_map = _randn(g, B, P)
    return ns


def grad_args(case, which):
    """(d_outbox, d_loc, d_only, dobj_map) of a gradient argument set; None stands for a NULL pointer."""
    i = tail_inputs(case)
    none = [None, None, None]
    if which == "all":
        return i.d_outbox, i.d_loc, i.d_only, i.dobj_map
    if which == "train":
        return i.d_outbox, i.d_loc, none, i.dobj_map
    if which == "outbox":
        return i.d_outbox, none, none, i.dobj_map
    if which == "scale1-null":
        return [i.d_outbox[0], None, i.d_outbox[2]], i.d_loc, none, i.dobj_map
    if which == "no-dobj":
        return i.d_outbox, i.d_loc, i.d_only, None
    raise KeyError(which)


# geometries that must raise ops.DcnError with nothing launched
BAD_GEOMETRY = {"Ppad > 8192": ((19, 27, 15), (32, 48, 15), (64, 96, 15)), "ld = 14": ((1, 1, 15), (1, 1, 14), (1, 1, 15))}


# ---- location embedding ----------------------------------------------------------------------------------------------------------
# plant:  deadrow   beta < 0 everywhere and one row of coord at the mean of the others: its eight BatchNorm outputs are all <= 0, its
#                   E8 row is 0 (ss == 0, the 1e-12 clamp)
#         const     coord column 6 constant (as the model's 1 / height map is) and row 2 of W zero elsewhere: channel 2 of the Linear has
#                   zero variance (the var > 0 ? var : 0 clamp), x-hat is exactly 0 on the device, and with beta[2] = 0 the BatchNorm
#                   output is an exact 0 in every row: the ReLU mask's boundary
LocembCase = collections.namedtuple("LocembCase", "name P B training plant bwd covers")
LocembCase.__str__ = lambda c: c.name
LOCEMB_CASES = [LocembCase(*c) for c in (
    ("P3-B2-train", 3, 2, True, "-", True, "ab"),
    ("P255-B5-eval", 255, 5, False, "-", True, ""),
    ("P256-B1-train-const", 256, 1, True, "const", True, "al"),
    ("P257-B2-train-deadrow", 257, 2, True, "deadrow", True, "ab"),
    ("P257-B2-eval-deadrow", 257, 2, False, "deadrow", True, ""),
    ("P1025-B5-train", 1025, 5, True, "-", True, "ab"),
    ("P8192-B2-train", 8192, 2, True, "-", False, "ab"),
)]
_LOCEMB_RESEED = {}
CONST_COL, CONST_CH = 6, 2


@functools.lru_cache(maxsize=None)
def locemb_inputs(case):
    g = _gen(_seed(case, LOCEMB_CASES, _LOCEMB_RESEED, 9400))
    P = case.P
    ns = types.SimpleNamespace(count=case.B * P)
    ns.coord = 2.0 * _rand(g, P, 8) - 1.0
    ns.W = 0.6 * _randn(g, 8, 8); ns.b = 0.1 * _randn(g, 8)
    ns.gamma = 1.0 + 0.2 * _randn(g, 8); ns.beta = 0.3 * _randn(g, 8)
    if case.plant == "const":
        ns.coord[:, CONST_COL] = 0.25
        ns.W[CONST_CH] = 0.0; ns.W[CONST_CH, CONST_COL] = 0.75
        ns.beta[CONST_CH] = 0.0
    if case.plant == "deadrow":
        ns.beta = -0.2 - 0.3 * _rand(g, 8)
        ns.dead = P // 2
        ns.coord[ns.dead] = (ns.coord.double().sum(0) - ns.coord[ns.dead].double()).div(P - 1).float()
    # running statistics sized so that the retained part (1 - momentum) * old never exceeds the update: the comparison of the updated
    # statistics is then relative to the update term within a factor of two
    ce = ns.coord.double() @ ns.W.double().t() + ns.b.double()
    mean, var = ce.mean(0), ce.var(0, unbiased=False)
    if case.training:
        ns.rm = (mean * (0.02 + 0.08 * _rand(g, 8).double())).float()
        ns.rv = (var * (0.02 + 0.08 * _rand(g, 8).double())).float()
        ns.rv[var < 1e-20] = 2.0 ** -10                                   # (a zero-variance channel: the retained part is all there is)
    else:
        ns.rm = (mean + 0.05 * _randn(g, 8).double()).float() if case.plant != "deadrow" else mean.float()
        ns.rv = (var * (0.5 + _rand(g, 8).double())).float() + 1e-3
    ns.dEa = _randn(g, P, 8); ns.dEb = _randn(g, P, 8)
    ns.dmom = _randn(g, 72).double() / P
    return ns


def locemb_bwd_xh(case, xh):
    """The x-hat a backward case is run on: the forward's, with the "const" plant's channel set to the exact 0 the device produces
    (every row's fp32 Linear output equals the fp64 batch mean there; a float64 forward leaves rounding dust instead)."""
    xh = xh.detach().float().clone()
    if case.plant == "const":
        xh[:, CONST_CH] = 0.0
    return xh


# ---- BatchNorm1d(512) from the moments -------------------------------------------------------------------------------------------------
# plant: zerocol  column 7 of M is zero across the batch: t1 == q2 == var == 0 (the clamp), r = 1 / sqrt(eps)
LocbnCase = collections.namedtuple("LocbnCase", "name B P training plant covers")
LocbnCase.__str__ = lambda c: c.name
LOCBN_CASES = [LocbnCase(*c) for c in (
    ("B1-P3-train", 1, 3, True, "-", "ce"),
    ("B2-P257-train-zerocol", 2, 257, True, "zerocol", "cde"),
    ("B5-P1025-train", 5, 1025, True, "-", "cde"),
    ("B2-P8192-train", 2, 8192, True, "-", "cde"),
    ("B1-P255-eval", 1, 255, False, "-", "n"),
    ("B5-P64-eval-zerocol", 5, 64, False, "zerocol", "n"),
)]
_LOCBN_RESEED = {}
ZERO_COL = 7


@functools.lru_cache(maxsize=None)
def locbn_inputs(case):
    g = _gen(_seed(case, LOCBN_CASES, _LOCBN_RESEED, 9700))
    B = case.B
    ns = types.SimpleNamespace(count=B * case.P)
    ns.mom = HR.moments(e8_rows(g, case.P))[0]
    ns.M = 0.1 * _randn(g, B, 8, 512)
    if case.plant == "zerocol":
        ns.M[:, :, ZERO_COL] = 0.0
    ns.b = 0.1 * _randn(g, 512); ns.gamma = 1.0 + 0.2 * _randn(g, 512); ns.beta = 0.2 * _randn(g, 512)
    r = HR.locbn_fwd(ns.M, ns.mom, ns.b, ns.gamma, ns.beta, torch.zeros(512), torch.ones(512), True, ns.count, MOMENTUM, EPS)
    mu_b = r["saved"][0][1] + ns.b.double()
    var = (r["rv"][0] - (1.0 - MOMENTUM)) / MOMENTUM
    if case.training:
        ns.rm = (mu_b * (0.02 + 0.08 * _rand(g, 512).double())).float()
        ns.rv = (var * (0.02 + 0.08 * _rand(g, 512).double())).float()
        ns.rv[var == 0] = 2.0 ** -10
    else:
        ns.rm = (mu_b + 0.02 * _randn(g, 512).double()).float()
        ns.rv = (var * (0.5 + _rand(g, 512).double())).float() + 1e-4
    ns.dsum = _randn(g, B, 10, 512)                                       # dMp is the strided view [:, :8] of it, or a contiguous copy
    ns.dbp = _randn(g, 512)
    return ns


# ---- location module core ------------------------------------------------------------------------------------------------------------
# 16 rows per wave, 64 per workgroup: P = 1; 15 / 16 / 17 around a wave's rows; 63 / 64 / 65 around a workgroup's; 130 = three chunks for
# the reduce kernel; 3549 (the 416 x 416 model's P) forward only.  The backward cases keep n P 512 <= 1.3e5 so that guard-band-free seeds
# exist.
# plant:  dead   b' < 0 everywhere; image 0 has M' == 0, so every row of it is dead (ss == 0, the 1e-12 clamp, loc == 0), and rows 0 and
#                P - 1 of E are 0: dead in every image
#         zero   row 1 of E is 0 and b'[5] = b'[300] = 0: two pre-activations of that row are exact zeros, the ReLU mask's boundary
LocmodCase = collections.namedtuple("LocmodCase", "name P n plant bwd covers")
LocmodCase.__str__ = lambda c: c.name
LOCMOD_CASES = [LocmodCase(*c) for c in (
    ("P1-n1", 1, 1, "-", True, ""),
    ("P15-n3", 15, 3, "-", True, ""),
    ("P16-n1-zero", 16, 1, "zero", True, "l"),
    ("P17-n3-dead", 17, 3, "dead", True, ""),
    ("P63-n1", 63, 1, "-", True, ""),
    ("P64-n3-zero", 64, 3, "zero", True, "l"),
    ("P65-n3", 65, 3, "-", True, ""),
    ("P130-n1", 130, 1, "-", True, ""),
    ("P3549-n2", 3549, 2, "-", False, ""),
)]
# inputs redrawn where a pre-activation fell inside the guard band
_LOCMOD_RESEED = {"P64-n3-zero": 10300}
ZERO_ROW, ZERO_CH = 1, (5, 300)


@functools.lru_cache(maxsize=None)
def locmod_inputs(case):
    g = _gen(_seed(case, LOCMOD_CASES, _LOCMOD_RESEED, 10000))
    P, n = case.P, case.n
    ns = types.SimpleNamespace()
    ns.E = e8_rows(g, P)
    ns.Mp = 0.3 * _randn(g, n, 8, 512); ns.bp = 0.2 * _randn(g, 512)
    ns.q = torch.nn.functional.normalize(_randn(g, n, 512), dim=1)
    ns.dloc = _randn(g, n, P)
    if case.plant == "dead":
        ns.bp = -0.05 - ns.bp.abs()
        ns.Mp[0] = 0.0
        ns.E[0] = 0.0; ns.E[P - 1] = 0.0
    if case.plant == "zero":
        ns.E[ZERO_ROW] = 0.0
        for c in ZERO_CH:
            ns.bp[c] = 0.0
    return ns


# ---- compositions shared by the host and the GPU tests ------------------------------------------------------------------------------
# the wrong variants: letter -> {stage: keyword arguments of that stage's reference}
VARIANTS = {
    "a": {"locemb_fwd": dict(biased=True)}, "b": {"locemb_fwd": dict(count_p=True)},
    "c": {"locbn_fwd": dict(biased=True)}, "d": {"locbn_fwd": dict(count_p=True)}, "e": {"locbn_fwd": dict(no_bias_rm=True)},
    "n": {"locbn_fwd": dict(no_bscale=True)},
    "f": {"final": dict(no_eps=True), "dloc": dict(no_eps=True)}, "g": {"final": dict(tie="last")},
    "h": {"dloc": dict(drop="min")}, "o": {"dloc": dict(drop="max")}, "i": {"dloc": dict(misplace=True)},
    "j": {"obj": dict(div3=False), "dlogits": dict(div3=False)}, "k": {"final": dict(box_mod=True), "dlogits": dict(box_mod=True)},
    "m": {s: dict(swap=True) for s in ("final", "dloc", "obj", "dlogits")},
    "p": {"obj": dict(pad_nonzero=True)}, "q": {"dlogits": dict(pad_nonzero=True)},
    "l": {"locemb_bwd": dict(mask_ge=True), "locmod_bwd": dict(mask_ge=True)},
}


def tail_forward_refs(case, dt=HR.F64, var={}):
    i = tail_inputs(case)
    return dict(obj=HR.head_obj(i.logits, i.sims, i.e8, dt, **var.get("obj", {})),
                final=HR.head_final_fwd(i.logits, i.sims, i.loc_map, dt, **var.get("final", {})))


@functools.lru_cache(maxsize=None)
def tail_forward_standins(case):
    """What the backward kernels receive from the forward, as float32: from the float64 reference here; the GPU test passes the device's
    own outputs in the same namespace instead."""
    r = tail_forward_refs(case)
    f = lambda t: t.float()
    return types.SimpleNamespace(loc=[f(r["final"][f"loc{s}"][0]) for s in range(3)], mm=f(r["final"]["mm"][0]), imn=r["final"]["imn"],
                                 imx=r["final"]["imx"], only=[f(r["obj"][f"only{s}"][0]) for s in range(3)], obj_map=f(r["obj"]["obj_map"][0]),
                                 objn=f(r["obj"]["objn"][0]))


def tail_backward_refs(case, which, fwd=None, dt=HR.F64, var={}):
    i = tail_inputs(case)
    fwd = fwd or tail_forward_standins(case)
    d_outbox, d_loc, d_only, dobj = grad_args(case, which)
    return dict(dloc=HR.head_dloc(i.logits, i.sims, fwd.loc, d_outbox, d_loc, fwd.mm, fwd.imn, fwd.imx, dt, **var.get("dloc", {})),
                fold=HR.head_fold(i.dX, i.e8, fwd.obj_map, dt),
                dlogits=HR.head_dlogits(i.logits, i.sims, fwd.loc, fwd.only, d_outbox, d_only, fwd.obj_map, fwd.objn, dobj, dt,
                                        **var.get("dlogits", {})))


def locemb_refs(case, fwd=None, dt=HR.F64, var={}, args="full"):
    """fwd: (xh, stat) float32 as the backward receives them (default: the float64 forward's).  args: "full" (dEa, dEb, dmom; dmom only in
    train mode, as in the model) or "dEa" (dEb and dmom NULL)."""
    i = locemb_inputs(case)
    out = dict(locemb_fwd=HR.locemb_fwd(i.coord, i.W, i.b, i.gamma, i.beta, i.rm, i.rv, case.training, i.count, MOMENTUM, EPS, dt,
                                        **var.get("locemb_fwd", {})))
    if case.bwd:
        if fwd is None:
            base = out["locemb_fwd"] if dt == HR.F64 and not var else locemb_refs(case)["locemb_fwd"]
            fwd = (base["xh"][0], base["stat"][0].float())
        dEb, dmom = (i.dEb, i.dmom if case.training else None) if args == "full" else (None, None)
        out["locemb_bwd"] = HR.locemb_bwd(i.coord, i.W, i.gamma, i.beta, locemb_bwd_xh(case, fwd[0]), fwd[1], i.dEa, dEb, dmom, case.training, dt,
                                          **var.get("locemb_bwd", {}))
    return out


def locbn_refs(case, saved=None, dt=HR.F64, var={}):
    i = locbn_inputs(case)
    out = dict(locbn_fwd=HR.locbn_fwd(i.M, i.mom, i.b, i.gamma, i.beta, i.rm, i.rv, case.training, i.count, MOMENTUM, EPS, dt,
                                      **var.get("locbn_fwd", {})))
    if saved is None:
        saved = (out["locbn_fwd"] if dt == HR.F64 and not var else locbn_refs(case)["locbn_fwd"])["saved"][0].float()
    out["locbn_bwd"] = HR.locbn_bwd(i.M, i.mom, i.b, i.gamma, i.rm, saved, i.dsum[:, :8], i.dbp, case.training, i.count, dt)
    return out


def locmod_refs(case, dt=HR.F64, var={}):
    i = locmod_inputs(case)
    out = dict(locmod_fwd=HR.locmod_fwd(i.E, i.Mp, i.bp, i.q, dt))
    if case.bwd:
        out["locmod_bwd"] = HR.locmod_bwd(i.E, i.Mp, i.bp, i.q, i.dloc, dt, **var.get("locmod_bwd", {}))
    return out


GUARD_KEYS = ("y", "v")                      # pre-activations returned for the guard band only: not outputs of a kernel


def worst(ref, other):
    """Over the stages and keys of two results of the same composition: the largest error of `other` in units of ref's scale (inf where
    an exact element, an index or a non-finite value differs), as {(stage, key): error}."""
    out = {}
    for st in ref:
        for k, r in ref[st].items():
            if k in GUARD_KEYS:
                continue
            if isinstance(r, tuple):
                e, exact = HR.err_units(other[st][k][0], r[0], r[1])
                out[st, k] = e if exact else float("inf")
            else:
                out[st, k] = 0.0 if torch.equal(r, other[st][k]) else float("inf")
    return out
