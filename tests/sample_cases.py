"""Case tables for the kernels of dcnet_amd/csrc/sample.hip, shared by tests/test_sample_ref_host.py (CPU: the cases tell the wrong
variants of tests/sample_ref.py apart) and tests/test_sample_edges_gpu.py (the kernels against the references on the same inputs).
Every generator is seeded from the case's position in its table (or from _RESEED), so a case is the same tensor everywhere.  Inputs are
finite and free of NaN throughout: the selection kernel's order of NaNs and infinities is not specified and not tested.  `hw` is a plain
number of positions, square or not.  `covers` names the variants (letters of sample_ref.py) a case tells from the right answer; the host
test asserts exactly that set.

Tolerance: SAMPLE_MARGIN * max(r32, 2**-24) per unit of the reference's scale, r32 = the same error figure of sample_ref.py evaluated
in fp32 on the CPU (never the kernel).  Worst err / max(r32, 2**-24) measured on an MI355X over these tables:

    colnorm_fwd   vit   1.19 (N3-HW37-E64: err 1.19 u, r32 0.94 u)     cnorm 1.18 (N3-HW61-E100: 1.30 u, 1.10 u)
    colnorm_bwd   dv    1.40 (N3-HW61-E100: 2.25 u, 1.61 u)
    lagnorm_fwd   lag   1.35 (N2-L32-E300: 1.53 u, 1.14 u)        lnorm 1.19 (N3-L20-E256: 1.59 u, 1.34 u)
    crossmap      lvmap 1.00 (L32-HW413-E4: 8.11 u, 8.11 u; L4-HW1030-E8: 2.95 u, 2.95 u)
    k14_dlag      dctx  1.37 (N1-L32-HW9-E4: 1.66 u, 1.21 u)

(u = 2**-24 of the element's scale).  Twice the worst, 1.40, is 2.80, and SAMPLE_MARGIN, the next integer above, is 3 (cap: the project's 8).
The yardstick of lvmap adds the 3 L + 1 terms of the convolution one after another, as any plain fp32 evaluation does; against a blocked
einsum (r32 1.36 u) the same kernel error of 8.11 u at L = 32 read 5.95.  Everything else in the tables is compared
bit for bit: indices, gathers, cols (no column is excluded), the sampler's tables, and the sums of k9_bwd / k14_negscatter against
fp32 sums added one term at a time in the documented order.

GUARD = 2**-18 (64 fp32 roundings of the scale) is the band a column's fp64 top-2 gap must clear for `cols` to be compared exactly; the host
test enforces it on the reference alone and seeds that violate it are replaced through _RESEED.
"""
import functools
import types
from typing import NamedTuple

import numpy as np
import torch

import sample_ref as SR

F64, F32 = SR.F64, SR.F32
SAMPLE_MARGIN_CAP = 8.0                      # the project's POST_MARGIN_CAP / HEAD_MARGIN_CAP
SAMPLE_MARGIN = 3.0
assert SAMPLE_MARGIN <= SAMPLE_MARGIN_CAP
GUARD = 2.0 ** -18


def sample_tol(r32):
    return SAMPLE_MARGIN * max(r32, SR.U)


def cap_tol(r32):
    return SAMPLE_MARGIN_CAP * max(r32, SR.U)


VARIANTS = {
    "a": dict(tie_high=True), "b": dict(equal_desc=True), "c": dict(raw_bits=True), "d": dict(swap_qk=True), "e": dict(no_skip=True),
    "f": dict(skip_gt=True), "g": dict(neg_frame1=True),
    "h": dict(over_channels=True), "i": dict(odd=True), "j": dict(no_eps=True),
    "k": dict(taps_rev=True), "l": dict(w_t=True), "m": dict(no_pad=True), "n": dict(no_bias=True), "o": dict(last_max=True),
    "p": dict(own_image=True), "q": dict(extra_all=True), "r": dict(extra_img0=True), "s": dict(no_proj=True), "t": dict(no_proj=True),
    "u": dict(bits_pm1=True), "v": dict(no_shift=True), "w": dict(no_hi_id=True), "x": dict(step_lo=True),
}
STAGE_VARIANTS = dict(k9="abcdefg", colnorm="hjqrs", lagnorm="hij", crossmap="klmno", gather="p", dlag="jt", sampler="uvwx")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _seed(case, table, reseed, base):
    return reseed.get(case.name, base + table.index(case))


def _rn(g, *s):
    return torch.randn(*s, generator=g)


_RESEED = dict(k9={}, colnorm={}, lagnorm={}, crossmap={}, gather={}, negscatter={}, dlag={}, k9_bwd={})


def worst(ref, other):
    """key -> error of `other` against `ref`: per unit of the scale for (value, scale) entries (inf if an exact element differs), 0 / inf
    for exact entries."""
    out = {}
    for k, r in ref.items():
        if isinstance(r, tuple):
            e, exact = SR.err_units(other[k][0], r[0], r[1])
            out[k] = e if exact else float("inf")
        else:
            out[k] = 0.0 if torch.equal(torch.as_tensor(r), torch.as_tensor(other[k])) else float("inf")
    return out


# ---- K9 select --------------------------------------------------------------------------------------------------------------------------
class K9(NamedTuple):
    name: str
    pairs: int
    hw: int
    e: int
    top_k: int
    neg_n: int
    kind: str
    covers: str

    def __str__(self):
        return self.name


K9_CASES = [
    K9("n4-topn", 1, 2, 4, 4, 1, "mixed4", "cdefg"),           # top_k = n: everything selected, k in {0, HW-1}, neg_n = HW-1
    K9("n4-top1", 1, 2, 4, 1, 0, "rand", "c"),
    K9("n1024-p3", 3, 32, 260, 30, 1, "rand", "cdefg"),         # three different pairs, second trip of the row copy
    K9("n1089-span", 1, 33, 4, 30, 1, "plateau_span", "abcdefg"),   # segments of 2, ties over 75 threads, cut inside a segment
    K9("n2116-inseg", 1, 46, 4, 30, 0, "plateau_in", "acd"),   # segments of 3, a plateau inside one segment, longer than krem
    K9("n1089-equal-k64", 1, 33, 4, 64, 1, "all_equal", "abdefg"),
    K9("n1024-neg-k64", 1, 32, 4, 64, 1, "all_neg", "cdefg"),
    K9("n1089-mixed-k64", 1, 33, 512, 64, 1, "mixed", "cdefg"),
    K9("n1024-bits16", 1, 32, 4, 30, 0, "bits16", "bd"),         # the first two digits shared by every element
    K9("n1024-lowbyte0", 1, 32, 4, 30, 0, "lowbyte0", "d"),     # the threshold's key ends in 0x00: the d == 0 fall-through
    K9("n1089-zeros", 1, 33, 4, 30, 0, "signed_zero", "acd"),  # -0.0 (lower index) and +0.0 at the threshold
    K9("n81-negall", 2, 9, 260, 30, 8, "rand", "cdefg"),        # neg_n = HW-1: every raw position against every k
]


def _bits_to_f32(bits):
    return torch.from_numpy(np.asarray(bits, np.uint32).view(np.float32).copy())


def _cmap_row(kind, hw, top_k, g):
    n = hw * hw
    below = -_rn(g, n).abs() - 0.1
    perm = torch.randperm(n, generator=g)
    if kind == "rand":
        x = _rn(g, n)
        if hw >= 8:                                             # selected entries with k == 0, k == HW-1, k == HW-2
            x[5 * hw] = 9.0; x[6 * hw + hw - 1] = 8.5; x[2 * hw + hw - 2] = 8.0
        return x
    if kind == "mixed4":
        return torch.tensor([-1.5, 0.5, -0.25, 2.0])
    if kind == "plateau_span":
        x = below - 1.0
        x[perm[perm >= 400][:top_k - 9]] = 1.0 + torch.rand(top_k - 9, generator=g)
        x[50:200] = 0.5                                        # krem = 7: 50..56, the cut falls on the first element of segment (56, 57)
        x[9 * hw] = 7.0; x[10 * hw + hw - 1] = 6.0             # k == 0 and k == HW-1 above the plateau
        return x
    if kind == "plateau_in":
        x = below.clone()
        x[perm[perm >= 400][:top_k - 1]] = 1.0 + torch.rand(top_k - 1, generator=g)
        x[301] = 0.5; x[302] = 0.5                             # segment 100 is (300, 301, 302); krem = 1
        return x
    if kind == "all_equal":
        return torch.full((n,), 0.25)
    if kind == "all_neg":
        x = below.clone()
        x[5 * hw] = -0.001; x[6 * hw + hw - 1] = -0.002
        return x
    if kind == "mixed":
        x = below.clone()
        x[perm[:20]] = _rn(g, 20).abs() + 0.1
        return x
    if kind == "bits16":
        return _bits_to_f32(0x3F800000 + torch.randint(0, 65536, (n,), generator=g).numpy().astype(np.int64))
    if kind == "lowbyte0":
        x = 0.5 * torch.rand(n, generator=g)
        top = perm[:top_k]
        x[top[:top_k - 6]] = 2.0 + torch.rand(top_k - 6, generator=g)
        x[top[top_k - 6:top_k - 1]] = _bits_to_f32([0x3F800001 + i for i in range(5)])
        x[top[top_k - 1]] = 1.0                                # bits 0x3F800000
        return x
    if kind == "signed_zero":
        x = below.clone()
        x[perm[perm >= 100][:top_k - 1]] = 1.0 + torch.rand(top_k - 1, generator=g)
        x[10] = -0.0; x[20] = 0.0; x[21] = 0.0                 # krem = 1: index 10, the -0.0
        return x
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def k9_inputs(case):
    g = _gen(_seed(case, K9_CASES, _RESEED["k9"], 20100))
    hw, top_k, m = case.hw, case.top_k, case.neg_n
    cmap = torch.stack([_cmap_row(case.kind, hw, top_k, g) for _ in range(case.pairs)]).contiguous()
    fv = _rn(g, 2 * case.pairs, hw, case.e)
    raw = torch.zeros(case.pairs, top_k, m, dtype=torch.int64)
    for b in range(case.pairs):
        k = SR.select(cmap[b].numpy(), top_k) % hw
        for j in range(top_k):
            if m == hw - 1:                                     # every raw position 0..HW-2
                raw[b, j] = torch.randperm(hw - 1, generator=g)
            elif m:                                             # raw == k, 0, HW-2, k-1 in turn
                kj = int(k[j])
                raw[b, j, 0] = (min(kj, hw - 2), 0, hw - 2, max(kj - 1, 0))[j % 4]
    return types.SimpleNamespace(cmap=cmap, fv=fv, raw=raw)


@functools.lru_cache(maxsize=None)
def _k9_refs(case, var):
    i = k9_inputs(case)
    return SR.k9_fwd(i.cmap, i.fv, i.raw, case.hw, case.top_k, **dict(var))


def k9_refs(case, dt=F64, var={}):
    return _k9_refs(case, tuple(sorted(var.items())))


# ---- colnorm forward / backward ---------------------------------------------------------------------------------------------------------
class CN(NamedTuple):
    name: str
    n: int
    hw: int
    e: int
    zero: bool              # a planted all-zero column (image 0, channel 1)
    extra: bool
    n_extra: int
    covers: str

    def __str__(self):
        return self.name


CN_CASES = [
    CN("N1-HW1-E4", 1, 1, 4, False, False, 0, "hs"),
    CN("N3-HW3-E64", 3, 3, 64, True, True, 2, "hjqrs"),
    CN("N1-HW4-E68", 1, 4, 68, False, True, 0, "hs"),
    CN("N3-HW5-E100", 3, 5, 100, True, True, 0, "hjqs"),
    CN("N3-HW28-E4", 3, 28, 4, False, True, 2, "hqrs"),
    CN("N1-HW29-E64", 1, 29, 64, True, False, 0, "hjs"),
    CN("N3-HW32-E68", 3, 32, 68, False, False, 2, "hs"),
    CN("N3-HW33-E100", 3, 33, 100, False, True, 2, "hqrs"),
    CN("N1-HW36-E68", 1, 36, 68, True, True, 0, "hjs"),
    CN("N3-HW37-E64", 3, 37, 64, False, True, 0, "hqs"),
    CN("N3-HW61-E100", 3, 61, 100, True, True, 2, "hjqrs"),
]


@functools.lru_cache(maxsize=None)
def colnorm_inputs(case):
    g = _gen(_seed(case, CN_CASES, _RESEED["colnorm"], 20400))
    v = _rn(g, case.n, case.hw, case.e) * (0.5 + torch.rand(1, 1, case.e, generator=g))
    if case.zero:
        v[0, :, 1] = 0.0
    dq = _rn(g, case.n, case.hw, case.e)
    extra = _rn(g, case.hw, case.e) if case.extra else None
    return types.SimpleNamespace(v=v.contiguous(), dq=dq, extra=extra)


def _pick(var, names):
    return {k: v for k, v in var.items() if k in names}


def colnorm_refs(case, dt=F64, var={}, fwd=None):
    """Forward, and backward on `fwd` = (vit, cnorm) float32 (the device's own in the GPU test; the fp32-rounded reference otherwise)."""
    i = colnorm_inputs(case)
    out = SR.colnorm_fwd(i.v, dt, **_pick(var, ("over_channels", "no_eps")))
    if fwd is None:
        right = SR.colnorm_fwd(i.v, F64)
        fwd = (right["vit"][0].float(), right["cnorm"][0].float())
    out.update(SR.colnorm_bwd(fwd[0], fwd[1], i.dq, i.extra, case.n_extra, dt,
                              **_pick(var, ("extra_all", "extra_img0", "no_proj", "no_eps"))))
    return out


# ---- lagnorm --------------------------------------------------------------------------------------------------------------------------------
class LN(NamedTuple):
    name: str
    n: int
    L: int
    e: int                  # D / 2
    zero: bool
    covers: str

    def __str__(self):
        return self.name


LN_CASES = [
    LN("N1-L1-E4", 1, 1, 4, False, "hi"),
    LN("N3-L20-E256", 3, 20, 256, True, "hij"),
    LN("N2-L32-E300", 2, 32, 300, False, "hi"),
    LN("N2-L20-E4", 2, 20, 4, True, "hij"),
]


@functools.lru_cache(maxsize=None)
def lagnorm_inputs(case):
    g = _gen(_seed(case, LN_CASES, _RESEED["lagnorm"], 20700))
    ctx = _rn(g, case.n, case.L, 2 * case.e)
    ctx[:, :, 1::2] = 1e30                                      # the odd channels must never be read
    if case.zero:
        ctx[0, :, 2] = 0.0
    return types.SimpleNamespace(ctx=ctx.contiguous())


def lagnorm_refs(case, dt=F64, var={}):
    return SR.lagnorm_fwd(lagnorm_inputs(case).ctx, dt, **_pick(var, ("odd", "over_channels", "no_eps")))


# ---- crossmap -----------------------------------------------------------------------------------------------------------------------------
class CM(NamedTuple):
    name: str
    n: int
    L: int
    hw: int
    e: int
    plant: str              # "-", "tie" (filter rows TIE_A < TIE_B equal, equal biases), "zero" (all weights 0, equal biases)
    covers: str

    def __str__(self):
        return self.name


TIE_A, TIE_B = 1, 3
CM_CASES = [
    CM("L1-HW1-E4", 2, 1, 1, 4, "-", "mn"),
    CM("L3-HW2-E8", 2, 3, 2, 8, "-", "klmn"),
    CM("L20-HW64-E260", 2, 20, 64, 260, "-", "klmn"),
    CM("L20-HW30-E1024", 1, 20, 30, 1024, "-", "klmn"),
    CM("L5-HW9-E1028", 2, 5, 9, 1028, "-", "klmn"),              # the E > 1024 path
    CM("L2-HW5-E2048", 1, 2, 5, 2048, "-", "klmn"),
    CM("L4-HW1030-E8", 1, 4, 1030, 8, "-", "klmn"),              # second trip of the arg-max loop
    CM("L32-HW413-E4", 1, 32, 413, 4, "-", "klmn"),              # exactly 64 KiB of LDS
    CM("L5-HW9-E8-tie", 2, 5, 9, 8, "tie", "klmno"),
    CM("L3-HW5-E8-zero", 2, 3, 5, 8, "zero", "no"),
]


@functools.lru_cache(maxsize=None)
def crossmap_inputs(case):
    g = _gen(_seed(case, CM_CASES, _RESEED["crossmap"], 21000))
    lag = torch.nn.functional.normalize(_rn(g, case.n, case.L, case.e), dim=1)
    vit = torch.nn.functional.normalize(_rn(g, case.n, case.hw, case.e), dim=1)
    w = _rn(g, case.L, case.L, 3) * 0.2; b = _rn(g, case.L) * 0.1
    if case.plant == "tie":
        w[TIE_B] = w[TIE_A]; b[TIE_A] = 0.5; b[TIE_B] = 0.5
    if case.plant == "zero":
        w.zero_(); b.fill_(0.25)
    return types.SimpleNamespace(lag=lag.contiguous(), vit=vit.contiguous(), w=w.contiguous(), b=b)


@functools.lru_cache(maxsize=None)
def _crossmap_refs(case, dt, var):
    i = crossmap_inputs(case)
    return SR.crossmap(i.lag, i.vit, i.w, i.b, dt, **dict(var))


def crossmap_refs(case, dt=F64, var={}):
    r = _crossmap_refs(case, dt, tuple(sorted(var.items())))
    return dict(lvmap=r["lvmap"], cols=r["cols"])


def crossmap_gap(case):
    return _crossmap_refs(case, F64, ())["gap"]


# ---- k14_gather ---------------------------------------------------------------------------------------------------------------------------
class GA(NamedTuple):
    name: str
    n: int
    hw: int
    L: int
    e: int
    neg_n: int
    covers: str

    def __str__(self):
        return self.name


GA_CASES = [
    GA("N1-HW1", 1, 1, 3, 4, 1, ""),                            # one wave of the last block
    GA("N3-HW5", 3, 5, 3, 260, 5, "p"),                         # 15 rows: three idle waves
    GA("N2-HW7", 2, 7, 4, 8, 1, "p"),
]


@functools.lru_cache(maxsize=None)
def gather_inputs(case):
    g = _gen(_seed(case, GA_CASES, _RESEED["gather"], 21300))
    c = torch.arange(case.e) / 1024.0
    vit = (100.0 * torch.arange(case.n).view(-1, 1, 1) + torch.arange(case.hw).view(1, -1, 1) + c).float().contiguous()
    lag = -(100.0 * torch.arange(case.n).view(-1, 1, 1) + torch.arange(case.L).view(1, -1, 1) + c).float().contiguous()
    cols = torch.randint(0, case.L, (case.n, case.hw), generator=g)
    neg = torch.randint(0, case.hw, (case.n, case.hw, case.neg_n), generator=g)
    return types.SimpleNamespace(lag=lag, vit=vit, cols=cols, neg=neg)


def gather_refs(case, dt=F64, var={}):
    i = gather_inputs(case)
    return SR.k14_gather(i.lag, i.vit, i.cols, i.neg, **_pick(var, ("own_image",)))


# ---- k14_negscatter -----------------------------------------------------------------------------------------------------------------------
class NS(NamedTuple):
    name: str
    e: int
    rows: tuple

    def __str__(self):
        return self.name


NS_ROWS = (0, 1, 7, 8, 9, 16, 17, 0)                            # around the 8-unroll; empty first and last rows
NS_CASES = [NS("E4", 4, NS_ROWS), NS("E300", 300, NS_ROWS)]


@functools.lru_cache(maxsize=None)
def negscatter_inputs(case):
    g = _gen(_seed(case, NS_CASES, _RESEED["negscatter"], 21600))
    total = sum(case.rows)
    perm = torch.randperm(total, generator=g)
    off = np.concatenate([[0], np.cumsum(case.rows)]).astype(np.int32)
    src = torch.cat([perm[off[p]:off[p + 1]].sort()[0] for p in range(len(case.rows))]).to(torch.int32)
    d_neg = _rn(g, total, case.e)
    return types.SimpleNamespace(d_neg=d_neg, off=torch.from_numpy(off), src=src, hw=len(case.rows))


# ---- k14_dlag -----------------------------------------------------------------------------------------------------------------------------
class DL(NamedTuple):
    name: str
    n: int
    L: int
    hw: int
    e: int
    zero: bool
    covers: str

    def __str__(self):
        return self.name


DL_CASES = [
    DL("N2-L1-HW1-E4", 2, 1, 1, 4, False, "t"),
    DL("N2-L1-HW9-E100", 2, 1, 9, 100, False, "t"),               # one word owns 9 positions
    DL("N2-L32-HW40-E130", 2, 32, 40, 130, True, "jt"),           # words owning 0 / 7 / 8 / 9 positions; a second channel block
    DL("N1-L32-HW9-E4", 1, 32, 9, 4, False, "t"),
]


@functools.lru_cache(maxsize=None)
def dlag_inputs(case):
    g = _gen(_seed(case, DL_CASES, _RESEED["dlag"], 21900))
    f = SR.lagnorm_fwd(_rn(g, case.n, case.L, 2 * case.e), F32)
    lag, lnorm = f["lag"][0].contiguous(), f["lnorm"][0].contiguous()
    if case.zero:
        lag[0, :, 1] = 0.0; lnorm[0, 1] = 0.0
    if case.L == 32 and case.hw == 40:
        words = [3] * 7 + [5] * 8 + [9] * 9 + list(range(10, 26))    # 7 + 8 + 9 + 16 singles; the other words own nothing
        cols = torch.stack([torch.tensor(words)[torch.randperm(40, generator=g)] for _ in range(case.n)])
    else:
        cols = torch.randint(0, case.L, (case.n, case.hw), generator=g)
    d_k = _rn(g, case.n, case.hw, 1, case.e)
    return types.SimpleNamespace(lag=lag, lnorm=lnorm, cols=cols, d_k=d_k)


def dlag_refs(case, dt=F64, var={}):
    i = dlag_inputs(case)
    return SR.k14_dlag(i.lag, i.lnorm, i.cols, i.d_k, dt, **_pick(var, ("no_proj", "no_eps")))


# ---- k9_bwd -------------------------------------------------------------------------------------------------------------------------------
class KB(NamedTuple):
    name: str
    pairs: int
    hw: int
    e: int
    top_k: int
    neg_n: int

    def __str__(self):
        return self.name


KB_CASES = [
    KB("HW1-k4-m0", 1, 1, 516, 4, 0),
    KB("HW16-k30-m1", 2, 16, 516, 30, 1),
    KB("HW17-k64-m14", 2, 17, 516, 64, 14),                     # 960 list entries: 65344 bytes of LDS, the most the check admits
]


@functools.lru_cache(maxsize=None)
def k9_bwd_inputs(case):
    g = _gen(_seed(case, KB_CASES, _RESEED["k9_bwd"], 22200))
    index = torch.randint(0, case.hw * case.hw, (case.pairs, case.top_k), generator=g)
    neg_idx = torch.randint(0, case.hw, (case.pairs, case.top_k, case.neg_n), generator=g)
    d_frame, d_corr = _rn(g, case.pairs, case.top_k, case.e), _rn(g, case.pairs, case.top_k, case.e)
    d_neg = _rn(g, case.pairs, case.top_k, case.neg_n, case.e)
    return types.SimpleNamespace(index=index, neg_idx=neg_idx, d_frame=d_frame, d_corr=d_corr, d_neg=d_neg)


# ---- the device sampler -------------------------------------------------------------------------------------------------------------------
class SP(NamedTuple):
    name: str
    n: int
    hw: int
    top_k: int
    neg_n: int
    neg_c: int
    seed: int
    step: int
    steps: int
    covers: str

    def __str__(self):
        return self.name


SP_CASES = [
    SP("pop1", 2, 2, 1, 1, 1, 0x1234567800000005, 0, 1, "uvw"),
    SP("perm16", 2, 17, 3, 16, 16, 77, 7, 1, "uvw"),                          # k = pop: many blocks per draw
    SP("pop64-carry", 4, 65, 5, 10, 5, 0x4F1BBCDCBFA53E0A, 2 ** 32 - 1, 3, "uvwx"),   # the step counter carries into its high word
    SP("pop63-64", 4, 64, 30, 10, 5, 0x0000000100000000, 3, 1, "uvw"),
    SP("total156", 6, 13, 2, 3, 2, 9, 0, 2, "vw"),
    SP("total262", 2, 131, 1, 1, 1, 0x7FFFFFFFFFFFFFFF, 5, 1, "vw"),
]


@functools.lru_cache(maxsize=None)
def _sampler_refs(case, var):
    v = dict(var)
    out = {}
    for s in range(case.steps):
        k14 = SR.k14_table(case.n, case.hw, case.neg_c, case.seed, case.step + s, **v)
        off, src = SR.csr(k14, case.hw)
        out[f"k9@{s}"] = torch.from_numpy(SR.k9_table(case.n, case.hw, case.top_k, case.neg_n, case.seed, case.step + s, **v))
        out[f"k14@{s}"] = torch.from_numpy(k14)
        out[f"csr_off@{s}"] = torch.from_numpy(off); out[f"csr_src@{s}"] = torch.from_numpy(src)
    return out


def sampler_refs(case, dt=F64, var={}):
    return _sampler_refs(case, tuple(sorted(var.items())))
