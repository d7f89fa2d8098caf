"""Case tables and seeded generators for the post-processing kernels (csrc/post.hip: post_topk / post_fusion / post_argmax; csrc/video.hip:
post_fusion_bank / bank_argmax), shared by test_post_ref_host.py (CPU: every case tells the wrong variants of post_ref.py from the right
answer) and test_post_edges_gpu.py (the kernels against the fp64 reference).  numpy only; the shapes are the smallest at which each
mechanism of the kernels can still go wrong.  Inputs and references are computed once per case and must not be modified."""
import collections
import functools
import types

import numpy as np

import post_ref as PR

# A case's tolerance is POST_MARGIN * max(r32, 2**-24) per unit of the reference's scale64, r32 = the same error figure of
# tests/post_torch.py evaluated on the CPU in fp32 at run time (the scheme of util.gemm_tol).  The per-lane strided dot product and expf
# against the CPU's exp each cost a small multiple of the yardstick.  Measured worst err / max(r32, 2**-24) on an MI355X over the tables
# below:
#   post_topk_kernel (boxes)          1.02 (S64-B2-E64-k64-equal-nchw: 2.45 against 2.41 units of 2**-24)
#   post_fusion_kernel                2.74 (B2-R32-K2-E2048-unit-some-tie: 2.74 units where every entry has a tie and r32 is at its floor;
#                                     1.55 at B2-R32-K64-E64, the worst case with a yardstick of its own)
#   post_fusion_bank_kernel           2.00 (n9-R2-K2-E64-norm3-dup and n65-R4-K2-E40-unit-dup, both at the floor; 1.34 at n9-R32-K2-E64)
# The margin is the next integer above twice the worst of them, below the 8 at which it would be capped.
POST_MARGIN_CAP = 8.0
POST_MARGIN = 6.0
assert POST_MARGIN <= POST_MARGIN_CAP


def post_tol(r32):
    return POST_MARGIN * max(r32, PR.U)


# a clamp counts as engaged when the unclamped fp64 value is past it by more than this share of the coordinate's scale64: 2**-12 is
# 2**9 times the largest tolerance the margin cap allows at r32 = 2**-24, so a coordinate engaged here is engaged at run time
ENGAGE = 2.0 ** -12

TopkCase = collections.namedtuple("TopkCase", "size B E k kind layout covers")
TopkCase.__str__ = lambda c: f"S{c.size}-B{c.B}-E{c.E}-k{c.k}-{c.kind}-{c.layout}"
FusionCase = collections.namedtuple("FusionCase", "B R K E regime valid plant covers")
FusionCase.__str__ = lambda c: f"B{c.B}-R{c.R}-K{c.K}-E{c.E}-{c.regime}-{c.valid}-{c.plant}"
BankCase = collections.namedtuple("BankCase", "n R K E regime plant covers")
BankCase.__str__ = lambda c: f"n{c.n}-R{c.R}-K{c.K}-E{c.E}-{c.regime}-{c.plant}"

# ---- top-k -----------------------------------------------------------------------------------------------------------------------
# n = 3 P candidates per clip, 1024 threads, seg = ceil(n / 1024) consecutive indices per thread in the tie scan:
#   size 32: n = 63 < 1024 (k = 63 = n = 3 P: everything is selected);  64: n = 252;  256: n = 4032, seg 4, 1008 active threads;
#   352: n = 7623, seg 8, the last active thread's segment is ragged (7 elements).
# Map kinds (the confidence channel; the box channels are randn):
#   randn    tie-free;
#   neg      -|randn| - 1: every selected key takes the negative branch of the key transform;
#   quant    round(4 randn) / 4: dozens of duplicates of the threshold value in every scale;
#   equal    one value everywhere: the answer is flat indices 0 ... k - 1;
#   planted  randn with the value of rank max(1, k - 2) copied to the last index of one thread's segment, the first index of the next
#            thread's, index n - 1 and one index in each scale: seven elements equal the threshold, at most three slots remain.
# No map contains NaN or -0.0 (asserted by the generator): the reference and torch treat -0.0 == 0.0, the kernel's key transform does
# not, and modulated confidences never produce it.
# Feature layouts: "nchw" contiguous, "nhwc" the strided view the model produces, "slice" channels 3 ... 3 + E of a wider tensor.
# The last clip of every case has ratio, dw, dh and frame_hw chosen so that its first candidate engages all four clamps (ENGAGE).
# covers: the wrong variants of post_ref.topk_ref (a ... f) that change this case's answer.
TOPK_CASES = [TopkCase(*c) for c in (
    (32, 2, 1, 63, "randn", "nchw", "cef"),
    (32, 2, 40, 5, "planted", "nhwc", "adef"),
    (32, 1, 64, 1, "neg", "slice", "cf"),
    (64, 3, 96, 17, "quant", "nhwc", "adef"),
    (64, 2, 64, 64, "equal", "nchw", "adef"),
    (64, 2, 40, 5, "neg", "nhwc", "cef"),
    (256, 2, 512, 5, "planted", "nhwc", "abdef"),
    (256, 2, 40, 64, "quant", "slice", "abdef"),
    (256, 3, 96, 17, "equal", "nchw", "abdf"),
    (256, 2, 64, 1, "planted", "slice", "af"),
    (256, 2, 64, 17, "neg", "nchw", "cef"),
    (352, 2, 96, 17, "planted", "nhwc", "abdef"),
    (352, 2, 40, 64, "quant", "nchw", "abdef"),
    (352, 2, 1, 5, "neg", "slice", "cef"),
    (352, 2, 64, 17, "randn", "nhwc", "ef"),
    (352, 2, 512, 64, "equal", "nhwc", "abdf"),
)]
TOPK_VARIANTS = {"a": dict(tie="last"), "b": dict(tie="strided"), "c": dict(key="bits"), "d": dict(rank="desc"),
                 "e": dict(anchor_scale0=True), "f": dict(clamp=False)}

# inputs redrawn where a clip's threshold class happened to fit the remaining slots exactly (a "quant" map must leave copies over)
_TOPK_RESEED = {"S256-B2-E40-k64-quant-slice": 7104}


def _seed(case, table, reseed):
    return reseed.get(str(case), 7000 + 31 * table.index(case))


def feature_view(base, layout, E):
    """The (B,E,g,g) view of a base tensor (numpy array or torch tensor alike) for a feature layout."""
    if layout == "nhwc":                      # base (B,g,g,E)
        return base.transpose(0, 3, 1, 2) if isinstance(base, np.ndarray) else base.permute(0, 3, 1, 2)
    if layout == "slice":                     # base (B,E+8,g,g)
        return base[:, 3:3 + E]
    return base


def _base_shape(layout, B, E, g):
    return {"nchw": (B, E, g, g), "nhwc": (B, g, g, E), "slice": (B, E + 8, g, g)}[layout]


def planted_positions(size):
    """The indices the "planted" kind copies the threshold value to."""
    grids = PR.grids_of(size)
    n = 3 * sum(g * g for g in grids)
    seg = -(-n // PR.THREADS)
    t = (n // seg) // 3
    pos = [t * seg + seg - 1, t * seg + seg, n - 1]
    off = 0
    for s, g in enumerate(grids):
        p = off + (3 * g * g) // 2 + s
        while p in pos:
            p += 1
        pos.append(p); off += 3 * g * g
    return pos


def _set_flat_conf(outbox, b, flat):
    off = 0
    for o in outbox:
        g = o.shape[-1]
        o[b].reshape(3, 5, g, g)[:, 4] = flat[off:off + 3 * g * g].reshape(3, g, g)
        off += 3 * g * g


def _conf_map(rs, kind, n, k, size):
    v = rs.standard_normal(n).astype(np.float32)
    if kind == "neg":
        v = -np.abs(v) - np.float32(1)
    elif kind == "quant":
        v = np.round(4 * v) / 4 + np.float32(0)                  # (-0.0 + 0.0 = +0.0)
    elif kind == "equal":
        v = np.full(n, 0.5, np.float32)
    elif kind == "planted":
        val = np.sort(v)[::-1][max(1, k - 2) - 1]
        pos = planted_positions(size)
        free = [q for q in range(n) if q not in pos and v[q] < val]
        for p in pos:                                             # a planted position never displaces a value above the threshold
            if v[p] >= val:
                q = free.pop(0)
                v[p], v[q] = v[q], v[p]
        v[pos] = val
    v = v.astype(np.float32)
    assert not np.isnan(v).any() and not (np.signbit(v) & (v == 0)).any()
    return v


@functools.lru_cache(maxsize=None)
def topk_inputs(case):
    """outbox[s] (B,15,g,g), feat_base[s] (the tensor feature_view takes the (B,E,g,g) view of), ratio / dw / dh (B,) float32,
    frame_hw (B,2) int64."""
    rs = np.random.RandomState(_seed(case, TOPK_CASES, _TOPK_RESEED))
    grids = PR.grids_of(case.size)
    n = 3 * sum(g * g for g in grids)
    B = case.B
    outbox = [rs.standard_normal((B, 15, g, g)).astype(np.float32) for g in grids]
    for b in range(B):
        _set_flat_conf(outbox, b, _conf_map(rs, case.kind, n, case.k, case.size))
    base = [rs.standard_normal(_base_shape(case.layout, B, case.E, g)).astype(np.float32) for g in grids]
    ratio = (0.5 + rs.rand(B)).astype(np.float32); dw = (8 * rs.rand(B)).astype(np.float32); dh = (8 * rs.rand(B)).astype(np.float32)
    hw = np.array([[case.size - 20, case.size - 8]] * B, np.int64)
    # the clamp clip: its first candidate gets a box of a fixed relative size, then a letterbox that cuts all four sides of it
    b = B - 1
    s, a, gj, gi = PR.unflatten(int(PR.stable_order(PR.flat_conf(outbox, b))[0]), case.size)
    outbox[s][b, a * 5 + 2, gj, gi] = 0.5; outbox[s][b, a * 5 + 3, gj, gi] = 0.5
    one = np.ones(B, np.float32); zero = np.zeros(B, np.float32)
    x1, y1, x2, y2 = PR.topk_ref([o[b:b + 1] for o in outbox], [feature_view(f, case.layout, case.E)[b:b + 1] for f in base], case.size, 1,
                                 one, zero, zero, hw, clamp=False).raw[0, 0]
    ratio[b] = (x2 - x1) / 64.0                                   # the box is 64 pixels wide in the original frame
    dw[b] = x1 + (x2 - x1) / 4; dh[b] = y1 + (y2 - y1) / 4       # a quarter of it lies left of / above the frame
    r = float(ratio[b])
    hw[b] = (int((y2 - float(dh[b])) / r / 2), int((x2 - float(dw[b])) / r / 2))      # the frame ends half way to its far sides
    return types.SimpleNamespace(outbox=outbox, feat_base=base, ratio=ratio, dw=dw, dh=dh, frame_hw=hw)


def topk_args(case):
    i = topk_inputs(case)
    return (i.outbox, [feature_view(f, case.layout, case.E) for f in i.feat_base], case.size, case.k, i.ratio, i.dw, i.dh, i.frame_hw)


@functools.lru_cache(maxsize=None)
def topk_reference(case):
    return PR.topk_ref(*topk_args(case))


# ---- fusion ----------------------------------------------------------------------------------------------------------------------
# Regimes: "unit" unit-norm rows as the model's features are (the softmax matters: weights within e^2 of each other), "norm3" rows of
# norm 3 (a sharper softmax), "sat" the un-normalised randn rows of test_post_kernels_against_the_torch_forms with the centre among the
# frames (one frame leads by hundreds: the fused score is exactly that frame's referred score, or exactly 0 if it is invalid).  In
# every regime frame R // 2 holds the centre's own rows.
# valid: "none" (no mask), "some" (frames invalid at random; the centre frame of window 0 is invalid), "all" (every frame invalid: the
# fused scores are exactly 0).
# plant: "tie"  the centre frame's reference row 0 copied to slot K - 1 with another score (an exact tie of the per-frame maximum);
#        "dup"  centre candidate K - 1 is a copy of candidate 0 (before the centre frame is filled in, so the frame ties as well), and
#               the centre frame's score of slot 0 is raised so that the two equal fused scores are the largest;
#        "-"    nothing.
# The large E (2048 staged, 2112 unstaged) go with small K R; B = 65 and 130 are for the arg-max kernels' second and third block.
# covers: the wrong variants of post_ref.fusion_ref / fusion_bank_ref (g ... l) that change this case's answer.
FUSION_CASES = [FusionCase(*c) for c in (
    (2, 5, 5, 512, "unit", "some", "tie", "ghl"),
    (3, 4, 5, 64, "unit", "some", "dup", "ghkl"),
    (2, 2, 2, 40, "unit", "none", "dup", "hkl"),
    (2, 1, 5, 64, "unit", "none", "tie", "h"),
    (2, 32, 2, 2048, "unit", "some", "tie", "ghl"),
    (2, 2, 1, 2112, "unit", "some", "-", "gl"),
    (2, 5, 64, 40, "norm3", "some", "tie", "ghl"),
    (2, 5, 64, 1, "unit", "none", "-", "hkl"),
    (65, 2, 2, 1, "unit", "all", "-", "k"),
    (130, 4, 2, 40, "unit", "some", "dup", "ghkl"),
    (3, 5, 5, 512, "sat", "some", "-", "gl"),
    (2, 4, 2, 2112, "sat", "none", "dup", "hk"),
    (2, 32, 64, 64, "unit", "some", "-", "gl"),
    (2, 5, 5, 512, "unit", "all", "-", "k"),
    (2, 5, 2, 2048, "norm3", "none", "dup", "hk"),
)]
# Bank cases: n = 1 (every neighbour missing), n = 2 < R, n = 9, n = 65 (the second arg-max block).  plant "dup": candidate K - 1 of
# every entry is a copy of candidate 0 with another score, and the score of candidate 0 is raised.
BANK_CASES = [BankCase(*c) for c in (
    (1, 5, 5, 64, "unit", "-", "gl"),
    (2, 4, 64, 40, "unit", "-", "gil"),
    (9, 5, 5, 512, "unit", "dup", "ghikl"),
    (9, 2, 2, 64, "norm3", "dup", "ghjkl"),
    (65, 4, 2, 40, "unit", "dup", "ghijkl"),
    (9, 32, 2, 64, "unit", "-", "gil"),
    (65, 5, 1, 1, "unit", "-", "gil"),
    (9, 4, 5, 512, "sat", "-", "gijl"),
    (2, 5, 2, 2112, "unit", "-", "gil"),
)]
FUSION_VARIANTS = {"g": dict(mask="before"), "h": dict(frame_tie="last"), "i": dict(missing="clamp"), "j": dict(start="ceil"),
                   "k": dict(best_tie="last"), "l": dict(weights="onehot")}
AMBIGUITY_CAP = 0.02                         # share of a case's (b, c, r) triples that may be ambiguous

_FUSION_RESEED = {}
_BANK_RESEED = {}


def _rows(rs, shape, regime):
    v = rs.standard_normal(shape)
    if regime != "sat":
        v = v / np.sqrt((v * v).sum(-1, keepdims=True)) * (3.0 if regime == "norm3" else 1.0)
    return v.astype(np.float32)


def _scores(rs, shape):
    return (1.25 * rs.rand(*shape) - 0.25).astype(np.float32)


@functools.lru_cache(maxsize=None)
def fusion_inputs(case):
    """center (B,K,E), ref (B,R,K,E), ref_score (B,R,K) float32, valid (B,R) bool or None"""
    rs = np.random.RandomState(_seed(case, FUSION_CASES, _FUSION_RESEED))
    B, R, K, E = case.B, case.R, case.K, case.E
    center = _rows(rs, (B, K, E), case.regime); ref = _rows(rs, (B, R, K, E), case.regime); score = _scores(rs, (B, R, K))
    if case.plant == "dup":
        center[:, K - 1] = center[:, 0]; score[:, R // 2, 0] = 64.0
    ref[:, R // 2] = center
    if case.plant == "tie":
        ref[:, R // 2, K - 1] = ref[:, R // 2, 0]
    valid = None
    if case.valid == "some":
        valid = rs.rand(B, R) > 0.3
        valid[0, R // 2] = False
        if B > 1:
            valid[1] = True; valid[1, 0] = False
    elif case.valid == "all":
        valid = np.zeros((B, R), bool)
    return center, ref, score, valid


@functools.lru_cache(maxsize=None)
def fusion_reference(case):
    return PR.fusion_ref(*fusion_inputs(case))


@functools.lru_cache(maxsize=None)
def bank_inputs(case):
    """feats (n,K,E), scores (n,K) float32"""
    rs = np.random.RandomState(_seed(case, BANK_CASES, _BANK_RESEED))
    feats = _rows(rs, (case.n, case.K, case.E), case.regime); scores = _scores(rs, (case.n, case.K))
    if case.plant == "dup":
        feats[:, case.K - 1] = feats[:, 0]; scores[:, 0] = 64.0
    return feats, scores


@functools.lru_cache(maxsize=None)
def bank_reference(case):
    return PR.fusion_bank_ref(*bank_inputs(case), case.R)
