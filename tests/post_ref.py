"""numpy restatement of the post-processing kernels (dcnet_amd/csrc/post.hip, the fusion of csrc/video.hip) that shares nothing with
the library: top-k selection by a stable sort (no arithmetic, exact), box decode and temporal fusion in float64.  No torch, no GPU.

Every input is the float32 (int64 for frame_hw) array the device reads; every reference value is computed in float64 from it.
The keyword arguments select deliberately WRONG variants; tests/test_post_ref_host.py shows that the shared cases of
tests/post_cases.py tell each of them from the right answer.

  topk_ref          tie="last"       (a) ties at the threshold taken highest index first
                    tie="strided"    (b) ties at the threshold taken in thread-strided order (i % 1024, then i)
                    key="bits"       (c) keys ordered by raw bit pattern: negative values come out reversed
                    rank="desc"      (d) equal values ranked index descending
                    anchor_scale0    (e) the anchors of scale 0 for every scale
                    clamp=False      (f) no clamp
  fusion_ref        mask="before"    (g) the valid mask applied before the softmax
                    frame_tie="last" (h) last maximum of a frame's similarities in place of the first
                    best_tie="last"  (k) the fused arg-max takes the highest index on ties
                    weights="onehot" (l) softmax weights replaced by one-hot on the largest frame
  fusion_bank_ref   missing="clamp"  (i) a missing neighbour read through a clamped index instead of the centre's entry
                    start="ceil"     (j) window start b - (R - 1) // 2
"""
import types

import numpy as np

U = 2.0 ** -24                              # unit roundoff of fp32
THREADS = 1024                              # for variant (b) only
ANCHOR_IMSIZE = 416.0
# the YOLOv3 anchors, largest first: scale s (grid size / (32 >> s)) owns rows 3 s ... 3 s + 2
ANCHORS = ((373., 326.), (156., 198.), (116., 90.), (59., 119.), (62., 45.), (30., 61.), (33., 23.), (16., 30.), (10., 13.))


def grids_of(size):
    return [size // 32, size // 16, size // 8]


def flat_conf(outbox, b):
    """The confidences of clip b in flat candidate order: scale-major, then anchor, row, column."""
    return np.concatenate([o[b].reshape(3, 5, o.shape[-2], o.shape[-1])[:, 4].reshape(-1) for o in outbox])


def unflatten(j, size):
    """flat candidate index -> (scale, anchor, row, column)"""
    off = 0
    for s, g in enumerate(grids_of(size)):
        if j < off + 3 * g * g:
            r = j - off
            return s, r // (g * g), (r % (g * g)) // g, r % g
        off += 3 * g * g
    raise IndexError(j)


def select(conf, k, tie="first", key="value", rank="asc"):
    """The k selected flat indices of one clip in output order.  conf (n,) float32.  The general form (threshold, ties at the
    threshold, ranking) that the wrong variants need; with the default keywords it equals ``stable_order(conf)[:k]``."""
    n = conf.shape[0]
    bits = conf.view(np.uint32).astype(np.int64)
    if key == "value":                       # an integer with the order of the float (no NaN, no -0.0 in any map)
        keys = np.where(bits >> 31 != 0, 0xFFFFFFFF - bits, bits + 0x80000000)
    else:
        keys = bits ^ 0x80000000
    idx = np.arange(n)
    T = np.sort(keys)[n - k]
    gt = idx[keys > T]; eq = idx[keys == T]
    krem = k - gt.size
    if tie == "last":
        eq = eq[::-1]
    elif tie == "strided":
        eq = eq[np.lexsort((eq, eq % THREADS))]
    chosen = np.concatenate([gt, np.sort(eq[:krem])])
    order = np.lexsort((chosen if rank == "asc" else -chosen, -keys[chosen]))
    return chosen[order]


def stable_order(conf):
    """fp32 value descending, flat index ascending: a stable sort of the negated values (exact: negation and the widening are)."""
    return np.argsort(-conf.astype(np.float64), kind="stable")


def topk_ref(outbox, corr, size, k, ratio, dw, dh, frame_hw, tie="first", key="value", rank="asc", anchor_scale0=False, clamp=True):
    """outbox[s] (B,15,g,g), corr[s] (B,E,g,g) (any strides), ratio / dw / dh (B,) float32, frame_hw (B,2) integers = (H, W).
    Returns idx (B,k) flat indices, cells (B,k,4) int64 (scale, anchor, row, column), scores (B,k) float32 and feats (B,k,E) float32
    (both bitwise the inputs'), and per box coordinate in float64: boxes (B,k,4) xyxy, raw (the unclamped value) and scale
    ((|x| + w/2 + |offset|) / ratio, what that coordinate's rounding errors are proportional to)."""
    B = outbox[0].shape[0]; E = corr[0].shape[1]
    wrong_select = (tie, key, rank) != ("first", "value", "asc")
    out = types.SimpleNamespace(idx=np.zeros((B, k), np.int64), cells=np.zeros((B, k, 4), np.int64), scores=np.zeros((B, k), np.float32),
                                feats=np.zeros((B, k, E), np.float32), boxes=np.zeros((B, k, 4)), raw=np.zeros((B, k, 4)),
                                scale=np.zeros((B, k, 4)))
    for b in range(B):
        conf = flat_conf(outbox, b)
        sel = select(conf, k, tie, key, rank) if wrong_select else stable_order(conf)[:k]
        r, ow, oh = float(ratio[b]), float(dw[b]), float(dh[b])
        H, W = float(frame_hw[b][0]), float(frame_hw[b][1])
        for j, fi in enumerate(sel):
            s, a, gj, gi = unflatten(int(fi), size)
            stride = float(32 >> s); g = size // (32 >> s)
            t = outbox[s][b, a * 5:a * 5 + 4, gj, gi].astype(np.float64)
            aw, ah = (v / (ANCHOR_IMSIZE / g) for v in ANCHORS[(0 if anchor_scale0 else 3 * s) + a])
            x = (1.0 / (1.0 + np.exp(-t[0])) + gi) * stride; y = (1.0 / (1.0 + np.exp(-t[1])) + gj) * stride
            w = np.exp(t[2]) * aw * stride; h = np.exp(t[3]) * ah * stride
            raw = np.array([(x - w / 2 - ow) / r, (y - h / 2 - oh) / r, (x + w / 2 - ow) / r, (y + h / 2 - oh) / r])
            sx, sy = (abs(x) + w / 2 + abs(ow)) / r, (abs(y) + h / 2 + abs(oh)) / r
            out.idx[b, j] = fi; out.cells[b, j] = (s, a, gj, gi); out.scores[b, j] = conf[fi]
            out.feats[b, j] = corr[s][b, :, gj, gi]
            out.raw[b, j] = raw; out.scale[b, j] = (sx, sy, sx, sy)
            out.boxes[b, j] = (max(raw[0], 0.0), max(raw[1], 0.0), min(raw[2], W), min(raw[3], H)) if clamp else raw
    return out


def fusion_ref(center, ref, ref_score, valid=None, mask="after", frame_tie="first", best_tie="first", weights="softmax"):
    """center (B,K,E), ref (B,R,K,E), ref_score (B,R,K) float32, valid (B,R) bool or None.  In float64: similarity of every centre
    candidate with every candidate of every frame, per frame the FIRST maximum, softmax over the frames, weights of invalid frames
    zeroed AFTER the softmax, fused score, arg-max (lowest index on ties).  Returns
      fused (B,K), scale (B,K) = sum over the valid frames of w_r |s_r|, best (B,),
      ambiguous (B,K,R): the gap between the two largest DISTINCT similarities of the frame is below 64 * 2^-24 * sum_e |c_e r_e| (the
                         larger of the two sums): fp32 may choose the other one.  Equal similarities are ties (the first wins), not
                         ambiguities: rows that are bitwise copies have the same float64 sum here and the same fp32 sum on the device,
      tied (B,K,R): the frame's maximum is attained more than once,
      exact (B,K) / exact_value (B,K) float32: one frame leads every other by more than 128 in the exponent (and its own triple is not
                         ambiguous), so that every fp32 softmax gives it the weight 1 and the others exactly 0: the fused score is then
                         exactly the referred score of that frame, or exactly 0 if it is invalid."""
    c64 = center.astype(np.float64); r64 = ref.astype(np.float64); s64 = ref_score.astype(np.float64)
    B, K, E = center.shape; R = ref.shape[1]
    ok = np.ones((B, R), bool) if valid is None else np.asarray(valid).astype(bool)
    sim = np.empty((B, K, R, K)); S = np.empty((B, K, R, K))
    for b in range(B):
        for r in range(R):
            prod = c64[b][:, None, :] * r64[b, r][None, :, :]                       # (K centre, K ref, E)
            sim[b, :, r, :] = prod.sum(-1); S[b, :, r, :] = np.abs(prod).sum(-1)      # (the same summation order for every row)
    top = sim.max(-1)
    arg = sim.argmax(-1) if frame_tie == "first" else K - 1 - sim[..., ::-1].argmax(-1)
    refer = np.take_along_axis(np.broadcast_to(s64[:, None], (B, K, R, K)), arg[..., None], 3)[..., 0]
    refer32 = np.take_along_axis(np.broadcast_to(ref_score[:, None], (B, K, R, K)), arg[..., None], 3)[..., 0]
    ex = np.exp(top - top.max(-1, keepdims=True))
    okf = ok[:, None, :].astype(np.float64)
    if weights == "onehot":
        w = np.zeros_like(ex); np.put_along_axis(w, top.argmax(-1)[..., None], 1.0, 2)
        w = w * okf
    elif mask == "after":
        w = ex / ex.sum(-1, keepdims=True) * okf
    else:
        den = (ex * okf).sum(-1, keepdims=True)
        w = np.where(den > 0, ex * okf / np.where(den > 0, den, 1.0), 0.0)
    fused = (w * refer).sum(-1); scale = (w * np.abs(refer)).sum(-1)
    best = fused.argmax(-1) if best_tie == "first" else K - 1 - fused[:, ::-1].argmax(-1)
    # ambiguity of the per-frame maximum
    second = np.where(sim < top[..., None], sim, -np.inf).max(-1)
    s_top = np.where(sim == top[..., None], S, 0.0).max(-1); s_sec = np.where(sim == second[..., None], S, 0.0).max(-1)
    ambiguous = np.isfinite(second) & (top - np.where(np.isfinite(second), second, 0.0) < 64 * U * np.maximum(s_top, s_sec))
    tied = (sim == top[..., None]).sum(-1) > 1
    lead = top.argmax(-1)                                                             # (B,K)
    rest = np.where(np.arange(R)[None, None, :] == lead[..., None], -np.inf, top - top.max(-1, keepdims=True))
    exact = (rest.max(-1) < -128.0) & ~np.take_along_axis(ambiguous, lead[..., None], 2)[..., 0]
    lead_ok = np.take_along_axis(np.broadcast_to(ok[:, None, :], (B, K, R)), lead[..., None], 2)[..., 0]
    exact_value = np.where(lead_ok, np.take_along_axis(refer32, lead[..., None], 2)[..., 0], np.float32(0)).astype(np.float32)
    return types.SimpleNamespace(fused=fused, scale=scale, best=best, ambiguous=ambiguous, tied=tied, exact=exact, exact_value=exact_value,
                                 weights=w, sim=sim)


def bank_window(n, R, missing="centre", start="floor"):
    """(src (n,R) entry each window slot reads, valid (n,R)): window b = entries b - R//2 ... b - R//2 + R - 1 of the run; a missing
    neighbour takes the centre's own entry and is invalid."""
    b = np.arange(n)[:, None]
    src = b - (R // 2 if start == "floor" else (R - 1) // 2) + np.arange(R)[None, :]
    valid = (src >= 0) & (src < n)
    src = np.where(valid, src, b) if missing == "centre" else np.clip(src, 0, n - 1)
    return src, valid


def fusion_bank_ref(feats, scores, R, missing="centre", start="floor", **kw):
    """feats (n,K,E), scores (n,K) float32: the candidates of n consecutive centres.  Gathers the windows itself (bank_window), then
    fusion_ref; the weight of a missing neighbour is zeroed after the softmax."""
    src, valid = bank_window(feats.shape[0], R, missing, start)
    return fusion_ref(feats, feats[src], scores[src], valid, **kw)
