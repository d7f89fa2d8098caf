"""fp64 numpy restatement of tube linking (dcnet_amd/csrc/tube.hip), a brute-force path search, the seeded
generators and the fixed cases that tests/test_tube_host.py and tests/test_tube_gpu.py share.  No torch, no GPU.

Every generated tensor is float32 (what the device reads); every reference value is computed in float64 from those float32 values."""
import functools
import itertools

import numpy as np

EPS = float(np.float32(1e-16))
U = 2.0 ** -24                         # unit roundoff of fp32
THRS = (0.3, 0.6)                      # NMS thresholds of the tests; the generator keeps every within-frame IoU 1e-4 away from both
FRAME = 416.0


# ---- the semantics ------------------------------------------------------------------------------------------------------------
def iou(a, b):
    """a (...,4), b (...,4) xyxy, broadcast; dcn_box_iou's formula with widths and heights clamped at 0."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    iw = np.maximum(np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]), 0.0)
    ih = np.maximum(np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]), 0.0)
    inter = iw * ih
    aa = np.maximum(a[..., 2] - a[..., 0], 0.0) * np.maximum(a[..., 3] - a[..., 1], 0.0)
    ab = np.maximum(b[..., 2] - b[..., 0], 0.0) * np.maximum(b[..., 3] - b[..., 1], 0.0)
    return inter / (aa + ab - inter + EPS)


def nms(boxes, thr, against_suppressed=False):
    """boxes (k,4) -> keep (k,) bool: greedy in index order.  ``against_suppressed``: the WRONG variant that also tests a candidate
    against lower-index candidates that were themselves suppressed."""
    k = boxes.shape[0]
    m = iou(boxes[:, None, :], boxes[None, :, :])
    keep = np.zeros(k, bool)
    for i in range(k):
        prior = np.arange(i) if against_suppressed else np.nonzero(keep[:i])[0]
        keep[i] = not np.any(m[prior, i] > thr)
    return keep


def nms_batch(boxes, thr, **kw):
    return np.stack([nms(b, thr, **kw) for b in boxes.reshape(-1, *boxes.shape[-2:])]).reshape(boxes.shape[:-1])


def transitions(boxes, feats, w_iou, w_feat):
    """boxes (n,k,4), feats (n,k,E) or None -> (W (n,k,k) with W[0] = 0, S (n,k,k) = sum_e |a_e b_e| of the dot products)."""
    n, k = boxes.shape[:2]
    W = np.zeros((n, k, k)); S = np.zeros((n, k, k))
    if n > 1:
        W[1:] = w_iou * iou(boxes[:-1, :, None, :], boxes[1:, None, :, :])
        if feats is not None:
            f = feats.astype(np.float64)
            W[1:] += w_feat * np.einsum("tie,tje->tij", f[:-1], f[1:])
            S[1:] = np.einsum("tie,tje->tij", np.abs(f[:-1]), np.abs(f[1:]))
    return W, S


def viterbi(unary, W, keep=None, tie="first", use_keep=True, bp_shift=0):
    """unary (n,k), W (n,k,k), keep (n,k) bool or None -> (path (n,), score, delta (n,k)) in fp64.  The keyword arguments select the
    WRONG variants of tests/test_tube_host.py: tie="last" (last maximum), use_keep=False, bp_shift=1 (the walk reads the
    back-pointer row of the frame below)."""
    unary = unary.astype(np.float64)
    n, k = unary.shape
    ok = np.ones((n, k), bool) if (keep is None or not use_keep) else keep.astype(bool)
    first = (lambda v: int(np.argmax(v))) if tie == "first" else (lambda v: int(len(v) - 1 - np.argmax(v[::-1])))
    delta = np.full((n, k), -np.inf); bp = np.zeros((n, k), np.int64)
    delta[0] = np.where(ok[0], unary[0], -np.inf)
    for t in range(1, n):
        cand = delta[t - 1][:, None] + W[t]                      # [i][j]
        for j in range(k):
            bp[t, j] = first(cand[:, j])
        delta[t] = np.where(ok[t], unary[t] + cand[bp[t], np.arange(k)], -np.inf)
    path = np.zeros(n, np.int64)
    path[n - 1] = first(delta[n - 1])
    for t in range(n - 1, 0, -1):
        path[t - 1] = bp[max(t - bp_shift, 1), path[t]]
    return path, float(delta[n - 1].max()), delta


def path_value(path, unary, W):
    n = len(path)
    return float(unary.astype(np.float64)[np.arange(n), path].sum() + sum(W[t][path[t - 1], path[t]] for t in range(1, n)))


def brute_force(unary, W, keep=None):
    """Every path over kept candidates: (best path, best value, second-best value)."""
    n, k = unary.shape
    slots = [[j for j in range(k) if keep is None or keep[t, j]] for t in range(n)]
    vals = sorted(((path_value(np.array(p), unary, W), p) for p in itertools.product(*slots)), key=lambda x: (-x[0], x[1]))
    return np.array(vals[0][1]), vals[0][0], (vals[1][0] if len(vals) > 1 else -np.inf)


def single_frame_margin(path, unary, W):
    """Value of ``path`` minus the best value of a path that leaves it in exactly one frame."""
    n, k = unary.shape
    u = unary.astype(np.float64)
    worst = np.inf
    for t in range(n):
        for j in range(k):
            if j == path[t]:
                continue
            d = u[t, path[t]] - u[t, j]
            if t > 0:
                d += W[t][path[t - 1], path[t]] - W[t][path[t - 1], j]
            if t < n - 1:
                d += W[t + 1][path[t], path[t + 1]] - W[t + 1][j, path[t + 1]]
            worst = min(worst, d)
    return worst


# ---- the workspace rule -------------------------------------------------------------------------------------------------------
def ranges(q, n, k, ws_bytes):
    per = max(1, ws_bytes // (q * k * k * 4))
    return [(t0, min(n, t0 + per)) for t0 in range(0, n, per)]


# ---- tolerances (derivations: tests/test_tube_gpu.py) ---------------------------------------------------------------------------
def w_bound(W64, S, E, w_iou, w_feat):
    return U * (8 * w_iou + (E + 8) * w_feat * S + 2 * np.abs(W64))


def path_slack(n, E, w_iou, w_feat):
    """The slack of the path value: 2n (2 u n M + eps_W); ``score`` gets half of it."""
    M = 1 + w_iou + w_feat
    eps_w = U * (8 * w_iou + (E + 8) * w_feat + 2 * M)
    return 2 * n * (2 * U * n * M + eps_w)


# ---- generators ---------------------------------------------------------------------------------------------------------------
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _xyxy(cx, cy, w, h):
    return np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], -1)


def gen_frame(rs, k, track, thrs=THRS):
    """One frame: the track box in a random slot, up to two near-duplicates of it (centre +-5 px, size +-10 %), random decoys;
    redrawn until no pair of the frame has an IoU within 1e-4 of a threshold (evaluated in fp64 on the float32 boxes).
    Returns (boxes (k,4) float32, slot, redraws)."""
    cx, cy, w, h = track
    redraws = 0
    while True:
        order = rs.permutation(k)
        boxes = np.zeros((k, 4))
        boxes[order[0]] = _xyxy(cx, cy, w, h)
        for d in order[1:3]:
            boxes[d] = _xyxy(cx + rs.uniform(-5, 5), cy + rs.uniform(-5, 5), w * rs.uniform(0.9, 1.1), h * rs.uniform(0.9, 1.1))
        for d in order[3:]:
            boxes[d] = _xyxy(rs.uniform(40, FRAME - 40), rs.uniform(40, FRAME - 40), rs.uniform(20, 160), rs.uniform(20, 160))
        boxes = boxes.astype(np.float32)
        m = iou(boxes[:, None, :], boxes[None, :, :])[~np.eye(k, dtype=bool)]
        if all(np.all(np.abs(m - t) >= 1e-4) for t in thrs):
            return boxes, int(order[0]), redraws
        redraws += 1


def gen_video(seed, n, k, E):
    """One query: a smooth track (centre random walk of +-6 px, size jitter of +-3 %) planted among duplicates and decoys; scores
    uniform in (0,1), sorted descending per frame; unit-norm features, the track's = a shared base vector + 10 % noise.
    Returns dict(boxes (n,k,4), unary (n,k), feats (n,k,E), slots (n,), redraws) — float32 / int64."""
    rs = np.random.RandomState(seed)
    cx, cy, w, h = rs.uniform(150, 266), rs.uniform(150, 266), rs.uniform(70, 120), rs.uniform(70, 120)
    base = _unit(rs.standard_normal(E))
    boxes = np.zeros((n, k, 4), np.float32); slots = np.zeros(n, np.int64); redraws = 0
    feats = _unit(rs.standard_normal((n, k, E)))
    for t in range(n):
        cx = float(np.clip(cx + rs.uniform(-6, 6), 80, FRAME - 80)); cy = float(np.clip(cy + rs.uniform(-6, 6), 80, FRAME - 80))
        w *= rs.uniform(0.97, 1.03); h *= rs.uniform(0.97, 1.03)
        boxes[t], slots[t], r = gen_frame(rs, k, (cx, cy, w, h))
        redraws += r
        feats[t, slots[t]] = _unit(base + 0.1 * _unit(rs.standard_normal(E)))
    unary = -np.sort(-rs.uniform(0, 1, (n, k)), axis=1)
    return {"boxes": boxes, "unary": unary.astype(np.float32), "feats": feats.astype(np.float32), "slots": slots, "redraws": redraws}


def gen_batch(seeds, n, k, E):
    vs = [gen_video(s, n, k, E) for s in seeds]
    return {key: np.stack([v[key] for v in vs]) for key in ("boxes", "unary", "feats", "slots")}


# ---- the fixed cases the host and GPU tests share -------------------------------------------------------------------------------
NMS_SHAPES = [(7, 1), (5, 5), (33, 20), (9, 64)]
TRANS_SHAPES = [(1, 2, 1, 32), (2, 5, 5, 96), (1, 4, 64, 512), (3, 9, 20, 64)]
TRANS_WEIGHTS = [(1.0, 1.0), (2.0, 0.5), (0.0, 1.0), (1.0, 0.0)]            # the last one runs with feats=None
PATH_SHAPES = [(1, 1, 5, 32), (2, 33, 5, 64), (1, 40, 20, 96), (1, 48, 64, 512)]
BRUTE_SHAPE = (6, 3, 32)
BRUTE_MARGIN = 0.1
PLANTED = [((48, 64, 512), 4800), ((40, 20, 96), 4000)]                      # (n,k,E), seed; weights (1,1), no NMS
PLANTED_MARGIN = 0.05
NMS_THR_PATH = 0.6


@functools.lru_cache(maxsize=None)
def nms_case(B, k):
    """(B + 2, k, 4) float32: B generated frames, one row of zero-area boxes and one whose odd candidates are inverted."""
    rs = np.random.RandomState(1000 * B + k)
    rows = [gen_frame(rs, k, (rs.uniform(150, 266), rs.uniform(150, 266), rs.uniform(70, 120), rs.uniform(70, 120)))[0] for _ in range(B)]
    flat = rows[0].copy(); flat[:, 2] = flat[:, 0]                           # zero width: IoU 0 with everything, all kept
    inv = rows[-1].copy(); inv[1::2] = inv[1::2][:, [2, 3, 0, 1]]            # x2 < x1, y2 < y1
    return np.stack(rows + [flat, inv]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def path_case(Q, n, k, E):
    d = gen_batch([7000 + 100 * n + k + q for q in range(Q)], n, k, E)
    d["keep"] = nms_batch(d["boxes"], NMS_THR_PATH)
    return d


@functools.lru_cache(maxsize=None)
def brute_cases():
    """8 videos of (n,k,E) = BRUTE_SHAPE as one batch, each redrawn (next seed) until best - second-best >= BRUTE_MARGIN; the odd
    ones under a keep mask.  Returns the batch dict + keep (8,n,k) + best (8,n) + margins."""
    n, k, E = BRUTE_SHAPE
    out, seed = [], 9000
    while len(out) < 8:
        v = gen_video(seed, n, k, E); seed += 1
        keep = np.ones((n, k), bool)
        if len(out) % 2:          # (k = 3 is the track and its two duplicates: an NMS would leave one path; a random mask, slot 0 kept)
            keep = np.random.RandomState(seed).uniform(size=(n, k)) < 0.6
            keep[:, 0] = True
        W, _ = transitions(v["boxes"], v["feats"], 1.0, 1.0)
        best, val, second = brute_force(v["unary"], W, keep)
        if val - second >= BRUTE_MARGIN:
            v.update(keep=keep, best=best, margin=val - second, value=val)
            out.append(v)
    return {key: np.stack([v[key] for v in out]) for key in ("boxes", "unary", "feats", "keep", "best", "margin", "value")}


@functools.lru_cache(maxsize=None)
def planted_case(i):
    (n, k, E), seed = PLANTED[i]
    return gen_video(seed, n, k, E)


@functools.lru_cache(maxsize=None)
def tie_case():
    """(n,k,E) = (12,10,32): candidates 5 ... 9 are bit-for-bit copies of candidates 0 ... 4 in every frame."""
    v = gen_video(123, 12, 5, 32)
    return {key: np.concatenate([v[key], v[key]], axis=1) for key in ("boxes", "unary", "feats")}
