"""float32 numpy restatement of streaming tube linking (dcnet_amd/csrc/tube.hip, tube_stream_step / _flush) and
the cases that tests/test_tube_stream_host.py and tests/test_tube_stream_gpu.py share.  No torch, no GPU.

The contract.  unary (n,k), W (n,k,k) (W[t][i][j]: candidate i of frame t-1 to candidate j of frame t; W[0] unused), keep (n,k), a lag
L in 1 ... 64.  keep, W, delta, the back-pointers and their tie rules are those of tube_ref.viterbi:
    delta_0[j] = keep ? unary[0,j] : -inf;   delta_t[j] = keep ? unary[t,j] + max_i (delta_{t-1}[i] + W[t][i][j]) : -inf
with the lowest arg-max as back-pointer.  After step t >= L frame t - L is committed:
    a[j]  = the ancestor at frame t - L of candidate j of frame t (the back-pointers of frames t, t-1, ..., t-L+1)
    live  = {j : delta_t[j] > -inf};   j* = first arg-max of delta_t;   c = a[j*]  is the candidate of frame t - L
    if some live j has a[j] != c the commit is FORCED: forced += 1 and delta_t[j] = -inf for every j with a[j] != c
(dead lanes take no part in the agreement test).  After n frames the last min(L, n) frames are the walk back from the first arg-max of
delta_{n-1}, and score = max delta_{n-1}.

Every delta update here is the two single fp32 additions the kernel makes (delta_{t-1}[i] + W, then unary + the maximum); there is no
multiply, so nothing can contract: on the same fp32 W the reference reproduces delta, and with it every decision, bit for bit."""
import functools

import numpy as np

from tube_ref import gen_batch, nms_batch, path_case, path_slack, path_value, tie_case, transitions, viterbi  # noqa: F401  (re-exported)

LAGS = (1, 2, 8, 64)
GEN_SHAPES = [(2, 33, 5, 64), (1, 40, 20, 96), (1, 48, 64, 512)]          # tube_ref.PATH_SHAPES without the single frame
BIG = GEN_SHAPES[2]


def stream_viterbi(unary, W, keep, lag, prune=True, tie="first", depth_shift=0, count_dead=False):
    """unary (n,k), W (n,k,k), keep (n,k) bool or None -> (path (n,) int64, forced, score float32): entries 0 ... n-min(lag,n)-1 of
    the path are the commits, the rest the tail of the flush.  The keyword arguments select the WRONG variants of
    tests/test_tube_stream_host.py: prune=False (delta is not altered after a forced commit), tie="last" (last maximum, at every
    step, for j* and at the end), depth_shift=1 (the ancestor is read one frame too shallow), count_dead=True (lanes at -inf take
    part in the agreement test)."""
    unary = np.asarray(unary, np.float32); W = np.asarray(W, np.float32)
    n, k = unary.shape
    ok = np.ones((n, k), bool) if keep is None else np.asarray(keep).astype(bool)
    ninf = np.float32(-np.inf)
    if tie == "first":
        amax = lambda v: int(np.argmax(v))
        amax0 = lambda m: np.argmax(m, axis=0)
    else:
        amax = lambda v: int(len(v) - 1 - np.argmax(v[::-1]))
        amax0 = lambda m: m.shape[0] - 1 - np.argmax(m[::-1], axis=0)
    cols = np.arange(k)
    bp = np.zeros((n, k), np.int64)
    path = np.full(n, -1, np.int64)
    forced = 0
    delta = np.where(ok[0], unary[0], ninf).astype(np.float32)
    for t in range(1, n):
        cand = delta[:, None] + W[t]                                       # one fp32 addition each
        bp[t] = amax0(cand)
        delta = np.where(ok[t], unary[t] + cand[bp[t], cols], ninf).astype(np.float32)      # the other one
        if t >= lag:
            a = cols.copy()
            for s in range(t, t - lag + depth_shift, -1):
                a = bp[s][a]
            c = a[amax(delta)]
            voters = np.ones(k, bool) if count_dead else delta > ninf
            if np.any(voters & (a != c)):
                forced += 1
                if prune:
                    delta = np.where(a != c, ninf, delta).astype(np.float32)
            path[t - lag] = c
    m = min(lag, n)
    path[n - 1] = amax(delta)
    for s in range(n - 1, n - m, -1):
        path[s - 1] = bp[s][path[s]]
    return path, forced, np.float32(delta.max())


# ---- the two hand cases ---------------------------------------------------------------------------------------------------------
def _diag_w(n, k):
    W = np.full((n, k, k), -5.0, np.float32)
    W[:, np.arange(k), np.arange(k)] = 0.0
    return W


@functools.lru_cache(maxsize=None)
def twin():
    """Two tracks of equal value that never merge (n 16, k 4): candidates 0 and 1 score 1 in every frame, candidate 1 scores 1.5 in the
    last; staying costs 0, changing 5.  Any commit before the last frame is forced and takes the first of the tie, candidate 0; the
    optimum is candidate 1 throughout."""
    n, k = 16, 4
    unary = np.zeros((n, k), np.float32)
    unary[:, 0] = unary[:, 1] = 1.0
    unary[15, 1] = 1.5
    return {"unary": unary, "W": _diag_w(n, k), "keep": None}


@functools.lru_cache(maxsize=None)
def dead_lane():
    """n 8, k 2: candidate 1 (0.9 per frame against 1) is suppressed from frame 2 on.  Its lane is dead at the first commit and its
    ancestor differs from the live one's: the commit is not forced."""
    n, k = 8, 2
    unary = np.zeros((n, k), np.float32)
    unary[:, 0] = 1.0; unary[:, 1] = 0.9
    keep = np.ones((n, k), bool)
    keep[2:, 1] = False
    return {"unary": unary, "W": _diag_w(n, k), "keep": keep}


def w32(c, q):
    """tube_ref's fp64 transitions of query q of a generated case, cast to fp32 (the host tests' stand-in for the device's W)."""
    return transitions(c["boxes"][q], c["feats"][q], 1.0, 1.0)[0].astype(np.float32)


def gen_cases():
    """(name, batch dict with boxes / unary / feats and keep or None) of every generated case: the three shapes with and without
    their NMS mask, and tie_case."""
    out = []
    for shape in GEN_SHAPES:
        c = path_case(*shape)
        out.append((f"{shape}", {**c, "keep": None}))
        out.append((f"{shape}+keep", c))
    out.append(("tie", {**{key: v[None] for key, v in tie_case().items()}, "keep": None}))
    return out
