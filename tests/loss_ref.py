"""Kernel-by-kernel restatement of dcnet_amd/csrc/loss.hip (target assignment, the dense yolo / rank / loc losses forward and backward,
the InfoNCE rows forward and backward, the evaluation decode, box IoU) in numpy / torch on the CPU, float64 by default: one function per
kernel, on the very float32 / int32 tensors the kernel receives.  No GPU, nothing of dcnet_amd, no code shared with oracle/train_oracle.py
(tests/test_loss_ref_host.py cross-checks the two once, in fp64).

Integer outputs (target_i, the decode's cellinfo, the dense target's positions) are exact.  Every floating-point result comes as
(value, scale), as in tests/head_ref.py and tests/sample_ref.py: `scale` is the sum of the absolute values of the terms that were added
into the element, carried to first order through log, exp, the sigmoid, quotients and square roots; it is the unit in which an error of
that element is judged.  scale == 0 marks an element that must be reproduced exactly: the structural zeros of d_outbox, d_sim and
d_negsim, everything multiplied by an upstream gradient of 0, an IoU without overlap.  An element that passes through exp carries TINY on
top: an fp32 result below 2**-126 may be flushed to zero.  `dt=torch.float32` evaluates the same formulas in fp32: the yardstick r32 of
loss_cases.loss_tol.  The constants the kernels hold as floats (0.1f, 1e-16f, 1e-12f) are those floats here.

The keyword arguments select deliberately WRONG variants; tests/test_loss_ref_host.py shows that the cases of tests/loss_cases.py tell
each of them from the right answer.

  target       last_max     (a) last maximum of the nine anchor IoUs instead of the first
               round_g      (b) gx, gy rounded instead of truncated
               no_clamp     (c) no clamp of the box to [0, size-1]
               fwd_table    (d) anchor table not reversed
               cell_swap    (e) flat cell gi * g + gj
               tw_scale0    (f) tw, th against anchor bn % 3 of scale 0
  dense fwd    conf_sca     (g) confidences concatenated as scale, cell, anchor
               no_max       (h) log-sum-exp without max subtraction (every exp rounded to fp32, as the kernel would hold it)
               partner_next (i) partner sample (n + 1) % N instead of N - 1 - n
               neg_partner  (j) second hinge reads negsim at the partner cell
               rank_n       (k) rank divided by N
               no_wcoord    (l) w_coord missing on the tw, th terms
               sig_tw       (m) sigmoid applied to tw
  dense bwd    no_softmax   (n) the softmax part of the confidence gradient dropped
               store_o      (o) the partner-cell term of d_sim stored instead of accumulated when cell == cell_o
               swap_up      (p) upstream gradients of rank and loc exchanged
               no_dsig      (q) sigmoid derivative missing
  contrastive  no_eps       (r) no 1e-12 clamp of the norms
               times_t      (s) logits multiplied by T
               cut768       (t) columns from 768 on ignored
               stride_m1    (u) negatives of row r read at stride M - 1
               mean_all     (v) mean over rows * (M + 1)
               no_proj      (w) dq without its projection term
  decode       last_max     (x) last maximum
               swap_wh      (y) anchor w and h exchanged
               stride0      (z) stride of scale 0 for all scales
               full_ext     (A) full instead of half extents in xywh to xyxy
  box_iou      no_inter     (B) union without - inter
               no_clamp     (C) overlap extents not clamped at 0
"""
import numpy as np
import torch

F64 = torch.float64
F32 = torch.float32
U = 2.0 ** -24                               # unit roundoff of fp32
TINY = 2.0 ** -126 / U                       # per unit of U: the smallest normal fp32
MARGIN_F = float(np.float32(0.1))            # RANK_MARGIN = 0.1f
EPS16_F = float(np.float32(1e-16))
EPS12_F = float(np.float32(1e-12))
ANCHORS = [(10, 13), (16, 30), (33, 23), (30, 61), (62, 45), (59, 119), (116, 90), (156, 198), (373, 326)]


def grids(size):
    return [size // 32, size // 16, size // 8]


def offsets(size):
    """First column of each scale among the P positions, and P."""
    o, off = 0, []
    for g in grids(size):
        off.append(o); o += g * g
    return off, o


def scaled_anchors(size, reverse=True, anchor_imsize=416):
    """(3,3,2) float32: the anchor table, largest first, in grid units of its scale; computed in double and rounded once."""
    table = ANCHORS[::-1] if reverse else ANCHORS
    rows = [[(a[0] / (anchor_imsize / g), a[1] / (anchor_imsize / g)) for a in table[3 * s:3 * s + 3]] for s, g in enumerate(grids(size))]
    return torch.tensor(rows, dtype=F64).to(F32)


def err_units(got, ref, scale):
    """max over the elements with scale > 0 of |got - ref| / scale, and whether every element with scale == 0 is reproduced exactly."""
    got = got.detach().to(F64).reshape(ref.shape); ref = ref.detach().to(F64); scale = scale.detach().to(F64)
    pos = scale > 0
    e = float(((got - ref).abs()[pos] / scale[pos]).max()) if bool(pos.any()) else 0.0
    exact = bool(torch.equal(got[~pos], ref[~pos]))
    finite = bool(torch.isfinite(got[pos]).all())
    return (e if finite else float("inf")), exact


def _sig(t):
    return 1.0 / (1.0 + torch.exp(-t))


# ---- target ------------------------------------------------------------------------------------------------------------------------------
def target(bbox, anchors, size, dt=F64, last_max=False, round_g=False, no_clamp=False, fwd_table=False, cell_swap=False, tw_scale0=False):
    """bbox (N,4) f32 xyxy pixels, anchors (3,3,2) f32 -> ti (N,4) int32 = bn, gi, gj, flat cell;  tf (N,4) = tx, ty, tw, th.
    Also iou_gap (N,): top-2 gap of the nine IoUs over the largest, and frac (N,2): distance of gx, gy to the next integer over |gx|, |gy|
    (inf where gx is 0), for the guard band."""
    N = bbox.shape[0]
    G, (off, _) = grids(size), offsets(size)
    an = (scaled_anchors(size, reverse=False) if fwd_table else anchors).to(dt).reshape(9, 2)
    b = bbox.to(dt)
    if not no_clamp:
        b = b.clamp(0.0, float(size - 1))
    fs = torch.tensor(float(size), dtype=dt)
    cx, cy = (b[:, 0] + b[:, 2]) / (2.0 * fs), (b[:, 1] + b[:, 3]) / (2.0 * fs)
    w, h = (b[:, 2] - b[:, 0]) / fs, (b[:, 3] - b[:, 1]) / fs
    eps = torch.tensor(EPS16_F, dtype=dt)
    ious = []
    for s in range(3):
        gw, gh = w * G[s], h * G[s]
        for a in range(3):
            aw, ah = an[s * 3 + a]
            inter = torch.minimum(gw, aw).clamp_min(0.0) * torch.minimum(gh, ah).clamp_min(0.0)
            ious.append(inter / (gw * gh + aw * ah - inter + eps))
    ious = torch.stack(ious, 1)                                   # (N, 9)
    top = ious.max(1, keepdim=True)[0]
    first = (ious == top).to(torch.int64).argmax(1)
    last = 8 - (ious == top).flip(1).to(torch.int64).argmax(1)
    bn = last if last_max else first
    top2 = ious.topk(2, dim=1)[0]
    iou_gap = (top2[:, 0] - top2[:, 1]) / top2[:, 0].clamp_min(1e-300)
    s = bn // 3
    g = torch.tensor(G)[s]
    gx, gy, gw, gh = cx * g, cy * g, w * g, h * g
    gi = (torch.floor(gx + 0.5) if round_g else torch.trunc(gx)).to(torch.int64)
    gj = (torch.floor(gy + 0.5) if round_g else torch.trunc(gy)).to(torch.int64)
    cell = torch.tensor(off)[s] + (gi * g + gj if cell_swap else gj * g + gi)
    ai = bn % 3 if tw_scale0 else bn
    argw, argh = gw / an[ai, 0] + eps, gh / an[ai, 1] + eps
    tx, ty, tw, th = gx - gi.to(dt), gy - gj.to(dt), torch.log(argw), torch.log(argh)
    tf = torch.stack([tx, ty, tw, th], 1)
    sc = torch.stack([gx.abs(), gy.abs(), (gw / an[ai, 0]) / argw + tw.abs(), (gh / an[ai, 1]) / argh + th.abs()], 1).to(F64)
    gxy = torch.stack([gx, gy], 1).to(F64)
    fr = gxy - torch.floor(gxy)
    frac = torch.where(gxy == 0, torch.full_like(gxy, float("inf")), torch.minimum(fr, 1 - fr) / gxy.abs().clamp_min(1e-300))
    ti = torch.stack([bn, gi, gj, cell], 1).to(torch.int32)
    return dict(ti=ti, tf=(tf, sc), iou_gap=iou_gap.to(F64), frac=frac)


def target_dense(ti, tf, size):
    """The reference's dense tensors by a numpy scatter: box[s] (N,3,5,g,g), ctr[s] (N,5,g,g), float32, zeros included."""
    N = ti.shape[0]
    G = grids(size)
    box = [np.zeros((N, 3, 5, g, g), np.float32) for g in G]; ctr = [np.zeros((N, 5, g, g), np.float32) for g in G]
    t_i, t_f = ti.numpy(), tf.numpy().astype(np.float32)
    for n in range(N):
        bn, gi, gj = int(t_i[n, 0]), int(t_i[n, 1]), int(t_i[n, 2])
        v = np.concatenate([t_f[n], np.ones(1, np.float32)])
        box[bn // 3][n, bn % 3, :, gj, gi] = v
        ctr[bn // 3][n, :, gj, gi] = v
    return [torch.from_numpy(x) for x in box], [torch.from_numpy(x) for x in ctr]


# ---- dense losses ------------------------------------------------------------------------------------------------------------------------
def _conf(outbox, dt, conf_sca=False):
    """(N, 3P): the confidence logits concatenated as scale, anchor, cell."""
    N = outbox[0].shape[0]
    cols = []
    for ob in outbox:
        c = ob.to(dt).reshape(N, 3, 5, -1)[:, :, 4]                # (N, 3, gg)
        cols.append((c.permute(0, 2, 1) if conf_sca else c).reshape(N, -1))
    return torch.cat(cols, 1)


def _flat(maps, dt):
    N = maps[0].shape[0]
    return torch.cat([m.to(dt).reshape(N, -1) for m in maps], 1)


def _lse(x, dt, no_max=False):
    """Row-wise log-sum-exp with its scale."""
    if no_max:
        e = torch.exp(x).to(F32).to(dt)
        v = torch.log(e.sum(1))
        return v, v.abs().to(F64) + 1.0
    m = x.max(1, keepdim=True)[0]
    d = x - m
    e = torch.exp(d)
    S = e.sum(1)
    v = torch.log(S) + m[:, 0]
    sc = m[:, 0].abs() + torch.log(S).abs() + (e * (1.0 + d.abs())).sum(1) / S + 1.0
    return v, sc.to(F64)


def _positions(ti, size):
    """Per sample: scale, anchor, gi, gj, cells per scale gg, index of the positive confidence among the 3P, flat cell."""
    G, (off, _) = grids(size), offsets(size)
    t = ti.to(torch.int64)
    bn, gi, gj, cell = t[:, 0], t[:, 1], t[:, 2], t[:, 3]
    s, a = bn // 3, bn % 3
    g = torch.tensor(G)[s]
    jpos = 3 * torch.tensor(off)[s] + a * g * g + gj * g + gi
    return s, a, gi, gj, g, jpos, cell


def _coords(outbox, ti, size, dt):
    """(N, 4): the four coordinate logits of the positive cell."""
    s, a, gi, gj, g, _, _ = _positions(ti, size)
    N = ti.shape[0]
    return torch.stack([outbox[int(s[n])].to(dt).reshape(N, 3, 5, int(g[n]), int(g[n]))[n, int(a[n]), :4, int(gj[n]), int(gi[n])] for n in range(N)])


def _partner(N, partner_next):
    ar = torch.arange(N)
    return (ar + 1) % N if partner_next else N - 1 - ar


def _hinges(sim, negsim, ti, size, dt, partner_next=False, neg_partner=False, margin=MARGIN_F):
    """The two hinge arguments per sample and the sum of the absolute terms of each."""
    N = ti.shape[0]
    cell = ti[:, 3].to(torch.int64)
    cell_o = cell[_partner(N, partner_next)]
    S, NS = _flat(sim, dt), _flat(negsim, dt)
    ar = torch.arange(N)
    pp, n1 = S[ar, cell], NS[ar, cell]
    n2 = (NS if neg_partner else S)[ar, cell_o]
    mg = torch.tensor(margin, dtype=dt)
    a1, a2 = (mg + n1) - pp, (mg + n2) - pp
    s1, s2 = mg + n1.abs() + pp.abs(), mg + n2.abs() + pp.abs()
    return a1, a2, s1.to(F64), s2.to(F64), cell, cell_o


def dense_fwd(outbox, sim, negsim, loc, ti, tf, size, dt=F64, conf_sca=False, no_max=False, partner_next=False, neg_partner=False,
              rank_n=False, no_wcoord=False, sig_tw=False, margin=MARGIN_F):
    """outbox[s] (N,15,g,g), sim / negsim / loc [s] (N,g,g) f32, ti (N,4) int32, tf (N,4) f32 ->
    lse (N,2), vals (N,8) = squared coordinate errors (4), CE(conf), CE(loc), rank term, 0;  out (3,) = yolo, rank, loc.
    hinge (N,2): |hinge argument| over the sum of its absolute terms, for the guard band."""
    N = ti.shape[0]
    ar = torch.arange(N)
    _, _, _, _, _, jpos, cell = _positions(ti, size)
    conf, L = _conf(outbox, dt, conf_sca), _flat(loc, dt)
    lse_c, sc_c = _lse(conf, dt, no_max)
    lse_l, sc_l = _lse(L, dt, no_max)
    t = _coords(outbox, ti, size, dt)
    tg = tf.to(dt)
    p = torch.stack([_sig(t[:, 0]), _sig(t[:, 1]), _sig(t[:, 2]) if sig_tw else t[:, 2], t[:, 3]], 1)
    d = p - tg
    v03 = d * d
    s03 = (2.0 * d.abs() * (p.abs() + tg.abs()) + v03).to(F64)
    cpos, lpos = conf[ar, jpos], L[ar, cell]
    v4, v5 = lse_c - cpos, lse_l - lpos
    s4, s5 = sc_c + cpos.abs().to(F64), sc_l + lpos.abs().to(F64)
    a1, a2, h1, h2, _, _ = _hinges(sim, negsim, ti, size, dt, partner_next, neg_partner, margin)
    v6 = a1.clamp_min(0.0) + a2.clamp_min(0.0)
    s6 = h1 * (a1 > 0) + h2 * (a2 > 0)
    zero = torch.zeros(N, dtype=dt)
    vals = torch.cat([v03, torch.stack([v4, v5, v6, zero], 1)], 1)
    sv = torch.cat([s03, torch.stack([s4, s5, s6, zero.to(F64)], 1)], 1)
    inv = torch.tensor(1.0, dtype=dt) / N
    tot, st = vals.sum(0), sv.sum(0)
    if no_wcoord:
        yolo = ((tot[0] * inv + tot[1] * inv) * 5.0 + (tot[2] * inv + tot[3] * inv)) + tot[4] * inv
    else:
        yolo = (((tot[0] * inv + tot[1] * inv) + tot[2] * inv) + tot[3] * inv) * 5.0 + tot[4] * inv
    rank = tot[6] / (N if rank_n else 2 * N)
    out = torch.stack([yolo, rank, tot[5] * inv])
    so = torch.stack([st[:4].sum() * 5.0 / N + st[4] / N, st[6] / (2 * N), st[5] / N])
    return dict(lse=(torch.stack([lse_c, lse_l], 1), torch.stack([sc_c, sc_l], 1)), vals=(vals, sv), out=(out, so),
                hinge=torch.stack([a1.abs().to(F64) / h1, a2.abs().to(F64) / h2], 1))


def dense_bwd(outbox, sim, negsim, loc, ti, tf, lse, gup, size, dt=F64, no_softmax=False, store_o=False, swap_up=False, no_dsig=False,
              partner_next=False, neg_partner=False, margin=MARGIN_F):
    """Gradients of gup . (yolo, rank, loc) on the forward's own lse (N,2): d_outbox[s], d_sim[s], d_negsim[s], d_loc[s], each (value,
    scale) in the inputs' shapes."""
    N = ti.shape[0]
    G, (off, P) = grids(size), offsets(size)
    ar = torch.arange(N)
    s_, a_, gi_, gj_, g_, jpos, cell = _positions(ti, size)
    up = gup.to(dt)
    if swap_up:
        up = up[[0, 2, 1]]
    gy, gr, gl = up[0] / N, up[1] / (2 * N), up[2] / N
    ls = lse.to(dt)
    # confidence and location: softmax - onehot
    conf, L = _conf(outbox, dt), _flat(loc, dt)
    dc_ = conf - ls[:, 0:1]; dl_ = L - ls[:, 1:2]
    ec, el = torch.exp(dc_), torch.exp(dl_)
    dconf = torch.zeros_like(conf) if no_softmax else gy * ec
    sconf = torch.zeros(conf.shape, dtype=F64) if no_softmax else (gy.abs() * (ec * (1.0 + dc_.abs()))).to(F64) + TINY * float(gy != 0)
    dloc = gl * el
    sloc = (gl.abs() * (el * (1.0 + dl_.abs()))).to(F64) + TINY * float(gl != 0)
    dconf[ar, jpos] = dconf[ar, jpos] - gy; sconf[ar, jpos] += float(gy.abs())
    dloc[ar, cell] = dloc[ar, cell] - gl; sloc[ar, cell] += float(gl.abs())
    # coordinates of the positive cell
    t = _coords(outbox, ti, size, dt)
    tg = tf.to(dt)
    p0 = _sig(t[:, :2])
    d0 = p0 - tg[:, :2]
    k = gy * 10.0
    if no_dsig:
        dxy = k * d0
        sxy = (k.abs() * (p0 + tg[:, :2].abs())).to(F64)
    else:
        dxy = k * d0 * p0 * (1.0 - p0)
        sxy = (k.abs() * ((p0 + tg[:, :2].abs()) * p0 * (1.0 - p0) + d0.abs() * p0 * (1.0 + p0))).to(F64) + TINY * float(gy != 0)
    dwh = k * (t[:, 2:] - tg[:, 2:])
    swh = (k.abs() * (t[:, 2:].abs() + tg[:, 2:].abs())).to(F64)
    dco = torch.cat([dxy, dwh], 1); sco = torch.cat([sxy, swh], 1)
    d_ob, c0 = [], 0
    for s, g in enumerate(G):
        gg = g * g
        v = torch.zeros(N, 3, 5, gg, dtype=dt); sc = torch.zeros(N, 3, 5, gg, dtype=F64)
        v[:, :, 4] = dconf[:, c0:c0 + 3 * gg].reshape(N, 3, gg); sc[:, :, 4] = sconf[:, c0:c0 + 3 * gg].reshape(N, 3, gg)
        for n in range(N):
            if int(s_[n]) == s:
                c = int(gj_[n]) * g + int(gi_[n])
                v[n, int(a_[n]), :4, c] = dco[n]; sc[n, int(a_[n]), :4, c] = sco[n]
        d_ob.append((v.reshape(N, 15, g, g), sc.reshape(N, 15, g, g)))
        c0 += 3 * gg
    # rank: the sparse rows of d_sim, d_negsim
    a1, a2, _, _, cell, cell_o = _hinges(sim, negsim, ti, size, dt, partner_next, neg_partner, margin)
    zero = torch.zeros((), dtype=dt)
    w1, w2 = torch.where(a1 > 0, gr, zero), torch.where(a2 > 0, gr, zero)
    dS = torch.zeros(N, P, dtype=dt); sS = torch.zeros(N, P, dtype=F64); dN = torch.zeros(N, P, dtype=dt); sN = torch.zeros(N, P, dtype=F64)
    dS[ar, cell] = dS[ar, cell] - (w1 + w2); sS[ar, cell] += (w1 + w2).abs().to(F64)
    if store_o:
        dS[ar, cell_o] = w2
    else:
        dS[ar, cell_o] = dS[ar, cell_o] + w2
    sS[ar, cell_o] += w2.abs().to(F64)
    dN[ar, cell] = w1; sN[ar, cell] = w1.abs().to(F64)

    def split(v, sc):
        return [(v[:, off[s]:off[s] + g * g].reshape(N, g, g), sc[:, off[s]:off[s] + g * g].reshape(N, g, g)) for s, g in enumerate(G)]
    return dict(d_outbox=d_ob, d_sim=split(dS, sS), d_negsim=split(dN, sN), d_loc=split(dloc, sloc))


# ---- InfoNCE rows ------------------------------------------------------------------------------------------------------------------------
def _cos(q, pos, neg, T, dt, no_eps, times_t, cut768, stride_m1):
    R, E = q.shape
    M = neg.shape[1]
    q, pos, neg = q.to(dt), pos.to(dt), neg.to(dt)
    if stride_m1:
        flat = neg.reshape(R * M, E)
        neg = flat[(torch.arange(R).view(-1, 1) * (M - 1) + torch.arange(M).view(1, -1))]
    x = torch.cat([pos.unsqueeze(1), neg], 1)                     # (R, 1+M, E)
    if cut768:
        q = q.clone(); x = x.clone(); q[:, 768:] = 0; x[:, :, 768:] = 0
    nq = (q * q).sum(1).sqrt(); nx = (x * x).sum(2).sqrt()
    if not no_eps:
        nq = nq.clamp_min(EPS12_F); nx = nx.clamp_min(EPS12_F)
    invT = torch.tensor(T, dtype=dt) if times_t else torch.tensor(1.0, dtype=dt) / torch.tensor(T, dtype=dt)
    dot = torch.einsum("re,rme->rm", q, x)
    adot = torch.einsum("re,rme->rm", q.abs(), x.abs())
    c = dot / nq.unsqueeze(1) / nx
    sc_c = (adot / nq.unsqueeze(1) / nx + 2.0 * c.abs()).to(F64)     # the two norms carry half a relative unit of their own sums each
    return q, x, nq, nx, invT, c, sc_c


def contrastive_fwd(q, pos, neg, T, dt=F64, no_eps=False, times_t=False, cut768=False, stride_m1=False, mean_all=False, no_proj=False):
    """q, pos (R,E), neg (R,M,E) f32 -> loss = mean_r (logsumexp_i s_i - s_0), s = cos / T;  rows (R,) the per-row terms."""
    R, M = q.shape[0], neg.shape[1]
    _, _, _, _, invT, c, sc_c = _cos(q, pos, neg, T, dt, no_eps, times_t, cut768, stride_m1)
    s = c * invT
    ss = sc_c * float(invT) + s.abs().to(F64)
    m = s.max(1, keepdim=True)[0]
    e = torch.exp(s - m)
    S = e.sum(1)
    p = (e / S.unsqueeze(1)).to(F64)
    row = torch.log(S) + m[:, 0] - s[:, 0]
    srow = (p * ss).sum(1) + ss[:, 0] + torch.log(S).abs().to(F64) + m[:, 0].abs().to(F64) + s[:, 0].abs().to(F64) + 1.0
    den = R * (M + 1) if mean_all else R
    return dict(rows=(row, srow), loss=(row.sum() / den, srow.sum() / R))


def contrastive_bwd(q, pos, neg, T, gup, dt=F64, no_eps=False, times_t=False, cut768=False, stride_m1=False, mean_all=False, no_proj=False):
    """Gradients of gup[0] * loss: dq, dpos (R,E), dneg (R,M,E).  The clamped norm is the constant it is."""
    R, E = q.shape
    M = neg.shape[1]
    qq, x, nq, nx, invT, c, sc_c = _cos(q, pos, neg, T, dt, no_eps, times_t, cut768, stride_m1)
    s = c * invT
    ss = sc_c * float(invT) + s.abs().to(F64)
    m = s.max(1, keepdim=True)[0]
    e = torch.exp(s - m)
    p = e / e.sum(1, keepdim=True)
    up = gup.to(dt)[0] / (R * (M + 1) if mean_all else R)
    onehot = torch.zeros_like(p); onehot[:, 0] = 1.0
    gx = (p - onehot) * up * invT                                  # (R, 1+M)
    p64 = p.to(F64)
    sg = gx.abs().to(F64) + abs(float(up * invT)) * p64 * (ss + (p64 * ss).sum(1, keepdim=True))
    qh = qq / nq.unsqueeze(1); xh = x / nx.unsqueeze(2)
    cq = c.unsqueeze(2)
    dx = gx.unsqueeze(2) * (qh.unsqueeze(1) - xh * cq) / nx.unsqueeze(2)
    sdx = (sg.unsqueeze(2) * (qh.abs().unsqueeze(1) + (xh * cq).abs()).to(F64) + (gx.abs().unsqueeze(2) * xh.abs()).to(F64) * sc_c.unsqueeze(2)) \
        / nx.unsqueeze(2).to(F64)
    proj = torch.zeros_like(xh) if no_proj else qh.unsqueeze(1) * cq
    dq = (gx.unsqueeze(2) * (xh - proj)).sum(1) / nq.unsqueeze(1)
    sdq = (sg.unsqueeze(2) * (xh.abs() + (qh.unsqueeze(1) * cq).abs()).to(F64)
           + (gx.abs().unsqueeze(2) * qh.abs().unsqueeze(1)).to(F64) * sc_c.unsqueeze(2)).sum(1) / nq.unsqueeze(1).to(F64)
    if stride_m1:                                                  # the gradient lands on the rows that were read
        dneg = torch.zeros(R * M, E, dtype=dt); idx = (torch.arange(R).view(-1, 1) * (M - 1) + torch.arange(M).view(1, -1)).reshape(-1)
        dneg[idx] = dx[:, 1:].reshape(R * M, E)
        dneg = dneg.reshape(R, M, E)
    else:
        dneg = dx[:, 1:]
    live = (sdx > 0).to(F64)
    return dict(dq=(dq, sdq + TINY), dpos=(dx[:, 0], sdx[:, 0] + TINY * live[:, 0]), dneg=(dneg, sdx[:, 1:] + TINY * live[:, 1:]))


# ---- evaluation decode -------------------------------------------------------------------------------------------------------------------
def first_max(row, last=False):
    """torch.max over a float vector: the first NaN if there is one, else the first (or, wrongly, the last) maximum."""
    row = np.asarray(row)
    nan = np.flatnonzero(np.isnan(row))
    if nan.size:
        return int(nan[-1] if last else nan[0])
    hit = np.flatnonzero(row == row.max())
    return int(hit[-1] if last else hit[0])


def decode(outbox, anchors, size, dt=F64, last_max=False, swap_wh=False, stride0=False, full_ext=False):
    """outbox[s] (N,15,g,g) f32 -> cellinfo (N,3) int32 = scale * 3 + anchor, gi, gj of the arg-max confidence;  boxes (N,4) xyxy.
    gap (N,): top-2 gap of the confidences over the largest magnitude (for the guard band; NaN rows give 0)."""
    N = outbox[0].shape[0]
    G = grids(size)
    conf = _conf(outbox, F64).numpy()
    an = anchors.to(dt)
    cells, boxes, scales, gaps = [], [], [], []
    for n in range(N):
        j = first_max(conf[n], last_max)
        s = 0
        while s < 2 and j >= 3 * G[s] * G[s]:
            j -= 3 * G[s] * G[s]; s += 1
        g = G[s]; gg = g * g
        a, cell = j // gg, j % gg
        gj, gi = cell // g, cell % g
        t = outbox[s].to(dt).reshape(N, 3, 5, gg)[n, a, :, cell]
        stride = float(32 if stride0 else size // g)
        aw, ah = (an[s, a, 1], an[s, a, 0]) if swap_wh else (an[s, a, 0], an[s, a, 1])
        x, y = (_sig(t[0]) + gi) * stride, (_sig(t[1]) + gj) * stride
        w, h = torch.exp(t[2]) * aw * stride, torch.exp(t[3]) * ah * stride
        hw, hh = (w, h) if full_ext else (w / 2.0, h / 2.0)
        boxes.append(torch.stack([x - hw, y - hh, x + hw, y + hh]))
        scales.append(torch.stack([x.abs() + w.abs(), y.abs() + h.abs(), x.abs() + w.abs(), y.abs() + h.abs()]).to(F64) + TINY)
        cells.append([s * 3 + a, gi, gj])
        top = np.sort(conf[n])[-2:] if conf.shape[1] > 1 else np.array([conf[n, 0] - 1, conf[n, 0]])
        gaps.append(float((top[1] - top[0]) / max(abs(top[1]), abs(top[0]), 1e-300)) if np.isfinite(top).all() else 0.0)
    return dict(cellinfo=torch.tensor(cells, dtype=torch.int32), boxes=(torch.stack(boxes), torch.stack(scales)), gap=torch.tensor(gaps, dtype=F64))


# ---- box IoU -----------------------------------------------------------------------------------------------------------------------------
def box_iou(b1, b2, dt=F64, no_inter=False, no_clamp=False):
    a, b = b1.to(dt), b2.to(dt)
    iw = torch.minimum(a[:, 2], b[:, 2]) - torch.maximum(a[:, 0], b[:, 0])
    ih = torch.minimum(a[:, 3], b[:, 3]) - torch.maximum(a[:, 1], b[:, 1])
    if not no_clamp:
        iw, ih = iw.clamp_min(0.0), ih.clamp_min(0.0)
    inter = iw * ih
    a1, a2 = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]), (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    den = a1 + a2 - (0.0 if no_inter else inter) + torch.tensor(EPS16_F, dtype=dt)
    iou = inter / den
    sc = iou.abs() * (4.0 + 3.0 * (a1.abs() + a2.abs() + inter.abs()) / den.abs())
    return dict(iou=(iou, sc.to(F64)))
