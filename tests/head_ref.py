"""Stage-by-stage restatement of the cross-scale head tail (dcnet_amd/csrc/head.hip, csrc/locmod.hip) in torch on the CPU, float64 by
default: one function per kernel, in the rank-8 forms of the kernels' header comments (no P x P tensor is ever built).  No GPU.

Every input is the float32 tensor (float64 for the moments) the kernel itself receives, so neither upstream rounding nor the
amplification of the min-max normalisation enters a comparison.  Every function returns a dict  name -> (value, scale):  `scale` is,
per element, the sum of the absolute values of the terms that were added into it (propagated to first order through quotients and
square roots), the unit in which an error of that element is judged.  scale == 0 marks an element that must be reproduced exactly
(copies, structural zeros).  `dt=torch.float32` evaluates the same formulas in fp32: the yardstick r32 of head_cases.head_tol.

The keyword arguments select deliberately WRONG variants; tests/test_head_ref_host.py shows that the cases of tests/head_cases.py tell
each of them from the right answer.

  locemb_fwd        biased            (a) running_var of BatchNorm1d(8) from the biased variance
                    count_p           (b) Bessel's factor from count = P instead of B P
  locbn_fwd         biased            (c) running_var of BatchNorm1d(512) from the biased variance
                    count_p           (d) Bessel's factor from count = P instead of B P
                    no_bias_rm        (e) running_mean without the Linear bias
                    no_bscale         (n) eval-mode b' without the b * scale term
  head_final_fwd    no_eps            (f) min-max denominator without the 1e-6
                    tie="last"        (g) last index instead of first on ties of the minimum / maximum
                    box_mod           (k) conf * sim * loc applied to a box channel as well
                    swap              (m) scales concatenated in the order 1, 0, 2
  head_dloc         no_eps            (f) as above
                    drop="min"        (h) the d/dmin term dropped
                    drop="max"        (o) the d/dmax term dropped
                    misplace          (i) the d/dmin term added at arg-max and the d/dmax term at arg-min
                    swap              (m)
  head_obj          div3=False        (j) the / 3 of the anchor mean dropped
                    pad_nonzero       (p) non-zero pad columns in X
                    swap              (m)
  head_dlogits      div3=False        (j)
                    pad_nonzero       (q) non-zero pad channels in dlogits
                    box_mod           (k)
                    swap              (m)
  locemb_bwd        mask_ge           (l) ReLU mask y >= 0 instead of y > 0
  locmod_bwd        mask_ge           (l)
"""
import torch

F64 = torch.float64
F32 = torch.float32
U = 2.0 ** -24                               # unit roundoff of fp32
U64 = 2.0 ** -53
EPS6 = 9.999999974752427e-07                 # float32(1e-6): the constant the fp32 model adds to the min-max denominator
NORM_EPS = 1e-12


def _a(x):
    return x.abs()


def order(swap):
    return (1, 0, 2) if swap else (0, 1, 2)


def cat_scales(xs, swap=False):
    """Per-scale (B, hw_s) tensors -> (B, P) in concatenation order."""
    return torch.cat([xs[s] for s in order(swap)], 1)


def split_scales(x, hws, swap=False):
    """(B, P) -> per-scale list, undoing cat_scales."""
    out, off = [None] * 3, 0
    for s in order(swap):
        out[s] = x[:, off:off + hws[s]]; off += hws[s]
    return out


def _flat(t, dt):
    """logits (B,H,W,ld) -> (B, hw, ld) in dt"""
    return t.to(dt).reshape(t.shape[0], -1, t.shape[-1])


def _opt(ts, s, dt):
    return None if ts is None or ts[s] is None else ts[s].to(dt)


def _running(old, new, s_new, momentum):
    """Updated running statistic and its scale |retained| + |update|.  The generators of head_cases.py keep the retained part below the
    update wherever the update is not zero, so the comparison is relative to the update term within a factor of two."""
    return (1.0 - momentum) * old + momentum * new, _a((1.0 - momentum) * old) + momentum * s_new


# ---- location embedding -----------------------------------------------------------------------------------------------------------
def _le_rows(y, s_y):
    """relu + L2-normalise over the 8 channels of rows y with scale s_y: E8, its scale, the clamped norm, z."""
    z = torch.relu(y)
    live = (y > 0).to(y.dtype)
    nrm = (z * z).sum(1, keepdim=True).sqrt()
    den = nrm.clamp_min(NORM_EPS)
    e = z / den
    s_z = s_y * live
    s_e = s_z / den + _a(e) * ((_a(e) * s_z).sum(1, keepdim=True) + nrm) / den
    return e, s_e, den, z


def locemb_fwd(coord, W, b, gamma, beta, rm, rv, training, count, momentum, eps, dt=F64, biased=False, count_p=False):
    """coord (P,8) -> Linear(8,8) -> BatchNorm1d(8) over the rows -> ReLU -> L2-normalise.  Keys: E8, xh, stat (mean | rstd), and
    in train mode rm, rv (the updated running statistics; their scale: _running)."""
    c, W, b, g, be = (x.to(dt) for x in (coord, W, b, gamma, beta))
    P = c.shape[0]
    ce = c @ W.t() + b
    s_ce = _a(c) @ _a(W).t() + _a(b)
    out = {}
    if training:
        mean = ce.mean(0); var = ((ce - mean) ** 2).mean(0)
        s_mean = s_ce.mean(0)
        cnt = float(P if count_p else count)
        bess = 1.0 if biased else cnt / (cnt - 1.0)
        out["rm"] = _running(rm.to(dt), mean, s_mean, momentum)
        out["rv"] = _running(rv.to(dt), var * bess, var * bess, momentum)
        s_var = 2.0 * (_a(ce - mean) * (s_ce + s_mean)).mean(0)
    else:
        mean, var = rm.to(dt), rv.to(dt)
        s_mean = _a(mean); s_var = _a(var)
    rstd = (var + eps).rsqrt()
    s_rstd = rstd * (1.0 + 0.5 * s_var / (var + eps))
    xh = (ce - mean) * rstd
    s_xh = (s_ce + s_mean) * rstd + _a(xh) * s_rstd / rstd
    y = g * xh + be
    e, s_e, _, _ = _le_rows(y, _a(g) * s_xh + _a(be))
    out.update(E8=(e, s_e), xh=(xh, s_xh), stat=(torch.cat([mean, rstd]), torch.cat([s_mean, s_rstd])))
    return out


def moments(e8):
    """mom[72] = sum_p E8_p | sum_p E8_p E8_p^T, in float64 from the given (the device's own) E8; scale = the sums of |terms|."""
    e = e8.to(F64)
    return torch.cat([e.sum(0), (e.t() @ e).reshape(-1)]), torch.cat([_a(e).sum(0), (_a(e).t() @ _a(e)).reshape(-1)])


def moments_exact(e8):
    """The same 72 sums, correctly rounded: the products of two float32 values are exact in float64 and math.fsum adds without error,
    so an error against this is the device's alone (a float64 sum of 8192 terms in torch carries tens of 2**-53 of its own)."""
    import math
    e = e8.to(F64)
    cols = [e[:, k].tolist() for k in range(8)]
    prods = [(e[:, k] * e[:, j]).tolist() for k in range(8) for j in range(8)]
    return torch.tensor([math.fsum(c) for c in cols] + [math.fsum(p) for p in prods], dtype=F64), moments(e8)[1]


def locemb_bwd(coord, W, gamma, beta, xh, stat, dEa, dEb, dmom, training, dt=F64, mask_ge=False):
    """grads [88] = dW (64) | db (8) | dgamma (8) | dbeta (8) of the location embedding, given d(E8) = dEa + dEb and d(moments).
    Also `y`, the BatchNorm output whose sign is the ReLU mask, with its scale (for the guard band)."""
    c, W, g, be, x = (t.to(dt) for t in (coord, W, gamma, beta, xh))
    rstd = stat.to(dt)[8:]
    P = c.shape[0]
    y = g * x + be
    s_y = _a(g * x) + _a(be)
    z = torch.relu(y)
    den = (z * z).sum(1, keepdim=True).sqrt().clamp_min(NORM_EPS)
    e = z / den
    dE = torch.zeros_like(e); s_dE = torch.zeros_like(e)
    if dmom is not None:
        dm = dmom.to(dt); d1 = dm[:8]; d2 = dm[8:].view(8, 8); sym = d2 + d2.t()
        dE = dE + d1 + e @ sym.t(); s_dE = s_dE + _a(d1) + _a(e) @ _a(sym).t()
    for t in (dEa, dEb):
        if t is not None:
            dE = dE + t.to(dt); s_dE = s_dE + _a(t.to(dt))
    mask = ((y >= 0) if mask_ge else (y > 0)).to(dt)
    dot = (dE * e).sum(1, keepdim=True)
    dy = mask * (dE - e * dot) / den
    s_dy = mask * (s_dE + _a(e) * (s_dE * _a(e)).sum(1, keepdim=True)) / den
    dgamma = (dy * x).sum(0); dbeta = dy.sum(0)
    s_dgamma = (s_dy * _a(x)).sum(0); s_dbeta = s_dy.sum(0)
    d, s_d = dy, s_dy
    if training:
        d = dy - dbeta / P - x * dgamma / P
        s_d = s_dy + s_dbeta / P + _a(x) * s_dgamma / P
    d = d * g * rstd; s_d = s_d * _a(g * rstd)
    dW = d.t() @ c; s_dW = s_d.t() @ _a(c)
    return dict(grads=(torch.cat([dW.reshape(-1), d.sum(0), dgamma, dbeta]), torch.cat([s_dW.reshape(-1), s_d.sum(0), s_dgamma, s_dbeta])),
                y=(y, s_y))


# ---- objectness map and the rank-8 GEMM operand ------------------------------------------------------------------------------------
def _only_obj(l, div3):
    a = l[..., 4] + l[..., 9] + l[..., 14]; s = _a(l[..., 4]) + _a(l[..., 9]) + _a(l[..., 14])
    return (a / 3.0, s / 3.0) if div3 else (a, s)


def head_obj(logits, sims, e8, dt=F64, div3=True, swap=False, pad_nonzero=False):
    """Keys: only[s] (B,hw_s), obj_map (B,P), objn (B,), X (B*8, Ppad)."""
    B = logits[0].shape[0]
    e = e8.to(dt)
    oo = [_only_obj(_flat(l, dt), div3) for l in logits]
    sm = [s.to(dt).reshape(B, -1) for s in sims]
    obj = cat_scales([o[0] * s for o, s in zip(oo, sm)], swap)
    s_obj = cat_scales([o[1] * _a(s) for o, s in zip(oo, sm)], swap)
    P = obj.shape[1]; Ppad = (P + 31) // 32 * 32
    nrm = (obj * obj).sum(1, keepdim=True).sqrt()
    den = nrm.clamp_min(NORM_EPS)
    om = obj / den
    s_nrm = (_a(om) * s_obj).sum(1, keepdim=True) + nrm
    s_om = s_obj / den + _a(om) * s_nrm / den
    X = torch.zeros(B, 8, Ppad, dtype=dt); s_X = torch.zeros(B, 8, Ppad, dtype=dt)
    X[:, :, :P] = e.t().unsqueeze(0) * om.unsqueeze(1); s_X[:, :, :P] = _a(e).t().unsqueeze(0) * s_om.unsqueeze(1)
    if pad_nonzero and Ppad > P:
        X[:, :, P:] = X[:, :, P - 1:P]
    out = dict(obj_map=(om, s_om), objn=(nrm[:, 0], s_nrm[:, 0]), X=(X.reshape(B * 8, Ppad), s_X.reshape(B * 8, Ppad)))
    for s in range(3):
        out[f"only{s}"] = oo[s]
    return out


def head_fold(dX, e8, obj_map, dt=F64):
    """dX (B*8,Ppad) -> dobj_map[n,p] = sum_k dX e8[p,k];  dE8x[p,k] = sum_n dX obj_map[n,p]."""
    B, P = obj_map.shape
    d = dX.to(dt).view(B, 8, -1)[:, :, :P]; e = e8.to(dt); om = obj_map.to(dt)
    dobj = torch.einsum("nkp,pk->np", d, e); s_dobj = torch.einsum("nkp,pk->np", _a(d), _a(e))
    de = torch.einsum("nkp,np->pk", d, om); s_de = torch.einsum("nkp,np->pk", _a(d), _a(om))
    return dict(dobj_map=(dobj, s_dobj), dE8x=(de, s_de))


# ---- BatchNorm1d(512) of the relation embedding from the moments ----------------------------------------------------------------------
def locbn_fwd(M, mom, b, gamma, beta, rm, rv, training, count, momentum, eps, dt=F64, biased=False, count_p=False, no_bias_rm=False,
              no_bscale=False):
    """M (B,8,512), mom [72] float64.  Keys: Mp, bp, saved ([3][512]: r | mu' | scale), and in train mode rm, rv."""
    M, b, g, be = (x.to(dt) for x in (M, b, gamma, beta))
    B = M.shape[0]
    mo = mom.to(dt); s1 = mo[:8]; S2 = mo[8:].view(8, 8)
    out = {}
    if training:
        t1 = torch.einsum("k,nkc->c", s1, M); s_t1 = torch.einsum("k,nkc->c", _a(s1), _a(M))
        q2 = torch.einsum("nkc,kj,njc->c", M, S2, M); s_q2 = torch.einsum("nkc,kj,njc->c", _a(M), _a(S2), _a(M))
        cnt = float(count)
        mu = t1 / cnt; s_mu = s_t1 / cnt
        var = (q2 / cnt - mu * mu).clamp_min(0.0); s_var = s_q2 / cnt + 2.0 * _a(mu) * s_mu
        bc = cnt / B if count_p else cnt
        bess = 1.0 if biased else bc / (bc - 1.0)
        r = (var + eps).rsqrt(); s_r = r * (1.0 + 0.5 * s_var / (var + eps))
        scale = g * r; s_scale = _a(g) * s_r
        bp = be - scale * mu; s_bp = _a(be) + s_scale * _a(mu) + _a(scale) * s_mu
        mean_t = mu if no_bias_rm else mu + b
        out["rm"] = _running(rm.to(dt), mean_t, _a(mu) + (0.0 if no_bias_rm else _a(b)), momentum)
        out["rv"] = _running(rv.to(dt), var * bess, var * bess, momentum)
        saved = torch.stack([r, mu, scale]); s_saved = torch.stack([s_r, s_mu, s_scale])
    else:
        rmean, rvar = rm.to(dt), rv.to(dt)
        r = (rvar + eps).rsqrt(); s_r = r * (1.0 + 0.5 * _a(rvar) / (rvar + eps))
        scale = g * r; s_scale = _a(g) * s_r
        bp = be - rmean * scale; s_bp = _a(be) + _a(rmean) * s_scale
        if not no_bscale:
            bp = bp + b * scale; s_bp = s_bp + _a(b) * s_scale
        saved = torch.stack([r, torch.zeros_like(r), scale]); s_saved = torch.stack([s_r, torch.zeros_like(r), s_scale])
    out.update(Mp=(M * scale, _a(M) * s_scale), bp=(bp, s_bp), saved=(saved, s_saved))
    return out


def locbn_bwd(M, mom, b, gamma, rmean, saved, dMp, dbp, training, count, dt=F64):
    """Keys: dM (B,8,512), out ([3][512]: dgamma | dbeta | db), and in train mode dmom [72] (float64 on the device)."""
    M, b, g, dMp, gb = (x.to(dt) for x in (M, b, gamma, dMp, dbp))
    sv = saved.to(dt); r, mu, scale = sv[0], sv[1], sv[2]
    A = (dMp * M).sum((0, 1)); s_A = _a(dMp * M).sum((0, 1))
    if not training:
        rm = rmean.to(dt)
        dgamma = (A + gb * (b - rm)) * r; s_dgamma = (s_A + _a(gb) * (_a(b) + _a(rm))) * r
        return dict(dM=(dMp * scale, torch.zeros_like(M) + _a(dMp * scale)),
                    out=(torch.stack([dgamma, gb, gb * scale]), torch.stack([s_dgamma, torch.zeros_like(gb), _a(gb * scale)])))
    mo = mom.to(dt); s1 = mo[:8]; S2 = mo[8:].view(8, 8); sym = S2 + S2.t()
    cnt = float(count)
    core = A - gb * mu; s_core = s_A + _a(gb * mu)
    dgamma = r * core; s_dgamma = r * s_core
    dvar = -0.5 * r ** 3 * g * core; s_dvar = 0.5 * r ** 3 * _a(g) * s_core
    dmu = -g * r * gb - 2.0 * mu * dvar; s_dmu = _a(g * r * gb) + 2.0 * _a(mu) * s_dvar
    dq2 = dvar / cnt; dt1 = dmu / cnt; s_dq2 = s_dvar / cnt; s_dt1 = s_dmu / cnt
    u = torch.einsum("kj,njc->nkc", sym, M); s_u = torch.einsum("kj,njc->nkc", _a(sym), _a(M))
    dM = dMp * scale + dt1 * s1.view(1, 8, 1) + dq2 * u
    s_dM = _a(dMp * scale) + s_dt1 * _a(s1).view(1, 8, 1) + s_dq2 * s_u
    sm = M.sum(0); smm = torch.einsum("nkc,njc->kjc", M, M)
    dm = torch.cat([(sm * dt1).sum(1), (smm * dq2).sum(2).reshape(-1)])
    s_dm = torch.cat([(_a(M).sum(0) * s_dt1).sum(1), (torch.einsum("nkc,njc->kjc", _a(M), _a(M)) * s_dq2).sum(2).reshape(-1)])
    z = torch.zeros_like(gb)
    return dict(dM=(dM, s_dM), out=(torch.stack([dgamma, gb, z]), torch.stack([s_dgamma, z, z])), dmom=(dm, s_dm))


# ---- location module core ------------------------------------------------------------------------------------------------------------
def _locmod_rows(E, Mp, bp, q, dt):
    e, m, b, q = (x.to(dt) for x in (E, Mp, bp, q))
    v = torch.einsum("ik,nkc->nic", e, m) + b                              # (n, P, 512) pre-activation
    s_v = torch.einsum("ik,nkc->nic", _a(e), _a(m)) + _a(b)
    z = torch.relu(v)
    nrm = (z * z).sum(2, keepdim=True).sqrt()
    den = nrm.clamp_min(NORM_EPS)
    return e, m, q, v, s_v, z, nrm, den


def locmod_fwd(E, Mp, bp, q, dt=F64):
    """loc[n,i] = < normalize(relu(E_i . M'_n + b')), q_n >.  Keys: loc (n,P)."""
    e, m, q, v, s_v, z, nrm, den = _locmod_rows(E, Mp, bp, q, dt)
    qn = q.unsqueeze(1)
    s_z = s_v * (v > 0).to(dt)
    loc = (z * qn).sum(2, keepdim=True) / den
    s_loc = ((_a(qn) * s_z).sum(2, keepdim=True) + _a(z * qn).sum(2, keepdim=True)) / den \
        + _a(loc) * ((z / den * s_z).sum(2, keepdim=True) / den + 1.0)
    return dict(loc=(loc[..., 0], s_loc[..., 0]))


def locmod_bwd(E, Mp, bp, q, dloc, dt=F64, mask_ge=False):
    """Keys: dE_part (n,P,8), dsum (n,10,512: rows 0..7 dM', 8 db', 9 dq), and the pre-activation v with its scale (guard band)."""
    e, m, q, v, s_v, z, nrm, den = _locmod_rows(E, Mp, bp, q, dt)
    qn = q.unsqueeze(1)
    g = dloc.to(dt).unsqueeze(2)
    zh = z / den
    lv = (z * qn).sum(2, keepdim=True) / den
    mask = ((v >= 0) if mask_ge else (v > 0)).to(dt)
    # the recomputed forward quantities carry the rounding of the pre-activation (a sum that cancels) into zhat, the norm and loc
    s_z = s_v * (v > 0).to(dt)
    s_den = (zh * s_z).sum(2, keepdim=True) + nrm
    s_zh = s_z / den + _a(zh) * s_den / den
    s_lv = ((_a(qn) * s_z).sum(2, keepdim=True) + _a(z * qn).sum(2, keepdim=True)) / den + _a(lv) * s_den / den
    dz = mask * g / den * (qn - zh * lv)
    s_dz = mask * (_a(g) / den * (_a(qn) + s_zh * _a(lv) + _a(zh) * s_lv) + _a(dz) * s_den / den)
    dM = torch.einsum("ik,nic->nkc", e, dz); s_dM = torch.einsum("ik,nic->nkc", _a(e), s_dz)
    dsum = torch.cat([dM, dz.sum(1, keepdim=True), (g * zh).sum(1, keepdim=True)], 1)
    s_dsum = torch.cat([s_dM, s_dz.sum(1, keepdim=True), (_a(g) * s_zh).sum(1, keepdim=True)], 1)
    dE = torch.einsum("nkc,nic->nik", m, dz); s_dE = torch.einsum("nkc,nic->nik", _a(m), s_dz)
    return dict(dE_part=(dE, s_dE), dsum=(dsum, s_dsum), v=(v, s_v))


# ---- min-max normalisation, confidence modulation, NCHW store -------------------------------------------------------------------------------
def minmax_index(x, tie="first"):
    """(min, max, argmin, argmax) per row of x (B,P); the first occurrence wins on ties (tie="last": the last)."""
    mn = x.min(1)[0]; mx = x.max(1)[0]
    P = x.shape[1]
    ar = torch.arange(P).unsqueeze(0).expand_as(x)
    if tie == "first":
        imn = torch.where(x == mn.unsqueeze(1), ar, P).min(1)[0]; imx = torch.where(x == mx.unsqueeze(1), ar, P).min(1)[0]
    else:
        imn = torch.where(x == mn.unsqueeze(1), ar, -1).max(1)[0]; imx = torch.where(x == mx.unsqueeze(1), ar, -1).max(1)[0]
    return mn, mx, imn, imx


def head_final_fwd(logits, sims, loc_map, dt=F64, no_eps=False, tie="first", box_mod=False, swap=False):
    """Keys: mm (B,2: min, max; exact), imn, imx (int64), loc[s] (B,hw_s), outbox[s] (B,15,hw_s)."""
    B = logits[0].shape[0]
    x = loc_map.to(dt)
    hws = [l.shape[1] * l.shape[2] for l in logits]
    mn, mx, imn, imx = minmax_index(x, tie)
    mn_, mx_ = mn.unsqueeze(1), mx.unsqueeze(1)
    den = mx_ - mn_ + (0.0 if no_eps else EPS6)
    s_den = _a(mx_) + _a(mn_) + EPS6
    lc = (x - mn_) / den
    s_lc = (_a(x) + _a(mn_)) / den + _a(lc) * s_den / den
    out = dict(mm=(torch.stack([mn, mx], 1), torch.zeros(B, 2, dtype=dt)), imn=imn, imx=imx)
    lcs = split_scales(lc, hws, swap); s_lcs = split_scales(s_lc, hws, swap)
    for s in range(3):
        l = _flat(logits[s], dt)[..., :15]; sm = sims[s].to(dt).reshape(B, -1)
        mod = (sm * lcs[s]).unsqueeze(2); s_mod = (_a(sm) * s_lcs[s]).unsqueeze(2)
        conf = torch.zeros(15, dtype=torch.bool); conf[4::5] = True
        if box_mod:
            conf[0] = True
        ob = torch.where(conf, l * mod, l); s_ob = torch.where(conf, _a(l) * s_mod, torch.zeros_like(l))
        out[f"loc{s}"] = (lcs[s], s_lcs[s]); out[f"outbox{s}"] = (ob.permute(0, 2, 1), s_ob.permute(0, 2, 1))
    return out


def head_dloc(logits, sims, loc, d_outbox, d_loc, mm, imn, imx, dt=F64, no_eps=False, drop=None, misplace=False, swap=False):
    """d(loc_map) (B,P) from d(loc_score) and d(outbox) (either may be None per scale), through conf * sim * loc and the min-max
    normalisation.  loc[s] (B,hw_s), d_outbox[s] (B,15,hw_s), mm (B,>=2) the device's min | max, imn / imx (B,) int64."""
    B = logits[0].shape[0]
    dys, s_dys, ys = [], [], []
    for s in range(3):
        l = _flat(logits[s], dt); sm = sims[s].to(dt).reshape(B, -1)
        dy = torch.zeros_like(sm); s_dy = torch.zeros_like(sm)
        dl = _opt(d_loc, s, dt)
        if dl is not None:
            dy = dy + dl.reshape(B, -1); s_dy = s_dy + _a(dl.reshape(B, -1))
        do = _opt(d_outbox, s, dt)
        if do is not None:
            do = do.reshape(B, 15, -1)
            t = sum(do[:, ch] * l[..., ch] for ch in (4, 9, 14)); s_t = sum(_a(do[:, ch] * l[..., ch]) for ch in (4, 9, 14))
            dy = dy + t * sm; s_dy = s_dy + s_t * _a(sm)
        dys.append(dy); s_dys.append(s_dy); ys.append(loc[s].to(dt).reshape(B, -1))
    dy, s_dy, y = cat_scales(dys, swap), cat_scales(s_dys, swap), cat_scales(ys, swap)
    m = mm.to(dt)
    den = (m[:, 1] - m[:, 0] + (0.0 if no_eps else EPS6)).unsqueeze(1)
    out = dy / den; sc = s_dy / den
    a0 = dy.sum(1); a1 = (dy * y).sum(1); s0 = s_dy.sum(1); s1 = (s_dy * _a(y)).sum(1)
    dmn = (a1 - a0) / den[:, 0]; dmx = -a1 / den[:, 0]
    s_dmn = (s1 + s0) / den[:, 0]; s_dmx = s1 / den[:, 0]
    at_mn, at_mx = (imx, imn) if misplace else (imn, imx)
    add = torch.zeros_like(out); s_add = torch.zeros_like(out)
    ar = torch.arange(B)
    if drop != "min":
        add[ar, at_mn] += dmn; s_add[ar, at_mn] += s_dmn
    if drop != "max":
        add[ar, at_mx] += dmx; s_add[ar, at_mx] += s_dmx
    return dict(dloc_map=(out + add, sc + s_add))


def head_dlogits(logits, sims, loc, only, d_outbox, d_only, obj_map, objn, dobj_map, dt=F64, div3=True, pad_nonzero=False, box_mod=False,
                 swap=False):
    """Keys: dlogits[s] (B,hw_s,ld_s) with zero pad channels, dsim[s] (B,hw_s)."""
    B = logits[0].shape[0]
    hws = [l.shape[1] * l.shape[2] for l in logits]
    om = obj_map.to(dt)
    inv = 1.0 / objn.to(dt).clamp_min(NORM_EPS).unsqueeze(1)
    if dobj_map is None:
        dobj = torch.zeros_like(om); s_dobj = torch.zeros_like(om)
    else:
        dm = dobj_map.to(dt)
        dot = (dm * om).sum(1, keepdim=True); s_dot = _a(dm * om).sum(1, keepdim=True)
        dobj = (dm - om * dot) * inv; s_dobj = (_a(dm) + _a(om) * s_dot) * inv
    dobjs = split_scales(dobj, hws, swap); s_dobjs = split_scales(s_dobj, hws, swap)
    out = {}
    for s in range(3):
        l = _flat(logits[s], dt); sm = sims[s].to(dt).reshape(B, -1); lc = loc[s].to(dt).reshape(B, -1); oo = only[s].to(dt).reshape(B, -1)
        donly = dobjs[s] * sm; s_donly = s_dobjs[s] * _a(sm)
        dn = _opt(d_only, s, dt)
        if dn is not None:
            donly = donly + dn.reshape(B, -1); s_donly = s_donly + _a(dn.reshape(B, -1))
        ds = dobjs[s] * oo; s_ds = s_dobjs[s] * _a(oo)
        third, s_third = (donly / 3.0, s_donly / 3.0) if div3 else (donly, s_donly)
        dl = torch.zeros_like(l); s_dl = torch.zeros_like(l)
        do = _opt(d_outbox, s, dt)
        for ch in range(15):
            dv = torch.zeros_like(sm) if do is None else do.reshape(B, 15, -1)[:, ch]
            if ch % 5 == 4 or (box_mod and ch == 0):
                dl[..., ch] = dv * sm * lc; s_dl[..., ch] = _a(dv * sm * lc)
                if ch % 5 == 4:
                    dl[..., ch] += third; s_dl[..., ch] += s_third
                    ds = ds + dv * l[..., ch] * lc; s_ds = s_ds + _a(dv * l[..., ch] * lc)
            else:
                dl[..., ch] = dv
        if pad_nonzero and l.shape[-1] > 15:
            dl[..., 15:] = l[..., 15:]
        out[f"dlogits{s}"] = (dl, s_dl); out[f"dsim{s}"] = (ds, s_ds)
    return out


# ---- copies and column sums ---------------------------------------------------------------------------------------------------------------
def pad_rows(src, cols_out, dt=F64):
    rows, cols = src.shape
    out = torch.zeros(rows, cols_out, dtype=dt)
    out[:, :min(cols, cols_out)] = src.to(dt)[:, :cols_out]
    return dict(out=(out, torch.zeros_like(out)))


def colsum(x2d, dt=F64):
    x = x2d.to(dt)
    return dict(out=(x.sum(0), _a(x).sum(0)))


# ---- comparison ---------------------------------------------------------------------------------------------------------------------------
def err_units(got, ref, scale):
    """max over the elements with scale > 0 of |got - ref| / scale, and whether every element with scale == 0 is reproduced exactly."""
    got = got.detach().to(F64).reshape(ref.shape); ref = ref.detach().to(F64); scale = scale.detach().to(F64)
    pos = scale > 0
    e = float(((got - ref).abs()[pos] / scale[pos]).max()) if bool(pos.any()) else 0.0
    exact = bool(torch.equal(got[~pos], ref[~pos]))
    finite = bool(torch.isfinite(got).all())
    return (e if finite else float("inf")), exact
