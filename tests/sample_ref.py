"""Kernel-by-kernel restatement of the correspondence-sampling heads and of the device sampler (dcnet_amd/csrc/sample.hip) in numpy /
torch on the CPU, float64 by default: one function per kernel, on the very float32 / int64 tensors the kernel receives.  No GPU, nothing
of dcnet_amd, no code shared with the older sampling tests.

Selections, gathers and the sampler are exact (integers and copies).  The floating-point stages return  (value, scale)  per element, as
tests/head_ref.py does: `scale` is the sum of the absolute values of the terms that were added into the element (carried to first
order through quotients and square roots), the unit in which an error of that element is judged; scale == 0 marks an element that must
be reproduced exactly.  `dt=torch.float32` evaluates the same formulas in fp32: the yardstick r32 of sample_cases.sample_tol.  The pure
sums (k9_bwd, k14_negscatter, the per-word sums of k14_dlag) also come as fp32 sums added one term at a time from +0.0f in the order
the kernel documents, which the kernel must reproduce bit for bit.

The keyword arguments select deliberately WRONG variants; tests/test_sample_ref_host.py shows that the cases of tests/sample_cases.py
tell each of them from the right answer.

  k9_fwd            tie_high          (a) ties at the threshold take the highest flat index
                    equal_desc        (b) equal values emitted in descending index order
                    raw_bits          (c) keys compared as raw unsigned bit patterns
                    swap_qk           (d) q = idx % HW, k = idx // HW
                    no_skip           (e) no skip of the matched position
                    skip_gt           (f) skip on raw > k instead of raw >= k
                    neg_frame1        (g) negatives gathered from frame 1
  colnorm / lagnorm over_channels     (h) normalised over the channels
                    odd               (i) lagnorm reads the odd channels
                    no_eps            (j) no 1e-12 clamp of the norm (forward and both backward kernels)
  crossmap          taps_rev          (k) conv taps reversed
                    w_t               (l) w[li][lo]
                    no_pad            (m) the neighbours wrap round instead of being zero
                    no_bias           (n)
                    last_max          (o) last maximum instead of the first
  k14_gather        own_image         (p) negatives taken from the own image
  colnorm_bwd       extra_all         (q) `extra` added to every image
                    extra_img0        (r) `extra` added to image 0
                    no_proj           (s) the projection term vit * dot dropped
  k14_dlag          no_proj           (t) the projection term lag * dot dropped
  sampler           bits_pm1          (u) (pop - 1).bit_length()
                    no_shift          (v) no shift on the removed position
                    no_hi_id          (w) K14 ids without 0x80000000
                    step_lo           (x) the high word of the step counter ignored
"""
import numpy as np
import torch

F64 = torch.float64
F32 = torch.float32
U = 2.0 ** -24                               # unit roundoff of fp32
NORM_EPS = 1e-12
M32 = 0xFFFFFFFF


def _a(x):
    return x.abs()


# ---- K9: selection and gathers (exact) ------------------------------------------------------------------------------------------------
def select(row, top_k, tie_high=False, equal_desc=False, raw_bits=False):
    """Flat indices of the top_k largest of the float32 vector `row`, by a stable sort on (value descending, index ascending); equal
    VALUES tie (+0.0 == -0.0)."""
    row = np.ascontiguousarray(row, np.float32)
    idx = np.arange(row.size, dtype=np.int64)
    key = row.view(np.uint32).astype(np.int64) if raw_bits else row.astype(np.float64)
    sel = np.lexsort((-idx if tie_high else idx, -key))[:top_k]
    return sel[np.lexsort((-sel if equal_desc else sel, -key[sel]))]


def k9_fwd(cmap, fv, raw, hw, top_k, tie_high=False, equal_desc=False, raw_bits=False, swap_qk=False, no_skip=False, skip_gt=False,
           neg_frame1=False):
    """cmap (pairs, hw*hw) f32, fv (2*pairs, hw, E) f32, raw (pairs, top_k, neg_n) int64 -> index, neg_idx, frame, corr, negf."""
    pairs = cmap.shape[0]
    index = torch.from_numpy(np.stack([select(cmap[b].numpy(), top_k, tie_high, equal_desc, raw_bits) for b in range(pairs)]))
    q, k = index // hw, index % hw
    if swap_qk:
        q, k = k, q
    kk = k.unsqueeze(2)
    neg = raw.clone() if no_skip else raw + ((raw > kk) if skip_gt else (raw >= kk)).long()
    f = fv.view(pairs, 2, hw, -1)
    ar = torch.arange(pairs)
    frame = f[:, 0][ar.unsqueeze(1), q]; corr = f[:, 1][ar.unsqueeze(1), k]
    negf = f[:, 0 if neg_frame1 else 1][ar.view(-1, 1, 1), neg]
    return dict(index=index, neg_idx=neg, frame=frame.contiguous(), corr=corr.contiguous(), negf=negf.contiguous())


def _seq_add(out, dest, rows):
    """out[dest[j]] += rows[j] for j = 0, 1, ... in fp32, one rounding per addition: every destination's sum in list order."""
    for j in range(len(dest)):
        out[dest[j]] += rows[j]


def k9_bwd(index, neg_idx, d_frame, d_corr, d_neg, hw):
    """dfv (2*pairs, hw, E): frame 0 of a pair collects d_frame at idx // hw; frame 1 collects d_corr at idx % hw, then d_neg at
    neg_idx.  Returns (fp64 sums, fp32 sums in list order: direct entries ascending, then negatives ascending)."""
    pairs, top_k = index.shape
    E = d_frame.shape[-1]
    out64 = torch.zeros(2 * pairs, hw, E, dtype=F64); out32 = torch.zeros(2 * pairs, hw, E, dtype=F32)
    for b in range(pairs):
        q, k = (index[b] // hw).tolist(), (index[b] % hw).tolist()
        ng = neg_idx[b].reshape(-1).tolist(); dn = d_neg[b].reshape(-1, E)
        for out, cast in ((out64, lambda t: t.double()), (out32, lambda t: t)):
            _seq_add(out[2 * b], q, cast(d_frame[b]))
            _seq_add(out[2 * b + 1], k, cast(d_corr[b]))
            _seq_add(out[2 * b + 1], ng, cast(dn))
    return out64, out32


# ---- K14: normalisations ---------------------------------------------------------------------------------------------------------------
def _normalise(x, dim, no_eps):
    """x / max(||x||, eps) along dim: value, scale, norm, scale of the norm.  The sum of squares has scale ss, so its root has scale
    nrm / 2 from the sum and nrm from its own rounding; the quotient adds |x / den|."""
    nrm = (x * x).sum(dim, keepdim=True).sqrt()
    den = nrm if no_eps else nrm.clamp_min(NORM_EPS)
    y = x / den
    s_nrm = 1.5 * nrm
    return y, _a(y) * (1.0 + s_nrm / den), nrm, s_nrm


def colnorm_fwd(v, dt=F64, over_channels=False, no_eps=False):
    """v (N, HW, E) -> vit = v / max(||v[n, :, c]||, 1e-12) over the POSITIONS, cnorm (N, E)."""
    x = v.to(dt)
    y, s_y, nrm, s_nrm = _normalise(x, 2 if over_channels else 1, no_eps)
    if over_channels:
        nrm = nrm.expand(-1, -1, x.shape[2])[:, 0]; s_nrm = s_nrm.expand(-1, -1, x.shape[2])[:, 0]
    else:
        nrm = nrm[:, 0]; s_nrm = s_nrm[:, 0]
    return dict(vit=(y, s_y), cnorm=(nrm, s_nrm))


def colnorm_bwd(vit, cnorm, dq, extra, n_extra, dt=F64, extra_all=False, extra_img0=False, no_proj=False, no_eps=False):
    """dv = (g - vit * sum_p(g * vit)) / max(cnorm, eps),  g = dq (+ extra for image n_extra; extra may be None)."""
    y, cn, g = vit.to(dt), cnorm.to(dt), dq.to(dt).clone()
    s_g = torch.zeros_like(g)
    if extra is not None:
        ex = extra.to(dt)
        rows = slice(None) if extra_all else (slice(0, 1) if extra_img0 else slice(n_extra, n_extra + 1))
        s_g[rows] = _a(g[rows]) + _a(ex)
        g[rows] = g[rows] + ex
    dot = (g * y).sum(1, keepdim=True); s_dot = (_a(g * y) + s_g * _a(y)).sum(1, keepdim=True)
    den = (cn if no_eps else cn.clamp_min(NORM_EPS)).unsqueeze(1)
    if no_proj:
        return dict(dv=(g / den, (_a(g) + s_g) / den))
    return dict(dv=((g - y * dot) / den, (_a(g) + s_g + _a(y) * s_dot) / den))


def lagnorm_fwd(ctx, dt=F64, odd=False, over_channels=False, no_eps=False):
    """ctx (N, L, D) -> lag = even channels / max(norm over the WORDS, 1e-12) (N, L, D/2), lnorm (N, D/2).  Only the even channels are
    ever converted or read."""
    x = ctx[:, :, (1 if odd else 0)::2].to(dt)
    y, s_y, nrm, s_nrm = _normalise(x, 2 if over_channels else 1, no_eps)
    if over_channels:
        nrm = nrm.expand(-1, -1, x.shape[2])[:, 0]; s_nrm = s_nrm.expand(-1, -1, x.shape[2])[:, 0]
    else:
        nrm = nrm[:, 0]; s_nrm = s_nrm[:, 0]
    return dict(lag=(y, s_y), lnorm=(nrm, s_nrm))


# ---- K14: conv map and arg-max -----------------------------------------------------------------------------------------------------------
def crossmap(lag, vit, w, b, dt=F64, taps_rev=False, w_t=False, no_pad=False, no_bias=False, last_max=False):
    """lvmap[n, lo, p] = b[lo] + sum_li sum_t w[lo, li, t] <lag[n, li], vit[n, p + t - 1]> (zero padded), cols = its FIRST maximum over lo,
    gap (N, HW) = (largest - second largest) / the largest scale of the column (inf for L == 1)."""
    la, vi, w, b = lag.to(dt), vit.to(dt), w.to(dt), b.to(dt)
    N, L, _ = la.shape
    HW = vi.shape[1]
    if taps_rev:
        w = w.flip(2)
    if w_t:
        w = w.transpose(0, 1)
    m = torch.einsum("nlc,npc->nlp", la, vi); s_m = torch.einsum("nlc,npc->nlp", _a(la), _a(vi))
    lv = torch.zeros(N, L, HW, dtype=dt); s_lv = torch.zeros(N, L, HW, dtype=dt)
    if not no_bias:
        lv += b.view(1, L, 1); s_lv += _a(b).view(1, L, 1)
    taps = []
    for t in range(3):
        if no_pad:
            sh, s_sh = torch.roll(m, 1 - t, 2), torch.roll(s_m, 1 - t, 2)
        else:
            sh = torch.zeros_like(m); s_sh = torch.zeros_like(m)
            lo_, hi_ = max(0, 1 - t), min(HW, HW + 1 - t)                  # destination positions p with 0 <= p + t - 1 < HW
            sh[:, :, lo_:hi_] = m[:, :, lo_ + t - 1:hi_ + t - 1]; s_sh[:, :, lo_:hi_] = s_m[:, :, lo_ + t - 1:hi_ + t - 1]
        taps.append((sh, s_sh))
    # the 3 L + 1 terms one after another (bias, then li ascending, taps ascending): in fp32 this is the plain evaluation of the formula,
    # whose rounding grows with the number of terms; a blocked einsum would understate the yardstick at L = 32
    for li in range(L):
        for t, (sh, s_sh) in enumerate(taps):
            lv = lv + w[:, li, t].view(1, L, 1) * sh[:, li].unsqueeze(1)
            s_lv = s_lv + _a(w[:, li, t]).view(1, L, 1) * s_sh[:, li].unsqueeze(1)
    mx = lv.max(1, keepdim=True)[0]
    ar = torch.arange(L).view(1, L, 1).expand_as(lv)
    cols = torch.where(lv == mx, ar, -1).max(1)[0] if last_max else torch.where(lv == mx, ar, L).min(1)[0]
    if L > 1:
        top2 = lv.topk(2, dim=1)[0]
        sc = s_lv.max(1)[0]
        gap = torch.where(sc > 0, (top2[:, 0] - top2[:, 1]) / sc.clamp_min(1e-300), torch.full_like(sc, float("inf")))
        gap = torch.where((sc == 0) & (top2[:, 0] == top2[:, 1]), torch.zeros_like(gap), gap)
    else:
        gap = torch.full((N, HW), float("inf"), dtype=dt)
    return dict(lvmap=(lv, s_lv), cols=cols, gap=gap)


def k14_gather(lag, vit, cols, neg, own_image=False):
    """lag_pos[n, p] = lag[n, cols[n, p]] (N, HW, 1, E);  neg_cross[n, p, m] = vit[N - 1, neg[n, p, m]] (N, HW, neg_n, E).  Exact copies."""
    N = lag.shape[0]
    ar = torch.arange(N)
    lag_pos = lag[ar.unsqueeze(1), cols].unsqueeze(2)
    neg_cross = vit[ar.view(N, 1, 1), neg] if own_image else vit[N - 1][neg]
    return dict(lag_pos=lag_pos.contiguous(), neg_cross=neg_cross.contiguous())


# ---- K14 backward ------------------------------------------------------------------------------------------------------------------------
def k14_negscatter(d_neg, csr_off, csr_src, hw):
    """extra[p] = sum of the rows d_neg[csr_src[i]], i in [csr_off[p], csr_off[p + 1]), in that (ascending source) order: fp64, fp32."""
    d = d_neg.reshape(-1, d_neg.shape[-1])
    off, src = csr_off.tolist(), csr_src.tolist()
    out64 = torch.zeros(hw, d.shape[1], dtype=F64); out32 = torch.zeros(hw, d.shape[1], dtype=F32)
    for p in range(hw):
        for i in range(off[p], off[p + 1]):
            out64[p] += d[src[i]].double(); out32[p] += d[src[i]]
    return out64, out32


def k14_word_sums(cols, d_k, L):
    """dlag[n, l] = sum over the positions p with cols[n, p] == l of d_k[n, p], ascending p: fp64, fp32 sequential."""
    N, HW = cols.shape
    E = d_k.shape[-1]
    d = d_k.reshape(N, HW, E)
    out64 = torch.zeros(N, L, E, dtype=F64); out32 = torch.zeros(N, L, E, dtype=F32)
    for n in range(N):
        _seq_add(out64[n], cols[n].tolist(), d[n].double()); _seq_add(out32[n], cols[n].tolist(), d[n])
    return out64, out32


def k14_dlag(lag, lnorm, cols, d_k, dt=F64, no_proj=False, no_eps=False):
    """dctx[n, l, 2c] = (dlag - lag * sum_l(dlag * lag)) / max(lnorm, eps);  the odd channels are +0 (scale 0: exact)."""
    la, ln = lag.to(dt), lnorm.to(dt)
    N, L, E = la.shape
    d = d_k.to(dt).reshape(N, -1, E)
    dl = torch.zeros(N, L, E, dtype=dt); s_dl = torch.zeros(N, L, E, dtype=dt)
    ix = cols.unsqueeze(2).expand(-1, -1, E)
    dl.scatter_add_(1, ix, d); s_dl.scatter_add_(1, ix, _a(d))
    dot = (dl * la).sum(1, keepdim=True); s_dot = (s_dl * _a(la)).sum(1, keepdim=True)
    den = (ln if no_eps else ln.clamp_min(NORM_EPS)).unsqueeze(1)
    val = dl / den if no_proj else (dl - la * dot) / den
    sc = s_dl / den if no_proj else (s_dl + _a(la) * s_dot) / den
    out = torch.zeros(N, L, 2 * E, dtype=dt); s_out = torch.zeros(N, L, 2 * E, dtype=dt)
    out[:, :, 0::2] = val; s_out[:, :, 0::2] = sc
    return dict(dctx=(out, s_out))


# ---- the device sampler: Philox-4x32-10 in Python integers --------------------------------------------------------------------------------
def philox4x32_10(ctr, key):
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def draw(pop, k, seed, step, sample_id, bits_pm1=False, step_lo=False):
    """k distinct values of [0, pop): block after block of counter (id, block, step low, step high) under key (seed low, seed high), each
    word shifted right by 32 - pop.bit_length(), a word >= pop or already drawn rejected."""
    shift = 32 - ((pop - 1) if bits_pm1 else pop).bit_length()
    sel, block = [], 0
    while len(sel) < k:
        words = philox4x32_10((sample_id & M32, block, step & M32, 0 if step_lo else (step >> 32) & M32), (seed & M32, (seed >> 32) & M32))
        for wd in words:
            r = wd >> shift
            if r < pop and r not in sel and len(sel) < k:
                sel.append(r)
        block += 1
        assert block < 4096, "draw: no progress"
    return sel


def k9_table(n, hw, top_k, neg_n, seed, step, **var):
    """(n/2, top_k, neg_n) raw positions of a population of hw - 1: sample t = pair * top_k + j has id t."""
    var = {k: v for k, v in var.items() if k in ("bits_pm1", "step_lo")}
    rows = [draw(hw - 1, neg_n, seed, step, t, **var) for t in range((n // 2) * top_k)]
    return np.array(rows, np.int64).reshape(n // 2, top_k, neg_n)


def k14_table(n, hw, neg_c, seed, step, no_shift=False, no_hi_id=False, **var):
    """(n, hw, neg_c) positions of [0, hw); for image n - 1 the own position jj is removed from the population (a draw >= jj moves up by
    one).  Sample u = ii * hw + jj has id 0x80000000 + u."""
    var = {k: v for k, v in var.items() if k in ("bits_pm1", "step_lo")}
    out = np.zeros((n, hw, neg_c), np.int64)
    for u in range(n * hw):
        ii, jj = divmod(u, hw)
        removed = ii == n - 1
        sel = draw(hw - 1 if removed else hw, neg_c, seed, step, u if no_hi_id else 0x80000000 + u, **var)
        out[ii, jj] = [s + 1 if removed and not no_shift and s >= jj else s for s in sel]
    return out


def csr(k14, hw):
    """Sources grouped by drawn position, ascending inside a group: a stable argsort and the cumulative counts."""
    flat = np.asarray(k14).reshape(-1)
    src = np.argsort(flat, kind="stable").astype(np.int32)
    off = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=hw))]).astype(np.int32)
    return off, src


# ---- comparison ---------------------------------------------------------------------------------------------------------------------------
def err_units(got, ref, scale):
    """max over the elements with scale > 0 of |got - ref| / scale, and whether every element with scale == 0 is reproduced exactly."""
    got = got.detach().to(F64).reshape(ref.shape); ref = ref.detach().to(F64); scale = scale.detach().to(F64)
    pos = scale > 0
    e = float(((got - ref).abs()[pos] / scale[pos]).max()) if bool(pos.any()) else 0.0
    exact = bool(torch.equal(got[~pos], ref[~pos]))
    finite = bool(torch.isfinite(got).all())
    return (e if finite else float("inf")), exact
