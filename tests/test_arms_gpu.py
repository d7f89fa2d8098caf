"""Every arm of every tuning knob (csrc/tuning.h) forced onto a launch it really redirects, at small shapes with tails and borders,
against fp64 — the README's "no knob changes results beyond rounding", checked.

One table: ARMS[knob] = [(values, workload, evidence), ...].
  values    what dcn_set_tuning gets (the knob under test and the knobs it needs to be reachable)
  workload  (kind, *arguments): one of WORKLOADS below
  evidence  (text, check): proof that the arm ran and not the default — in this order of preference a profiling-tag count
            (csrc/prof.h), a result that is not bitwise the default's, and where two arms book the same tag and agree bitwise by
            construction a read-only dispatch query of the C ABI (dcn_conv1_tile, dcn_l2norm_score_fwd_form, dcn_bn_apply_form,
            dcn_conv2d_stats_rows, dcn_conv2d_bwd_weight_ws[_b16])
The fp64 references are tests/util.py conv_by_taps (torch.matmul per tap on the device), F.batch_norm, F.normalize and torch.bmm in
fp64: nothing of this library.  Tolerances, relative to max(1, |ref|max), are those the existing tests use for the same operation:
2e-5 forward / data gradient, 3e-5 weight gradient, 1e-4 summed BatchNorm partials, the exact-model bounds of test_b16_gpu.py /
test_f8_gpu.py for the storage modes.  tests/test_tuning.py checks (without a GPU) that no knob is missing from this table.

Gemm3 schedule variants: gemm3.hip's K loop knows G3Params::var 0 (B pieces issued ahead of the MFMA groups), 1 (behind them) and
2 (between them).  Any other number never issued the B pieces again — stale LDS, wrong products, in a default build — until
gemm3_variant() mapped it to 0; Gemm3 = 769 (the knob's upper bits say 3) holds that.  Covered: Gemm3 = 0 (engine off), 1, 257, 513, 769;
dcn_gemm3_variant is the launcher's own answer for each."""
import functools

import pytest
import torch
import torch.nn.functional as F

from util import close, conv_by_taps, prof_counts, rand, tuning

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


class Ctx:
    """what an evidence check sees: the case, the arm's and the default's outputs and launch counts per part, the library"""

    def __init__(self, case, arm, base):
        from dcnet_amd.lib import lib
        self.case, self.arm, self.base, self.L = case, arm, base, lib()

    def n(self, part, *tags):
        return sum(self.arm["counts"][part][t] for t in tags)

    def n0(self, part, *tags):
        return sum(self.base["counts"][part][t] for t in tags)

    def launches(self, part):
        return sum(self.arm["counts"][part])

    def launches0(self, part):
        return sum(self.base["counts"][part])

    def differs(self, *keys):
        return any(not torch.equal(self.arm[k], self.base[k]) for k in keys)


def _out_hw(h, w, k, st):
    pad = (k - 1) // 2
    return (h + 2 * pad - k) // st + 1, (w + 2 * pad - k) // st + 1


# ---- convolutions ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _conv_data(case):
    """inputs and fp64 references of a case (n, h, w, cin, cout, k, stride), all on the device"""
    n, h, w, cin, cout, k, st = case
    ho, wo = _out_hw(h, w, k, st)
    d = {}
    d["x"] = rand(n, h, w, cin, seed=41).to(DEV)
    d["wt"] = (rand(cout, k, k, cin, seed=42) / (cin * k * k) ** 0.5).to(DEV)
    d["scale"] = (rand(cout, seed=43).abs() + 0.5).to(DEV); d["shift"] = rand(cout, seed=44).to(DEV)
    d["res"] = rand(n, ho, wo, cout, seed=45).to(DEV)
    d["dy"] = (rand(n, ho, wo, cout, seed=46) / 8).to(DEV)
    d["base"] = rand(n, h, w, cin, seed=47).to(DEV)
    d["raw"], d["dx"], d["dw"] = conv_by_taps(d["x"], d["wt"], k, st, d["dy"])
    d["y"] = F.leaky_relu(d["raw"] * d["scale"].double() + d["shift"].double(), 0.1) + d["res"].double()
    rb = lambda t: t.bfloat16().double()                            # the exact model of wsplit = 2: operands rounded to bf16 (nearest even)
    d["dw_b16"] = conv_by_taps(rb(d["x"]), d["wt"], k, st, rb(d["dy"]))[2]
    return d


def _conv_run(case, parts):
    from dcnet_amd import ops
    n, h, w, cin, cout, k, st = case
    ho, wo = _out_hw(h, w, k, st)
    d = _conv_data(case)
    x, wt, dy = d["x"], d["wt"], d["dy"]
    out, counts = {}, {}

    def fwd():
        out["y"], out["stats"] = ops.conv2d_fwd(x, wt, k, st, d["scale"], d["shift"], ops.ACT_LEAKY, 0.1, residual=d["res"], want_stats=True)
        out["raw"], out["raw_stats"] = ops.conv2d_fwd(x, wt, k, st, want_stats=True)
        buf = torch.zeros(n, ho, wo, cout + 64, device=DEV)
        am = ops.amax_slot(x.device)
        ops.conv2d_fwd(x, wt, k, st, out=buf[..., 32:32 + cout], amax_out=am)
        out["slice"] = buf; out["amax"] = am.clone()
        acc = d["raw"].float().clone()
        _, out["acc_stats"] = ops.conv2d_fwd(x, wt, k, st, out=acc, accumulate=True, want_stats=True)
        out["acc"] = acc

    def dgrad():
        out["dx"] = ops.conv2d_bwd_data(dy, wt, (h, w), k, st)
        dx2 = d["base"].clone()
        ops.conv2d_bwd_data(dy, wt, (h, w), k, st, out=dx2, accumulate=True)
        out["dx_acc"] = dx2

    def wgrad():
        out["dw"] = ops.conv2d_bwd_weight(x, dy, k, st)

    for part, fn in (("fwd", fwd), ("dgrad", dgrad), ("wgrad", wgrad)):
        if part in parts:
            _, counts[part] = prof_counts(fn)
    out["counts"] = counts
    return out


def _conv_check(case, r, parts, name, wsplit2=False):
    d = _conv_data(case)
    cout = case[4]
    if "fwd" in parts:
        raw2 = d["raw"].reshape(-1, cout)
        close(r["y"], d["y"], 2e-5, f"{name}: forward, fused epilogue + shortcut")
        close(r["raw"], d["raw"], 2e-5, f"{name}: forward, raw")
        for key, mul in (("stats", 1), ("raw_stats", 1), ("acc_stats", 2)):
            close(r[key][:, 0].double().sum(0), mul * raw2.sum(0), 1e-4, f"{name}: {key} sum")
            close(r[key][:, 1].double().sum(0), mul * mul * (raw2 * raw2).sum(0), 1e-4, f"{name}: {key} sum of squares")
        close(r["slice"][..., 32:32 + cout], d["raw"], 2e-5, f"{name}: concat-slice destination")
        assert float(r["slice"][..., :32].abs().max()) == 0 and float(r["slice"][..., 32 + cout:].abs().max()) == 0, f"{name}: wrote beside its slice"
        assert float(r["amax"].view(torch.float32).max()) == float(r["slice"].abs().max()), f"{name}: abs-max word"
        close(r["acc"], 2 * d["raw"], 2e-5, f"{name}: accumulate")
    if "dgrad" in parts:
        close(r["dx"], d["dx"], 2e-5, f"{name}: data gradient")
        close(r["dx_acc"], d["dx"] + d["base"].double(), 2e-5, f"{name}: data gradient, accumulating")
    if "wgrad" in parts:
        close(r["dw"], d["dw_b16"] if wsplit2 else d["dw"], 3e-5, f"{name}: weight gradient" + (" against its bf16-operand exact model" if wsplit2 else ""))
        if wsplit2:       # ... and it IS that mode: about 2^-9 from fp64, not fp32-accurate
            e = float((r["dw"].double() - d["dw"]).abs().max()) / max(1.0, float(d["dw"].abs().max()))
            assert 1e-5 < e <= 1e-2, f"{name}: wsplit = 2 is {e:.2e} from fp64"


def _conv(values, evidence, cases, parts):
    parts = parts.split()
    for case in cases:
        with tuning():
            base = _conv_run(case, parts)
        with tuning(values):
            arm = _conv_run(case, parts)
            name = f"{values} on {case}"
            _conv_check(case, arm, parts, name, wsplit2=values.get("wsplit") == 2)
            booked = {who: {p: {t: v for t, v in enumerate(c) if v} for p, c in r["counts"].items()} for who, r in (("arm", arm), ("default", base))}
            assert evidence[1](Ctx(case, arm, base)), f"{name}: no evidence that the arm ran ({evidence[0]}); launches per tag: {booked}"
        _conv_check(case, base, parts, f"default knobs on {case}")


def _fwd_tile(c, stats=1):
    n, h, w, cin, cout, k, st = c.case
    ho, wo = _out_hw(h, w, k, st)
    return c.L.conv1_tile(n * ho * wo, cout, k * k, cin, stats, 0)


def _dgrad_tile(c):            # (1x1 layers: the data gradient is a plain GEMM towards cin "filters")
    n, h, w, cin, cout, k, st = c.case
    return c.L.conv1_tile(n * h * w, cin, 1, cout, 0, 0)


def _wide(tile):
    """conv1.hip's two 128-row tiles book the same tag and agree bitwise: the dispatcher's own answer, for the forward with and without
    BatchNorm partials and — where the data gradient has a multiple of 256 "filters" — for the data gradient"""
    def check(c):
        cin, k = c.case[3], c.case[5]
        ok = _fwd_tile(c, 1) == tile and _fwd_tile(c, 0) == tile and c.n("fwd", 35) == 4
        if k == 1 and cin % 256 == 0:
            ok = ok and _dgrad_tile(c) == tile and c.n("dgrad", 35) == 2
        return ok
    return check


def _wgrad_splits(c, b16=False):
    n, h, w, cin, cout, k, st = c.case
    ws = (c.L.conv2d_bwd_weight_ws_b16 if b16 else c.L.conv2d_bwd_weight_ws)(n, h, w, cin, cout, k, st)
    return max(1, ws // (cout * k * k * cin))


def _splits_for(target, b16=False):
    """split-K slabs for a workgroup target: 1 -> one; 64 -> more than one; 4096 -> the cap of M / 256 (>= 8 K-steps per slab)"""
    def check(c):
        n, h, w, cin, cout, k, st = c.case
        ho, wo = _out_hw(h, w, k, st)
        s, cap = _wgrad_splits(c, b16), n * ho * wo // 256
        return s == 1 if target == 1 else (s == cap if target == 4096 else 1 < s <= cap)
    return check


# 1x1 layers of >= 1024 rows with an M tail (3 x 37 x 29 = 3219 = 25 x 128 + 19), Ci = 32: a K loop shorter than the ring; 256 / 1024
# input channels: data gradients on the wide tile as well; 3x3 stride 2 on an odd map (borders, 1104 rows)
WIDE_CASES = ((3, 37, 29, 32, 256, 1, 1), (3, 37, 29, 96, 512, 1, 1), (3, 37, 29, 1024, 768, 1, 1), (3, 37, 29, 256, 512, 1, 1),
              (2, 45, 47, 64, 256, 3, 2))
DMA_CASES = ((3, 37, 29, 96, 128, 1, 1), (2, 45, 47, 64, 128, 3, 2))
ODD_S2 = ((2, 45, 47, 128, 256, 3, 2), (2, 45, 47, 64, 128, 3, 2), (3, 27, 29, 32, 64, 3, 2))     # parity classes of 23x24 | 23x23 | 22x24 | 22x23 pixels ...
BIG_S2 = ((1, 513, 515, 32, 64, 3, 2),)                                                          # classes of more than 65536 rows: four launches by default
N1_CASE, D2_CASE, D2S_CASE = (1, 256, 260, 32, 64, 3, 1), (2, 128, 256, 64, 128, 3, 2), (4, 128, 128, 32, 64, 3, 2)
BM_CASES = ((2, 26, 27, 256, 512, 1, 1), (2, 26, 27, 64, 128, 3, 1))
K_CASES = ((2, 52, 51, 64, 128, 1, 1), (8, 52, 53, 64, 128, 1, 1))                   # 5304 and 22048 rows: either side of 16384
SPLIT_FREE = ((3, 37, 29, 96, 128, 1, 1), (2, 45, 47, 64, 128, 3, 2), (2, 26, 27, 64, 128, 3, 1))
OCC_CASES = ((2, 26, 27, 32, 128, 1, 1), (2, 26, 27, 64, 128, 3, 1))                 # 2 and 36 K-steps of 16
CO32 = ((2, 40, 37, 64, 32, 1, 1), (2, 40, 37, 32, 32, 3, 1))                       # Co = 32: K = 64 and K = 288
NARROW = ((2, 40, 37, 64, 32, 1, 1), (2, 40, 37, 128, 64, 1, 1))
T64_CASES = ((2, 37, 41, 64, 64, 3, 1), (1, 40, 33, 128, 64, 3, 1))
W64_CASES = ((3, 30, 27, 128, 64, 1, 1), (3, 30, 27, 64, 128, 1, 1), (2, 45, 47, 128, 64, 3, 2))
XWG_NARROW, XWG_WIDE = ((2, 37, 41, 64, 64, 3, 1),), ((1, 40, 33, 128, 128, 3, 1),)   # M = 3034 and 1320: no multiples of 32
ZWG_CASES = ((3, 37, 29, 512, 512, 1, 1), (2, 45, 47, 128, 128, 3, 2))              # M = 3219 and 1104
WSPLIT_CASES = ((2, 26, 27, 128, 256, 1, 1), (2, 45, 47, 128, 128, 3, 2))
W9_P, W9_Q, W9_R = (2, 64, 64, 32, 64, 3, 1), (2, 64, 64, 64, 128, 3, 1), (2, 64, 64, 64, 128, 3, 2)


def _tap9(v):
    takes = {0: (), 1: (W9_P,), 2: (W9_P, W9_Q), 3: (W9_P, W9_Q, W9_R)}[v]
    return lambda c: c.n("wgrad", 36) == (1 if c.case in takes else 0)


def _k_tag(k):
    return lambda c: c.n("fwd", 15 if k == 32 else 0) == 4 and c.n("fwd", 0 if k == 32 else 15) == 0


def _occ3(v):
    def check(c):
        ksteps = c.case[5] ** 2 * c.case[3] // 16
        return c.n("fwd", 16) == 4 and c.L.igemm_split_build(1, ksteps) == (163 if ksteps <= v else 161) and c.L.igemm_split_build(1, 1 << 20) == 161
    return check


def _gk32(v):
    def check(c):
        kk = c.case[3] * c.case[5] ** 2
        return (c.n("fwd", 24) == 4 and c.n("fwd", 2) == 0) if kk >= v else (c.n("fwd", 2) == 4 and c.n("fwd", 24) == 0)
    return check


# ---- storage modes: the exact models of test_b16_gpu.py / test_f8_gpu.py ----------------------------------------------------------
B16_WIDE = ((3, 9, 11, 256, 256, 1, 1), (1, 27, 29, 128, 256, 3, 2), (1, 20, 20, 256, 256, 3, 2))
B16_WG3, B16_WGS = ((1, 40, 33, 128, 256, 3, 1),), ((2, 27, 29, 128, 128, 1, 1),)


def _storage(values, evidence, mode, cases):
    import test_b16_gpu
    import test_f8_gpu
    for case in cases:
        with tuning(values):
            if mode == "bf16s":
                test_b16_gpu._conv_case(case)
            else:
                test_f8_gpu.test_f8_conv_forward_and_data_gradient_match_their_exact_model(case)
            assert evidence[1](Ctx(case, None, None)), f"{values} on {case}: no evidence that the arm ran ({evidence[0]})"


def _b16_tile(tile):
    def check(c):
        n, h, w, cin, cout, k, st = c.case
        ho, wo = _out_hw(h, w, k, st)
        return c.L.conv1_tile(n * ho * wo, cout, k * k, cin, 1, 1) == tile
    return check


# ---- NN products --------------------------------------------------------------------------------------------------------------
def _gemm_nn(values, evidence, cases):
    from dcnet_amd import ops
    for m, n, k, kvalid in cases:
        a = rand(m, k, seed=1).to(DEV); b = (rand(k, n, seed=2) / k ** 0.5).to(DEV)
        kv = kvalid or k
        ref = a.double()[:, :kv] @ b.double()[:kv]
        with tuning():
            base, cb = prof_counts(lambda: ops.gemm_nn(a, b, kvalid=kvalid))
        with tuning(values):
            out, ca = prof_counts(lambda: ops.gemm_nn(a, b, kvalid=kvalid))
        close(out, ref, 3e-5, f"{values}: gemm_nn {m} x {n} x {k}")
        c = Ctx((m, n, k), {"counts": {"nn": ca}, "out": out}, {"counts": {"nn": cb}, "out": base})
        assert evidence[1](c), f"{values} on gemm_nn {m} x {n} x {k}: no evidence that the arm ran ({evidence[0]})"


# ---- BatchNorm --------------------------------------------------------------------------------------------------------------
BN_CASES = ((4, 2, 33, 31), (8, 3, 19, 23), (32, 3, 9, 7), (96, 3, 9, 7), (1024, 3, 9, 7), (2048, 1, 9, 7))      # c, n, h, w: 2046 | 1311 | 189 | 63 rows


def _off(t, by):
    """the same values in a tensor that starts ``by`` floats behind a 16-byte boundary"""
    buf = torch.zeros(t.numel() + 8, device=t.device)
    v = buf[by:by + t.numel()]
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * by
    return v


def _bn(values, evidence, cases):
    from dcnet_amd import ops
    for c, n, h, w in cases:
        for by in (0, 1):
            y = rand(n, h, w, c, seed=20) * 2 + 0.5
            gamma = rand(c, seed=21).abs() + 0.5; beta = rand(c, seed=22)
            rm = rand(c, seed=23); rv = rand(c, seed=24).abs() + 0.5
            res = rand(n, h, w, c, seed=25); dout = rand(n, h, w, c, seed=26)
            yd = y.permute(0, 3, 1, 2).double().requires_grad_(True); gd = gamma.double().requires_grad_(True); bd = beta.double().requires_grad_(True)
            rm_ref, rv_ref = rm.clone().double(), rv.clone().double()
            out_ref = F.leaky_relu(F.batch_norm(yd, rm_ref, rv_ref, gd, bd, True, 0.1, 1e-5), 0.1) + res.permute(0, 3, 1, 2).double()
            out_ref.backward(dout.permute(0, 3, 1, 2).double())
            name = f"{values}: BatchNorm c = {c}, {n * h * w} rows, parameters {4 * by} bytes off"
            with tuning(values):
                yv = y.to(DEV)
                g, b = _off(gamma.to(DEV), by), _off(beta.to(DEV), by)
                rmd, rvd = rm.to(DEV), rv.to(DEV)
                stats = ops.channel_stats(yv.view(-1, c))
                mi = ops.bn_finalize(stats, n * h * w, g, b, 1e-5, 0.1, rmd, rvd)
                out = ops.scale_act(yv, _off(mi[2], by), _off(mi[3], by), ops.ACT_LEAKY, 0.1, residual=res.to(DEV))
                dy, dgamma, dbeta = ops.bn_act_bwd(yv, dout.to(DEV), mi[0], mi[1], g, b, ops.ACT_LEAKY, 0.1)
                assert evidence[1](Ctx((c, by == 0), None, None)), f"{name}: no evidence that the arm ran ({evidence[0]})"
            close(out, out_ref.permute(0, 2, 3, 1), 2e-5, name + ": forward")
            close(rmd, rm_ref, 1e-5, name + ": running_mean"); close(rvd, rv_ref, 1e-5, name + ": running_var")
            close(dy, yd.grad.permute(0, 2, 3, 1), 3e-5, name + ": dy")
            close(dgamma, gd.grad, 3e-5, name + ": dgamma"); close(dbeta, bd.grad, 3e-5, name + ": dbeta")


def _bn_form(pc):
    """channel-per-thread kernels for c / 4 a power of two <= 256 and aligned parameters (c = 96, 2048: never), else the grid-stride forms"""
    def check(c):
        ch, aligned = c.case
        c4 = ch // 4
        want = c4.bit_length() - 1 if (pc and aligned and c4 <= 256 and c4 & (c4 - 1) == 0) else -1
        return c.L.bn_apply_form(ch, int(aligned)) == want
    return check


# ---- scoring --------------------------------------------------------------------------------------------------------------------
# c, rows per image, images: 111 | 21 | 13 rows leave a tail for 1, 2, 4 and 8 rows per wave; rows_per_image 3 and 1: image boundaries
# inside one wave's rows, images shorter than them
SCORE_CASES = ((64, 37, 3), (256, 3, 7), (512, 1, 13), (1024, 37, 3), (512, 37, 3))


def _score(values, evidence, cases):
    from dcnet_amd import ops
    for c, rpi, nimg in cases:
        rows = nimg * rpi
        x = rand(nimg, rpi, c, seed=40); x.view(rows, c)[5].zero_()        # an all-zero row: F.normalize's eps gives 0
        q = F.normalize(rand(nimg, c, seed=41), dim=1)
        keep = torch.ones(rows, dtype=torch.bool); keep[5] = False
        xd = x.double().requires_grad_(True); qd = q.double().requires_grad_(True)
        o = F.normalize(xd, dim=2)
        sc = (o * qd.unsqueeze(1)).sum(2); scf = (o * qd.flip(0).unsqueeze(1)).sum(2)
        do = rand(nimg, rpi, c, seed=42); ds = rand(nimg, rpi, seed=43); dsf = rand(nimg, rpi, seed=44)
        do.view(rows, c)[5].zero_(); ds.view(-1)[5] = 0; dsf.view(-1)[5] = 0            # (no gradient into the zero row: its Jacobian is 1 / eps)
        ((o * do.double()).sum() + (sc * ds.double()).sum() + (scf * dsf.double()).sum()).backward()
        base = rand(rows, c + 32, seed=45)
        name = f"{values}: l2norm_score c = {c}, {nimg} images of {rpi} rows"
        with tuning(values):
            xv, qv = x.to(DEV), q.to(DEV)
            out, norm, score, flip = ops.l2norm_score_fwd(xv, qv, rpi, want_flip=True)
            buf = base.to(DEV)
            out2, _, score2, _ = ops.l2norm_score_fwd(xv.view(rows, c), qv, rpi, out=buf[:, 16:16 + c], out_scale=0.75, accumulate=True)
            plain, norm3, none, none2 = ops.l2norm_score_fwd(xv)
            dx, dq = ops.l2norm_score_bwd(out, norm, do.to(DEV), qv, ds.to(DEV).view(-1), rpi, dscore_flip=dsf.to(DEV).view(-1))
            assert evidence[1](Ctx((c,), None, None)), f"{name}: no evidence that the arm ran ({evidence[0]})"
        close(out, o, 1e-6, name + ": normalize"); close(norm.view(nimg, rpi), xd.detach().norm(dim=2), 1e-6, name + ": norm")
        close(score.view(nimg, rpi), sc, 1e-5, name + ": score"); close(flip.view(nimg, rpi), scf, 1e-5, name + ": flipped score")
        assert float(out.view(rows, c)[5].abs().max()) == 0 and float(norm[5]) == 0 and float(score[5]) == 0, name + ": the all-zero row"
        close(buf[:, 16:16 + c], base[:, 16:16 + c].double() + 0.75 * o.detach().view(rows, c), 1e-6, name + ": out_scale + accumulate into a strided slice")
        assert torch.equal(buf[:, :16].cpu(), base[:, :16]) and torch.equal(buf[:, 16 + c:].cpu(), base[:, 16 + c:]), name + ": wrote beside its slice"
        assert torch.equal(score2, score) and none is None and none2 is None
        assert torch.equal(plain, out) and torch.equal(norm3, norm), name + ": without q"
        close(dx.view(rows, c)[keep.to(DEV)], xd.grad.view(rows, c)[keep], 2e-5, name + ": dx"); close(dq, qd.grad, 2e-5, name + ": dq")


def _score_form(rpw, nt):
    return lambda c: c.L.l2norm_score_fwd_form(c.case[0]) == 10 * (4 if (rpw == 8 and c.case[0] > 512) else rpw) + nt


# ---- co-attention ---------------------------------------------------------------------------------------------------------------
COATTN_LARGE = ((2, 26, 256), (1, 23, 256), (2, 52, 512))          # the cases of test_coattn_fwd_bwd whose nine products run on gemm3.hip


def _coattn(values, evidence, cases):
    from dcnet_amd import ops
    for b, g, c in cases:
        hw = g * g
        f1 = F.normalize(rand(b, hw, c, seed=30), dim=2).to(DEV); f2 = F.normalize(rand(b, hw, c, seed=31), dim=2).to(DEV)
        a = f1.double().requires_grad_(True); bb = f2.double().requires_grad_(True)
        A = torch.bmm(a, bb.transpose(1, 2))
        o1 = torch.bmm(F.softmax(A * 10, dim=2), bb); o2 = torch.bmm(F.softmax(A * 10, dim=1).transpose(1, 2), a)
        d1 = rand(b, hw, c, seed=32).to(DEV); d2 = rand(b, hw, c, seed=33).to(DEV)
        ((o1 * d1.double()).sum() + (o2 * d2.double()).sum()).backward()
        base1 = rand(b, hw, c, seed=34).to(DEV); base2 = rand(b, hw, c, seed=35).to(DEV)

        def run():
            cat = torch.zeros(2, b, hw, 2 * c, device=DEV)
            out1, out2 = cat[0, :, :, c:], cat[1, :, :, c:]
            E, rc = ops.coattn_fwd(f1, f2, out1, out2, 10.0)
            g1, g2 = base1.clone(), base2.clone()
            ops.coattn_bwd(f1, f2, d1, d2, out1, out2, E, rc, g1, g2, True, 10.0)
            return {"o1": out1, "o2": out2, "g1": g1, "g2": g2, "pad": cat[..., :c]}

        with tuning():
            r0, c0 = prof_counts(run)
        name = f"{values}: co-attention {b} x {hw} x {c}"
        with tuning(values):
            r, c1 = prof_counts(run)
            r["counts"], r0["counts"] = {"all": c1}, {"all": c0}
            assert evidence[1](Ctx((b, g, c), r, r0)), f"{name}: no evidence that the arm ran ({evidence[0]}); tag 40: {c1[40]} (default {c0[40]})"
        close(r["o1"], o1, 2e-5, name + ": f1_attn"); close(r["o2"], o2, 2e-5, name + ": f2_attn")
        close(r["g1"], a.grad + base1.double(), 5e-5, name + ": d_f1"); close(r["g2"], bb.grad + base2.double(), 5e-5, name + ": d_f2")
        assert float(r["pad"].abs().max()) == 0


def _g3(var):
    return lambda c: c.n("all", 40) == 9 and c.L.gemm3_variant() == var


def _gemm3(values, evidence, cases):
    """test_gemm3_presplit_operands itself under the knob: fp64 in the three forms, and it asserts that tag 40 (gemm3.hip) took the launch"""
    import test_ops_gpu
    for case in cases:
        with tuning(values):
            test_ops_gpu.test_gemm3_presplit_operands(torch.device(DEV), case)
            assert evidence[1](Ctx(case, None, None)), f"{values}: no evidence that the arm ran ({evidence[0]})"


def _g3_cases():
    import test_ops_gpu
    return tuple(test_ops_gpu.G3_CASES)


WORKLOADS = {"conv": _conv, "storage": _storage, "gemm_nn": _gemm_nn, "bn": _bn, "score": _score, "coattn": _coattn, "gemm3": _gemm3}

# profiling tags (csrc/prof.h): 0 / 1 / 2 / 6 / 15 fp32-pipe NT tiles, 16 three-piece split, 24 / 26 f16 split, 35 conv1.hip, 28 / 29 / 51 strip kernels,
# 5 / 17 / 20 / 25 weight-gradient tiles (fp32, bf16 split, bf16 operands, f16 split), 36 wgrad9.hip, 37 / 38 nconv.hip, 40 gemm3.hip
NN_TAGS = (3, 4, 21, 27)

ARMS = {
    "1wide": [
        ({"1wide": 1}, ("conv", WIDE_CASES, "fwd dgrad"), ("dcn_conv1_tile says 128 x 256 (18) and tag 35 took the launches", _wide(18))),
        ({"1wide": 0}, ("conv", WIDE_CASES, "fwd dgrad"), ("dcn_conv1_tile says 128 x 128 (14) and tag 35 took the launches", _wide(14))),
    ],
    "bwide": [
        ({"bwide": 1, "2btile": 0}, ("storage", "bf16s", B16_WIDE), ("dcn_conv1_tile(storage = 1) says 18", _b16_tile(18))),
        ({"bwide": 1}, ("storage", "fp8s", B16_WIDE), ("dcn_conv1_tile(storage = 1) says 18", _b16_tile(18))),
        ({"bwide": 0, "2btile": 0}, ("storage", "bf16s", B16_WIDE[:1]), ("dcn_conv1_tile(storage = 1) says 14", _b16_tile(14))),
    ],
    "1x1dma": [
        ({"1x1dma": 2}, ("conv", DMA_CASES, "fwd dgrad"),
         ("tag 35 keeps the 1x1 launches and loses the gathered ones", lambda c: c.n("fwd", 35) == (4 if c.case[5] == 1 else 0) and c.n0("fwd", 35) == 4)),
        ({"1x1dma": 0}, ("conv", DMA_CASES, "fwd dgrad"), ("no launch under tag 35", lambda c: c.n("fwd", 35) + c.n("dgrad", 35) == 0 and c.n0("fwd", 35) == 4)),
    ],
    "merge": [
        ({"merge": 0}, ("conv", ODD_S2, "dgrad"), ("four launches per data gradient instead of one", lambda c: c.launches("dgrad") == 8 and c.launches0("dgrad") == 2)),
        ({"merge": 2}, ("conv", BIG_S2, "dgrad"), ("one launch per data gradient instead of four", lambda c: c.launches("dgrad") == 2 and c.launches0("dgrad") == 8)),
    ],
    "Nconv": [
        ({"Nconv": 0}, ("conv", (N1_CASE, D2S_CASE), "fwd dgrad"), ("tags 37 / 38 (nconv.hip) took launches by default and take none", lambda c: c.n("fwd", 38) + c.n("dgrad", 37, 38) == 0 and c.n0("fwd", 38) + c.n0("dgrad", 37, 38) >= 1)),
        ({"Nconv": 2}, ("conv", (D2_CASE,), "dgrad"), ("tag 37 loses the 64 <- 128 data gradient", lambda c: c.n("dgrad", 37) == 0 and c.n0("dgrad", 37) == 2)),
        ({"Nconv": 2}, ("conv", (D2S_CASE,), "dgrad"), ("tag 37 keeps the 32 <- 64 data gradient", lambda c: c.n("dgrad", 37) == 2)),
        ({"Nconv": 3}, ("conv", (N1_CASE,), "fwd dgrad"), ("tag 38 (nconv1) takes nothing", lambda c: c.n("fwd", 38) + c.n("dgrad", 38) == 0 and c.n0("fwd", 38) + c.n0("dgrad", 38) >= 2)),
        ({"Nconv": 3}, ("conv", (D2_CASE, D2S_CASE), "dgrad"), ("tag 37 (dgrad2) keeps both forms", lambda c: c.n("dgrad", 37) == 2)),
    ],
    "bm": [
        ({"bm": 64}, ("conv", BM_CASES, "fwd dgrad"), ("tag 6, the 64 x 128 tile", lambda c: c.n("fwd", 6) == 4 and (c.case[3] <= 64 or c.n("dgrad", 6) == 2))),
        ({"bm": 128}, ("conv", BM_CASES, "fwd dgrad"),
         ("dcn_conv2d_stats_rows counts 128-row tiles: the automatic choice, so bitwise the default — except that a 3x3 data gradient towards 64 "
          "channels leaves the 256 x 64 split tile (tag 26) for the 128 x 64 one (tag 1)",
          lambda c: c.L.conv2d_stats_rows(*c.case[:3], c.case[4], *c.case[5:]) == -(-c.arm["raw"][..., 0].numel() // 128) and not c.differs("y") and
          ((c.n("dgrad", 1) == 2 and c.n0("dgrad", 26) == 2) if (c.case[3] <= 64 and c.case[5] == 3) else not c.differs("dx")))),
        ({"bm": 64}, ("gemm_nn", ((2048, 384, 256, 0), (1500, 132, 320, 300))), ("tag 7, the 64 x 128 NN tile", lambda c: c.n("nn", 7) == 1)),
        ({"bm": 128}, ("gemm_nn", ((2048, 384, 256, 0), (1500, 132, 320, 300))), ("a 128-row NN tile, not tag 7", lambda c: c.n("nn", 7) == 0 and c.n("nn", *NN_TAGS) == 1)),
    ],
    "k": [
        ({"precision": 0, "k": 16}, ("conv", K_CASES, "fwd dgrad"), ("tag 0 (16-float K-step) and not tag 15", _k_tag(16))),
        ({"precision": 0, "k": 32}, ("conv", K_CASES, "fwd dgrad"), ("tag 15 (32-float K-step) and not tag 0", _k_tag(32))),
    ],
    "ypresplit": [
        ({"ypresplit": 0}, ("conv", SPLIT_FREE, "fwd dgrad"),
         ("tag 24, the f16-split tile of igemm.hip, not conv1.hip / the strip kernels", lambda c: c.n("fwd", 24) == 4 and c.n("fwd", 35, 28, 29, 51) == 0 and c.n0("fwd", 24) == 0 and c.L.igemm_split_build(0, 0) == 162)),
    ],
    "qbk": [
        # (qbk / h2occ: other builds of the same tile under the same tag: the launcher's own choice, dcn_igemm_split_build, on the launches counted)
        ({"ypresplit": 0, "qbk": 32}, ("conv", SPLIT_FREE, "fwd dgrad"),
         ("tag 24 without a bank, and dcn_igemm_split_build(0) says K-step 32 (322; default 162)",
          lambda c: c.n("fwd", 24) == 4 and c.n("fwd", 35, 28, 29, 51) == 0 and c.L.igemm_split_build(0, 0) == 322)),
    ],
    "h2occ": [
        ({"ypresplit": 0, "h2occ": 1}, ("conv", SPLIT_FREE, "fwd dgrad"),
         ("tag 24 without a bank, and dcn_igemm_split_build(0) says 3 waves / SIMD (163; default 162)",
          lambda c: c.n("fwd", 24) == 4 and c.n("fwd", 35, 28, 29, 51) == 0 and c.L.igemm_split_build(0, 0) == 163)),
    ],
    "occ3": [
        ({"precision": 1, "occ3": 0}, ("conv", OCC_CASES, "fwd dgrad"), ("tag 16, and dcn_igemm_split_build(1, K-steps) says the 1-wave build (161) for both", _occ3(0))),
        ({"precision": 1, "occ3": 4}, ("conv", OCC_CASES, "fwd dgrad"), ("tag 16, and dcn_igemm_split_build(1, K-steps) says 163 at 2 K-steps, 161 at 36", _occ3(4))),
    ],
    "gk32": [
        ({"gk32": 32}, ("conv", CO32, "fwd"), ("tag 24 from K = 32 on: both launches", _gk32(32))),
        ({"gk32": 1 << 30}, ("conv", CO32, "fwd"), ("tag 2 (fp32 pipe) for both", _gk32(1 << 30))),
    ],
    "rnarrow": [
        ({"rnarrow": 1}, ("conv", NARROW, "fwd dgrad"), ("tags 24 / 26 instead of the fp32-pipe tags 1 / 2", lambda c: c.n("fwd", 24, 26) == 4 and c.n("fwd", 1, 2) == 0 and c.n0("fwd", 1, 2) == 4)),
    ],
    "tile64": [
        ({"tile64": 0}, ("conv", T64_CASES, "fwd dgrad"), ("tag 1 (128 x 64 fp32 pipe) instead of tag 26", lambda c: c.n("fwd", 1) == 4 and c.n("fwd", 26) == 0 and c.n0("fwd", 26) == 4)),
    ],
    "cwide64": [
        ({"cwide64": 0}, ("conv", W64_CASES, "wgrad"), ("tag 5 (fp32-pipe narrow tile) instead of tag 25", lambda c: c.n("wgrad", 5) == 1 and c.n("wgrad", 25) == 0 and c.n0("wgrad", 25) == 1)),
    ],
    "xwgtarget": [({"xwgtarget": t}, ("conv", XWG_NARROW, "wgrad"), ("split-K slabs, from dcn_conv2d_bwd_weight_ws", _splits_for(t))) for t in (1, 64, 4096)] +
                 [({"xwgtarget": t, "u3row": 0}, ("conv", XWG_WIDE, "wgrad"), ("split-K slabs, from dcn_conv2d_bwd_weight_ws", _splits_for(t))) for t in (1, 64, 4096)],
    "zwgsmall": [({"zwgsmall": t}, ("conv", ZWG_CASES, "wgrad"), ("split-K slabs, from dcn_conv2d_bwd_weight_ws", _splits_for(t))) for t in (1, 64, 4096)],
    "wsplit": [({"wsplit": v}, ("conv", WSPLIT_CASES, "wgrad"), (f"tag {t}", lambda c, t=t: c.n("wgrad", t) == 1)) for v, t in ((0, 5), (1, 17), (2, 20), (4, 25))],
    "9tap": [({"9tap": v}, ("conv", (W9_P, W9_Q, W9_R), "wgrad"), ("tag 36 on exactly the layers this value admits", _tap9(v))) for v in (0, 1, 2, 3)],
    "qtargetb16": [({"qtargetb16": t, "u3row": 0}, ("storage", "bf16s", B16_WG3), ("split-K slabs, from dcn_conv2d_bwd_weight_ws_b16", _splits_for(t, True))) for t in (1, 4096)],
    "qsmallb16": [({"qsmallb16": t}, ("storage", "bf16s", B16_WGS), ("split-K slabs, from dcn_conv2d_bwd_weight_ws_b16", _splits_for(t, True))) for t in (1, 4096)],
    "Bpc": [({"Bpc": v}, ("bn", BN_CASES), ("dcn_bn_apply_form", _bn_form(v))) for v in (0, 1)],
    "e2rpw": [({"e2rpw": r, "f2nt": nt}, ("score", SCORE_CASES), ("dcn_l2norm_score_fwd_form", _score_form(r, nt))) for r in (1, 2, 4, 8) for nt in (1, 0) if (r, nt) != (2, 0)],
    "f2nt": [({"f2nt": 0, "e2rpw": 2}, ("score", SCORE_CASES), ("dcn_l2norm_score_fwd_form", _score_form(2, 0)))],
    "Gemm3": [
        ({"Gemm3": 0}, ("coattn", COATTN_LARGE), ("tag 40 (gemm3.hip) took the nine products by default and takes none", lambda c: c.n("all", 40) == 0 and c.n0("all", 40) == 9)),
        ({"Gemm3": 1}, ("coattn", COATTN_LARGE), ("tag 40, the nine products, dcn_gemm3_variant 0", _g3(0))),
        ({"Gemm3": 257}, ("coattn", COATTN_LARGE), ("tag 40, the nine products, dcn_gemm3_variant 1", _g3(1))),
        ({"Gemm3": 513}, ("coattn", COATTN_LARGE), ("tag 40, the nine products, dcn_gemm3_variant 2", _g3(2))),
        ({"Gemm3": 769}, ("coattn", COATTN_LARGE), ("tag 40, the nine products, dcn_gemm3_variant 0: no schedule for 3", _g3(0))),
        ({"Gemm3": 257}, ("gemm3", _g3_cases), ("tag 40 == 1 (asserted by test_gemm3_presplit_operands), dcn_gemm3_variant 1", lambda c: c.L.gemm3_variant() == 1)),
        ({"Gemm3": 513}, ("gemm3", _g3_cases), ("tag 40 == 1 (asserted by test_gemm3_presplit_operands), dcn_gemm3_variant 2", lambda c: c.L.gemm3_variant() == 2)),
        ({"Gemm3": 769}, ("gemm3", _g3_cases), ("tag 40 == 1 (asserted by test_gemm3_presplit_operands), dcn_gemm3_variant 0", lambda c: c.L.gemm3_variant() == 0)),
    ],
}

# knobs whose arms an existing test already forces and compares: knob -> (module, test function[, helper it calls]); the source of the
# function (of the helper, which the function must call) must name the knob
COVERED_BY = {
    "jstem": ("test_ops_gpu", "test_stem_direct_kernel"),
    "3x3strip": ("test_ops_gpu", "test_conv3_strip_kernel"),
    "3bm": ("test_ops_gpu", "test_conv3_strip_kernel"),
    "3m16": ("test_ops_gpu", "test_bn_tap_on_stride1_data_gradients"),
    "U3m16": ("test_ops_gpu", "test_wgrad3_filter_row_kernel"),
    "u3row": ("test_ops_gpu", "test_wgrad3_filter_row_kernel"),
    "v3target": ("test_ops_gpu", "test_wgrad3_filter_row_kernel"),
    "9target": ("test_ops_gpu", "test_wgrad9_nine_tap_kernel"),
    "Y1wide": ("test_ops_gpu", "test_wgrad1x_wide_tile_kernel"),
    "Slabfold": ("test_ops_gpu", "test_slab_fold_is_bitwise_the_separate_pass"),
    "nnsplit": ("test_ops_gpu", "test_gemm_nn_split_pipe"),
    "split": ("test_ops_gpu", "test_split_pipe_forced_on_every_nt_tile"),
    "precision": ("test_ops_gpu", "test_split_pipe_is_fp32_accurate"),
    "2btile": ("test_b16_gpu", "test_b16_conv_forward_dgrad_wgrad_match_their_exact_model"),
    "3h16": ("test_b16_gpu", "test_b16_conv_forward_dgrad_wgrad_match_their_exact_model"),
    "Nb16": ("test_b16_gpu", "test_b16_conv_forward_dgrad_wgrad_match_their_exact_model", "_conv_case"),
    "Db16": ("test_b16_gpu", "test_b16_conv_forward_dgrad_wgrad_match_their_exact_model", "_conv_case"),
    "w3b16": ("test_b16_gpu", "test_b16_conv_forward_dgrad_wgrad_match_their_exact_model", "_conv_case"),
    "9b16": ("test_b16_gpu", "test_b16_conv_forward_dgrad_wgrad_match_their_exact_model", "_conv_case"),
    "H1gemm3": ("test_b16_gpu", "test_coattention_on_one_f16_piece_in_the_bf16_modes"),
    "1stages": ("test_ops_gpu", "test_conv1_lds_dma_kernel"),
}

# switches that make results wrong by construction exist only in ablation builds: knob -> (which values, compile flag)
EXEMPT = {
    "abl": ("every non-zero value", "-DDCN_ABL=1"),
    "3abl": ("every non-zero value", "-DC3_ABL=1"),
    "Gemm3": ("bits 4-7", "-DG3_ABL=1"),
    "Slabfold": ("< 0", "-DDCN_ABL=1"),
}

_ARM_IDS = [(k, i) for k, arms in ARMS.items() for i in range(len(arms))]


@pytest.mark.parametrize("knob,i", _ARM_IDS, ids=[f"{k}-{i}" for k, i in _ARM_IDS])
def test_arm_against_fp64(dev, knob, i):
    values, (kind, *args), evidence = ARMS[knob][i]
    assert knob in values
    args = [a() if callable(a) else a for a in args]
    WORKLOADS[kind](values, evidence, *args)
