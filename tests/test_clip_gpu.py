"""Global-norm gradient clipping and the non-finite skip of the fused optimiser steps (csrc/optim.hip: grad_sumsq_kernel,
grad_clip_coef_kernel, grad_scale_kernel and the clipped forms of the update kernels; dcnet_amd.optim) against fp64 norms computed on
the CPU and against torch.optim's single-tensor steps fed pre-clipped gradients.

Data: the shape list of test_optim_gpu.py (two pointer chunks, scalar tails, the grid-stride loop), generator seed 31, initial values
drawn first, then per step ``it`` the gradients ``randn * (it + 1)``.  Their fp64 norms are 1466.45, 2933.43, 4396.93, 5868.72, so
``max_norm = 2000`` leaves step 0 alone and clips steps 1-3."""
import copy
import functools
import math
import random

import numpy as np
import pytest
import torch

from util import build_product, close, synth_sd

pytestmark = pytest.mark.gpu

SHAPES = [(7,), (64, 33), (3, 3, 16, 5), (1,), (1024, 257), (40, 8, 3, 3)] * 8
TOL = 2e-6          # x max(1, max|ref|): the project's bar for an optimiser step (test_optim_gpu.py)
MAX_NORM = 2000.0
ULP = 2.0 ** -23    # one fp32 ulp, relative: double accumulation of 2.15 M terms errs by < 1e-9, which leaves the final rounding
OPTIMS = ["rmsprop", "adam", "sgd"]
STATE_KEYS = {"rmsprop": ("square_avg",), "adam": ("exp_avg", "exp_avg_sq"), "sgd": ("momentum_buffer",)}


@functools.lru_cache(maxsize=None)
def _data():
    """(initial values, gradients of steps 0..3, their fp64 norms) on the CPU — made once, never modified (users clone)"""
    g = torch.Generator().manual_seed(31)
    init = [torch.randn(*s, generator=g) for s in SHAPES]
    grads = [[torch.randn(*s, generator=g) * (it + 1) for s in SHAPES] for it in range(4)]
    norms = [math.sqrt(sum(float(t.double().pow(2).sum()) for t in gs)) for gs in grads]
    assert np.allclose(norms, [1466.45, 2933.43, 4396.93, 5868.72], atol=0.01), norms
    return init, grads, norms


def _coef_ref(norm64, max_norm=MAX_NORM):
    return np.float32(min(1.0, max_norm / (norm64 + 1e-6)))


def _norm_ok(got, norm64):
    got = float(got)
    print(f"norm {got!r} fp64 {norm64!r} rel {abs(got - float(np.float32(norm64))) / norm64:.3e}")
    assert abs(got - float(np.float32(norm64))) <= ULP * norm64, (got, norm64)


def _params(dev, values, grads=None):
    ps = [torch.nn.Parameter(t.clone().to(dev)) for t in values]
    if grads is not None:
        for p, g in zip(ps, grads):
            p.grad = g.clone().to(dev)
    return ps


def _view_of(t, dev):
    """the same values one float into a flat buffer: 4-byte aligned, as gradients bound to a flat all-reduce buffer are"""
    flat = torch.zeros(t.numel() + 5, device=dev)
    v = flat[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# ---- 1. the norm ----------------------------------------------------------------------------------------------------------------
def test_norm_meets_fp64_to_one_ulp_and_is_reproducible(dev):
    """For each of the four steps: within 2^-23 relative of the fp64 norm rounded to fp32 (not torch's fp32 norm, which is 1.1-1.6e-6
    off on this data); a second call gives the same bits; so do the same values as views one float off a 16-byte boundary."""
    from dcnet_amd.optim import clip_grad_norm_
    init, grads, norms = _data()
    for it in range(4):
        ps = _params(dev, init, grads[it])
        a = clip_grad_norm_(ps, 1e30)
        _norm_ok(a, norms[it])
        a = a.clone()
        b = clip_grad_norm_(ps, 1e30).clone()
        assert torch.equal(a, b), (it, float(a), float(b))
        for p, g in zip(ps, grads[it]):              # max_norm 1e30: the coefficient is exactly 1, nothing moved
            assert torch.equal(p.grad.cpu(), g)
        qs = _params(dev, init)
        for q, g in zip(qs, grads[it]):
            q.grad = _view_of(g, dev)
        c = clip_grad_norm_(qs, 1e30)
        assert all(q.grad.data_ptr() % 16 == 4 for q in qs) and all(p.grad.data_ptr() % 16 == 0 for p in ps)
        assert torch.equal(a, c), (it, float(a), float(c))


def test_norm_of_odd_lists(dev):
    """A 0-element tensor, a (1,) tensor and a parameter without a gradient: the first adds nothing, the last is left out.  And a
    gradient holding one 3e19 — whose square overflows fp32 — has a finite norm, the fp64 one."""
    from dcnet_amd.optim import clip_grad_norm_
    ps = [torch.nn.Parameter(torch.zeros(0, 3, device=dev)), torch.nn.Parameter(torch.zeros(1, device=dev)),
          torch.nn.Parameter(torch.ones(5, device=dev))]
    ps[0].grad = torch.zeros(0, 3, device=dev)
    ps[1].grad = torch.full((1,), -3.0, device=dev)
    n = clip_grad_norm_(ps, 1.5)
    assert float(n) == 3.0 and ps[2].grad is None
    coef = np.float32(1.5) / (np.float32(3.0) + np.float32(1e-6))
    assert abs(float(ps[1].grad) - (-3.0 * float(coef))) <= 3.0 * 2.0 ** -21
    assert float(clip_grad_norm_(ps[1], 1e30)) == abs(float(ps[1].grad))          # a single tensor, as torch's function accepts

    g = torch.Generator().manual_seed(32)
    big = [torch.randn(1000, generator=g), torch.randn(33, 7, generator=g)]
    big[1][5, 3] = 3e19
    norm64 = math.sqrt(sum(float(t.double().pow(2).sum()) for t in big))
    qs = _params(dev, big, big)
    n = clip_grad_norm_(qs, 1e30, error_if_nonfinite=True)              # finite: the synchronising form has nothing to raise
    assert math.isfinite(float(n))
    _norm_ok(n, norm64)
    qs[0].grad[17] = float("inf")
    before = [q.grad.clone() for q in qs]
    with pytest.raises(RuntimeError, match="non-finite"):
        clip_grad_norm_(qs, 1.0, error_if_nonfinite=True)
    assert all(torch.equal(q.grad, b) for q, b in zip(qs, before))      # raised before any gradient was touched


# ---- 2. clip_grad_norm_ in place ------------------------------------------------------------------------------------------------
def test_clip_grad_norm_in_place(dev):
    """Step 0 (norm 1466 < 2000): the coefficient is exactly 1.0 and the gradients keep their bits.  Steps 1-3: every element within
    2^-21 relative of g * coef_ref, coef_ref = float32(2000 / (norm64 + 1e-6)) — four fp32 roundings (norm, add, divide, multiply) of
    2^-24 each, doubled for margin."""
    from dcnet_amd.optim import clip_grad_norm_
    init, grads, norms = _data()
    for it in range(4):
        ps = _params(dev, init, grads[it])
        n = clip_grad_norm_(ps, MAX_NORM)
        _norm_ok(n, norms[it])
        coef = _coef_ref(norms[it])
        assert (coef == 1.0) == (it == 0)
        worst = 0.0
        for p, g in zip(ps, grads[it]):
            got = p.grad.cpu()
            if it == 0:
                assert torch.equal(got, g)
            else:
                want = g.double() * float(coef)
                worst = max(worst, float(((got.double() - want).abs() / want.abs().clamp_min(1e-300)).max()))
                assert bool(((got.double() - want).abs() <= 2.0 ** -21 * want.abs()).all()), (it, tuple(g.shape))
        print(f"step {it}: coef_ref {coef!r}, worst relative error {worst:.3e}")


# ---- 3. the fused steps ---------------------------------------------------------------------------------------------------------
def _groups(ps):
    return [{"params": ps[:20]}, {"params": ps[20:], "lr": 1e-3}]


def _make(name, ps, fused, **clip):
    from dcnet_amd import optim
    if name == "rmsprop":
        return optim.RMSprop(_groups(ps), lr=1e-2, weight_decay=5e-4, **clip) if fused else \
            torch.optim.RMSprop(_groups(ps), lr=1e-2, weight_decay=5e-4, foreach=False)
    if name == "adam":
        return optim.Adam(_groups(ps), lr=1e-2, weight_decay=5e-4, **clip) if fused else \
            torch.optim.Adam(_groups(ps), lr=1e-2, weight_decay=5e-4, foreach=False)
    return optim.SGD(_groups(ps), lr=1e-2, momentum=0.99, **clip) if fused else \
        torch.optim.SGD(_groups(ps), lr=1e-2, momentum=0.99, foreach=False)


def _set_grads(ps, grads, dev, scale=None):
    for p, g in zip(ps, grads):
        g = g.clone().to(dev)
        p.grad = g if scale is None else g * torch.tensor(scale, dtype=torch.float32, device=dev)      # one fp32 multiply, as mul_ does


def _agree(name, pa, pb, oa, ob):
    for x, y in zip(pa, pb):
        close(x, y, TOL, "param")
        for k in STATE_KEYS[name]:
            close(oa.state[x][k], ob.state[y][k], TOL, k)


def _bitwise(name, pa, pb, oa, ob):
    for x, y in zip(pa, pb):
        assert torch.equal(x, y), tuple(x.shape)
        for k in STATE_KEYS[name]:
            assert torch.equal(oa.state[x][k], ob.state[y][k]), (k, tuple(x.shape))


@pytest.mark.parametrize("name", OPTIMS)
def test_clipped_steps_match_torch_on_preclipped_gradients(dev, name):
    """Four steps with max_grad_norm = 2000 against torch.optim (foreach=False) fed gradients multiplied in fp32 by coef_ref: parameters
    and every state tensor within 2e-6 x max(1, max|ref|); .grad keeps its bits; opt.grad_norm meets the fp64 norm to one ulp."""
    init, grads, norms = _data()
    pa, pb = _params(dev, init), _params(dev, init)
    oa, ob = _make(name, pa, True, max_grad_norm=MAX_NORM), _make(name, pb, False)
    assert oa.grad_norm is None
    for it in range(4):
        _set_grads(pa, grads[it], dev)
        _set_grads(pb, grads[it], dev, scale=float(_coef_ref(norms[it])))
        oa.step(); ob.step()
        _norm_ok(oa.grad_norm, norms[it])
        for p, g in zip(pa, grads[it]):
            assert torch.equal(p.grad.cpu(), g)
    _agree(name, pa, pb, oa, ob)
    assert oa.skipped_steps() == 0
    if name != "sgd":
        assert all(float(oa.state[x]["step"]) == 4 for x in pa)


@pytest.mark.parametrize("name", OPTIMS)
def test_a_threshold_never_reached_changes_no_bit(dev, name):
    """max_grad_norm = 1e30: the coefficient is exactly 1.0, g * 1.0 is g — bitwise the run without the option."""
    init, grads, _ = _data()
    pa, pb = _params(dev, init), _params(dev, init)
    oa, ob = _make(name, pa, True, max_grad_norm=1e30), _make(name, pb, True)
    for it in range(4):
        _set_grads(pa, grads[it], dev); _set_grads(pb, grads[it], dev)
        oa.step(); ob.step()
    _bitwise(name, pa, pb, oa, ob)
    assert ob.grad_norm is None and float(oa.grad_norm) > 0


@pytest.mark.parametrize("name", OPTIMS)
def test_entry_points_of_a_step(dev, name, monkeypatch):
    """Options off: a step calls exactly the entry points it called before there were any — one dcn_rmsprop_step / dcn_sgd_step, or
    dcn_adam_prepare + dcn_adam_step, per group, nothing else.  Options on: dcn_grad_sumsq and dcn_grad_clip_coef once, over the
    gradients of all groups, then the groups' ``_clipped`` calls."""
    from dcnet_amd.lib import SIGNATURES, lib
    L = lib()
    calls = []
    for sym in SIGNATURES:
        if sym.startswith(("dcn_grad_", "dcn_rmsprop_", "dcn_adam_", "dcn_sgd_")):
            fn = getattr(L, sym[4:])
            monkeypatch.setattr(L, sym[4:], lambda *a, _fn=fn, _sym=sym: (calls.append((_sym, a)), _fn(*a))[1])
    init, grads, _ = _data()
    per_group = {"rmsprop": ["dcn_rmsprop_step"], "adam": ["dcn_adam_prepare", "dcn_adam_step"], "sgd": ["dcn_sgd_step"]}[name]
    pa = _params(dev, init, grads[0])
    _make(name, pa, True).step()
    assert [c[0] for c in calls] == per_group * 2
    del calls[:]
    pb = _params(dev, init, grads[0])
    pb[30].grad = None                               # a parameter that sits the step out is not in the norm either
    _make(name, pb, True, max_grad_norm=MAX_NORM).step()
    assert [c[0] for c in calls] == ["dcn_grad_sumsq_slots", "dcn_grad_sumsq", "dcn_grad_clip_coef"] + [s + "_clipped" for s in per_group] * 2
    assert calls[1][1][2] == len(SHAPES) - 1         # count: one norm over both groups' live gradients


# ---- 4. the skip ----------------------------------------------------------------------------------------------------------------
def _poisoned(grads, bad):
    out = [g.clone() for g in grads]
    out[25][3, 11] = bad                             # one element of one gradient (a (64, 33) tensor of the second chunk and group)
    return out


@pytest.mark.parametrize("bad,max_norm", [(float("inf"), MAX_NORM), (float("nan"), None)], ids=["inf-clipped", "nan-skip-only"])
@pytest.mark.parametrize("name", OPTIMS)
def test_nonfinite_step_is_skipped(dev, name, bad, max_norm):
    """Three steps with skip_nonfinite; step 1 has one inf (with max_grad_norm = 2000) or one NaN (skip_nonfinite alone) in one gradient.
    Over that step every parameter, every state tensor and Adam's device step words keep their bits, skipped_steps() is 1; after
    step 2 everything equals a torch run of steps 0 and 2 only (same bar); state_dict() reads step == 2; and a fresh optimiser that
    loads that state_dict continues bitwise like the uninterrupted one."""
    init, grads, norms = _data()
    pa, pb = _params(dev, init), _params(dev, init)
    oa, ob = _make(name, pa, True, max_grad_norm=max_norm, skip_nonfinite=True), _make(name, pb, False)
    coef = (lambda it: float(_coef_ref(norms[it]))) if max_norm else (lambda it: None)
    _set_grads(pa, grads[0], dev); _set_grads(pb, grads[0], dev, scale=coef(0))
    oa.step(); ob.step()
    assert oa.skipped_steps() == 0

    before = [(x.detach().clone(), {k: oa.state[x][k].clone() for k in STATE_KEYS[name]}) for x in pa]
    words = {gi: t["steps"].clone() for gi, t in getattr(oa, "_tables", {}).items()}
    _set_grads(pa, _poisoned(grads[1], bad), dev)
    oa.step()
    for x, (p0, st0) in zip(pa, before):
        assert torch.equal(x, p0), tuple(x.shape)
        for k in STATE_KEYS[name]:
            assert torch.equal(oa.state[x][k], st0[k]), (k, tuple(x.shape))
    for gi, w in words.items():
        assert torch.equal(oa._tables[gi]["steps"], w) and w.tolist() == [1] * len(w)
    assert (name == "adam") == bool(words)
    assert oa.skipped_steps() == 1
    assert not math.isfinite(float(oa.grad_norm))

    _set_grads(pa, grads[2], dev); _set_grads(pb, grads[2], dev, scale=coef(2))
    oa.step(); ob.step()
    _agree(name, pa, pb, oa, ob)
    _norm_ok(oa.grad_norm, norms[2])
    sd = copy.deepcopy(oa.state_dict())
    if name != "sgd":
        assert len(sd["state"]) == len(SHAPES) and all(float(s["step"]) == 2 for s in sd["state"].values())
        assert all(float(oa.state[x]["step"]) == 2 for x in pa)
        assert [float(s["step"]) for s in oa.state_dict()["state"].values()] == [2.0] * len(SHAPES)      # a second look takes nothing off again
    assert oa.skipped_steps() == 1

    pc = _params(dev, [x.detach().cpu() for x in pa])
    oc = _make(name, pc, True, max_grad_norm=max_norm, skip_nonfinite=True)
    oc.load_state_dict(sd)
    _set_grads(pa, grads[3], dev); _set_grads(pc, grads[3], dev)
    oa.step(); oc.step()
    _bitwise(name, pa, pc, oa, oc)
    assert torch.equal(oa.grad_norm, oc.grad_norm) and oc.skipped_steps() == 0
    if name != "sgd":
        assert all(float(s["step"]) == 3 for o in (oa, oc) for s in o.state_dict()["state"].values())


@pytest.mark.parametrize("name", OPTIMS)
def test_inf_without_the_skip_follows_torch(dev, name):
    """skip_nonfinite off, one inf in step 1: torch's clip_grad_norm_ gives norm inf, coefficient 2000 / inf = 0, and inf * 0 = NaN in
    that element, 0 everywhere else.  The fused step computes the same: NaN where torch has NaN, the bar elsewhere."""
    init, grads, norms = _data()
    pa, pb = _params(dev, init), _params(dev, init)
    oa, ob = _make(name, pa, True, max_grad_norm=MAX_NORM), _make(name, pb, False)
    _set_grads(pa, grads[0], dev); _set_grads(pb, grads[0], dev, scale=float(_coef_ref(norms[0])))
    oa.step(); ob.step()
    bad = _poisoned(grads[1], float("inf"))
    _set_grads(pa, bad, dev); _set_grads(pb, bad, dev, scale=0.0)
    assert int(torch.isnan(pb[25].grad).sum()) == 1
    oa.step(); ob.step()
    assert float(oa.grad_norm) == float("inf") and oa.skipped_steps() == 0

    def same(a, b, what):
        a, b = a.detach().double(), b.detach().double()
        assert torch.equal(torch.isnan(a), torch.isnan(b)), what
        ref = max(1.0, float(torch.nan_to_num(b).abs().max()))
        assert torch.allclose(a, b, rtol=0.0, atol=TOL * ref, equal_nan=True), what
        return int(torch.isnan(a).sum())

    nans = 0
    for x, y in zip(pa, pb):
        nans += same(x, y, "param")
        for k in STATE_KEYS[name]:
            same(oa.state[x][k], ob.state[y][k], k)
    assert nans == 1


# ---- 5. inside a graph, optimiser level -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", OPTIMS)
def test_captured_step_equals_eager_steps_bitwise(dev, name, monkeypatch):
    """An eager first step on static gradient tensors, then ``opt.step()`` alone captured on one stream (no forked branches) and
    replayed with finite, inf and finite gradients copied into them: bitwise the same four steps made eagerly on a twin — parameters,
    state, the norm, the skip counter and the ``step`` the state_dict shows."""
    init, grads, _ = _data()
    pick = [0, 1, 3, 4, 5]                           # (7,), (64, 33), (1,), (1024, 257), (40, 8, 3, 3)
    values = [init[i] for i in pick]
    feed = [[grads[it][i] for i in pick] for it in range(4)]
    feed[2][1] = feed[2][1].clone(); feed[2][1][7, 7] = float("inf")
    clip = dict(max_grad_norm=800.0, skip_nonfinite=True)           # the norms of these five tensors: ~518 x (it + 1): step 0 is not clipped
    from dcnet_amd import optim
    make = {"rmsprop": lambda q: optim.RMSprop(q, lr=1e-2, weight_decay=5e-4, **clip), "adam": lambda q: optim.Adam(q, lr=1e-2, weight_decay=5e-4, **clip),
            "sgd": lambda q: optim.SGD(q, lr=1e-2, momentum=0.99, **clip)}[name]

    pe = _params(dev, values)
    oe = make(pe)
    norms_e = []
    for it in range(4):
        _set_grads(pe, feed[it], dev)
        oe.step()
        norms_e.append(oe.grad_norm.clone())

    pg = _params(dev, values, feed[0])               # .grad: the static tensors
    og = make(pg)
    with monkeypatch.context() as mp:                # a first step inside a capture is refused (the workspace is made by an eager step),
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)      # before anything is launched
        with pytest.raises(RuntimeError, match="eager step first"):
            og.step()
    og = make(pg)
    og.step()
    assert torch.equal(og.grad_norm, norms_e[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        og.step()                                    # (captured, not run: the host counters advanced, the device did nothing)
    for it in range(1, 4):
        for p, g in zip(pg, feed[it]):
            p.grad.copy_(g)
        if it > 1:
            og.bump_steps()
        graph.replay()
        assert torch.equal(og.grad_norm, norms_e[it]), it
    torch.cuda.synchronize()
    _bitwise(name, pe, pg, oe, og)
    assert og.skipped_steps() == oe.skipped_steps() == 1
    assert float(norms_e[0]) < 800.0 < float(norms_e[1]) and not math.isfinite(float(norms_e[2]))
    if name != "sgd":
        for o in (oe, og):
            assert [float(s["step"]) for s in o.state_dict()["state"].values()] == [3.0] * len(pick)


# ---- 6. the training step -------------------------------------------------------------------------------------------------------
def _setup(dev, size, n, seed, name, **clip):
    from dcnet_amd.parallel import freeze_gradless
    from dcnet_amd.train import make_optimizer
    from dcnet_amd.utils.synth import synth_boxes, synth_inputs
    m = build_product(size, synth_sd(size), dev)
    freeze_gradless(m)
    opt = make_optimizer(m, 1e-4, name, **clip)
    image, word_id, word_mask = (t.to(dev) for t in synth_inputs(n, size, seed=seed))
    bbox = synth_boxes(n, size, seed=seed).to(dev)
    return m, opt, image, word_id, word_mask, bbox


def _same_training_state(m1, o1, m2, o2, steps):
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    for k in sd1:
        assert torch.equal(sd1[k], sd2[k]), k
    s1, s2 = o1.state_dict()["state"], o2.state_dict()["state"]
    assert s1.keys() == s2.keys() and len(s1) > 100
    for k in s1:
        assert s1[k].keys() == s2[k].keys()
        for name, v in s1[k].items():
            if name == "step":
                assert float(v) == float(s2[k]["step"]) == steps, (k, float(v), float(s2[k]["step"]))
            else:
                assert torch.equal(v, s2[k][name]), (k, name)


TRAIN_MAX_NORM = 20000.0     # between the smallest and the largest norm measured with clipping off (the test's docstring)


@pytest.mark.parametrize("name", ["rmsprop", "adam"])
def test_replayed_clipped_steps_equal_eager_steps_bitwise(dev, name):
    """The scenario of test_optim_gpu.test_replayed_steps_equal_eager_steps_bitwise at 256 x 256, n = 2, four steps under a changing
    learning rate, with max_grad_norm set: once with train_step and once as one eager warm-up step + the captured pass + two replays
    — identical losses, parameters, running statistics, optimiser state, ``step`` counters and the gradient norm of the last step.

    The threshold: with clipping off (max_grad_norm = 1e30) the four norms measured on an MI355X were
        rmsprop  38091.40, 14661.65, 29880.33, 8251.12
        adam     38091.40, 11712.88, 14731.79, 6797.45
    (step 0 is the same gradient for both).  20000 lies between the smallest and the largest of either run, so step 0 is clipped
    (coefficient 0.525) and steps with a smaller norm are not: the clipped runs measured 38091.40, 18202.23, 19291.17, 9721.47
    (rmsprop) and 38091.40, 11572.77, 21043.55, 8076.44 (adam), so both arms run in either.  The test asserts from ``grad_norm``
    that at least one step had coef < 1 and prints the norms."""
    from dcnet_amd.graph import GraphedTrainStep
    from dcnet_amd.train import adjust_learning_rate, train_step
    size, n, steps = 256, 2, 4
    max_norm = TRAIN_MAX_NORM
    lr_of = lambda it: 1e-4 if it < 2 else 1e-4 * (1 - it / 10.0)     # the constructor's two steps run at the initial rate
    m1, o1, image, word_id, word_mask, bbox = _setup(dev, size, n, 21, name, max_grad_norm=max_norm)
    random.seed(99)
    ref_losses, ref_norms = [], []
    for it in range(steps):
        adjust_learning_rate(o1, 0, lr_of(it), 1, 0.9)
        loss, _ = train_step(m1, o1, image, word_id, word_mask, bbox, size)
        ref_losses.append(float(loss)); ref_norms.append(o1.grad_norm.clone())
    print("norms under max_grad_norm", max_norm, [float(v) for v in ref_norms])
    assert any(float(v) + 1e-6 > max_norm for v in ref_norms), "no step was clipped"       # coef < 1

    m2, o2, image, word_id, word_mask, bbox = _setup(dev, size, n, 21, name, max_grad_norm=max_norm)
    random.seed(99)
    step = GraphedTrainStep(m2, o2, image, word_id, word_mask, bbox, size, warmup=1)      # steps 0 (eager) and 1 (captured pass)
    got = [None, float(step.loss)]
    for it in range(2, steps):
        adjust_learning_rate(o2, 0, lr_of(it), 1, 0.9)
        got.append(float(step()))
    assert got[1:] == ref_losses[1:], (got, ref_losses)
    assert torch.equal(step.grad_norm, ref_norms[-1]), (float(step.grad_norm), float(ref_norms[-1]))
    _same_training_state(m1, o1, m2, o2, steps)
