"""The weight EMA inside the fused step, the in-place swap and AdamW (csrc/optim.hip: ema_prepare_kernel, ema_update_kernel,
tensor_swap_kernel, adamw_prepare_kernel, adamw_kernel / adamw_clip_kernel; dcnet_amd.optim.WeightEMA / AdamW) against the fp64
recursion, against torch.optim.AdamW's single-tensor step, and for the properties the replayed training step leans on: a misaligned
view rounds like an aligned tensor, a tensor nobody trains keeps its bits, a skipped step skips the average, a replayed step is
bitwise the eager one, and a checkpoint carries the shadows and the update count."""
import copy
import functools
import math
import random

import numpy as np
import pytest
import torch

from util import build_product, close, synth_sd

pytestmark = pytest.mark.gpu

TOL = 2e-6          # x max(1, max|ref|): tests/test_optim_gpu.py's bar for an optimiser step
# 0 values; below, at and above one 16-byte group; one block with a scalar tail; two blocks; and 2 x 131072 + 5: 65 537 groups of 16
# bytes, past the 128 blocks x 256 threads of blocks_for (the grid-stride loop, both of its trips, and a tail)
SIZES = [0, 1, 3, 4, 5, 1023, 1025, 2 * 131072 + 5]
COUNT = 70          # more than two pointer chunks of 32
TWINS = {68: 5, 69: 7}        # tensors 68 and 69 are views one float off a 16-byte boundary, fed what tensors 5 (1023) and 7 (262149) are fed


class Bag(torch.nn.Module):
    """A model that is a list of tensors and one integer buffer."""

    def __init__(self, tensors):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(t) for t in tensors])
        self.register_buffer("seen", torch.tensor([7, 11], dtype=torch.int64, device=tensors[0].device))


def _view_of(t, dev):
    """the same values one float into a flat buffer: 4-byte aligned, as tensors bound to a flat buffer are"""
    flat = torch.zeros(t.numel() + 5, device=dev)
    v = flat[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _kernel_data():
    """(initial values, the sources of five updates) of the 70 tensors on the CPU — made once, never modified"""
    g = torch.Generator().manual_seed(41)
    sizes = [SIZES[i % len(SIZES)] for i in range(COUNT)]
    for i, j in TWINS.items():
        sizes[i] = sizes[j]
    draw = lambda: [torch.randn(n, generator=g) for n in sizes]
    init, feeds = draw(), [draw() for _ in range(5)]
    for vals in [init] + feeds:
        for i, j in TWINS.items():
            vals[i] = vals[j]
    assert sizes[5] == 1023 and sizes[7] == 2 * 131072 + 5 and sizes[0] == 0
    return init, feeds


def _bag(dev, init):
    return Bag([_view_of(t, dev) if i in TWINS else t.clone().to(dev) for i, t in enumerate(init)])


# ---- 1. the kernels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [0.0, 3.0])
def test_updates_meet_the_fp64_recursion(dev, tau):
    """Five updates at decay 0.9 with freshly drawn sources, against s <- s + w_t (x - s) in fp64 from the same fp32 inputs with
    w_t = weight_at(t): every shadow within 2e-6 x max(1, max|ref|) (an update rounds three times, each by at most 2^-24 of a value
    no larger than the largest one: five of them stay under 15 x 6e-8 = 9e-7).  tau = 0: w = 0.1, the form for w < 0.5; tau = 3:
    w = 0.745, 0.562, 0.431, 0.331, 0.255, both forms.  After each update the device weight word is within one fp32 ulp of
    weight_at(t) and the step word reads t.  The views one float off a 16-byte boundary hold bitwise what their aligned twins hold."""
    from dcnet_amd.optim import WeightEMA, weight_at
    init, feeds = _kernel_data()
    bag = _bag(dev, init)
    assert all(bag.ps[i].data_ptr() % 16 == 4 for i in TWINS) and all(bag.ps[j].data_ptr() % 16 == 0 for j in TWINS.values())
    ema = WeightEMA(bag, decay=0.9, tau=tau)
    assert ema.updates() == 0 and not ema.swapped and len(ema.shadow) == COUNT and "seen" not in ema.shadow
    shadows = [ema.shadow[f"ps.{i}"] for i in range(COUNT)]
    assert all(torch.equal(s.cpu(), t) for s, t in zip(shadows, init))              # shadow_0 = theta_0
    ref = [t.double() for t in init]
    forms = set()
    for it, feed in enumerate(feeds):
        t = it + 1
        with torch.no_grad():
            for p, x in zip(bag.ps, feed):
                p.copy_(x)
        ema.update()
        w = weight_at(t, 0.9, tau)
        forms.add(np.float32(w) < 0.5)
        got_w = float(ema._w)
        print(f"update {t}: weight {got_w!r}, weight_at {w!r}")
        assert abs(got_w - w) <= float(np.spacing(np.float32(w))) and ema.updates() == t
        ref = [s + w * (x.double() - s) for s, x in zip(ref, feed)]
    assert forms == ({True} if tau == 0 else {True, False})
    worst = 0.0
    for i, (s, r) in enumerate(zip(shadows, ref)):
        assert s.shape == r.shape
        if r.numel():
            worst = max(worst, float((s.cpu().double() - r).abs().max()) / max(1.0, float(r.abs().max())))
            close(s, r, TOL, f"shadow {i} ({r.numel()} values)")
    print(f"tau {tau}: worst error {worst:.3e} of max(1, max|ref|)")
    for i, j in TWINS.items():
        assert shadows[i].data_ptr() % 16 == 0 and torch.equal(_bits(shadows[i]), _bits(shadows[j])), (i, j)
    for p, x in zip(bag.ps, feeds[-1]):             # the update only reads the model
        assert torch.equal(p.detach().cpu(), x)
    assert bag.seen.tolist() == [7, 11]


def test_misaligned_shadows_round_like_aligned_ones(dev):
    """Both sides of the update one float off a 16-byte boundary (the shadow as well: placed by hand, the pointer table rebuilt), and
    only one side: bitwise the aligned run, for both forms of the lerp."""
    from dcnet_amd.optim import WeightEMA, _ptrs
    g = torch.Generator().manual_seed(42)
    init = [torch.randn(n, generator=g) for n in (1023, 2 * 131072 + 5, 5)]
    feeds = [[torch.randn(t.shape, generator=g) for t in init] for _ in range(3)]

    def run(place_model, place_shadow):
        bag = Bag([place_model(t) for t in init])
        ema = WeightEMA(bag, decay=0.9, tau=3.0)
        ema._shadow = [place_shadow(t) for t in init]
        ema._p_shadow = _ptrs([s.data_ptr() for s in ema._shadow])
        for feed in feeds:
            with torch.no_grad():
                for p, x in zip(bag.ps, feed):
                    p.copy_(x)
            ema.update()
        return ema._shadow

    aligned, off = (lambda t: t.clone().to(dev)), (lambda t: _view_of(t, dev))
    want = run(aligned, aligned)
    for pm, ps in ((off, off), (aligned, off), (off, aligned)):
        for a, b in zip(want, run(pm, ps)):
            assert torch.equal(_bits(a), _bits(b)), a.numel()


def test_a_tensor_equal_to_its_shadow_keeps_its_bits(dev):
    """src == shadow bitwise (a tensor nobody trains): bit-identical after updates with w = 0.745, 0.562 (x - d (1 - w)) and 0.431,
    0.331 (s + w d) — zeros of either sign, denormals, the largest finite value and ordinary values alike."""
    from dcnet_amd.optim import WeightEMA
    g = torch.Generator().manual_seed(43)
    special = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 1e-38, 3.4028234e38, -3.4028234e38, 1.0, -1.0, 1 / 3, 1e-20, 6e4])
    vals = [torch.cat([special, torch.randn(1029, generator=g)]), special.clone(), torch.randn(3, generator=g) * 1e6]
    bag = Bag([vals[0].to(dev), _view_of(vals[1], dev), vals[2].to(dev)])
    ema = WeightEMA(bag, decay=0.9, tau=3.0)
    before = [_bits(s).clone() for s in ema.shadow.values()]
    ws = []
    for _ in range(4):
        ema.update()
        ws.append(float(ema._w))
        for s, b, v in zip(ema.shadow.values(), before, vals):
            assert torch.equal(_bits(s), b) and torch.equal(_bits(s).cpu(), v.view(torch.int32))
    assert ws[0] > ws[1] > 0.5 > ws[2] > ws[3]


# ---- 2. the swap ------------------------------------------------------------------------------------------------------------------
def test_swap_exchanges_in_place_and_back(dev):
    from dcnet_amd.optim import WeightEMA
    init, feeds = _kernel_data()
    bag = _bag(dev, init)
    ema = WeightEMA(bag, decay=0.5, tau=0.0)
    with torch.no_grad():
        for p, x in zip(bag.ps, feeds[0]):
            p.copy_(x)
    ema.update()
    shadows = list(ema.shadow.values())
    model_bits = [_bits(p).clone() for p in bag.ps]
    shadow_bits = [_bits(s).clone() for s in shadows]
    addresses = [p.data_ptr() for p in bag.ps] + [s.data_ptr() for s in shadows] + [bag.seen.data_ptr()]
    assert any(not torch.equal(a, b) for a, b in zip(model_bits, shadow_bits))
    sd = ema.state_dict()
    assert sorted(sd) == ["decay", "shadow", "tau", "updates"] and sd["updates"] == 1 and sd["decay"] == 0.5 and sd["tau"] == 0.0
    assert list(sd["shadow"]) == [f"ps.{i}" for i in range(COUNT)]

    ema.swap()
    assert ema.swapped
    for p, s, mb, sb in zip(bag.ps, shadows, model_bits, shadow_bits):
        assert torch.equal(_bits(p), sb) and torch.equal(_bits(s), mb), p.numel()
    with pytest.raises(RuntimeError, match="swap"):
        ema.update()
    with pytest.raises(RuntimeError, match="swap"):
        ema.state_dict()
    with pytest.raises(RuntimeError, match="swap"):
        ema.load_state_dict(sd)
    assert ema.updates() == 1
    ema.swap()
    assert not ema.swapped
    for p, s, mb, sb in zip(bag.ps, shadows, model_bits, shadow_bits):
        assert torch.equal(_bits(p), mb) and torch.equal(_bits(s), sb), p.numel()
    assert bag.seen.tolist() == [7, 11]
    assert addresses == [p.data_ptr() for p in bag.ps] + [s.data_ptr() for s in shadows] + [bag.seen.data_ptr()]

    with pytest.raises(ZeroDivisionError):          # the way back is taken when the body raises, too
        with ema.applied() as inside:
            assert inside is ema and ema.swapped and torch.equal(_bits(bag.ps[7]), shadow_bits[7])
            1 / 0
    assert not ema.swapped and all(torch.equal(_bits(p), mb) for p, mb in zip(bag.ps, model_bits))

    other = _bag(dev, init)                          # the one-way case
    ema.copy_to(other)
    assert all(torch.equal(_bits(p), sb) for p, sb in zip(other.ps, shadow_bits)) and all(torch.equal(_bits(s), sb) for s, sb in zip(shadows, shadow_bits))


def test_load_state_dict_is_strict_and_in_place(dev):
    from dcnet_amd.optim import WeightEMA
    g = torch.Generator().manual_seed(44)
    vals = [torch.randn(5, generator=g), torch.randn(33, 3, generator=g)]
    a, b = WeightEMA(Bag([v.to(dev) for v in vals]), 0.9, 3.0), WeightEMA(Bag([(v * 2).to(dev) for v in vals]), 0.9, 3.0)
    a.update(); a.update()
    sd = copy.deepcopy(a.state_dict())
    addresses = [s.data_ptr() for s in b.shadow.values()] + [b._step.data_ptr(), b._w.data_ptr()]
    b.load_state_dict({**sd, "shadow": {"module." + k: v.cpu() for k, v in sd["shadow"].items()}})      # a DDP writer's keys, host tensors
    assert b.updates() == 2 and all(torch.equal(x, y) for x, y in zip(a.shadow.values(), b.shadow.values()))
    assert addresses == [s.data_ptr() for s in b.shadow.values()] + [b._step.data_ptr(), b._w.data_ptr()]
    with pytest.raises(KeyError, match="ps.1"):
        b.load_state_dict({**sd, "shadow": {"ps.0": sd["shadow"]["ps.0"]}})
    with pytest.raises(KeyError, match="extra"):
        b.load_state_dict({**sd, "shadow": {**sd["shadow"], "extra": torch.zeros(1)}})
    with pytest.raises(ValueError, match="shape"):
        b.load_state_dict({**sd, "shadow": {**sd["shadow"], "ps.1": torch.zeros(3, 33)}})
    assert b.updates() == 2 and all(torch.equal(x, y) for x, y in zip(a.shadow.values(), b.shadow.values()))      # a refused load wrote nothing


# ---- 3. with the fused optimisers -------------------------------------------------------------------------------------------------
def _make(name, params, **kw):
    from dcnet_amd import optim
    return {"rmsprop": lambda: optim.RMSprop(params, lr=1e-2, weight_decay=5e-4, **kw), "adam": lambda: optim.Adam(params, lr=1e-2, weight_decay=5e-4, **kw),
            "sgd": lambda: optim.SGD(params, lr=1e-2, momentum=0.99, **kw), "adamw": lambda: optim.AdamW(params, lr=1e-2, **kw)}[name]()


@pytest.mark.parametrize("name", ["rmsprop", "adam", "sgd", "adamw"])
def test_a_skipped_step_skips_the_average(dev, name):
    """skip_nonfinite with an attached EMA: a finite step updates the average (t = 1), a step with one inf in one gradient leaves every
    shadow, the weight word and the update count alone (skipped_steps() == 1), and the next finite step is update t = 2 — its weight
    weight_at(2), its result the lerp of the untouched shadows towards the new parameters."""
    from dcnet_amd.optim import WeightEMA, weight_at
    g = torch.Generator().manual_seed(45)
    vals = [torch.randn(n, generator=g) for n in (1025, 7, 40 * 33, 1)]
    bag = Bag([v.to(dev) for v in vals])
    opt = _make(name, list(bag.parameters()), skip_nonfinite=True)
    ema = WeightEMA(bag, decay=0.9, tau=3.0)
    opt.attach_ema(ema)

    def step(poison=None):
        for i, p in enumerate(bag.ps):
            p.grad = torch.randn(p.shape, generator=g).to(dev)
            if poison is not None and i == 2:
                p.grad[17] = poison
        opt.step()

    step()
    assert ema.updates() == 1 and opt.skipped_steps() == 0
    for s, p, v in zip(ema.shadow.values(), bag.ps, vals):
        close(s, v.double() + weight_at(1, 0.9, 3.0) * (p.detach().cpu().double() - v.double()), TOL, "first update")
    shadow_bits = [_bits(s).clone() for s in ema.shadow.values()]
    params = [p.detach().clone() for p in bag.ps]
    w1 = float(ema._w)

    step(poison=float("inf"))
    assert opt.skipped_steps() == 1 and ema.updates() == 1 and float(ema._w) == w1
    assert all(torch.equal(_bits(s), b) for s, b in zip(ema.shadow.values(), shadow_bits))
    assert all(torch.equal(p, q) for p, q in zip(bag.ps, params))

    step()
    assert opt.skipped_steps() == 1 and ema.updates() == 2
    w2 = weight_at(2, 0.9, 3.0)
    assert abs(float(ema._w) - w2) <= float(np.spacing(np.float32(w2)))
    for s, b, p in zip(ema.shadow.values(), shadow_bits, bag.ps):
        assert not torch.equal(_bits(s), b)
        old = b.view(torch.float32).cpu().double()
        close(s, old + w2 * (p.detach().cpu().double() - old), TOL, "update after the skip")

    opt.attach_ema(None)                             # detached: the step is the step again
    step()
    assert ema.updates() == 2


def test_entry_points_of_a_step_with_and_without_an_ema(dev, monkeypatch):
    """Without an EMA a step calls no EMA entry point; with one, dcn_ema_prepare + dcn_ema_update once, after the last group's update,
    with the step's control block (0 without clipping)."""
    from dcnet_amd.lib import SIGNATURES, lib
    from dcnet_amd.optim import SGD, WeightEMA
    L = lib()
    calls = []
    for sym in SIGNATURES:
        if sym.startswith(("dcn_grad_", "dcn_sgd_", "dcn_ema_", "dcn_tensor_")):
            fn = getattr(L, sym[4:])
            monkeypatch.setattr(L, sym[4:], lambda *a, _fn=fn, _sym=sym: (calls.append((_sym, a)), _fn(*a))[1])
    bag = Bag([torch.ones(9, device=dev), torch.ones(1030, device=dev)])

    def step(opt):
        for p in bag.ps:
            p.grad = torch.ones_like(p)
        del calls[:]
        opt.step()
        return [c[0] for c in calls]

    groups = lambda: [{"params": [bag.ps[0]]}, {"params": [bag.ps[1]], "lr": 1e-3}]
    plain = SGD(groups(), lr=1e-2, momentum=0.9)
    assert step(plain) == ["dcn_sgd_step"] * 2
    ema = WeightEMA(bag, 0.9, 0.0)
    plain.attach_ema(ema)
    assert step(plain) == ["dcn_sgd_step"] * 2 + ["dcn_ema_prepare", "dcn_ema_update"]
    assert calls[2][1][4] == 0 and calls[3][1][5] == 0
    clipped = SGD(groups(), lr=1e-2, momentum=0.9, max_grad_norm=1.0)
    clipped.attach_ema(ema)
    assert step(clipped) == ["dcn_grad_sumsq_slots", "dcn_grad_sumsq", "dcn_grad_clip_coef"] + ["dcn_sgd_step_clipped"] * 2 + ["dcn_ema_prepare", "dcn_ema_update"]
    ctl = clipped._clip_ws["ctrl"].data_ptr()
    assert calls[5][1][4] == ctl and calls[6][1][5] == ctl
    assert ema.updates() == 2
    for p in bag.ps:
        p.grad = None                                # a step without any gradient updates nothing
    del calls[:]
    plain.step()
    assert calls == [] and ema.updates() == 2


# ---- 4. AdamW ---------------------------------------------------------------------------------------------------------------------
# the data of test_optim_gpu.py / test_clip_gpu.py: 48 tensors = two pointer chunks, scalar tails, the grid-stride loop
SHAPES = [(7,), (64, 33), (3, 3, 16, 5), (1,), (1024, 257), (40, 8, 3, 3)] * 8
MAX_NORM = 2000.0


def _groups(ps):
    return [{"params": ps[:20]}, {"params": ps[20:], "lr": 1e-3}]


def _agree(pa, pb, oa, ob):
    for x, y in zip(pa, pb):
        close(x, y, TOL, "param")
        for k in ("exp_avg", "exp_avg_sq"):
            close(oa.state[x][k], ob.state[y][k], TOL, k)


def test_fused_adamw_matches_torch(dev):
    """The scenario of test_optim_gpu.test_fused_adam_matches_torch — two groups with different rates, 5 steps with gradients scaled by
    the step number — with decoupled weight decay 1e-2, against torch.optim.AdamW(foreach=False): parameters, exp_avg and exp_avg_sq
    within 2e-6 x max(1, max|ref|); the state_dicts load both ways and two more steps after the exchange still agree.  And
    Adam(decoupled_weight_decay=True) is the same thing, bitwise."""
    from dcnet_amd.optim import Adam, AdamW
    g = torch.Generator().manual_seed(5)
    init = [torch.randn(*s, generator=g) for s in SHAPES]
    mk = lambda: [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    pa, pb, pc = mk(), mk(), mk()
    oa = AdamW(_groups(pa), lr=1e-2, weight_decay=1e-2)
    ob = torch.optim.AdamW(_groups(pb), lr=1e-2, weight_decay=1e-2, foreach=False)
    oc = Adam(_groups(pc), lr=1e-2, weight_decay=1e-2, decoupled_weight_decay=True)

    def steps(first, count, sides):
        for it in range(first, first + count):
            for ps in zip(*[s[0] for s in sides]):
                gr = torch.randn(ps[0].shape, generator=g).to(dev) * (it + 1)
                for p in ps:
                    p.grad = gr.clone()
            for _, o in sides:
                o.step()

    steps(0, 5, [(pa, oa), (pb, ob), (pc, oc)])
    _agree(pa, pb, oa, ob)
    for x, z in zip(pa, pc):
        assert torch.equal(x, z) and all(torch.equal(oa.state[x][k], oc.state[z][k]) for k in ("exp_avg", "exp_avg_sq"))
    assert all(float(oa.state[x]["step"]) == 5 for x in pa)
    assert oa._tables[0]["scal"].shape == (20, 3)
    sa, sb = copy.deepcopy(oa.state_dict()), copy.deepcopy(ob.state_dict())
    strip = lambda groups: [{k: v for k, v in grp.items() if k != "foreach"} for grp in groups]       # (torch's side was told foreach=False)
    assert strip(sa["param_groups"]) == strip(sb["param_groups"]) and sa["param_groups"][0]["decoupled_weight_decay"] is True
    oa.load_state_dict(sb); ob.load_state_dict(sa)
    for grp in ob.param_groups:
        grp["foreach"] = False
    steps(5, 2, [(pa, oa), (pb, ob)])
    _agree(pa, pb, oa, ob)
    assert all(float(oa.state[x]["step"]) == float(ob.state[y]["step"]) == 7 for x, y in zip(pa, pb))


@functools.lru_cache(maxsize=None)
def _clip_data():
    """test_clip_gpu.py's data: seed 31, initial values first, then per step ``it`` the gradients ``randn * (it + 1)``; their fp64 norms
    are 1466.45, 2933.43, 4396.93, 5868.72, so max_norm = 2000 leaves step 0 alone and clips steps 1-3"""
    g = torch.Generator().manual_seed(31)
    init = [torch.randn(*s, generator=g) for s in SHAPES]
    grads = [[torch.randn(*s, generator=g) * (it + 1) for s in SHAPES] for it in range(4)]
    norms = [math.sqrt(sum(float(t.double().pow(2).sum()) for t in gs)) for gs in grads]
    assert np.allclose(norms, [1466.45, 2933.43, 4396.93, 5868.72], atol=0.01), norms
    return init, grads, norms


def test_clipped_adamw_steps_match_torch_on_preclipped_gradients(dev):
    """Four steps with max_grad_norm = 2000 against torch.optim.AdamW(foreach=False) fed gradients multiplied in fp32 by
    coef_ref = float32(min(1, 2000 / (norm64 + 1e-6))): the bar of the plain step; .grad keeps its bits."""
    from dcnet_amd.optim import AdamW
    init, grads, norms = _clip_data()
    pa = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    pb = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    oa = AdamW(_groups(pa), lr=1e-2, weight_decay=1e-2, max_grad_norm=MAX_NORM)
    ob = torch.optim.AdamW(_groups(pb), lr=1e-2, weight_decay=1e-2, foreach=False)
    for it in range(4):
        coef = np.float32(min(1.0, MAX_NORM / (norms[it] + 1e-6)))
        assert (coef == 1.0) == (it == 0)
        for x, y, gr in zip(pa, pb, grads[it]):
            x.grad = gr.clone().to(dev)
            y.grad = gr.clone().to(dev) * torch.tensor(float(coef), dtype=torch.float32, device=dev)      # one fp32 multiply, as mul_ does
        oa.step(); ob.step()
        assert abs(float(oa.grad_norm) - float(np.float32(norms[it]))) <= 2.0 ** -23 * norms[it]
        assert all(torch.equal(x.grad.cpu(), gr) for x, gr in zip(pa, grads[it]))
    _agree(pa, pb, oa, ob)
    assert oa.skipped_steps() == 0 and all(float(oa.state[x]["step"]) == 4 for x in pa)


def test_captured_adamw_step_equals_eager_steps_bitwise(dev):
    """The scenario of test_clip_gpu.test_captured_step_equals_eager_steps_bitwise for AdamW with an attached EMA: an eager first step
    on static gradient tensors, then ``opt.step()`` alone captured and replayed with finite, inf and finite gradients copied into
    them, the learning rate read from the device scalar and changed between replays: bitwise the same four steps made eagerly on a
    twin — parameters, state, every shadow, the EMA's step and weight words, the norm and the skip counter."""
    from dcnet_amd.optim import AdamW, WeightEMA
    init, grads, _ = _clip_data()
    pick = [0, 1, 3, 4, 5]
    values = [init[i] for i in pick]
    feed = [[grads[it][i] for i in pick] for it in range(4)]
    feed[2][1] = feed[2][1].clone(); feed[2][1][7, 7] = float("inf")
    lrs = [1e-2, 1e-2, 7e-3, 5e-3]

    def make():
        bag = Bag([v.clone().to(dev) for v in values])
        opt = AdamW(list(bag.parameters()), lr=1e-2, weight_decay=1e-2, max_grad_norm=800.0, skip_nonfinite=True)
        opt.device_lr = True
        ema = WeightEMA(bag, decay=0.9, tau=3.0)
        opt.attach_ema(ema)
        return bag, opt, ema

    be, oe, ee = make()
    for it in range(4):
        oe.param_groups[0]["lr"] = lrs[it]
        for p, gr in zip(be.ps, feed[it]):
            p.grad = gr.clone().to(dev)
        oe.step()
    norm_e = oe.grad_norm.clone()

    bg, og, eg = make()
    for p, gr in zip(bg.ps, feed[0]):
        p.grad = gr.clone().to(dev)                  # the static gradient tensors
    og.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        og.step()                                    # (captured, not run)
    for it in range(1, 4):
        og.param_groups[0]["lr"] = lrs[it]
        og.sync_lr()
        for p, gr in zip(bg.ps, feed[it]):
            p.grad.copy_(gr)
        if it > 1:
            og.bump_steps()
        graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(be.ps, bg.ps):
        assert torch.equal(x, y), tuple(x.shape)
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(oe.state[x][k], og.state[y][k]), (k, tuple(x.shape))
    for (k, a), b in zip(ee.shadow.items(), eg.shadow.values()):
        assert torch.equal(_bits(a), _bits(b)), k
        assert not torch.equal(a, dict(be.named_parameters())[k])
    assert ee.updates() == eg.updates() == 3 and torch.equal(_bits(ee._w), _bits(eg._w))
    assert torch.equal(og.grad_norm, norm_e) and og.skipped_steps() == oe.skipped_steps() == 1
    for o in (oe, og):
        assert [float(s["step"]) for s in o.state_dict()["state"].values()] == [3.0] * len(pick)


# ---- 5. the training step -----------------------------------------------------------------------------------------------------------
def _setup(dev, size, n, seed, with_ema, name="adamw"):
    from dcnet_amd.optim import WeightEMA
    from dcnet_amd.parallel import freeze_gradless
    from dcnet_amd.train import make_optimizer
    from dcnet_amd.utils.synth import synth_boxes, synth_inputs
    m = build_product(size, _synth_sd(size), dev)
    freeze_gradless(m)
    opt = make_optimizer(m, 1e-4, name)
    ema = None
    if with_ema:
        ema = WeightEMA(m, decay=0.9, tau=3.0)       # (a short memory: five steps move the average visibly, and w_t differs in every step)
        opt.attach_ema(ema)                          # before the graph is built
    image, word_id, word_mask = (t.to(dev) for t in synth_inputs(n, size, seed=seed))
    bbox = synth_boxes(n, size, seed=seed).to(dev)
    return m, opt, ema, (image, word_id, word_mask, bbox)


@functools.lru_cache(maxsize=None)
def _synth_sd(size):
    return synth_sd(size)


def _run(dev, with_ema, graphed, size=256, n=4, steps=5):
    """five steps under a changing learning rate: eagerly, or as one eager warm-up step + the captured pass + three replays"""
    from dcnet_amd.graph import GraphedTrainStep
    from dcnet_amd.train import adjust_learning_rate, train_step
    lr_of = lambda it: 1e-4 if it < 2 else 1e-4 * (1 - it / 10.0)     # the constructor's two steps run at the initial rate
    m, opt, ema, data = _setup(dev, size, n, 21, with_ema)
    random.seed(99)
    if not graphed:
        losses = []
        for it in range(steps):
            adjust_learning_rate(opt, 0, lr_of(it), 1, 0.9)
            losses.append(float(train_step(m, opt, *data, size)[0]))
    else:
        step = GraphedTrainStep(m, opt, *data, size, warmup=1)
        losses = [None, float(step.loss)]
        for it in range(2, steps):
            adjust_learning_rate(opt, 0, lr_of(it), 1, 0.9)
            losses.append(float(step()))
    return m, opt, ema, losses


def _same_model(m1, m2):
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    assert sd1.keys() == sd2.keys()
    for k in sd1:
        assert torch.equal(sd1[k], sd2[k]), k


def _same_optimizer(o1, o2, steps):
    s1, s2 = o1.state_dict()["state"], o2.state_dict()["state"]
    assert s1.keys() == s2.keys() and len(s1) > 100
    for k in s1:
        assert s1[k].keys() == s2[k].keys()
        for name, v in s1[k].items():
            if name == "step":
                assert float(v) == float(s2[k]["step"]) == steps, (k, float(v), float(s2[k]["step"]))
            else:
                assert torch.equal(v, s2[k][name]), (k, name)


def _same_ema(e1, e2, updates):
    assert e1.updates() == e2.updates() == updates and torch.equal(_bits(e1._w), _bits(e2._w))
    s1, s2 = e1.shadow, e2.shadow
    assert s1.keys() == s2.keys() and len(s1) > 400
    for k in s1:
        assert torch.equal(_bits(s1[k]), _bits(s2[k])), k


_kept = {}


def test_replayed_steps_with_an_ema_equal_eager_steps_bitwise(dev):
    """The scenario of test_optim_gpu.test_replayed_steps_equal_eager_steps_bitwise (256 x 256, N = 4, five steps under a changing
    learning rate) with the fused AdamW and an attached EMA: identical losses, parameters, running statistics, optimiser state, every
    shadow and the EMA's step and weight words.  The average has moved away from the weights, running statistics included."""
    m1, o1, e1, ref_losses = _run(dev, True, False)
    m2, o2, e2, got = _run(dev, True, True)
    assert got[1:] == ref_losses[1:], (got, ref_losses)
    _same_model(m1, m2)
    _same_optimizer(o1, o2, 5)
    _same_ema(e1, e2, 5)
    sd = m1.state_dict()
    assert set(e1.shadow) == {k for k, v in sd.items() if v.is_floating_point()} and len(sd) > len(e1.shadow)
    moved = [k for k, s in e1.shadow.items() if not torch.equal(s, sd[k])]
    assert any("running_mean" in k for k in moved) and any(k.endswith(".weight") for k in moved) and len(moved) > 100
    _kept["with_ema"] = ({k: v.clone() for k, v in sd.items()}, ref_losses)


def test_the_ema_only_reads(dev):
    """The same five steps without the EMA, eager and replayed: bitwise the parameters, running statistics and losses of the runs with it."""
    if "with_ema" not in _kept:
        m1, _, _, ref_losses = _run(dev, True, False)
        _kept["with_ema"] = ({k: v.clone() for k, v in m1.state_dict().items()}, ref_losses)
    want, ref_losses = _kept.pop("with_ema")
    m3, o3, e3, eager = _run(dev, False, False)
    m4, o4, e4, replayed = _run(dev, False, True)
    assert e3 is None and e4 is None and o3._ema is None
    assert eager == ref_losses and replayed[1:] == ref_losses[1:]
    _same_optimizer(o3, o4, 5)
    for m in (m3, m4):
        sd = m.state_dict()
        assert sd.keys() == want.keys()
        for k in sd:
            assert torch.equal(sd[k], want[k]), k


def test_evaluate_under_applied(dev):
    """Boxes from ``evaluate`` inside ``with ema.applied():`` equal those of a fresh model loaded with the shadows (integer buffers taken
    from the model), and after the context the model's state_dict is bitwise what it was."""
    from dcnet_amd.optim import WeightEMA
    from dcnet_amd.train import evaluate
    from dcnet_amd.utils.synth import synth_boxes, synth_inputs
    size, n = 256, 2
    m = build_product(size, _synth_sd(size), dev)
    ema = WeightEMA(m, decay=0.5, tau=0.0)
    g = torch.Generator(device=dev).manual_seed(46)
    with torch.no_grad():                            # the weights move (here: by 1 % noise), the average follows halfway
        for v in m.state_dict().values():
            if v.is_floating_point():
                v.mul_(1.0 + 0.01 * torch.randn(v.shape, generator=g, device=dev))
    ema.update()
    image, word_id, word_mask = (t.to(dev) for t in synth_inputs(n, size, seed=5))
    bbox = synth_boxes(n, size, seed=5).to(dev)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    shadow = {k: v.clone() for k, v in ema.state_dict()["shadow"].items()}
    assert any(not torch.equal(shadow[k], before[k]) for k in shadow)
    with ema.applied():
        acc, miou, boxes = evaluate(m, image, word_id, word_mask, bbox, size)
        boxes = boxes.clone()
        inside = m.state_dict()
        assert all(torch.equal(inside[k], shadow[k]) for k in shadow)
    after = m.state_dict()
    assert after.keys() == before.keys() and all(torch.equal(_bits(after[k]) if after[k].is_floating_point() else after[k],
                                                             _bits(before[k]) if before[k].is_floating_point() else before[k]) for k in after)
    fresh = build_product(size, _synth_sd(size), dev)
    fresh.load_state_dict({k: shadow.get(k, v) for k, v in before.items()}, strict=True)
    acc2, miou2, boxes2 = evaluate(fresh, image, word_id, word_mask, bbox, size)
    assert torch.equal(boxes, boxes2) and float(acc) == float(acc2) and float(miou) == float(miou2)


def test_resumed_run_with_an_ema_equals_uninterrupted_run_bitwise(dev, tmp_path):
    """3 steps, save_checkpoint with an "ema" entry, a fresh model, optimiser and EMA, load_checkpoint(..., ema=ema), 2 more steps:
    bitwise the 5 uninterrupted steps, shadows and update count included (w_t of steps 4 and 5 needs t from the checkpoint)."""
    from dcnet_amd.train import load_checkpoint, save_checkpoint, train_step
    size, n = 256, 2
    m1, o1, e1, data = _setup(dev, size, n, 22, True)
    random.seed(7)
    ref_losses = [float(train_step(m1, o1, *data, size)[0]) for _ in range(5)]

    m2, o2, e2, _ = _setup(dev, size, n, 22, True)
    random.seed(7)
    got = [float(train_step(m2, o2, *data, size)[0]) for _ in range(3)]
    path = save_checkpoint({"epoch": 3, "state_dict": m2.state_dict(), "best_loss": 1.0, "optimizer": o2.state_dict(), "ema": e2.state_dict()},
                           False, "resume", str(tmp_path))
    draws = random.getstate()
    m3, o3, e3, _ = _setup(dev, size, n, 23, True)
    assert e3.updates() == 0
    assert load_checkpoint(m3, path, o3, ema=e3) == (3, 1.0)
    assert e3.updates() == 3
    random.setstate(draws)
    got += [float(train_step(m3, o3, *data, size)[0]) for _ in range(2)]
    assert got == ref_losses, (got, ref_losses)
    _same_model(m1, m3)
    _same_optimizer(o1, o3, 5)
    _same_ema(e1, e3, 5)
