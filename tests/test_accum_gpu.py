"""Gradient accumulation inside the fused step (csrc/optim.hip: accum_prepare_kernel, grad_accumulate_kernel, accum_clip_coef_kernel;
``accum_steps`` of dcnet_amd.optim's classes; dcnet_amd.graph.GraphedTrainStep).  Everything here is bitwise: K calls with
``accum_steps=K`` against one call of the same class with ``accum_steps=1`` on the mean formed in torch, ``((g1 + g2) + ...) *
fl32(1/K)`` — fp32 additions in call order and one multiplication are what the pass computes, so there is no tolerance to choose."""
import ctypes
import functools
import random

import pytest
import torch

from util import build_product, synth_sd

pytestmark = pytest.mark.gpu

# body and tail edges of the 16-byte walk; (1024, 257) = 65 792 groups of 16 bytes, more than the 128 blocks x 256 threads of
# blocks_for (the grid-stride loop); 34 tensors cross the 32-tensor chunk edge
EDGES = [(1,), (3,), (4,), (5,), (7,), (64, 33)]
SHAPES = EDGES + [(1024, 257)] + [EDGES[i % len(EDGES)] for i in range(27)]
assert len(SHAPES) == 34
WINDOWS, KMAX = 3, 4
KEYS = {"rmsprop": ("square_avg",), "adam": ("exp_avg", "exp_avg_sq"), "adamw": ("exp_avg", "exp_avg_sq"), "sgd": ("momentum_buffer",)}
NAMES = ["rmsprop", "adam", "adamw", "sgd"]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _aligned(dev):
    return lambda t: t.clone().to(dev)


def _view(dev):
    """the same values one float into a flat buffer: 4-byte aligned, as tensors bound to a flat buffer are"""
    def place(t):
        flat = torch.zeros(t.numel() + 5, device=dev)
        v = flat[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.numel() == 0 or (v.data_ptr() % 16 == 4 and v.is_contiguous())
        return v
    return place


@functools.lru_cache(maxsize=None)
def _data():
    """(initial values, gradients [window][call] of the 34 tensors) on the CPU — made once, never modified.  Gradients of the size of
    the window's number: the mean is no multiple of any single call's gradient."""
    g = torch.Generator().manual_seed(318)
    init = [torch.randn(*s, generator=g) for s in SHAPES]
    grads = [[[torch.randn(*s, generator=g) * (w + 1) for s in SHAPES] for _ in range(KMAX)] for w in range(WINDOWS)]
    return init, grads


@functools.lru_cache(maxsize=None)
def _means(k):
    """the window means of the first ``k`` calls of every window, formed in torch: ((g1 + g2) + ...) * fl32(1/k)"""
    _, grads = _data()
    inv = torch.tensor(1 / k, dtype=torch.float32)
    out = []
    for w in range(WINDOWS):
        means = []
        for i in range(len(SHAPES)):
            s = grads[w][0][i]
            for j in range(1, k):
                s = s + grads[w][j][i]
            means.append(s * inv)
        out.append(means)
    return out


def _make(name, ps, **kw):
    from dcnet_amd import optim
    groups = [{"params": ps[:20]}, {"params": ps[20:], "lr": 1e-3}]
    if name == "rmsprop":
        return optim.RMSprop(groups, lr=1e-2, weight_decay=5e-4, **kw)
    if name == "adam":
        return optim.Adam(groups, lr=1e-2, weight_decay=5e-4, **kw)
    if name == "adamw":
        return optim.AdamW(groups, lr=1e-2, weight_decay=1e-2, **kw)
    return optim.SGD(groups, lr=1e-2, momentum=0.9, weight_decay=5e-4, **kw)


def _fresh(name, place, **kw):
    """parameters and the state the first step would create, all placed by ``place``"""
    init, _ = _data()
    ps = [torch.nn.Parameter(place(t)) for t in init]
    opt = _make(name, ps, **kw)
    for p in ps:
        opt.state[p] = {k: place(torch.zeros(p.shape)) for k in KEYS[name]}
        if name != "sgd":
            opt.state[p]["step"] = torch.zeros((), dtype=torch.float32)
    return ps, opt


def _snapshot(ps, opt, ema=None, host_steps=True):
    """every bit a non-boundary call must leave alone: parameters, state tensors, host counters, Adam's device step words and scalars
    (zeros before the group's first step makes them), the EMA's shadows and count.  ``host_steps=False`` leaves the host counters
    out: under skip_nonfinite they count windows until state_dict() reconciles them."""
    snap = [p.detach().clone() for p in ps]
    for p in ps:
        snap += [v.clone() for k, v in opt.state[p].items() if torch.is_tensor(v) and (host_steps or k != "step")]
    if hasattr(opt, "_tables"):
        for gi, group in enumerate(opt.param_groups):
            tab, n, width = opt._tables.get(gi), len(group["params"]), 3 if group.get("decoupled_weight_decay") else 2
            snap += [tab["steps"].clone(), tab["scal"].clone()] if tab else \
                [torch.zeros(n, dtype=torch.int32, device=ps[0].device), torch.zeros(n, width, device=ps[0].device)]
    if ema is not None:
        snap += [s.clone() for s in ema.shadow.values()] + [ema._step.clone(), ema._w.clone()]
    return snap


def _unchanged(a, b):
    return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))


def _state_equal(name, pa, oa, pb, ob):
    for i, (x, y) in enumerate(zip(pa, pb)):
        assert _same(x, y), ("param", i, tuple(x.shape))
        for k in KEYS[name]:
            assert _same(oa.state[x][k], ob.state[y][k]), (k, i, tuple(x.shape))
        if name != "sgd":
            assert float(oa.state[x]["step"]) == float(ob.state[y]["step"]), i
    ta, tb = getattr(oa, "_tables", {}), getattr(ob, "_tables", {})
    assert ta.keys() == tb.keys()
    for gi in ta:
        assert torch.equal(ta[gi]["steps"], tb[gi]["steps"])


def _run_windows(name, k, place, windows, ema_of=None, **kw):
    """``windows`` windows of ``k`` calls with ``accum_steps=k``.  After every non-boundary call nothing but the accumulation buffers
    has changed (and ``grad_norm`` keeps its bits); after the boundary call ``.grad`` holds the torch mean.  Returns (parameters,
    optimiser, the norm bits after each window, the EMA)."""
    _, grads = _data()
    ps, opt = _fresh(name, place, accum_steps=k, **kw)
    ema = ema_of(ps, opt) if ema_of else None
    norms = []
    for w in windows:
        for j in range(k):
            assert opt.window_position == j and opt.at_boundary == (j == k - 1)
            before = _snapshot(ps, opt, ema)
            norm_before = None if opt.grad_norm is None else opt.grad_norm.clone()
            for p, gr in zip(ps, grads[w][j]):
                p.grad = place(gr)
            opt.step()
            if j < k - 1:
                assert _unchanged(before, _snapshot(ps, opt, ema)), (w, j)
                for p, gr in zip(ps, grads[w][j]):           # a non-boundary call only reads .grad
                    assert _same(p.grad, gr.to(p.device))
                if norm_before is not None:
                    assert _same(opt.grad_norm, norm_before)
        for i, (p, m) in enumerate(zip(ps, _means(k)[w])):
            assert _same(p.grad, m.to(p.device)), ("mean", w, i, tuple(p.shape))
        norms.append(None if opt.grad_norm is None else opt.grad_norm.clone())
    assert opt.window_position == 0
    return ps, opt, norms, ema


def _run_reference(name, k, place, windows, ema_of=None, **kw):
    """the same class with ``accum_steps=1``, stepped once per window on the torch mean"""
    ps, opt = _fresh(name, place, **kw)
    ema = ema_of(ps, opt) if ema_of else None
    norms = []
    for w in windows:
        for p, m in zip(ps, _means(k)[w]):
            p.grad = place(m)
        opt.step()
        norms.append(None if opt.grad_norm is None else opt.grad_norm.clone())
    return ps, opt, norms, ema


# ---- 0. the pass itself ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_the_pass_by_phase_with_an_empty_tensor(dev, k):
    """dcn_accum_prepare + dcn_grad_accumulate on the 34 tensors plus one of 0 values (NULL pointers), aligned and as views 4 bytes off a
    16-byte boundary: two windows of k calls.  The block reads (position, phase, fl32(1/k), windows closed) after every call; the first
    call overwrites buffers filled with NaN; off the boundary the gradients keep their bits; on it they hold the torch mean and the
    buffers keep theirs.  k = 1: a window of one call touches nothing."""
    from dcnet_amd.lib import lib
    L = lib()
    _, grads = _data()
    inv_bits = int(torch.tensor(1 / k, dtype=torch.float32).view(torch.int32))
    results = []
    for place in (_aligned(dev), _view(dev)):
        acc = [place(torch.full(s, float("nan"))) for s in SHAPES] + [torch.empty(0, device=dev)]
        g = [place(torch.zeros(s)) for s in SHAPES] + [torch.empty(0, device=dev)]
        n = len(acc)
        ptrs = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
        numel = (ctypes.c_int64 * n)(*[t.numel() for t in acc])
        assert numel[n - 1] == 0 and acc[n - 1].data_ptr() == 0
        blk = torch.zeros(4, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        for w in range(2):
            for j in range(k):
                for t, gr in zip(g, grads[w][j]):
                    t.copy_(gr)
                acc_before = [a.clone() for a in acc]
                L.accum_prepare(blk.data_ptr(), k, stream)
                L.grad_accumulate(ptrs(acc), ptrs(g), numel, n, blk.data_ptr(), stream)
                last = j == k - 1
                phase = 3 if k == 1 else (2 if last else (0 if j == 0 else 1))
                assert blk.tolist() == [0 if last else j + 1, phase, inv_bits, w + (1 if last else 0)], (w, j, blk.tolist())
                if last:
                    assert all(_same(t, m.to(dev)) for t, m in zip(g, _means(k)[w])), (w, j)
                    assert all(_same(a, b) for a, b in zip(acc, acc_before))
                else:
                    assert all(_same(t, gr.to(dev)) for t, gr in zip(g, grads[w][j]))
                    assert not any(bool(torch.isnan(a).any()) for a in acc)
        results.append([t.clone() for t in acc + g])
    assert all(_same(a, b) for a, b in zip(*results))


# ---- 1. bitwise against the plain step ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3, 4])
@pytest.mark.parametrize("name", NAMES)
def test_windows_equal_plain_steps_on_the_mean_bitwise(dev, name, k):
    """Two windows of k calls (k = 2: first and boundary only; 3: an inexact 1/k; 4: two middle calls) against the same class with
    accum_steps=1 stepped once per window on the mean: parameters, every state tensor, the step counters and Adam's step words are
    bit-equal; the run on views 4 bytes off a 16-byte boundary equals the aligned one."""
    pr, orf, _, _ = _run_reference(name, k, _aligned(dev), (0, 1))
    pa, oa, norms, _ = _run_windows(name, k, _aligned(dev), (0, 1))
    assert norms == [None, None] and oa.skipped_steps() == 0
    _state_equal(name, pa, oa, pr, orf)
    pv, ov, _, _ = _run_windows(name, k, _view(dev), (0, 1))
    assert all(p.data_ptr() % 16 == 4 and p.grad.data_ptr() % 16 == 4 for p in pv)
    _state_equal(name, pv, ov, pa, oa)
    if name != "sgd":
        assert all(float(oa.state[p]["step"]) == 2 for p in pa)
        assert all(float(v["step"]) == 2 for v in oa.state_dict()["state"].values())


# ---- 2. clipping acts on the mean ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_clipped_windows_equal_clipped_steps_on_the_mean(dev, name):
    """max_grad_norm = 1 against window norms of several hundred: every window clips.  K = 3, two windows, aligned and misaligned:
    state bit-equal to the clipped accum_steps=1 step on the mean, grad_norm bit-equal to the reference arm's after every window and
    unchanged during the non-boundary calls (_run_windows)."""
    pr, orf, norms_r, _ = _run_reference(name, 3, _aligned(dev), (0, 1), max_grad_norm=1.0)
    assert all(float(x) > 100.0 for x in norms_r)
    for place in (_aligned(dev), _view(dev)):
        pa, oa, norms, _ = _run_windows(name, 3, place, (0, 1), max_grad_norm=1.0)
        assert all(_same(x, y) for x, y in zip(norms, norms_r)), (norms, norms_r)
        _state_equal(name, pa, oa, pr, orf)


# ---- 3. a non-finite window is skipped as a whole ---------------------------------------------------------------------------------------
class Bag(torch.nn.Module):
    def __init__(self, ps):
        super().__init__()
        self.ps = torch.nn.ParameterList(ps)


def _ema_of(ps, opt):
    from dcnet_amd.optim import WeightEMA
    ema = WeightEMA(Bag(ps), decay=0.9, tau=3.0)
    opt.attach_ema(ema)
    return ema


@pytest.mark.parametrize("name", ["rmsprop", "adam", "sgd"])
def test_window_with_an_inf_is_skipped_and_the_next_starts_clean(dev, name):
    """skip_nonfinite, K = 3, three windows, an inf in micro-step 2 of window 2: window 2 changes nothing (parameters, state, step
    words, the attached EMA's shadows and count), skipped_steps() is 1, and window 3 ends bit-equal to a run that never had window 2.
    The host step counters read 2 after state_dict()."""
    _, grads = _data()
    place = _aligned(dev)
    pr, orf, _, er = _run_windows(name, 3, place, (0, 2), ema_of=_ema_of, skip_nonfinite=True)

    ps, opt = _fresh(name, place, accum_steps=3, skip_nonfinite=True)
    ema = _ema_of(ps, opt)
    for w in range(3):
        before = _snapshot(ps, opt, ema, host_steps=False)
        for j in range(3):
            for i, (p, gr) in enumerate(zip(ps, grads[w][j])):
                p.grad = place(gr)
                if (w, j, i) == (1, 1, 5):
                    p.grad.view(-1)[1000] = float("inf")
            opt.step()
        if w == 0:
            assert opt.skipped_steps() == 0 and ema.updates() == 1 and not _unchanged(before, _snapshot(ps, opt, ema, host_steps=False))
        if w == 1:
            assert _unchanged(before, _snapshot(ps, opt, ema, host_steps=False))
            assert opt.skipped_steps() == 1 and ema.updates() == 1
            assert not bool(torch.isfinite(opt.grad_norm))
    assert opt.skipped_steps() == 1 and ema.updates() == 2 == er.updates()
    sd = opt.state_dict()
    if name != "sgd":
        assert all(float(v["step"]) == 2 for v in sd["state"].values())
    _state_equal(name, ps, opt, pr, orf)
    for a, b in zip(ema.shadow.values(), er.shadow.values()):
        assert _same(a, b)
    assert bool(torch.isfinite(opt.grad_norm)) and _same(opt.grad_norm, orf.grad_norm)


# ---- 4. the EMA follows the windows -------------------------------------------------------------------------------------------------
def test_ema_updates_once_per_window(dev):
    """SGD, K = 2, no clipping, an attached EMA: updates() reads 0, 1, 1, 2 after the four calls, the shadows move only on the boundary
    calls (_run_windows) and end bit-equal to those of the accum_steps=1 run on the means."""
    _, grads = _data()
    place = _aligned(dev)
    ps, opt = _fresh("sgd", place, accum_steps=2)
    ema = _ema_of(ps, opt)
    seen = []
    for w in range(2):
        for j in range(2):
            for p, gr in zip(ps, grads[w][j]):
                p.grad = place(gr)
            opt.step()
            seen.append(ema.updates())
    assert seen == [0, 1, 1, 2] and opt.grad_norm is None
    pr, orf, _, er = _run_reference("sgd", 2, place, (0, 1), ema_of=_ema_of)
    pa, oa, _, ea = _run_windows("sgd", 2, place, (0, 1), ema_of=_ema_of)
    assert ea.updates() == er.updates() == 2
    for a, b, c in zip(ea.shadow.values(), er.shadow.values(), ema.shadow.values()):
        assert _same(a, b) and _same(a, c)


def test_learning_rate_is_the_one_at_the_boundary_call(dev):
    """Schedules are in units of updates: the rate set during calls 1 ... K-1 is never used, the update takes the rate in force at call
    K — eager (a kernel argument) and with device_lr (the device scalar).  Against accum_steps=1 at that rate on the mean, bitwise."""
    _, grads = _data()
    place = _aligned(dev)
    pr, orf = _fresh("sgd", place)
    for w in range(2):
        orf.param_groups[0]["lr"], orf.param_groups[1]["lr"] = 3e-2 / (w + 1), 3e-3 / (w + 1)
        for p, m in zip(pr, _means(3)[w]):
            p.grad = place(m)
        orf.step()
    for device_lr in (False, True):
        ps, opt = _fresh("sgd", place, accum_steps=3)
        opt.device_lr = device_lr
        for w in range(2):
            for j in range(3):
                scale = 1.0 if j == 2 else 100.0 * (j + 1)
                opt.param_groups[0]["lr"], opt.param_groups[1]["lr"] = scale * 3e-2 / (w + 1), scale * 3e-3 / (w + 1)
                for p, gr in zip(ps, grads[w][j]):
                    p.grad = place(gr)
                opt.step()
        _state_equal("sgd", ps, opt, pr, orf)


# ---- 5. captured against eager --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["adam", "rmsprop"])
def test_replayed_optimizer_step_walks_through_the_window(dev, name):
    """The optimiser alone, K = 3 with max_grad_norm and an EMA, static gradient tensors: one eager call, the captured pass, five
    replays (bump_steps after each replay but the first, as GraphedTrainStep does) under a learning rate that changes every call,
    against seven eager calls: parameters, state, step counters, step words, norm and shadows bit-equal after every call."""
    _, grads = _data()
    place = _aligned(dev)
    feed = [grads[w][j] for w in range(3) for j in range(3)][:7]
    lrs = [1e-2 * (1 - it / 10.0) for it in range(7)]

    def set_lr(opt, it):
        opt.param_groups[0]["lr"], opt.param_groups[1]["lr"] = lrs[it], lrs[it] / 10

    pe, oe = _fresh(name, place, accum_steps=3, max_grad_norm=1.0)
    ee = _ema_of(pe, oe)
    trail = []
    for it in range(7):
        set_lr(oe, it)
        for p, gr in zip(pe, feed[it]):
            p.grad = place(gr)
        oe.step()
        trail.append((_snapshot(pe, oe, ee), oe.grad_norm.clone(), oe.window_position))

    pg, og = _fresh(name, place, accum_steps=3, max_grad_norm=1.0)
    eg = _ema_of(pg, og)
    og.device_lr = True
    static = [place(gr) for gr in feed[0]]
    for p, t in zip(pg, static):
        p.grad = t
    set_lr(og, 0)
    og.step()
    assert _unchanged(trail[0][0], _snapshot(pg, og, eg))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        og.step()                                    # (captured, not run: the host's window position advanced, the device's did not)
    assert og.window_position == 2
    for it in range(1, 7):
        set_lr(og, it)
        og.sync_lr()
        for t, gr in zip(static, feed[it]):
            t.copy_(gr)
        if it > 1:
            og.bump_steps()
        graph.replay()
        assert _unchanged(trail[it][0], _snapshot(pg, og, eg)), it
        assert _same(og.grad_norm, trail[it][1]) and og.window_position == trail[it][2], it
    assert og.window_position == 1 and eg.updates() == 2
    if name == "adam":
        assert all(float(og.state[p]["step"]) == 2 for p in pg) and og._tables[0]["steps"].tolist() == [2] * 20


def _setup(dev, size, n, seed, **kw):
    from dcnet_amd.parallel import freeze_gradless
    from dcnet_amd.train import make_optimizer
    from dcnet_amd.utils.synth import synth_boxes, synth_inputs
    m = build_product(size, synth_sd(size), dev)
    freeze_gradless(m)
    opt = make_optimizer(m, 1e-4, "rmsprop", **kw)
    image, word_id, word_mask = (t.to(dev) for t in synth_inputs(n, size, seed=seed))
    bbox = synth_boxes(n, size, seed=seed).to(dev)
    return m, opt, image, word_id, word_mask, bbox


def test_replayed_training_steps_equal_eager_ones_bitwise(dev):
    """The scenario of test_graph_gpu.test_replayed_steps_equal_eager_steps_bitwise with accum_steps=2: six calls under a changing
    learning rate, once with train_step and once as one eager warm-up step + the captured pass + four replays — identical losses,
    parameters, running statistics, optimiser state and ``step`` counters (3: they count updates); the parameters keep their bits
    across each non-boundary replay and move on each boundary one."""
    from dcnet_amd.graph import GraphedTrainStep
    from dcnet_amd.train import adjust_learning_rate, train_step
    size, n, calls = 256, 4, 6
    lr_of = lambda it: 1e-4 if it < 2 else 1e-4 * (1 - it / 10.0)     # the constructor's two calls run at the initial rate
    m1, o1, image, word_id, word_mask, bbox = _setup(dev, size, n, 21, accum_steps=2)
    random.seed(99)
    ref_losses = []
    for it in range(calls):
        adjust_learning_rate(o1, 0, lr_of(it), 1, 0.9)
        ref_losses.append(float(train_step(m1, o1, image, word_id, word_mask, bbox, size)[0]))
    assert o1.window_position == 0

    m2, o2, image, word_id, word_mask, bbox = _setup(dev, size, n, 21, accum_steps=2)
    random.seed(99)
    step = GraphedTrainStep(m2, o2, image, word_id, word_mask, bbox, size, warmup=1)      # calls 0 (eager) and 1 (captured pass): one window
    assert step.window_position == 0
    got = [None, float(step.loss)]
    params = [p for p in m2.parameters() if p.grad is not None]
    assert len(params) > 100
    for it in range(2, calls):
        adjust_learning_rate(o2, 0, lr_of(it), 1, 0.9)
        before = [p.detach().clone() for p in params]
        got.append(float(step()))
        same = [_same(p, b) for p, b in zip(params, before)]
        assert step.window_position == (it + 1) % 2
        assert all(same) if it % 2 == 0 else not all(same), it
    assert got[1:] == ref_losses[1:], (got, ref_losses)
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    for k in sd1:
        assert torch.equal(sd1[k], sd2[k]), k
    s1, s2 = o1.state_dict()["state"], o2.state_dict()["state"]
    assert s1.keys() == s2.keys() and len(s1) > 100
    for k in s1:
        assert float(s1[k]["step"]) == float(s2[k]["step"]) == calls // 2, (k, float(s1[k]["step"]), float(s2[k]["step"]))
        assert torch.equal(s1[k]["square_avg"], s2[k]["square_avg"]), k


# ---- 6. the reducer runs once per window, on the mean -----------------------------------------------------------------------------------
def test_post_backward_reducer_runs_once_per_window_on_the_mean(dev):
    """GraphedTrainStep with a post-backward reducer (forward + backward captured, accumulate / reducer / step eager), K = 2, warm-up
    1: over the constructor's two calls and two more the reducer is called twice, each time between accumulate() and step() of a
    boundary call, and the gradient it sees is ((g1 + g2) * 0.5) of the two micro-gradients, bit for bit."""
    from dcnet_amd.graph import GraphedTrainStep
    size, n = 256, 2
    m, opt, image, word_id, word_mask, bbox = _setup(dev, size, n, 23, accum_steps=2)
    watched = m.visumodel.module_list[0][0].weight
    micro, seen, order = [], [], []
    accumulate, opt_step = opt.accumulate, opt.step

    def spy_accumulate():
        micro.append(watched.grad.detach().clone())         # this call's own gradient, before the pass may turn it into the mean
        order.append("accumulate")
        accumulate()

    def spy_step():
        order.append("step")
        opt_step()

    def reducer():
        assert opt.at_boundary
        order.append("reduce")
        seen.append(watched.grad.detach().clone())

    opt.accumulate, opt.step = spy_accumulate, spy_step
    random.seed(5)
    step = GraphedTrainStep(m, opt, image, word_id, word_mask, bbox, size, reducer=reducer, warmup=1)
    assert len(seen) == 1 and step.window_position == 0
    step()
    assert len(seen) == 1 and step.window_position == 1
    step()
    assert len(seen) == 2 and len(micro) == 4
    assert order == ["accumulate", "step", "accumulate", "reduce", "step"] * 2
    half = torch.tensor(0.5, dtype=torch.float32, device=dev)
    for w in range(2):
        assert _same(seen[w], (micro[2 * w] + micro[2 * w + 1]) * half), w
        assert not _same(seen[w], micro[2 * w + 1])
    assert float(opt.state[watched]["step"]) == 2


# ---- 7. K = 1 is today's step -----------------------------------------------------------------------------------------------------------
def test_entry_points_of_a_step_without_and_with_accumulation(dev, monkeypatch):
    """accum_steps=1 (spelled out or left at its default) calls the entry points a step called before there was accumulation, in the
    same order: plain and clipped, with and without an EMA, no dcn_accum_* among them.  K = 2 for the record: prepare + pass in front,
    the gated coefficient launch in place of dcn_grad_clip_coef, the ``_clipped`` updates in both forms."""
    from dcnet_amd.lib import SIGNATURES, lib
    from dcnet_amd.optim import SGD, Adam, WeightEMA
    L = lib()
    calls = []
    for sym in SIGNATURES:
        if sym.startswith(("dcn_grad_", "dcn_sgd_", "dcn_adam_", "dcn_ema_", "dcn_tensor_", "dcn_accum_")):
            fn = getattr(L, sym[4:])
            monkeypatch.setattr(L, sym[4:], lambda *a, _fn=fn, _sym=sym: (calls.append(_sym), _fn(*a))[1])
    bag = Bag([torch.nn.Parameter(torch.ones(9, device=dev)), torch.nn.Parameter(torch.ones(1030, device=dev))])

    def step(opt):
        for p in bag.ps:
            p.grad = torch.ones_like(p)
        del calls[:]
        opt.step()
        return list(calls)

    groups = lambda: [{"params": [bag.ps[0]]}, {"params": [bag.ps[1]], "lr": 1e-3}]
    norm = ["dcn_grad_sumsq_slots", "dcn_grad_sumsq", "dcn_grad_clip_coef"]
    tail = ["dcn_ema_prepare", "dcn_ema_update"]
    for kw in ({}, {"accum_steps": 1}):
        plain = SGD(groups(), lr=1e-2, momentum=0.9, **kw)
        assert step(plain) == ["dcn_sgd_step"] * 2
        plain.attach_ema(WeightEMA(bag, 0.9, 0.0))
        assert step(plain) == ["dcn_sgd_step"] * 2 + tail
        clipped = SGD(groups(), lr=1e-2, momentum=0.9, max_grad_norm=1.0, **kw)
        assert step(clipped) == norm + ["dcn_sgd_step_clipped"] * 2
        assert step(clipped) == norm[1:] + ["dcn_sgd_step_clipped"] * 2
        clipped.attach_ema(WeightEMA(bag, 0.9, 0.0))
        assert step(clipped) == norm[1:] + ["dcn_sgd_step_clipped"] * 2 + tail
        adam = Adam(groups(), lr=1e-2, **kw)
        assert step(adam) == ["dcn_adam_prepare", "dcn_adam_step"] * 2
        adam = Adam(groups(), lr=1e-2, skip_nonfinite=True, **kw)
        assert step(adam) == norm + ["dcn_adam_prepare_clipped", "dcn_adam_step_clipped"] * 2
        assert plain.at_boundary and plain.window_position == 0
    front = ["dcn_accum_prepare", "dcn_grad_accumulate"]
    two = SGD(groups(), lr=1e-2, momentum=0.9, accum_steps=2)
    two.attach_ema(WeightEMA(bag, 0.9, 0.0))
    for _ in range(3):                                # every call of the window launches the same thing
        assert step(two) == front + ["dcn_accum_clip_coef"] + ["dcn_sgd_step_clipped"] * 2 + tail
    two = SGD(groups(), lr=1e-2, momentum=0.9, accum_steps=2, max_grad_norm=1.0)
    assert step(two) == front + ["dcn_grad_sumsq_slots", "dcn_grad_sumsq", "dcn_accum_clip_coef"] + ["dcn_sgd_step_clipped"] * 2
    for p in bag.ps:
        p.grad = torch.ones_like(p)
    del calls[:]
    two.accumulate()                                  # the data-parallel order: the pass, (the reducer,) the step — the pass runs once
    assert calls == front
    two.step()
    assert calls == front + ["dcn_grad_sumsq", "dcn_accum_clip_coef"] + ["dcn_sgd_step_clipped"] * 2
    with pytest.raises(RuntimeError, match="already called"):
        two.accumulate(); two.accumulate()


# ---- 8. the window's edges ------------------------------------------------------------------------------------------------------------
def test_live_set_change_inside_a_window_raises(dev):
    from dcnet_amd.optim import SGD
    ps = [torch.nn.Parameter(torch.ones(5, device=dev)) for _ in range(3)]
    opt = SGD(ps, lr=1e-2, momentum=0.9, accum_steps=2)
    for p in ps:
        p.grad = torch.ones_like(p)
    opt.step()
    before = [p.detach().clone() for p in ps]
    ps[1].grad = None                                 # loses its gradient inside the window
    with pytest.raises(RuntimeError, match="live set is fixed per window"):
        opt.step()
    assert opt.window_position == 1 and all(_same(p, b) for p, b in zip(ps, before))
    ps[1].grad = torch.ones(5, device=dev)
    opt.step()                                        # the window closes as if nothing had happened
    assert opt.window_position == 0 and not any(_same(p, b) for p, b in zip(ps, before))
    ps[1].grad = None                                 # between windows the set may change
    opt.step()
    ps[1].grad = torch.ones(5, device=dev)            # ... but a parameter that gains a gradient inside one is refused too
    with pytest.raises(RuntimeError, match="live set is fixed per window"):
        opt.step()
    for p in ps:                                      # a step without any gradient opens no window
        p.grad = None
    opt.reset_accumulation()
    opt.step()
    assert opt.window_position == 0


def test_first_accumulating_step_cannot_be_captured(dev, monkeypatch):
    from dcnet_amd.optim import SGD
    p = torch.nn.Parameter(torch.ones(5, device=dev))
    p.grad = torch.ones(5, device=dev)
    opt = SGD([p], lr=1e-2, momentum=0.9, accum_steps=2)
    with monkeypatch.context() as mp:                 # refused before anything is launched or allocated
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="first accumulating step cannot be a captured one"):
            opt.step()
        assert opt._accum is None and opt.window_position == 0
    opt.step()
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="not during a stream capture"):
            opt.reset_accumulation()
        with pytest.raises(RuntimeError, match="load_state_dict during a stream capture"):
            opt.load_state_dict(opt.state_dict())
    assert opt.window_position == 1


@pytest.mark.parametrize("how", ["reset_accumulation", "load_state_dict"])
@pytest.mark.parametrize("name", ["adam", "sgd"])
def test_restarted_window_equals_a_fresh_one(dev, name, how):
    """K = 3: window 1, then two calls of a window fed window 3's gradients, then reset_accumulation() / load_state_dict(state_dict()):
    the next three calls (window 2's gradients) end bit-equal to a run of windows 1 and 2 that never saw the abandoned calls, and the
    state_dict carries neither buffers nor position."""
    _, grads = _data()
    place = _aligned(dev)
    pr, orf, _, _ = _run_windows(name, 3, place, (0, 1))
    ps, opt = _fresh(name, place, accum_steps=3)
    feed = [(0, 0), (0, 1), (0, 2), (2, 0), (2, 1)]
    for w, j in feed:
        for p, gr in zip(ps, grads[w][j]):
            p.grad = place(gr)
        opt.step()
    assert opt.window_position == 2
    sd = opt.state_dict()
    assert sorted(sd) == ["param_groups", "state"] and all(sorted(v) == sorted(KEYS[name] + (("step",) if name != "sgd" else ())) for v in sd["state"].values())
    assert "accum_steps" not in sd["param_groups"][0]
    if how == "reset_accumulation":
        opt.reset_accumulation()
    else:
        opt.load_state_dict(sd)
    assert opt.window_position == 0 and not opt.at_boundary
    for j in range(3):
        for p, gr in zip(ps, grads[1][j]):
            p.grad = place(gr)
        opt.step()
    assert opt.window_position == 0
    _state_equal(name, ps, opt, pr, orf)
