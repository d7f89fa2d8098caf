"""dcnet_amd.optim.Adam / SGD (dcn_adam_prepare + dcn_adam_step, dcn_sgd_step) against torch.optim's single-tensor implementations,
and the properties the captured training step leans on: a misaligned tensor rounds like an aligned one, a parameter without a
gradient keeps its step count, a replayed step is bitwise the eager step, and a checkpoint carries Adam's device step words."""
import copy
import random

import pytest
import torch

from util import build_product, close, synth_sd

pytestmark = pytest.mark.gpu

# the shape list of test_ops_gpu.test_fused_rmsprop_matches_torch: 48 tensors = two pointer chunks; vector bodies with scalar tails;
# (1024, 257) is long enough for the grid-stride loop (65 792 float4 > 128 blocks x 256 threads)
SHAPES = [(7,), (64, 33), (3, 3, 16, 5), (1,), (1024, 257), (40, 8, 3, 3)] * 8
TOL = 2e-6          # x max(1, max|ref|): the bar of test_fused_rmsprop_matches_torch


def _pair(dev, seed):
    g = torch.Generator().manual_seed(seed)
    init = [torch.randn(*s, generator=g) for s in SHAPES]
    mk = lambda: [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    return g, mk(), mk()


def _groups(ps):
    return [{"params": ps[:20]}, {"params": ps[20:], "lr": 1e-3}]


def _steps(g, dev, pa, pb, oa, ob, first, count):
    for it in range(first, first + count):
        for x, y in zip(pa, pb):
            gr = torch.randn(x.shape, generator=g).to(dev) * (it + 1)
            x.grad = gr.clone(); y.grad = gr.clone()
        oa.step(); ob.step()


def _agree(pa, pb, oa, ob, keys):
    for x, y in zip(pa, pb):
        close(x, y, TOL, "param")
        for k in keys:
            close(oa.state[x][k], ob.state[y][k], TOL, k)


def _exchange(oa, ob):
    """each optimiser continues from the other's state_dict; torch's side stays on its single-tensor implementation"""
    sa, sb = copy.deepcopy(oa.state_dict()), copy.deepcopy(ob.state_dict())
    oa.load_state_dict(sb); ob.load_state_dict(sa)
    for grp in ob.param_groups:
        grp["foreach"] = False


def test_fused_adam_matches_torch(dev):
    """Two groups with different rates, weight decay 5e-4, 5 steps with gradients scaled by the step number: parameters, exp_avg and
    exp_avg_sq within 2e-6 x max(1, max|ref|) of torch.optim.Adam(foreach=False); the state_dicts load both ways and two more steps
    after the exchange still agree."""
    from dcnet_amd.optim import Adam
    g, pa, pb = _pair(dev, 5)
    oa = Adam(_groups(pa), lr=1e-2, weight_decay=5e-4)
    ob = torch.optim.Adam(_groups(pb), lr=1e-2, weight_decay=5e-4, foreach=False)
    _steps(g, dev, pa, pb, oa, ob, 0, 5)
    _agree(pa, pb, oa, ob, ("exp_avg", "exp_avg_sq"))
    assert all(float(oa.state[x]["step"]) == 5 for x in pa)
    _exchange(oa, ob)
    _steps(g, dev, pa, pb, oa, ob, 5, 2)
    _agree(pa, pb, oa, ob, ("exp_avg", "exp_avg_sq"))
    assert all(float(oa.state[x]["step"]) == float(ob.state[y]["step"]) == 7 for x, y in zip(pa, pb))


@pytest.mark.parametrize("wd", [0.0, 5e-4])
def test_fused_sgd_matches_torch(dev, wd):
    """momentum 0.99 with and without weight decay, 4 steps, against torch.optim.SGD(foreach=False).  The bar is Adam's: a step rounds
    three times (g + wd p, mu buf + g, p - lr buf), each by at most 2^-24 of a value no larger than the largest reference value, so
    four steps stay below 12 x 6e-8 = 7.2e-7 < 2e-6 of it."""
    from dcnet_amd.optim import SGD
    g, pa, pb = _pair(dev, 6)
    oa = SGD(_groups(pa), lr=1e-2, momentum=0.99, weight_decay=wd)
    ob = torch.optim.SGD(_groups(pb), lr=1e-2, momentum=0.99, weight_decay=wd, foreach=False)
    _steps(g, dev, pa, pb, oa, ob, 0, 4)
    _agree(pa, pb, oa, ob, ("momentum_buffer",))
    _exchange(oa, ob)
    _steps(g, dev, pa, pb, oa, ob, 4, 2)
    _agree(pa, pb, oa, ob, ("momentum_buffer",))


@pytest.mark.parametrize("clip", [None, 100.0])
@pytest.mark.parametrize("name", ["rmsprop", "adam", "adamw", "sgd"])
def test_misaligned_views_round_like_aligned_tensors(dev, name, clip):
    """The same values once in 16-byte-aligned tensors (the float4 path) and once as views one float into a flat buffer — parameter,
    gradient and state all 4-byte aligned, as gradients bound to a flat all-reduce buffer are — (the scalar path): bitwise equal
    after 3 steps, in the plain form of every update kernel and in the clipped one (``max_grad_norm`` = 100 against gradient norms of
    several hundred: every step clips)."""
    from dcnet_amd import optim
    shapes = [(7,), (64, 33), (1,), (1024, 257), (40, 8, 3, 3)]
    keys = {"rmsprop": ("square_avg",), "adam": ("exp_avg", "exp_avg_sq"), "adamw": ("exp_avg", "exp_avg_sq"), "sgd": ("momentum_buffer",)}[name]
    make = {"rmsprop": lambda q: optim.RMSprop(q, lr=1e-2, weight_decay=5e-4, max_grad_norm=clip),
            "adam": lambda q: optim.Adam(q, lr=1e-2, weight_decay=5e-4, max_grad_norm=clip),
            "adamw": lambda q: optim.AdamW(q, lr=1e-2, weight_decay=5e-4, max_grad_norm=clip),
            "sgd": lambda q: optim.SGD(q, lr=1e-2, momentum=0.99, weight_decay=5e-4, max_grad_norm=clip)}[name]
    g = torch.Generator().manual_seed(7)
    init = [torch.randn(*s, generator=g) for s in shapes]
    grads = [[torch.randn(*s, generator=g) * (it + 1) for s in shapes] for it in range(3)]

    def view_of(t):
        flat = torch.zeros(t.numel() + 5, device=dev)
        v = flat[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    def run(place):
        ps = [torch.nn.Parameter(place(t)) for t in init]
        opt = make(ps)
        for p in ps:                 # the state the first step would create, placed like the parameter
            opt.state[p] = {k: place(torch.zeros(p.shape)) for k in keys}
            if name != "sgd":
                opt.state[p]["step"] = torch.zeros((), dtype=torch.float32)
        for it in range(3):
            for p, gr in zip(ps, grads[it]):
                p.grad = place(gr)
            opt.step()
            if clip is not None:     # (the clipped kernels ran, and with a coefficient below 1)
                assert float(opt.grad_norm) > clip
        return ps, opt

    pa, oa = run(lambda t: t.clone().to(dev))
    pb, ob = run(view_of)
    assert all(p.data_ptr() % 16 == 0 for p in pa) and all(p.data_ptr() % 16 == 4 and p.grad.data_ptr() % 16 == 4 for p in pb)
    for x, y in zip(pa, pb):
        assert torch.equal(x, y), tuple(x.shape)
        for k in keys:
            assert ob.state[y][k].data_ptr() % 16 == 4
            assert torch.equal(oa.state[x][k], ob.state[y][k]), (k, tuple(x.shape))


def test_adam_parameter_without_gradient_keeps_its_step(dev):
    """A parameter whose grad is None in step 2 of 3 keeps its value in that step, its ``step`` reads 2 at the end (host counter and
    device word), and its bias correction in step 3 is that of t = 2 — compared with torch, whose 1 - 0.9^t is 0.19 against 0.271."""
    from dcnet_amd.optim import Adam
    g = torch.Generator().manual_seed(8)
    init = [torch.randn(*s, generator=g) for s in [(64, 33), (129,), (40, 8, 3, 3)]]
    pa = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    pb = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    oa = Adam(pa, lr=1e-2, weight_decay=5e-4)
    ob = torch.optim.Adam(pb, lr=1e-2, weight_decay=5e-4, foreach=False)
    for it in range(3):
        before = pa[1].detach().clone()
        for i, (x, y) in enumerate(zip(pa, pb)):
            gr = torch.randn(x.shape, generator=g).to(dev)
            x.grad, y.grad = (None, None) if (it == 1 and i == 1) else (gr.clone(), gr.clone())
        oa.step(); ob.step()
        if it == 1:
            assert torch.equal(pa[1], before)
    assert [float(oa.state[x]["step"]) for x in pa] == [3, 2, 3] == [float(ob.state[y]["step"]) for y in pb]
    assert oa._tables[0]["steps"].tolist() == [3, 2, 3]
    for x, y in zip(pa, pb):
        close(x, y, TOL, "param")
        close(oa.state[x]["exp_avg"], ob.state[y]["exp_avg"], TOL, "exp_avg")
        close(oa.state[x]["exp_avg_sq"], ob.state[y]["exp_avg_sq"], TOL, "exp_avg_sq")


# ---- the training step ------------------------------------------------------------------------------------------------------
def _setup(dev, size, n, seed, name):
    from dcnet_amd.parallel import freeze_gradless
    from dcnet_amd.train import make_optimizer
    from dcnet_amd.utils.synth import synth_boxes, synth_inputs
    m = build_product(size, synth_sd(size), dev)
    freeze_gradless(m)
    opt = make_optimizer(m, 1e-4, name)
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
    for o in (o1, o2):               # Adam: the device step words are where the host counters are
        for gi, tab in getattr(o, "_tables", {}).items():
            assert tab["steps"].tolist() == [int(o.state[p]["step"]) if p in o.state else 0 for p in o.param_groups[gi]["params"]]


@pytest.mark.parametrize("name", ["adam", "sgd"])
def test_replayed_steps_equal_eager_steps_bitwise(dev, name):
    """The scenario of test_graph_gpu.test_replayed_steps_equal_eager_steps_bitwise with the fused Adam / SGD: five steps under a
    changing learning rate, once with train_step and once as one eager warm-up step + the captured pass + three replays — identical
    losses, parameters, running statistics, every optimiser state tensor and every ``step``."""
    from dcnet_amd.graph import GraphedTrainStep
    from dcnet_amd.train import adjust_learning_rate, train_step
    size, n, steps = 256, 4, 5
    lr_of = lambda it: 1e-4 if it < 2 else 1e-4 * (1 - it / 10.0)     # the constructor's two steps run at the initial rate
    m1, o1, image, word_id, word_mask, bbox = _setup(dev, size, n, 21, name)
    random.seed(99)
    ref_losses = []
    for it in range(steps):
        adjust_learning_rate(o1, 0, lr_of(it), 1, 0.9)
        loss, _ = train_step(m1, o1, image, word_id, word_mask, bbox, size)
        ref_losses.append(float(loss))

    m2, o2, image, word_id, word_mask, bbox = _setup(dev, size, n, 21, name)
    random.seed(99)
    step = GraphedTrainStep(m2, o2, image, word_id, word_mask, bbox, size, warmup=1)      # steps 0 (eager) and 1 (captured pass)
    got = [None, float(step.loss)]
    for it in range(2, steps):
        adjust_learning_rate(o2, 0, lr_of(it), 1, 0.9)
        got.append(float(step()))
    assert got[1:] == ref_losses[1:], (got, ref_losses)
    _same_training_state(m1, o1, m2, o2, steps)


@pytest.mark.parametrize("name", ["adam", "sgd"])
def test_resumed_run_equals_uninterrupted_run_bitwise(dev, tmp_path, name):
    """3 steps, save_checkpoint, a fresh model and optimiser, load_checkpoint, 2 more steps: bitwise the 5 uninterrupted steps — the
    checkpoint's ``step`` counters reach Adam's device step words."""
    from dcnet_amd.train import load_checkpoint, save_checkpoint, train_step
    size, n = 256, 2
    m1, o1, image, word_id, word_mask, bbox = _setup(dev, size, n, 22, name)
    random.seed(7)
    ref_losses = [float(train_step(m1, o1, image, word_id, word_mask, bbox, size)[0]) for _ in range(5)]

    m2, o2, *_ = _setup(dev, size, n, 22, name)
    random.seed(7)
    got = [float(train_step(m2, o2, image, word_id, word_mask, bbox, size)[0]) for _ in range(3)]
    path = save_checkpoint({"epoch": 3, "state_dict": m2.state_dict(), "best_loss": 1.0, "optimizer": o2.state_dict()}, False, "resume", str(tmp_path))
    draws = random.getstate()
    m3, o3, *_ = _setup(dev, size, n, 23, name)
    assert load_checkpoint(m3, path, o3) == (3, 1.0)
    random.setstate(draws)
    got += [float(train_step(m3, o3, image, word_id, word_mask, bbox, size)[0]) for _ in range(2)]
    assert got == ref_losses, (got, ref_losses)
    _same_training_state(m1, o1, m3, o3, 5)
