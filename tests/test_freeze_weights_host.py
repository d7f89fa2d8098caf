"""CPU: partial fine-tuning's bookkeeping.  darknet.backward_needs — which weight gradients, BatchNorm sums and data gradients a backward
launches and which layers keep a record, as a pure function of the plan and the trainable (slot, key) pairs — against a brute-force
reachability walk on the real yolov3 plan; grounding_model.freeze_weights (scopes, undo, the other switches that turn requires_grad
off); the driver's --freeze-weights flag.  What the reduced backward computes is tests/test_freeze_weights_gpu.py."""
import os

import pytest
import torch

from util import ROOT, new_product

_BN = torch.nn.modules.batchnorm._BatchNorm


def _plan():
    from dcnet_amd import darknet as D
    defs = D.parse_model_config(os.path.join(ROOT, "model", "yolov3.cfg"))
    plan, taps, _ = D.build_plan(defs[1:], 3)
    return D, plan, taps


def _brute(D, plan, trainable):
    """For every tensor: the conv slots among its producer and all of the producer's ancestors (a walk per tensor, no shared state).  Its
    gradient is needed iff one of them has a trainable parameter."""
    producer = {op.dst: op for op in plan}
    inputs = lambda op: [s for s in ((op.src, op.res) if isinstance(op, D._ConvOp) else (op.up_src, op.lat_src) if isinstance(op, D._UpCatOp)
                                     else (op.src,)) if s is not None]

    def convs_at_or_above(t):
        seen, found, stack = set(), set(), [t]
        while stack:
            s = stack.pop()
            if s in seen or s < 0:
                continue
            seen.add(s)
            op = producer[s]
            if isinstance(op, D._ConvOp):
                found.add(op.slot)
            stack += inputs(op)
        return found

    has = {op.slot: any((op.slot, k) in trainable for k in ("w", "gamma", "beta", "b")) for op in plan if isinstance(op, D._ConvOp)}
    need = lambda t: any(has[s] for s in convs_at_or_above(t))
    conv = {}
    for op in plan:
        if isinstance(op, D._ConvOp):
            want_dx = need(op.src)
            conv[op.slot] = dict(want_w=(op.slot, "w") in trainable,
                                 want_affine=any((op.slot, k) in trainable for k in ("gamma", "beta", "b")),
                                 want_dx=want_dx, want_res=op.res is not None and need(op.res), live=has[op.slot] or want_dx)
    tensor = {op.dst: need(op.dst) for op in plan}
    return conv, tensor


def _cases(D, plan):
    every = D.all_trainable(plan)
    yield "nothing frozen", every
    yield "everything frozen", frozenset()
    for k in (0, 4, 36, 61, 74):
        yield f"prefix {k}", frozenset(x for x in every if x[0] > k)
    yield "neck frozen", frozenset(x for x in every if x[0] < 75)
    yield "weights frozen, gamma and beta trainable", frozenset(x for x in every if x[1] != "w")
    yield "one residual block frozen", frozenset(x for x in every if x[0] not in (41, 42))


def test_backward_needs_equals_a_reachability_walk():
    D, plan, taps = _plan()
    convs = [op for op in plan if isinstance(op, D._ConvOp)]
    ups = [op for op in plan if isinstance(op, D._UpCatOp)]
    assert len(convs) == 68 and taps == [78, 90, 102]
    assert [(u.dst, u.lat_src) for u in ups] == [(86, 61), (98, 36)]
    assert any(op.slot == 42 and op.res is not None for op in convs) and any(op.slot == 41 for op in convs)      # (the block the last case freezes)
    for name, trainable in _cases(D, plan):
        got = D.backward_needs(plan, trainable)
        conv, tensor = _brute(D, plan, trainable)
        assert set(got.conv) == set(conv), name
        for slot, want in conv.items():
            assert got.conv[slot]._asdict() == want, (name, slot, got.conv[slot], want)
        for t, want in tensor.items():
            assert got.tensor[t] == want, (name, t)
        assert got.tensor[-1] is False
        assert got.live == frozenset(s for s, c in conv.items() if c["live"]), name
    # nothing frozen: the schedule there always was — every layer live, every gradient wanted, no data gradient for the stem alone
    full = D.backward_needs(plan, D.all_trainable(plan))
    assert len(full.live) == 68 and all(c.want_w and c.want_affine for c in full.conv.values())
    assert [s for s, c in full.conv.items() if not c.want_dx] == [0]
    assert all(c.want_res == (op.res is not None) for op in convs for c in [full.conv[op.slot]])
    # everything frozen: nothing at all
    none = D.backward_needs(plan, frozenset())
    assert not none.live and not any(none.tensor.values()) and not any(any(c) for c in none.conv.values())
    # the stem frozen, slot 1 trainable: slot 1 is live (it reads the dead stem's output for its weight gradient) and wants no data gradient
    k0 = D.backward_needs(plan, frozenset(x for x in D.all_trainable(plan) if x[0] > 0))
    assert 0 not in k0.live and k0.conv[1].live and k0.conv[1].want_w and not k0.conv[1].want_dx


def test_backward_needs_worked_example_prefix_74():
    """freeze_weights(74): the neck trains.  16 live convs, all 16 want their weight gradient, 15 their data gradient (all but module 75,
    whose input is the frozen extractor's output), and neither lateral (61, 36) gets a gradient."""
    D, plan, _ = _plan()
    nd = D.backward_needs(plan, frozenset(x for x in D.all_trainable(plan) if x[0] > 74))
    assert len(nd.live) == 16 and min(nd.live) == 75
    assert sum(nd.conv[s].want_w for s in nd.live) == 16
    assert sorted(s for s in nd.live if not nd.conv[s].want_dx) == [75]
    assert nd.tensor[61] is False and nd.tensor[36] is False and nd.tensor[74] is False
    assert not any(c.want_w or c.want_dx or c.want_affine or c.want_res for s, c in nd.conv.items() if s <= 74)


def _off(m):
    return {n for n, p in m.named_parameters() if not p.requires_grad}


def test_freeze_weights_bookkeeping():
    from dcnet_amd.parallel import freeze_gradless
    m = new_product(256)
    names = [n for n, _ in m.named_parameters()]
    keys = list(m.state_dict().keys())
    assert not _off(m)
    assert m.freeze_weights("backbone") is m
    backbone = {n for n in names if n.startswith("visumodel.")}
    assert _off(m) == backbone and len(backbone) > 200
    assert all(x.training for x in m.modules() if isinstance(x, _BN))          # how BatchNorm normalises is not touched
    m.train(); m.eval(); m.train()
    assert _off(m) == backbone
    # an int: module_list[0..k]; a second call replaces the first
    m.freeze_weights(74)
    upto74 = {n for n in backbone if int(n.split(".")[2]) <= 74}
    assert _off(m) == upto74 and 0 < len(upto74) < len(backbone)
    assert m.visumodel.backward_needs().live == frozenset(op.slot for op in m.visumodel._conv_ops if op.slot > 74)
    m.freeze_weights(0)
    assert _off(m) == {n for n in backbone if n.split(".")[2] == "0"} and len(_off(m)) == 3
    # prefixes: whole components of a name
    m.freeze_weights(["visumodel", "textmodel"])
    assert _off(m) == {n for n in names if n.startswith(("visumodel.", "textmodel."))}
    m.freeze_weights(("mapping_visu.0",))
    assert _off(m) == {n for n in names if n.startswith("mapping_visu.0.")} and len(_off(m)) == 3
    m.freeze_weights(x for x in ["visumodel.module_list.1"])
    assert _off(m) == {n for n in names if n.startswith("visumodel.module_list.1.")}          # (not module_list.10 ...)
    m.freeze_weights(None)
    assert not _off(m)
    assert m.visumodel.backward_needs().live == frozenset(op.slot for op in m.visumodel._conv_ops)
    # undo gives back exactly what the call switched off: not freeze_gradless's, not the caller's
    gradless = set(freeze_gradless(m))
    m.sub_attn.fc.bias.requires_grad_(False)
    mine = gradless | {"sub_attn.fc.bias"}
    m.freeze_weights(["visumodel", "sub_attn"])
    assert _off(m) == mine | backbone | {"sub_attn.fc.weight"}
    m.freeze_weights(None)
    assert _off(m) == mine
    # ... nor freeze_batchnorm(train_affine=False)'s, in either order of the calls and of the undos
    affine = {n for n in backbone if "batch_norm" in n}
    m.freeze_batchnorm("backbone", train_affine=False)
    assert _off(m) == mine | affine
    m.freeze_weights("backbone")
    assert _off(m) == mine | backbone
    m.freeze_weights(None)
    assert _off(m) == mine | affine
    m.freeze_weights("backbone")
    m.freeze_batchnorm(None)                                 # gamma and beta stay with freeze_weights
    assert _off(m) == mine | backbone
    m.freeze_batchnorm("backbone", train_affine=False)       # (they were off already: held by both now)
    m.freeze_weights(None)
    assert _off(m) == mine | affine
    m.freeze_batchnorm(None)
    assert _off(m) == mine
    m.freeze_weights(74)
    m.freeze_batchnorm("backbone", train_affine=False)
    m.freeze_batchnorm("backbone", train_affine=True)
    assert _off(m) == mine | upto74
    m.freeze_batchnorm(None); m.freeze_weights(None)
    assert _off(m) == mine
    assert list(m.state_dict().keys()) == keys
    for bad in ("head", "all", "", True, -1, 107, 3.5, [], ["nosuchmodule"], ["visumodel", 3], ["visu"]):
        with pytest.raises(ValueError):
            m.freeze_weights(bad)
    assert _off(m) == mine                                   # a refused call changes nothing
    assert "freeze_batchnorm" in m.freeze_weights.__doc__ and "running statistics" in m.freeze_weights.__doc__


def test_freeze_weights_argument_parses():
    from dcnet_amd.train import arg_parser
    ap = arg_parser()
    assert ap.parse_args([]).freeze_weights is None
    assert ap.parse_args(["--freeze-weights", "none"]).freeze_weights is None
    assert ap.parse_args(["--freeze-weights", "backbone"]).freeze_weights == "backbone"
    assert ap.parse_args(["--freeze-weights", "74"]).freeze_weights == 74
    a = ap.parse_args(["--freeze-weights", "74", "--freeze-bn", "backbone", "--accum-steps", "2", "--ema-decay", "0.99", "--clip-grad-norm", "1"])
    assert (a.freeze_weights, a.freeze_bn, a.accum_steps, a.ema_decay, a.clip_grad_norm) == (74, "backbone", 2, 0.99, 1.0)
    for bad in ("head", "-1", "7.5"):
        with pytest.raises(SystemExit):
            ap.parse_args(["--freeze-weights", bad])
