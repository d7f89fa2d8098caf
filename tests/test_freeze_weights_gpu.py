"""Partial fine-tuning on the device (grounding_model.freeze_weights, darknet.backward_needs): requires_grad decides the work.

1. work removed: the C entry points a backward calls, recorded on lib(), frozen against all-trainable — exactly the calls backward_needs
   says are not wanted disappear, matched by their geometry integers; 2. nothing else moves: forward and the remaining gradients bitwise;
3. storage: the slots that keep a record are backward_needs().live; 4. the whole model, eager and replayed; 5. the head's blocks;
6. the language branch; 7. the reducer's sink; 8. fp8 storage trains around a frozen backbone.  The host half is tests/test_freeze_weights_host.py.

The Darknet module alone runs at 2 x 128^2 (every layer, both concats, the fused stem backward's minimum width of 32), the model at
2 x 256^2."""
import random
from collections import Counter

import pytest
import torch

from util import build_product, rand as _rand, synth_sd

pytestmark = pytest.mark.gpu

N, HW = 2, 128
CUTS = [("prefix", 0), ("prefix", 4), ("prefix", 36), ("prefix", 74), ("neck", None)]
_CACHE = {}


def _sd(size=256):
    if ("sd", size) not in _CACHE:
        _CACHE[("sd", size)] = synth_sd(size)
    return _CACHE[("sd", size)]


def _darknet(dev):
    """One backbone for the whole file: every run starts from the same state dict (train-mode runs move the running statistics)."""
    if "net" not in _CACHE:
        import os
        from dcnet_amd.darknet import Darknet
        from util import ROOT
        net = Darknet(config_path=os.path.join(ROOT, "model", "yolov3.cfg"), img_size=HW)
        sd = {k[len("visumodel."):]: v for k, v in _sd().items() if k.startswith("visumodel.")}
        net.load_state_dict(sd, strict=True)
        _CACHE["net"], _CACHE["net_sd"] = net.to(dev), {k: v.to(dev) for k, v in sd.items()}
        _CACHE["img"] = _rand(N, 3, HW, HW, seed=1).to(dev)
    return _CACHE["net"]


def _frozen_index(cut):
    kind, k = cut
    return (lambda i: i <= k) if kind == "prefix" else (lambda i: i >= 75) if kind == "neck" else (lambda i: True) if kind == "all" else (lambda i: False)


def _set_frozen(net, cut):
    frozen = _frozen_index(cut)
    for name, p in net.named_parameters():
        p.requires_grad_(not frozen(int(name.split(".")[1])))


def _dark_run(dev, cut, mode="fp32", bn_frozen=False, sink=None):
    """Forward + backward of the Darknet module alone, the three taps summed into a scalar with fixed random weights.  Returns taps,
    gradients by name, the saved slots and backward_needs of the run."""
    from dcnet_amd import ops
    net = _darknet(dev)
    net.load_state_dict(_CACHE["net_sd"])
    net.freeze_batchnorm(bn_frozen)
    net.train()
    _set_frozen(net, cut)
    for p in net.parameters():
        p.grad = None
    if sink is not None:
        net.__dict__["_grad_reducer"] = sink
    ops.set_precision(mode)
    try:
        if ops.use_amax():
            ops.amax_begin_step(dev)
        taps = net.forward_nhwc(_CACHE["img"])
        saved = net.saved_slots
        if "gouts" not in _CACHE:
            _CACHE["gouts"] = [_rand(*t.shape, seed=10 + i).to(dev) / t[0].numel() ** 0.5 for i, t in enumerate(taps)]
        needs_grad = [t.requires_grad for t in taps]
        if any(needs_grad):
            sum((t * g).sum() for t, g in zip(taps, _CACHE["gouts"])).backward()
        torch.cuda.synchronize()
    finally:
        ops.set_precision("fp32")
        net.__dict__.pop("_grad_reducer", None)
        net.freeze_batchnorm(False)
    in_plan = {id(p) for p in net._slot_params().values()}          # (the dead YOLO heads' parameters never get a gradient)
    r = dict(taps=[t.detach().clone() for t in taps], needs_grad=needs_grad, saved=saved, needs=net.backward_needs(),
             grads={k: (None if p.grad is None else p.grad.detach().clone()) for k, p in net.named_parameters() if id(p) in in_plan},
             dead_grads=[p.grad for p in net.parameters() if id(p) not in in_plan], trainable=net.trainable_keys())
    _set_frozen(net, ("none", None))
    return r


# ---- recording the C entry points ---------------------------------------------------------------------------------------------------------
def _family(sym):
    if sym.endswith("_supported") or "_ws" in sym or sym.endswith("_rows") or "_rows_" in sym:
        return None          # (queries: no launch)
    if sym.startswith(("dcn_conv2d_bwd_weight", "dcn_stem_bwd_weight_bn")):
        return "w"
    if sym.startswith("dcn_conv2d_bwd_data"):
        return "dx"
    if sym.startswith(("dcn_bn_act_bwd_", "dcn_frozen_bn_act_bwd")):
        return "bn"
    return None


def _record(monkeypatch, pick):
    """Wrap every entry point ``pick(sym)`` accepts on lib(): calls = [(sym, the integer arguments it takes, in order)]."""
    from dcnet_amd.lib import I, L as L64, SIGNATURES, lib
    L = lib()
    calls = []
    for sym, (_, types) in SIGNATURES.items():
        if not pick(sym):
            continue
        fn = getattr(L, sym[4:])
        at = [i for i, t in enumerate(types) if t is I or t is L64]

        def wrapped(*a, _fn=fn, _sym=sym, _at=at):
            calls.append((_sym, tuple(int(a[i]) for i in _at)))
            return _fn(*a)
        monkeypatch.setattr(L, sym[4:], wrapped)
    return calls


def _geometries(net):
    """{slot: (N, H_in, W_in, Cin as the kernels see it, Cout, k, stride)} and {slot: (rows, Cout) of the BatchNorm backward}."""
    from dcnet_amd import darknet as D
    from dcnet_amd import ops
    hw = {-1: (HW, HW)}
    conv, bn = {}, {}
    for op in net._plan:
        if isinstance(op, D._ConvOp):
            h, w = hw[op.src]
            ho, wo = ops.conv_out_hw(h, w, op.k, op.stride)
            conv[op.slot] = (N, h, w, D._cpad(op.cin), op.cout, op.k, op.stride)
            bn[op.slot] = (N * ho * wo, op.cout)
            hw[op.dst] = (ho, wo)
        elif isinstance(op, D._UpCatOp):
            hw[op.dst] = hw[op.lat_src]
        else:
            hw[op.dst] = hw[op.src]
    return conv, bn


def _window(ints, known, width):
    """the last run of ``width`` consecutive integer arguments that is one of the plan's geometries"""
    for i in range(len(ints) - width, -1, -1):
        if ints[i:i + width] in known:
            return ints[i:i + width]
    raise AssertionError(f"no known geometry among {ints}")


def _conv_geoms(calls, fam, conv_g):
    known = set(conv_g.values())
    out = []
    for sym, ints in calls:
        if _family(sym) != fam:
            continue
        out.append(conv_g[0] if sym.startswith("dcn_stem_bwd_weight_bn") else _window(ints, known, 7))       # (only the stem takes its fused kernel)
    return out


def test_frozen_layers_launch_no_backward_work(dev, monkeypatch):
    """1. Work removed.  Against the all-trainable run, per family — weight gradients, data gradients, BatchNorm backward passes — the
    calls that disappear are exactly those of the layers backward_needs says do not want them, by geometry; none appears.  The BatchNorm
    passes are attributed layer by layer (the sweep visits the layers in reverse plan order, one apply-type call each, its reduce in
    front of it where the data gradient above did not form the sums), so for them the whole remaining sequence is compared.  With
    everything frozen no backward entry point is called at all and the taps do not require grad."""
    net = _darknet(dev)
    conv_g, bn_g = _geometries(net)
    calls = _record(monkeypatch, lambda s: "_bwd" in s)
    full = _dark_run(dev, ("none", None))
    full_calls = list(calls)
    F = full["needs"]
    assert len(F.live) == 68 and full["saved"] == F.live
    order = [op.slot for op in reversed(net._conv_ops)]
    assert sorted(_conv_geoms(full_calls, "w", conv_g)) == sorted(conv_g.values())                  # one weight gradient per layer
    assert sorted(_conv_geoms(full_calls, "dx", conv_g)) == sorted(g for s, g in conv_g.items() if s != 0)

    def bn_by_slot(cs, slots):
        """the BatchNorm family's calls split per layer: [reduce] + apply, in sweep order"""
        seq = [(sym, _window(ints, set(bn_g.values()), 2)) for sym, ints in cs if _family(sym) == "bn"]
        per, i = {}, 0
        for s in slots:
            take = []
            if i < len(seq) and "reduce" in seq[i][0]:
                take.append(seq[i]); i += 1
            if s == 0 and stem_fused:          # (the fused stem kernel is the apply pass: it is counted with the weight gradients)
                assert all(t[1] == bn_g[s] for t in take), (s, take)
                per[s] = take
                continue
            assert i < len(seq) and "reduce" not in seq[i][0] and seq[i][1] == bn_g[s], (s, seq[i] if i < len(seq) else None)
            take.append(seq[i]); i += 1
            assert all(t[1] == bn_g[s] for t in take), (s, take)
            per[s] = take
        assert i == len(seq), (i, len(seq))
        return per

    stem_fused = any(sym.startswith("dcn_stem_bwd_weight_bn") for sym, _ in full_calls)
    full_bn = bn_by_slot(full_calls, order)
    for cut in CUTS:
        del calls[:]
        r = _dark_run(dev, cut)
        Z = r["needs"]
        got = list(calls)
        assert 0 < len(Z.live) <= 68 and r["saved"] == Z.live, cut
        for fam, want in (("w", "want_w"), ("dx", "want_dx")):
            a, b = Counter(_conv_geoms(full_calls, fam, conv_g)), Counter(_conv_geoms(got, fam, conv_g))
            assert not (b - a), (cut, fam, "a call appeared", b - a)
            gone = Counter(conv_g[s] for s in order if getattr(F.conv[s], want) and not getattr(Z.conv[s], want))
            assert a - b == gone, (cut, fam, (a - b) - gone, gone - (a - b))
            assert sum(gone.values()) > 0 or (fam == "dx" and cut[0] == "neck"), (cut, fam)      # (a frozen neck: every data gradient stays)
        seq = [(sym, _window(ints, set(bn_g.values()), 2)) for sym, ints in got if _family(sym) == "bn"]
        assert seq == [c for s in order if s in Z.live for c in full_bn[s]], (cut, "BatchNorm backward passes")
        # everything else the backward calls (upsample, copies are not C entry points with _bwd in their name; dcn_act_bwd is not used here)
        other = lambda cs: Counter(sym for sym, _ in cs if _family(sym) is None and not sym.endswith(("_supported", "_rows", "_ws")) and "_ws_" not in sym
                                   and "_rows_" not in sym)
        assert not (other(got) - other(full_calls)), cut
    del calls[:]
    r = _dark_run(dev, ("all", None))
    assert [c for c in calls if _family(c[0]) is not None or "_bwd" in c[0]] == []
    assert r["needs_grad"] == [False, False, False] and r["saved"] == frozenset() and not r["needs"].live
    assert all(g is None for g in r["grads"].values())
    for a, b in zip(full["taps"], r["taps"]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("mode", ["fp32", "bf16s"])
@pytest.mark.parametrize("bn_frozen", [False, True], ids=["batch_stats", "running_stats"])
def test_nothing_else_moves_and_dead_layers_keep_nothing(dev, mode, bn_frozen):
    """2. and 3.  For every cut: the taps are the bits of the all-trainable run, so is the gradient of every parameter that stays trainable,
    a frozen parameter's .grad is None, and the slots that kept a record after the train-mode forward are backward_needs().live."""
    full = _dark_run(dev, ("none", None), mode, bn_frozen)
    assert full["saved"] == full["needs"].live and len(full["saved"]) == 68
    assert len(full["grads"]) == 68 * 3 and all(g is None for g in full["dead_grads"])
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in full["grads"].values())
    assert sum(float(g.abs().max()) > 0 for g in full["grads"].values()) > 68 * 3 // 2          # (the comparison below is not one of zeros)
    for cut in CUTS:
        r = _dark_run(dev, cut, mode, bn_frozen)
        frozen = _frozen_index(cut)
        for i, (a, b) in enumerate(zip(full["taps"], r["taps"])):
            assert torch.equal(a, b), (cut, "tap", i)
        assert r["saved"] == r["needs"].live, cut
        assert r["saved"] == frozenset(s for s in full["saved"] if not frozen(s) or any(not frozen(t) for t in range(s))), cut
        n_live = 0
        for k, g in r["grads"].items():
            if frozen(int(k.split(".")[1])):
                assert g is None, (cut, k)
            else:
                assert g is not None and torch.equal(g, full["grads"][k]), (cut, k)
                n_live += 1
        assert n_live > 0
        if cut == ("prefix", 0):
            # the stem frozen, slot 1 trainable: slot 1 kept the dead stem's output in the form its weight gradient reads (the bits above)
            assert 0 not in r["saved"] and 1 in r["saved"] and r["grads"]["module_list.1.conv_1.weight"] is not None


def test_reducer_sink_receives_exactly_the_trainable_gradients(dev):
    """7. A recording sink on the Darknet alone, modules 0..74 frozen: every trainable (slot, key) once, nothing else, in the order the
    all-trainable sweep hands over those that remain."""
    net = _darknet(dev)
    pmap = {id(p): k for k, p in net._slot_params().items()}

    class Sink:
        bucket_bytes = 1 << 16

        def __init__(self):
            self.seen = []

        def push(self, items):
            self.seen += [pmap[id(p)] for p, _ in items]

        def join_backward(self):
            pass

    a, b = Sink(), Sink()
    _dark_run(dev, ("none", None), sink=a)
    r = _dark_run(dev, ("prefix", 74), sink=b)
    assert len(a.seen) == len(set(a.seen)) == 68 * 3
    keep = r["trainable"]
    assert len(keep) == 16 * 3 and set(b.seen) == keep and len(b.seen) == len(keep)
    assert b.seen == [x for x in a.seen if x in keep]


# ---- the whole model ------------------------------------------------------------------------------------------------------------------------
SIZE = 256


def _setup(dev, n, seed, scope=None, bn=None, **opt_kw):
    from dcnet_amd.parallel import freeze_gradless
    from dcnet_amd.train import make_optimizer
    from dcnet_amd.utils.synth import synth_boxes, synth_inputs
    m = build_product(SIZE, _sd(), dev)
    freeze_gradless(m)
    if bn is not None:
        m.freeze_batchnorm(bn)
    if scope is not None:
        m.freeze_weights(scope)
    opt = make_optimizer(m, 1e-4, **opt_kw)
    image, word_id, word_mask = (t.to(dev) for t in synth_inputs(n, SIZE, seed=seed))
    return m, opt, image, word_id, word_mask, synth_boxes(n, SIZE, seed=seed).to(dev)


def test_frozen_backbone_two_eager_steps(dev):
    """4a. freeze_weights("backbone"), fused RMSprop with weight decay, two eager steps: the frozen parameters keep their bits (no
    gradient, no decay), the first loss is bitwise the unfrozen model's, the backbone kept nothing."""
    from dcnet_amd.train import train_step
    losses_ = {}
    for scope in (None, "backbone"):
        m, opt, image, word_id, word_mask, bbox = _setup(dev, N, 21, scope)
        assert opt.param_groups[0]["weight_decay"] > 0
        before = {k: v.detach().clone() for k, v in m.named_parameters()}
        random.seed(99)
        losses_[scope] = [float(train_step(m, opt, image, word_id, word_mask, bbox, SIZE)[0]) for _ in range(2)]
        if scope is not None:
            assert m.visumodel.saved_slots == frozenset()
            moved = 0
            for k, p in m.named_parameters():
                if k.startswith("visumodel."):
                    assert p.grad is None and torch.equal(p.detach(), before[k]), k
                elif p.requires_grad:
                    moved += int(not torch.equal(p.detach(), before[k]))
            assert sum(p.requires_grad for p in m.parameters()) == 91 and moved > 91 // 2          # (the rest does train)
        else:
            assert len(m.visumodel.saved_slots) == 68
    assert losses_["backbone"][0] == losses_[None][0], losses_
    assert all(map(lambda x: x == x, losses_["backbone"]))


@pytest.mark.parametrize("accum", [1, 2])
def test_frozen_backbone_replayed_steps_equal_eager_steps_bitwise(dev, accum):
    """4b. test_graph_gpu.test_replayed_steps_equal_eager_steps_bitwise with the backbone frozen (and once with accum_steps=2): an eager
    warm-up, the captured pass and three replays under a changing learning rate against five eager steps — losses, state dict, optimiser
    state.  Changing the frozen set after the capture raises."""
    from dcnet_amd.graph import GraphedTrainStep
    from dcnet_amd.train import adjust_learning_rate, train_step
    steps = 5
    lr_of = lambda it: 1e-4 if it < 2 else 1e-4 * (1 - it / 10.0)
    m1, o1, image, word_id, word_mask, bbox = _setup(dev, N, 21, "backbone", accum_steps=accum)
    random.seed(99)
    ref = []
    for it in range(steps):
        adjust_learning_rate(o1, 0, lr_of(it), 1, 0.9)
        ref.append(float(train_step(m1, o1, image, word_id, word_mask, bbox, SIZE)[0]))
    m2, o2, image, word_id, word_mask, bbox = _setup(dev, N, 21, "backbone", accum_steps=accum)
    random.seed(99)
    step = GraphedTrainStep(m2, o2, image, word_id, word_mask, bbox, SIZE, warmup=1)
    got = [None, float(step.loss)]
    for it in range(2, steps):
        adjust_learning_rate(o2, 0, lr_of(it), 1, 0.9)
        got.append(float(step()))
    assert got[1:] == ref[1:], (got, ref)
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    for k in sd1:
        assert torch.equal(sd1[k], sd2[k]), k
    s1, s2 = o1.state_dict()["state"], o2.state_dict()["state"]
    assert s1.keys() == s2.keys() and len(s1) == 91          # (one state per parameter that trains: none for the backbone)
    for k in s1:
        assert torch.equal(s1[k]["square_avg"], s2[k]["square_avg"]), k
    assert all(p.grad is None for p in m2.visumodel.parameters())
    m2.freeze_weights(74)
    with pytest.raises(RuntimeError, match="trainable parameters changed after the capture"):
        step()
    m2.freeze_weights("backbone")
    step()
    torch.cuda.synchronize()


def _model_run(dev, scope, staged=False):
    """One training forward + five losses + backward of the model (p_dropout = 0) with ``scope`` frozen.  Returns loss and gradients."""
    from dcnet_amd import losses, ops
    m, _, image, word_id, word_mask, bbox = _setup(dev, N, 33, scope)
    m.train()
    random.seed(7)
    was = ops.WGRAD_DIRECT
    m.defer_language_backward = staged
    ops.WGRAD_DIRECT = staged
    try:
        loss, _ = losses.total_loss(m(image, word_id, word_mask), bbox, SIZE)
        loss.backward()
        if staged:
            m.finish_backward()
            ops.finish_wgrads(dev)
    finally:
        ops.WGRAD_DIRECT = was
        m.defer_language_backward = False
    torch.cuda.synchronize()
    return m, float(loss.detach()), {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()}


def _same_but(full, part, frozen):
    n = 0
    for k, g in part.items():
        if frozen(k):
            assert g is None, k
        else:
            assert (g is None) == (full[k] is None), k
            if g is not None:
                assert torch.equal(g, full[k]), k
                n += 1
    return n


def test_frozen_head_weights_launch_no_weight_gradient(dev, monkeypatch):
    """5. mapping_visu's three convolution weights frozen, nothing else: their weight-gradient calls are gone (by geometry: 1x1,
    1024 / 512 / 256 -> 512 on the three grids), every data gradient is still there — the backbone's among them —, and every other
    gradient keeps its bits.  Plain and with the staged backward a captured step uses (ops.WGRAD_DIRECT: the blocks hold their gradients)."""
    calls = _record(monkeypatch, lambda s: _family(s) in ("w", "dx"))
    names = [f"mapping_visu.{s}.conv.weight" for s in range(3)]
    fam = lambda f: Counter(c for c in calls if _family(c[0]) == f)
    for staged in (False, True):
        del calls[:]
        _, l0, g0 = _model_run(dev, None, staged)
        w0, dx0 = fam("w"), fam("dx")
        del calls[:]
        _, l1, g1 = _model_run(dev, names, staged)
        w1, dx1 = fam("w"), fam("dx")
        assert l0 == l1
        assert dx1 == dx0 and sum(dx0.values()) > 67
        gone = w0 - w1
        assert not (w1 - w0) and sum(gone.values()) == 3, gone
        g = SIZE // 32
        want = [(N, g, g, 1024, 512, 1, 1), (N, 2 * g, 2 * g, 512, 512, 1, 1), (N, 4 * g, 4 * g, 256, 512, 1, 1)]      # n, h, w, cin, cout, k, stride
        assert sorted(_window(ints, set(want), 7) for _, ints in gone.elements()) == sorted(want), gone
        assert _same_but(g0, g1, lambda k: k in names) > 200


def test_frozen_language_branch_has_no_backward(dev, monkeypatch):
    """6. textmodel frozen: no BiLSTM, embedding or MLP backward entry point is called — eager, with the language backward staged
    (model.finish_backward), and while a GraphedTrainStep warms up and captures — and the remaining gradients keep their bits.  The MLP's
    and the BiLSTM's products are the only ones over N x L = 40 rows: GEMMs with a 40 among their integers."""
    from dcnet_amd.graph import GraphedTrainStep
    lang = ("dcn_bilstm_bwd", "dcn_lstm_cell_bwd", "dcn_embedding_bwd")
    calls = _record(monkeypatch, lambda s: s in lang or s in ("dcn_gemm_tn", "dcn_gemm_nn", "dcn_act_bwd", "dcn_colsum"))
    rows = N * 20
    branch = lambda: [c for c in calls if c[0] in lang or (c[0].startswith("dcn_gemm_") and rows in c[1])]
    for staged in (False, True):
        del calls[:]
        _, l0, g0 = _model_run(dev, None, staged)
        assert {c[0] for c in branch()} >= {"dcn_bilstm_bwd", "dcn_embedding_bwd", "dcn_gemm_tn", "dcn_gemm_nn"}
        del calls[:]
        _, l1, g1 = _model_run(dev, ["textmodel"], staged)
        assert branch() == [], branch()
        assert l0 == l1
        assert _same_but(g0, g1, lambda k: k.startswith("textmodel.")) > 200
    m, opt, image, word_id, word_mask, bbox = _setup(dev, N, 33, ["textmodel"])
    del calls[:]
    random.seed(7)
    step = GraphedTrainStep(m, opt, image, word_id, word_mask, bbox, SIZE, warmup=1)
    step()
    torch.cuda.synchronize()
    assert branch() == [], branch()
    assert len(calls) > 0 and all(p.grad is None for p in m.textmodel.parameters())


def test_fp8_storage_trains_around_a_frozen_backbone(dev):
    """8. fp8 storage has no backward through BatchNorm on running statistics.  With the backbone's weights frozen as well it needs none:
    freeze_weights("backbone") + freeze_batchnorm("backbone") trains — finite loss and gradients, a second identical step gives the
    same bits — while freeze_batchnorm("all") (the head's blocks on running statistics, and trainable) still raises."""
    from dcnet_amd import losses, ops
    ops.set_precision("fp8s")
    try:
        m, _, image, word_id, word_mask, bbox = _setup(dev, N, 33, "backbone", bn="backbone")
        state = {k: v.clone() for k, v in m.state_dict().items()}
        runs = []
        for _ in range(2):
            m.load_state_dict(state)
            for p in m.parameters():
                p.grad = None
            m.train()
            random.seed(7)
            loss, _ = losses.total_loss(m(image, word_id, word_mask), bbox, SIZE)
            loss.backward()
            torch.cuda.synchronize()
            runs.append((float(loss.detach()), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}))
        assert runs[0][0] == runs[0][0] and abs(runs[0][0]) < float("inf")
        assert len(runs[0][1]) == 91 and not any(k.startswith("visumodel.") for k in runs[0][1])
        assert all(bool(torch.isfinite(g).all()) for g in runs[0][1].values())
        assert sum(float(g.abs().max()) > 0 for g in runs[0][1].values()) > 45
        assert runs[1][0] == runs[0][0] and runs[1][1].keys() == runs[0][1].keys()
        for k, g in runs[0][1].items():
            assert torch.equal(g, runs[1][1][k]), k
        assert m.visumodel.saved_slots == frozenset()
        m.freeze_batchnorm("all")
        m.train()
        random.seed(7)
        loss, _ = losses.total_loss(m(image, word_id, word_mask), bbox, SIZE)
        with pytest.raises(NotImplementedError, match="fp32 and bf16 storage"):
            loss.backward()
    finally:
        ops.reset_held_wgrads()
        torch.cuda.synchronize()
        ops.set_precision("fp32")
