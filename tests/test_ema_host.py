"""CPU: the interface of the weight EMA and of AdamW (dcnet_amd.optim.WeightEMA / AdamW, train.make_optimizer, the driver's flags, the
checkpoint entry, the C entry points' argument checks).  Nothing here launches a kernel."""
import ctypes
import math

import pytest
import torch

from util import new_product


@pytest.fixture(scope="module")
def product():
    return new_product(256)


def test_weight_at_hand_values():
    """tau = 0: 1 - decay at every t.  t = 1, tau = 2000: 1 - decay * (1 - e^(-1/2000)).  The weight falls monotonically in t (the average
    follows the weights closely at first) towards 1 - decay, which it never undercuts."""
    from dcnet_amd.optim import WeightEMA, weight_at
    assert WeightEMA.weight_at is weight_at
    for t in (1, 2, 1000):
        assert weight_at(t, 0.9, 0) == 1 - 0.9 and weight_at(t, 0.9999, 0.0) == 1 - 0.9999
    assert weight_at(1, 0.9999, 2000) == 1 - 0.9999 * (1 - math.exp(-1 / 2000))
    assert abs(weight_at(1, 0.9999, 2000) - 0.99950017) < 1e-8              # e^(-1/2000) = 1 - 4.99875e-4
    assert weight_at(3, 0.9, 3) == 1 - 0.9 * (1 - math.exp(-1.0))
    ws = [weight_at(t, 0.9999, 2000.0) for t in range(1, 20001, 7)]
    assert all(a > b for a, b in zip(ws, ws[1:]))
    assert all(w >= 1 - 0.9999 for w in ws) and ws[-1] < 1.5e-4
    assert isinstance(weight_at(1, 0.5, 0), float)


@pytest.mark.parametrize("kw", [dict(decay=1.0), dict(decay=-0.1), dict(decay=1.5), dict(decay=math.nan), dict(decay="0.9"), dict(decay=True),
                                dict(tau=-1.0), dict(tau=math.nan), dict(tau=math.inf), dict(tau=None)])
def test_constructor_validates_before_it_looks_at_the_model(kw):
    from dcnet_amd.optim import WeightEMA
    with pytest.raises(ValueError, match="decay" if "decay" in kw else "tau"):
        WeightEMA(torch.nn.Linear(2, 2), **kw)


def test_cpu_model_has_no_path(product):
    from dcnet_amd.optim import WeightEMA
    for model in (torch.nn.Linear(3, 2), product):
        with pytest.raises(RuntimeError, match="no CPU path"):
            WeightEMA(model)
    with pytest.raises(RuntimeError, match="no CPU path"):
        WeightEMA(torch.nn.Linear(3, 2), decay=0.0, tau=0)          # the edges of the valid ranges pass validation


def test_make_optimizer_adamw_yields_torchs_groups(product):
    from dcnet_amd import optim
    from dcnet_amd.train import make_optimizer
    ours = make_optimizer(product, 3e-4, "adamw")
    assert type(ours) is optim.AdamW and isinstance(ours, optim.Adam)
    params = list(product.parameters())
    want = torch.optim.AdamW(params, lr=3e-4, weight_decay=1e-2)
    assert ours.state_dict()["param_groups"] == want.state_dict()["param_groups"]
    assert sorted(ours.param_groups[0]) == sorted(want.param_groups[0])
    assert ours.param_groups[0]["decoupled_weight_decay"] is True and ours.param_groups[0]["weight_decay"] == 1e-2
    assert len(ours.param_groups) == 1 and all(a is b for a, b in zip(ours.param_groups[0]["params"], params))
    stock = make_optimizer(product, 3e-4, "AdamW", fused=False)
    assert type(stock) is torch.optim.AdamW and stock.state_dict()["param_groups"] == want.state_dict()["param_groups"]
    want.load_state_dict(ours.state_dict()); ours.load_state_dict(want.state_dict())
    clipped = make_optimizer(product, 3e-4, "adamw", max_grad_norm=2.0, skip_nonfinite=True)
    assert type(clipped) is optim.AdamW and clipped.max_grad_norm == 2.0 and clipped.skip_nonfinite is True


def test_adamw_defaults_and_the_group_key():
    from dcnet_amd.optim import Adam, AdamW
    p = [torch.nn.Parameter(torch.zeros(4))]
    assert AdamW(p).state_dict()["param_groups"] == torch.optim.AdamW(p).state_dict()["param_groups"]          # lr 1e-3, weight decay 1e-2
    assert Adam(p, decoupled_weight_decay=True, weight_decay=1e-2).state_dict()["param_groups"] == torch.optim.AdamW(p).state_dict()["param_groups"]
    assert Adam(p).param_groups[0]["decoupled_weight_decay"] is False                                           # Adam itself is as it was
    assert Adam(p).state_dict()["param_groups"] == torch.optim.Adam(p).state_dict()["param_groups"]
    opt = Adam(p)                                                     # the key travels with a state_dict, as every group key does
    opt.load_state_dict(torch.optim.AdamW(p).state_dict())
    assert opt.param_groups[0]["decoupled_weight_decay"] is True


def test_options_that_are_not_built_still_raise():
    from dcnet_amd.optim import Adam, AdamW
    p = [torch.nn.Parameter(torch.zeros(4))]
    for make in (lambda: Adam(p, amsgrad=True), lambda: Adam(p, maximize=True), lambda: AdamW(p, amsgrad=True), lambda: AdamW(p, maximize=True),
                 lambda: Adam(p, decoupled_weight_decay=True, amsgrad=True)):
        with pytest.raises(NotImplementedError):
            make()
    with pytest.raises(NotImplementedError):
        AdamW(p).load_state_dict(torch.optim.AdamW(p, amsgrad=True).state_dict())
    with pytest.raises(ValueError):
        AdamW(p, weight_decay=-1.0)
    q = torch.nn.Parameter(torch.ones(8))
    opt = AdamW([q], lr=1e-2)
    q.grad = torch.ones(8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        opt.step()
    assert torch.equal(q.detach(), torch.ones(8))


def test_attach_ema_takes_an_ema_or_none():
    from dcnet_amd.optim import SGD
    opt = SGD([torch.nn.Parameter(torch.zeros(4))], lr=1e-2)
    assert opt._ema is None
    with pytest.raises(TypeError, match="WeightEMA"):
        opt.attach_ema(object())
    opt.attach_ema(None)
    assert opt._ema is None and "ema" not in opt.state_dict()


def test_train_parser_accepts_the_flags():
    from dcnet_amd.train import arg_parser, ema_args
    a = arg_parser().parse_args(["--optimizer", "adamw", "--ema-decay", "0.999", "--ema-tau", "100"])
    assert a.optimizer == "adamw" and a.ema_decay == 0.999 and a.ema_tau == 100.0
    assert ema_args(a) == dict(decay=0.999, tau=100.0)
    a = arg_parser().parse_args([])
    assert a.ema_decay is None and a.ema_tau is None and ema_args(a) is None and a.optimizer == "rmsprop"
    assert ema_args(arg_parser().parse_args(["--ema-tau", "0"])) == dict(decay=0.9999, tau=0.0)
    assert ema_args(arg_parser().parse_args(["--ema-decay", "0.5"])) == dict(decay=0.5, tau=2000.0)


def test_checkpoint_without_the_entry(tmp_path):
    """A checkpoint without "ema" loads as before; asking for the entry it lacks is a KeyError that names it — raised by the loader,
    before the EMA object is touched."""
    from dcnet_amd.train import load_checkpoint, save_checkpoint
    m = torch.nn.Linear(3, 2)
    path = save_checkpoint({"epoch": 4, "state_dict": m.state_dict(), "best_loss": 0.5}, False, "plain", str(tmp_path))
    assert load_checkpoint(torch.nn.Linear(3, 2), path) == (4, 0.5)
    with pytest.raises(KeyError, match="ema"):
        load_checkpoint(torch.nn.Linear(3, 2), path, ema=object())

    class Taker:
        got = None

        def load_state_dict(self, sd):
            self.got = sd
    path = save_checkpoint({"epoch": 4, "state_dict": m.state_dict(), "best_loss": 0.5, "ema": {"updates": 3}}, False, "with", str(tmp_path))
    taker = Taker()
    assert load_checkpoint(torch.nn.Linear(3, 2), path, ema=taker) == (4, 0.5) and taker.got == {"updates": 3}
    assert load_checkpoint(torch.nn.Linear(3, 2), path) == (4, 0.5)            # nobody asked: the entry is ignored


def test_new_entry_points_reject_bad_arguments_with_a_message():
    """Null tables, negative counts, hyper-parameters out of range: an error code and a text before any launch (the addresses handed
    over are host memory and never reach the device).  count = 0 is accepted and launches nothing."""
    from dcnet_amd.lib import DcnError, lib
    L = lib()
    numel = (ctypes.c_int64 * 2)(5, 1000)
    host = (ctypes.c_void_p * 2)(ctypes.addressof(numel), ctypes.addressof(numel))
    some = ctypes.addressof(numel)

    def refused(fn, *args, match):
        with pytest.raises(DcnError, match=match):
            fn(*args)

    refused(L.ema_prepare, 0, some, 0.9, 0.0, 0, 0, match="ema_prepare: bad argument")
    refused(L.ema_prepare, some, 0, 0.9, 0.0, 0, 0, match="ema_prepare: bad argument")
    for bad in (1.0, -0.5, math.nan):
        refused(L.ema_prepare, some, some, bad, 0.0, 0, 0, match="decay")
    for bad in (-1.0, math.nan):
        refused(L.ema_prepare, some, some, 0.9, bad, 0, 0, match="tau")
    refused(L.ema_update, host, host, numel, 2, 0, 0, 0, match="ema_update: bad argument")
    refused(L.ema_update, 0, host, numel, 2, some, 0, 0, match="ema_update: bad argument")
    refused(L.ema_update, host, host, 0, 2, some, 0, 0, match="ema_update: bad argument")
    refused(L.ema_update, host, host, numel, -1, some, 0, 0, match="ema_update: bad argument")
    refused(L.ema_update, host, (ctypes.c_void_p * 2)(some, None), numel, 2, some, 0, 0, match="null tensor 1")
    refused(L.ema_update, host, host, (ctypes.c_int64 * 2)(5, -1), 2, some, 0, 0, match="null tensor 1")
    L.ema_update(0, 0, 0, 0, some, 0, 0)
    refused(L.tensor_swap, 0, host, numel, 2, 0, match="tensor_swap: bad argument")
    refused(L.tensor_swap, host, host, numel, -2, 0, match="tensor_swap: bad argument")
    refused(L.tensor_swap, (ctypes.c_void_p * 2)(None, some), host, numel, 2, 0, match="null tensor 0")
    L.tensor_swap(0, 0, 0, 0, 0)
    refused(L.adamw_prepare, 0, host, 2, 1e-3, 0, 0.9, 0.999, 1e-2, 0, match="adamw_prepare: bad argument")
    refused(L.adamw_prepare, host, host, 0, 1e-3, 0, 0.9, 0.999, 1e-2, 0, match="adamw_prepare: bad argument")
    refused(L.adamw_prepare, host, host, 2, 1e-3, 0, 0.9, 0.999, -1e-2, 0, match="weight_decay")
    refused(L.adamw_prepare, host, host, 2, 1e-3, 0, 1.0, 0.999, 1e-2, 0, match="betas")
    refused(L.adamw_prepare_clipped, host, host, 2, 1e-3, 0, 0.9, 0.999, 1e-2, 0, 0, match="control block")
    refused(L.adamw_step, host, host, host, host, 0, numel, 2, 0.9, 0.999, 1e-8, 0, match="adamw_step: bad argument")
    refused(L.adamw_step, host, host, host, host, host, numel, 0, 0.9, 0.999, 1e-8, 0, match="adamw_step: bad argument")
    refused(L.adamw_step_clipped, host, host, host, host, host, numel, 2, 0.9, 0.999, 1e-8, 0, 0, match="control block")
    refused(L.adamw_step_clipped, host, host, host, host, host, numel, -1, 0.9, 0.999, 1e-8, some, 0, match="adamw_step_clipped: bad argument")
