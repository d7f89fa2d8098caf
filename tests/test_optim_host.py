"""CPU: the fused Adam / SGD of dcnet_amd.optim stand where torch.optim's stood — same groups and hyper-parameters out of
train.make_optimizer, the options that are not built refuse loudly, and there is no CPU path."""
import pytest
import torch

from util import new_product


@pytest.fixture(scope="module")
def product():
    return new_product(256)


@pytest.mark.parametrize("name", ["adam", "sgd"])
def test_make_optimizer_yields_torchs_groups(product, name):
    from dcnet_amd import optim
    from dcnet_amd.train import make_optimizer
    ours = make_optimizer(product, 3e-4, name)
    assert type(ours) is {"adam": optim.Adam, "sgd": optim.SGD}[name]
    params = list(product.parameters())
    want = (torch.optim.Adam(params, lr=3e-4, weight_decay=0.0005) if name == "adam"            # train_DCNet.py:528-531
            else torch.optim.SGD(params, lr=3e-4, momentum=0.99))
    assert ours.state_dict()["param_groups"] == want.state_dict()["param_groups"]
    assert len(ours.param_groups) == 1 and len(ours.param_groups[0]["params"]) == len(params)
    assert all(a is b for a, b in zip(ours.param_groups[0]["params"], params))                 # model.parameters() order
    stock = make_optimizer(product, 3e-4, name, fused=False)                                   # torch's classes stay reachable
    assert type(stock) is type(want) and stock.state_dict()["param_groups"] == want.state_dict()["param_groups"]
    # an untouched optimiser's state_dict moves both ways
    want.load_state_dict(ours.state_dict()); ours.load_state_dict(want.state_dict())


def test_default_is_still_the_two_group_rmsprop(product):
    from dcnet_amd import optim
    from dcnet_amd.train import make_optimizer
    opt = make_optimizer(product, 1e-4)
    assert type(opt) is optim.RMSprop and [g["lr"] for g in opt.param_groups] == [1e-4, 1e-5]
    assert sum(len(g["params"]) for g in opt.param_groups) == len(list(product.parameters()))


def test_options_that_are_not_built_raise():
    from dcnet_amd.optim import SGD, Adam
    p = [torch.nn.Parameter(torch.zeros(4))]
    for make in (lambda: Adam(p, amsgrad=True), lambda: Adam(p, maximize=True), lambda: SGD(p, momentum=0.9, nesterov=True),
                 lambda: SGD(p, momentum=0.9, dampening=0.1), lambda: SGD(p, maximize=True)):
        with pytest.raises(NotImplementedError):
            make()
    # ... and a state_dict that asks for one of them is refused when it is loaded
    opt = Adam(p)
    sd = torch.optim.Adam(p, amsgrad=True).state_dict()
    with pytest.raises(NotImplementedError):
        opt.load_state_dict(sd)


@pytest.mark.parametrize("name", ["Adam", "SGD"])
def test_cpu_parameter_has_no_path(name):
    from dcnet_amd import optim
    p = torch.nn.Parameter(torch.ones(8))
    opt = getattr(optim, name)([p], lr=1e-2)
    p.grad = torch.ones(8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        opt.step()
    assert torch.equal(p.detach(), torch.ones(8))
