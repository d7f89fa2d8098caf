"""CPU: the interface of global-norm gradient clipping and the non-finite skip (dcnet_amd.optim, train.make_optimizer, the driver's
flags, the C entry points' argument checks).  Nothing here launches a kernel."""
import ctypes
import math

import pytest
import torch

from util import new_product

CLASSES = ["RMSprop", "Adam", "SGD"]


@pytest.fixture(scope="module")
def product():
    return new_product(256)


@pytest.mark.parametrize("name", CLASSES)
@pytest.mark.parametrize("bad", [0, 0.0, -1.0, math.nan, math.inf, -math.inf])
def test_bad_max_grad_norm_raises(name, bad):
    from dcnet_amd import optim
    with pytest.raises(ValueError, match="max_grad_norm"):
        getattr(optim, name)([torch.nn.Parameter(torch.zeros(4))], lr=1e-2, max_grad_norm=bad)


@pytest.mark.parametrize("name", CLASSES)
def test_options_are_attributes_not_group_keys(name):
    """torch's group layout is untouched: no new key in the groups or in state_dict()["param_groups"], whatever the options are, and
    skip_nonfinite alone (no threshold) is accepted."""
    from dcnet_amd import optim
    cls = getattr(optim, name)
    p = [torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(3, 2))]
    plain = cls(p, lr=1e-2)
    assert plain.max_grad_norm is None and plain.skip_nonfinite is False and not plain.clipping
    assert plain.grad_norm is None and plain.skipped_steps() == 0
    for kw in ({"max_grad_norm": 2.5}, {"skip_nonfinite": True}, {"max_grad_norm": 3, "skip_nonfinite": True}):
        opt = cls(p, lr=1e-2, **kw)
        assert opt.clipping
        assert opt.max_grad_norm == kw.get("max_grad_norm") and opt.skip_nonfinite is kw.get("skip_nonfinite", False)
        assert [sorted(g) for g in opt.param_groups] == [sorted(g) for g in plain.param_groups]
        assert opt.state_dict()["param_groups"] == plain.state_dict()["param_groups"]
        assert opt.state_dict()["state"] == {}
        # checkpoints move both ways between an optimiser with the options and one without
        plain.load_state_dict(opt.state_dict()); opt.load_state_dict(plain.state_dict())
        assert opt.max_grad_norm == kw.get("max_grad_norm")


def test_clip_grad_norm_refuses_other_norms_and_cpu_gradients():
    from dcnet_amd.optim import clip_grad_norm_
    p = torch.nn.Parameter(torch.ones(8))
    p.grad = torch.ones(8)
    for norm_type in (1, 1.0, math.inf, 3):
        with pytest.raises(NotImplementedError):
            clip_grad_norm_([p], 1.0, norm_type=norm_type)
    with pytest.raises(RuntimeError, match="no CPU path"):
        clip_grad_norm_([p], 1.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        clip_grad_norm_(p, 1.0)                      # a single tensor, as torch's function accepts
    with pytest.raises(ValueError):
        clip_grad_norm_([p], 0.0)
    assert torch.equal(p.grad, torch.ones(8))
    q = torch.nn.Parameter(torch.ones(3))            # nothing to clip: torch's answer, a zero
    assert float(clip_grad_norm_([q], 1.0)) == 0.0


@pytest.mark.parametrize("name", ["rmsprop", "adam", "sgd"])
def test_make_optimizer_passes_the_options(product, name):
    from dcnet_amd import optim
    from dcnet_amd.train import make_optimizer
    opt = make_optimizer(product, 1e-4, name, max_grad_norm=7.5, skip_nonfinite=True)
    assert type(opt) is {"rmsprop": optim.RMSprop, "adam": optim.Adam, "sgd": optim.SGD}[name]
    assert opt.max_grad_norm == 7.5 and opt.skip_nonfinite is True
    off = make_optimizer(product, 1e-4, name)
    assert off.max_grad_norm is None and off.skip_nonfinite is False
    assert opt.state_dict()["param_groups"] == off.state_dict()["param_groups"]
    with pytest.raises(ValueError, match="max_grad_norm"):
        make_optimizer(product, 1e-4, name, max_grad_norm=-1.0)


@pytest.mark.parametrize("name", ["adam", "sgd"])
def test_make_optimizer_unfused_points_at_the_function(product, name):
    from dcnet_amd.train import make_optimizer
    with pytest.raises(ValueError, match="clip_grad_norm_"):
        make_optimizer(product, 1e-4, name, fused=False, max_grad_norm=1.0)
    with pytest.raises(ValueError, match="clip_grad_norm_"):
        make_optimizer(product, 1e-4, name, fused=False, skip_nonfinite=True)


def test_train_parser_accepts_the_flags():
    from dcnet_amd.train import arg_parser
    a = arg_parser().parse_args(["--clip-grad-norm", "12.5", "--skip-nonfinite", "--optimizer", "adam"])
    assert a.clip_grad_norm == 12.5 and a.skip_nonfinite is True
    a = arg_parser().parse_args([])
    assert a.clip_grad_norm is None and a.skip_nonfinite is False


def test_graphed_step_hands_out_the_optimisers_norm():
    from dcnet_amd.graph import GraphedTrainStep

    class Opt:
        grad_norm = "norm"
    step = GraphedTrainStep.__new__(GraphedTrainStep)
    step.opt = Opt()
    assert step.grad_norm == "norm"
    step.opt = object()
    assert step.grad_norm is None


def test_new_entry_points_reject_bad_arguments_with_a_message():
    """Null pointers, count <= 0, max_norm <= 0 (and NaN), a partials buffer of the wrong size: an error code and a text, before any
    launch — the addresses handed over are host memory and are never dereferenced on the device."""
    from dcnet_amd.lib import DcnError, lib
    L = lib()
    numel = (ctypes.c_int64 * 2)(5, 1000)
    host = (ctypes.c_void_p * 2)(ctypes.addressof(numel), ctypes.addressof(numel))         # two non-null "tensors"
    some = ctypes.addressof(numel)
    assert L.grad_sumsq_slots(numel, 2) == 2                  # one chunk: blocks_for(1000) = 1 block x 2 tensors
    big = (ctypes.c_int64 * 33)(*([1 << 20] * 32 + [7]))
    assert L.grad_sumsq_slots(big, 33) == 128 * 32 + 1        # (2^20 / 4 + 255) / 256 = 1024 -> capped at 128; second chunk 1 x 1
    assert L.grad_sumsq_slots(0, 2) == -1 and L.grad_sumsq_slots(numel, 0) == -1
    neg = (ctypes.c_int64 * 2)(5, -1)
    assert L.grad_sumsq_slots(neg, 2) == -1

    def refused(fn, *args, match):
        with pytest.raises(DcnError, match=match):
            fn(*args)

    refused(L.grad_sumsq, 0, numel, 2, some, 2, 0, match="grad_sumsq: bad argument")
    refused(L.grad_sumsq, host, 0, 2, some, 2, 0, match="grad_sumsq: bad argument")
    refused(L.grad_sumsq, host, numel, 2, 0, 2, 0, match="grad_sumsq: bad argument")
    refused(L.grad_sumsq, host, numel, 0, some, 2, 0, match="grad_sumsq: bad argument")
    refused(L.grad_sumsq, host, numel, -3, some, 2, 0, match="grad_sumsq: bad argument")
    refused(L.grad_sumsq, (ctypes.c_void_p * 2)(some, None), numel, 2, some, 2, 0, match="null tensor 1")
    refused(L.grad_sumsq, host, numel, 2, some, 3, 0, match="slots")
    refused(L.grad_clip_coef, 0, 2, 1.0, 0, some, 0, match="grad_clip_coef: bad argument")
    refused(L.grad_clip_coef, some, 2, 1.0, 0, 0, 0, match="grad_clip_coef: bad argument")
    refused(L.grad_clip_coef, some, 0, 1.0, 0, some, 0, match="grad_clip_coef: bad argument")
    for bad in (0.0, -2.0, math.nan):
        refused(L.grad_clip_coef, some, 2, bad, 0, some, 0, match="max_norm")
    refused(L.grad_scale, 0, numel, 2, some, 0, match="grad_scale: bad argument")
    refused(L.grad_scale, host, numel, 2, 0, 0, match="grad_scale: bad argument")
    refused(L.grad_scale, host, numel, 0, some, 0, match="grad_scale: bad argument")
    refused(L.rmsprop_step_clipped, host, host, host, numel, 2, 1e-3, 0, 0.99, 1e-8, 0.0, 0, 0, match="control block")
    refused(L.rmsprop_step_clipped, host, host, host, numel, 0, 1e-3, 0, 0.99, 1e-8, 0.0, some, 0, match="rmsprop_step_clipped: bad argument")
    refused(L.rmsprop_step_clipped, 0, host, host, numel, 2, 1e-3, 0, 0.99, 1e-8, 0.0, some, 0, match="rmsprop_step_clipped: bad argument")
    refused(L.sgd_step_clipped, host, host, host, numel, 2, 1e-3, 0, 0.99, 0.0, 0, 0, match="control block")
    refused(L.sgd_step_clipped, host, host, host, numel, -1, 1e-3, 0, 0.99, 0.0, some, 0, match="sgd_step_clipped: bad argument")
    refused(L.sgd_step_clipped, host, 0, host, numel, 2, 1e-3, 0, 0.99, 0.0, some, 0, match="sgd_step_clipped: bad argument")
    refused(L.adam_prepare_clipped, host, host, 2, 1e-3, 0, 0.9, 0.999, 0, 0, match="control block")
    refused(L.adam_prepare_clipped, host, host, 0, 1e-3, 0, 0.9, 0.999, some, 0, match="adam_prepare_clipped: bad argument")
    refused(L.adam_prepare_clipped, 0, host, 2, 1e-3, 0, 0.9, 0.999, some, 0, match="adam_prepare_clipped: bad argument")
    refused(L.adam_step_clipped, host, host, host, host, host, numel, 2, 0.9, 0.999, 1e-8, 0.0, 0, 0, match="control block")
    refused(L.adam_step_clipped, host, host, host, host, host, numel, 0, 0.9, 0.999, 1e-8, 0.0, some, 0, match="adam_step_clipped: bad argument")
    refused(L.adam_step_clipped, host, host, host, host, 0, numel, 2, 0.9, 0.999, 1e-8, 0.0, some, 0, match="adam_step_clipped: bad argument")


def test_update_entry_points_check_every_tensor_before_the_first_launch():
    """33 tensors — a second chunk of 32 — of 0 values each, a null gradient at index 32: the update entry points name tensor 32 and
    launch nothing before they do (without a GPU a launch of the first chunk would fail with another text).  With 0 values per
    tensor a launch that did happen would dereference nothing."""
    from dcnet_amd.lib import DcnError, lib
    L = lib()
    n = 33
    numel = (ctypes.c_int64 * n)(*([0] * n))
    some = ctypes.addressof(numel)
    host = (ctypes.c_void_p * n)(*([some] * n))
    grads = (ctypes.c_void_p * n)(*([some] * (n - 1) + [None]))
    for fn, args in ((L.rmsprop_step, (host, grads, host, numel, n, 1e-3, 0, 0.99, 1e-8, 0.0, 0)),
                     (L.sgd_step, (host, grads, host, numel, n, 1e-3, 0, 0.9, 0.0, 0)),
                     (L.adam_step, (host, grads, host, host, host, numel, n, 0.9, 0.999, 1e-8, 0.0, 0)),
                     (L.adamw_step, (host, grads, host, host, host, numel, n, 0.9, 0.999, 1e-8, 0))):
        with pytest.raises(DcnError, match="null tensor 32"):
            fn(*args)
