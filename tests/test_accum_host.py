"""CPU: the interface of gradient accumulation (``accum_steps`` of dcnet_amd.optim's classes, the host mirror of the window position,
train.make_optimizer, the driver's flag, the C entry points' argument checks).  Nothing here launches a kernel."""
import ctypes

import pytest
import torch

from util import new_product


def _classes():
    from dcnet_amd import optim
    return [optim.RMSprop, optim.Adam, optim.AdamW, optim.SGD]


@pytest.mark.parametrize("bad", [0, -1, True, False, 2.0, "2", None])
def test_constructors_refuse_what_is_not_an_integer_from_one_up(bad):
    for cls in _classes():
        with pytest.raises(ValueError, match="accum_steps"):
            cls([torch.nn.Parameter(torch.zeros(4))], accum_steps=bad)


def test_accum_steps_is_an_attribute_not_a_group_key():
    """Groups and state_dict keep torch's layout whatever K is; K = 1 is the default."""
    for cls in _classes():
        p = [torch.nn.Parameter(torch.zeros(4))]
        one, four = cls(p), cls(p, accum_steps=4)
        assert one.accum_steps == 1 and four.accum_steps == 4 and type(four.accum_steps) is int
        assert "accum_steps" not in four.param_groups[0] and "accum_steps" not in four.defaults
        assert four.state_dict() == one.state_dict()
        assert four.grad_norm is None and four.skipped_steps() == 0
        four.load_state_dict(one.state_dict())                       # nothing on a device yet: allowed anywhere
        assert four.window_position == 0


def test_window_position_is_a_host_mirror_that_bump_steps_advances():
    """K = 3: at_boundary is True exactly while two calls of the window are done; bump_steps (a replay ran one call) walks 0, 1, 2, 0
    and adds to the step counters only when it closes a window; reset_accumulation goes back to 0.  K = 1: always at the boundary,
    every bump counts."""
    from dcnet_amd.optim import RMSprop
    p = torch.nn.Parameter(torch.zeros(4))
    opt = RMSprop([p], accum_steps=3)
    counter = torch.zeros(())
    opt._stepped, opt._stepped_params = [counter], [p]
    seen = []
    for _ in range(7):
        seen.append((opt.window_position, opt.at_boundary))
        opt.bump_steps()
    assert seen == [(0, False), (1, False), (2, True)] * 2 + [(0, False)]
    assert float(counter) == 2 and opt.window_position == 1
    opt.reset_accumulation()
    assert opt.window_position == 0 and not opt.at_boundary
    one = RMSprop([p])
    one._stepped = [counter]
    for _ in range(3):
        assert one.at_boundary and one.window_position == 0
        one.bump_steps()
    assert float(counter) == 5
    one.accumulate()                                                 # K = 1: nothing to do, nothing to refuse
    one.accumulate()


def test_no_cpu_path():
    from dcnet_amd.optim import SGD
    q = torch.nn.Parameter(torch.ones(8))
    opt = SGD([q], lr=1e-2, accum_steps=2)
    q.grad = torch.ones(8)
    for call in (opt.accumulate, opt.step):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    assert torch.equal(q.detach(), torch.ones(8)) and opt.window_position == 0


def test_make_optimizer_passes_accum_steps_on():
    from dcnet_amd import optim
    from dcnet_amd.train import make_optimizer
    product = new_product(256)
    for name, cls in (("rmsprop", optim.RMSprop), ("adam", optim.Adam), ("adamw", optim.AdamW), ("sgd", optim.SGD)):
        opt = make_optimizer(product, 3e-4, name, accum_steps=4, max_grad_norm=2.0)
        assert type(opt) is cls and opt.accum_steps == 4 and opt.max_grad_norm == 2.0
        assert make_optimizer(product, 3e-4, name).accum_steps == 1
        assert opt.state_dict()["param_groups"] == make_optimizer(product, 3e-4, name).state_dict()["param_groups"]
    for bad in (0, True, 1.5):
        with pytest.raises(ValueError, match="accum_steps"):
            make_optimizer(product, 3e-4, "adam", accum_steps=bad)
    with pytest.raises(ValueError, match="accum_steps belongs to the fused optimisers"):
        make_optimizer(product, 3e-4, "adam", fused=False, accum_steps=2)
    assert type(make_optimizer(product, 3e-4, "adam", fused=False, accum_steps=1)) is torch.optim.Adam


def test_train_parser_accepts_the_flag():
    from dcnet_amd.train import arg_parser
    assert arg_parser().parse_args([]).accum_steps == 1
    a = arg_parser().parse_args(["--accum-steps", "4", "--steps", "10", "--clip-grad-norm", "1.0"])
    assert a.accum_steps == 4 and a.steps == 10
    with pytest.raises(SystemExit):
        arg_parser().parse_args(["--accum-steps", "two"])


def test_bench_optim_accepts_the_flag():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "bench_optim.py")
    spec = importlib.util.spec_from_file_location("bench_optim_for_accum", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.arg_parser().parse_args(["--accum", "4", "--step"])
    assert a.accum == 4 and a.step and mod.arg_parser().parse_args([]).accum == 0


def test_new_entry_points_reject_bad_arguments_with_a_message():
    """Null tables, negative counts, k < 1, a null block: an error code and a text before any launch (the addresses handed over are
    host memory and never reach the device).  count = 0 is accepted and launches nothing."""
    from dcnet_amd.lib import ABI_VERSION, DcnError, lib
    L = lib()
    assert ABI_VERSION == 318 and L.version() == 318
    numel = (ctypes.c_int64 * 2)(5, 1000)
    host = (ctypes.c_void_p * 2)(ctypes.addressof(numel), ctypes.addressof(numel))
    some = ctypes.addressof(numel)

    def refused(fn, *args, match):
        with pytest.raises(DcnError, match=match):
            fn(*args)

    refused(L.accum_prepare, 0, 2, 0, match="accum_prepare: no accumulation block")
    for k in (0, -3):
        refused(L.accum_prepare, some, k, 0, match="accum_prepare: k = ")
    refused(L.grad_accumulate, 0, host, numel, 2, some, 0, match="grad_accumulate: bad argument")
    refused(L.grad_accumulate, host, 0, numel, 2, some, 0, match="grad_accumulate: bad argument")
    refused(L.grad_accumulate, host, host, 0, 2, some, 0, match="grad_accumulate: bad argument")
    refused(L.grad_accumulate, host, host, numel, -1, some, 0, match="grad_accumulate: bad argument")
    refused(L.grad_accumulate, host, host, numel, 2, 0, 0, match="grad_accumulate: no accumulation block")
    refused(L.grad_accumulate, 0, 0, 0, 0, 0, 0, match="grad_accumulate: no accumulation block")
    refused(L.grad_accumulate, host, (ctypes.c_void_p * 2)(some, None), numel, 2, some, 0, match="null tensor 1")
    refused(L.grad_accumulate, (ctypes.c_void_p * 2)(None, some), host, numel, 2, some, 0, match="null tensor 0")
    refused(L.grad_accumulate, host, host, (ctypes.c_int64 * 2)(5, -1), 2, some, 0, match="null tensor 1")
    L.grad_accumulate(0, 0, 0, 0, some, 0)
    refused(L.accum_clip_coef, some, 8, 1.0, 0, some, 0, 0, match="accum_clip_coef: bad argument")            # no control block
    refused(L.accum_clip_coef, 0, 8, 1.0, 0, some, some, 0, match="accum_clip_coef: bad argument")            # slots without partials
    refused(L.accum_clip_coef, some, 0, 1.0, 0, some, some, 0, match="accum_clip_coef: bad argument")         # partials without slots
    refused(L.accum_clip_coef, some, -4, 1.0, 0, some, some, 0, match="accum_clip_coef: bad argument")
    refused(L.accum_clip_coef, some, 8, 1.0, 0, 0, some, 0, match="accum_clip_coef: no accumulation block")
    refused(L.accum_clip_coef, 0, 0, 1.0, 0, 0, some, 0, match="accum_clip_coef: no accumulation block")
    for bad in (0.0, -1.0, float("nan")):
        refused(L.accum_clip_coef, some, 8, bad, 0, some, some, 0, match="max_norm")
