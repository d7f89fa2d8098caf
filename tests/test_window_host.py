"""CPU: the interface of window training (``n_frame`` of train.train_step / graph.GraphedTrainStep, the driver's ``--n-frame``,
losses.window_loss's shape checks, the argument checks of the dcn_coattn_center_* entry points).  Nothing here launches a kernel."""
import inspect

import pytest
import torch


def test_driver_flag_parses():
    from dcnet_amd.train import arg_parser
    ap = arg_parser()
    assert ap.parse_args([]).n_frame is None
    a = ap.parse_args(["--n-frame", "5", "--clips", "8", "--size", "416"])
    assert a.n_frame == 5 and a.clips == 8 and a.frames is None       # (--frames defaults to K: resolved by main())
    with pytest.raises(SystemExit):
        ap.parse_args(["--n-frame", "five"])
    assert "--n-frame" in ap.format_help() and "exactly K" in ap.format_help()


def test_driver_refuses_frames_that_are_not_one_window(capsys):
    """--frames other than K, and K < 2, end in argparse's error before the model is built."""
    from dcnet_amd.train import main
    for argv in (["--n-frame", "3", "--frames", "6"], ["--n-frame", "1"]):
        with pytest.raises(SystemExit) as e:
            main(argv)
        assert e.value.code == 2
        assert "--n-frame" in capsys.readouterr().err


def test_step_functions_accept_n_frame():
    from dcnet_amd.graph import GraphedTrainStep
    from dcnet_amd.train import train_step
    for fn in (train_step, GraphedTrainStep.__init__):
        p = inspect.signature(fn).parameters
        assert "n_frame" in p and p["n_frame"].default is None, fn


@pytest.mark.parametrize("n_frame", [4, 0, 1, True, 2.0])
def test_captured_step_refuses_a_batch_that_is_no_multiple_of_n_frame_before_any_warm_up(n_frame):
    """6 images are not windows of 4, and n_frame must be an integer >= 2: ValueError before anything touches model or device."""
    from dcnet_amd.graph import GraphedTrainStep
    image = torch.zeros(6, 3, 32, 32)
    with pytest.raises(ValueError, match="n_frame"):
        GraphedTrainStep(None, None, image, torch.ones(2, 20, dtype=torch.long), None, torch.zeros(2, 4), 32, n_frame=n_frame)


def _fake(n_out, B, g=(2, 4, 8)):
    z = lambda *s: torch.zeros(*s)
    five = ([z(B, 15, x, x) for x in g], [z(B, x, x) for x in g], [z(B, x, x) for x in g], [z(B, 512, x, x) for x in g], z(B, 512, 1, 1))
    return five if n_out == 5 else five + tuple([z(1)] for _ in range(n_out - 5))


def test_window_loss_checks_shapes_before_any_device_work():
    """CPU tensors: a device call would raise RuntimeError ("HIP kernels only"); the shape errors come first, as ValueError."""
    from dcnet_amd.losses import window_loss
    B, T = 2, 3
    with pytest.raises(ValueError, match="5-tuple"):
        window_loss(_fake(11, B), torch.zeros(B, 4), 64)
    with pytest.raises(ValueError, match="5-tuple"):
        window_loss(_fake(5, B)[:4], torch.zeros(B, 4), 64)
    with pytest.raises(ValueError, match="bbox"):
        window_loss(_fake(5, B), torch.zeros(B * T, 4), 64)
    with pytest.raises(ValueError, match="bbox"):
        window_loss(_fake(5, B), torch.zeros(B, 5), 64)
    with pytest.raises(ValueError, match="bbox"):
        window_loss(_fake(5, B), torch.zeros(4), 64)
    with pytest.raises(RuntimeError, match="HIP kernels only"):       # well-formed: only now does it ask for the device
        window_loss(_fake(5, B), torch.zeros(B, 4), 64)


def test_entry_points_refuse_bad_arguments_with_a_message():
    """No device memory: the pointers are never dereferenced, every call ends at its argument check (fake non-null addresses are
    16-byte aligned so that the shape checks are what is reached)."""
    from dcnet_amd.lib import DcnError, lib
    L = lib()
    assert L.version() == 318
    p = 4096
    fwd = lambda clips=p, attn=p, E=p, rinv=p, ws=p, b=2, t=3, hw=25, c=96, ctr=1: \
        L.coattn_center_fwd(clips, attn, 2 * c, 0, 0, E, rinv, ws, b, t, hw, c, ctr, 10.0, 0)
    bwd = lambda clips=p, d_attn=p, attn=p, E=p, rinv=p, d_clips=p, ws=p, b=2, t=3, hw=25, c=96, ctr=1: \
        L.coattn_center_bwd(clips, d_attn, 2 * c, 0, 0, attn, 2 * c, 0, 0, E, rinv, d_clips, 1, ws, b, t, hw, c, ctr, 10.0, 0)
    for name in ("clips", "attn", "E", "rinv", "ws"):
        with pytest.raises(DcnError, match="coattn_center_fwd: null pointer"):
            fwd(**{name: 0})
    for name in ("clips", "d_attn", "attn", "E", "rinv", "d_clips", "ws"):
        with pytest.raises(DcnError, match="coattn_center_bwd: null pointer"):
            bwd(**{name: 0})
    for call, who in ((fwd, "coattn_center_fwd"), (bwd, "coattn_center_bwd")):
        with pytest.raises(DcnError, match=who + r".*c=100 must be a multiple of 32"):
            call(c=100)
        for t in (1, 0, -3):
            with pytest.raises(DcnError, match=who + r".*t >= 2"):
                call(t=t)
        for ctr in (-1, 3, 7):
            with pytest.raises(DcnError, match=who + r".*ctr=-?\d+ out of range"):
                call(ctr=ctr)
        with pytest.raises(DcnError, match=who):
            call(b=0)
        with pytest.raises(DcnError, match=who + r".*16-byte"):
            call(clips=4100)


def test_sizes_are_host_arithmetic():
    """E holds one hw x ld_pad(hw) matrix per clip and neighbour (no split copy below the gemm3 shapes); the backward's workspace holds
    ONE such matrix per clip, however many neighbours; degenerate shapes size to 0."""
    from dcnet_amd.lib import lib
    L = lib()
    b, t, hw, c = 2, 5, 25, 96
    assert L.coattn_center_saved_size(b, t, hw, c) == L.coattn_e_size(b * (t - 1), hw) == b * 4 * 25 * 32
    ws3, ws5 = L.coattn_center_bwd_ws(b, 3, hw, c), L.coattn_center_bwd_ws(b, 5, hw, c)
    assert ws3 >= b * hw * 32 + b * hw * c + b * hw
    assert 0 < ws5 - ws3 < b * hw * 32, "the product buffer must not grow with the number of neighbours"
    assert L.coattn_center_bwd_ws(b, 3, hw, c) < L.coattn_bwd_ws(b, hw, c)
    assert L.coattn_center_saved_size(b, 1, hw, c) == 0 and L.coattn_center_bwd_ws(0, 3, hw, c) == 0
