"""CPU: the split-K workspace sizes of the weight gradient (dcn_conv2d_bwd_weight_ws / _ws_b16).  The buffer they size is shared scratch
that only grows: a size that falls behind the kernel a launch picks does not fail, it lets the slabs run into whatever follows.  Both
functions are host code: no device needed.  (tests/test_ops_gpu.py::test_wgrad_workspace_covers_every_slab is the device side.)"""
import pytest

from util import tuning

# (n, h, w, cin, cout, k, stride)
SHAPES = [
    # narrow generic tiles, the stem, tiny maps
    (2, 16, 20, 64, 32, 1, 1), (1, 32, 32, 4, 32, 3, 1), (1, 5, 3, 32, 32, 3, 1), (2, 12, 12, 32, 32, 1, 1), (1, 1, 1, 32, 32, 1, 1),
    (3, 7, 9, 96, 40, 3, 2),
    # filter rows (wgrad3.hip)
    (8, 13, 13, 128, 256, 3, 1), (2, 33, 31, 136, 160, 3, 1), (2, 40, 40, 64, 128, 3, 1), (2, 40, 40, 128, 64, 3, 1),
    # 1x1 and the wide 1x1 tile
    (8, 26, 26, 256, 512, 1, 1), (7, 25, 27, 384, 192, 1, 1), (4, 26, 26, 256, 128, 1, 1), (32, 13, 13, 1024, 512, 1, 1),
    # nine taps (wgrad9.hip), stride 1 and 2
    (1, 64, 64, 32, 64, 3, 1), (2, 64, 64, 32, 64, 3, 2), (2, 64, 64, 64, 128, 3, 1), (4, 52, 52, 32, 64, 3, 1), (16, 104, 104, 64, 128, 3, 1),
    # stride 2 on the 128 x 128 tile
    (8, 54, 58, 64, 128, 3, 2),
]
TARGET_KNOBS = ("xwgtarget", "zwgsmall", "qtargetb16", "qsmallb16")
TARGETS = [None, 1, 96, 4096]           # None: the defaults
ROUTES_OFF = {"u3row": 0, "9tap": 0, "Y1wide": 0, "w3b16": 0, "9b16": 0}
FAMILIES = [{"u3row": 1, "w3b16": 1}, {"9tap": 2, "9b16": 1}, {"Y1wide": 1}]        # filter rows, nine taps, wide 1x1
ROUTES_ON = {k: v for fam in FAMILIES for k, v in fam.items()}


def _check(b16, target):
    """asserts (i) and (ii) for every shape; returns, per shape checked, whether the generic tile splits K"""
    from dcnet_amd.lib import lib
    size = lib().conv2d_bwd_weight_ws_b16 if b16 else lib().conv2d_bwd_weight_ws
    multi = []
    with tuning({k: target for k in TARGET_KNOBS} if target else {}) as tune:
        for shape in SHAPES:
            n, h, w, cin, cout, k, stride = shape
            if b16 and (cin % 8 or cout % 8):
                continue
            # (i) no shortcut route: a whole number of slabs of the generic tile, each split with at least 256 pixels
            tune(ROUTES_OFF)
            generic = size(*shape)
            pad = (k - 1) // 2
            m = n * ((h + 2 * pad - k) // stride + 1) * ((w + 2 * pad - k) // stride + 1)
            slab = cout * (64 if cin == 4 else k * k * cin)
            assert generic % slab == 0, (shape, generic, slab)
            splits = generic // slab or 1
            assert splits <= max(m // 256, 1), (shape, splits, m)
            multi.append(splits > 1)
            # (ii) every route on: the largest of what each route family needs alone, and of the generic tile
            singles = [generic]
            for family in FAMILIES:
                tune(ROUTES_OFF); tune(family)
                singles.append(size(*shape))
            tune(ROUTES_ON)
            assert size(*shape) == max(singles), (shape, size(*shape), singles)
    return multi


@pytest.mark.parametrize("target", TARGETS, ids=lambda t: f"target={t or 'default'}")
@pytest.mark.parametrize("b16", [False, True], ids=["fp32", "bf16"])
def test_workspace_is_whole_slabs_and_covers_every_route(b16, target):
    assert _check(b16, target)


def test_the_shapes_exercise_split_k():
    """at least a third of the (entry, targets, shape) combinations split K: a later change of defaults cannot empty the test"""
    multi = [m for b16 in (False, True) for target in TARGETS for m in _check(b16, target)]
    assert 3 * sum(multi) >= len(multi), (sum(multi), len(multi))
