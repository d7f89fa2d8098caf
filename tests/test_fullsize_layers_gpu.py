"""The default dispatch at the benchmark's launch sizes, against fp64: every distinct conv shape of the backbone at 64 images of 416 x 416
(derived from darknet.build_plan, shortcut flag included), the head's conv blocks at that batch, and at 256 images (the BASELINE.json
configs[4] batch) the shapes whose dispatcher decision differs from the 64-image one.  The size-gated choices — conv1.hip's 128 x 256
tile from 1024 workgroups on, the split-K slab counts at M = 11 M rows, the K-step rule, merged / separate parity classes — are only
taken here; tests/test_arms_gpu.py forces the same arms at small edge shapes.

Per shape, default knobs, fp32: forward with BatchNorm partial sums, forward with the fused epilogue (and the shortcut where the layer
has one), data gradient, weight gradient.

Reference: tests/util.py conv_by_taps in fp64 on the device (torch.matmul, one tap at a time on shifted slices of the padded input):
nothing of this library.  Half the shapes read leaky_relu(randn, 0.1), as the layers see it, the others randn.

Bound (a rule, nobody had measured these errors): error = max |got - fp64| / max |fp64|.  The same per-tap products evaluated in plain
fp32 by torch (TF32 off, asserted) give the baseline error of an independent fp32 implementation; the kernel passes with
error <= max(small-shape tolerance, 4 x baseline error) — small-shape tolerances as in tests/test_ops_gpu.py (2e-5 forward / data
gradient, 3e-5 weight gradient, 1e-4 summed partials); 4 = 2^2: the two-piece f16 split carries 22 significand bits against fp32's
24.  The bound must stay discriminating: for every weight gradient it has to be below a tenth of the relative change that zeroing one
32-row K chunk of the input makes to the fp64 reference.  Every figure is printed before it is asserted (pytest -s / -rA shows them;
the CHANGELOG records them per layer family)."""
import pytest
import torch
import torch.nn.functional as F

from util import conv_by_taps, new_product

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZE = 416


def backbone_shapes():
    """distinct (map, cin, cout, k, stride, shortcut) of the plan's convolutions at SIZE x SIZE, in plan order"""
    from dcnet_amd.darknet import _AliasOp, _ConvOp, _UpCatOp, build_plan, yolov3_blocks
    plan, _, _ = build_plan(yolov3_blocks(SIZE, SIZE)[1:])
    hw, shapes = {-1: SIZE}, []
    for op in plan:
        if isinstance(op, _ConvOp):
            h = hw[op.src]
            hw[op.slot] = hw[op.dst] = h // op.stride
            s = (h, op.cin, op.cout, op.k, op.stride, op.res is not None)
            if s not in shapes:
                shapes.append(s)
        elif isinstance(op, _UpCatOp):
            hw[op.dst] = hw[op.lat_src]
        else:
            assert isinstance(op, _AliasOp)
            hw[op.dst] = hw[op.src]
    return shapes


def head_shapes():
    """distinct shapes of the head's conv + BatchNorm blocks (mapping_visu, corr_conv, fcn_emb, fcn_out): scale i works on the
    13 * 2^i map; input channels padded to a multiple of 32 as the kernels take them"""
    from dcnet_amd import ops
    from dcnet_amd.model import ConvBatchNormReLU
    shapes = []
    for name, m in new_product(SIZE).named_modules():
        if not isinstance(m, ConvBatchNormReLU):
            continue
        parts = name.split(".")
        heads = [i for i, p in enumerate(parts) if p in ("mapping_visu", "corr_conv", "fcn_emb", "fcn_out")]
        if not heads:
            continue
        scale = int(parts[heads[0] + 1])
        s = (SIZE // 32 * 2 ** scale, ops.pad32(m.conv.in_channels), m.conv.out_channels, m.conv.kernel_size[0], 1, False)
        if s not in shapes:
            shapes.append(s)
    return shapes


BACKBONE = backbone_shapes()

# 256 images: the backbone shapes whose launches the dispatcher sends elsewhere than at 64 images — all of them conv1.hip's 128 x 256
# tile, which needs 1024 workgroups: the forward of the 26-wide 1x1 layers towards 256 filters and of the two deepest stride-2 layers,
# the data gradients of the 26- / 13-wide 1x1 layers that have 256 / 512 / 1024 input channels (found with dcn_conv1_tile, asserted below)
BATCH256 = [(26, 512, 256, 1, 1, False), (26, 768, 256, 1, 1, False), (26, 256, 128, 1, 1, False), (13, 1024, 512, 1, 1, False),
            (52, 256, 512, 3, 2, False), (26, 512, 1024, 3, 2, False)]
# the layer shapes tests/test_configs_gpu.py uses as its exact model at 64 / 256 images: its reference side is pinned here
CONFIGS_SHAPES = [(52, 128, 256, 3, 1, False), (26, 512, 256, 1, 1, False), (104, 128, 256, 3, 2, False)]


def _decision(n, shape):
    """what the dispatch queries say for a shape at n images: conv1.hip tile of the forward (with / without partials) and of the
    data gradient, rows per BatchNorm partial"""
    from dcnet_amd.lib import lib
    h, cin, cout, k, st, _ = shape
    ho = (h + 2 * ((k - 1) // 2) - k) // st + 1
    L = lib()
    rows = n * ho * ho
    fwd = (L.conv1_tile(rows, cout, k * k, cin, 1, 0), L.conv1_tile(rows, cout, k * k, cin, 0, 0)) if (k == 1 or st == 2) and cin % 32 == 0 else (0, 0)
    dgrad = L.conv1_tile(n * h * h, cin, 1, cout, 0, 0) if k == 1 else 0
    return fwd + (dgrad, -(-rows // L.conv2d_stats_rows(n, h, h, cout, k, st)) > 128)


def _err(got, ref):
    return float((got.double() - ref).abs().max()) / float(ref.abs().max())


def _report(name, what, tol, kernel, baseline, extra=""):
    bound = max(tol, 4 * baseline)
    print(f"FULLSIZE {name} {what}: kernel {kernel:.3e} fp32-baseline {baseline:.3e} bound {bound:.3e}{extra}")
    return bound


def check_layer(n, shape, leaky_input, seed):
    from dcnet_amd import ops
    assert not torch.backends.cuda.matmul.allow_tf32, "the fp32 baseline must be plain fp32"
    h, cin, cout, k, st, shortcut = shape
    name = f"{n}x{h}x{h} {cin}->{cout} {k}x{k}/{st}" + (" +shortcut" if shortcut else "")
    g = torch.Generator(device=DEV).manual_seed(seed)
    randn = lambda *s: torch.randn(*s, generator=g, device=DEV)
    stem = cin == 3
    ci = 4 if stem else cin
    x = randn(n, h, h, ci)
    if leaky_input and not stem:
        x = F.leaky_relu(x, 0.1)
    w = randn(cout, k, k, ci) / (cin * k * k) ** 0.5
    if stem:
        x[..., 3] = 0; w[..., 3] = 0
    ho = (h + 2 * ((k - 1) // 2) - k) // st + 1
    dy = randn(n, ho, ho, cout)
    scale = randn(cout).abs() + 0.5; shift = randn(cout)
    res = randn(n, ho, ho, cout) if shortcut else None
    M = n * ho * ho
    chunk = slice(M // 2, M // 2 + 32)
    # ---- this library ----
    wl = ops.weight_to_ohwi(w[..., :3].permute(0, 3, 1, 2).contiguous()) if stem else w
    raw, stats = ops.conv2d_fwd(x, wl, k, st, want_stats=True)
    y, _ = ops.conv2d_fwd(x, wl, k, st, scale, shift, ops.ACT_LEAKY, 0.1, residual=res)
    dx = None if stem else ops.conv2d_bwd_data(dy, w, (h, h), k, st)
    dw = ops.conv2d_bwd_weight(x, dy, k, st)
    if stem:
        dw = ops.weight_grad_to_oihw(dw, (cout, 3, 3, 3)).permute(0, 2, 3, 1)
    torch.cuda.synchronize()
    # ---- fp64, and the same products in fp32 ----
    raw64, dx64, dw64, dwc64 = conv_by_taps(x, w, k, st, dy, chunk=chunk)
    raw32, dx32, dw32 = conv_by_taps(x, w, k, st, dy, dtype=torch.float32)
    if stem:
        dw64, dwc64, dw32 = dw64[..., :3], dwc64[..., :3], dw32[..., :3]
    epi = lambda r, dt: F.leaky_relu(r * scale.to(dt) + shift.to(dt), 0.1) + (0 if res is None else res.to(dt))
    fails = []

    def judge(what, tol, got, ref, base, floor=None):
        e, b = _err(got, ref), _err(base, ref)
        extra = "" if floor is None else f" one-chunk change {floor:.3e}"
        bound = _report(name, what, tol, e, b, extra)
        if not e <= bound:
            fails.append(f"{what}: error {e:.3e} beyond {bound:.3e}")
        if floor is not None and not bound < 0.1 * floor:
            fails.append(f"{what}: the bound {bound:.3e} is not below a tenth of the change {floor:.3e} one 32-row K chunk makes")

    judge("forward", 2e-5, raw, raw64, raw32)
    r64 = raw64.reshape(-1, cout); r32 = raw32.reshape(-1, cout)
    judge("partials-sum", 1e-4, stats[:, 0].double().sum(0), r64.sum(0), r32.sum(0))
    judge("partials-sumsq", 1e-4, stats[:, 1].double().sum(0), (r64 * r64).sum(0), (r32 * r32).sum(0))
    judge("epilogue", 2e-5, y, epi(raw64, torch.float64), epi(raw32, torch.float32))
    if dx is not None:
        judge("dgrad", 2e-5, dx, dx64, dx32)
    judge("wgrad", 3e-5, dw, dw64, dw32, floor=float(dwc64.abs().max()) / float(dw64.abs().max()))
    del raw64, dx64, dw64, dwc64, raw32, dx32, dw32, r64, r32, x, w, dy, raw, y, dx, dw, stats, res
    torch.cuda.empty_cache()
    assert not fails, f"{name}: " + "; ".join(fails)


@pytest.mark.parametrize("i", range(len(BACKBONE)), ids=["{}-{}to{}-k{}s{}{}".format(*s[:5], "r" if s[5] else "") for s in BACKBONE])
def test_backbone_layer_at_64_images(dev, i):
    check_layer(64, BACKBONE[i], leaky_input=i % 2 == 0, seed=100 + i)


def test_head_layers_at_64_images(dev):
    shapes = head_shapes()
    assert len(shapes) >= 9 and all(s[3] in (1, 3) for s in shapes), shapes
    for i, s in enumerate(shapes):
        check_layer(64, s, leaky_input=i % 2 == 1, seed=200 + i)


def test_layers_whose_dispatch_differs_at_256_images(dev):
    differ = [s for s in BACKBONE if _decision(64, s) != _decision(256, s)]
    assert sorted(differ) == sorted(BATCH256), (differ, BATCH256)
    for i, s in enumerate(BATCH256):
        assert 18 in _decision(256, s) and 18 not in _decision(64, s), (s, _decision(64, s), _decision(256, s))
        check_layer(256, s, leaky_input=i % 2 == 0, seed=300 + i)


def test_exact_model_layers_of_the_reduced_precision_configs_at_256_images(dev):
    """the fp32 kernels tests/test_configs_gpu.py compares the bf16 / fp8 modes with, at its shapes and batches: at 64 images they are
    backbone shapes (checked above), at 256 images those not already in BATCH256 run here"""
    assert all(s in BACKBONE for s in CONFIGS_SHAPES)
    todo = [s for s in CONFIGS_SHAPES if s not in BATCH256]
    assert len(todo) == 2
    for i, s in enumerate(todo):
        check_layer(256, s, leaky_input=i % 2 == 0, seed=400 + i)
