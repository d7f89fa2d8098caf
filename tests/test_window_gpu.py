"""GPU: window training — the centre-versus-neighbours co-attention of csrc/coattn_center.hip (host code: the kernels it launches are the
pair node's, in csrc/coattn.hip, in their row-only forms) against fp64 torch, on the engines it must run on and bit for bit against the
pair forward, the window model in train mode through functions.CoAttentionWindow and losses.window_loss against the oracle, and the
captured window step (graph.GraphedTrainStep(..., n_frame=K)) against the eager one it was captured from."""
import pytest
import torch
import torch.nn.functional as F

from util import build_product, close as _close, maxdiff, prof_launches as _prof_launches, rand as _rand, synth_sd

pytestmark = pytest.mark.gpu
TOL = 1e-3

# (B, T, g, C), HW = g * g
KERNEL_SHAPES = [(2, 3, 5, 96),       # tile engines; HW = 25, neither a multiple of 4 nor of 32
                 (1, 4, 13, 512),     # even T: ctr = 2, two neighbours before the centre and one after
                 (2, 3, 23, 256),     # gemm3 path (HW >= 512, C >= 256) with an odd row count (529)
                 (1, 5, 26, 256)]     # gemm3, four neighbours


def _on_gemm3(hw, c):
    return hw >= 512 and c >= 256


@pytest.mark.parametrize("b,t,g,c", KERNEL_SHAPES)
def test_coattn_center_fwd_bwd(dev, b, t, g, c):
    """The construction of test_ops_gpu.py::test_coattn_fwd_bwd for the one-sided node: normalised random features, fp64 torch as the
    reference, outputs in a 2C-wide slice, the centre's gradient accumulated onto a random base.  d_clips starts as that base in EVERY
    frame: a neighbour's rows must come out as that neighbour's fp64 gradient alone (written, not added to, and by no other neighbour),
    the centre's as base + the sum over the neighbours.  Tolerances: 2e-5 on attn, 5e-5 on the gradients (that test's)."""
    from dcnet_amd import ops
    from dcnet_amd.lib import lib
    hw, ctr, temp = g * g, t // 2, 10.0
    others = [j for j in range(t) if j != ctr]
    clips = F.normalize(_rand(b, t, hw, c, seed=60), dim=3)
    d_out = _rand(t - 1, b, hw, c, seed=61)
    base = _rand(b, t, hw, c, seed=62)
    # fp64: one leaf per use of a frame, so that every neighbour's share of the centre's gradient is seen on its own
    ctr_leaves = [clips[:, ctr].double().requires_grad_(True) for _ in others]
    nb_leaves = [clips[:, j].double().requires_grad_(True) for j in others]
    ref_out = []
    for n in range(t - 1):
        A = torch.bmm(ctr_leaves[n], nb_leaves[n].transpose(1, 2))
        o = torch.bmm(F.softmax(A * temp, dim=2), nb_leaves[n])
        (o * d_out[n].double()).sum().backward()
        ref_out.append(o.detach())
    ref_ctr = sum(l.grad for l in ctr_leaves)

    cd = clips.to(dev)
    cat = torch.zeros(t - 1, b, hw, 2 * c, device=dev)                 # outputs land in a slice (ldo = 2c)
    dcat = torch.zeros(t - 1, b, hw, 2 * c, device=dev)
    dcat[..., c:] = d_out.to(dev)
    lib().prof_enable(1)
    try:
        E, rinv = ops.coattn_center_fwd(cd, ctr, cat[..., c:], temp)
        d = base.to(dev).clone()
        ops.coattn_center_bwd(cd, ctr, dcat[..., c:], cat[..., c:], E, rinv, d, True, temp)
        torch.cuda.synchronize()
    finally:
        lib().prof_enable(0)
    ran = _prof_launches(40)
    assert float(cat[..., :c].abs().max()) == 0.0, "the call wrote outside its slice"
    for n, j in enumerate(others):
        _close(cat[n, :, :, c:], ref_out[n].float(), 2e-5, f"attn of frame {j}")
        _close(d[:, j], nb_leaves[n].grad.float(), 5e-5, f"d_f of frame {j}: its own neighbour's gradient, nothing else")
    _close(d[:, ctr], ref_ctr.float() + base[:, ctr], 5e-5, "d_f_ctr = base + sum over the neighbours")
    # accumulate = False: the centre's rows are written as well (a NaN base must not survive anywhere)
    d2 = torch.full((b, t, hw, c), float("nan"), device=dev)
    ops.coattn_center_bwd(cd, ctr, dcat[..., c:], cat[..., c:], E, rinv, d2, False, temp)
    _close(d2[:, ctr], ref_ctr.float(), 5e-5, "d_f_ctr without a base")
    assert torch.equal(d2[:, others], d[:, others]), "neighbour rows depend on the accumulate flag"
    # Engines.  Per neighbour the call runs 2 products forward (A = f_ctr . f_j^T, attn = E . f_j) and 4 backward (dP = d_attn . f_j^T,
    # dA . f_j, dA^T . f_ctr, E^T . d_attn / rowsum): 6 * (T - 1) launches on gemm3.hip where coattn_on_gemm3 holds (tag 40), none below.
    assert ran == (6 * (t - 1) if _on_gemm3(hw, c) else 0), ("which engine ran the products", ran)


@pytest.mark.parametrize("b,g,c", [(2, 5, 96),       # tile engines; HW = 25, neither a multiple of 4 nor of 32
                                   (2, 23, 256)])    # gemm3, an odd row count
def test_window_of_two_is_the_pair_forward_bitwise(dev, b, g, c):
    """A window of T = 2 (ctr = 1) attends from frame 1 to frame 0: the same A product, the same row sums and the same E . f product as
    the first direction of the pair node on (f1, f2) = (frame 1, frame 0).  Both run ONE set of kernels and one product path, so the
    two outputs (each in a 2C-wide slice) are equal bit for bit."""
    from dcnet_amd import ops
    hw, temp = g * g, 10.0
    clips = F.normalize(_rand(b, 2, hw, c, seed=80), dim=3).to(dev)
    win = torch.zeros(1, b, hw, 2 * c, device=dev)
    pair = torch.zeros(b, hw, 2 * c, device=dev)
    ops.coattn_center_fwd(clips, 1, win[..., c:], temp)
    ops.coattn_fwd(clips[:, 1], clips[:, 0], pair[..., c:], None, temp)
    assert float(pair[..., c:].abs().max()) > 0
    assert torch.equal(win[0], pair), ("window and pair forward differ", maxdiff(win[0], pair))


@pytest.mark.parametrize("b,t,g,c", KERNEL_SHAPES)
def test_window_node_matches_fp64_autograd(dev, b, t, g, c):
    """functions.CoAttentionWindow as autograd sees it: cat[n] = [f_ctr | attn_n], one (B,T,HW,C) gradient with the pass-through halves
    of all T - 1 concats in the centre's rows."""
    from dcnet_amd.functions import CoAttentionWindow
    hw, ctr, temp = g * g, t // 2, 10.0
    others = [j for j in range(t) if j != ctr]
    clips = F.normalize(_rand(b, t, hw, c, seed=70), dim=3)
    w = _rand(t - 1, b, hw, 2 * c, seed=71)
    x = clips.double().requires_grad_(True)
    ref = torch.stack([torch.cat([x[:, ctr], torch.bmm(F.softmax(torch.bmm(x[:, ctr], x[:, j].transpose(1, 2)) * temp, dim=2), x[:, j])], dim=2)
                       for j in others])
    (ref * w.double()).sum().backward()
    xd = clips.to(dev).requires_grad_(True)
    cat = CoAttentionWindow.apply(xd, ctr, temp)
    assert cat.shape == (t - 1, b, hw, 2 * c) and cat.is_contiguous()
    sum((cn * w[n].to(dev)).sum() for n, cn in enumerate(cat.unbind(0))).backward()
    _close(cat, ref.float(), 2e-5, "cat")
    _close(xd.grad, x.grad.float(), 5e-5, "d_clips")


def _window_setup(dev, size, b, t, seed):
    from dcnet_amd.utils.synth import synth_boxes, synth_inputs
    image, word_id, word_mask = synth_inputs(b * t, size, n_queries=b, seed=seed)
    return image, word_id, word_mask, synth_boxes(b, size, seed=seed)


def test_window_model_and_loss_match_the_oracle(dev):
    """The window model in train mode (size 256, B 2, T 3, fp32) through CoAttentionWindow: outputs within TOL of the oracle, and
    window_loss's three parts against the oracle's loss functions (oracle/train_oracle.py) on the ORACLE's outputs.
    Same inputs on both sides (window_loss on the oracle's outputs): the tolerance tests/test_losses_gpu.py holds these three losses to
    in that very comparison, 2e-5 relative to max(1, |ref|).  Measured on an MI355X: yolo 0, rank 1.5e-8, loc 4.8e-7 absolute.
    window_loss on the PRODUCT's own outputs sees inputs that differ from the oracle's by up to TOL per element, so no same-input
    tolerance applies; it is held to what test_train_forward_backward_matches_oracle holds the pair model's losses to in the same
    whole-path comparison, 2e-3 relative.  Measured: yolo 1.5e-3 of 26.5 (5.6e-5 relative), rank 2.2e-7, loc 2.7e-5 absolute."""
    from dcnet_amd import losses
    from oracle import dcnet_oracle as O
    from oracle import train_oracle as TO
    size, b, t = 256, 2, 3
    sd = synth_sd(size)
    image, word_id, word_mask, bbox = _window_setup(dev, size, b, t, 91)
    m = build_product(size, sd, dev, test_model=True).train()
    out = m(image.to(dev), word_id.to(dev), word_mask.to(dev), t)
    assert len(out) == 5
    outbox, sim, loc, corr, flang_attn = out
    with torch.no_grad():
        o = O.grounding_forward_nframe({k: v.clone() for k, v in sd.items()}, image, word_id, t, training=True)
    for s_ in range(3):
        assert maxdiff(outbox[s_], o["outbox"][s_]) < TOL and maxdiff(sim[s_], o["sim_score"][s_]) < TOL
        assert maxdiff(loc[s_], o["loc_score"][s_]) < TOL and maxdiff(corr[s_], o["corr_feat"][s_]) < TOL
    assert maxdiff(flang_attn.view(b, -1), o["flang_attn"].view(b, -1)) < TOL
    # the oracle's three dense losses on the oracle's outputs (train_oracle.total_loss without its two contrastive terms)
    box = torch.clamp(bbox, min=0, max=size - 1)
    gt_param, gi, gj, best_n, gt_center = TO.build_target(box, size)
    pred5 = [p.view(p.size(0), 3, 5, p.size(2), p.size(3)) for p in o["outbox"]]
    fa = o["flang_attn"].view(b, -1, 1, 1)
    neg = [torch.sum(fa.flip(0) * cf[:, :512], dim=1) for cf in o["corr_feat"]]
    ref = dict(yolo=TO.yolo_loss(pred5, gt_param, gi, gj, best_n), rank=TO.rank_loss(o["sim_score"], neg, gt_center),
               loc=TO.loc_loss(o["loc_score"], gt_center))
    ref_loss = ref["yolo"] + 100 * ref["rank"] + ref["loc"]
    on_oracle = ([x.to(dev) for x in o["outbox"]], [x.to(dev) for x in o["sim_score"]], [x.to(dev) for x in o["loc_score"]],
                 [x.to(dev) for x in o["corr_feat"]], fa.to(dev))
    for what, outputs, tol in (("oracle outputs", on_oracle, 2e-5), ("product outputs", out, 2e-3)):
        loss, parts = losses.window_loss(outputs, bbox.to(dev), size)
        assert sorted(parts) == ["loc", "rank", "yolo"]
        for k in parts:
            print(f"window_loss on {what}: {k} {float(parts[k].detach()):.8f} oracle {float(ref[k]):.8f} diff {abs(float(parts[k].detach()) - float(ref[k])):.3e}")
        for k in parts:
            got = float(parts[k].detach())
            assert abs(got - float(ref[k])) < tol * max(1.0, abs(float(ref[k]))), (what, k, got, float(ref[k]))
        assert abs(float(loss.detach()) - float(ref_loss)) < 5 * tol * max(1.0, abs(float(ref_loss))), (what, float(loss.detach()), float(ref_loss))
    loss.backward()
    g = next(iter(m.mapping_visu[0].parameters())).grad
    assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0, "no gradient reached the mapping through the window node"


def _step_setup(dev, size, b, t, seed):
    from dcnet_amd.parallel import freeze_gradless
    from dcnet_amd.train import make_optimizer
    m = build_product(size, synth_sd(size), dev, test_model=True)
    freeze_gradless(m)
    opt = make_optimizer(m, 1e-4)
    image, word_id, word_mask, bbox = (x.to(dev) for x in _window_setup(dev, size, b, t, seed))
    return m, opt, image, word_id, word_mask, bbox


def test_replayed_window_steps_equal_eager_window_steps_bitwise(dev):
    """Five window steps (size 256, B 2, n_frame 3), once eagerly (train.train_step(..., n_frame=3)) and once as one eager warm-up
    step + the captured pass + THREE replays, after the pattern of tests/test_graph_gpu.py: identical losses, and identical bits in a
    sample of parameters (mapping, corr_conv and its BatchNorm statistics, head, backbone) and in the optimiser state."""
    from dcnet_amd.graph import GraphedTrainStep
    from dcnet_amd.train import train_step
    size, b, t, steps = 256, 2, 3, 5
    m1, o1, image, word_id, word_mask, bbox = _step_setup(dev, size, b, t, 21)
    ref, ref_parts = [], None
    for _ in range(steps):
        loss, ref_parts = train_step(m1, o1, image, word_id, word_mask, bbox, size, n_frame=t)
        ref.append(float(loss))
    assert sorted(ref_parts) == ["loc", "rank", "yolo"]
    m2, o2, image, word_id, word_mask, bbox = _step_setup(dev, size, b, t, 21)
    step = GraphedTrainStep(m2, o2, image, word_id, word_mask, bbox, size, warmup=1, n_frame=t)   # steps 0 (eager) and 1 (captured pass)
    assert step.samples is None and not step.host_draws
    got = [None, float(step.loss)] + [float(step()) for _ in range(2, steps)]
    assert step.replays == 4                                    # the captured pass's own replay + three
    assert got[1:] == ref[1:], (got, ref)
    assert all(torch.isfinite(torch.tensor(ref)))
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    sample = [k for k in sd1 if k.startswith(("mapping_visu.0", "corr_conv.", "fcn_out.2", "visumodel.module_list.0.", "visumodel.module_list.74."))]
    assert len(sample) > 20
    for k in sample:
        assert torch.equal(sd1[k], sd2[k]), k
    s1, s2 = o1.state_dict()["state"], o2.state_dict()["state"]
    assert s1.keys() == s2.keys() and len(s1) > 100
    for k in s1:
        assert torch.equal(s1[k]["square_avg"], s2[k]["square_avg"]), k


def test_captured_window_step_in_bf16_storage(dev):
    """"bf16s": the captured window step runs, its loss and every gradient it left are finite, and its replay repeats an eager step's
    loss bit for bit in this mode too."""
    from dcnet_amd import ops
    from dcnet_amd.graph import GraphedTrainStep
    from dcnet_amd.train import train_step
    size, b, t = 256, 2, 3
    try:
        ops.set_precision("bf16s")
        m1, o1, image, word_id, word_mask, bbox = _step_setup(dev, size, b, t, 23)
        ref = [float(train_step(m1, o1, image, word_id, word_mask, bbox, size, n_frame=t)[0]) for _ in range(3)]
        m2, o2, image, word_id, word_mask, bbox = _step_setup(dev, size, b, t, 23)
        step = GraphedTrainStep(m2, o2, image, word_id, word_mask, bbox, size, warmup=1, n_frame=t)
        got = [float(step.loss), float(step())]
        torch.cuda.synchronize()
        grads = [p.grad for p in m2.parameters() if p.grad is not None]
    finally:
        ops.set_precision("fp32")
    assert all(torch.isfinite(torch.tensor(got))) and got == ref[1:], (got, ref)
    assert len(grads) > 150 and all(bool(torch.isfinite(g_).all()) for g_ in grads)
    assert any(float(g_.abs().max()) > 0 for g_ in grads)
