"""GPU: clip preprocessing (csrc/prep.hip dcn_clip_prep through dcnet_amd.prep) against the numpy restatement of its pixel
spec (tests/prep_np.py), batching, and the hand-off to a captured training step."""
import random

import numpy as np
import pytest
import torch

import prep_np as R

pytestmark = pytest.mark.gpu


def _frame(rs, h, w):
    """Noise over smooth gradients: every HSV sector, grey pixels, saturated and dark values."""
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    base = np.stack([xx * 255, yy * 255, (1 - xx) * yy * 255], -1)
    img = base + rs.randint(-60, 61, size=(h, w, 3))
    img[: h // 8] = rs.randint(0, 256, size=(h // 8, w, 1))                 # grey rows (S = 0)
    img[h // 8: h // 4, : w // 3] = 250 + rs.randint(0, 6, size=(h // 4 - h // 8, w // 3, 3))   # bright: saturates for a_V > 1
    return np.clip(img, 0, 255).astype(np.uint8)


def _compare_stages(res, frames, S):
    lb_k = res.letterbox_u8.cpu().numpy()[..., :3]
    wp_k = res.warped_u8.cpu().numpy()
    img = res.image.cpu().numpy()
    flat = [f for clip in frames for f in clip]
    for i, (f, job) in enumerate(zip(flat, res.jobs)):
        want = R.letterbox_u8(f, job, S)
        d = np.abs(want.astype(np.int64) - lb_k[i].astype(np.int64))
        down = f.shape[0] >= job["rh"] and f.shape[1] >= job["rw"]
        if down:          # INTER_AREA downscale: <= 1 LSB on <= 0.1 % of values (fp32 summation order)
            assert d.max() <= 1 and (d > 0).mean() <= 1e-3, (i, d.max(), (d > 0).mean())
        else:
            assert d.max() == 0, (i, d.max())
        assert np.array_equal(R.warp_u8(lb_k[i], job), wp_k[i]), i
        assert R.normalize(wp_k[i]).tobytes() == img[i].tobytes(), i


def test_kernel_matches_the_restatement(dev):
    from dcnet_amd import prep
    rs = np.random.RandomState(0)
    S = 416
    # non-integer downscale, exact 2x downscale, same size, portrait, landscape, a 4:3 frame
    shapes = [(720, 1280), (832, 600), (234, 416), (640, 360), (375, 500), (601, 517)]
    frames = [[_frame(rs, h, w) for h, w in shapes[:3]], [_frame(rs, h, w) for h, w in shapes[3:]]]
    boxes = [[[5, 6, 50, 60]] * 3, [[5, 6, 50, 60]] * 3]
    plan = prep.plan_batch(frames, boxes, [["a"] * 3, ["b"] * 3], S, True, rng=random.Random(11))
    J = plan.jobs
    J["flip"] = [1, 0, 1, 0, 1, 0]
    J["a_v"] = np.array([0.55, 1.45, 1.0, 1.3, 0.8, 1.49], np.float32)
    # a warp that reaches far past the border: scale 0.7 about the centre + shift
    M = np.array([[0.7, 0.05, 80.0], [-0.04, 0.7, 40.0], [0, 0, 1.0]])
    J["minv"][3] = np.linalg.inv(M)[:2].reshape(6)
    res = prep.run_plan(plan, frames, S, debug=True)
    torch.cuda.synchronize()
    _compare_stages(res, frames, S)
    wp = res.warped_u8.cpu().numpy()
    assert (wp[3] == np.array(prep.PAD, np.uint8)).all(-1).mean() > 0.1            # the border shows
    # the same frames in evaluation mode (letterbox only, no flip, no HSV) and an upscale to 608
    ev = prep.prepare_clips(frames, boxes, [["a"] * 3, ["b"] * 3], S, False, debug=True)
    torch.cuda.synchronize()
    _compare_stages(ev, frames, S)
    up = [[_frame(rs, 375, 500), _frame(rs, 500, 375)]]
    for aug in (False, True):
        r = prep.prepare_clips(up, [[[1, 2, 30, 40]] * 2], [["c", "d"]], 608, aug, rng=random.Random(3), debug=True)
        torch.cuda.synchronize()
        assert int(r.jobs["rw"][0]) == 608 and int(r.jobs["rh"][1]) == 608
        _compare_stages(r, up, 608)


def test_ragged_batch_equals_per_clip_calls(dev):
    """256 frames of four sizes in ONE call == 32 per-clip calls (same draws), and == per-clip calls through out= slices."""
    from dcnet_amd import prep
    rs = np.random.RandomState(5)
    S, B, T = 256, 32, 8
    sizes = [(360, 640), (375, 500), (240, 320), (500, 375)]
    frames = [[rs.randint(0, 256, size=(*sizes[(c + t) % 4], 3), dtype=np.uint8) for t in range(T)] for c in range(B)]
    boxes = [[[10, 10, 100, 120]] * T for _ in range(B)]
    phrases = [["the left cat"] * T for _ in range(B)]
    whole = prep.prepare_clips(frames, boxes, phrases, S, True, rng=random.Random(7))
    assert whole.image.shape == (B * T, 3, S, S) and whole.bbox.shape == (B * T, 4)
    rng = random.Random(7)
    big = torch.full((B * T, 3, S, S), float("nan"), device=dev)
    parts, boxes_dev = [], []
    for c in range(B):
        parts.append(prep.prepare_clips(frames[c:c + 1], boxes[c:c + 1], phrases[c:c + 1], S, True, rng=rng).image)
    rng = random.Random(7)
    for c in range(B):
        r = prep.prepare_clips(frames[c:c + 1], boxes[c:c + 1], phrases[c:c + 1], S, True, rng=rng, out=big[c * T:(c + 1) * T])
        assert r.image.data_ptr() == big[c * T].data_ptr()
        boxes_dev.append(r.bbox)
    torch.cuda.synchronize()
    assert torch.equal(whole.image, torch.cat(parts))
    assert torch.equal(whole.image, big)
    assert torch.equal(whole.bbox, torch.cat(boxes_dev))
    assert torch.equal(whole.bbox.cpu(), torch.from_numpy(whole.bbox_host))


def test_captured_step_fed_through_out_equals_copy(dev):
    """A GraphedTrainStep whose static image is written by prepare_clips(out=step.image) on the step's stream gives bitwise the
    losses of the same step fed by copy_ of the same tensors: the preprocessing is ordered before each replay."""
    from dcnet_amd import prep
    from dcnet_amd.graph import GraphedTrainStep
    from dcnet_amd.parallel import freeze_gradless
    from dcnet_amd.train import make_optimizer
    from dcnet_amd.utils.synth import synth_boxes, synth_inputs
    from util import build_product, synth_sd
    size, B, T, steps = 256, 2, 2, 3
    n = B * T
    rs = np.random.RandomState(9)
    batches = []
    for k in range(steps):
        frames = [[rs.randint(0, 256, size=(*((360, 640) if (c + t + k) % 2 else (375, 500)), 3), dtype=np.uint8) for t in range(T)]
                  for c in range(B)]
        batches.append((frames, [[[20, 30, 200, 300]] * T] * B, [["a dog on the left"] * T] * B))

    def run(feed_out):
        m = build_product(size, synth_sd(size), dev)
        freeze_gradless(m)
        opt = make_optimizer(m, 1e-4)
        image, word_id, word_mask = (t.to(dev) for t in synth_inputs(n, size, seed=4))
        bbox = synth_boxes(n, size, seed=4).to(dev)
        random.seed(99)
        step = GraphedTrainStep(m, opt, image, word_id, word_mask, bbox, size, warmup=1)
        losses = []
        for k, (frames, boxes, phrases) in enumerate(batches):
            if feed_out:
                r = prep.prepare_clips(frames, boxes, phrases, size, True, rng=random.Random(k), out=step.image)
                step.bbox.copy_(r.bbox)
            else:
                r = prep.prepare_clips(frames, boxes, phrases, size, True, rng=random.Random(k))
                torch.cuda.synchronize()
                img, box = r.image.clone(), r.bbox.clone()
                step.image.copy_(img)
                step.bbox.copy_(box)
            losses.append(float(step()))
        return losses

    a = run(True)
    b = run(False)
    assert a == b, (a, b)
    assert all(np.isfinite(a))
