"""CPU: the host half of clip preprocessing (dcnet_amd/prep.py) against the reference's ReferDataset.__getitem__, recorded
through cv2 stubs by tools/make_prep_goldens.py (tests/golden/prep_geometry.json): same seeds -> the same flip flags, swapped
phrases, V planes, resize targets, pads, affine matrices and boxes, floats compared bitwise.  Also: Python's global ``random``
is never touched, the pixel spec's restatement agrees with itself on trivial cases, and the C entry point rejects bad
arguments before it launches anything."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

from util import ROOT

import prep_np as R

GOLD = os.path.join(ROOT, "tests", "golden", "prep_geometry.json")


def _cases():
    with open(GOLD) as fh:
        return json.load(fh)["cases"]


@pytest.mark.parametrize("case", _cases(), ids=lambda c: f"seed{c['seed']}_{'train' if c['augment'] else 'eval'}_T{len(c['shapes'])}")
def test_draws_and_geometry_match_the_reference(case):
    from dcnet_amd import prep
    rng = random.Random(case["seed"])
    S = case["size"]
    cp = prep.plan_clip(case["shapes"], case["boxes"], case["phrases"], S, case["augment"], rng)
    T = len(case["shapes"])
    # the same number of draws from the same MT19937 stream
    ref = random.Random(case["seed"])
    for _ in range(case["draws"]):
        ref.random()
    assert rng.getstate() == ref.getstate()
    assert cp.flip == case["flip"] and case["flip_calls"] == ([1] * T if cp.flip else [])
    assert cp.phrases == case["tokenized"]
    # letterbox: resize target (w, h) with INTER_AREA, pads, pad colour
    assert [[l.rw, l.rh, 3] for l in cp.lb] == case["resize"]
    for l, (top, bottom, left, right, value) in zip(cp.lb, case["border"]):
        assert (l.top, l.bottom, l.left, l.right) == (top, bottom, left, right)
        assert tuple(int(np.clip(np.rint(v), 0, 255)) for v in value) == prep.PAD
    assert np.array(case["ratio"], np.float32).tobytes() == np.array([l.ratio for l in cp.lb], np.float32).tobytes()
    assert np.array(case["dw"], np.float32).tobytes() == np.array([l.dw for l in cp.lb], np.float32).tobytes()
    assert np.array(case["dh"], np.float32).tobytes() == np.array([l.dh for l in cp.lb], np.float32).tobytes()
    if case["augment"]:
        # V' = trunc(float32(V) * float32(a_V)) for V = 0 ... 255: pins the draw and the rule
        assert len(cp.a_v) == T == len(case["vplanes"])
        for a, vp in zip(cp.a_v, case["vplanes"]):
            assert R.scale_v(np.arange(256), a).tolist() == vp
        assert len(case["warp"]) == T
        for M, a, w, rot in zip(cp.M, cp.angle, case["warp"], case["rot"]):
            assert np.array(w["M"]).tobytes() == M.tobytes()
            assert w["dsize"] == [S, S] and w["flags"] == 1 and w["border"] == [123.7, 116.3, 103.5]
            assert rot[:2] == [S / 2, S / 2] and rot[2] == a
    else:
        assert not cp.a_v and not cp.M and case["vplanes"] == [] and case["warp"] == []
    assert np.array(case["bbox"], np.float32).tobytes() == cp.bbox.tobytes()


def test_fixture_covers_the_contract():
    cases = _cases()
    assert {len(c["shapes"]) for c in cases} == {2, 5, 8}
    assert any(c["flip"] for c in cases) and any(c["augment"] and not c["flip"] for c in cases)
    assert any(not c["augment"] for c in cases)
    aug = [a for c in cases for a in c["vplanes"]]
    assert any(v[255] > 255 * 0.99 for v in aug) and any(v[255] < 200 for v in aug)        # a_V > 1 (saturating) and < 1


def _batch(rng_np, T=3, sizes=((720, 1280), (375, 500))):
    frames = [[rng_np.randint(0, 256, size=(*sizes[(c + t) % len(sizes)], 3), dtype=np.uint8) for t in range(T)] for c in range(2)]
    boxes = [[[10, 20, 100, 200]] * T for _ in range(2)]
    phrases = [["the left one"] * T for _ in range(2)]
    return frames, boxes, phrases


def test_global_random_is_untouched(monkeypatch):
    """The host part of prepare_clips draws from its own generator only: the global stream's state is unchanged, and a global
    ``random.random`` that raises is never called."""
    from dcnet_amd import prep
    frames, boxes, phrases = _batch(np.random.RandomState(0))
    random.seed(1234)
    before = random.getstate()

    def boom(*a, **k):
        raise AssertionError("global random used")

    for name in ("random", "uniform", "randint", "choice", "shuffle", "sample", "seed"):
        monkeypatch.setattr(random, name, boom)
    p1 = prep.plan_batch(frames, boxes, phrases, 416, True)                       # the module's own generator
    p2 = prep.plan_batch(frames, boxes, phrases, 416, True, rng=random.Random(5))
    monkeypatch.undo()
    assert random.getstate() == before
    assert len(p1.jobs) == len(p2.jobs) == 6
    with pytest.raises(ValueError):
        prep.plan_batch(frames, boxes, phrases, 416, True, rng=random._inst)


def test_phrase_swap_and_letterbox_padding():
    from dcnet_amd import prep
    assert prep.swap_left_right("the left dog right of the leftmost") == "the right dog left of the rightmost"
    # odd padding: the extra row goes to the bottom / right; even padding is symmetric; content + pads == size
    for h, w, S in ((375, 500, 416), (720, 1280, 416), (500, 375, 608), (100, 100, 256), (233, 911, 416)):
        lb = prep.letterbox_geometry(h, w, S)
        assert lb.top + lb.rh + lb.bottom == S and lb.left + lb.rw + lb.right == S
        assert lb.bottom - lb.top in (0, 1) and lb.right - lb.left in (0, 1)
    lb = prep.letterbox_geometry(375, 500, 416)           # rh = 312: dh = 52.0
    assert (lb.rw, lb.rh, lb.top, lb.bottom, lb.left, lb.right) == (416, 312, 52, 52, 0, 0)
    lb = prep.letterbox_geometry(720, 1280, 416)          # rh = 234: dh = 91.0
    assert (lb.rh, lb.top, lb.bottom) == (234, 91, 91)
    lb = prep.letterbox_geometry(233, 911, 416)           # rh = round(106.4) = 106: dh = 155.0
    assert (lb.rh, lb.top, lb.bottom) == (106, 155, 155)
    lb = prep.letterbox_geometry(300, 911, 416)           # rh = round(136.99) = 137: dh = 139.5 -> 139 / 140
    assert (lb.rh, lb.top, lb.bottom) == (137, 139, 140)


def test_eval_meta_and_boxes():
    from dcnet_amd import prep
    from dcnet_amd.postprocess import letterbox_frame
    frames = [[np.zeros((375, 500, 3), np.uint8), np.zeros((720, 1280, 3), np.uint8)]]
    p = prep.plan_batch(frames, [[[10, 20, 110, 220], [0, 0, 1279, 719]]], [["Left", "right"]], 416, False)
    assert p.ratio.dtype == np.float32 and p.ratio.tolist() == [np.float32(416 / 500), np.float32(416 / 1280)]
    assert p.dw.tolist() == [0.0, 0.0] and p.dh.tolist() == [52.0, 91.0]
    assert p.phrases == [["left", "right"]]                                        # lower-cased, no swap in evaluation
    # int truncation of x * ratio + d: 10 * 0.832 = 8.32 -> 8, 20 * 0.832 + 52 = 68.64 -> 68 ...
    assert p.bbox[0].tolist() == [8.0, 68.0, 91.0, 235.0]
    for r, dw, dh, hw in zip(p.ratio, p.dw, p.dh, ((375, 500), (720, 1280))):
        assert letterbox_frame(416, float(r), float(dw), float(dh)) == hw         # postprocess un-letterboxes to the source
    assert p.jobs["warp"].tolist() == [0, 0] and p.jobs["hsv"].tolist() == [0, 0] and p.jobs["flip"].tolist() == [0, 0]
    assert p.jobs["src_off"][1] % 256 == 0 and p.jobs["src_off"][1] >= 375 * 500 * 3


def test_restatement_sanity():
    """The numpy restatement on cases with known answers: same-size resize is the identity, a constant frame stays constant
    under downscale, HSV with a_V = 1 changes grey pixels not at all, the identity warp is the identity."""
    rs = np.random.RandomState(1)
    img = rs.randint(0, 256, size=(40, 64, 3)).astype(np.uint8)
    assert np.array_equal(R.resize_area_down(img, 40, 64), img)
    assert np.array_equal(R.resize_area_down(np.full((90, 160, 3), 77, np.uint8), 27, 48), np.full((27, 48, 3), 77))
    assert np.array_equal(R.resize_area_up(np.full((30, 40, 3), 9, np.uint8), 45, 60), np.full((45, 60, 3), 9))
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)[None]
    assert np.array_equal(R.hsv_adjust(grey, 1.0), grey)
    x = R.hsv_adjust(grey, 0.5)
    assert np.array_equal(x[0, :, 0], np.arange(256) // 2)
    from dcnet_amd import prep
    job = np.zeros(1, prep.JOB_DTYPE)[0]
    job["warp"] = 1
    job["minv"] = [1, 0, 0, 0, 1, 0]
    lb = rs.randint(0, 256, size=(32, 32, 3)).astype(np.uint8)
    assert np.array_equal(R.warp_u8(lb, job), lb)
    n = R.normalize(lb)
    assert n.shape == (3, 32, 32) and n.dtype == np.float32


def test_c_entry_rejects_bad_arguments():
    """Validation happens on the host copy of the job table before anything is launched (so this runs without a GPU)."""
    from dcnet_amd import prep
    from dcnet_amd.lib import DcnError, lib
    L = lib()
    p = prep.plan_batch([[np.zeros((375, 500, 3), np.uint8)]], [[[1, 2, 3, 4]]], [["x"]], 416, False)
    jobs = p.jobs.copy()
    fake = 4096                                         # never dereferenced: every call below fails validation first
    assert L.clip_prep_ws(3, 416) == 3 * 416 * 416 * 4

    def call(jobs, n=1, size=416, src_bytes=p.src_bytes):
        L.clip_prep(fake, src_bytes, fake, jobs.ctypes.data, n, size, fake, fake, None, None)

    with pytest.raises(DcnError, match="multiple of 32"):
        call(jobs, size=400)
    with pytest.raises(DcnError, match="bad batch"):
        call(jobs, n=0)
    with pytest.raises(DcnError, match="outside the source buffer"):
        call(jobs, src_bytes=375 * 500 * 3 - 1)
    bad = jobs.copy(); bad["h"] = 0
    with pytest.raises(DcnError, match="bad frame size"):
        call(bad)
    bad = jobs.copy(); bad["src_off"] = 256
    with pytest.raises(DcnError, match="outside the source buffer"):
        call(bad)
    bad = jobs.copy(); bad["top"] = 200
    with pytest.raises(DcnError, match="does not fit"):
        call(bad)
    with pytest.raises(DcnError, match="null"):
        L.clip_prep(None, p.src_bytes, fake, jobs.ctypes.data, 1, 416, fake, fake, None, None)
    assert ctypes.sizeof(ctypes.c_void_p) == 8
