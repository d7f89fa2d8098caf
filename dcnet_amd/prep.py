"""Clip preprocessing: decoded uint8 frames -> the model's ``image`` / ``bbox`` tensors, pixel work on the device.

The reference does this per clip in ``ReferDataset.__getitem__`` (dataset/vid_loader.py:333-395) with cv2 on the CPU at full
source resolution: flip, HSV jitter, letterbox (utils/transforms.py:123-137), random affine (:139-185) and ``ToTensor`` +
``Normalize``.  Here the work splits in two:

  * host, float64 numpy like the reference: the random draws and the box geometry (flip, letterbox with the int truncation of
    the reference's int box arrays, ``M = S @ T @ R``, ``wrap_points``) — one function per step, no GPU needed;
  * device, ``csrc/prep.hip`` (``dcn_clip_prep``): every pixel of a whole batch in two launches, from one packed byte buffer
    and a table of per-frame ``DcnPrepJob`` records (include/dcnet_hip.h).

Random draws come from a caller-given ``random.Random`` (default: one owned by this module, seeded explicitly).  Python's
global ``random`` stream is never touched: the model's negative sampling advances that stream exactly like the reference
(INTEGRATION.md §1), and in the reference these draws run in DataLoader workers, not in the training process.

Decoding stays with the caller (PIL, cv2, a video decoder ...): ``prepare_clips`` takes uint8 RGB HWC numpy frames.
"""
from __future__ import annotations

import math
import random
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

MEAN = (0.485, 0.456, 0.406)              # train_DCNet.py:420-425
STD = (0.229, 0.224, 0.225)
PAD = (124, 116, 104)                     # saturate_cast<uchar>((123.7, 116.3, 103.5)): letterbox pad and warp border
DEGREES, TRANSLATE, SCALE, SHEAR = (-5, 5), (0.10, 0.10), (0.90, 1.10), (-2, 2)    # vid_loader.py:393-394, transforms.py:139

# the host image of DcnPrepJob (include/dcnet_hip.h): 96 bytes, field for field
JOB_DTYPE = np.dtype([("src_off", "<i8"), ("h", "<i4"), ("w", "<i4"), ("rh", "<i4"), ("rw", "<i4"), ("top", "<i4"),
                      ("left", "<i4"), ("flip", "<i4"), ("hsv", "<i4"), ("a_v", "<f4"), ("warp", "<i4"), ("minv", "<f8", (6,))])
assert JOB_DTYPE.itemsize == 96

_RNG = random.Random(20240607)            # the module's own generator (never Python's global one)


def default_rng() -> random.Random:
    return _RNG


# ---- host steps: draws and geometry (float64 numpy, like the reference) --------------------------------------------
def draw_flip(rng: random.Random) -> bool:
    """One draw per clip (vid_loader.py:351)."""
    return rng.random() > 0.5


def flip_box(box: np.ndarray, w: int) -> np.ndarray:
    """x1, x2 = w-1-x2, w-1-x1 on the int box (vid_loader.py:354); ``w`` is frame 0's width."""
    b = box.copy()
    b[0], b[2] = w - box[2] - 1, w - box[0] - 1
    return b


def swap_left_right(phrase: str) -> str:
    """'left' <-> 'right' through a placeholder (vid_loader.py:355)."""
    tmp = "*&^special^&*"
    return phrase.replace("right", tmp).replace("left", "right").replace(tmp, "left")


def draw_hsv(rng: random.Random) -> float:
    """Two draws per frame (vid_loader.py:364-368): the saturation factor (drawn, never used: S is only clipped) and the
    value factor a_V = (r*2-1)*0.5+1, which is returned."""
    rng.random()
    return (rng.random() * 2 - 1) * 0.50 + 1


@dataclass
class Letterbox:
    ratio: float
    rh: int
    rw: int
    dw: float
    dh: float
    top: int
    bottom: int
    left: int
    right: int


def letterbox_geometry(h: int, w: int, size: int) -> Letterbox:
    """transforms.py:123-137: ratio = size / max(h, w), content (round(w ratio), round(h ratio)) with Python's round,
    pads round(dh -+ 0.1) / round(dw -+ 0.1)."""
    ratio = float(size) / max(h, w)
    rw, rh = round(w * ratio), round(h * ratio)
    dw, dh = (size - rw) / 2, (size - rh) / 2
    return Letterbox(ratio, rh, rw, dw, dh, round(dh - 0.1), round(dh + 0.1), round(dw - 0.1), round(dw + 0.1))


def letterbox_box(box: np.ndarray, lb: Letterbox) -> np.ndarray:
    """x ratio + dw, y ratio + dh assigned back into the int box: truncation toward zero (vid_loader.py:379-380)."""
    b = box.copy()
    b[0], b[2] = box[0] * lb.ratio + lb.dw, box[2] * lb.ratio + lb.dw
    b[1], b[3] = box[1] * lb.ratio + lb.dh, box[3] * lb.ratio + lb.dh
    return b


def rotation_matrix_2d(cx: float, cy: float, angle: float, scale: float) -> np.ndarray:
    """The 2x3 matrix of OpenCV's documented getRotationMatrix2D (angle in degrees, counter-clockwise)."""
    t = angle * (math.pi / 180)
    al, be = math.cos(t) * scale, math.sin(t) * scale
    return np.array([[al, be, (1 - al) * cx - be * cy], [-be, al, be * cx + (1 - al) * cy]])


def draw_affine(rng: random.Random, size: int, degrees=DEGREES, translate=TRANSLATE, scale=SCALE, shear=SHEAR):
    """random_affine's six draws (angle, scale, tx, ty, shear-x, shear-y; transforms.py:143-163) on a size x size letterboxed
    frame.  Returns (M = S @ T @ R as 3x3 float64, the angle in degrees)."""
    R = np.eye(3)
    a = rng.random() * (degrees[1] - degrees[0]) + degrees[0]
    s = rng.random() * (scale[1] - scale[0]) + scale[0]
    R[:2] = rotation_matrix_2d(size / 2, size / 2, a, s)
    T = np.eye(3)
    T[0, 2] = (rng.random() * 2 - 1) * translate[0] * size + 0
    T[1, 2] = (rng.random() * 2 - 1) * translate[1] * size + 0
    Sh = np.eye(3)
    Sh[0, 1] = math.tan((rng.random() * (shear[1] - shear[0]) + shear[0]) * math.pi / 180)
    Sh[1, 0] = math.tan((rng.random() * (shear[1] - shear[0]) + shear[0]) * math.pi / 180)
    return Sh @ T @ R, a


def warp_box(box: np.ndarray, M: np.ndarray, size: int, angle: float) -> np.ndarray:
    """wrap_points (transforms.py:236-275): the four corners through M, their bounding box shrunk about its centre by
    sqrt(max(|sin a|, |cos a|)), clipped to [0, size].  float64 (4,)."""
    corners = np.ones((4, 3))
    corners[:, :2] = box[[0, 1, 2, 3, 0, 3, 2, 1]].reshape(4, 2)
    p = (corners @ M.T)[:, :2].reshape(1, 8)
    xs, ys = p[:, [0, 2, 4, 6]], p[:, [1, 3, 5, 7]]
    bb = np.concatenate((xs.min(1), ys.min(1), xs.max(1), ys.max(1))).reshape(4, 1).T
    red = max(abs(math.sin(angle * math.pi / 180)), abs(math.cos(angle * math.pi / 180))) ** 0.5
    cx, cy = (bb[:, 2] + bb[:, 0]) / 2, (bb[:, 3] + bb[:, 1]) / 2
    hw, hh = (bb[:, 2] - bb[:, 0]) * red, (bb[:, 3] - bb[:, 1]) * red
    out = np.concatenate((cx - hw / 2, cy - hh / 2, cx + hw / 2, cy + hh / 2)).reshape(4, 1).T
    np.clip(out, 0, size, out=out)
    return out[0]


@dataclass
class ClipPlan:
    """Host part of one clip: what the kernel needs per frame and the finished boxes."""
    flip: bool
    phrases: List[str]
    a_v: List[float]              # per frame (training), [] in evaluation
    lb: List[Letterbox]
    M: List[np.ndarray]           # per frame 3x3 (training), [] in evaluation
    angle: List[float]
    bbox: np.ndarray              # (T, 4) float32


def plan_clip(shapes: Sequence[Sequence[int]], boxes, phrases: Sequence[str], size: int, augment: bool,
              rng: random.Random) -> ClipPlan:
    """Draws and geometry of one clip, in the reference's draw order: flip (1), then (a_S, a_V) for every frame, then the six
    affine draws for every frame (vid_loader.py:347-395).  ``shapes``: (h, w) per frame; ``boxes``: (T, 4) x1y1x2y2 pixels
    (converted to the reference's int arrays)."""
    T = len(shapes)
    ib = [np.array(b, dtype=int) for b in boxes]
    ph = [p.lower() for p in phrases]
    flip = False
    a_v, Ms, angles = [], [], []
    lbs = [letterbox_geometry(int(h), int(w), size) for h, w in shapes]
    if augment:
        w0 = int(shapes[0][1])
        flip = draw_flip(rng)
        if flip:
            ib = [flip_box(b, w0) for b in ib]
            ph = [swap_left_right(p) for p in ph]
        for i in range(T):
            a_v.append(draw_hsv(rng))
            ib[i] = letterbox_box(ib[i], lbs[i])
        out = []
        for i in range(T):
            M, a = draw_affine(rng, size)
            Ms.append(M); angles.append(a)
            out.append(warp_box(ib[i], M, size, a))
        bbox = np.array(out, dtype=np.float32)
    else:
        bbox = np.array([letterbox_box(ib[i], lbs[i]) for i in range(T)], dtype=np.float32)
    return ClipPlan(flip, ph, a_v, lbs, Ms, angles, bbox)


def job_record(jobs: np.ndarray, i: int, src_off: int, h: int, w: int, lb: Letterbox, flip: bool,
               a_v: Optional[float], M: Optional[np.ndarray]) -> None:
    j = jobs[i]
    j["src_off"], j["h"], j["w"], j["rh"], j["rw"], j["top"], j["left"] = src_off, h, w, lb.rh, lb.rw, lb.top, lb.left
    j["flip"] = int(flip)
    j["hsv"] = int(a_v is not None)
    j["a_v"] = np.float32(a_v if a_v is not None else 1.0)
    j["warp"] = int(M is not None)
    j["minv"] = np.linalg.inv(M)[:2].reshape(6) if M is not None else np.array([1.0, 0, 0, 0, 1.0, 0])


@dataclass
class Plan:
    jobs: np.ndarray              # (n,) JOB_DTYPE
    src_bytes: int                # packed source bytes (frames at 256-byte aligned offsets)
    bbox: np.ndarray              # (n, 4) float32
    phrases: List[List[str]]
    ratio: np.ndarray             # (n,) float32
    dw: np.ndarray
    dh: np.ndarray
    clips: List[ClipPlan]


def _align(v: int, a: int = 256) -> int:
    return (v + a - 1) // a * a


def plan_batch(frames, boxes, phrases, size: int, augment: bool, rng: Optional[random.Random] = None) -> Plan:
    """Host part of ``prepare_clips`` (no GPU): the job table, the packed layout and the finished boxes / phrases / letterbox
    meta of a batch of clips, clip by clip in order (one ``__getitem__`` after the other)."""
    if size <= 0 or size % 32:
        raise ValueError(f"prep: size {size} must be a positive multiple of 32")
    rng = _RNG if rng is None else rng
    if rng is random or rng is getattr(random, "_inst", None):
        raise ValueError("prep: pass a random.Random instance, not Python's global generator")
    n = sum(len(c) for c in frames)
    jobs = np.zeros(n, dtype=JOB_DTYPE)
    clips, off, i = [], 0, 0
    for ci, clip in enumerate(frames):
        shapes = []
        for f in clip:
            if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
                raise ValueError(f"prep: clip {ci}: frames must be uint8 HWC RGB, got {f.dtype} {f.shape}")
            shapes.append(f.shape[:2])
        if len(boxes[ci]) != len(clip) or len(phrases[ci]) != len(clip):
            raise ValueError(f"prep: clip {ci}: {len(clip)} frames, {len(boxes[ci])} boxes, {len(phrases[ci])} phrases")
        cp = plan_clip(shapes, boxes[ci], phrases[ci], size, augment, rng)
        for t, (h, w) in enumerate(shapes):
            job_record(jobs, i, off, h, w, cp.lb[t], cp.flip, cp.a_v[t] if augment else None, cp.M[t] if augment else None)
            off = _align(off + h * w * 3)
            i += 1
        clips.append(cp)
    lbs = [lb for c in clips for lb in c.lb]
    return Plan(jobs, off, np.concatenate([c.bbox for c in clips]).reshape(n, 4), [c.phrases for c in clips],
                np.array([l.ratio for l in lbs], dtype=np.float32), np.array([l.dw for l in lbs], dtype=np.float32),
                np.array([l.dh for l in lbs], dtype=np.float32), clips)


# ---- device part ------------------------------------------------------------------------------------------------------
@dataclass
class Prepared:
    image: "object"               # (n, 3, size, size) fp32 CUDA tensor
    bbox: "object"                # (n, 4) fp32 CUDA tensor
    bbox_host: np.ndarray         # the same boxes on the host
    phrases: List[List[str]]      # lower-cased, left/right swapped where the clip was flipped
    ratio: np.ndarray             # (n,) float32 letterbox meta (evaluation un-letterboxes with it)
    dw: np.ndarray
    dh: np.ndarray
    jobs: np.ndarray = None           # the (n,) JOB_DTYPE table that was run
    letterbox_u8: "object" = None     # debug=True: (n, size, size, 4) uint8 RGBx letterbox stage
    warped_u8: "object" = None        # debug=True: (n, size, size, 3) uint8 warped stage


class _Stager:
    """A ring of page-locked staging buffers and their device twins.  The host packs call k+1 while the device still runs
    call k; a slot is rewritten on the host only after the copy that last read it has run (its event), and on the device
    only after the kernels that last read it have run (the copy stream waits for their event) — the ``optim.RMSprop.sync_lr``
    discipline, for bytes."""
    RING = 2

    def __init__(self, device):
        import torch
        self.device = device
        self.copy_stream = torch.cuda.Stream(device=device)
        self.slots = [{"pinned": None, "dev": None, "copied": None, "used": None} for _ in range(self.RING)]
        self.next = 0

    def slot(self, nbytes: int):
        import torch
        s = self.slots[self.next]
        self.next = (self.next + 1) % self.RING
        if s["copied"] is not None:
            s["copied"].synchronize()            # the last copy out of this pinned buffer has run
        if s["pinned"] is None or s["pinned"].numel() < nbytes:
            if s["used"] is not None:
                s["used"].synchronize()          # the device twin is about to be freed: its last readers must have run
            cap = _align(int(nbytes * 1.25), 1 << 20)
            s["pinned"] = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
            s["dev"] = torch.empty(cap, dtype=torch.uint8, device=self.device)
        return s


_stagers = {}


def prepare_clips(frames, boxes, phrases, size: int, augment: bool, rng: Optional[random.Random] = None, out=None,
                  stream=None, debug: bool = False) -> Prepared:
    """A batch of clips -> model input, in one ``dcn_clip_prep`` call (two launches).

    frames   list of clips, each a list of T uint8 (h, w, 3) RGB numpy frames (any sizes)
    boxes    list of clips, each (T, 4) x1y1x2y2 source pixels
    phrases  list of clips, each T strings
    augment  True: training (flip, HSV, letterbox, affine); False: evaluation (letterbox only)
    rng      random.Random of the draws (default: the module's own); Python's global ``random`` is never used
    out      an existing contiguous (n, 3, size, size) fp32 CUDA tensor to write (e.g. ``GraphedTrainStep.image``)
    stream   torch.cuda.Stream to order the work on (default: the current stream); nothing synchronises the host

    Returns ``Prepared``: image, bbox (device), bbox_host, phrases, ratio / dw / dh (float32, per frame)."""
    return run_plan(plan_batch(frames, boxes, phrases, size, augment, rng), frames, size, out, stream, debug)


def run_plan(plan: Plan, frames, size: int, out=None, stream=None, debug: bool = False) -> Prepared:
    """The device half of ``prepare_clips`` for a plan made by ``plan_batch`` (whose job table a caller may adjust first)."""
    import torch
    from .lib import lib
    n = len(plan.jobs)
    dev = out.device if out is not None else torch.device("cuda", torch.cuda.current_device())
    stream = stream if stream is not None else torch.cuda.current_stream(dev)
    if out is not None and not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
                                and tuple(out.shape) == (n, 3, size, size)):
        raise ValueError(f"prep: out must be a contiguous fp32 CUDA tensor of shape {(n, 3, size, size)}")
    st = _stagers.get(dev.index)
    if st is None:
        st = _stagers[dev.index] = _Stager(dev)
    jb, bb = n * JOB_DTYPE.itemsize, n * 16
    o_box = _align(jb)
    o_src = _align(o_box + bb)
    total = o_src + plan.src_bytes
    slot = st.slot(total)
    host = slot["pinned"].numpy()
    host[:jb] = plan.jobs.view(np.uint8)
    host[o_box:o_box + bb] = plan.bbox.view(np.uint8).reshape(-1)
    i = 0
    for clip in frames:
        for f in clip:
            off = int(plan.jobs[i]["src_off"])
            host[o_src + off:o_src + off + f.size] = np.ascontiguousarray(f).reshape(-1)
            i += 1
    with torch.cuda.stream(stream):
        image = out if out is not None else torch.empty((n, 3, size, size), dtype=torch.float32, device=dev)
        ws = torch.empty(int(lib().clip_prep_ws(n, size)), dtype=torch.uint8, device=dev)
        u8 = torch.empty((n, size, size, 3), dtype=torch.uint8, device=dev) if debug else None
        bbox = torch.empty((n, 4), dtype=torch.float32, device=dev)
    if slot["used"] is not None:
        st.copy_stream.wait_event(slot["used"])          # the kernels that last read the device twin have run
    with torch.cuda.stream(st.copy_stream):
        slot["dev"][:total].copy_(slot["pinned"][:total], non_blocking=True)
        copied = torch.cuda.Event()
        copied.record(st.copy_stream)
    stream.wait_event(copied)
    d = slot["dev"]
    base = d.data_ptr()
    with torch.cuda.stream(stream):
        bbox.copy_(d[o_box:o_box + bb].view(torch.float32).view(n, 4))
    lib().clip_prep(base + o_src, plan.src_bytes, base, plan.jobs.ctypes.data, n, size, ws.data_ptr(), image.data_ptr(),
                    u8.data_ptr() if u8 is not None else None, stream.cuda_stream)
    used = torch.cuda.Event()
    used.record(stream)
    slot["copied"], slot["used"] = copied, used
    return Prepared(image, bbox, plan.bbox, plan.phrases, plan.ratio, plan.dw, plan.dh, plan.jobs,
                    ws.view(n, size, size, 4) if debug else None, u8)
