"""Pin dcnet_amd/prep.py's draws and box geometry to the REAL reference and write tests/golden/prep_geometry.json.

Runs only where the reference checkout exists (like oracle/make_goldens.py), never on the GPU box:

    python tools/make_prep_goldens.py

``ReferDataset.__getitem__`` (dataset/vid_loader.py:333-440) is driven on a bare instance (``object.__new__``, fields set by
hand, ``lstm=True`` with a stub corpus whose ``tokenize`` records the phrase and returns fixed ids) for seeded clips of varied
source sizes and T in {2, 5, 8}, in both modes.  cv2 is replaced by RECORDING stubs: they log what the reference hands them
(flip calls, the V plane given back to HSV->BGR, resize targets, border widths / values, the rotation-matrix arguments, the M
and dsize of warpPerspective) and return blank images of the right shape; ``getRotationMatrix2D`` computes OpenCV's
documented formula.  The remaining import shells are oracle/make_goldens.py's.  Python's global ``random``
is seeded per clip and its ``random()`` is wrapped to count the draws.

The fixture holds data only (seeds, shapes, boxes, phrases and the recorded values); no reference text.
"""
from __future__ import annotations

import json
import math
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "prep_geometry.json")

# (seed, augment, size, frame sizes (h, w) of the clip): varied sources, T in {2, 5, 8}, portrait / landscape, up and down
CASES = []
_SIZES = [(720, 1280), (375, 500), (500, 375), (416, 234), (480, 640), (1080, 1920), (333, 517), (600, 600), (233, 911), (300, 200)]
for k in range(20):
    T = (2, 5, 8)[k % 3]
    size = (416, 256, 608)[k % 3] if k % 4 else 416
    hw = _SIZES[k % len(_SIZES)]
    frames = [hw] * T if k % 5 else [hw if t % 2 == 0 else _SIZES[(k + 3) % len(_SIZES)] for t in range(T)]
    CASES.append((1000 + k, bool(k % 2 == 0 or k % 7 == 3), size, frames))

PHRASES = ["the Left dog", "a cat on the right", "Right and left", "red car", "the leftmost bird on the right of it"]


def _box(rs: np.random.RandomState, h: int, w: int):
    x1, y1 = int(rs.randint(0, w // 2)), int(rs.randint(0, h // 2))
    return [x1, y1, int(rs.randint(x1 + 1, w)), int(rs.randint(y1 + 1, h))]


def main():
    from oracle import make_goldens as MG
    MG._import_reference()
    import cv2
    rec = {}

    def imread(path):
        h, w = rec["shapes"][int(os.path.basename(path).split(".")[0])]
        return np.zeros((h, w, 3), dtype=np.uint8)

    def cvtColor(img, code):
        if code == cv2.COLOR_BGR2HSV:
            hsv = np.zeros(img.shape, dtype=np.uint8)
            hsv[..., 2].reshape(-1)[:256] = np.arange(256)          # V = 0 ... 255 in the first 256 pixels
            return hsv
        if code == cv2.COLOR_HSV2BGR:
            rec["vplanes"].append([int(v) for v in img[..., 2].reshape(-1)[:256]])
        return img.copy()

    def flip(img, code):
        rec["flips"].append(int(code))
        return img[:, ::-1].copy()

    def resize(img, shape, interpolation=None):
        rec["resize"].append([int(shape[0]), int(shape[1]), int(interpolation)])
        return np.zeros((shape[1], shape[0], 3), dtype=np.uint8)

    def copyMakeBorder(img, top, bottom, left, right, border, value=None):
        rec["border"].append([int(top), int(bottom), int(left), int(right), [float(v) for v in value]])
        return np.zeros((img.shape[0] + top + bottom, img.shape[1] + left + right, 3), dtype=np.uint8)

    def getRotationMatrix2D(center, angle, scale):        # OpenCV's documented formula
        rec["rot"].append([float(center[0]), float(center[1]), float(angle), float(scale)])
        t = angle * (math.pi / 180)
        al, be = math.cos(t) * scale, math.sin(t) * scale
        return np.array([[al, be, (1 - al) * center[0] - be * center[1]], [-be, al, be * center[0] + (1 - al) * center[1]]])

    def warpPerspective(img, M, dsize, flags=None, borderValue=None):
        rec["warp"].append({"M": [[float(v) for v in row] for row in M], "dsize": [int(d) for d in dsize],
                            "flags": int(flags), "border": [float(v) for v in borderValue]})
        return np.zeros((dsize[1], dsize[0], 3), dtype=np.uint8)

    consts = dict(COLOR_BGR2RGB=4, COLOR_RGB2BGR=4, COLOR_BGR2HSV=40, COLOR_HSV2BGR=54, INTER_AREA=3, INTER_LINEAR=1,
                  INTER_NEAREST=0, BORDER_CONSTANT=0)
    cv2.__dict__.update(consts, imread=imread, cvtColor=cvtColor, flip=flip, resize=resize, copyMakeBorder=copyMakeBorder,
                        getRotationMatrix2D=getRotationMatrix2D, warpPerspective=warpPerspective)
    import torch
    from dataset import vid_loader as VL                     # the reference's loader module
    assert VL.__file__.startswith(MG.REF), VL.__file__

    class Corpus:
        def tokenize(self, phrase, max_len):
            rec["tokenized"].append(phrase)
            return [1] * max_len

    real_random = random.random

    def counted():
        rec["draws"] += 1
        return real_random()

    out = []
    for seed, augment, size, shapes in CASES:
        T = len(shapes)
        rs = np.random.RandomState(seed)
        boxes = [_box(rs, h, w) for h, w in shapes]
        phrases = [PHRASES[(seed + t) % len(PHRASES)] for t in range(T)]
        ds = object.__new__(VL.ReferDataset)
        ds.dataset, ds.im_dir, ds.imsize, ds.query_len, ds.lstm = "VID", "", size, 20, True
        ds.corpus, ds.augment, ds.testmode, ds.num_frame_k = Corpus(), augment, True, T
        ds.transform = lambda im: torch.from_numpy(np.ascontiguousarray(im))
        ds.images = [([f"{t}.JPEG" for t in range(T)], [list(b) for b in boxes], list(phrases))]
        rec.clear()
        rec.update(shapes=shapes, vplanes=[], flips=[], resize=[], border=[], rot=[], warp=[], tokenized=[], draws=0)
        random.seed(seed)
        random.random = counted
        try:
            _, _, _, bbox, ratio, dw, dh, _, ori = ds[0]
        finally:
            random.random = real_random
        out.append({"seed": seed, "augment": augment, "size": size, "shapes": [list(s) for s in shapes], "boxes": boxes,
                    "phrases": phrases, "flip": len(rec["flips"]) > 0, "flip_calls": rec["flips"], "tokenized": rec["tokenized"],
                    "vplanes": rec["vplanes"], "resize": rec["resize"], "border": rec["border"], "rot": rec["rot"],
                    "warp": rec["warp"], "draws": rec["draws"], "bbox": [[float(v) for v in b] for b in bbox],
                    "ratio": [float(v) for v in ratio], "dw": [float(v) for v in dw], "dh": [float(v) for v in dh],
                    "returned_phrases": list(ori)})
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump({"cases": out}, fh, indent=0)
    print(f"wrote {OUT}: {len(out)} clips, {sum(len(c['shapes']) for c in out)} frames, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
