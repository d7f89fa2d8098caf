"""Pin dcnet_amd/video.py's window rule to the REAL reference and write tests/golden/video_windows.json.

Runs only where the reference checkout exists (like oracle/make_goldens.py and tools/make_prep_goldens.py), never on the GPU box:

    python tools/make_video_goldens.py

``getChunk`` (dataset/vid_loader.py:143-180) builds the windows that test_DCNet.py feeds to the n_frame model.  It is driven here on
synthetic videos — a frame's "path" is its index as a string — for F in {2, 5, 6, 8, 12} frames and K in {2, 3, 5, 8} frames per
window, in the evaluation split.  The fixture holds the windows as lists of frame indices: data only, no reference text.
"""
from __future__ import annotations

import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "video_windows.json")
FRAMES = (2, 5, 6, 8, 12)
WINDOWS = (2, 3, 5, 8)


def main():
    from oracle import make_goldens as MG
    MG._import_reference()
    import torch
    from dataset import vid_loader as VL                     # the reference's loader module
    assert VL.__file__.startswith(MG.REF), VL.__file__
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        for F in FRAMES:
            path = os.path.join(tmp, f"video_{F}.pth")
            torch.save([[(str(i), [0, 0, 1, 1], "a phrase") for i in range(F)]], path)
            for K in WINDOWS:
                chunks = VL.getChunk(path, "val", num_frame_k=K)
                cases.append({"frames": F, "n_frame": K, "windows": [[int(p) for p in c[0]] for c in chunks]})
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump({"cases": cases}, fh, indent=0)
    print(f"wrote {OUT}: {len(cases)} cases, {sum(len(c['windows']) for c in cases)} windows, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
