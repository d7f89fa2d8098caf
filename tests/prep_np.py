"""numpy restatement of the clip-preprocessing pixel spec (DESIGN.md "Clip preprocessing"): the tests' second opinion on
csrc/prep.hip, written from the spec, not from the kernel.  Every fp32 / fp64 operation is a separate numpy op (no fused
multiply-add), so where the spec fixes the order of operations the results are bit-exact.

    letterbox_u8(frame, job, size)  -> (size, size, 3) uint8     flip, HSV V-scaling, INTER_AREA resize, pad
    warp_u8(lb, job)                -> (size, size, 3) uint8     inverse affine on a 1/32 grid, 15-bit bilinear, border
    normalize(u8)                   -> (3, size, size) float32   ToTensor + Normalize
"""
from __future__ import annotations

import numpy as np

PAD = np.array([124, 116, 104], dtype=np.int64)
MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)

_I = np.arange(256, dtype=np.float64)
with np.errstate(divide="ignore"):
    SDIV = np.where(_I > 0, np.rint(1044480.0 / np.maximum(_I, 1)), 0).astype(np.int64)          # round((255 << 12) / v)
    HDIV = np.where(_I > 0, np.rint(737280.0 / (6.0 * np.maximum(_I, 1))), 0).astype(np.int64)   # round((180 << 12) / (6 d))


def rgb_to_hsv8(rgb: np.ndarray):
    """8-bit RGB -> (H in [0, 180), S, V) with the 12-bit division tables."""
    r, g, b = (rgb[..., c].astype(np.int64) for c in range(3))
    v = np.maximum(np.maximum(r, g), b)
    vmin = np.minimum(np.minimum(r, g), b)
    diff = v - vmin
    s = (diff * SDIV[v] + (1 << 11)) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * HDIV[diff] + (1 << 11)) >> 12
    h = np.where(h < 0, h + 180, h)
    return h, s, v


def hsv8_to_rgb(h, s, v) -> np.ndarray:
    """8-bit HSV -> RGB through float32: h*6/180 -> sector + fraction, s/255, v/255, round-to-nearest-even on x255."""
    f32 = np.float32
    hh = h.astype(f32) * (f32(6) / f32(180))
    sv = s.astype(f32) * (f32(1) / f32(255))
    vv = v.astype(f32) * (f32(1) / f32(255))
    sector = np.floor(hh).astype(np.int64)
    hh = hh - sector.astype(f32)
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector)
    hh = np.where(bad, f32(0), hh)
    one = f32(1)
    tab = np.stack([vv, vv * (one - sv), vv * (one - sv * hh), vv * (one - sv * (one - hh))])      # (4, ...)
    sel = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])              # (b, g, r) per sector
    bgr = [np.take_along_axis(tab, sel[sector, k][None], 0)[0] for k in range(3)]
    grey = s == 0
    rgb = np.stack([np.where(grey, vv, bgr[2]), np.where(grey, vv, bgr[1]), np.where(grey, vv, bgr[0])], -1)
    return np.clip(np.rint(rgb * f32(255)), 0, 255).astype(np.int64)


def scale_v(v, a_v: float):
    """V' = trunc(float32(V) * float32(a_v)), clipped to 255 first when a_v > 1 (vid_loader.py:367-370)."""
    x = v.astype(np.float32) * np.float32(a_v)
    if np.float32(a_v) > 1:
        x = np.minimum(x, np.float32(255))
    return x.astype(np.int64)


def hsv_adjust(rgb: np.ndarray, a_v: float) -> np.ndarray:
    h, s, v = rgb_to_hsv8(rgb)
    return hsv8_to_rgb(h, s, scale_v(v, a_v))


def _area_axis(ssize: int, dsize: int):
    """Per destination index: list of (source index, float32 weight) in OpenCV's area-table order."""
    scale = 1.0 / (float(dsize) / float(ssize))
    taps = []
    for d in range(dsize):
        fs1 = float(d) * scale
        fs2 = fs1 + scale
        cell = min(scale, float(ssize) - fs1)
        s1, s2 = int(np.ceil(fs1)), int(np.floor(fs2))
        s2 = min(s2, ssize - 1)
        s1 = min(s1, s2)
        t = []
        if float(s1) - fs1 > 1e-3:
            t.append((s1 - 1, np.float32((float(s1) - fs1) / cell)))
        for s in range(s1, s2):
            t.append((s, np.float32(1.0 / cell)))
        if fs2 - float(s2) > 1e-3:
            t.append((s2, np.float32(min(min(fs2 - float(s2), 1.0), cell) / cell)))
        taps.append(t)
    K = max(len(t) for t in taps)
    idx = np.zeros((dsize, K), dtype=np.int64)
    wt = np.zeros((dsize, K), dtype=np.float32)
    for d, t in enumerate(taps):
        for k, (s, w) in enumerate(t):
            idx[d, k], wt[d, k] = s, w
    return idx, wt


def resize_area_down(img: np.ndarray, rh: int, rw: int) -> np.ndarray:
    """Area-weighted box (both factors >= 1): per source row a horizontal fp32 sum in tap order, then the weighted vertical
    fp32 sum in tap order, round half to even.  Padding taps have weight 0 and sit after the real ones (x + 0 == x)."""
    h, w = img.shape[:2]
    xi, xw = _area_axis(w, rw)
    yi, yw = _area_axis(h, rh)
    src = img.astype(np.float32)
    rows = np.zeros((h, rw, 3), dtype=np.float32)
    for k in range(xi.shape[1]):
        rows = rows + xw[None, :, k, None] * src[:, xi[:, k], :]
    tot = np.zeros((rh, rw, 3), dtype=np.float32)
    for k in range(yi.shape[1]):
        tot = tot + yw[:, k, None, None] * rows[yi[:, k], :, :]
    return np.clip(np.rint(tot), 0, 255).astype(np.int64)


def _lin_axis(ssize: int, dsize: int):
    inv = float(dsize) / float(ssize)
    scale = 1.0 / inv
    s0 = np.zeros(dsize, np.int64); s1 = np.zeros(dsize, np.int64)
    a0 = np.zeros(dsize, np.int64); a1 = np.zeros(dsize, np.int64)
    for d in range(dsize):
        sx = int(np.floor(float(d) * scale))
        fx = np.float32(float(d + 1) - float(sx + 1) * inv)
        fx = np.float32(0) if fx <= 0 else np.float32(fx - np.floor(fx))
        if sx < 0:
            fx, sx = np.float32(0), 0
        if sx >= ssize - 1:
            fx, sx = np.float32(0), ssize - 1
        s0[d], s1[d] = sx, min(sx + 1, ssize - 1)
        a0[d], a1[d] = int(np.rint((np.float32(1) - fx) * np.float32(2048))), int(np.rint(fx * np.float32(2048)))
    return s0, s1, a0, a1


def resize_area_up(img: np.ndarray, rh: int, rw: int) -> np.ndarray:
    """OpenCV's INTER_AREA rule when a factor is < 1: two taps per axis, fx = (d+1) - (s+1)/scale reduced to its fraction,
    11-bit weights, (b0*D0 + b1*D1 + 2^21) >> 22."""
    h, w = img.shape[:2]
    x0, x1, a0, a1 = _lin_axis(w, rw)
    y0, y1, b0, b1 = _lin_axis(h, rh)
    src = img.astype(np.int64)
    D = a0[None, :, None] * src[:, x0, :] + a1[None, :, None] * src[:, x1, :]
    o = (b0[:, None, None] * D[y0] + b1[:, None, None] * D[y1] + (1 << 21)) >> 22
    return np.clip(o, 0, 255)


def letterbox_u8(frame: np.ndarray, job, size: int) -> np.ndarray:
    """The letterbox stage of one DcnPrepJob record (a JOB_DTYPE row) on its source frame."""
    img = frame[:, ::-1] if int(job["flip"]) else frame
    if int(job["hsv"]):
        img = hsv_adjust(img, float(job["a_v"]))
    h, w = img.shape[:2]
    rh, rw, top, left = int(job["rh"]), int(job["rw"]), int(job["top"]), int(job["left"])
    res = resize_area_down(img, rh, rw) if (w >= rw and h >= rh) else resize_area_up(img, rh, rw)
    out = np.empty((size, size, 3), dtype=np.int64)
    out[:] = PAD
    out[top:top + rh, left:left + rw] = res
    return out.astype(np.uint8)


def warp_u8(lb: np.ndarray, job) -> np.ndarray:
    """Output pixel (x, y) -> source (m0 x + m1 y + m2, m3 x + m4 y + m5) in fp64, x32, rounded half to even, clamped to
    +-2^30; taps at (X >> 5, Y >> 5) and their +1 neighbours with weights (32-ax)(32-ay)32 ..., (sum + 2^14) >> 15; a tap
    outside the image reads the border value."""
    S = lb.shape[0]
    if not int(job["warp"]):
        return lb.copy()
    m = np.asarray(job["minv"], dtype=np.float64)
    y, x = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    X = m[0] * x + m[1] * y + m[2]
    Y = m[3] * x + m[4] * y + m[5]
    lim = 1073741824.0
    Xi = np.rint(np.clip(X * 32.0, -lim, lim)).astype(np.int64)
    Yi = np.rint(np.clip(Y * 32.0, -lim, lim)).astype(np.int64)
    sx, sy, ax, ay = Xi >> 5, Yi >> 5, Xi & 31, Yi & 31
    src = lb.astype(np.int64)
    acc = np.zeros((S, S, 3), dtype=np.int64)
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = sx + dx, sy + dy
            inside = (xx >= 0) & (yy >= 0) & (xx < S) & (yy < S)
            v = np.where(inside[..., None], src[np.clip(yy, 0, S - 1), np.clip(xx, 0, S - 1)], PAD)
            wgt = (ax if dx else 32 - ax) * (ay if dy else 32 - ay) * 32
            acc = acc + v * wgt[..., None]
    return np.minimum((acc + (1 << 14)) >> 15, 255).astype(np.uint8)


def normalize(u8: np.ndarray) -> np.ndarray:
    """(S, S, 3) uint8 -> (3, S, S) float32: (u8 / 255 - mean) / std, each a separate float32 op (torchvision's order)."""
    x = u8.astype(np.float32).transpose(2, 0, 1) / np.float32(255)
    return ((x - MEAN[:, None, None]) / STD[:, None, None]).astype(np.float32)
