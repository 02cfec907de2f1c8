"""Host tables of Pillow's 8-bit resampling (numpy only; csrc/resample.hip runs them on the device).

`Image.resize` on an 8-bit image is integer arithmetic on tables computed once per (in, out) size
on the host (Pillow's precompute_coeffs + normalize_coeffs_8bpc for the convolution filters, the
scale-only affine walk for NEAREST).  The tables here are those tables, in IEEE doubles and C
truncation, so a kernel that runs the same integer sums is byte-exact against Pillow:

  bicubic_table(in, out) -> (bounds int32 [out][2] = (first tap, taps), coeffs int32 [out][ksize], ksize)
  nearest_table(in, out) -> int32 [out] source index of every output index

One bicubic pass over an axis is  out = clamp((2^21 + sum_k pixel[first + k] * coeff[k]) >> 22, 0, 255)
(int32, arithmetic shift).  A resize runs the horizontal pass into a uint8 image, then the
vertical pass on that; an axis whose size does not change gets no pass.  `resize_bicubic` /
`resize_nearest` are that in numpy: the restatement the tests and scripts compare against.

Crop semantics (datasets/cityscapes_Dataset.py:186-196 of the reference: `img.crop(...)`, then
`resize` on the crop): the crop is a source offset and the table's in-size is the crop size, so no
tap reads outside the crop (unlike Pillow's `box=` argument).  The mirror is applied to the whole
source first: crop coordinates are coordinates in the mirrored image.
"""
import functools
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2  # Pillow's fixed point of the 8-bit paths
MAX_KSIZE = 64               # the kernels' bound on taps per output (msl_resize_bicubic_rgb)


def _bicubic(t):
    a = -0.5
    if t < 0.0:
        t = -t
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    if t < 2.0:
        return (((t - 5) * t + 8) * t - 4) * a
    return 0.0


@functools.lru_cache(maxsize=256)
def bicubic_table(in_size, out_size):
    """Pillow's BICUBIC coefficients for one axis, normalised to 22-bit fixed point."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"bicubic_table: sizes must be positive, got {in_size} -> {out_size}")
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), np.int32)
    coeffs = np.zeros((out_size, ksize), np.int32)
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, xmax)
        for x, v in enumerate(w):
            coeffs[xx, x] = int(v * one + 0.5) if v >= 0 else int(v * one - 0.5)
    bounds.setflags(write=False)
    coeffs.setflags(write=False)
    return bounds, coeffs, ksize


@functools.lru_cache(maxsize=256)
def nearest_table(in_size, out_size):
    """Pillow's NEAREST source index per output index (the incremental fp64 walk of its affine path)."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"nearest_table: sizes must be positive, got {in_size} -> {out_size}")
    a = in_size / out_size
    xo = a * 0.5
    idx = np.zeros(out_size, np.int32)
    for x in range(out_size):
        idx[x] = min(int(xo), in_size - 1)
        xo += a
    idx.setflags(write=False)
    return idx


def _pass(img, bounds, coeffs, axis):
    """One resampling pass of a uint8 array along `axis` (0 = vertical, 1 = horizontal)."""
    src = np.moveaxis(img, axis, 0).astype(np.int32)
    out = np.empty((len(bounds),) + src.shape[1:], np.uint8)
    for i, (lo, n) in enumerate(bounds):
        k = coeffs[i, :n].astype(np.int32).reshape((n,) + (1,) * (src.ndim - 1))
        acc = (1 << (PRECISION_BITS - 1)) + (src[lo:lo + n] * k).sum(axis=0, dtype=np.int32)
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def source_view(arr, crop=None, mirror=False):
    """The (mirrored, then cropped) view of an (H, W[, C]) array; crop = (x1, y1, w, h)."""
    if mirror:
        arr = arr[:, ::-1]
    if crop is not None:
        x1, y1, cw, ch = (int(v) for v in crop)
        h, w = arr.shape[:2]
        if x1 < 0 or y1 < 0 or cw < 1 or ch < 1 or x1 + cw > w or y1 + ch > h:
            raise ValueError(f"crop {crop} leaves the {w}x{h} source")
        arr = arr[y1:y1 + ch, x1:x1 + cw]
    return arr


def resize_bicubic(rgb, out_wh, crop=None, mirror=False):
    """`Image.resize(out_wh, BICUBIC)` of the mirrored / cropped uint8 (H, W, C) image, in numpy."""
    img = np.ascontiguousarray(source_view(np.asarray(rgb, np.uint8), crop, mirror))
    ow, oh = int(out_wh[0]), int(out_wh[1])
    h, w = img.shape[:2]
    if ow != w:
        b, k, _ = bicubic_table(w, ow)
        img = _pass(img, b, k, 1)
    if oh != h:
        b, k, _ = bicubic_table(h, oh)
        img = _pass(img, b, k, 0)
    return np.ascontiguousarray(img)


def resize_nearest(ids, out_wh, crop=None, mirror=False):
    """`Image.resize(out_wh, NEAREST)` of the mirrored / cropped uint8 (H, W) map, in numpy."""
    img = source_view(np.asarray(ids, np.uint8), crop, mirror)
    ow, oh = int(out_wh[0]), int(out_wh[1])
    h, w = img.shape[:2]
    if oh != h:
        img = img[nearest_table(h, oh)]
    if ow != w:
        img = img[:, nearest_table(w, ow)]
    return np.ascontiguousarray(img)


def bgr_minus_mean(rgb, mean):
    """The reference's _img_transform on a uint8 (H, W, 3) image: fp32 BGR - mean, (3, H, W)."""
    img = np.asarray(rgb, np.float32)[:, :, ::-1] - np.asarray(mean, np.float32)
    return np.ascontiguousarray(img.transpose(2, 0, 1))
