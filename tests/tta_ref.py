"""Inputs and a torch-CPU restatement of the multi-scale / mirror fusion (--scales; msl_predict_tta), shared by
tests/test_tta.py, tests/test_gpu_tta.py and scripts/time_tta.py.

    acc = 0
    for L, m in entries:                                     # fp32, summed in entry order
        p = softmax(F.interpolate(L, (ho, wo), mode="bilinear", align_corners=True), dim=1)
        acc = acc + (p.flip(-1) if m else p)
    cls  = np.argmax(acc)                                    # first maximum; a NaN pixel gives class 0
    prob = acc[cls] / n

As in tests/evaluate_ref.py the class depends on fp32 softmax values two math libraries round differently, so
the restatement also returns the near-tie mask - the top-2 gap of acc / n below evaluate_ref.NEAR_TIE - and
the two leading classes: off the mask a device result must agree exactly, on it it must be one of the two.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import evaluate_ref as er

# (C, low sizes (hi, wi), (ho, wo), flip): odd and even wo (the mirror column), three class counts, two
# entries without a mirror, entries larger and smaller than each other, and at 512 x 1024 - the low sizes of
# --scales 0.75,1.0,1.25 at 1024 x 512 - twice the pixels one pass of the grid covers
CASES = [
    (19, ((5, 9), (9, 17), (11, 21)), (33, 65), True),
    (16, ((4, 7), (5, 9), (7, 12)), (40, 71), True),
    (13, ((2, 3), (3, 3)), (7, 9), False),
    (19, ((7, 13), (9, 17), (12, 22)), (64, 128), True),
    (19, ((49, 97), (65, 129), (81, 161)), (512, 1024), True),
]
IDS = ["%dc_%dx%d" % (c, hw[0], hw[1]) for c, _, hw, _ in CASES]


def size_at(n, s):
    return max(1, int(math.floor(n * s + 0.5)))


def entries(case, nan=False):
    """[(logits (1,C,hi,wi), mirror)] of a case: entry (k, m) is evaluate_ref.logits(..., tag=f"T{k}{m}");
    `nan` plants a NaN in entry 1."""
    C, lows, _, flip = case
    out = []
    for k, (hi, wi) in enumerate(lows):
        for m in ((0, 1) if flip else (0,)):
            out.append((er.logits(C, hi, wi, tag=f"T{k}{m}", nan=nan and len(out) == 1), m))
    return out


def fuse(ents, hw, dtype=torch.float32):
    """acc [C, ho*wo] (numpy, `dtype`) by the rule above."""
    acc = 0
    for L, m in ents:
        p = F.softmax(er.up(L.to(dtype).cpu(), hw), dim=1)
        acc = acc + (p.flip(-1) if m else p)
    return acc[0].numpy().reshape(acc.shape[1], -1)


def tta_ref(ents, hw, dtype=torch.float32):
    """(cls int64 [ho*wo], near bool [ho*wo], top2 int64 [2, ho*wo]) of the fusion on torch-CPU."""
    acc = fuse(ents, hw, dtype)
    cls = np.argmax(acc, axis=0)
    avg = acc / acc.dtype.type(len(ents))
    order = np.argsort(-avg, axis=0, kind="stable")[:2]
    top = np.take_along_axis(avg, order, axis=0)
    with np.errstate(invalid="ignore"):
        near = (top[0] - top[1]) < er.NEAR_TIE  # False where the pixel is NaN: there the class is 0 for everyone
    return cls, near, order


@functools.lru_cache(maxsize=None)
def case_ref(index, nan=False):
    """tta_ref of CASES[index], computed once per process; treat the arrays as read-only."""
    return tta_ref(entries(CASES[index], nan), CASES[index][2])


def agrees(cls, ref):
    """Whether a device class map equals the restatement's off its mask and is one of its two leaders on it."""
    rc, near, top2 = ref
    cls = np.asarray(cls).reshape(-1).astype(np.int64)
    return bool(np.array_equal(cls[~near], rc[~near]) and
                ((cls[near] == top2[0][near]) | (cls[near] == top2[1][near])).all())
