"""Inputs and the torch-CPU restatement of the prediction images (msl_predict_images), shared by
tests/test_predict_images.py and tests/test_gpu_predict_images.py.  Built on tests/evaluate_ref.py: the class is
that file's predict_ref; this file adds the winning probability and what is decided from it.

    no flip:  P = softmax(up(low))                        flip:  P = (softmax(up(low)) + flip(softmax(up(low_flip)))) / 2
    top = max over classes of P; bucket 0 where top > 0.9, else 1 where > 0.8, else 2 where > 0.7, else 3 where
    > 0.5, else 4 (black); the pseudo-label keeps the class where top > THR (0.95), else 255.

Two fp32 softmaxes round differently (about 1e-6 relative), so a pixel whose reference `top` lies within
NEAR_EDGE = 1e-5 of one of the five cut values may land on either side of it: the near-edge mask.  A NaN pixel
(top is NaN) is black and 255 for everyone and is never on the mask.
"""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

import evaluate_ref as ev

SPLITS = (0.9, 0.8, 0.7, 0.5)
THR = 0.95
NEAR_EDGE = 1e-5
GRID_CAP = 1024  # kPredictBlocks of csrc/predict.hip: blocks of 256 threads, four pixels per thread
# (C, hi, wi, ho, wo): wo % 4 != 0 in one block; the dword path; odd wo (the mirror column); several blocks; and
# more pixels than one pass of the capped grid covers (1028 * 1032 > 1024 * 256 * 4)
SHAPES = [(13, 3, 3, 7, 9), (19, 5, 7, 12, 16), (16, 5, 9, 40, 71), (19, 9, 17, 33, 65), (19, 33, 65, 1028, 1032)]
assert SHAPES[-1][3] * SHAPES[-1][4] > GRID_CAP * 256 * 4 and SHAPES[-1][4] % 4 == 0


def gold():
    return np.load(os.path.join(ev.GOLD, "predict_images_kat.npz"), allow_pickle=False)


def inputs(C, hi, wi, flip, nan=False):
    """(low, low_flip or None): std 6 logits; the mirrored image's logits are the mirror of low plus std 1 noise,
    so that the averaged maximum spreads over every bucket (independent flip logits pile it onto 0.5)."""
    low = ev.logits(C, hi, wi, std=6.0, nan=nan)
    if not flip:
        return low, None
    return low, low.flip(-1) + ev.logits(C, hi, wi, tag="F", std=1.0)


@functools.lru_cache(maxsize=None)
def reference(shape, flip, nan=False):
    """dict(cls, near_tie, top2, top, bucket, keep, near_edge) of one case, each [ho*wo]; computed once."""
    C, hi, wi, ho, wo = shape
    low, lowf = inputs(C, hi, wi, flip, nan)
    cls, near_tie, top2 = ev.predict_ref(low, (ho, wo), lowf)
    p = F.softmax(ev.up(low, (ho, wo)), dim=1)
    if flip:
        p = (p + F.softmax(ev.up(lowf, (ho, wo)), dim=1).flip(-1)) / 2
    top = p[0].numpy().reshape(C, -1).max(axis=0)  # NaN where the pixel is NaN
    with np.errstate(invalid="ignore"):
        bucket = np.full(top.shape, 4, np.int64)
        for b in reversed(range(4)):
            bucket[top > np.float32(SPLITS[b])] = b
        keep = top > np.float32(THR)
        near_edge = np.zeros(top.shape, bool)
        for e in SPLITS + (THR,):
            near_edge |= np.abs(top.astype(np.float64) - e) <= NEAR_EDGE
    return dict(cls=cls, near_tie=near_tie, top2=top2, top=top, bucket=bucket, keep=keep, near_edge=near_edge)
