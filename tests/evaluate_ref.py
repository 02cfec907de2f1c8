"""Inputs and a torch-CPU restatement of the evaluator's per-pixel class (tools/evaluate.py:114-141 of the
reference), shared by tests/test_evaluate.py, tests/test_gpu_evaluate.py, scripts/gen_golden_evaluate.py and
scripts/time_evaluate.py.

    pred = F.interpolate(low, size, mode="bilinear", align_corners=True)          (deeplab_multi.py:124)
    no flip:  np.argmax(pred, axis=1)                                             (evaluate.py:137-139)
    flip:     np.argmax((softmax(pred) + flip(softmax(pred_of_flipped_image))) / 2)   (:120-135, :139)

The flip class depends on fp32 softmax values that two math libraries round differently (about 1e-6
relative over <= 19 classes), so the restatement also returns a per-pixel near-tie mask - the top-2 gap of
the averaged probability below NEAR_TIE = 1e-5 - and the two leading classes: off the mask a device result
must agree exactly, on it it must be one of the two.
"""
import contextlib
import io
import os

import numpy as np
import torch
import torch.nn.functional as F

from maxsquareloss_amd.utils.synthetic import counter_normal, counter_uniform

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEAR_TIE = 1e-5
SEED = 83
# (C, hi, wi, ho, wo): odd and even wo (the mirror column), three class counts, one block up to more
# pixels than one pass of the grid covers (512 x 1024 = 2048 blocks of 256 over a grid of 1024)
SHAPES = [(19, 9, 17, 33, 65), (16, 5, 9, 40, 71), (13, 3, 3, 7, 9), (19, 9, 17, 64, 128), (19, 65, 129, 512, 1024)]


def logits(C, hi, wi, tag="L", std=3.0, nan=False):
    """(1, C, hi, wi) counter_normal logits, std 3; `nan` plants one NaN away from the border."""
    t = torch.from_numpy(counter_normal(SEED, f"ev_{tag}_{C}_{hi}x{wi}", C * hi * wi, std)).view(1, C, hi, wi).clone()
    if nan:
        t[0, C // 2, hi // 2, wi // 2] = float("nan")
    return t


def labels(C, ho, wo):
    """int64 (ho, wo) uniform over {-1, ..., C} (both ends ignored) with a run of 255 in the first row."""
    u = counter_uniform(SEED, f"ev_label_{C}_{ho}x{wo}", ho * wo)
    lab = torch.from_numpy(np.floor(u * (C + 2)).astype(np.int64) - 1).view(ho, wo).clone()
    lab[0, :min(5, wo)] = 255
    return lab


def up(low, hw):
    return F.interpolate(low, size=tuple(hw), mode="bilinear", align_corners=True)


def predict_ref(low, hw, low_flip=None):
    """(cls int64 [ho*wo], near bool [ho*wo], top2 int64 [2, ho*wo]) of the evaluator on torch-CPU.
    Without low_flip the class is exact: near is all False and top2 is None."""
    C = low.size(1)
    pred = up(low.float().cpu(), hw)
    if low_flip is None:
        cls = np.argmax(pred[0].numpy().reshape(C, -1), axis=0)
        return cls, np.zeros(cls.shape, dtype=bool), None
    p = F.softmax(pred, dim=1)
    pf = F.softmax(up(low_flip.float().cpu(), hw), dim=1).flip(-1)
    avg = ((p + pf) / 2)[0].numpy().reshape(C, -1)
    cls = np.argmax(avg, axis=0)
    order = np.argsort(-avg, axis=0, kind="stable")[:2]
    top = np.take_along_axis(avg, order, axis=0)
    with np.errstate(invalid="ignore"):
        near = (top[0] - top[1]) < NEAR_TIE  # False where the pixel is NaN: there the class is 0 for everyone
    return cls, near, order


def confusion_ref(gt, cls, C):
    """utils/eval.py:109-115 on a class map."""
    g = np.asarray(gt).reshape(-1)
    keep = (g >= 0) & (g < C)
    return np.bincount(C * g[keep].astype(np.int64) + cls[keep], minlength=C * C).reshape(C, C)


def kat_matrix(C):
    """A fixed [C, C] count matrix with absent classes: 3 never labelled nor predicted, 5 never labelled,
    7 never predicted (NaN cells in three different columns of the per-class table)."""
    m = np.random.default_rng(1000 + C).integers(0, 5000, size=(C, C)).astype(np.float64)
    m[3, :] = 0
    m[:, 3] = 0
    m[5, :] = 0
    m[:, 7] = 0
    return m


KAT_CASES = [(19, False), (19, True), (16, False)]


def kat_key(C, out_16_13):
    return f"table{C}" + ("_16_13" if out_16_13 else "")


def table_text(ev, out_16_13=False):
    """What ev.Print_Every_class_Eval(out_16_13) prints."""
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        ev.Print_Every_class_Eval(out_16_13)
    return buf.getvalue()


def gold(name="evaluate_kat.npz"):
    return np.load(os.path.join(GOLD, name), allow_pickle=False)
