"""TEST INFRASTRUCTURE - a numpy restatement of the two per-image analysis kernels (msl_image_metrics,
msl_analysis_maps) and the inputs the CPU and GPU tests share.

metrics_row restates the scores with exact integer sums, one fp64 conversion, numpy's per-class ratios and
*sequential* sums in class order for the nan-means and FWIoU - the kernel's own order, so the only difference
to numpy's pairwise np.nanmean / np.sum is the summation order of at most 32 fp64 terms in [0, 1]:
2 * 31 * 32 * 2^-53 ~ 2.2e-13 < 1e-12.  maps restates the four RGB maps byte for byte.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HEAD = 9  # PA, MPA, MIoU, FWIoU, MPA_13, MIoU_13, FWIoU_13, pixels, selected
SET_16_TO_13 = [0, 1, 2, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]
MEAN_TOL = 1e-12
IMG_MEAN = np.array((104.00698793, 116.66876762, 122.67891434), dtype=np.float32)


def gold():
    return np.load(os.path.join(HERE, "golden", "analysis_kat.npz"))


# ----------------------------------------------------------------------------- msl_image_metrics
def _nanmean_seq(v):
    s, n = 0.0, 0
    for a in v:
        if not np.isnan(a):
            s, n = s + float(a), n + 1
    return s / n if n else float("nan")


def _fw_seq(r, iou, total):
    s = 0.0
    for w, u in zip(r, iou):
        if not np.isnan(u):
            s = s + float(w) * float(u)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(s) / np.float64(total))


def metrics_row(cm, threshold):
    """The row msl_image_metrics writes for the integer matrix cm [C, C] (fp64 [9 + C])."""
    m = np.asarray(cm).astype(np.uint64)
    C = m.shape[0]
    r, s, d = m.sum(axis=1, dtype=np.uint64), m.sum(axis=0, dtype=np.uint64), np.diag(m).copy()
    total, trace = int(r.sum(dtype=np.uint64)), int(d.sum(dtype=np.uint64))
    rd, sd, dd = r.astype(np.float64), s.astype(np.float64), d.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        acc, iou = dd / rd, dd / (rd + sd - dd)
    row = np.full(HEAD + C, np.nan)
    row[0] = float(np.float64(trace) / np.float64(total)) if total else 0.0
    row[1], row[2], row[3] = _nanmean_seq(acc), _nanmean_seq(iou), _fw_seq(rd, iou, float(total))
    if C == 16:
        k = SET_16_TO_13
        row[4], row[5], row[6] = _nanmean_seq(acc[k]), _nanmean_seq(iou[k]), _fw_seq(rd[k], iou[k], float(total))
    row[7] = float(total)
    miou = row[5] if C == 16 else row[2]
    row[8] = 1.0 if miou < threshold else 0.0  # strict; NaN < x is False
    row[HEAD:] = iou
    return row


def val_miou(row, C):
    """The MIoU the decision is taken on: val_info's (the 13-class one for 16 classes)."""
    return row[5] if C == 16 else row[2]


def _random(C, seed, scale=2000):
    rng = np.random.default_rng(1000 * C + seed)
    m = rng.integers(0, scale, size=(C, C)).astype(np.int64)
    m[np.arange(C), np.arange(C)] += rng.integers(0, 8 * scale, size=C)
    return m


def matrices(C):
    """name -> int64 [C, C]: the hand-made matrices of the issue and two random ones."""
    out = {}
    m = _random(C, 1)
    if C > 1:
        m[C // 2, :] = 0
        m[:, C // 2] = 0
    out["absent"] = m  # a class neither labelled nor predicted: acc and IoU NaN
    m = _random(C, 2)
    m[C - 1, :] = 0
    out["only_predicted"] = m  # the last class is predicted, never labelled: IoU 0 (C > 1), acc NaN
    out["zero"] = np.zeros((C, C), np.int64)
    m = _random(C, 3, 1000) + (np.int64(1) << 40)
    m[0, 0] += 12345
    out["big"] = m  # counts near 2^40: sums near 2^45, exact in fp64
    m = np.zeros((C, C), np.int64)
    for i in range(C):
        m[i, i] += 2
        m[i, (i + 1) % C] += 1
    out["half"] = m  # C > 1: r = s = 3, d = 2, every IoU exactly 2 / 4
    out["random_a"], out["random_b"] = _random(C, 4), _random(C, 5, 7)
    return out


# ----------------------------------------------------------------------------- msl_analysis_maps
def input_image(x, mean=IMG_MEAN):
    """utils/images.py:recover_input's bytes of x [3, h, w] fp32 BGR - mean: uint8 (h, w, 3) RGB."""
    with np.errstate(invalid="ignore"):
        v = np.rint(x.astype(np.float32) + mean.astype(np.float32)[:, None, None])  # fp32 add, half to even
        v = np.where(np.isnan(v), np.float32(0), np.clip(v, 0, 255))
    return np.ascontiguousarray(v.astype(np.uint8)[::-1].transpose(1, 2, 0))


def maps(x, label, cls, palette, C, mean=IMG_MEAN):
    """{"label", "pred", "input", "error"} -> uint8 (h, w, 3) of x [3, h, w] fp32, label int64 (h, w), cls uint8
    (h, w) and palette uint8 [C, 3]."""
    label, cls = np.asarray(label, np.int64), np.asarray(cls, np.uint8).astype(np.int64)
    valid = (label >= 0) & (label < C)
    black = np.zeros(label.shape + (3,), np.uint8)
    lab = np.where(valid[..., None], palette[np.clip(label, 0, C - 1)], black)
    pred = np.where((cls < C)[..., None], palette[np.minimum(cls, C - 1)], black)
    inp = input_image(x, mean)
    err = np.where(valid[..., None], np.where((cls == label)[..., None], inp >> 1, pred), black)
    return {"label": lab, "pred": pred, "input": inp, "error": err}


def map_inputs(h, w, C, seed=0):
    """(x [3, h, w] fp32, label int64 (h, w), cls uint8 (h, w)): x is uint8 - mean plus injected x.5 values
    (on the fp32 grid after adding the mean), negatives, values over 255 and one NaN; the labels hold -1, 255, C
    and valid classes; cls agrees with the label on about half of the pixels."""
    rng = np.random.default_rng(97 + 1000 * seed + h * w)
    u8 = rng.integers(0, 256, size=(3, h, w)).astype(np.float32)
    x = (u8 - IMG_MEAN[:, None, None]).astype(np.float32)
    flat = x.reshape(-1)
    n = flat.size
    half = np.array([0.5, 1.5, 2.5, 127.5, 128.5, 254.5, 255.5, -0.5], np.float32)
    for i, v in enumerate(half[:min(len(half), n // 2)]):  # sums that land on x.5 after the fp32 add of the mean
        k = (7 * i + 1) % n
        flat[k] = np.float32(v) - IMG_MEAN[k // (h * w)]
    extra = [-300.0, 400.0, 1e9, -1e9, np.nan]
    for i, v in enumerate(extra):
        flat[(11 * i + 5) % n] = v
    label = rng.integers(0, C, size=(h, w)).astype(np.int64)
    lf = label.reshape(-1)
    for i, v in enumerate((-1, 255, C, 0, C - 1)):
        lf[(5 * i + 2) % lf.size] = v
    cls = np.where(rng.random((h, w)) < 0.5, np.clip(label, 0, C - 1), rng.integers(0, C, size=(h, w))).astype(np.uint8)
    return x, label, cls
