"""The torch-CPU / numpy restatement of the class-balanced pseudo-label thresholds (msl_confidence_hist,
msl_class_thresholds, msl_pseudo_classwise), shared by tests/test_pseudo_cw.py and tests/test_gpu_pseudo_cw.py.
Built on tests/predict_images_ref.py: reference(shape, flip) gives the class `cls`, the winning probability `top`
(fp32, NaN where the pixel is NaN) and the `near_tie` mask of the flip rule.

    hist[k][b] += 1   with k = cls, b = min(bins - 1, int(fp32(top) * fp32(bins)))           (hist_ref)
    thr[k] = min(thr_max, b* / bins), b* the largest bin whose suffix sum reaches ceil(portion * N_k)
                                                                                            (thresholds_ref)
    label = cls where top > thr[cls], else -1                                                (labels_ref)

Two fp32 softmaxes round differently (about 1e-6 relative), so a pixel whose fp64 `top` lies within
NEAR_EDGE = 1e-5 of a bin edge j / bins (the histogram) or of thr[k] (the labels) may fall on either side: the
near-edge masks, the allowance tests/test_gpu_predict_images.py makes for its five cut values.
"""
import functools

import numpy as np

import predict_images_ref as pir

NEAR_EDGE = 1e-5
SHAPES = pir.SHAPES
BINS = (64, 512)
# the largest tile msl_confidence_hist takes, 32 * 512 = 16384 cells (64 KB of LDS), on the generic class-count body
LIMIT_SHAPE, LIMIT_BINS = (32, 9, 17, 33, 65), 512
assert LIMIT_SHAPE[0] * LIMIT_BINS == 16384


def near_cap(npx):
    """How many pixels of an image may lie near a bin edge before the allowance could hide a wrong bin rule: 2 %
    of the image.  The 7 x 9 image has 63 pixels, of which the restatement itself puts 3 near one of 511 edges
    (flip, 512 bins): for that image alone the cap is those three pixels."""
    return 3 if npx == 63 else 0.02 * npx


def bin_of(top, bins):
    """The fp32 bin rule on an fp32 array without NaNs."""
    t = np.asarray(top, np.float32) * np.float32(bins)
    assert t.dtype == np.float32
    return np.minimum(bins - 1, t.astype(np.int64))


def near_bin_edge(top, bins):
    """(near bool, j int64): whether the fp64 value of `top` lies within NEAR_EDGE of an inner edge j / bins,
    1 <= j <= bins - 1, and that edge (the edges are at least 1 / 1024 apart: at most one).  Below edge 0 there is
    nothing and at 1.0 the bin is clamped, so neither is an edge.  NaN pixels are never near."""
    t = np.asarray(top).astype(np.float64)
    with np.errstate(invalid="ignore"):
        j = np.where(np.isnan(t), 0, np.rint(t * bins)).astype(np.int64)
        near = (np.abs(t - j / bins) <= NEAR_EDGE) & (j >= 1) & (j <= bins - 1)
    return near, j


def hist_of(cls, top, C, bins, mask=None):
    """int64 [C, bins]: the counts of the non-NaN pixels (inside `mask`, if given)."""
    ok = ~np.isnan(top)
    if mask is not None:
        ok &= mask
    flat = cls[ok].astype(np.int64) * bins + bin_of(top[ok], bins)
    return np.bincount(flat, minlength=C * bins).reshape(C, bins)


@functools.lru_cache(maxsize=None)
def hist_ref(shape, flip, bins, nan=False):
    """dict(hist, hist_off_tie, edge_count, tie_count, valid) of one case.  hist: all non-NaN pixels; hist_off_tie:
    those off the near-tie mask; edge_count[k][j]: class-k pixels off the near-tie mask that are near edge j;
    tie_count[k]: near-tie pixels one of whose two leading classes is k (they may be counted in either row);
    valid: the number of non-NaN pixels."""
    C = shape[0]
    r = pir.reference(shape, flip, nan)
    cls, top, tie = r["cls"], r["top"], r["near_tie"]
    near, j = near_bin_edge(top, bins)
    edge_count = np.zeros((C, bins + 1), np.int64)
    sel = near & ~tie
    np.add.at(edge_count, (cls[sel], j[sel]), 1)
    tie_count = np.zeros(C, np.int64)
    if tie.any():
        for row in r["top2"]:
            tie_count += np.bincount(row[tie], minlength=C)
    return dict(hist=hist_of(cls, top, C, bins), hist_off_tie=hist_of(cls, top, C, bins, ~tie),
                edge_count=edge_count, tie_count=tie_count, valid=int((~np.isnan(top)).sum()),
                near=int(near.sum()))


def suffix(hist):
    """[C, bins + 1]: column j = the count at or above edge j (column bins is 0)."""
    h = np.asarray(hist, np.int64)
    out = np.zeros((h.shape[0], h.shape[1] + 1), np.int64)
    out[:, :-1] = h[:, ::-1].cumsum(axis=1)[:, ::-1]
    return out


def thresholds_ref(hist, portion, thr_max):
    """(thr fp32 [C], kept int64 [C], q fp32 [C]) in numpy integers and fp64, as include/msl_hip.h states the
    rule."""
    h = np.asarray(hist, np.int64)
    C, bins = h.shape
    suf = suffix(h)
    thr, kept, qs = np.empty(C, np.float32), np.empty(C, np.int64), np.empty(C, np.float32)
    for k in range(C):
        n = int(suf[k, 0])
        need = int(np.ceil(np.float64(portion) * np.float64(n)))
        if need == 0:
            b = bins
        else:
            ok = np.nonzero(suf[k, :bins] >= need)[0]
            b = int(ok[-1]) if len(ok) else 0
        q = np.float32(b) / np.float32(bins)
        t = np.float32(thr_max) if n == 0 else min(np.float32(thr_max), q)
        thr[k], qs[k] = t, q
        kept[k] = suf[k, min(bins, int(np.float32(t) * np.float32(bins)))]
    return thr, kept, qs


def labels_ref(cls, top, thr):
    """int64 [npx]: cls where top > thr[cls] (strict, fp32; NaN fails), else -1."""
    thr = np.asarray(thr, np.float32)
    with np.errstate(invalid="ignore"):
        keep = np.asarray(top, np.float32) > thr[cls]
    return np.where(keep, cls, -1).astype(np.int64)


def near_threshold(cls, top, thr):
    """bool [npx]: the fp64 top within NEAR_EDGE of the pixel's own class's threshold."""
    with np.errstate(invalid="ignore"):
        return np.abs(np.asarray(top).astype(np.float64) - np.asarray(thr, np.float32).astype(np.float64)[cls]) \
            <= NEAR_EDGE


# hand-built histograms for msl_class_thresholds: (name, hist [C, bins], portion, thr_max, thr expected or None)
def hand_cases():
    bins = 16
    z = np.zeros((6, bins), np.int64)
    a = z.copy()
    a[0, 3], a[0, 9], a[0, 15] = 5, 3, 2      # 10 pixels: suffix sums 2 (15), 5 (9), 10 (3)
    a[1, 15] = 7                              # all mass in the top bin
    a[2, 0] = 4                               # all mass in the lowest bin
    a[3, 8], a[3, 12] = 4, 4                  # need lands exactly on a bin boundary at portion 0.5
    a[5, 14], a[5, 15] = 10, 10               # row 4 stays empty
    out = [
        ("half", a, 0.5, 0.9, [9 / 16, 0.9, 0.0, 12 / 16, 0.9, 0.9]),
        ("portion0", a, 0.0, 0.9, [0.9] * 6),
        ("portion1", a, 1.0, 0.9, [3 / 16, 0.9, 0.0, 8 / 16, 0.9, 14 / 16]),
        ("nocap", a, 0.5, 1.0, [9 / 16, 15 / 16, 0.0, 12 / 16, 1.0, 15 / 16]),
        ("just_over", a, 0.500001, 0.95, [3 / 16, 0.9375, 0.0, 8 / 16, 0.95, 14 / 16]),
    ]
    rng = np.random.default_rng(11)
    big = rng.integers(0, 1 << 40, size=(19, 512)).astype(np.int64)   # sums far above 2^32
    big[7] = 0
    out.append(("wide", big, 0.3, 0.9, None))
    small = rng.integers(0, 3, size=(13, 1024)).astype(np.int64)      # 13 * 1024 cells, many zeros
    out.append(("bins1024", small, 0.75, 0.8, None))
    few = rng.integers(0, 50, size=(32, 32)).astype(np.int64)         # fewer bins than lanes in a wave
    out.append(("bins32", few, 0.5, 0.9, None))
    return out
