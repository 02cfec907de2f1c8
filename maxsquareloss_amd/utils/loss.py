"""Loss modules with the reference's signatures (utils/loss.py) on HIP kernels.

`MaxSquareloss.forward(pred, prob)` / `IW_MaxSquareloss.forward(pred, prob, label)`
behave exactly like loss.py:69-119 when given an explicit probability tensor.
Passing `prob=None` selects the fused path: the loss is computed straight
from the logits behind `pred` (the low-res ASPP output when `pred` came from
this package's DeeplabMulti), with softmax, upsampling and the loss fused into
one forward and one backward kernel pair.
"""
import torch
import torch.nn as nn

from .. import ops


def _fused_source(pred):
    low = ops.low_of(pred)
    if low is None:  # a plain hi-res logits tensor: identity interpolation
        low = pred
    return low, tuple(pred.shape[2:])


class MaxSquareloss(nn.Module):
    """loss = -sum(p^2) / (2*N*C*H*W) (loss.py:104-119; the `prob != -1` mask is a no-op, Q5)."""

    def __init__(self, ignore_index=-1, num_class=19):
        super().__init__()
        self.ignore_index = ignore_index
        self.num_class = num_class

    def forward(self, pred, prob=None):
        if prob is None:
            low, hw = _fused_source(pred)
            return ops.maxsquare_up(low, hw)
        return ops.maxsquare_prob(prob)


class IW_MaxSquareloss(nn.Module):
    """Image-wise class-balanced MaxSquare (loss.py:69-102).

    hist = per-class pixel count of argmax(prob) (or of `label`), weights
    w_c = 1/max(hist_c^ratio * (sum hist)^(1-ratio), 1),
    loss = -sum_px w[argmax] * sum_c p^2 / (N*C).  The last histogram and
    weights are kept on the module (`last_hist`, `last_weights`, device tensors).
    """

    def __init__(self, ignore_index=-1, num_class=19, ratio=0.2):
        super().__init__()
        self.ignore_index = ignore_index
        self.num_class = num_class
        self.ratio = ratio
        self.last_hist = None
        self.last_weights = None

    def forward(self, pred, prob=None, label=None):
        if prob is None:
            if label is not None:
                raise NotImplementedError("fused IW_MaxSquareloss counts argmax(prob); pass prob with label")
            low, hw = _fused_source(pred)
            loss, hist, w = ops.iw_maxsquare_up(low, hw, self.ratio)
        else:
            loss, hist, w = ops.iw_maxsquare_prob(prob, label, self.ratio)
        self.last_hist, self.last_weights = hist, w
        return loss


class softCrossEntropy(nn.Module):
    """loss = mean over target != ignore_index of -log_softmax(inputs) * target (loss.py:17-35).
    `target=None` is the trainer's call softCrossEntropy()(pred, softmax(pred)) (the `entropy` target
    mode, target not detached) fused from the logits behind `inputs`: sum_px sum_c -lp_c p_c / (C*H*W)."""

    def __init__(self, ignore_index=-1):
        super().__init__()
        self.ignore_index = ignore_index

    def forward(self, inputs, target=None):
        if target is None:
            low, hw = _fused_source(inputs)
            return ops.entropy_up(low, hw)
        return ops.soft_ce(inputs, target, self.ignore_index)


class IWsoftCrossEntropy(nn.Module):
    """Image-wise class-balanced soft cross-entropy (loss.py:37-67).

    hist = per-class pixel count of argmax(inputs) (the logits), weights as IW_MaxSquareloss,
    loss = sum_px w[argmax] * sum_c -log_softmax(inputs)_c * target_c / (N*C) over target != ignore_index.
    `target=None` is the `IW_entropy` target mode (target = softmax(inputs), not detached), fused.
    The last histogram and weights are kept on the module (`last_hist`, `last_weights`)."""

    def __init__(self, ignore_index=-1, num_class=19, ratio=0.2):
        super().__init__()
        self.ignore_index = ignore_index
        self.num_class = num_class
        self.ratio = ratio
        self.last_hist = None
        self.last_weights = None

    def forward(self, inputs, target=None):
        if inputs.size(1) != self.num_class:
            raise ValueError(f"IWsoftCrossEntropy(num_class={self.num_class}) on {inputs.size(1)} channels")
        if target is None:
            low, hw = _fused_source(inputs)
            loss, hist, w = ops.iw_entropy_up(low, hw, self.ratio)
        else:
            loss, hist, w = ops.iw_soft_ce(inputs, target, self.ratio, self.ignore_index)
        self.last_hist, self.last_weights = hist, w
        return loss


class CrossEntropyLoss(nn.Module):
    """nn.CrossEntropyLoss(ignore_index=-1) on (1,C,H,W) logits and (1,H,W) int64 labels
    (train_source.py:128).  Mean over non-ignored pixels; nan when none (quirk Q8)."""

    def __init__(self, weight=None, ignore_index=-1):
        super().__init__()
        if weight is not None or ignore_index != -1:
            raise NotImplementedError("only weight=None, ignore_index=-1 (the reference's setting)")
        self.ignore_index = ignore_index

    def forward(self, pred, target):
        low, hw = _fused_source(pred)
        return ops.ce_up(low, target.reshape(-1), hw)


def multi_level_guidance_ce(pred, pred_2, threshold):
    """CE(pred_2, label_2) with label_2 = (max P > thr | max P2 > thr) ? argmax((P+P2)/2) : -1,
    P = softmax(pred), P2 = softmax(pred_2)  (solve_gta5.py:206-213).  Gradient flows to pred_2 only."""
    low1, hw = _fused_source(pred_2)
    low2, hw2 = _fused_source(pred)
    if hw != hw2:
        raise ValueError("both heads must be upsampled to the same size")
    return ops.multi_ce_up(low1, low2.detach(), hw, threshold)


def pseudo_label_ce(pred, threshold):
    """The `hard` target mode (solve_gta5.py:185-199): CE(pred, label) with label = argmax softmax(pred)
    where its maximum > threshold, else ignored (label detached); nan with a zero gradient when no pixel
    passes (quirk Q8)."""
    low, hw = _fused_source(pred)
    return ops.hard_ce_up(low, hw, threshold)


class PseudoLabelCEClasswise(nn.Module):
    """The `hard` target mode with one threshold per class (--threshold_mode class): label = argmax
    softmax(pred) where its maximum > thr_dev[that class], else ignored, written as an int64 map by one
    launch (ops.pseudo_classwise) into a buffer this object owns; then the fused CE of the low-resolution
    logits with that map (ops.ce_up).  One launch more than pseudo_label_ce, no other loss kernel.
    `thr_dev` is a device fp32 [C] tensor the launch reads: a captured step follows new values.
    The CE's backward reads the buffer: run a call's backward before the same object's next forward."""

    def __init__(self):
        super().__init__()
        self.labels = None  # int64 [ho*wo], allocated on the first call and whenever the size changes

    def forward(self, pred, thr_dev):
        low, hw = _fused_source(pred)
        n = int(hw[0]) * int(hw[1])
        if self.labels is None or self.labels.numel() != n or self.labels.device != low.device:
            self.labels = torch.empty(n, dtype=torch.int64, device=low.device)
        ops.pseudo_classwise(thr_dev, hw, low.detach(), label=self.labels)
        return ops.ce_up(low, self.labels, hw)


def pseudo_label_ce_classwise(pred, thr_dev):
    """PseudoLabelCEClasswise as a function, with a label map of its own per call: the CE's backward reads the
    map its forward saved, so two losses formed before either backward must not share one.  A trainer keeps one
    PseudoLabelCEClasswise instead (one forward, then its backward, per step: a static buffer for a captured
    step)."""
    return PseudoLabelCEClasswise()(pred, thr_dev)
