"""Inputs and an fp64 restatement of the entropy / IW-entropy / hard target modes (utils/loss.py:17-67,
solve_gta5.py:185-199 of the reference), shared by tests/test_target_modes.py (which pins it to
tests/golden/target_modes_kat.npz, the reference's own outputs), tests/test_gpu_target_modes.py (its second
opinion) and scripts/gen_golden_target_modes.py (which regenerates the same inputs).

Decisions (argmax, threshold, histogram, IW weights) are taken in fp32 on torch-CPU's upsampled logits, as
the reference takes them; the sums and gradients are fp64 autograd of the closed forms.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from maxsquareloss_amd.utils.synthetic import counter_normal

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
THRESHOLDS = (0.95, 0.5)
RATIO = 0.2
SAMPLES = 1024


def gold(name):
    return np.load(os.path.join(GOLD, name), allow_pickle=False)


def tag(thr):
    return str(thr).replace(".", "p")


def case_a(C):
    """(low (1,C,9,17), low2, hw): the loss KAT's logits."""
    g = gold("loss_kat.npz")
    return torch.from_numpy(g[f"C{C}_low"]), torch.from_numpy(g[f"C{C}_low2"]), (64, 128)


def case_b():
    """Wi = 65 >= 64: two column chunks in the backward's row kernel."""
    low = torch.from_numpy(counter_normal(79, "tm_wide_19", 19 * 5 * 65, 4.0)).view(1, 19, 5, 65)
    return low, (33, 513)


def case_tie():
    tie = torch.from_numpy(gold("loss_kat.npz")["tie_logits"])
    return tie, tuple(tie.shape[2:])


def up(low, hw):
    return F.interpolate(low, size=hw, mode="bilinear", align_corners=True)


def explicit_pair(C):
    """(inputs, target) of the explicit-tensor cases: the upsampled KAT logits and the softmax of the
    second KAT tensor's (a target that is not softmax(inputs), so d inputs does not vanish)."""
    low, low2, hw = case_a(C)
    return up(low, hw), F.softmax(up(low2, hw), dim=1)


def masked(target):
    """Every 7th element (flat index % 7 == 3) set to the ignore value -1."""
    t = target.clone().reshape(-1)
    t[3::7] = -1.0
    return t.view_as(target)


def sample_idx(n):
    return np.unique(np.linspace(0, n - 1, SAMPLES).astype(np.int64))


def summary(t):
    """fp64 per-channel sums, |.| sum and sampled elements of a (1,C,H,W) tensor."""
    a = t.detach().double().cpu().numpy()
    flat = a.reshape(-1)
    return {"chsum": a.reshape(a.shape[1], -1).sum(1), "abssum": np.array(np.abs(a).sum()),
            "sample": flat[sample_idx(flat.size)].astype(np.float32)}


def iw_weights(arg, C, ratio=RATIO):
    """hist of the argmax map and w = 1 / max(hist^r * (sum hist)^(1-r), 1), fp32 (loss.py:58-61)."""
    hist = torch.bincount(arg.reshape(-1), minlength=C).float()
    w = 1.0 / torch.max(torch.pow(hist, ratio) * torch.pow(hist.sum(), 1 - ratio), torch.ones(1))
    return hist.long(), w


def _grad(loss, leaf):
    if not torch.isfinite(loss):
        return torch.zeros_like(leaf)
    (g,) = torch.autograd.grad(loss, leaf)
    return g


def fused_ref(low, hw, mode, thr=None, ratio=RATIO):
    """fp64 loss and d low of one target mode, with the fp32 decisions: dict(loss, dlow[, hist, arg, label])."""
    C = low.size(1)
    out = {}
    pred32 = up(low, hw)
    l64 = low.double().requires_grad_()
    v = up(l64, hw)
    lp = F.log_softmax(v, dim=1)
    p = lp.exp()
    if mode == "entropy":
        loss = (-lp * p).sum() / (C * hw[0] * hw[1])
    elif mode == "IW_entropy":
        arg = pred32.argmax(1)
        hist, w = iw_weights(arg, C, ratio)
        loss = ((-lp * p).sum(1) * w.double()[arg]).sum() / C
        out.update(hist=hist.numpy(), arg=arg.numpy())
    elif mode == "hard":
        maxp, label = torch.max(F.softmax(pred32, dim=1), dim=1)
        label = torch.where(maxp > thr, label, torch.full_like(label, -1))
        keep = label >= 0
        picked = -lp.gather(1, label.clamp(min=0).unsqueeze(1)).squeeze(1)
        loss = (picked * keep).sum() / keep.sum()  # 0 / 0 = nan when nothing passes
        out.update(label=label.numpy())
    else:
        raise ValueError(mode)
    out.update(loss=loss.item(), dlow=_grad(loss, l64))
    return out


def soft_ref(inputs, target, ignore=-1.0, ratio=None):
    """fp64 softCrossEntropy (ratio None) / IWsoftCrossEntropy on explicit tensors: dict(loss, dinputs,
    dtarget[, hist])."""
    C = inputs.size(1)
    x = inputs.double().requires_grad_()
    m = target != ignore
    t = torch.where(m, target, torch.zeros_like(target)).double().requires_grad_()
    lp = F.log_softmax(x, dim=1)
    terms = -lp * t * m
    out = {}
    if ratio is None:
        loss = terms.sum() / m.sum()
    else:
        arg = inputs.argmax(1)
        hist, w = iw_weights(arg, C, ratio)
        loss = (terms.sum(1) * w.double()[arg]).sum() / C
        out.update(hist=hist.numpy())
    if torch.isfinite(loss):
        dx, dt = torch.autograd.grad(loss, (x, t))
    else:
        dx, dt = torch.zeros_like(x), torch.zeros_like(t)
    out.update(loss=loss.item(), dinputs=dx, dtarget=dt * m)
    return out
