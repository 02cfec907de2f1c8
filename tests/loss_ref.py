"""An fp64 restatement of what csrc/loss.hip computes for the training side: the bilinear upsample, the seven fused
losses on upsampled logits with their gradients, and the prob-input and soft forms - plain torch and numpy.

Interpolation is the definition: the align_corners weights are torch's fp32 ones (the scale (in-1)/(out-1), the
product s*o, the floor, lambda and 1 - lambda all rounded to fp32), held in dense matrices Wy [Ho x Hi] and
Wx [Wo x Wi].  Everything after the weights is fp64: up = Wy L Wx^T, the softmax, each loss by its formula
(utils/loss.py and the trainer lines csrc/loss.hip cites), the gradient by double autograd through the matrices.

Every decision a loss takes (an argmax, a threshold, a histogram) comes back with a per-pixel margin - the gap of
the top two, the distance of the maximum from the threshold - so that a test can require its inputs to keep the
decisions clear of fp32 rounding instead of excusing pixels.  Every gradient comes back with a local error scale
A[e] = (Wy^T M Wx)[e]: M[px] is the magnitude of the pixel's gradient coefficient, so A is what one ulp of
relative error in every pixel's gradient could add up to in a low-resolution element, and exactly 0 where no
pixel contributes.
"""
import numpy as np
import torch
import torch.nn.functional as F

import target_modes_ref as tm

UP_KINDS = ("ce", "maxsquare", "iw_maxsquare", "multi_ce", "entropy", "iw_entropy", "hard_ce")
EPS32 = 2.0 ** -24


# ------------------------------------------------------------------------------------------ interpolation
def lin_taps(n_in, n_out, ft=np.float32):
    """lin() of csrc/loss.hip for every output index, every step rounded to `ft` (fp32 as the kernels and torch's
    fp32 path; np.float64: the weights torch's double path takes): (i0, i1 int64, w0, w1)."""
    s = ft(n_in - 1) / ft(n_out - 1) if n_out > 1 else ft(0)
    real = (s * np.arange(n_out, dtype=ft)).astype(ft)
    i0 = np.minimum(np.floor(real).astype(np.int64), n_in - 1)
    lam = np.minimum(np.maximum(real - i0.astype(ft), ft(0)), ft(1)).astype(ft)
    i1 = i0 + (i0 < n_in - 1)
    return i0, i1, (ft(1) - lam).astype(ft), lam


WEIGHTS = [np.float32]  # the precision of the interpolation weights (test_loss_forms.py switches it to compare with
                        # torch's double path)


def dense(n_in, n_out):
    """The [n_out x n_in] interpolation matrix of the fp32 weights, as fp64."""
    i0, i1, w0, w1 = lin_taps(n_in, n_out, WEIGHTS[0])
    w = np.zeros((n_out, n_in))
    o = np.arange(n_out)
    np.add.at(w, (o, i0), w0.astype(np.float64))
    np.add.at(w, (o, i1), w1.astype(np.float64))
    return torch.from_numpy(w)


def upsample(low, hw):
    """Wy L Wx^T of a double (C, Hi, Wi) tensor -> (C, Ho, Wo)."""
    wy, wx = dense(low.shape[-2], hw[0]), dense(low.shape[-1], hw[1])
    return torch.matmul(torch.matmul(wy, low), wx.t())


def pull(m, hi, wi):
    """Wy^T M Wx of per-pixel magnitudes (.., Ho, Wo) -> (.., Hi, Wi)."""
    wy, wx = dense(hi, m.shape[-2]), dense(wi, m.shape[-1])
    return torch.matmul(torch.matmul(wy.t(), m), wx)


# ------------------------------------------------------------------------------------------ decisions
def top_gap(x):
    """(first-max argmax, top value, gap of the top two) over dim 0; the gap is inf with one class."""
    top, arg = torch.max(x, 0)  # torch.max returns the first maximum
    if x.shape[0] == 1:
        return arg, top, torch.full_like(top, float("inf"))
    two = torch.topk(x, 2, dim=0).values
    return arg, top, two[0] - two[1]


def iw_weights(arg, c, ratio):
    """hist of the class map and w = 1 / max(hist^r * (sum hist)^(1-r), 1) (loss.py:58-61, :92-95), fp64."""
    hist = torch.bincount(arg.reshape(-1), minlength=c).double()
    w = 1.0 / torch.clamp(torch.pow(hist, ratio) * torch.pow(hist.sum(), 1.0 - ratio), min=1.0)
    return hist.long(), w


def decide(kind, v, v2=None, labels=None, thr=None, ratio=None):
    """The decisions of one loss on fp64 upsampled logits v (C, Ho, Wo): a dict with `margin` (Ho, Wo) and, by
    kind, `label` (-1 = ignored), `arg`, `hist`, `w`."""
    c = v.shape[0]
    p = F.softmax(v, 0)
    inf = torch.full(v.shape[1:], float("inf"), dtype=torch.float64)
    if kind == "ce":
        y = labels.reshape(v.shape[1:])
        return {"label": torch.where((y >= 0) & (y < c), y, torch.full_like(y, -1)), "margin": inf}
    if kind in ("maxsquare", "entropy"):
        return {"margin": inf}
    if kind in ("iw_maxsquare", "iw_entropy"):
        arg, _, gap = top_gap(p if kind == "iw_maxsquare" else v)
        hist, w = iw_weights(arg, c, ratio)
        return {"arg": arg, "hist": hist, "w": w, "margin": gap}
    if kind == "hard_ce":
        arg, top, gap = top_gap(p)
        keep = top > thr
        return {"label": torch.where(keep, arg, torch.full_like(arg, -1)),
                "margin": torch.minimum((top - thr).abs(), torch.where(keep, gap, inf))}
    if kind == "multi_ce":  # P = softmax(up(low2)), P2 = softmax(up(low1)) (solve_gta5.py:206-212)
        big = F.softmax(v2, 0)
        m = torch.maximum(big.max(0).values, p.max(0).values)
        keep = m > thr
        arg, _, gap = top_gap((big + p) / 2)
        return {"label": torch.where(keep, arg, torch.full_like(arg, -1)),
                "margin": torch.minimum((m - thr).abs(), torch.where(keep, gap, inf))}
    raise ValueError(kind)


# ------------------------------------------------------------------------------------------ the losses
def loss_of(kind, v, dec):
    """The loss on upsampled logits v (C, Ho, Wo; any float dtype) under the decisions `dec`."""
    c, npx = v.shape[0], v.shape[1] * v.shape[2]
    lp = F.log_softmax(v, 0)
    p = lp.exp()
    if kind in ("ce", "multi_ce", "hard_ce"):
        lab = dec["label"]
        keep = lab >= 0
        picked = -lp.gather(0, lab.clamp(min=0).unsqueeze(0)).squeeze(0)
        return (picked * keep).sum() / keep.sum()  # 0 / 0 = nan when nothing is kept
    if kind == "maxsquare":
        return -(p * p).sum() / (2.0 * c * npx)
    if kind == "entropy":
        return (-lp * p).sum() / (c * npx)
    w = dec["w"].to(v.dtype)[dec["arg"]]
    if kind == "iw_maxsquare":
        return -((p * p).sum(0) * w).sum() / c
    return ((-lp * p).sum(0) * w).sum() / c


def coefficient(kind, v, dec, gout):
    """M[px]: the magnitude of the pixel's gradient coefficient (Ho, Wo), from the fp64 values."""
    c, npx = v.shape[0], v.shape[1] * v.shape[2]
    g = abs(float(gout))
    one = torch.ones(v.shape[1:], dtype=torch.float64)
    lp = F.log_softmax(v, 0)
    ent = (-lp * lp.exp()).sum(0)
    if kind in ("ce", "multi_ce", "hard_ce"):
        keep = dec["label"] >= 0
        return keep.double() * (g / max(int(keep.sum()), 1))
    if kind == "maxsquare":
        return one * (g / (c * npx))
    if kind == "entropy":
        return (1.0 + ent) * (g / (c * npx))
    w = dec["w"][dec["arg"]]
    if kind == "iw_maxsquare":
        return w * (2.0 * g / c)
    return w * (1.0 + ent) * (g / c)


def up_loss(kind, low, hw, low2=None, labels=None, thr=None, ratio=None, gout=1.0):
    """One fused loss of the upsampled logits in fp64.  low, low2: (1, C, Hi, Wi) fp32.  Returns dict(loss,
    dlow (1, C, Hi, Wi) - zero when the loss is nan, as the library's -, A (Hi, Wi), margin (Ho, Wo), and the
    decisions)."""
    l64 = low[0].double().requires_grad_()
    v = upsample(l64, hw)
    dec = decide(kind, v.detach(), None if low2 is None else upsample(low2[0].double(), hw), labels, thr, ratio)
    loss = loss_of(kind, v, dec)
    if torch.isfinite(loss):
        (d,) = torch.autograd.grad(loss * float(gout), l64)
        a = pull(coefficient(kind, v.detach(), dec, gout), low.shape[2], low.shape[3])
    else:
        d, a = torch.zeros_like(l64), torch.zeros(low.shape[2:], dtype=torch.float64)
    out = dict(dec)
    out.update(loss=loss.item(), dlow=d.unsqueeze(0), A=a)
    return out


def up_loss_fp32(kind, low, hw, dec, gout=1.0):
    """torch-CPU fp32 autograd of the same loss (F.interpolate, then the formulas in fp32) under the fp64
    decisions: the arithmetic the reference project runs.  Returns (loss, dlow)."""
    l32 = low.clone().requires_grad_()
    v = F.interpolate(l32, size=tuple(hw), mode="bilinear", align_corners=True)[0]
    loss = loss_of(kind, v, dec)
    if not torch.isfinite(loss):
        return loss.item(), torch.zeros_like(low)
    (d,) = torch.autograd.grad(loss * torch.tensor(float(gout)), l32)
    return loss.item(), d


def up_labels(low, low2, hw, thr):
    """(argmax of p, its margin, the multi-level label or None, its margin): msl_loss_labels_up."""
    v = upsample(low[0].double(), hw)
    arg, _, gap = top_gap(F.softmax(v, 0))
    if low2 is None:
        return arg, gap, None, None
    dec = decide("multi_ce", v, upsample(low2[0].double(), hw), thr=thr)
    return arg, gap, dec["label"], dec["margin"]


def pseudo_labels(low, hw, thr):
    """(hard label, its margin, argmax of the logits, its margin): msl_pseudo_labels_up."""
    v = upsample(low[0].double(), hw)
    dec = decide("hard_ce", v, thr=thr)
    arg, _, gap = top_gap(v)
    return dec["label"], dec["margin"], arg, gap


# ------------------------------------------------------------------------------------------ upsample / resize
def upsample_fwd(x, hw):
    """(y, S): the fp64 interpolation of x (1, C, Hi, Wi) and S = sum |w| |x| per output, the forward's scale."""
    x64 = x[0].double()
    return upsample(x64, hw).unsqueeze(0), upsample(x64.abs(), hw).unsqueeze(0)


def upsample_bwd(gy, hi, wi):
    """(dx, A): Wy^T g Wx of a hi-res gradient (1, C, Ho, Wo) in fp64 and A = sum |w| |g|."""
    g64 = gy[0].double()
    return pull(g64, hi, wi).unsqueeze(0), pull(g64.abs(), hi, wi).unsqueeze(0)


# ------------------------------------------------------------------------------------------ prob-input forms
def prob_loss(prob, iw, label=None, ratio=None, gout=1.0):
    """MaxSquareloss / IW_MaxSquareloss on a probability tensor (1, C, H, W) (loss.py:69-119): the histogram is
    of `label` when given, else of the argmax.  dict(loss, dprob, A, margin[, hist, w])."""
    p = prob[0].double().requires_grad_()
    c, npx = p.shape[0], p.shape[1] * p.shape[2]
    out = {}
    if not iw:
        loss = -(p * p).sum() / (2.0 * c * npx)
        coef = torch.full(p.shape[1:], abs(float(gout)) / (c * npx), dtype=torch.float64)
        out["margin"] = torch.full(p.shape[1:], float("inf"), dtype=torch.float64)
    else:
        arg, _, gap = top_gap(p.detach())
        src = arg if label is None else label.reshape(-1)
        hist, w = iw_weights(src[(src >= 0) & (src < c)], c, ratio)
        loss = -((p * p).sum(0) * w[arg]).sum() / c
        coef = w[arg] * (2.0 * abs(float(gout)) / c)
        out.update(hist=hist, w=w, margin=gap)
    (d,) = torch.autograd.grad(loss * float(gout), p)
    out.update(loss=loss.item(), dprob=d.unsqueeze(0), A=(coef * p.detach().abs()).unsqueeze(0))
    return out


def prob_loss_fp32(prob, iw, ref, gout=1.0):
    p = prob[0].clone().requires_grad_()
    c, npx = p.shape[0], p.shape[1] * p.shape[2]
    if not iw:
        loss = -(p * p).sum() / (2.0 * c * npx)
    else:
        loss = -((p * p).sum(0) * ref["w"].float()[p.detach().argmax(0)]).sum() / c
    (d,) = torch.autograd.grad(loss * torch.tensor(float(gout)), p)
    return loss.item(), d.unsqueeze(0)


# ------------------------------------------------------------------------------------------ soft forms
def soft_loss(inputs, target, ignore=-1.0, ratio=None, gout=1.0):
    """softCrossEntropy / IWsoftCrossEntropy on explicit tensors: target_modes_ref.soft_ref scaled by gout, with
    the local scales of both gradients: |a| (p S + |t|) for d inputs, |a| (1 + |x - max| + log sum) for d target
    (the terms the fp32 log-softmax is assembled from; the 1 is the sum's own relative rounding, which the
    log of a sum >= 1 turns into an absolute error), a the pixel's coefficient."""
    r = tm.soft_ref(inputs, target, ignore, ratio)
    c = inputs.size(1)
    x, t = inputs[0].double(), target[0].double()
    m = target[0] != ignore
    g = abs(float(gout))
    if ratio is None:
        n = int(m.sum())
        a = torch.full(x.shape[1:], g / n if n else 0.0, dtype=torch.float64)
    else:
        arg = inputs[0].argmax(0)
        a = iw_weights(arg, c, ratio)[1][arg] * (g / c)
        r["w"] = iw_weights(arg, c, ratio)[1]
    tk = torch.where(m, t, torch.zeros_like(t))
    p = F.softmax(x, 0)
    sh = x - x.max(0).values
    r.update(dinputs=r["dinputs"] * float(gout), dtarget=r["dtarget"] * float(gout),
             A_inputs=(a * (p * tk.sum(0) + tk.abs())).unsqueeze(0),
             A_target=(a * (1.0 + sh.abs() + sh.exp().sum(0).log()) * m).unsqueeze(0))
    return r


def soft_loss_fp32(inputs, target, ignore=-1.0, ratio=None, gout=1.0):
    """torch-CPU fp32 autograd of the same forms, as utils/loss.py writes them."""
    c = inputs.size(1)
    x = inputs.clone().requires_grad_()
    m = target != ignore
    t = torch.where(m, target, torch.zeros_like(target)).requires_grad_()
    terms = -F.log_softmax(x, 1) * t * m
    if ratio is None:
        loss = terms.sum() / m.sum()
    else:
        arg = inputs.argmax(1)
        loss = (terms.sum(1) * iw_weights(arg, c, ratio)[1].float()[arg]).sum() / c
    if not torch.isfinite(loss):
        return loss.item(), torch.zeros_like(inputs), torch.zeros_like(target)
    dx, dt = torch.autograd.grad(loss * torch.tensor(float(gout)), (x, t))
    return loss.item(), dx, dt * m


# ------------------------------------------------------------------------------------------ comparisons
def rel(got, ref):
    """The project's normwise bar: the largest error over the largest reference value."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def local_ratio(got, ref, a):
    """max over the elements of |got - ref| / (2^-24 A), and whether got is exactly 0 wherever A is 0."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    a = a.expand_as(ref) if a.dim() == ref.dim() else a.expand(ref.shape)
    err = (got - ref).abs()
    live = a > 0
    ratio = (err[live] / (EPS32 * a[live])).max().item() if live.any() else 0.0
    return ratio, bool((got[~live] == 0).all())
