"""Every fused-loss, upsample and resize kernel form against fp64, through maxsquareloss_amd.ops (GPU only).

One test over tests/loss_form_cases.py TABLE: the operation's forward, then backward(gout), compared with
tests/loss_ref.py - fp64 on the CPU with the fp32 interpolation weights that define the operation.  Bars:
  the loss value              1e-5 relative, nan exactly where the reference is nan;
  every decision              the histogram, the labels and the argmax maps bit for bit, every pixel (the inputs keep
                              each decision MARGIN clear of flipping: test_loss_forms.py::test_decision_margins);
  the gradient, globally      max |d - ref| <= 1e-5 max |ref|;
  the gradient, locally       |d - ref|[e] <= K 2^-24 A[e] for every element, A the reference's local error scale
                              (loss_ref), and exactly 0 wherever A is 0: low-res columns no pixel reads when
                              shrinking, fully ignored regions, a threshold nobody passes;
  the upsample / resize       |y - ref| <= 4 2^-24 sum |w| |x| forward, K = 3 backward (derived: loss_form_cases);
  run to run                  every output bit-identical across two runs.
K of each loss kind and the measured ratios are in profiles/loss_forms_errors.txt (loss_form_cases.K).
"""
import math
import os

import pytest
import torch

import loss_form_cases as lc
import loss_ref as lr

pytestmark = pytest.mark.gpu

from maxsquareloss_amd import hip, ops  # noqa: E402

DEV = "cuda"
BAR = 1e-5
WORST = {}  # K's kind -> (worst local ratio, case id): printed by the last test


def _note(kind, ratio, cid):
    if ratio >= WORST.get(kind, (-1.0, ""))[0]:
        WORST[kind] = (ratio, cid)


def _same_bits(a, b, what):
    for x, y in zip(a, b):
        if x is None and y is None:
            continue
        assert torch.equal(x.cpu().view(torch.int32) if x.dtype == torch.float32 else x.cpu(),
                           y.cpu().view(torch.int32) if y.dtype == torch.float32 else y.cpu()), what + ": two runs differ"


def _loss_close(got, ref, what):
    if math.isnan(ref):
        assert math.isnan(got), "%s: loss %r where the reference is nan" % (what, got)
    else:
        assert abs(got - ref) <= BAR * abs(ref), "%s: loss %.9g vs %.17g" % (what, got, ref)


def _grad_close(got, ref, a, k, kind, cid, name):
    ratio, zero = lr.local_ratio(got, ref, a)
    _note(kind, ratio, cid)
    print("%s %s: rel %.3e local ratio %.3f (K %d)" % (cid, name, lr.rel(got, ref) if ref.abs().max() > 0 else 0.0,
                                                       ratio, k))
    assert zero, "%s %s: not exactly 0 where no pixel contributes" % (cid, name)
    if ref.abs().max() > 0:
        assert lr.rel(got, ref) < BAR, "%s %s" % (cid, name)
    else:
        assert got.abs().max().item() == 0, "%s %s" % (cid, name)
    assert ratio <= k, "%s %s: |d - ref| reaches %.2f x 2^-24 A, K = %d" % (cid, name, ratio, k)


def _up_call(cs, low, other):
    hw = (cs.ho, cs.wo)
    return {"ce": lambda: ops.ce_up(low, other, hw), "maxsquare": lambda: ops.maxsquare_up(low, hw),
            "iw_maxsquare": lambda: ops.iw_maxsquare_up(low, hw, cs.ratio),
            "multi_ce": lambda: ops.multi_ce_up(low, other, hw, cs.thr), "entropy": lambda: ops.entropy_up(low, hw),
            "iw_entropy": lambda: ops.iw_entropy_up(low, hw, cs.ratio),
            "hard_ce": lambda: ops.hard_ce_up(low, hw, cs.thr)}[cs.kind]()


def _run_up(cs, refused):
    low = lc.logits(cs).to(DEV).requires_grad_()
    other = None
    if cs.kind == "ce":
        other = lc.ce_labels(cs).to(DEV)
    elif cs.kind == "multi_ce":
        other = lc.logits(cs, 1).to(DEV)
    out = _up_call(cs, low, other)
    loss, extra = (out[0], out[1:]) if isinstance(out, tuple) else (out, ())
    g = torch.tensor(cs.gout, device=DEV)
    if refused:
        with pytest.raises(hip.MSLError):
            loss.backward(g)
        torch.cuda.synchronize()
        assert low.grad is None
        return (loss.detach(), *extra, None)
    loss.backward(g)
    return (loss.detach(), *extra, low.grad)


def _check_decisions(cs, ref, low):
    """The decision maps the loss took, through the label entry points: every pixel."""
    hw = (cs.ho, cs.wo)
    flat = lambda t: t.reshape(-1).to(torch.int32)  # noqa: E731
    if cs.kind == "iw_maxsquare":
        arg, _ = ops.loss_labels_up(low, None, hw)
        assert torch.equal(arg.cpu(), flat(ref["arg"]))
    elif cs.kind == "multi_ce":
        _, lab = ops.loss_labels_up(low, lc.logits(cs, 1).to(DEV), hw, cs.thr)
        assert torch.equal(lab.cpu(), flat(ref["label"]))
    elif cs.kind == "hard_ce":
        assert torch.equal(ops.pseudo_labels_up(low, hw, cs.thr).cpu(), flat(ref["label"]))
    elif cs.kind == "iw_entropy":
        assert torch.equal(ops.logits_argmax_up(low, hw).cpu(), flat(ref["arg"]))


def _check_up(row):
    name, classes, cs = row
    cid = lc.case_id(row)
    ref = lc.reference(cs)
    refused = "lds_refused" in classes
    a, b = _run_up(cs, refused), _run_up(cs, refused)
    _same_bits(a, b, cid)
    _loss_close(a[0].item(), ref["loss"], cid)
    if cs.kind in ("iw_maxsquare", "iw_entropy"):
        hist, w = a[1].cpu(), a[2].cpu()
        assert torch.equal(hist.long(), ref["hist"]), cid + ": histogram"
        assert torch.equal(w == 1.0, (ref["w"] == 1.0)) or cs.ho * cs.wo == 1, cid + ": the weights' support"
        assert lr.rel(w, ref["w"]) < BAR, cid + ": class weights"
    _check_decisions(cs, ref, lc.logits(cs).to(DEV))
    if refused:  # the stream is usable after the refusal
        small = [r for r in lc.TABLE if r[2].op == "up" and r[2].kind == "maxsquare" and r[0].endswith(":19")][0]
        _check_up(small)
        return
    _grad_close(a[-1], ref["dlow"], ref["A"], lc.K[cs.kind], cs.kind, cid, "dlow")


def _check_upsample(row):
    _, classes, cs = row
    cid = lc.case_id(row)
    x, gy = lc.upsample_inputs(cs)
    hw = (cs.ho, cs.wo)
    yr, s = lr.upsample_fwd(x, hw)
    dxr, a = lr.upsample_bwd(gy, cs.hi, cs.wi)
    runs = []
    for _ in range(2):
        xg = x.to(DEV).requires_grad_()
        y = ops.upsample_bilinear(xg, hw)
        if "lds_refused" in classes:
            with pytest.raises(hip.MSLError):
                y.backward(gy.to(DEV))
            assert xg.grad is None
        else:
            y.backward(gy.to(DEV))
        runs.append((y.detach(), xg.grad))
    _same_bits(*runs, cid)
    y, dx = runs[0]
    err = (y.double().cpu() - yr).abs()
    assert bool((err <= lc.K_UPSAMPLE_FWD * lr.EPS32 * s).all()), "%s: forward off by %.2f x 2^-24 sum |w||x|" % (
        cid, (err / (lr.EPS32 * s).clamp_min(1e-300)).max().item())
    if dx is not None:
        _grad_close(dx, dxr, a, lc.K_UPSAMPLE_BWD, "upsample", cid, "dx")


def _check_resize(row):
    cs = row[2]
    x, _ = lc.upsample_inputs(cs)
    yr, s = lr.upsample_fwd(x, (cs.ho, cs.wo))
    ys = [ops.resize_bilinear(x.to(DEV), (cs.ho, cs.wo)) for _ in range(2)]
    _same_bits(ys[:1], ys[1:], lc.case_id(row))
    err = (ys[0].double().cpu() - yr).abs()
    ratio = (err / (lr.EPS32 * s).clamp_min(1e-300)).max().item()
    _note("resize", ratio, lc.case_id(row))
    assert bool((err <= lc.K_UPSAMPLE_FWD * lr.EPS32 * s).all()), "%s: off by %.2f x 2^-24 sum |w||x|" % (
        lc.case_id(row), ratio)


def _check_labels(row):
    cs = row[2]
    hw = (cs.ho, cs.wo)
    low, low2 = lc.logits(cs).to(DEV), lc.logits(cs, 1).to(DEV)
    flat = lambda t: t.reshape(-1).to(torch.int32)  # noqa: E731
    if cs.op == "labels" and "solo" in cs.data:
        arg = lr.up_labels(lc.logits(cs), None, hw, cs.thr)[0]
        for _ in range(2):
            only, none = ops.loss_labels_up(low, None, hw, cs.thr)
            assert none is None and torch.equal(only.cpu(), flat(arg))
    elif cs.op == "labels":
        arg, _, lab, _ = lr.up_labels(lc.logits(cs), lc.logits(cs, 1), hw, cs.thr)
        for _ in range(2):
            g_arg, g_lab = ops.loss_labels_up(low, low2, hw, cs.thr)
            assert torch.equal(g_arg.cpu(), flat(arg)) and torch.equal(g_lab.cpu(), flat(lab))
        only, none = ops.loss_labels_up(low, None, hw, cs.thr)
        assert none is None and torch.equal(only.cpu(), flat(arg))
    else:
        lab, _, arg, _ = lr.pseudo_labels(lc.logits(cs), hw, cs.thr)
        for _ in range(2):
            assert torch.equal(ops.pseudo_labels_up(low, hw, cs.thr).cpu(), flat(lab))
            assert torch.equal(ops.logits_argmax_up(low, hw).cpu(), flat(arg))


def _check_flat(row):
    cs = row[2]
    cid = lc.case_id(row)
    kind, outs, ref = lc.run_reference(cs)
    g = torch.tensor(cs.gout, device=DEV)
    tok = cs.data.split("+")
    runs = []
    for _ in range(2):
        if cs.op == "prob":
            p, lab = lc.flat_inputs(cs)
            pg = p.to(DEV).requires_grad_()
            out = ops.maxsquare_prob(pg) if cs.kind == "ms" else ops.iw_maxsquare_prob(
                pg, None if lab is None else lab.to(DEV), cs.ratio)
            grads = {"dprob": pg}
        else:
            x, t = lc.flat_inputs(cs)
            xg, tg = x.to(DEV), t.to(DEV)
            if "dt" not in tok:
                xg.requires_grad_()
            if "di" not in tok:
                tg.requires_grad_()
            out = ops.soft_ce(xg, tg) if cs.kind == "plain" else ops.iw_soft_ce(xg, tg, cs.ratio)
            grads = {"dinputs": xg, "dtarget": tg}
        loss, extra = (out[0], out[1:]) if isinstance(out, tuple) else (out, ())
        loss.backward(g)
        runs.append((loss.detach(), *extra, *(grads[n].grad for n in sorted(grads))))
    _same_bits(*runs, cid)
    _loss_close(runs[0][0].item(), ref["loss"], cid)
    if cs.kind == "iw":
        assert torch.equal(runs[0][1].cpu().long(), torch.as_tensor(ref["hist"]).long()), cid + ": histogram"
        assert lr.rel(runs[0][2], ref["w"]) < BAR, cid + ": class weights"
    for n, leaf in grads.items():
        if leaf.requires_grad:
            _grad_close(leaf.grad, outs[n][0], outs[n][1], lc.K[kind], kind, cid, n)
        else:
            assert leaf.grad is None


CHECK = {"up": _check_up, "upsample": _check_upsample, "resize": _check_resize, "labels": _check_labels,
         "pseudo": _check_labels, "prob": _check_flat, "soft": _check_flat}


@pytest.mark.parametrize("row", [pytest.param(r, id=lc.case_id(r)) for r in lc.TABLE])
def test_case_against_fp64(row):
    pl = lc.plans(hip, row[2])
    assert (lc.name_of(row[2], pl), lc.classes_of(row[2], pl)) == row[:2]  # the library still plans it as filed
    CHECK[row[2].op](row)


def test_refused_class_counts_raise():
    """C = 33 through a loss and through msl_upsample_bwd, C = 5 through resize_bilinear: refused before any launch."""
    low = torch.randn(1, 33, 3, 5, device=DEV, requires_grad=True)
    with pytest.raises(hip.MSLError):
        ops.maxsquare_up(low, (7, 11))
    y = ops.upsample_bilinear(low, (7, 11))  # the forward takes any class count
    yr, s = lr.upsample_fwd(low.detach().cpu(), (7, 11))
    assert bool(((y.detach().double().cpu() - yr).abs() <= lc.K_UPSAMPLE_FWD * lr.EPS32 * s).all())
    with pytest.raises(hip.MSLError):
        y.backward(torch.ones_like(y))
    assert low.grad is None
    with pytest.raises(hip.MSLError):
        ops.resize_bilinear(torch.randn(1, 5, 3, 5, device=DEV), (7, 11))
    torch.cuda.synchronize()


def test_zz_report_measured_ratios():
    """The worst local ratio per kind over the cases that ran (with -s; MSL_LOSS_FORMS_REPORT=path also writes it)."""
    lines = ["%-13s gpu worst ratio %8.3f  K %s   %s" % (k, r, lc.K.get(k, {"upsample": lc.K_UPSAMPLE_BWD,
                                                                             "resize": lc.K_UPSAMPLE_FWD}.get(k)), cid)
             for k, (r, cid) in sorted(WORST.items())]
    print("\n".join(lines))
    path = os.environ.get("MSL_LOSS_FORMS_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
