"""The entropy / IW_entropy / hard target modes on the HIP kernels (GPU only).

tests/golden/target_modes_kat.npz holds the reference's own outputs (utils/loss.py:17-67 and the trainer's
hard pseudo-label lines, solve_gta5.py:185-199; scripts/gen_golden_target_modes.py) on inputs this file
regenerates (tests/target_modes_ref.py):
  - the fused ops (ops.entropy_up / iw_entropy_up / hard_ce_up / pseudo_labels_up) on the loss KAT logits for
    C = 19 / 16 / 13, a wide case whose backward runs two column chunks, the argmax-tie logits and a threshold
    nobody passes: loss and d low within 1e-5, histogram, logits-argmax and pseudo-label maps bit-exact, nan
    with a zero gradient in the degenerate case (the bars of test_fused_losses_on_reference_kat);
  - the explicit-tensor forms (ops.soft_ce / iw_soft_ce) with plain, partly masked and fully masked targets;
  - run-to-run bit identity of every new op;
  - the trainer in each new mode at 128x256 (a 17x33 feature map) with --multi True: an eager and a --graph
    trainer bit-identical over 3 iterations, and iteration 0 against a CPU restatement built from the oracle's
    model and tests/target_modes_ref.py (itself pinned to the goldens by tests/test_target_modes.py).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import target_modes_ref as ref  # noqa: E402
from oracle import msl_oracle as orc  # noqa: E402
from maxsquareloss_amd import ops  # noqa: E402
from maxsquareloss_amd.tools.solve_gta5 import UDATrainer, build_parser  # noqa: E402
from maxsquareloss_amd.tools.train_source import init_args  # noqa: E402
from maxsquareloss_amd.utils import loss as L  # noqa: E402
from maxsquareloss_amd.utils.synthetic import synthetic_image, synthetic_labels  # noqa: E402

DEV = "cuda"


def _rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def _run(fn, low):
    lg = low.clone().requires_grad_()
    out = fn(lg)
    loss = out[0] if isinstance(out, tuple) else out
    loss.backward()
    torch.cuda.synchronize()
    return out, lg.grad


def _check_fused(g, prefix, low, hw, thresholds):
    low = low.to(DEV)
    out, d = _run(lambda t: ops.entropy_up(t, hw), low)
    assert out.item() == pytest.approx(float(g[prefix + "ent"]), rel=1e-5)
    assert _rel(d, g[prefix + "ent_dlow"]) < 1e-5
    (out, hist, w), d = _run(lambda t: ops.iw_entropy_up(t, hw, ref.RATIO), low)
    assert np.array_equal(hist.cpu().numpy().astype(np.int64), g[prefix + "iwent_hist"]), "IW-entropy histogram"
    want = g[prefix + "argmax_logits"].astype(np.int32)
    assert np.array_equal(ops.logits_argmax_up(low, hw).cpu().numpy().reshape(want.shape), want), "logits argmax"
    assert out.item() == pytest.approx(float(g[prefix + "iwent"]), rel=1e-5)
    assert _rel(d, g[prefix + "iwent_dlow"]) < 1e-5
    assert w.shape == (low.size(1),)
    for thr in thresholds:
        t = ref.tag(thr)
        want = g[prefix + f"hard{t}_label"].astype(np.int32)
        lab = ops.pseudo_labels_up(low, hw, thr)
        assert np.array_equal(lab.cpu().numpy().reshape(want.shape), want), f"pseudo-label thr {thr}"
        out, d = _run(lambda x: ops.hard_ce_up(x, hw, thr), low)
        assert out.item() == pytest.approx(float(g[prefix + f"hard{t}_ce"]), rel=1e-5)
        assert _rel(d, g[prefix + f"hard{t}_dlow"]) < 1e-5


@pytest.mark.parametrize("C", [19, 16, 13])
def test_fused_target_modes_on_reference_kat(C):
    low, _, hw = ref.case_a(C)
    _check_fused(ref.gold("target_modes_kat.npz"), f"A{C}_", low, hw, ref.THRESHOLDS)


def test_fused_target_modes_wide_case():
    """Wi = 65: rows_chunks = 2, so pixels on the chunk border are formed by both chunks of k_bwd_rows."""
    low, hw = ref.case_b()
    _check_fused(ref.gold("target_modes_kat.npz"), "B_", low, hw, ref.THRESHOLDS)


def test_ties_and_nobody_passes():
    g = ref.gold("target_modes_kat.npz")
    tie, hw = ref.case_tie()
    tie = tie.to(DEV)
    want = g["tie_argmax_logits"].astype(np.int32)
    assert np.array_equal(ops.logits_argmax_up(tie, hw).cpu().numpy().reshape(want.shape), want), \
        "first-max argmax on exact ties"
    (out, hist, w), d = _run(lambda t: ops.iw_entropy_up(t, hw, ref.RATIO), tie)
    assert np.array_equal(hist.cpu().numpy().astype(np.int64), g["tie_iwent_hist"])
    assert (w.cpu().numpy()[g["tie_iwent_hist"] == 0] == 1.0).all()  # empty classes: w = 1
    assert out.item() == pytest.approx(float(g["tie_iwent"]), rel=1e-5)
    assert _rel(d, g["tie_iwent_dlow"]) < 1e-5
    # max p = 0.12 everywhere: no pixel passes 0.95 -> nan loss (quirk Q8) and a zero gradient
    assert (ops.pseudo_labels_up(tie, hw, 0.95) == -1).all()
    out, d = _run(lambda t: ops.hard_ce_up(t, hw, 0.95), tie)
    assert np.isnan(out.item()) and np.isnan(float(g["tie_hard_ce"]))
    assert torch.count_nonzero(d).item() == 0


def _explicit(fn, inputs, target):
    x, t = inputs.to(DEV).requires_grad_(), target.to(DEV).requires_grad_()
    out = fn(x, t)
    loss = out[0] if isinstance(out, tuple) else out
    loss.backward()
    torch.cuda.synchronize()
    return out, x.grad, t.grad


def _check_explicit(g, prefix, inputs, target):
    for name, mod in (("soft", L.softCrossEntropy()), ("iwsoft", L.IWsoftCrossEntropy(num_class=19, ratio=ref.RATIO))):
        out, dx, dt = _explicit(mod, inputs, target)
        assert out.item() == pytest.approx(float(g[prefix + name]), rel=1e-5), name
        for k, d in (("dinputs", dx), ("dtarget", dt)):
            s = ref.summary(d)
            assert _rel(s["sample"], g[f"{prefix}{name}_{k}_sample"]) < 1e-5, (name, k)
            assert np.abs(s["chsum"] - g[f"{prefix}{name}_{k}_chsum"]).max() < 1e-5 * float(g[f"{prefix}{name}_{k}_abssum"])
        if name == "iwsoft":
            assert np.array_equal(mod.last_hist.cpu().numpy().astype(np.int64), g[prefix + "iwsoft_hist"])
            assert mod.last_weights.shape == (19,)
        # the whole tensors against the fp64 restatement (pinned to the same goldens on the CPU)
        r = ref.soft_ref(inputs, target, ratio=None if name == "soft" else ref.RATIO)
        assert _rel(dx, r["dinputs"]) < 1e-5 and _rel(dt, r["dtarget"]) < 1e-5, name


def test_explicit_forms_on_reference_kat():
    _check_explicit(ref.gold("target_modes_kat.npz"), "A19_", *ref.explicit_pair(19))


def test_explicit_forms_masked_targets():
    g = ref.gold("target_modes_kat.npz")
    inputs, target = ref.explicit_pair(19)
    _check_explicit(g, "M19_", inputs, ref.masked(target))
    none = torch.full_like(target, -1.0)
    out, dx, dt = _explicit(L.softCrossEntropy(), inputs, none)
    assert np.isnan(out.item()) and np.isnan(float(g["allmasked_soft"]))
    assert torch.count_nonzero(dx).item() == 0 and torch.count_nonzero(dt).item() == 0
    out, dx, dt = _explicit(L.IWsoftCrossEntropy(), inputs, none)
    assert out.item() == 0.0 == float(g["allmasked_iwsoft"])
    assert torch.count_nonzero(dx).item() == 0 and torch.count_nonzero(dt).item() == 0


def test_fused_path_equals_explicit_path():
    """softCrossEntropy()(pred) (fused from the low-res logits) against softCrossEntropy()(pred, softmax(pred))
    on the upsampled tensor: the interpolation is bit-identical, only the summation order (and torch's
    softmax rounding) differs - 1e-6 relative; likewise the IW form, whose histograms must be equal."""
    low, _, hw = ref.case_a(19)
    low = low.to(DEV)
    pred = ops.upsample_bilinear(low, hw)
    assert ops.low_of(pred) is low
    plain = pred.detach().clone()  # no low-res source behind it: the explicit kernels read it as is
    fused = L.softCrossEntropy()(pred)
    expl = L.softCrossEntropy()(plain, F.softmax(plain, dim=1))
    assert fused.item() == pytest.approx(expl.item(), rel=1e-6)
    mf, me = L.IWsoftCrossEntropy(), L.IWsoftCrossEntropy()
    fused, expl = mf(pred), me(plain, F.softmax(plain, dim=1))
    assert fused.item() == pytest.approx(expl.item(), rel=1e-6)
    assert torch.equal(mf.last_hist, me.last_hist) and torch.equal(mf.last_weights, me.last_weights)
    # a plain hi-res tensor through the fused path is the identity interpolation: same loss again
    assert L.softCrossEntropy()(plain).item() == pytest.approx(L.softCrossEntropy()(pred).item(), rel=1e-6)
    hard_f, hard_p = L.pseudo_label_ce(pred, 0.5), L.pseudo_label_ce(plain, 0.5)
    assert hard_f.item() == pytest.approx(hard_p.item(), rel=1e-6)


def test_new_ops_are_bit_reproducible():
    low, hw = ref.case_b()
    low = low.to(DEV)
    inputs, target = (t.to(DEV) for t in ref.explicit_pair(19))
    tm = ref.masked(target.cpu()).to(DEV)
    fused = {"entropy": lambda t: ops.entropy_up(t, hw), "iw_entropy": lambda t: ops.iw_entropy_up(t, hw, ref.RATIO),
             "hard": lambda t: ops.hard_ce_up(t, hw, 0.5)}
    for name, fn in fused.items():
        (a, da), (b, db) = _run(fn, low), _run(fn, low)
        a, b = (a[0], b[0]) if isinstance(a, tuple) else (a, b)
        assert a.item() == b.item() and torch.equal(da, db), name
    for name, fn in (("soft", lambda x, t: ops.soft_ce(x, t)), ("iwsoft", lambda x, t: ops.iw_soft_ce(x, t, ref.RATIO))):
        (a, ax, at), (b, bx, bt) = _explicit(fn, inputs, tm), _explicit(fn, inputs, tm)
        a, b = (a[0], b[0]) if isinstance(a, tuple) else (a, b)
        assert a.item() == b.item() and torch.equal(ax, bx) and torch.equal(at, bt), name


# ----------------------------------------------------------------------------- trainer
H, W = 128, 256  # a 17x33 feature map, the conv KATs' size
LAMBDA_T = 0.09


def _trainer(mode, graph):
    argv = ["--crop_size", f"{W},{H}", "--target_crop_size", f"{W},{H}", "--imagenet_pretrained", "False",
            "--save_dir", "", "--target_mode", mode, "--multi", "True", "--lambda_target", str(LAMBDA_T),
            "--iter_max", "1000", "--graph", str(graph)]
    args, _, _ = init_args(build_parser().parse_args(argv))
    tr = UDATrainer(args, cuda=True)
    tr.optimizer.zero_grad()
    return tr


def _inputs(it):
    return synthetic_image(H, W, 40 + it), synthetic_labels(H, W, 19, 40 + it), synthetic_image(H, W, 540 + it)


def _state(tr):
    return ([p.detach().clone() for p in tr.model.parameters()] + [b.detach().clone() for b in tr.model.buffers()] +
            [tr.optimizer.state[p]["momentum_buffer"].detach().clone() for p in tr.optimizer._uniq
             if p in tr.optimizer.state])


def _hard_slack(low, hw, thr, scale, eps=5e-4):
    """How far the hard mode's CE may move under rounding-level logit changes (as test_gpu_model's
    _guidance_slack): a pixel whose max probability is within eps of the threshold may enter or leave the
    kept set, one whose two top classes are within eps may change label; each moves the mean by at most its
    worst CE among the two top classes plus the mean itself, over the kept count."""
    mean = ref.fused_ref(low, hw, "hard", thr)["loss"]
    with torch.no_grad():
        v = ref.up(low, hw)
        P = F.softmax(v, 1)
        top2, cls2 = P.topk(2, dim=1)
        keep = top2[:, 0] > thr
        risk = ((top2[:, 0] - thr).abs() < eps) | (keep & (top2[:, 0] - top2[:, 1] < eps))
        worst = (-F.log_softmax(v, 1)).gather(1, cls2).max(1)[0]
        return scale * float(((worst + mean) * risk).sum()) / max(int(keep.sum()), 1)


@pytest.mark.parametrize("mode", ["entropy", "IW_entropy", "hard"])
def test_trainer_mode_eager_graph_and_oracle(mode):
    """An eager and a --graph trainer, same init and images, 3 iterations (the last two replayed): losses,
    the IW histogram, every parameter, buffer and momentum buffer bit-identical.  Iteration 0 against the
    CPU restatement: loss_seg and loss_target at 1e-3, the IW-entropy histogram within 0.2 % of
    the pixels in L1, the hard CE with the slack of the pixels within rounding of a decision."""
    eager, graphed = _trainer(mode, False), _trainer(mode, True)
    assert graphed.use_graph and not eager.use_graph
    names = [n for n, _ in eager.model.named_parameters()] + [n for n, _ in eager.model.named_buffers()]
    model = orc.Model({k: v.cpu().clone() for k, v in eager.model.state_dict().items()})
    thr = eager.args.threshold
    for it in range(3):
        xs, ys, xt = _inputs(it)
        for tr in (eager, graphed):
            tr.uda_step(xs.cuda(), ys.cuda(), xt.cuda())
        torch.cuda.synchronize()
        for name in ("loss_val", "loss_target", "loss_target_2"):
            a, b = getattr(graphed, name).item(), getattr(eager, name).item()
            assert a == b or (np.isnan(a) and np.isnan(b)), (it, name, a, b)
        if mode == "IW_entropy":
            assert torch.equal(graphed.target_loss.last_hist, eager.target_loss.last_hist), it
        sa, sb = _state(graphed), _state(eager)
        diff = next((names[i] if i < len(names) else i for i, (x, y) in enumerate(zip(sa, sb))
                     if not torch.equal(x, y)), None)
        assert diff is None, (it, diff)
        if it == 0:
            with torch.no_grad():
                bufs = {k: v.clone() for k, v in model.buffers.items()}  # (train mode updates the running stats)
                src2, _ = orc.forward(model.params, bufs, xs, conv=model.conv)
                low2, _ = orc.forward_low(model.params, bufs, xt, True, model.conv)
            assert eager.loss_val.item() == pytest.approx(orc.ce(src2, ys).item(), rel=1e-3)
            r = ref.fused_ref(low2, (H, W), mode, thr, ratio=eager.args.IW_ratio)
            slack = _hard_slack(low2, (H, W), thr, LAMBDA_T) if mode == "hard" else 0.0
            assert np.isfinite(r["loss"]) and r["loss"] > 0
            assert eager.loss_target.item() == pytest.approx(LAMBDA_T * r["loss"], rel=1e-3, abs=slack), slack
            if mode == "IW_entropy":
                h = eager.target_loss.last_hist.cpu().numpy().astype(np.int64)
                assert h.sum() == H * W and np.abs(h - r["hist"]).sum() <= 2 * 0.001 * H * W
    assert graphed._graphed is not None and graphed._graphed.replays == 2
    for name in ("loss_seg_value", "loss_target_value", "loss_target_value_2"):
        a, b = getattr(graphed, name).item(), getattr(eager, name).item()
        assert a == b or (np.isnan(a) and np.isnan(b)), name
