"""CPU tests of the entropy / IW_entropy / hard target modes: the public interface, and the tests' own fp64
restatement (tests/target_modes_ref.py) pinned to the reference's outputs in tests/golden/target_modes_kat.npz
(scripts/gen_golden_target_modes.py) - losses and gradients within 1e-5, labels and histograms exact - so
the second opinion tests/test_gpu_target_modes.py uses for the trainer is itself checked against the reference."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import target_modes_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["msl_entropy_up_fwd", "msl_entropy_up_bwd", "msl_iw_entropy_up_fwd", "msl_iw_entropy_up_bwd",
               "msl_hard_ce_up_fwd", "msl_hard_ce_up_bwd", "msl_pseudo_labels_up", "msl_soft_ce_fwd",
               "msl_soft_ce_bwd", "msl_iw_soft_ce_fwd", "msl_iw_soft_ce_bwd"]


def _rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def _params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values() if p.name != "self"]


def test_modules_have_the_reference_signatures():
    from maxsquareloss_amd.utils import loss
    assert _params(loss.softCrossEntropy.__init__) == [("ignore_index", -1)]
    assert _params(loss.IWsoftCrossEntropy.__init__) == [("ignore_index", -1), ("num_class", 19), ("ratio", 0.2)]
    for cls in (loss.softCrossEntropy, loss.IWsoftCrossEntropy):
        assert [n for n, _ in _params(cls.forward)] == ["inputs", "target"]
        assert issubclass(cls, torch.nn.Module)
    iw = loss.IWsoftCrossEntropy(num_class=16, ratio=0.5)
    assert (iw.ignore_index, iw.num_class, iw.ratio, iw.last_hist, iw.last_weights) == (-1, 16, 0.5, None, None)
    assert [n for n, _ in _params(loss.pseudo_label_ce)] == ["pred", "threshold"]


def test_ops_are_exported():
    from maxsquareloss_amd import ops
    for name in ("entropy_up", "iw_entropy_up", "hard_ce_up", "pseudo_labels_up", "soft_ce", "iw_soft_ce"):
        assert callable(getattr(ops, name)), name


@pytest.mark.parametrize("mode", ["entropy", "IW_entropy", "hard"])
def test_parser_and_trainer_accept_the_mode(mode):
    from maxsquareloss_amd.tools import solve_gta5
    args = solve_gta5.build_parser().parse_args(["--target_mode", mode])
    assert args.target_mode == mode
    src = inspect.getsource(solve_gta5.UDATrainer.__init__)
    assert f'"{mode}"' in src, "UDATrainer.__init__ routes the mode"


def test_new_entry_points_declared_and_signed():
    from maxsquareloss_amd import hip
    header = open(os.path.join(ROOT, "include", "msl_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert s in hip.SIGNATURES, s
        # every entry takes an explicit stream last and returns an int status
        assert hip.SIGNATURES[s][0] is hip.c_int and hip.SIGNATURES[s][1][-1] is hip.c_p, s
    assert hip.ABI_VERSION == 3  # purely additive
    lib = hip.load(require_gpu=False)
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s


def _check_fused(g, prefix, low, hw, thresholds):
    r = ref.fused_ref(low, hw, "entropy")
    assert r["loss"] == pytest.approx(float(g[prefix + "ent"]), rel=1e-5)
    assert _rel(r["dlow"], g[prefix + "ent_dlow"]) < 1e-5
    r = ref.fused_ref(low, hw, "IW_entropy")
    assert np.array_equal(r["hist"], g[prefix + "iwent_hist"])
    assert np.array_equal(r["arg"], g[prefix + "argmax_logits"].astype(np.int64))
    assert r["loss"] == pytest.approx(float(g[prefix + "iwent"]), rel=1e-5)
    assert _rel(r["dlow"], g[prefix + "iwent_dlow"]) < 1e-5
    for thr in thresholds:
        t = ref.tag(thr)
        r = ref.fused_ref(low, hw, "hard", thr)
        assert np.array_equal(r["label"], g[prefix + f"hard{t}_label"].astype(np.int64)), thr
        assert r["loss"] == pytest.approx(float(g[prefix + f"hard{t}_ce"]), rel=1e-5)
        assert _rel(r["dlow"], g[prefix + f"hard{t}_dlow"]) < 1e-5


@pytest.mark.parametrize("C", [19, 16, 13])
def test_restatement_reproduces_the_reference_case_a(C):
    g = ref.gold("target_modes_kat.npz")
    low, _, hw = ref.case_a(C)
    _check_fused(g, f"A{C}_", low, hw, ref.THRESHOLDS)
    hist = g[f"A{C}_iwent_hist"]
    assert hist.sum() == hw[0] * hw[1]  # no ignore bin
    for t, (lo, hi) in (("0p95", (0.02, 0.07)), ("0p5", (0.5, 0.6))):  # the thresholds cut, not all / none
        assert lo <= (g[f"A{C}_hard{t}_label"] >= 0).mean() <= hi


def test_restatement_reproduces_the_reference_wide_case():
    g = ref.gold("target_modes_kat.npz")
    low, hw = ref.case_b()
    assert low.size(3) >= 64  # more than one column chunk in k_bwd_rows
    _check_fused(g, "B_", low, hw, ref.THRESHOLDS)


def test_restatement_reproduces_the_reference_ties_and_degenerates():
    g = ref.gold("target_modes_kat.npz")
    tie, hw = ref.case_tie()
    r = ref.fused_ref(tie, hw, "IW_entropy")
    assert np.array_equal(r["hist"], g["tie_iwent_hist"]) and (g["tie_iwent_hist"] == 0).sum() == 17
    assert np.array_equal(r["arg"], g["tie_argmax_logits"].astype(np.int64))
    assert r["loss"] == pytest.approx(float(g["tie_iwent"]), rel=1e-5)
    assert _rel(r["dlow"], g["tie_iwent_dlow"]) < 1e-5
    r = ref.fused_ref(tie, hw, "hard", 0.95)
    assert np.isnan(r["loss"]) and np.isnan(float(g["tie_hard_ce"]))
    assert (r["label"] == -1).all() and torch.count_nonzero(r["dlow"]).item() == 0


def _check_explicit(g, prefix, inputs, target):
    for name, ratio in (("soft", None), ("iwsoft", ref.RATIO)):
        r = ref.soft_ref(inputs, target, ratio=ratio)
        assert r["loss"] == pytest.approx(float(g[prefix + name]), rel=1e-5)
        for k in ("dinputs", "dtarget"):
            s = ref.summary(r[k])
            assert _rel(s["sample"], g[f"{prefix}{name}_{k}_sample"]) < 1e-5, (name, k)
            assert np.abs(s["chsum"] - g[f"{prefix}{name}_{k}_chsum"]).max() < 1e-5 * float(g[f"{prefix}{name}_{k}_abssum"])
        if ratio is not None:
            assert np.array_equal(r["hist"], g[prefix + "iwsoft_hist"])


@pytest.mark.parametrize("C", [19, 16, 13])
def test_explicit_restatement_reproduces_the_reference(C):
    _check_explicit(ref.gold("target_modes_kat.npz"), f"A{C}_", *ref.explicit_pair(C))


def test_explicit_restatement_masked_targets():
    g = ref.gold("target_modes_kat.npz")
    inputs, target = ref.explicit_pair(19)
    tm = ref.masked(target)
    assert 0.1 < (tm == -1).float().mean().item() < 0.2
    _check_explicit(g, "M19_", inputs, tm)
    none = torch.full_like(target, -1.0)
    r = ref.soft_ref(inputs, none)
    assert np.isnan(r["loss"]) and np.isnan(float(g["allmasked_soft"]))
    assert torch.count_nonzero(r["dinputs"]).item() == 0 and torch.count_nonzero(r["dtarget"]).item() == 0
    assert ref.soft_ref(inputs, none, ratio=ref.RATIO)["loss"] == 0.0 == float(g["allmasked_iwsoft"])


def test_golden_file_is_small():
    assert os.path.getsize(os.path.join(ref.GOLD, "target_modes_kat.npz")) < 512 * 1024
