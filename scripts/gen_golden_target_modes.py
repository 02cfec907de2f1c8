"""Golden vectors of the entropy / IW_entropy / hard target modes - runs only where the reference is present.

Loads the reference's utils/loss.py by file path (as oracle/gen_golden.py does; the file itself only needs
torch), runs its softCrossEntropy / IWsoftCrossEntropy modules and a restatement of the trainer's hard
pseudo-label lines (solve_gta5.py:185-199) around nn.CrossEntropyLoss on the inputs of
tests/target_modes_ref.py, and writes their OUTPUTS to tests/golden/target_modes_kat.npz (the tests
regenerate the inputs).  No reference source leaves that machine.

    python scripts/gen_golden_target_modes.py --ref PATH_TO_THE_REFERENCE_CHECKOUT

Keys (t = 0p95 | 0p5):
  A{C}_*  C in {19, 16, 13}: loss_kat.npz's C{C}_low, (9,17) -> (64,128)
  B_*     counter_normal(79, "tm_wide_19"), (5,65) -> (33,513)
      ent, ent_dlow            softCrossEntropy()(pred, softmax(pred)), d low
      iwent, iwent_dlow, iwent_hist, argmax_logits     IWsoftCrossEntropy(ratio 0.2), same call
      hard{t}_label, hard{t}_ce, hard{t}_dlow          the hard mode at threshold t
  A{C}_soft*, A{C}_iwsoft*     the modules on explicit tensors (ref.explicit_pair): loss, summaries of
                               d inputs / d target (chsum, abssum, sample), iwsoft_hist
  M19_*   the same with target entries masked to -1 (ref.masked); allmasked_soft (nan), allmasked_iwsoft (0)
  tie_*   loss_kat.npz's tie_logits at identity interpolation: iwent, iwent_hist, argmax_logits, hard_ce (nan)
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import target_modes_ref as ref  # noqa: E402


def load_loss(ref_root):
    spec = importlib.util.spec_from_file_location("ref_loss", os.path.join(ref_root, "utils/loss.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def fused(ls, low, hw, prefix, out, thresholds=ref.THRESHOLDS):
    C = low.size(1)

    def run(fn):
        lr = low.clone().requires_grad_()
        pred = ref.up(lr, hw)
        loss = fn(pred)
        if torch.isfinite(loss):
            loss.backward()
        return loss.item(), (torch.zeros_like(low) if lr.grad is None else lr.grad).numpy(), pred.detach()

    l, d, pred = run(lambda pred: ls.softCrossEntropy()(pred, F.softmax(pred, dim=1)))
    out[prefix + "ent"], out[prefix + "ent_dlow"] = np.array(l, np.float32), d
    l, d, _ = run(lambda pred: ls.IWsoftCrossEntropy(num_class=C, ratio=ref.RATIO)(pred, F.softmax(pred, dim=1)))
    out[prefix + "iwent"], out[prefix + "iwent_dlow"] = np.array(l, np.float32), d
    _, arg = torch.max(pred, 1)
    out[prefix + "iwent_hist"] = torch.histc(arg.float(), bins=C, min=0, max=C - 1).numpy().astype(np.int64)
    out[prefix + "argmax_logits"] = arg.numpy().astype(np.int8)
    for thr in thresholds:
        labels = []

        def hard(pred):
            maxpred, label = torch.max(F.softmax(pred, dim=1).detach(), dim=1)
            label = torch.where(maxpred > thr, label, torch.ones(1, dtype=torch.long) * -1)
            labels.append(label)
            return torch.nn.CrossEntropyLoss(ignore_index=-1)(pred, label)

        l, d, _ = run(hard)
        t = ref.tag(thr)
        out[prefix + f"hard{t}_label"] = labels[0].numpy().astype(np.int8)
        out[prefix + f"hard{t}_ce"], out[prefix + f"hard{t}_dlow"] = np.array(l, np.float32), d


def explicit(ls, inputs, target, prefix, out):
    C = inputs.size(1)
    for name, mod in (("soft", ls.softCrossEntropy()), ("iwsoft", ls.IWsoftCrossEntropy(num_class=C, ratio=ref.RATIO))):
        x, t = inputs.clone().requires_grad_(), target.clone().requires_grad_()
        loss = mod(x, t)
        out[prefix + name] = np.array(loss.item(), np.float32)
        if not torch.isfinite(loss):
            continue
        loss.backward()
        for k, g in (("dinputs", x.grad), ("dtarget", t.grad)):
            for kk, v in ref.summary(g).items():
                out[f"{prefix}{name}_{k}_{kk}"] = v
    _, arg = torch.max(inputs, 1)
    out[prefix + "iwsoft_hist"] = torch.histc(arg.float(), bins=C, min=0, max=C - 1).numpy().astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference repository's checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    if not os.path.isdir(a.ref):
        print("reference not present; the golden file is committed, nothing to do")
        return
    ls = load_loss(a.ref)
    out = {}
    for C in (19, 16, 13):
        low, _, hw = ref.case_a(C)
        fused(ls, low, hw, f"A{C}_", out)
        explicit(ls, *ref.explicit_pair(C), f"A{C}_", out)
    low, hw = ref.case_b()
    fused(ls, low, hw, "B_", out)
    tie, hw = ref.case_tie()
    tmp = {}
    fused(ls, tie, hw, "tie_", tmp, thresholds=(0.95,))
    for k in ("iwent", "iwent_dlow", "iwent_hist", "argmax_logits"):
        out["tie_" + k] = tmp["tie_" + k]
    out["tie_hard_ce"] = tmp["tie_hard0p95_ce"]  # max p = e / (2e + 17) = 0.12: nobody passes
    inputs, target = ref.explicit_pair(19)
    explicit(ls, inputs, ref.masked(target), "M19_", out)
    tmp = {}
    explicit(ls, inputs, torch.full_like(target, -1.0), "allmasked_", tmp)
    out["allmasked_soft"], out["allmasked_iwsoft"] = tmp["allmasked_soft"], tmp["allmasked_iwsoft"]
    path = os.path.join(a.out, "target_modes_kat.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
