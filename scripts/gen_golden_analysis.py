"""TEST INFRASTRUCTURE - writes tests/golden/analysis_kat.npz from the reference's own code.

As scripts/gen_golden_predict_images.py does, this script reads the source text of the reference's
utils/eval.py (whose imports pull in torchvision, so it cannot be imported whole), takes the three SYNTHIA
index lists and the class `Eval` out of it by AST and runs them unmodified: per matrix, what
tools/analysis.py:176-183 reads per image - Pixel_Accuracy, Mean_Pixel_Accuracy,
Mean_Intersection_over_Union and Frequency_Weighted_Intersection_over_Union.  Only data is written; no
reference source enters the repository.  Needs the reference checkout (--ref).

Keys, for k = 0 .. count-1:
  count       the number of matrices
  cm_{k}      int64 [C, C], C in {1, 13, 16, 19, 32}
  scores_{k}  float64: [PA, MPA, MIoU, FWIoU]; for C = 16 the reference returns (16-class, 13-class) tuples:
              [PA, MPA_16, MIoU_16, FWIoU_16, MPA_13, MIoU_13, FWIoU_13]
"""
import argparse
import ast
import os
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = ("synthia_set_16", "synthia_set_13", "synthia_set_16_to_13")


def load(ref_root):
    tree = ast.parse(open(os.path.join(ref_root, "utils", "eval.py")).read())
    env = {"np": np, "name_classes": []}
    body = [n for n in tree.body
            if (isinstance(n, ast.Assign) and any(isinstance(t, ast.Name) and t.id in NAMES for t in n.targets))
            or (isinstance(n, ast.ClassDef) and n.name == "Eval")]
    exec(compile(ast.Module(body=body, type_ignores=[]), "<ref>", "exec"), env)
    return env


def matrices():
    out = []
    for C in (1, 13, 16, 19, 32):
        rng = np.random.default_rng(4200 + C)
        for kind in ("dense", "sparse", "absent", "only_predicted", "zero", "big"):
            m = rng.integers(0, 3000, size=(C, C)).astype(np.int64)
            m[np.arange(C), np.arange(C)] += rng.integers(0, 20000, size=C)
            if kind == "sparse":
                m[rng.random((C, C)) < 0.7] = 0
            elif kind == "absent" and C > 1:
                m[C // 3, :] = 0
                m[:, C // 3] = 0
            elif kind == "only_predicted":
                m[C - 1, :] = 0
            elif kind == "zero":
                m[:] = 0
            elif kind == "big":
                m += np.int64(1) << 40
            out.append(m)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    Eval = load(a.ref)["Eval"]
    np.seterr(divide="ignore", invalid="ignore")  # utils/eval.py:8
    warnings.simplefilter("ignore")               # nanmean of an all-NaN slice; np.sum of a generator
    out = {}
    mats = matrices()
    for k, m in enumerate(mats):
        ev = Eval(m.shape[0])
        ev.confusion_matrix += m  # the float64 matrix add_batch accumulates into
        PA, MPA, MIoU, FWIoU = (ev.Pixel_Accuracy(), ev.Mean_Pixel_Accuracy(), ev.Mean_Intersection_over_Union(),
                                ev.Frequency_Weighted_Intersection_over_Union())
        if m.shape[0] == 16:
            scores = [PA, MPA[0], MIoU[0], FWIoU[0], MPA[1], MIoU[1], FWIoU[1]]
        else:
            scores = [PA, MPA, MIoU, FWIoU]
        out[f"cm_{k}"], out[f"scores_{k}"] = m, np.array(scores, np.float64)
    out["count"] = np.int64(len(mats))
    path = os.path.join(a.out, "analysis_kat.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(mats), "matrices,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
