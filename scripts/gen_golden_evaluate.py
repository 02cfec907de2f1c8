"""Golden text of Eval.Print_Every_class_Eval - runs only where the reference is present.

Loads the reference's utils/eval.py by file path.  That module imports `name_classes` from
datasets.cityscapes_Dataset, whose own imports (the data files' loaders) are not needed here: a stub module of
that name is registered first, holding the `name_classes` list read out of the reference's file as a literal
(ast, nothing executed).  The reference's Eval then prints its per-class table for the fixed matrices of
tests/evaluate_ref.py (kat_matrix), and the captured text is written to tests/golden/evaluate_kat.npz together
with the matrices.  No reference source leaves that machine.

    python scripts/gen_golden_evaluate.py --ref PATH_TO_THE_REFERENCE_CHECKOUT

Keys: cm{C} (float64 [C, C]), table19, table19_16_13, table16 (the printed text), name_classes.
"""
import argparse
import ast
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import evaluate_ref as ref  # noqa: E402


def read_name_classes(ref_root):
    tree = ast.parse(open(os.path.join(ref_root, "datasets", "cityscapes_Dataset.py")).read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "name_classes" for t in node.targets):
            return list(ast.literal_eval(node.value))
    raise RuntimeError("name_classes not found in the reference's datasets/cityscapes_Dataset.py")


def load_eval(ref_root, names):
    pkg, stub = types.ModuleType("datasets"), types.ModuleType("datasets.cityscapes_Dataset")
    stub.name_classes = names
    pkg.cityscapes_Dataset = stub
    sys.modules["datasets"], sys.modules["datasets.cityscapes_Dataset"] = pkg, stub
    spec = importlib.util.spec_from_file_location("ref_eval", os.path.join(ref_root, "utils", "eval.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference repository's checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    if not os.path.isdir(a.ref):
        print("reference not present; the golden file is committed, nothing to do")
        return
    names = read_name_classes(a.ref)
    mod = load_eval(a.ref, names)
    out = {"name_classes": np.array(names)}
    for C, out_16_13 in ref.KAT_CASES:
        ev = mod.Eval(C)
        ev.confusion_matrix = ref.kat_matrix(C)
        out[f"cm{C}"] = ev.confusion_matrix
        out[ref.kat_key(C, out_16_13)] = np.array(ref.table_text(ev, out_16_13))
    path = os.path.join(a.out, "evaluate_kat.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")
    print(str(out["table19_16_13"]))


if __name__ == "__main__":
    main()
