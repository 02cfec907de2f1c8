"""CPU tests of the evaluator: the new C entry point's declaration, Eval.Print_Every_class_Eval against text
recorded from the reference's own Eval (tests/golden/evaluate_kat.npz, scripts/gen_golden_evaluate.py), the
tests' restatement of the per-pixel class (tests/evaluate_ref.py) against the oracle's argmax, and the new
flags' defaults."""
import os
import re

import numpy as np
import pytest

import evaluate_ref as ref
from oracle import msl_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_predict_up_declared_bound_and_exported():
    from maxsquareloss_amd import hip
    header = open(os.path.join(ROOT, "include", "msl_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+msl_predict_up\s*\(([^)]*)\)", header)
    assert m, "include/msl_hip.h declares msl_predict_up"
    assert len(m.group(1).split(",")) == 11
    res, args = hip.SIGNATURES["msl_predict_up"]
    assert res is hip.c_int and len(args) == 11 and args[-1] is hip.c_p
    assert args[2:7] == [hip.c_int] * 5 and all(a is hip.c_p for a in args[:2] + args[7:])
    assert hip.ABI_VERSION == 3  # purely additive
    assert hasattr(hip.load(require_gpu=False), "msl_predict_up")
    from maxsquareloss_amd import ops
    from maxsquareloss_amd.utils.eval import Eval
    assert callable(ops.predict_up) and callable(Eval.add_batch_low)


@pytest.mark.parametrize("C,out_16_13", ref.KAT_CASES)
def test_per_class_table_matches_the_reference_text(C, out_16_13, capsys):
    from maxsquareloss_amd.utils import eval as ev_mod
    g = ref.gold()
    cm = ref.kat_matrix(C)
    assert np.array_equal(cm, g[f"cm{C}"])  # the matrix the reference printed
    assert list(g["name_classes"]) == ev_mod.name_classes
    ev = ev_mod.Eval(C)
    ev.confusion_matrix = cm
    ev.Print_Every_class_Eval(out_16_13)
    text = capsys.readouterr().out
    want = str(g[ref.kat_key(C, out_16_13)])
    assert text == want
    lines = want.splitlines()
    assert len(lines) == 1 + (16 if (out_16_13 or C == 16) else C)
    assert "nan" in lines[4] and "nan" in lines[6] and "nan" in lines[8]  # classes 3, 5, 7


@pytest.mark.parametrize("C,hi,wi,ho,wo", ref.SHAPES[:4])
def test_restatement_no_flip_is_the_oracle_argmax(C, hi, wi, ho, wo):
    low = ref.logits(C, hi, wi, nan=True)
    lab = ref.labels(C, ho, wo)
    cls, near, top2 = ref.predict_ref(low, (ho, wo))
    cm, arg = orc.confusion(lab.numpy(), ref.up(low, (ho, wo))[0].numpy(), C)
    assert np.array_equal(cls, arg) and not near.any() and top2 is None
    assert np.array_equal(ref.confusion_ref(lab.numpy(), cls, C), cm)
    assert ref.up(low, (ho, wo)).isnan().any()  # the planted NaN reaches the prediction
    # the labels exercise both ignored ends and 255
    v = set(np.unique(lab.numpy()).tolist())
    assert {-1, C, 255} <= v and cm.sum() == int(((lab >= 0) & (lab < C)).sum())


def test_restatement_flip_mask_and_mirror():
    """The near-tie mask stays small at the small shapes, and the mirror is the one the reference applies:
    swapping the two inputs' roles mirrors the class map - (P + flip(Pf)) / 2 flipped is (Pf + flip(P)) / 2,
    the same sums bit for bit - at odd and even widths."""
    for C, hi, wi, ho, wo in ref.SHAPES[:4]:
        low, lowf = ref.logits(C, hi, wi), ref.logits(C, hi, wi, tag="Lf")
        cls, near, top2 = ref.predict_ref(low, (ho, wo), lowf)
        assert near.mean() <= 1e-3 and (top2[0] == cls).all()
        cls2, _, _ = ref.predict_ref(lowf, (ho, wo), low)
        assert np.array_equal(cls2.reshape(ho, wo)[:, ::-1], cls.reshape(ho, wo))
        assert not np.array_equal(cls2, cls)


def test_new_flags_default_off():
    import argparse
    from maxsquareloss_amd.tools.train_source import add_train_args
    from maxsquareloss_amd.tools import evaluate, solve_gta5
    assert add_train_args(argparse.ArgumentParser()).parse_args([]).val_images == 0
    assert solve_gta5.build_parser().parse_args([]).val_images == 0
    a = evaluate.build_parser().parse_args([])
    assert (a.flip, a.graph, a.val_images) == (False, False, 0)
    args, _, _ = evaluate.parse_args(["--target_crop_size", "256,128"])
    assert args.split == "val" and args.crop_size == (256, 128) == args.target_crop_size
