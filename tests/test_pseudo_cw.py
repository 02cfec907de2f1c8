"""Class-balanced pseudo-label thresholds without a GPU: the C ABI's new entry points (header, library, ctypes
table), the flags of the trainer and the tools, the numpy restatement (tests/pseudo_cw_ref.py) on hand-built
histograms and against the reference's own `hard` rule (tests/target_modes_ref.py), and the checkpoint key."""
import argparse
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pseudo_cw_ref as ref
import target_modes_ref as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("msl_confidence_hist", "msl_confidence_hist_tta", "msl_class_thresholds", "msl_pseudo_classwise",
       "msl_pseudo_classwise_tta")


# ----------------------------------------------------------------------------- the C ABI
def test_header_declares_and_library_exports_the_entry_points():
    from maxsquareloss_amd import hip
    header = open(os.path.join(ROOT, "include", "msl_hip.h")).read()
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert hasattr(lib, name), name
        assert name in hip.SIGNATURES
    lib.msl_abi_version.restype = ctypes.c_int
    assert lib.msl_abi_version() == 3 == hip.ABI_VERSION  # entry points were added, none changed
    assert len(hip.SIGNATURES["msl_confidence_hist"][1]) == 10
    assert len(hip.SIGNATURES["msl_confidence_hist_tta"][1]) == 8
    assert len(hip.SIGNATURES["msl_class_thresholds"][1]) == 8
    assert hip.SIGNATURES["msl_class_thresholds"][1][3] is ctypes.c_double  # portion is fp64
    assert len(hip.SIGNATURES["msl_pseudo_classwise"][1]) == 11
    assert len(hip.SIGNATURES["msl_pseudo_classwise_tta"][1]) == 9


# ----------------------------------------------------------------------------- flags
def test_trainer_flags_and_defaults():
    from maxsquareloss_amd.tools import ADAIN, solve_crosscity, solve_gta5
    for mod in (solve_gta5, solve_crosscity, ADAIN):
        a = mod.build_parser().parse_args([])
        assert (a.threshold_mode, a.pseudo_portion, a.threshold_bins, a.threshold_images) == ("fixed", 0.5, 512, 500)
    p = solve_gta5.build_parser()
    assert p.parse_args([]).threshold == 0.95
    a = p.parse_args(["--target_mode", "hard", "--threshold_mode", "class", "--pseudo_portion", "0.3",
                      "--threshold_bins", "64", "--threshold_images", "0", "--threshold", "0.9"])
    assert (a.threshold_mode, a.pseudo_portion, a.threshold_bins, a.threshold_images, a.threshold) == \
        ("class", 0.3, 64, 0, 0.9)
    help_text = p.format_help()
    assert "--multi's guidance label" in " ".join(help_text.split())


HARD_CLASS = ["--threshold_mode", "class", "--target_mode", "hard"]


@pytest.mark.parametrize("argv,message", [
    (["--threshold_mode", "class"], "--threshold_mode class needs --target_mode hard, not "),  # each tool's default
    (["--threshold_mode", "class", "--target_mode", "maxsquare"], "needs --target_mode hard, not maxsquare"),
    (["--threshold_mode", "class", "--target_mode", "IW_entropy"], "needs --target_mode hard, not IW_entropy"),
    (["--threshold_mode", "quantile", "--target_mode", "hard"], "invalid choice: 'quantile'"),
    (HARD_CLASS + ["--threshold_bins", "100"], "--threshold_bins 100 must be a power of two"),
    (HARD_CLASS + ["--threshold_bins", "2048"], "--threshold_bins 2048 must be a power of two"),
    (HARD_CLASS + ["--threshold_bins", "1024"], "num_classes * bins <= 16384"),         # 19 * 1024 cells
    (HARD_CLASS + ["--pseudo_portion", "1.5"], "--pseudo_portion 1.5 must lie in [0, 1]"),
    (HARD_CLASS + ["--threshold", "0"], "--threshold 0.0 must lie in (0, 1]"),
    (HARD_CLASS + ["--threshold_images", "-1"], "--threshold_images must not be negative"),
])
def test_trainer_flags_that_are_parser_errors(argv, message, capsys):
    from maxsquareloss_amd.tools import ADAIN, solve_crosscity, solve_gta5
    for mod in (solve_gta5, solve_crosscity, ADAIN):
        if "<= 16384" in message and mod.build_parser().parse_args([]).num_classes * 1024 <= 16384:
            continue  # solve_crosscity.py: 13 classes by default, whose 1024-bin tile fits
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(argv)
        assert message in capsys.readouterr().err, mod.__name__
    # the same values are fine where the mode does not read them, and the hook is installed once per parser
    p = solve_gta5.build_parser()
    assert p.parse_args(["--threshold_bins", "100"]).threshold_mode == "fixed"
    assert len(p._msl_checks) == 1
    assert p.parse_args(HARD_CLASS + ["--num_classes", "16", "--threshold_bins", "1024"]).threshold_bins == 1024


def test_the_pass_loader_leaves_the_training_loader_alone(tmp_path):
    """The file-backed statistics pass (utils/thresholds.py pass_loader): the training dataset copied with the val
    transform - resize only, no mirror, no crop -, the list order, and a random stream of its own: after the pass
    walked its items, stopping early, the training loader draws the plans it would have drawn without it."""
    pytest.importorskip("PIL")
    import test_input_pipeline as tip
    from maxsquareloss_amd.datasets import City_DataLoader
    from maxsquareloss_amd.utils.thresholds import first_items, pass_loader
    paths, made = tip.write_tree(tmp_path, n=3, val_n=2)
    cfg = {"chain_cfg": [40, 30, 50, 36, 33, 20, 70, 44]}

    def loader():
        return City_DataLoader(tip.chain_args(cfg), training=True, datasets_path={"Cityscapes": paths}).data_loader

    def plans(ld, n):
        out = []
        while len(out) < n:  # epochs of the seeded permutation, plans drawn on this thread
            out += [(ident, plan) for _, _, plan, ident, _ in ld.host_items()]
        return out[:n]

    undisturbed, train = loader(), loader()
    assert train.shuffle and train.dataset.is_train() and train.dataset.random_mirror and train.dataset.random_crop
    want = plans(undisturbed, 9)
    got = plans(train, 3)
    ps = pass_loader(train, seed=0)
    assert ps.dataset is not train.dataset and ps.dataset.rng is not train.dataset.rng and not ps.shuffle
    assert ps.dataset.items is train.dataset.items and not ps.dataset.is_train()
    for n in (2, 0, 5):  # an early stop, the whole list, more than the list holds
        walked = [(ident, plan) for _, _, plan, ident, _ in first_items(_Host(ps), n)]
        assert [i for i, _ in walked] == list(range(len(ps)))[:n or None]
        assert all(plan == (False, [((33, 20), None)]) for _, plan in walked)  # seg_size, no mirror, no crop
    got += plans(train, 6)
    assert got == want and train.epoch == undisturbed.epoch
    assert len({steps[0][1] for _, (_, steps) in want}) > 1  # the training plans do draw crops from the stream


def test_the_pass_loader_on_an_unlabelled_nthu_train_list(tmp_path):
    """An NTHU city's train list has no label files, and its dataset tells labelled from `training`: the pass's
    copy, whose training flag is off, must still read the images alone."""
    pytest.importorskip("PIL")
    import argparse
    import jpeg_ref
    from maxsquareloss_amd.datasets import CrossCity_DataLoader
    from maxsquareloss_amd.utils import jpeg
    from maxsquareloss_amd.utils.thresholds import first_items, pass_loader
    paths, made = jpeg_ref.nthu_tree(tmp_path / "N", n=3, val_n=2, png_item=1)

    def loader():
        args = argparse.Namespace(base_size=(48, 32), crop_size=(40, 24), seg_size=(48, 32), random_mirror=True,
                                  random_crop=True, resize=True, DA=False, seed=3, split="train", class_16=False,
                                  class_13=True, batch_size=1, data_loader_workers=0, jpeg_decode="device")
        return CrossCity_DataLoader(args, training=True, datasets_path=paths).data_loader

    def plans(ld, n):
        out = []
        while len(out) < n:
            out += [(ident, plan[:2]) for _, _, plan, ident, _ in ld.host_items()]
        return out[:n]

    undisturbed, train = loader(), loader()
    assert train.dataset.is_train() and not train.dataset.labelled() and train.dataset.decode(0)[1] is None
    want = plans(undisturbed, 9)
    got = plans(train, 3)
    ps = pass_loader(train, seed=3)
    assert not ps.dataset.is_train() and not ps.dataset.labelled() and not ps.shuffle
    assert ps.dataset.paths(0)[1] is None and not train.dataset.labelled()
    for n in (2, 0):
        walked = list(first_items(_Host(ps), n))
        assert [ident for _, _, _, ident, _ in walked] == list(range(3))[:n or None]
        for rgb, ids, plan, ident, _ in walked:
            assert ids is None and jpeg.is_payload(rgb) == (ident != 1)            # item 1 is stored as a .png
            assert plan[:2] == (False, [((48, 32), None)])                        # base_size, no mirror, no crop
    got += plans(train, 6)
    assert got == want and train.epoch == undisturbed.epoch
    assert len({steps[0][1] for _, (_, steps) in want}) > 1


class _Host:
    """A DeviceLoader's host side as an iterable with a length: what first_items walks, without the device."""

    def __init__(self, loader):
        self.loader = loader

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        return self.loader.host_items()


def test_wrappers_refuse_a_call_without_a_source():
    from maxsquareloss_amd import hip, ops
    hist = torch.zeros(19, 64, dtype=torch.int64)
    with pytest.raises(hip.MSLError, match="give low"):
        ops.confidence_hist(hist, (7, 9))
    with pytest.raises(hip.MSLError, match="give low"):
        ops.pseudo_classwise(torch.zeros(19), (7, 9))
    with pytest.raises(hip.MSLError, match="not both"):
        ops.confidence_hist(hist, (7, 9), low=torch.zeros(1, 19, 3, 3), entries=[])


def _write_thresholds(path, n):
    rows = [dict(name=str(k), pixels=10, share=1.0 / n, quantile=0.5, threshold=0.5 + 0.01 * k, kept_share=0.5)
            for k in range(n)]
    with open(path, "w") as f:
        json.dump({"bins": 64, "portion": 0.5, "thr_max": 0.9, "images": 1, "classes": rows}, f)


def test_class_thresholds_flag_of_the_tools(tmp_path, capsys):
    from maxsquareloss_amd.hip import MSLError
    from maxsquareloss_amd.tools import evaluate, predict, pseudo_thresholds
    from maxsquareloss_amd.utils.thresholds import load_class_thresholds
    good, bad = str(tmp_path / "t19.json"), str(tmp_path / "t16.json")
    _write_thresholds(good, 19)
    _write_thresholds(bad, 16)
    for mod in (evaluate, predict):
        a = mod.build_parser().parse_args([])
        assert a.class_thresholds is None and a.class_threshold_values is None
        a = mod.build_parser().parse_args(["--class_thresholds", good, "--save_predictions", "d", "--save_kinds",
                                           "pseudo,color"])
        req = evaluate.output_request(a)
        assert req.class_thresholds == pytest.approx([0.5 + 0.01 * k for k in range(19)]) and req.threshold == 0.95
        with pytest.raises(SystemExit):  # 16 classes in the file, --num_classes 19
            mod.build_parser().parse_args(["--class_thresholds", bad])
        assert "16 classes" in capsys.readouterr().err
        assert mod.build_parser().parse_args(["--class_thresholds", bad, "--num_classes", "16"]).class_threshold_values
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(["--class_thresholds", str(tmp_path / "missing.json")])
        capsys.readouterr()
    with pytest.raises(MSLError, match="16 classes"):
        load_class_thresholds(bad, 19)
    assert evaluate.output_request(evaluate.build_parser().parse_args(["--save_predictions", "d"])).class_thresholds is None
    # the tool's own flags
    a = pseudo_thresholds.build_parser().parse_args([])
    assert (a.pseudo_portion, a.threshold_bins, a.threshold_images, a.threshold, a.flip, a.graph) == \
        (0.5, 512, 0, 0.95, False, False)
    with pytest.raises(SystemExit):
        pseudo_thresholds.build_parser().parse_args(["--threshold_bins", "48"])


def test_validator_refuses_a_wrong_class_count():
    from maxsquareloss_amd.hip import MSLError
    from maxsquareloss_amd.utils.images import OutputRequest
    from maxsquareloss_amd.utils.validate import Validator
    req = OutputRequest("d", ("pseudo",), class_thresholds=[0.5] * 16)
    with pytest.raises(MSLError, match="16 classes"):
        Validator(None, 19, (33, 65), 1, torch.device("cpu"), data=[], outputs=req)
    v = Validator(None, 16, (33, 65), 1, torch.device("cpu"), data=[], outputs=req)
    assert v._class_thr.dtype == torch.float32 and v._class_thr.numel() == 16


# ----------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("case", ref.hand_cases(), ids=lambda c: c[0])
def test_thresholds_ref_on_hand_built_histograms(case):
    name, hist, portion, thr_max, want = case
    thr, kept, q = ref.thresholds_ref(hist, portion, thr_max)
    C, bins = hist.shape
    n = hist.sum(axis=1)
    assert thr.dtype == np.float32 and (thr <= np.float32(thr_max)).all()
    assert (thr[n == 0] == np.float32(thr_max)).all()                       # an empty class gets the cap
    if want is not None:
        assert np.array_equal(thr, np.asarray(want, np.float32)), (name, thr)
    suf = ref.suffix(hist)
    for k in range(C):
        b = int(np.float32(thr[k]) * np.float32(bins))
        assert kept[k] == hist[k, b:].sum()
        need = int(np.ceil(portion * float(n[k])))
        assert kept[k] >= need                                              # at least `portion` of the class is kept
        if need > 0:                                                        # and one bin higher would keep too little
            b = int(q[k] * bins)
            assert suf[k, b] >= need and suf[k, b + 1] < need               # suf[k, bins] is 0
    if portion == 0.0:
        assert (thr == np.float32(thr_max)).all()
    if portion == 1.0:                                                      # the lowest occupied bin's edge, or the cap
        for k in np.nonzero(n)[0]:
            low = int(np.nonzero(hist[k])[0][0])
            assert thr[k] == min(np.float32(thr_max), np.float32(low) / np.float32(bins))


def test_bin_rule_is_fp32_and_clamped():
    top = np.array([0.0, 1.0, 0.5, np.float32(0.99999994), 1.0 / 64, np.nextafter(np.float32(1.0 / 64), np.float32(0))],
                   np.float32)
    assert ref.bin_of(top, 64).tolist() == [0, 63, 32, 63, 1, 0]
    near, j = ref.near_bin_edge(np.array([0.5, 0.5 + 2e-5, 1.0, 0.0, np.nan, 0.25 - 5e-6], np.float32), 64)
    assert near.tolist() == [True, False, False, False, False, True] and j[0] == 32 and j[5] == 16


@pytest.mark.parametrize("shape", ref.SHAPES[:4] + [ref.LIMIT_SHAPE])
@pytest.mark.parametrize("flip", [False, True])
def test_near_edge_pixels_are_few_and_small_shapes_have_empty_classes(shape, flip):
    npx = shape[3] * shape[4]
    for bins in ref.BINS:
        r = ref.hist_ref(shape, flip, bins)
        print(f"{shape} flip={flip} bins={bins}: near-edge {r['near']} of {npx}, most on one edge "
              f"{int(r['edge_count'].sum(axis=0).max())}, empty classes {int((r['hist'].sum(axis=1) == 0).sum())}")
        assert r["near"] <= ref.near_cap(npx)
        assert r["hist"].sum() == r["valid"] == npx
    if not flip and shape in ref.SHAPES[:2]:
        assert (ref.hist_ref(shape, flip, 64)["hist"].sum(axis=1) == 0).any()  # exercises N == 0


@pytest.mark.parametrize("thr", tm.THRESHOLDS)
def test_uniform_thresholds_are_the_hard_rule(thr):
    """With every thr[k] equal to the scalar threshold, labels_ref is the reference's own pseudo-label
    (solve_gta5.py:185-199 through tests/target_modes_ref.py)."""
    import evaluate_ref as ev
    for C in (19, 16):
        low, _, hw = tm.case_a(C)
        cls = ev.predict_ref(low, hw)[0]
        top = F.softmax(tm.up(low, hw), dim=1)[0].numpy().reshape(C, -1).max(axis=0)
        got = ref.labels_ref(cls, top, np.full(C, thr, np.float32))
        want = tm.fused_ref(low, hw, "hard", thr)["label"].reshape(-1)
        assert np.array_equal(got, want)
        assert 0 < (got >= 0).sum() < got.size
        # and a per-class vector decides class by class
        vec = np.where(np.arange(C) % 2 == 0, np.float32(thr), np.float32(1.0))
        mixed = ref.labels_ref(cls, top, vec)
        assert (mixed[cls % 2 == 1] == -1).all() and np.array_equal(mixed[cls % 2 == 0], want[cls % 2 == 0])


# ----------------------------------------------------------------------------- the checkpoint key
class _Opt:
    def __init__(self):
        self.state = {"k": 1}

    def state_dict(self):
        return dict(self.state)

    def load_state_dict(self, sd):
        self.state = dict(sd)


def test_checkpoint_round_trip_of_the_class_thresholds_key(tmp_path):
    from maxsquareloss_amd.utils.checkpoint import load_checkpoint, save_checkpoint
    model = torch.nn.Conv2d(3, 4, 1)
    thr = torch.tensor([0.9, 0.5, 0.25, 0.8125], dtype=torch.float32)
    fixed, cls = str(tmp_path / "fixed.pth"), str(tmp_path / "class.pth")
    save_checkpoint(fixed, model, _Opt(), 3, 40, 0.5)
    save_checkpoint(cls, model, _Opt(), 3, 40, 0.5, class_thresholds=thr)
    raw = torch.load(fixed, weights_only=True)
    assert sorted(raw) == ["best_MIou", "epoch", "iteration", "optimizer", "state_dict"]  # as before this mode
    assert sorted(torch.load(cls, weights_only=True)) == ["best_MIou", "class_thresholds", "epoch", "iteration",
                                                          "optimizer", "state_dict"]
    got = load_checkpoint(fixed, torch.nn.Conv2d(3, 4, 1), _Opt())
    assert got == {"epoch": 3, "iteration": 40, "best_MIou": 0.5}
    got = load_checkpoint(cls, torch.nn.Conv2d(3, 4, 1), _Opt())
    assert torch.equal(got.pop("class_thresholds"), thr) and got == {"epoch": 3, "iteration": 40, "best_MIou": 0.5}
