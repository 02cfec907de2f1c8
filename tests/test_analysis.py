"""CPU tests of the per-image analysis: the two new C entry points' declarations and their argument refusals
(which return before any launch, so they run without a GPU), the tool's flags, the reference's file names, and
the numpy restatement the GPU tests compare against (tests/analysis_ref.py) - against the host `Eval` on the
hand-made matrices and against scores recorded from the reference's own `Eval`
(tests/golden/analysis_kat.npz, scripts/gen_golden_analysis.py)."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

import analysis_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -3


# ----------------------------------------------------------------------------- C-ABI
@pytest.mark.parametrize("name,nargs", [("msl_image_metrics", 8), ("msl_analysis_maps", 15)])
def test_entry_points_declared_bound_and_exported(name, nargs):
    from maxsquareloss_amd import hip
    header = open(os.path.join(ROOT, "include", "msl_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header)
    assert m, f"include/msl_hip.h declares {name}"
    params = [p.strip() for p in m.group(1).split(",")]
    res, args = hip.SIGNATURES[name]
    assert res is hip.c_int and len(params) == len(args) == nargs and args[-1] is hip.c_p

    def ctype(p):  # the ctypes type of one declared parameter
        if "*" in p or "msl_stream_t" in p:
            return hip.c_p
        return {"int": hip.c_int, "float": hip.c_f, "double": hip.c_d,
                "long long": hip.c_ll}[p.rsplit(" ", 1)[0].replace("const ", "")]

    assert [ctype(p) for p in params] == args
    lib = hip.load(require_gpu=False)
    assert hasattr(lib, name) and lib.msl_abi_version() == 3 == hip.ABI_VERSION
    from maxsquareloss_amd import ops
    assert callable(ops.image_metrics) and callable(ops.analysis_maps)
    assert len(ops.METRICS_HEAD) == ref.HEAD and ops.ANALYSIS_MAPS == ("label", "pred", "input", "error")


def _buf(nbytes=64):
    """Host memory standing in for a device pointer: a refused call never reads it."""
    b = ctypes.create_string_buffer(nbytes)
    return b, ctypes.addressof(b)


def test_image_metrics_refuses_bad_arguments_before_any_launch():
    from maxsquareloss_amd import hip
    lib = hip.load(require_gpu=False)
    keep, p = _buf()

    def call(image=p, total=p, c=19, rows=p, capacity=4, state=p):
        return lib.msl_image_metrics(image, total, c, 0.5, rows, capacity, state, None)

    assert call(image=None) == ERR_ARG and call(total=None) == ERR_ARG
    assert call(rows=None) == ERR_ARG and call(state=None) == ERR_ARG
    assert call(c=0) == ERR_ARG and call(c=33) == ERR_ARG and call(c=-1) == ERR_ARG
    assert call(capacity=0) == ERR_ARG and call(capacity=-3) == ERR_ARG
    assert bytes(keep) == bytes(64)


def test_analysis_maps_refuses_bad_arguments_before_any_launch():
    from maxsquareloss_amd import hip
    lib = hip.load(require_gpu=False)
    keep, p = _buf()

    def call(x=p, mean=p, label=p, cls=p, palette=p, c=19, h=4, w=4, state=None, stride=48,
             outs=(p, p, p, p)):
        return lib.msl_analysis_maps(x, mean, label, cls, palette, c, h, w, state, stride, *outs, None)

    assert call(outs=(None,) * 4) == ERR_ARG                                   # no output
    assert call(c=0) == ERR_ARG and call(c=33) == ERR_ARG                      # the LDS palette holds 32 classes
    assert call(h=0) == ERR_ARG and call(w=0) == ERR_ARG and call(h=-2) == ERR_ARG
    assert call(h=1 << 16, w=1 << 15) == ERR_ARG                               # h * w = 2^31
    assert call(h=46341, w=46341) == ERR_ARG                                   # just above 2^31
    assert call(stride=-1) == ERR_ARG
    # an input a requested map reads: label (label, error), x and mean (input, error), cls (pred, error),
    # palette (all but input)
    assert call(label=None, outs=(p, None, None, None)) == ERR_ARG
    assert call(label=None, outs=(None, None, None, p)) == ERR_ARG
    assert call(x=None, outs=(None, None, p, None)) == ERR_ARG
    assert call(mean=None, outs=(None, None, p, None)) == ERR_ARG
    assert call(x=None, outs=(None, None, None, p)) == ERR_ARG
    assert call(cls=None, outs=(None, p, None, None)) == ERR_ARG
    assert call(cls=None, outs=(None, None, None, p)) == ERR_ARG
    assert call(palette=None, outs=(p, None, None, None)) == ERR_ARG
    assert call(palette=None, outs=(None, p, None, None)) == ERR_ARG
    assert call(palette=None, outs=(None, None, None, p)) == ERR_ARG
    assert bytes(keep) == bytes(64)


# ----------------------------------------------------------------------------- flags and names
def test_parser_defaults_and_rejections(capsys):
    from maxsquareloss_amd.tools import analysis, evaluate
    a = analysis.build_parser().parse_args([])
    assert a.miou_threshold == 0.5 and a.analysis_kinds == ("label", "pred", "style") and a.ring == 8 and a.worst == 0
    assert (a.flip, a.graph, a.scales, a.data_root_path) == (False, False, (1.0,), None)  # the evaluator's parser
    base = {x.dest for x in evaluate.build_parser()._actions}
    assert {x.dest for x in analysis.build_parser()._actions} - base == {"miou_threshold", "analysis_kinds", "ring",
                                                                         "worst"}
    a = analysis.build_parser().parse_args(["--analysis_kinds", "error, label,error", "--ring", "64", "--worst", "3",
                                            "--miou_threshold", "0.25", "--data_loader_workers", "2"])
    assert (a.analysis_kinds, a.ring, a.worst, a.miou_threshold) == (("error", "label"), 64, 3, 0.25)
    assert analysis.build_parser().parse_args(["--ring", "1"]).ring == 1
    for argv, word in ((["--ring", "0"], "0"), (["--ring", "65"], "65"), (["--ring", "x"], "x"),
                       (["--analysis_kinds", "label,heat"], "heat"), (["--analysis_kinds", ""], "kinds")):
        with pytest.raises(SystemExit):
            analysis.build_parser().parse_args(argv)
        assert word in capsys.readouterr().err
    assert hasattr(analysis.resultEvaluater, "main") and hasattr(analysis.resultEvaluater, "getvalResult")
    # the evaluator's own picture flags would be ignored here: refused, not accepted silently
    for argv in (["--save_predictions", "d"], ["--image_summary", "True"]):
        with pytest.raises(SystemExit):
            analysis.parse_args(["--imagenet_pretrained", "False", "--save_dir", ""] + argv)
        assert "savePics" in capsys.readouterr().err
    args, _, _ = analysis.parse_args(["--imagenet_pretrained", "False", "--save_dir", "", "--split", "train"])
    assert args.split == "val" and args.crop_size == args.target_crop_size


def test_analyzer_checks_its_ring_and_kinds():
    import argparse
    import torch
    from maxsquareloss_amd.hip import MSLError
    from maxsquareloss_amd.utils.analysis import Analyzer
    dev = torch.device("cpu")
    a = Analyzer(None, 19, (8, 12), 3, dev, "out", ring=2, kinds=("style", "error"))
    assert (a.ring, a.kinds, a.drains, a.replays, a.rows, a.valid_iterations) == (2, ("style", "error"), 0, 0, [], 3)
    assert a.out_dir == os.path.join("out", "savePics") and a.Eval is not a.totalEval
    for ring in (0, 65):
        with pytest.raises(MSLError, match="ring"):
            Analyzer(None, 19, (8, 12), 3, dev, "out", ring=ring)
    with pytest.raises(argparse.ArgumentTypeError):
        Analyzer(None, 19, (8, 12), 3, dev, "out", kinds=("heat",))


def test_file_names_are_the_references():
    from maxsquareloss_amd.utils import analysis as an
    # tools/analysis.py:211-227, evaluated by hand
    base = an.base_name("frankfurt/frankfurt_000000_000294_leftImg8bit.png", 0.91234, 0.5, 0.31999, 0.876)
    assert base == "frankfurt_000000_000294_leftImg8bit_PA_0.91_MPA_0.50_MIoU_0.32_FWIoU_0.88_"
    assert an.base_name("000003", 0, float("nan"), 0.125, 1.0) == "000003_PA_0.00_MPA_nan_MIoU_0.12_FWIoU_1.00_"
    names = [an.file_name("a.b.png", (0.1, 0.2, 0.3, 0.4), k) for k in an.KINDS]
    assert names == ["a.b_PA_0.10_MPA_0.20_MIoU_0.30_FWIoU_0.40_" + s + ".png"
                     for s in ("label_img", "pred_img", "style_img", "error_img")]
    row = np.arange(9 + 16, dtype=np.float64)
    assert an.row_scores(row, 16) == (0.0, 4.0, 5.0, 6.0) and an.row_scores(row, 19) == (0.0, 1.0, 2.0, 3.0)
    assert an.MIOU_THRESHOLD == 0.5 and an.DEFAULT_KINDS == ("label", "pred", "style")


# ----------------------------------------------------------------------------- the restatement
def _host_scores(m):
    """The host Eval's values in msl_image_metrics' field order (NaN where it has none)."""
    from maxsquareloss_amd.utils.eval import Eval
    C = m.shape[0]
    ev = Eval(C)
    ev.confusion_matrix = m.astype(np.float64)
    out = np.full(7, np.nan)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")  # nanmean of an all-NaN slice, 0 / 0
        out[0] = ev.Pixel_Accuracy()
        vals = (ev.Mean_Pixel_Accuracy(), ev.Mean_Intersection_over_Union(),
                ev.Frequency_Weighted_Intersection_over_Union())
        for i, v in enumerate(vals):
            if C == 16:
                out[1 + i], out[4 + i] = v
            else:
                out[1 + i] = v
        iou = ev._iou(ev.confusion_matrix)
    return out, iou


def _same(got, want, exact=()):
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    ok = ~np.isnan(want)
    assert (np.abs(got[ok] - want[ok]) <= ref.MEAN_TOL).all(), (got, want)
    for i in exact:
        assert got[i] == want[i] or (np.isnan(got[i]) and np.isnan(want[i]))


@pytest.mark.parametrize("C", [1, 13, 16, 19, 32])
def test_restatement_equals_the_host_eval_on_the_hand_made_matrices(C, capsys):
    for name, m in ref.matrices(C).items():
        row = ref.metrics_row(m, 0.5)
        want, iou = _host_scores(m)
        _same(row[:7], want, exact=(0,))
        assert np.array_equal(row[ref.HEAD:], iou, equal_nan=True), name  # per-class IoU bit for bit
        assert row[7] == float(m.sum()) and row[7] == float(int(m.sum()))  # exact, also near 2^45
    ms = ref.matrices(C)
    assert np.isnan(ref.metrics_row(ms["zero"], 0.5)[1:7]).all() and ref.metrics_row(ms["zero"], 0.5)[0] == 0.0
    assert ref.metrics_row(ms["zero"], 2.0)[8] == 0.0  # NaN is not selected
    assert ms["big"].min() >= 1 << 40
    if C > 1:
        r = ref.metrics_row(ms["absent"], 0.5)
        assert np.isnan(r[ref.HEAD + C // 2]) and np.isnan(r[ref.HEAD:]).sum() == 1
        r = ref.metrics_row(ms["only_predicted"], 0.5)
        assert r[ref.HEAD + C - 1] == 0.0 and ms["only_predicted"][:, C - 1].sum() > 0  # IoU 0, accuracy NaN
        assert np.isnan(_host_scores(ms["only_predicted"])[1]).sum() == 0
        r = ref.metrics_row(ms["half"], 0.5)
        assert (r[ref.HEAD:] == 0.5).all() and ref.val_miou(r, C) == 0.5 and r[8] == 0.0  # strict
        assert ref.metrics_row(ms["half"], np.nextafter(0.5, 1))[8] == 1.0
    capsys.readouterr()


def test_restatement_equals_the_reference_eval_golden():
    g = ref.gold()
    n = int(g["count"])
    seen = set()
    for k in range(n):
        m, want = g[f"cm_{k}"], g[f"scores_{k}"]
        C = m.shape[0]
        seen.add(C)
        row = ref.metrics_row(m, 0.5)
        got = row[:7] if C == 16 else row[:4]
        assert want.shape == got.shape
        _same(got, want, exact=(0,))
        if C != 16:
            assert np.isnan(row[4:7]).all()
    assert seen == {1, 13, 16, 19, 32} and n == 30
    assert sum(1 for k in range(n) if g[f"cm_{k}"].max() >= 1 << 40) == 5


def test_map_restatement_inputs_hit_every_case():
    from maxsquareloss_amd.utils.synthetic import IMG_MEAN
    assert np.array_equal(IMG_MEAN, ref.IMG_MEAN)
    C = 19
    pal = np.arange(C * 3, dtype=np.uint8).reshape(C, 3) + 7
    for h, w in ((3, 4), (5, 7), (8, 12), (33, 64)):
        x, label, cls = ref.map_inputs(h, w, C)
        s = x + ref.IMG_MEAN[:, None, None]
        assert np.isnan(x).sum() == 1 and (s < 0).any() and (s > 255).any()
        assert (np.abs(s - np.floor(s)) == 0.5).sum() >= 3  # exact ties: round half to even decides
        assert {-1, 255, C} <= set(label.reshape(-1).tolist()) and ((label >= 0) & (label < C)).sum() > h * w // 2
        m = ref.maps(x, label, cls, pal, C)
        valid = (label >= 0) & (label < C)
        right = valid & (cls == label)
        assert right.any() and (valid & ~right).any()
        assert (m["label"][~valid] == 0).all() and (m["error"][~valid] == 0).all()
        assert np.array_equal(m["error"][right], m["input"][right] >> 1)
        assert np.array_equal(m["error"][valid & ~right], pal[cls[valid & ~right]])
        assert np.array_equal(m["pred"], pal[cls])
    # recover_input's bytes, by torch
    import torch
    from maxsquareloss_amd.utils.images import recover_input
    x, _, _ = ref.map_inputs(8, 12, C)
    ok = ~np.isnan(x).any(axis=0)
    want = recover_input(torch.from_numpy(x)[None]).numpy()
    assert np.array_equal(ref.input_image(x)[ok], want[ok])
    # half to even, by hand: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 254.5 -> 254, 255.5 -> 255 (clamped), -0.5 -> 0
    t = np.array([0.5, 1.5, 2.5, 254.5, 255.5, -0.5, np.nan, 300, -7], np.float32).reshape(1, 1, 9).repeat(3, axis=0)
    assert ref.input_image(t, np.zeros(3, np.float32))[0, :, 0].tolist() == [0, 2, 2, 254, 255, 0, 0, 255, 0]
