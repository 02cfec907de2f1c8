"""The host side of in-loop AdaIN domain adaptation (tools/ADAIN.py): the plateau scheduler against torch's, the
parser, and the new entry points of the C ABI.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("msl_style_input_window", "msl_style_output_resampled", "msl_label_resize_nearest",
                    "msl_predict_rectify")


class _Groups:
    def __init__(self, lrs):
        self.param_groups = [{"lr": lr} for lr in lrs]


# improvements, a tie with the best, relative improvements below the threshold, plateaus longer than the
# patience (two reductions in a row of bad epochs), and a late improvement
LOSSES = [2.0, 1.5, 1.5, 1.49999, 1.6, 1.7, 1.8, 1.4, 1.4, 1.4, 1.4, 1.4, 1.4, 1.4, 1.4, 1.4, 1.39, 1.5, 1.5, 1.5, 1.5,
          1.5, 0.2, 0.2, 0.2, 0.2, 0.2, 0.3]


def test_plateau_scheduler_equals_torch():
    from maxsquareloss_amd.tools.ADAIN import ReduceLROnPlateau
    p0, p1 = torch.nn.Parameter(torch.zeros(1)), torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([{"params": [p0], "lr": 2.5e-4}, {"params": [p1], "lr": 2.5e-3}], lr=2.5e-4, momentum=0.9)
    ref = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.9, patience=3)
    mine_opt = _Groups([2.5e-4, 2.5e-3])
    mine = ReduceLROnPlateau(mine_opt, factor=0.9, patience=3)
    seen = set()
    for loss in LOSSES:
        ref.step(loss)
        mine.step(loss)
        want = [g["lr"] for g in opt.param_groups]
        got = [g["lr"] for g in mine_opt.param_groups]
        assert got == want, (loss, got, want)
        assert mine.num_bad_epochs == ref.num_bad_epochs and mine.best == ref.best
        seen.add(want[0])
    assert len(seen) >= 4  # the sequence did reduce the rate, more than twice


def _required(tmp="x"):
    return ["--vgg", "vgg_normalised.pth", "--decoder", "decoder.pth", "--style", "styles/"]


def test_parser_accepts_the_reference_command_line():
    """Every flag of the reference's add_train_args and of its ADAIN.py add_UDA_train_args, with values."""
    from maxsquareloss_amd.tools import ADAIN
    from maxsquareloss_amd.tools.train_source import init_args
    argv = ["--data_root_path", "d", "--list_path", "l", "--checkpoint_dir", "c", "--save_dir", "s",
            "--backbone", "deeplabv2_multi", "--bn_momentum", "0.1", "--imagenet_pretrained", "True",
            "--pretrained_ckpt_file", "p", "--continue_training", "False", "--show_num_images", "2", "--seed", "12345",
            "--gpu", "0", "--batch_size", "1", "--exp_tag", "DA", "--dataset", "cityscapes", "--base_size", "1280,720",
            "--crop_size", "640,360", "--target_base_size", "1280,720", "--target_crop_size", "640,360",
            "--seg_size", "1280,640", "--num_classes", "19", "--data_loader_workers", "4", "--pin_memory", "2",
            "--split", "train", "--random_mirror", "True", "--random_crop", "False", "--resize", "True",
            "--gaussian_blur", "False", "--numpy_transform", "True", "--freeze_bn", "False", "--optim", "SGD",
            "--momentum", "0.9", "--weight_decay", "5e-4", "--lr", "2.5e-4", "--iter_max", "200000", "--iter_stop", "80000",
            "--poly_power", "0.9", "--rectification", "True", "--crop_trans", "True", "--DA", "True", "--multi", "True",
            "--lambda_seg", "0.1",
            "--source_dataset", "gta5", "--source_split", "train", "--init_round", "0", "--round_num", "40",
            "--epoch_each_round", "2", "--target_mode", "IW_maxsquare", "--lambda_target", "0.09", "--gamma", "0",
            "--IW_ratio", "0.2", "--threshold", "0.95", "--adain_lr", "1e-4"] + _required()
    args, _, _ = init_args(ADAIN.parse_args(argv))
    assert args.seg_size == (1280, 640) and args.base_size == (1280, 720) and args.crop_size == (640, 360)
    assert args.rectification and args.crop_trans and args.adain_lr == 1e-4 and args.weights is None
    ADAIN.check_sizes(args)
    # the reference's defaults of ADAIN.py
    d = ADAIN.parse_args(_required())
    assert (d.round_num, d.target_mode, d.lambda_target, d.alpha) == (40, "IW_maxsquare", 0.09, 1.0)
    assert d.seg_size == (1280, 640) and not d.crop_trans and not d.rectification
    w = ADAIN.parse_args(_required() + ["--style", "a.png", "b.png", "--style_interpolation_weight", "1,3"])
    assert w.style == ["a.png", "b.png"] and w.weights == [0.25, 0.75]


@pytest.mark.parametrize("missing", ["--vgg", "--decoder", "--style"])
def test_missing_style_network_flags_are_parser_errors(missing, capsys):
    from maxsquareloss_amd.tools import ADAIN
    argv = _required()
    k = argv.index(missing)
    with pytest.raises(SystemExit) as e:
        ADAIN.parse_args(argv[:k] + argv[k + 2:])
    assert e.value.code == 2 and missing in capsys.readouterr().err


def test_bad_sizes_and_weights_are_parser_errors():
    from maxsquareloss_amd.tools import ADAIN
    for extra in (["--seg_size", "1280"], ["--alpha", "1.5"], ["--style_interpolation_weight", "a,b"],
                  ["--style_interpolation_weight", "0,0"]):
        with pytest.raises(SystemExit):
            ADAIN.parse_args(_required() + extra)


def test_size_checks():
    from maxsquareloss_amd.hip import MSLError
    from maxsquareloss_amd.tools import ADAIN
    from maxsquareloss_amd.tools.train_source import init_args

    def args_of(*extra):
        return init_args(ADAIN.parse_args(_required() + list(extra)))[0]

    ok = args_of("--base_size", "1280,720", "--crop_size", "640,360", "--target_base_size", "1280,720",
                 "--seg_size", "1280,640", "--crop_trans", "True", "--rectification", "True")
    ADAIN.check_sizes(ok)
    for bad in (("--base_size", "1280,720", "--crop_size", "640,320", "--crop_trans", "True"),
                ("--base_size", "1284,644", "--target_base_size", "1280,640", "--seg_size", "1284,644"),
                ("--target_base_size", "1281,640", "--rectification", "True"),
                ("--target_base_size", "1280,641", "--rectification", "True"),
                ("--seg_size", "1279,640", "--rectification", "True"),
                ("--seg_size", "1280,639", "--rectification", "True")):
        with pytest.raises(MSLError):
            ADAIN.check_sizes(args_of(*bad))


def test_nearest_index_is_torchs_rule():
    """The host-side index table the windows of crop_trans are cut with: torch's on every size pair tried, where
    the integer rule dst * in // out is not (24 -> 74, 56 -> 46)."""
    import torch.nn.functional as F
    from maxsquareloss_amd.utils.style_transform import _quadrant_span, nearest_index
    differs = 0
    for n_in in list(range(2, 70)) + [399, 640, 1280]:
        src = torch.arange(n_in, dtype=torch.float32).reshape(1, 1, 1, n_in)
        for n_out in list(range(1, 90)) + [399, 720, 1280]:
            want = F.interpolate(src, size=(1, n_out))[0, 0, 0].long().numpy()
            assert np.array_equal(nearest_index(n_in, n_out), want), (n_in, n_out)
            differs += int(not np.array_equal(want, np.arange(n_out) * n_in // n_out))
    assert differs > 0
    for full, dest in ((24, 74), (40, 46), (720, 640), (1280, 1280)):
        (a0, an), (b0, bn) = _quadrant_span(full, dest, 0, full // 2), _quadrant_span(full, dest, full // 2, full // 2)
        assert a0 == 0 and b0 == an and an + bn == dest  # the two halves tile the destination


def test_new_entry_points_are_declared_and_exported():
    from maxsquareloss_amd import hip, ops
    header = open(os.path.join(ROOT, "include", "msl_hip.h")).read()
    lib = hip.load(require_gpu=False)
    for name in NEW_ENTRY_POINTS:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header)
        assert m, f"include/msl_hip.h declares {name}"
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        res, args = hip.SIGNATURES[name]
        assert res is hip.c_int and len(params) == len(args), name
        for p, a in zip(params, args):
            want = hip.c_p if "*" in p or "msl_stream_t" in p else (hip.c_f if p.startswith("float") else hip.c_int)
            assert a is want, (name, p)
        assert hasattr(lib, name), name
    assert lib.msl_abi_version() == hip.ABI_VERSION == 3
    for fn in ("style_input_window", "style_output_resampled", "label_resize_nearest", "predict_rectify"):
        assert callable(getattr(ops, fn))
    # the rectification kernels neither spill nor use scratch (the build's resource report)
    path = os.path.join(ROOT, "maxsquareloss_amd", "_lib", "obj", "predict.o.remarks")
    if os.path.exists(path):
        text = open(path).read()
        blocks = re.findall(r"Function Name: (\S*k_predict_rectify\S*)(.*?)(?=Function Name:|\Z)", text, flags=re.S)
        assert len(blocks) == 4  # 19, 16, 13 and up to 32 classes
        for name, body in blocks:
            assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", body) and re.search(r"VGPRs Spill: 0\b", body), name
