"""CPU: the host side of the AdaIN style pass (csrc/style.hip's C-ABI, tools/net.py, tools/stylize.py).

Nothing here launches a kernel: the entry points are called with arguments they must refuse before any
launch, the network classes are checked against torch.nn stacks this module builds itself, and the conv
calls of a pass are planned through msl_conv_fwd_plan (host only) and held to the kernels and schedules
tests/conv_form_cases.py TABLE compares with fp64.
"""
import os

import pytest
import torch
import torch.nn as nn

import conv_form_cases as cf
from style_ref import ref_decoder, ref_vgg
from maxsquareloss_amd import hip
from maxsquareloss_amd.tools import net, stylize

OK_PTR = 0x1000  # never dereferenced: the checks refuse the call before any launch
ERR_SHAPE, ERR_ARG = -1, -3
NEW_SYMBOLS = ("msl_style_pad", "msl_style_input", "msl_style_stats_workspace", "msl_style_stats",
               "msl_style_max_styles", "msl_style_adain_coef", "msl_style_output")


def test_library_exports_the_style_entry_points():
    lib = hip.load(require_gpu=False)
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in hip.SIGNATURES, s
    assert hip.ABI_VERSION == 3 and lib.msl_abi_version() == 3
    assert lib.msl_style_max_styles() == 16


# ------------------------------------------------------------------------------------------ refusals
def _pad(x=OK_PTR, grid=0, c=4, h=8, w=8, act=0, rs=0, a=None, b=None, y=OK_PTR, cpad=4):
    return hip.load(require_gpu=False).msl_style_pad(x, grid, c, h, w, act, rs, a, b, y, cpad, None)


def test_style_pad_refuses_before_any_launch():
    assert _pad(x=None) == ERR_ARG and _pad(y=None) == ERR_ARG
    assert _pad(a=OK_PTR) == ERR_ARG and _pad(b=OK_PTR) == ERR_ARG  # the affine is both or neither
    for kw in (dict(c=0), dict(c=-1), dict(h=0), dict(w=-3), dict(cpad=3), dict(act=3), dict(act=-1), dict(rs=3),
               dict(grid=2)):
        assert _pad(**kw) == ERR_ARG, kw
    for rs in (0, 1, 2):
        assert _pad(h=1, rs=rs) == ERR_SHAPE and _pad(w=1, rs=rs) == ERR_SHAPE
    # a 2x2 map pools to 1x1, which has no reflection (torch's ReflectionPad2d(1) refuses it too)
    assert _pad(h=2, w=8, rs=1) == ERR_SHAPE and _pad(h=8, w=2, rs=1) == ERR_SHAPE
    assert _pad(c=64, cpad=64, h=40000, w=40000) == ERR_ARG  # cells past 2^31
    assert _pad(c=1, cpad=1, h=30000, w=30000, rs=2) == ERR_ARG  # the output grid past 2^31


def test_style_input_refuses_before_any_launch():
    f = hip.load(require_gpu=False).msl_style_input
    ok = OK_PTR
    assert f(None, None, 8, 8, ok, ok, ok, 3, None) == ERR_ARG  # no image
    assert f(ok, ok, 8, 8, ok, ok, ok, 3, None) == ERR_ARG      # two images
    assert f(ok, None, 8, 8, None, ok, ok, 3, None) == ERR_ARG
    assert f(ok, None, 8, 8, ok, None, ok, 3, None) == ERR_ARG
    assert f(None, ok, 8, 8, ok, ok, None, 3, None) == ERR_ARG
    assert f(ok, None, 8, 8, ok, ok, ok, 2, None) == ERR_ARG
    assert f(ok, None, 0, 8, ok, ok, ok, 3, None) == ERR_ARG and f(ok, None, 8, -1, ok, ok, ok, 3, None) == ERR_ARG
    assert f(ok, None, 1, 8, ok, ok, ok, 3, None) == ERR_SHAPE and f(None, ok, 8, 1, ok, ok, ok, 3, None) == ERR_SHAPE
    assert f(ok, None, 30000, 30000, ok, ok, ok, 3, None) == ERR_ARG


def test_style_stats_refuses_before_any_launch():
    lib = hip.load(require_gpu=False)
    f, ok = lib.msl_style_stats, OK_PTR
    assert f(None, 0, 4, 8, 8, 1, ok, None, 0, None) == ERR_ARG
    assert f(ok, 0, 4, 8, 8, 1, None, None, 0, None) == ERR_ARG
    for c, h, w in ((0, 8, 8), (4, 0, 8), (4, 8, -2)):
        assert f(ok, 0, c, h, w, 1, ok, None, 0, None) == ERR_ARG
    assert f(ok, 2, 4, 8, 8, 1, ok, None, 0, None) == ERR_ARG and f(ok, 0, 4, 8, 8, 2, ok, None, 0, None) == ERR_ARG
    assert f(ok, 0, 4, 1, 1, 1, ok, None, 0, None) == ERR_SHAPE  # H*W < 2: torch's unbiased variance is NaN
    assert f(ok, 0, 64, 40000, 40000, 1, ok, None, 0, None) == ERR_ARG
    # more than one 8192-pixel chunk per channel needs the workspace
    assert lib.msl_style_stats_workspace(5, 1, 8192) == 0
    need = lib.msl_style_stats_workspace(5, 1, 65539)
    assert need == 5 * 9 * 12
    assert f(ok, 0, 5, 1, 65539, 1, ok, None, 0, None) == -2 and f(ok, 0, 5, 1, 65539, 1, ok, ok, need - 1, None) == -2


def test_style_adain_coef_refuses_before_any_launch():
    f, ok = hip.load(require_gpu=False).msl_style_adain_coef, OK_PTR
    for i in (0, 1, 2, 7, 8):
        a = [ok, ok, ok, 1, 512, 1.0, 1e-5, ok, ok, None]
        a[i] = None
        assert f(*a) == ERR_ARG, i
    assert f(ok, ok, ok, 0, 512, 1.0, 1e-5, ok, ok, None) == ERR_ARG
    assert f(ok, ok, ok, 17, 512, 1.0, 1e-5, ok, ok, None) == ERR_ARG
    assert f(ok, ok, ok, 1, 0, 1.0, 1e-5, ok, ok, None) == ERR_ARG
    for alpha in (-0.01, 1.01, float("nan")):
        assert f(ok, ok, ok, 1, 512, alpha, 1e-5, ok, ok, None) == ERR_ARG, alpha
    assert f(ok, ok, ok, 1, 512, 0.5, -1e-5, ok, ok, None) == ERR_ARG


def test_style_output_refuses_before_any_launch():
    f, ok = hip.load(require_gpu=False).msl_style_output, OK_PTR
    assert f(None, 0, 8, 8, ok, ok, 0.0, 0.0, 0.0, None) == ERR_ARG
    assert f(ok, 0, 8, 8, None, None, 0.0, 0.0, 0.0, None) == ERR_ARG  # no output at all
    assert f(ok, 0, 0, 8, ok, None, 0.0, 0.0, 0.0, None) == ERR_ARG and f(ok, 0, 8, -1, ok, None, 0.0, 0.0, 0.0, None) == ERR_ARG
    assert f(ok, 3, 8, 8, ok, None, 0.0, 0.0, 0.0, None) == ERR_ARG
    assert f(ok, 1, 30000, 30000, ok, None, 0.0, 0.0, 0.0, None) == ERR_ARG


# ------------------------------------------------------------------------------------------ the network
@pytest.fixture(scope="module")
def states():
    torch.manual_seed(0)
    return ref_vgg().state_dict(), ref_decoder().state_dict()


def test_stacks_load_reference_indexed_state_dicts(states):
    vs, ds = states
    assert len(net.vgg) == 53 and len(net.decoder) == 29
    assert list(vs) == list(net.vgg.state_dict()) and list(ds) == list(net.decoder.state_dict())
    assert "0.weight" in vs and "2.weight" in vs and "51.bias" in vs and "1.weight" in ds and "28.bias" in ds
    net.make_vgg().load_state_dict(vs)
    net.make_decoder().load_state_dict(ds)
    for mine, ref in ((net.vgg, ref_vgg()), (net.decoder, ref_decoder())):
        assert [type(m) for m in mine] == [type(m) for m in ref]
    assert net.vgg[7].ceil_mode and net.decoder[3].mode == "nearest"
    assert isinstance(net.vgg[net.ENCODER_CHILDREN - 1], nn.ReLU) and net.vgg[net.ENCODER_CHILDREN - 2].out_channels == 512


def test_stylenet_takes_both_decoder_checkpoint_shapes(states):
    vs, ds = states
    bare = net.StyleNet(vs, ds, device="cpu")
    wrapped = net.StyleNet(vs, {"state_dict": ds, "loss_c_best": 1.0, "loss_s_best": 2.0}, device="cpu")
    assert len(bare.enc_stages) == 9 and len(bare.dec_stages) == 9
    for a, b in zip(bare.dec_stages, wrapped.dec_stages):
        assert torch.equal(a.weight, b.weight) and torch.equal(a.bias, b.bias)
    assert torch.equal(bare.w1, vs["0.weight"]) and torch.equal(bare.enc_stages[0].weight, vs["2.weight"])
    assert torch.equal(bare.enc_stages[-1].weight, vs["29.weight"]) and torch.equal(bare.dec_stages[-1].bias, ds["28.bias"])
    assert [(s.act, s.resample) for s in bare.enc_stages] == [
        ("none", "none"), ("relu", "none"), ("relu", "pool"), ("relu", "none"), ("relu", "pool"), ("relu", "none"),
        ("relu", "none"), ("relu", "none"), ("relu", "pool")]
    assert [(s.act, s.resample) for s in bare.dec_stages] == [
        ("none", "none"), ("relu", "up"), ("relu", "none"), ("relu", "none"), ("relu", "none"), ("relu", "up"),
        ("relu", "none"), ("relu", "up"), ("relu", "none")]


def test_stylenet_refuses_a_state_dict_of_the_wrong_shape(states):
    vs, ds = states
    bad = dict(ds)
    bad["1.weight"] = torch.zeros(256, 256, 3, 3)
    with pytest.raises(RuntimeError):
        net.StyleNet(vs, bad, device="cpu")
    short = {k: v for k, v in vs.items() if not k.startswith("51.")}
    with pytest.raises(RuntimeError):
        net.StyleNet(short, ds, device="cpu")


@pytest.mark.parametrize("h,w", [(37, 53), (512, 1024), (720, 1280), (1, 1), (8, 9), (17, 16)])
def test_output_size_formula_matches_the_stacks(h, w):
    """H' = 8 ceil(ceil(ceil(H/2)/2)/2): three ceil-mode pools, then three doublings."""
    x = torch.zeros(1, 1, h, w)
    pool = nn.MaxPool2d((2, 2), (2, 2), (0, 0), ceil_mode=True)
    up = nn.Upsample(scale_factor=2, mode="nearest")
    y = up(up(up(pool(pool(pool(x))))))
    assert net.out_hw(h, w) == tuple(y.shape[-2:])


def test_conv_calls_follow_the_pass(states):
    sn = net.StyleNet(*states, device="cpu")
    calls = sn.conv_calls(37, 53)
    assert calls[0] == (3, 64, 39, 55) and calls[2] == (64, 128, 21, 29) and calls[8] == (256, 512, 7, 9)
    assert calls[9] == (512, 256, 7, 9) and calls[10] == (256, 256, 12, 16) and calls[-1] == (64, 3, 42, 58)
    assert len(sn.conv_calls(37, 53, decode=False)) == 9
    assert (calls[-1][2] - 2, calls[-1][3] - 2) == net.out_hw(37, 53)


# ------------------------------------------------------------------------------------------ the plan gate
@pytest.mark.parametrize("family", ["fp32", "fp16"])
@pytest.mark.parametrize("w,h", [(1024, 512), (1280, 640), (1280, 720), (53, 37)])
def test_every_conv_call_lands_on_a_kernel_held_to_fp64(states, family, w, h):
    """Every conv call of a style pass (content and style encoders, decoder), as the library plans it under the
    default forms: not refused, and on a (kernel, schedule class) TABLE has a case of - or a flat schedule,
    which exercises no tile-straddling worker range."""
    sn = net.StyleNet(*states, device="cpu")
    table = {(k, c) for k, c, _ in cf.TABLE}
    keys = cf.all_form_keys(hip)
    for cin, cout, gh, gw in sn.conv_calls(h, w):
        case = cf.Case("dconv_fwd", family, "f16x3", 1, 1, cin, cout, gh, gw, 1, 1, 0)
        pl = cf.plan_of(hip, case)
        assert pl.status == cf.MSL_OK, (case, pl.status)
        cls = cf.schedule_class(pl)
        key = keys[pl.row] if pl.stream_k else "tile"
        assert cls == "flat" or (key, cls) in table, (case, key, cls)


# ------------------------------------------------------------------------------------------ the tool
BASE = ["--vgg", "v.pth", "--decoder", "d.pth", "--output_path", "out", "--style", "s/ambulance.jpg"]


def test_stylize_arguments():
    a = stylize.parse_args(BASE + ["--content_dir", "c", "--content_size", "1024,512", "--style_size", "640,320",
                                   "--alpha", "0.6", "--save_ext", "png", "--data_loader_workers", "3",
                                   "--conv_math", "fp16", "--keep_tree", "True"])
    assert a.content_size == (1024, 512) and a.style_size == (640, 320) and a.alpha == 0.6
    assert a.save_ext == "png" and a.data_loader_workers == 3 and a.conv_math == "fp16" and a.keep_tree is True
    assert a.weights is None and a.style == ["s/ambulance.jpg"]
    a = stylize.parse_args(["--vgg", "v", "--decoder", "d", "--output_path", "o", "--content_list", "l.txt",
                            "--content_root", "r", "--style", "a.jpg", "b.jpg", "--style_interpolation_weight", "1,3"])
    assert a.weights == [0.25, 0.75] and a.save_ext == "jpg" and a.keep_tree is False
    for bad in (["--content_dir", "c"],                                        # no weights, no style
                ["--vgg", "v", "--output_path", "o", "--style", "s.jpg", "--content_dir", "c"],      # no decoder
                ["--decoder", "d", "--output_path", "o", "--style", "s.jpg", "--content_dir", "c"],  # no encoder
                BASE,                                                           # no content
                BASE + ["--content_dir", "c", "--content_list", "l", "--content_root", "r"],
                BASE + ["--content_list", "l"],
                BASE + ["--content_dir", "c", "--alpha", "1.5"],
                BASE + ["--content_dir", "c", "--save_ext", "bmp"],
                BASE + ["--content_dir", "c", "--style", "a.jpg", "b.jpg"],
                BASE + ["--content_dir", "c", "--style", "a.jpg", "b.jpg", "--style_interpolation_weight", "1,2,3"]):
        with pytest.raises(SystemExit):
            stylize.parse_args(bad)


def test_stylize_output_names():
    one = ["styles/ambulance.jpg"]
    assert stylize.output_name("images/00001.png", 512, 1024, one, "jpg") == "00001_512r1024_ambulance.jpg"
    assert stylize.output_name("00001.png", 37, 53, one, "png") == "00001_37r53_ambulance.png"
    assert stylize.output_name("a/b/x.png", 512, 1024, one + ["t.png"], "png") == "xstylized.png"
    assert stylize.output_name("images/00001.png", 512, 1024, one, "jpg", keep_tree=True) == "images/00001.png"


def test_stylize_content_items(tmp_path):
    for rel in ("images/00002.png", "images/00001.png", "images/notes.txt", "top.JPG"):
        p = tmp_path / rel
        p.parent.mkdir(exist_ok=True)
        p.write_bytes(b"")
    a = stylize.parse_args(BASE + ["--content_dir", str(tmp_path)])
    assert [r for _, r in stylize.content_items(a)] == ["images/00001.png", "images/00002.png", "top.JPG"]
    lst = tmp_path / "list.txt"
    lst.write_text("images/00002.png\n\nimages/00001.png\n")
    a = stylize.parse_args(BASE + ["--content_list", str(lst), "--content_root", str(tmp_path)])
    items = stylize.content_items(a)
    assert [r for _, r in items] == ["images/00002.png", "images/00001.png"]
    assert items[0][0] == os.path.join(str(tmp_path), "images/00002.png")
