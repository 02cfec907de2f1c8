"""The AdaIN style pass on the GPU (csrc/style.hip, ops.style_* / ops.conv3x3_reflect, tools/net.StyleNet,
utils/style_transform, tools/stylize).

torch itself is the oracle: its own modules on the CPU for what must agree bit for bit (ReLU, ceil-mode
max-pool, nearest up-sampling, reflection padding, the 8-bit and segmentation-input quantisation), fp64 on the
CPU for what is arithmetic, with torch's fp32 CPU run of the same formula as the yardstick for the error a
correct fp32 evaluation may have.  Every test prints the figures it asserts on.
"""
import argparse
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

import style_ref as sr  # noqa: E402
from maxsquareloss_amd import hip, ops  # noqa: E402
from maxsquareloss_amd.tools import net, stylize  # noqa: E402
from maxsquareloss_amd.utils import style_transform as st  # noqa: E402
from maxsquareloss_amd.utils.synthetic import IMG_MEAN  # noqa: E402

DEV = "cuda"
SENTINEL = 12345.0
EPS = 1e-5


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def in_grid(x, fill=SENTINEL):
    """x (1, C, H, W) as the interior of a grid whose border holds `fill`."""
    g = torch.full((1, x.size(1), x.size(2) + 2, x.size(3) + 2), fill, dtype=x.dtype)
    g[:, :, 1:-1, 1:-1] = x
    return g


def ulp(v):
    v = v.float().abs()
    return (torch.nextafter(v, torch.full_like(v, float("inf"))) - v).double()


# ------------------------------------------------------------------------------------------ msl_style_pad
def _signed_data(c, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, c, h, w, generator=g)
    flat = x.view(-1)
    flat[::5] = -0.0
    flat[1::7] = 0.0
    flat[2::11] = -flat[2::11].abs()
    return x


def _torch_pad(x, relu, mode):
    y = nn.ReLU()(x) if relu else x
    if mode == "pool":
        y = nn.MaxPool2d((2, 2), (2, 2), (0, 0), ceil_mode=True)(y)
    elif mode == "up":
        y = nn.Upsample(scale_factor=2, mode="nearest")(y)
    return nn.ReflectionPad2d(1)(y)


PAD_CASES = [(3, 5, 7, "none"), (3, 5, 7, "pool"), (3, 5, 7, "up"), (17, 2, 2, "none"), (17, 2, 2, "up"),
             (64, 33, 65, "pool"), (5, 9, 130, "up")]


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("c,h,w,mode", PAD_CASES)
def test_style_pad_is_bit_identical_to_torch(c, h, w, mode, relu):
    x = _signed_data(c, h, w, seed=c * 1000 + h)
    want = _torch_pad(x, relu, mode)
    if (c, h, w, mode) == (3, 5, 7, "pool"):
        assert want.shape[-2:] == (3 + 2, 4 + 2)  # one-row and one-column windows at the odd ends
    got = ops.style_pad(x.to(DEV), act="relu" if relu else "none", resample=mode)
    assert same_bits(got, want)


def test_style_pad_refuses_a_pool_to_one_pixel():
    """The smallest legal size, 2x2, pools to 1x1, which torch's ReflectionPad2d(1) refuses; so does the kernel."""
    x = _signed_data(17, 2, 2, seed=3)
    with pytest.raises(RuntimeError):
        _torch_pad(x, False, "pool")
    with pytest.raises(hip.MSLError, match="status -1"):
        ops.style_pad(x.to(DEV), resample="pool")


@pytest.mark.parametrize("mode", ["none", "pool", "up"])
def test_style_pad_zero_fills_added_channels_and_reads_a_grid_interior(mode):
    x = _signed_data(3, 5, 7, seed=11)
    want = _torch_pad(x, True, mode)
    got = ops.style_pad(in_grid(x).to(DEV), grid=True, act="relu", resample=mode, cpad=8).cpu()
    assert got.shape[1] == 8 and same_bits(got[:, :3], want)
    assert torch.equal(bits(got[:, 3:]), torch.zeros_like(bits(got[:, 3:])))
    assert not (got == SENTINEL).any()


# ------------------------------------------------------------------------------------------ msl_style_stats
def _stats_data(h, w, seed=2):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, 5, h, w, generator=g)
    x[0, 1] = 0.37                                                # constant: variance 0, sigma = sqrt(eps)
    x[0, 2] = 1000.0 + 0.01 * torch.randn(h, w, generator=g)      # a large mean with a small spread
    x[0, 3] = -x[0, 3].abs() - 0.1                                # all negative before the ReLU
    x[0, 4] = 3.0 * x[0, 4] + 1.0
    return x


@pytest.mark.parametrize("h,w,grid", [(1, 2, False), (5, 7, True), (8191, 1, False), (1, 65539, False)])
def test_style_stats_against_fp64(h, w, grid):
    x = _stats_data(h, w)
    r = torch.relu(x)[0].reshape(5, -1)
    mean64, sig64 = r.double().mean(1), (r.double().var(1) + EPS).sqrt()
    mean32, sig32 = r.mean(1), (r.var(1) + EPS).sqrt()
    src = (in_grid(x) if grid else x).to(DEV)
    got = ops.style_stats(src, grid=grid, relu=True)
    again = ops.style_stats(src, grid=grid, relu=True)
    assert same_bits(got, again)
    got = got.cpu()
    for name, mine, ref64, ref32 in (("mean", got[0], mean64, mean32), ("sigma", (got[1] + EPS).sqrt(), sig64, sig32)):
        err = (mine.double() - ref64).abs()
        own = (ref32.double() - ref64).abs()
        bar = 4.0 * torch.maximum(own, ulp(ref64))
        print(f"stats {h}x{w} {name}: error {err.tolist()} torch-fp32 error {own.tolist()} bar {bar.tolist()}")
        assert (err <= bar).all(), (name, err.tolist(), bar.tolist())
    assert got[0, 3] == 0.0 and got[1, 3] == 0.0


def test_calc_mean_std_matches_the_formula():
    x = _stats_data(9, 13, seed=4)
    mean, std = st.calc_mean_std(x.to(DEV))
    m64, s64 = sr.mean_std(x.double())
    assert mean.shape == (1, 5, 1, 1) and std.shape == (1, 5, 1, 1)
    assert torch.allclose(mean.cpu().double(), m64, rtol=1e-6, atol=1e-7)
    assert torch.allclose(std.cpu().double(), s64, rtol=1e-5, atol=0)


# ------------------------------------------------------------------------------------------ msl_style_adain_coef
def _feats(seed=6):
    g = torch.Generator().manual_seed(seed)
    content = torch.relu(torch.randn(1, 6, 9, 11, generator=g) * 2.0 + 0.5)
    content.view(-1)[::13] = -0.0
    styles = [torch.relu(torch.randn(1, 6, 7, 5, generator=g) * 0.7 + 1.0),
              torch.relu(torch.randn(1, 6, 4, 15, generator=g) * 3.0 - 0.5)]
    return content, styles


def _adain_gpu(content, styles, alpha, weights):
    cs = ops.style_stats(content.to(DEV), relu=False)
    ss = torch.stack([ops.style_stats(s.to(DEV), relu=False) for s in styles])
    a, b = ops.style_adain_coef(cs, ss, weights, alpha)
    return ops.style_pad(content.to(DEV), a=a, b=b)[:, :, 1:-1, 1:-1].cpu(), a.cpu(), b.cpu()


def test_adain_alpha_zero_returns_the_content_bit_for_bit():
    content, styles = _feats()
    got, a, b = _adain_gpu(content, styles, 0.0, (0.25, 0.75))
    assert torch.equal(a, torch.ones(6)) and torch.equal(b, torch.zeros(6))
    assert same_bits(got, content)


@pytest.mark.parametrize("alpha", [0.3, 1.0])
def test_adain_against_the_reference_formula_in_fp64(alpha):
    content, styles = _feats()
    w = (0.25, 0.75)
    want = sr.mix(content.double(), [s.double() for s in styles], alpha, w)
    own = (sr.mix(content, styles, alpha, w).double() - want).abs().max().item()
    got, _, _ = _adain_gpu(content, styles, alpha, w)
    err = (got.double() - want).abs().max().item()
    print(f"adain alpha {alpha}: error {err:.3e}, torch-fp32 error {own:.3e}, ratio {err / own:.2f}")
    assert err <= 4.0 * own


def test_adaptive_instance_normalization_is_the_reference_function():
    content, styles = _feats()
    got = st.adaptive_instance_normalization(content.to(DEV), styles[0].expand(1, -1, -1, -1).to(DEV))
    want = sr.adain(content.double(), styles[0].double())
    assert got.shape == content.shape and (got.cpu().double() - want).abs().max().item() < 1e-5


# ------------------------------------------------------------------------------------------ msl_style_output
def _output_data(h=24, w=40):
    k = torch.arange(256, dtype=torch.float32)
    pts = torch.cat([k / 255, (k + 0.5) / 255, (k - 0.5) / 255])
    up, down = torch.full_like(pts, float("inf")), torch.full_like(pts, float("-inf"))
    vals = torch.cat([pts, torch.nextafter(pts, up), torch.nextafter(pts, down),
                      torch.tensor([-0.0, 0.0, -1e-3, -2.0, 1.0, 1.0000001, 1.002, 1.5, 7.0, -1e-9, 0.9999999])])
    g = torch.Generator().manual_seed(8)
    x = torch.rand(3 * h * w, generator=g) * 1.2 - 0.1
    assert vals.numel() <= x.numel()
    x[:vals.numel()] = vals
    return x[torch.randperm(x.numel(), generator=g)].reshape(1, 3, h, w)


@pytest.mark.parametrize("grid", [False, True])
def test_style_output_is_bit_identical_to_torch(grid):
    x = _output_data()
    q = x.mul(255).add(0.5).clamp(0, 255)
    want_u8 = q.to(torch.uint8)[0].permute(1, 2, 0).contiguous()
    mean_rgb = torch.tensor(IMG_MEAN[::-1].copy()).reshape(3, 1, 1)  # the reference subtracts per R, G, B ...
    want_seg = (q[0] - mean_rgb).flip(0).unsqueeze(0)                 # ... and then reorders to B, G, R
    src = (in_grid(x) if grid else x).to(DEV)
    u8, seg = ops.style_output(src, grid=grid, rgb=True, seg=True, mean=[float(m) for m in IMG_MEAN])
    assert torch.equal(u8.cpu(), want_u8)
    assert same_bits(seg, want_seg)
    only_u8, none = ops.style_output(src, grid=grid, rgb=True, seg=False)
    assert none is None and torch.equal(only_u8.cpu(), want_u8)
    if not grid:
        assert same_bits(st.seg_transform(x.to(DEV)), want_seg) and torch.equal(st.to_uint8(x.to(DEV)).cpu(), want_u8)


# ------------------------------------------------------------------------------------------ the convs
LAYERS = [(3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 512), (512, 256), (256, 128),
          (128, 64), (64, 3)]


@pytest.mark.parametrize("cin,cout", LAYERS)
def test_conv3x3_reflect_against_fp64(cin, cout):
    """Every distinct conv layer of the network on a 20x28 map, default forms (f16x3): the project's bar,
    max |gpu - fp64| <= 1e-3 max |fp64|."""
    g = torch.Generator().manual_seed(cin * 7 + cout)
    x = torch.randn(1, cin, 20, 28, generator=g)
    conv = sr.he_init(nn.Sequential(nn.Conv2d(cin, cout, 3)), cin + cout)[0]
    with torch.no_grad():
        want = nn.functional.conv2d(nn.ReflectionPad2d(1)(x.double()), conv.weight.double(), conv.bias.double())
    grid = ops.style_pad(x.to(DEV))
    y = ops.conv3x3_reflect(grid, conv.weight.detach().to(DEV), conv.bias.detach().to(DEV), ops.PackCache())
    assert y.shape == (1, cout, 22, 30) and torch.isfinite(y).all()
    got = y[:, :, 1:-1, 1:-1].cpu().double()
    rel = (got - want).abs().max().item() / want.abs().max().item()
    print(f"conv {cin}->{cout}: max |gpu - fp64| / max |fp64| = {rel:.3e}")
    assert rel <= 1e-3


# ------------------------------------------------------------------------------------------ the whole pass
@pytest.fixture(scope="module")
def stacks():
    return sr.he_init(sr.ref_vgg(), 21), sr.he_init(sr.ref_decoder(), 22)


@pytest.fixture(scope="module")
def stylenet(stacks):
    vgg, dec = stacks
    return net.StyleNet(vgg.state_dict(), dec.state_dict(), DEV)


@pytest.fixture(scope="module")
def images():
    g = torch.Generator().manual_seed(31)
    return torch.rand(1, 3, 37, 53, generator=g), torch.rand(1, 3, 41, 29, generator=g)


@pytest.mark.parametrize("alpha", [1.0, 0.6])
def test_whole_pass_against_fp64(stacks, stylenet, images, alpha):
    """Bar: max |gpu - fp64| <= 8 x max |torch fp32 - fp64| + 1e-5 (f16x3 carries about two mantissa bits
    fewer than fp32: 4x; another summation order: 2x)."""
    vgg, dec = stacks
    content, style = images
    want = sr.style_pass(vgg, dec, content, [style], alpha, (1.0,), torch.float64)
    own = (sr.style_pass(vgg, dec, content, [style], alpha, (1.0,), torch.float32).double() - want).abs().max().item()
    with torch.no_grad():
        got = st.style_transfer(stylenet, content.to(DEV), style.to(DEV), alpha=alpha)
        again = st.style_transfer(stylenet, content.to(DEV), style.to(DEV), alpha=alpha)
        stats = stylenet.encode_style(style.to(DEV))
        cached = st.style_transfer(stylenet, content.to(DEV), stats, alpha=alpha)
    assert got.shape == (1, 3, 40, 56) == tuple(want.shape) and net.out_hw(37, 53) == (40, 56)
    err = (got.cpu().double() - want).abs().max().item()
    print(f"style pass alpha {alpha}: max |gpu - fp64| {err:.3e}, torch-fp32 {own:.3e}, ratio {err / own:.2f}, "
          f"output range [{want.min().item():.3f}, {want.max().item():.3f}]")
    assert err <= 8.0 * own + 1e-5
    assert same_bits(got, again)      # two runs
    assert same_bits(got, cached)     # the style encoded once


def test_interpolated_styles_and_refusals(stacks, stylenet, images):
    vgg, dec = stacks
    content, style = images
    style2 = torch.rand(1, 3, 41, 29, generator=torch.Generator().manual_seed(5))
    want = sr.style_pass(vgg, dec, content, [style, style2], 1.0, (0.25, 0.75), torch.float64)
    own = (sr.style_pass(vgg, dec, content, [style, style2], 1.0, (0.25, 0.75), torch.float32).double()
           - want).abs().max().item()
    both = torch.cat([style, style2]).to(DEV)
    got = st.style_transfer(stylenet, content.to(DEV), both, interpolation_weights=(0.25, 0.75))
    err = (got.cpu().double() - want).abs().max().item()
    print(f"style pass, two styles: max |gpu - fp64| {err:.3e}, torch-fp32 {own:.3e}, ratio {err / own:.2f}")
    assert err <= 8.0 * own + 1e-5
    with pytest.raises(NotImplementedError):
        st.style_transfer(stylenet, content.to(DEV), style.to(DEV), preserve_color=True)
    with pytest.raises(ValueError):
        st.style_transfer(stylenet, content.to(DEV), both)
    with pytest.raises(ValueError):
        st.style_transfer(stylenet, content.to(DEV), style.to(DEV), alpha=1.5)


# ------------------------------------------------------------------------------------------ the tool
def test_stylize_tool_writes_what_the_api_returns(tmp_path, stacks):
    from PIL import Image
    from maxsquareloss_amd.datasets import GTA5_Dataset
    vgg, dec = stacks
    rng = np.random.default_rng(3)
    root, out1, out2 = tmp_path / "gta", tmp_path / "flat", tmp_path / "tree"
    (root / "images").mkdir(parents=True)
    (root / "labels").mkdir()
    contents = []
    for i in (1, 2):
        rgb = rng.integers(0, 256, (24, 32, 3), dtype=np.uint8)
        Image.fromarray(rgb).save(root / "images" / f"{i:05d}.png")
        Image.fromarray(rng.integers(0, 30, (24, 32), dtype=np.uint8)).save(root / "labels" / f"{i:05d}.png")
        contents.append(rgb)
    (root / "train.txt").write_text("1\n2\n")
    (root / "list.txt").write_text("images/00001.png\nimages/00002.png\n")
    style = rng.integers(0, 256, (20, 28, 3), dtype=np.uint8)
    Image.fromarray(style).save(tmp_path / "wave.png")
    torch.save(vgg.state_dict(), tmp_path / "vgg.pth")
    torch.save({"state_dict": dec.state_dict(), "loss_c_best": 0.0}, tmp_path / "decoder.pth.tar")
    base = ["--vgg", str(tmp_path / "vgg.pth"), "--decoder", str(tmp_path / "decoder.pth.tar"), "--style",
            str(tmp_path / "wave.png"), "--save_ext", "png", "--data_loader_workers", "2", "--alpha", "0.8"]

    args = stylize.parse_args(base + ["--content_dir", str(root / "images"), "--output_path", str(out1)])
    written = stylize.run(args)
    assert written == ["00001_24r32_wave.png", "00002_24r32_wave.png"]
    sn = stylize.load_net(args)
    stats = sn.encode_style([torch.from_numpy(style)])
    want = []
    for rgb, name in zip(contents, written):
        y = sn.stylize(torch.from_numpy(rgb).to(DEV), stats, 0.8)
        want.append(ops.style_output(y, grid=True)[0].cpu().numpy())
        assert want[-1].shape == (24, 32, 3) and want[-1].std() > 0
        assert np.array_equal(np.asarray(Image.open(out1 / name)), want[-1])

    args = stylize.parse_args(base + ["--content_list", str(root / "list.txt"), "--content_root", str(root),
                                      "--output_path", str(out2), "--keep_tree", "True"])
    assert stylize.run(args) == ["images/00001.png", "images/00002.png"]
    ds_args = argparse.Namespace(base_size=(32, 24), crop_size=(32, 24), random_mirror=False, random_crop=False,
                                 resize=False, seed=0)
    ds = GTA5_Dataset(ds_args, data_root_path=str(out2), list_path=str(root), gt_path=str(root / "labels"),
                      split="train")
    assert len(ds) == 2 and ds.paths(1)[0] == os.path.join(str(out2), "images", "00002.png")
    for i in (0, 1):
        rgb, ids = ds.decode(i)
        assert np.array_equal(rgb, want[i]) and ids.shape == (24, 32)
