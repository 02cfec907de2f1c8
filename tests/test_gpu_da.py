"""In-loop AdaIN domain adaptation on the GPU (tools/ADAIN.py): the kernels between the style network and the
segmentation network (msl_style_input_window, msl_style_output_resampled, msl_label_resize_nearest,
msl_predict_rectify), utils/style_transform's stylise_for_seg / crop_trans / seg_transform over them, and the
trainer.

The oracle is live torch on the CPU.  The kernels only move data, or compare values that the existing kernels
already produce bit-equal to torch, so every comparison is exact: no tolerance anywhere.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import evaluate_ref as er  # noqa: E402
import style_ref as sr  # noqa: E402
from maxsquareloss_amd import hip, ops  # noqa: E402
from maxsquareloss_amd.tools import net  # noqa: E402
from maxsquareloss_amd.utils import style_transform as st  # noqa: E402
from maxsquareloss_amd.utils.synthetic import IMG_MEAN  # noqa: E402

DEV = "cuda"
SENTINEL = 12345.0
MEAN = [float(m) for m in IMG_MEAN]
ERR_ARG = -3


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def in_grid(x, fill=SENTINEL):
    g = torch.full((1, x.size(1), x.size(2) + 2, x.size(3) + 2), fill, dtype=x.dtype)
    g[:, :, 1:-1, 1:-1] = x
    return g


def torch_index(n_in, n_out):
    """torch's own nearest index table of an axis, read off F.interpolate."""
    src = torch.arange(n_in, dtype=torch.float32).reshape(1, 1, 1, n_in)
    return F.interpolate(src, size=(1, n_out))[0, 0, 0].long()


def integer_index(n_in, n_out):
    return (torch.arange(n_out) * n_in) // n_out


def torch_seg(x):
    """The reference's seg_transform after its interpolate: mul, add, clamp, minus the mean per R, G, B, then
    B, G, R."""
    q = x.mul(255).add(0.5).clamp(0, 255)
    mean_rgb = torch.tensor(IMG_MEAN[::-1].copy()).reshape(3, 1, 1)
    return (q[0] - mean_rgb).flip(0).unsqueeze(0)


# ------------------------------------------------------------------------------ msl_style_output_resampled
def _output_data(h=24, w=56, seed=8):
    """Values in [-0.2, 1.2] with every rounding cut k/255, (k +- 0.5)/255 and their neighbours."""
    k = torch.arange(256, dtype=torch.float32)
    pts = torch.cat([k / 255, (k + 0.5) / 255, (k - 0.5) / 255])
    up, down = torch.full_like(pts, float("inf")), torch.full_like(pts, float("-inf"))
    vals = torch.cat([pts, torch.nextafter(pts, up), torch.nextafter(pts, down),
                      torch.tensor([-0.0, 0.0, -1e-3, -0.2, 1.0, 1.0000001, 1.002, 1.2, -1e-9, 0.9999999])])
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(3 * h * w, generator=g) * 1.4 - 0.2
    assert vals.numel() <= x.numel()
    x[:vals.numel()] = vals
    return x[torch.randperm(x.numel(), generator=g)].reshape(1, 3, h, w)


def test_the_resampling_case_keeps_its_point():
    """24 -> 74 and 56 -> 46 each hold a destination where torch's fp32 rule and dst * in // out differ, and
    the host-side table of utils/style_transform is torch's."""
    for n_in, n_out in ((24, 74), (56, 46), (8, 82)):
        t = torch_index(n_in, n_out)
        assert not torch.equal(t, integer_index(n_in, n_out)), (n_in, n_out)
        assert np.array_equal(st.nearest_index(n_in, n_out), t.numpy()), (n_in, n_out)


@pytest.mark.parametrize("grid", [False, True])
@pytest.mark.parametrize("size", [(74, 46), (24, 56), (24, 1), (1, 56), (7, 130)])
def test_output_resampled_is_bit_identical_to_torch(size, grid):
    x = _output_data()
    want = torch_seg(F.interpolate(x, size=size))
    src = (in_grid(x) if grid else x).to(DEV)
    out = torch.full((1, 3) + size, SENTINEL, device=DEV)
    ops.style_output_resampled(src, out, grid=grid, mean=MEAN)
    assert same_bits(out, want)
    if size == (24, 56):  # the identity is today's seg_transform, and seg_transform with a size takes this path
        assert same_bits(st.seg_transform(x.to(DEV)), want)
    assert same_bits(st.seg_transform(x.to(DEV), size=(size[1], size[0])), want)


def test_output_resampled_window_keeps_its_surroundings():
    x = _output_data()
    want = torch.full((1, 3, 80, 61), SENTINEL)
    want[:, :, 5:79, 9:55] = torch_seg(F.interpolate(x, size=(74, 46)))
    out = torch.full((1, 3, 80, 61), SENTINEL, device=DEV)
    ops.style_output_resampled(in_grid(x).to(DEV), out, (9, 5, 46, 74), grid=True, mean=MEAN)
    assert same_bits(out, want)


@pytest.mark.parametrize("dest", [(74, 46), (24, 40), (31, 93)])
def test_output_resampled_composes_two_maps(dest):
    """cropTrans then seg_transform: four 24 x 56 maps resized to 12 x 20 quadrants, stitched to 24 x 40 and
    resized to `dest`; each launch is handed the whole destination and writes its own share only, and the
    tight windows of utils/style_transform cover the same cells."""
    maps = [_output_data(seed=20 + k) for k in range(4)]
    quads = [F.interpolate(m, size=(12, 20)) for m in maps]
    stitched = torch.cat([torch.cat(quads[:2], dim=3), torch.cat(quads[2:], dim=3)], dim=2)
    want = torch_seg(F.interpolate(stitched, size=dest))
    whole = torch.full((1, 3) + dest, SENTINEL, device=DEV)
    tight = torch.full((1, 3) + dest, SENTINEL, device=DEV)
    for k, m in enumerate(maps):
        qy, qx = divmod(k, 2)
        kw = dict(grid=True, mid=(12, 20), full=(24, 40), off=(qy * 12, qx * 20), mean=MEAN)
        ops.style_output_resampled(in_grid(m).to(DEV), whole, **kw)
        dy0, dh = st._quadrant_span(24, dest[0], qy * 12, 12)
        dx0, dw = st._quadrant_span(40, dest[1], qx * 20, 20)
        ops.style_output_resampled(in_grid(m).to(DEV), tight, (dx0, dy0, dw, dh), **kw)
    assert same_bits(whole, want) and same_bits(tight, want)


def test_output_resampled_argument_errors():
    lib, s = hip.load(), hip.stream_ptr()
    x = torch.zeros(1, 3, 8, 8, device=DEV)
    out = torch.full((1, 3, 10, 10), SENTINEL, device=DEV)

    def call(xp=x.data_ptr(), mid=(10, 10), full=(0, 0), off=(0, 0), win=(0, 0, 10, 10)):
        return lib.msl_style_output_resampled(xp, 0, 8, 8, mid[0], mid[1], full[0], full[1], off[0], off[1],
                                              out.data_ptr(), 10, 10, win[0], win[1], win[2], win[3], 0.0, 0.0, 0.0, s)

    assert call(xp=None) == ERR_ARG
    assert call(win=(1, 0, 10, 10)) == ERR_ARG and call(win=(0, 3, 10, 8)) == ERR_ARG  # outside the destination
    assert call(win=(0, 0, 0, 10)) == ERR_ARG and call(win=(-1, 0, 5, 5), mid=(5, 5)) == ERR_ARG
    assert call(mid=(9, 10)) == ERR_ARG                                      # one map: mid is the window
    assert call(mid=(4, 4), full=(8, 8), off=(5, 0)) == ERR_ARG              # a part outside the stitched map
    assert call(mid=(4, 4), full=(8, 0)) == ERR_ARG
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    assert call() == 0


# ------------------------------------------------------------------------------ msl_style_input_window
def _u8_image(h=24, w=40, seed=4):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8))


def _first_conv(seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(3, 3, 1, 1, generator=g).to(DEV), torch.randn(3, generator=g).to(DEV)


WINDOWS = [((20, 12, 20, 12), (24, 40)),   # the exact x2 of cropTrans and rectification
           ((5, 3, 8, 10), (25, 82)),      # 8 -> 82 columns: the fp32 rule and the integer rule differ
           ((0, 0, 40, 24), (24, 40)),     # the whole image: msl_style_input itself
           ((39, 23, 1, 1), (2, 2)),       # one pixel magnified
           ((3, 1, 33, 20), (9, 130))]     # shrinking rows, more than one block


@pytest.mark.parametrize("window,size", WINDOWS)
@pytest.mark.parametrize("form", ["u8", "f32"])
def test_input_window_equals_style_input_of_the_gathered_image(window, size, form):
    img = _u8_image()
    w1, b1 = _first_conv()
    x0, y0, cw, ch = window
    chw = img.permute(2, 0, 1).unsqueeze(0).float()
    if form == "f32":
        chw = chw / 255 + torch.rand(1, 3, 24, 40, generator=torch.Generator().manual_seed(6)) * 1e-3
    gathered = F.interpolate(chw[:, :, y0:y0 + ch, x0:x0 + cw], size=size)
    if form == "u8":
        src, plain = img.to(DEV), gathered[0].permute(1, 2, 0).to(torch.uint8).contiguous().to(DEV)
    else:
        src, plain = chw.to(DEV), gathered.contiguous().to(DEV)
    want = ops.style_input(plain, w1, b1, cpad=5)
    got = ops.style_input_window(src, window, size, w1, b1, cpad=5)
    assert got.shape == (1, 5, size[0] + 2, size[1] + 2) and same_bits(got, want)


def test_input_window_argument_errors():
    lib, s = hip.load(), hip.stream_ptr()
    img = _u8_image().to(DEV)
    w1, b1 = _first_conv()
    y = torch.full((1, 3, 10, 10), SENTINEL, device=DEV)

    def call(win=(0, 0, 8, 8), size=(8, 8), u8=img.data_ptr(), f32=None):
        return lib.msl_style_input_window(u8, f32, 24, 40, win[0], win[1], win[2], win[3], size[0], size[1],
                                          w1.data_ptr(), b1.data_ptr(), y.data_ptr(), 3, s)

    assert call(win=(33, 0, 8, 8)) == ERR_ARG and call(win=(0, 17, 8, 8)) == ERR_ARG
    assert call(win=(-1, 0, 8, 8)) == ERR_ARG and call(win=(0, 0, 0, 8)) == ERR_ARG
    assert call(u8=None) == ERR_ARG and call(f32=img.data_ptr()) == ERR_ARG
    assert call(size=(1, 8)) == -1  # MSL_ERR_SHAPE: reflection needs two rows
    torch.cuda.synchronize()
    assert (y == SENTINEL).all()
    assert call() == 0


# ------------------------------------------------------------------------------ msl_label_resize_nearest
@pytest.mark.parametrize("size", [(74, 46), (24, 40), (1, 1), (9, 300)])
def test_label_resize_equals_torch(size):
    rng = np.random.default_rng(11)
    lab = torch.from_numpy(rng.integers(-1, 19, (24, 40)).astype(np.int64))
    lab[0, :5] = 255
    lab[23, 39] = 255
    want = F.interpolate(lab.float()[None, None], size=size)[0, 0].long()
    got = ops.label_resize_nearest(lab.to(DEV), size)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), want)
    img, lab2 = st.seg_transform(torch.rand(1, 3, 24, 40).to(DEV), lab[None].to(DEV), size=(size[1], size[0]))
    assert img.shape == (1, 3) + size and torch.equal(lab2.cpu(), want[None])
    lib = hip.load()
    assert lib.msl_label_resize_nearest(None, 24, 40, got.data_ptr(), size[0], size[1], hip.stream_ptr()) == ERR_ARG
    assert lib.msl_label_resize_nearest(lab.to(DEV).data_ptr(), 24, 40, got.data_ptr(), 0, 4, hip.stream_ptr()) == ERR_ARG


# ------------------------------------------------------------------------------ stylise_for_seg, crop_trans
@pytest.fixture(scope="module")
def stacks():
    return sr.he_init(sr.ref_vgg(), 21), sr.he_init(sr.ref_decoder(), 22)


@pytest.fixture(scope="module")
def stylenet(stacks):
    vgg, dec = stacks
    return net.StyleNet(vgg.state_dict(), dec.state_dict(), DEV)


@pytest.fixture(scope="module")
def style_stats(stylenet):
    g = torch.Generator().manual_seed(41)
    styles = torch.rand(2, 3, 20, 28, generator=g)
    return stylenet.encode_style(styles.to(DEV))


WEIGHTS = (0.25, 0.75)


def _interior(y):
    return y[:, :3, 1:-1, 1:-1].contiguous()


@pytest.mark.parametrize("seg_size", [None, (46, 74), (40, 24), (32, 16)])
def test_stylise_for_seg_equals_the_composition(stylenet, style_stats, seg_size):
    content = _u8_image(seed=9)
    got = st.stylise_for_seg(stylenet, content.to(DEV), style_stats, seg_size, alpha=0.8, weights=WEIGHTS)
    y = _interior(stylenet.stylize(content.to(DEV), style_stats, 0.8, WEIGHTS)).cpu()
    if seg_size is not None:
        y = F.interpolate(y, size=(seg_size[1], seg_size[0]))
    want = st.seg_transform(y.to(DEV))
    assert same_bits(got, want) and same_bits(want, torch_seg(y))


@pytest.mark.parametrize("seg_size", [None, (46, 74), (32, 16)])
def test_crop_trans_equals_the_composition(stylenet, style_stats, seg_size):
    content = _u8_image(seed=10)
    chw = content.permute(2, 0, 1).unsqueeze(0).float() / 255  # torchvision's ToTensor
    quads = []
    for qy in (0, 1):
        for qx in (0, 1):
            c = F.interpolate(chw[:, :, qy * 12:qy * 12 + 12, qx * 20:qx * 20 + 20], size=(24, 40))
            ct = _interior(stylenet.stylize(c.to(DEV), style_stats, 1.0, WEIGHTS)).cpu()
            quads.append(F.interpolate(ct, size=(12, 20)))
    y = torch.cat([torch.cat(quads[:2], dim=3), torch.cat(quads[2:], dim=3)], dim=2)
    if seg_size is not None:
        y = F.interpolate(y, size=(seg_size[1], seg_size[0]))
    want = st.seg_transform(y.to(DEV))
    for src in (content.to(DEV), chw.to(DEV)):
        got = st.crop_trans(stylenet, src, style_stats, (20, 12), (40, 24), seg_size, weights=WEIGHTS)
        assert same_bits(got, want)
    with pytest.raises(hip.MSLError):
        st.crop_trans(stylenet, content.to(DEV), style_stats, (20, 12), (48, 24), seg_size, weights=WEIGHTS)


# ------------------------------------------------------------------------------ msl_predict_rectify
def rectify_ref(base, crops, hw, segy0):
    """Trainer.validate's rectification (tools/train_source.py:457-475 and :353-381 of the reference) restated:
    (class map int64 [ho, wo], share of the region's pixels replaced)."""
    ho, wo = hw
    pred = er.up(base, hw)[0].numpy()
    maxpred, argpred = np.amax(pred, axis=0), np.argmax(pred, axis=0)
    replaced = 0
    for k, crop in enumerate(crops):
        new = F.interpolate(er.up(crop, hw), size=[int(0.5 * ho), int(0.5 * wo)])[0].numpy()
        new_arg, new_max = np.argmax(new, axis=0), np.amax(new, axis=0)
        segx0 = k * (wo // 2)
        with np.errstate(invalid="ignore"):
            mask = new_max > maxpred[segy0:int(segy0 + 0.5 * ho), segx0:int(segx0 + 0.5 * wo)]
        argpred[segy0:int(segy0 + 0.5 * ho), segx0:int(segx0 + 0.5 * wo)][mask] = new_arg[mask]
        replaced += int(mask.sum())
    return argpred, replaced / float((ho // 2) * wo)


def _rectify(base, crops, hw, segy0, C):
    lab = er.labels(C, *hw)
    cm = torch.zeros(C * C, dtype=torch.int64, device=DEV)
    arg = ops.predict_rectify(base.to(DEV), crops[0].to(DEV), crops[1].to(DEV), hw, segy0, lab.to(DEV).reshape(-1), cm,
                              want_argmax=True)
    return arg.cpu().numpy().reshape(hw), cm.cpu().numpy().reshape(C, C), lab


RECTIFY_SHAPES = [(19, 9, 17, 32, 48, 5), (13, 5, 7, 18, 22, 2), (16, 33, 65, 66, 130, 16),
                  (19, 9, 17, 32, 48, 0), (19, 9, 17, 32, 48, 16)]


@pytest.mark.parametrize("C,hi,wi,ho,wo,segy0", RECTIFY_SHAPES)
def test_rectify_equals_the_reference_slicing(C, hi, wi, ho, wo, segy0):
    base = er.logits(C, hi, wi, "rb")
    crops = [er.logits(C, hi, wi, "rc0"), er.logits(C, hi, wi, "rc1")]
    want, share = rectify_ref(base, crops, (ho, wo), segy0)
    print(f"rectify {C}x{hi}x{wi} -> {ho}x{wo} at {segy0}: {share:.2f} of the region replaced")
    assert 0.2 < share < 0.8
    cls, cm, lab = _rectify(base, crops, (ho, wo), segy0, C)
    assert np.array_equal(cls, want)
    assert np.array_equal(cm, er.confusion_ref(lab, want.reshape(-1), C))
    plain = ops.predict_up(base.to(DEV), (ho, wo), want_argmax=True).cpu().numpy().reshape(ho, wo)
    outside = np.ones((ho, wo), bool)
    outside[segy0:segy0 + ho // 2] = False
    assert np.array_equal(cls[outside], plain[outside]) and (cls != plain).any()


def test_rectify_nan_and_ties():
    C, hi, wi, hw, segy0 = 19, 9, 17, (32, 48), 5
    crops = [er.logits(C, hi, wi, "rc0"), er.logits(C, hi, wi, "rc1")]
    for base, cr in ((er.logits(C, hi, wi, "rb", nan=True), crops),
                     (er.logits(C, hi, wi, "rb"), [er.logits(C, hi, wi, "rc0", nan=True), crops[1]])):
        want, _ = rectify_ref(base, cr, hw, segy0)
        cls, cm, lab = _rectify(base, cr, hw, segy0, C)
        assert np.array_equal(cls, want) and np.array_equal(cm, er.confusion_ref(lab, want.reshape(-1), C))
    # all logits equal: nothing is replaced and the lowest class wins.  Zero, the one value every bilinear
    # blend (1 - l) * v + l * v reproduces exactly; with another one the reference's own blends differ in the
    # last bit from pixel to pixel.
    flat = torch.zeros(1, C, hi, wi)
    want, share = rectify_ref(flat, [flat, flat], hw, segy0)
    cls, _, _ = _rectify(flat, [flat, flat], hw, segy0, C)
    assert share == 0.0 and (want == 0).all() and (cls == 0).all()
    # and equal maps with different classes ahead: ties everywhere, the strict comparison keeps the base's class
    tie = er.logits(C, hi, wi, "rb")
    want, share = rectify_ref(tie, [tie, tie], (18, 34), 4)
    cls, _, _ = _rectify(tie, [tie, tie], (18, 34), 4, C)
    assert np.array_equal(cls, want)


def test_rectify_argument_errors():
    lib, s = hip.load(), hip.stream_ptr()
    low = er.logits(19, 3, 3).to(DEV)
    big = torch.zeros(1, 33, 3, 3, device=DEV)
    arg = torch.full((8 * 10,), -7, dtype=torch.int32, device=DEV)
    lab = torch.zeros(8 * 10, dtype=torch.int64, device=DEV)
    p = low.data_ptr()

    def call(base=p, c0=p, c1=p, c=19, ho=8, wo=10, segy0=2, label=None, cm=None, out=arg.data_ptr()):
        return lib.msl_predict_rectify(base, c0, c1, c, 3, 3, ho, wo, segy0, label, cm, out, s)

    assert call(ho=7) == ERR_ARG and call(wo=9) == ERR_ARG
    assert call(segy0=-1) == ERR_ARG and call(segy0=5) == ERR_ARG
    assert call(base=big.data_ptr(), c0=big.data_ptr(), c1=big.data_ptr(), c=33) == ERR_ARG
    assert call(base=None) == ERR_ARG and call(c0=None) == ERR_ARG and call(c1=None) == ERR_ARG
    assert call(out=None) == ERR_ARG and call(label=lab.data_ptr()) == ERR_ARG and call(ho=0) == ERR_ARG
    torch.cuda.synchronize()
    assert (arg == -7).all()
    assert call() == 0 and call(segy0=4) == 0 and call(segy0=0) == 0


# ------------------------------------------------------------------------------ the trainer (tools/ADAIN.py)
@pytest.fixture(scope="module")
def trees(tmp_path_factory, stacks):
    """Tiny GTA5 and Cityscapes trees, two style images and the style network's checkpoints as files."""
    from PIL import Image
    from test_input_pipeline import write_tree
    root = tmp_path_factory.mktemp("da")
    spaths, _ = write_tree(root / "gta", n=3, val_n=1, hw=(40, 56), gta=True, seed=4)
    tpaths, _ = write_tree(root / "city", n=2, val_n=2, hw=(44, 60), seed=6)
    vgg, dec = stacks
    torch.save(vgg.state_dict(), root / "vgg.pth")
    torch.save({"state_dict": dec.state_dict(), "loss_c_best": 0.0}, root / "decoder.pth.tar")
    rng = np.random.default_rng(3)
    (root / "styles").mkdir()
    for name in ("b.png", "a.png"):
        Image.fromarray(rng.integers(0, 256, (20, 28, 3), dtype=np.uint8)).save(root / "styles" / name)
    return root, spaths, tpaths


def _argv(trees, base="48,32", seg="48,32", extra=()):
    root, spaths, tpaths = trees
    return ["--imagenet_pretrained", "False", "--save_dir", "", "--resize", "True", "--random_crop", "False",
            "--base_size", base, "--target_base_size", base, "--crop_size", "24,16", "--target_crop_size", "24,16",
            "--seg_size", seg, "--seed", "21", "--data_loader_workers", "2", "--round_num", "1",
            "--epoch_each_round", "1", "--source_data_path", spaths["data_root_path"],
            "--target_data_path", tpaths["data_root_path"], "--target_list_path", tpaths["list_path"],
            "--target_gt_path", tpaths["gt_path"], "--vgg", str(root / "vgg.pth"),
            "--decoder", str(root / "decoder.pth.tar"), "--style", str(root / "styles"),
            "--style_interpolation_weight", "1,3", "--alpha", "0.8", "--target_mode", "maxsquare",
            "--lambda_target", "0.1"] + list(extra)


def _da_trainer(trees, **kw):
    from maxsquareloss_amd.tools import ADAIN
    from maxsquareloss_amd.tools.train_source import init_args
    args, _, _ = init_args(ADAIN.parse_args(_argv(trees, **kw)))
    return ADAIN.UDATrainer(args, cuda=True, train_id="da")


def _close(tr):
    for items in (tr._source_items, tr._target_items):
        if items is not None:
            items.close()
    tr.dataloader.close()
    tr.source_loader.close()


def _weights(tr):
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in tr.model.state_dict().items()}


def _same_weights(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if a[k].dtype == torch.float32:
            assert same_bits(a[k], b[k]), k
        else:
            assert torch.equal(a[k], b[k]), k


def test_trainer_eager_graph_and_the_plain_step_agree(trees):
    """Two iterations at 48 x 32: eager and --graph True leave bit-identical weights, and so does solve_gta5's
    plain uda_step (poly off) fed with stylise_for_seg's tensors of the same items."""
    from maxsquareloss_amd.tools import ADAIN, solve_gta5
    runs = {}
    for graph in (False, True):
        tr = _da_trainer(trees, extra=["--graph", str(graph)])
        assert tr.dataloader.num_iterations == 2 and tr.args.DA and tr.style_weights == (0.25, 0.75)
        assert [os.path.basename(p) for p in ADAIN.style_files(tr.args.style)] == ["a.png", "b.png"]
        before = _weights(tr)
        tr.optimizer.zero_grad()
        tr.train_one_epoch(0)
        runs[graph] = _weights(tr)
        assert tr.current_iter == 2 and torch.isfinite(tr.loss_seg_value) and torch.isfinite(tr.loss_target_value)
        assert any(not torch.equal(before[k], runs[graph][k]) for k in before)
        if graph:
            assert tr._graphed is not None and tr._graphed.replays == 1
        lrs = tr.optimizer.group_lrs()
        assert lrs == (tr.args.lr, 10 * tr.args.lr)  # no poly schedule; one epoch is no plateau
        _close(tr)
    _same_weights(runs[False], runs[True])

    src = _da_trainer(trees, extra=["--graph", "False"])      # its loaders, style network and statistics
    plain = solve_gta5.UDATrainer(src.args, cuda=True, train_id="plain")
    plain.poly_lr_scheduler = lambda *a, **k: None
    plain.optimizer.zero_grad()
    plain.model.train()
    plain.iter_num = 2
    items_s, items_t = src.source_dataloader.cycle(), src.target_dataloader.cycle()
    for _ in range(2):
        c_s, y_s, _ = next(items_s)
        c_t, _, _ = next(items_t)
        assert c_s.dtype == torch.uint8 and c_s.shape == (32, 48, 3) and y_s.shape == (1, 32, 48)
        x_s = st.stylise_for_seg(src.network, c_s, src.style_stats, (48, 32), alpha=0.8, weights=(0.25, 0.75))
        x_t = st.stylise_for_seg(src.network, c_t, src.style_stats, (48, 32), alpha=0.8, weights=(0.25, 0.75))
        plain.uda_step(x_s, y_s, x_t)
    _same_weights(runs[False], _weights(plain))
    items_s.close()
    items_t.close()
    _close(src)
    plain.dataloader.close()
    plain.source_loader.close()


def test_trainer_with_crop_trans(trees):
    tr = _da_trainer(trees, seg="40,24", extra=["--crop_trans", "True"])
    seen, step = [], tr.uda_step

    def spy(x_s, y_s, x_t):
        seen.append((x_s.clone(), y_s.clone(), x_t.clone()))
        step(x_s, y_s, x_t)

    tr.uda_step = spy
    tr.optimizer.zero_grad()
    tr.train_one_epoch(0)
    torch.cuda.synchronize()
    assert tr.current_iter == 2 and len(seen) == 2
    assert torch.isfinite(tr.loss_seg_value) and torch.isfinite(tr.loss_target_value)
    for x_s, y_s, x_t in seen:
        assert x_s.shape == (1, 3, 24, 40) == x_t.shape and y_s.shape == (1, 24, 40) and torch.isfinite(x_s).all()
    _close(tr)


def test_main_with_validation_and_rectification(trees):
    """One epoch of main(): the steps, validate_source, then the rectified target validation, whose matrix is the
    one the reference's slicing gives on the same y0 draws."""
    import random
    tr = _da_trainer(trees, base="64,48", seg="48,32", extra=["--rectification", "True"])
    calls = []
    for name in ("validate", "validate_source", "uda_step"):
        def wrap(*a, _f=getattr(tr, name), _n=name, **kw):
            out = _f(*a, **kw)
            calls.append((_n, out))
            return out
        setattr(tr, name, wrap)
    tr.main()
    torch.cuda.synchronize()
    assert [n for n, _ in calls] == ["uda_step"] * 2 + ["validate_source", "validate"]
    for name, out in calls[2:]:
        assert len(out) == 4 and np.isfinite(out[2]) and 0.0 <= out[2] <= 1.0, (name, out)
    rng = random.Random(tr.args.seed)
    assert tr.rect_draws == [rng.randint(int(0.083 * 48), int(0.25 * 48)) for _ in range(2)]
    want = np.zeros((19, 19))
    tr.model.eval()
    with torch.no_grad():
        for (content, label, _), y0 in zip(tr.dataloader.val_loader, tr.rect_draws):
            assert content.shape == (48, 64, 3)
            x, y = tr.seg_input(content, label)
            assert x.shape == (1, 3, 32, 48) and y.shape == (1, 32, 48)
            low = tr.model.predict_low(x)[0].cpu()
            crops = []
            for x0 in (0, 32):
                gathered = F.interpolate(content.cpu().permute(2, 0, 1)[None, :, y0:y0 + 24, x0:x0 + 32].float(),
                                         size=(48, 64))[0].permute(1, 2, 0).to(torch.uint8).contiguous()
                xc = st.stylise_for_seg(tr.network, gathered.to(DEV), tr.style_stats, (48, 32), alpha=0.8,
                                        weights=tr.style_weights)
                crops.append(tr.model.predict_low(xc)[0].cpu())
            cls, _ = rectify_ref(low, crops, (32, 48), int((y0 / 48) * 32))
            want += er.confusion_ref(y.cpu().numpy(), cls.reshape(-1), 19)
    assert want.sum() > 0 and np.array_equal(tr.rect_eval.confusion_matrix, want)
    _close(tr)


def test_sizes_refused_before_anything_is_built(trees):
    from maxsquareloss_amd.tools import ADAIN
    from maxsquareloss_amd.tools.train_source import init_args
    bad = [dict(base="48,33", seg="48,32", extra=["--rectification", "True"]),       # odd H0
           dict(base="49,32", seg="48,32", extra=["--rectification", "True"]),       # odd W0
           dict(base="48,32", seg="46,31", extra=["--rectification", "True"]),       # odd Hs
           dict(base="48,32", seg="45,30", extra=["--rectification", "True"]),       # odd Ws
           dict(base="50,34", seg="48,32", extra=["--crop_trans", "True"]),          # base != 2 * crop
           dict(base="44,28", seg="44,28")]                                          # seg == base, no multiple of 8
    for kw in bad:
        args, _, _ = init_args(ADAIN.parse_args(_argv(trees, **kw)))
        with pytest.raises(hip.MSLError):
            ADAIN.UDATrainer(args, cuda=True)
    args, _, _ = init_args(ADAIN.parse_args(_argv(trees, base="44,28", seg="48,32")))
    ADAIN.check_sizes(args)                                                           # resized: any base will do
