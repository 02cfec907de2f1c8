"""GPU tests of the file-backed input pipeline: csrc/resample.hip through utils/preprocess.py
resize_image / resize_label against the reference loader's recorded outputs
(tests/golden/input_pipeline_kat.npz) byte for byte - no Pillow needed for those - and the
file-backed trainers / evaluator on a tiny tree of PNGs (Pillow needed to write and decode them)."""
import argparse
import random

import numpy as np
import pytest
import torch

from test_input_pipeline import CASES, GOLD, _NoFiles, _gen, chain_args, f32_of, write_tree

pytestmark = pytest.mark.gpu

LUTS = {"city19": ("cityscapes", False), "city16": ("cityscapes", True), "gta19": ("gta5", False), "gta16": ("gta5", True)}


@pytest.fixture(scope="module")
def fix():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def gen():
    return _gen()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_image(fix, rgb, out_wh, want_u8, crop=None, mirror=False, tag=""):
    from maxsquareloss_amd.utils.preprocess import resize_image
    d = dev(rgb)
    u8 = resize_image(d, out_wh, crop, mirror, as_uint8=True).cpu().numpy()
    f32 = resize_image(d, out_wh, crop, mirror, mean=fix["img_mean"]).cpu().numpy()
    assert u8.shape == want_u8.shape and f32.shape == (1, 3) + want_u8.shape[:2]
    assert np.array_equal(u8, want_u8), f"{tag}: {(u8 != want_u8).sum()} uint8 bytes differ"
    assert f32[0].tobytes() == f32_of(fix, want_u8).tobytes(), f"{tag}: fp32 output differs"


@pytest.mark.parametrize("case", range(len(CASES)))
def test_resize_equals_the_reference_recording(fix, gen, case):
    from maxsquareloss_amd.utils.preprocess import build_lut, resize_label
    h, w, ow, oh = CASES[case]
    ids = gen.kat_input(fix, f"c{case}_ids")
    for m in (0, 1):
        for k in "us":
            check_image(fix, gen.kat_input(fix, f"c{case}_{k}_rgb"), (ow, oh), fix[f"c{case}_{k}_m{m}_u8"],
                        mirror=bool(m), tag=f"case {case} {k} mirror {m}")
        raw = resize_label(dev(ids), (ow, oh), None, mirror=bool(m)).cpu().numpy()
        assert np.array_equal(raw, fix[f"c{case}_m{m}_ids"])
        n = 0
        for tag, (ds, c16) in LUTS.items():
            if f"c{case}_m{m}_{tag}" in fix:
                lab = resize_label(dev(ids), (ow, oh), build_lut(ds, class_16=c16), mirror=bool(m))
                assert lab.dtype == torch.int64 and lab.shape == (1, oh, ow)
                assert np.array_equal(lab[0].cpu().numpy(), fix[f"c{case}_m{m}_{tag}"].astype(np.int64)), (tag, m)
                n += 1
        assert n == (4 if m == 0 else 1)


def test_crop_at_an_odd_offset(fix, gen):
    from maxsquareloss_amd.utils.preprocess import build_lut, resize_label
    box = tuple(int(v) for v in fix["crop_box"])
    ids = gen.kat_input(fix, "crop_ids")
    for j, (ow, oh) in enumerate(fix["crop_sizes"]):
        for m in (0, 1):
            for k in "us":
                check_image(fix, gen.kat_input(fix, f"crop_{k}_rgb"), (int(ow), int(oh)), fix[f"crop_{k}_o{j}_m{m}_u8"],
                            crop=box, mirror=bool(m), tag=f"crop size {j} {k} mirror {m}")
            raw = resize_label(dev(ids), (ow, oh), None, crop=box, mirror=bool(m)).cpu().numpy()
            assert np.array_equal(raw, fix[f"crop_o{j}_m{m}_ids"])
            lab = resize_label(dev(ids), (ow, oh), build_lut("cityscapes"), crop=box, mirror=bool(m))
            assert np.array_equal(lab[0].cpu().numpy(), fix[f"crop_o{j}_m{m}_city19"].astype(np.int64))


def test_chained_transforms_equal_the_reference(fix, gen):
    rgb, ids = gen.kat_input(fix, "crop_u_rgb"), gen.kat_input(fix, "crop_ids")
    for name, val in (("chain_train0", False), ("chain_train1", False), ("chain_val0", True)):
        ds = _NoFiles(chain_args(fix, val=val), training=not val)
        ds.rng = random.Random(int(fix[name + "_seed"]))
        plan = ds.plan(rgb.shape[1], rgb.shape[0])
        img, lab = ds.device_transform(dev(rgb), dev(ids), plan)
        assert img.cpu().numpy()[0].tobytes() == f32_of(fix, fix[name + "_u8"]).tobytes(), name
        assert np.array_equal(lab[0].cpu().numpy(), fix[name + "_city19"].astype(np.int64)), name
        himg, hlab = ds.host_transform(rgb, ids, plan)
        assert torch.equal(img.cpu(), himg) and torch.equal(lab.cpu(), hlab)


def test_bad_arguments_return_their_status_without_launching():
    from maxsquareloss_amd import hip
    from maxsquareloss_amd.utils import resample
    lib = hip.load()
    ERR = -3
    sh, sw, ow, oh = 30, 50, 20, 12
    src = torch.zeros((sh, sw, 3), dtype=torch.uint8, device="cuda")
    sentinel_u8 = torch.full((oh, ow, 3), 77, dtype=torch.uint8, device="cuda")
    sentinel_f32 = torch.full((3, oh, ow), 5.0, device="cuda")

    def table(n_in, n_out):
        b, k, ks = resample.bicubic_table(n_in, n_out)
        return np.ascontiguousarray(b), dev(np.concatenate([b, k], axis=1).T), ks

    assert lib.msl_resize_workspace(sh, ow) == sh * ow * 3
    ws = torch.empty(sh * ow * 3, dtype=torch.uint8, device="cuda")
    xb, xk, xks = table(sw, ow)
    yb, yk, yks = table(sh, oh)

    def call(**kw):
        a = dict(src=src.data_ptr(), sh=sh, sw=sw, x0=0, y0=0, cw=sw, ch=sh, mirror=0, xb=xb.ctypes.data,
                 xk=xk.data_ptr(), xks=xks, yb=yb.ctypes.data, yk=yk.data_ptr(), yks=yks, ow=ow, oh=oh,
                 out_u8=sentinel_u8.data_ptr(), out_f32=sentinel_f32.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws.numel())
        a.update(kw)
        return lib.msl_resize_bicubic_rgb(a["src"], a["sh"], a["sw"], a["x0"], a["y0"], a["cw"], a["ch"], a["mirror"],
                                          a["xb"], a["xk"], a["xks"], a["yb"], a["yk"], a["yks"], a["ow"], a["oh"],
                                          a["out_u8"], a["out_f32"], 1.0, 2.0, 3.0, a["ws"], a["ws_bytes"],
                                          hip.stream_ptr())

    bad_b = xb.copy()
    bad_b[-1, 0] += 1                       # the last row's taps now end one column past the crop
    neg_b = xb.copy()
    neg_b[0, 0] = -1
    wide_b = xb.copy()
    wide_b[3, 1] = xks + 1
    cases = dict(
        crop_past_the_right_edge=dict(x0=1), crop_past_the_bottom=dict(y0=1), negative_offset=dict(x0=-1, cw=sw - 1),
        empty_crop=dict(cw=0), no_source=dict(src=None), no_output=dict(out_u8=None, out_f32=None),
        bounds_leave_the_crop=dict(xb=bad_b.ctypes.data), negative_first_tap=dict(xb=neg_b.ctypes.data),
        more_taps_than_ks=dict(xb=wide_b.ctypes.data), table_built_for_a_wider_crop=dict(cw=sw - 3),
        y_table_built_for_a_taller_crop=dict(ch=sh - 2), ks_zero=dict(xks=0), ks_65=dict(yks=65),
        half_a_table=dict(xk=None), other_half=dict(yb=None), no_x_pass_but_sizes_differ=dict(xb=None, xk=None),
        no_y_pass_but_sizes_differ=dict(yb=None, yk=None), short_workspace=dict(ws_bytes=ws.numel() - 1),
        no_workspace=dict(ws=None), zero_output_size=dict(ow=0))
    for name, kw in cases.items():
        assert call(**kw) == ERR, name
    torch.cuda.synchronize()
    assert bool((sentinel_u8 == 77).all()) and bool((sentinel_f32 == 5.0).all()), "a refused call launched"
    assert call() == 0                       # the same arguments, unbroken, are accepted
    torch.cuda.synchronize()
    assert not bool((sentinel_u8 == 77).all())

    ids = torch.zeros((sh, sw), dtype=torch.uint8, device="cuda")
    out8 = torch.full((oh, ow), 77, dtype=torch.uint8, device="cuda")
    out64 = torch.full((oh, ow), 77, dtype=torch.int64, device="cuda")
    xt, yt = dev(np.array(resample.nearest_table(sw, ow))), dev(np.array(resample.nearest_table(sh, oh)))
    lut = torch.zeros(256, dtype=torch.int32, device="cuda")

    def ncall(**kw):
        a = dict(ids=ids.data_ptr(), x0=0, y0=0, cw=sw, ch=sh, xt=xt.data_ptr(), yt=yt.data_ptr(), ow=ow, oh=oh,
                 lut=lut.data_ptr(), o8=out8.data_ptr(), o64=out64.data_ptr())
        a.update(kw)
        return lib.msl_resize_nearest_label(a["ids"], sh, sw, a["x0"], a["y0"], a["cw"], a["ch"], 0, a["xt"], a["yt"],
                                            a["ow"], a["oh"], a["lut"], a["o8"], a["o64"], hip.stream_ptr())

    for name, kw in dict(crop_outside=dict(x0=2), negative=dict(y0=-1, ch=sh - 1), no_ids=dict(ids=None),
                         no_output=dict(o8=None, o64=None), trainids_without_a_table=dict(lut=None),
                         identity_but_sizes_differ=dict(xt=None), identity_y_but_sizes_differ=dict(yt=None),
                         zero_size=dict(oh=0)).items():
        assert ncall(**kw) == ERR, name
    torch.cuda.synchronize()
    assert bool((out8 == 77).all()) and bool((out64 == 77).all())
    assert ncall() == 0 and ncall(lut=None, o64=None) == 0
    torch.cuda.synchronize()
    assert bool((out8 == 0).all()) and bool((out64 == 0).all())
    with pytest.raises(hip.MSLError, match="leaves"):
        from maxsquareloss_amd.utils.preprocess import resize_image
        resize_image(src, (ow, oh), crop=(45, 0, 10, 10))


def test_side_stream_and_captured_graph(fix, gen):
    """Stream-ordered and capturable: the same bytes on a side stream, and from one captured graph
    replayed with new source bytes in the static input."""
    from maxsquareloss_amd.utils.preprocess import build_lut, resize_image, resize_label
    box = tuple(int(v) for v in fix["crop_box"])
    ow, oh = (int(v) for v in fix["crop_sizes"][0])
    lut = build_lut("cityscapes")
    srcs = [gen.kat_input(fix, "crop_u_rgb"), gen.kat_input(fix, "crop_s_rgb")]
    ids = gen.kat_input(fix, "crop_ids")
    want = [fix[f"crop_{k}_o0_m1_u8"] for k in "us"]

    def body(x, y):
        return (resize_image(x, (ow, oh), box, True, mean=fix["img_mean"]), resize_image(x, (ow, oh), box, True, as_uint8=True),
                resize_label(y, (ow, oh), lut, box, True))

    x, y = dev(srcs[0]), dev(ids)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        f32, u8, lab = body(x, y)   # also builds every cached table before the capture
    side.synchronize()
    assert np.array_equal(u8.cpu().numpy(), want[0]) and f32[0].cpu().numpy().tobytes() == f32_of(fix, want[0]).tobytes()
    assert np.array_equal(lab[0].cpu().numpy(), fix["crop_o0_m1_city19"].astype(np.int64))

    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        f32, u8, lab = body(x, y)
    for n in (1, 0, 1):  # new source bytes before every replay
        x.copy_(dev(srcs[n]))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(u8.cpu().numpy(), want[n]), n
        assert f32[0].cpu().numpy().tobytes() == f32_of(fix, want[n]).tobytes(), n
        assert np.array_equal(lab[0].cpu().numpy(), fix["crop_o0_m1_city19"].astype(np.int64))


# ------------------------------------------------------------------------------------ trainers on files
OW, OH = 256, 128      # network input (w, h)
CROP = "120,72"
SRC_HW = (96, 160)


def _common(extra):
    return ["--imagenet_pretrained", "False", "--save_dir", "", "--random_crop", "True", "--resize", "True",
            "--base_size", f"{OW},{OH}", "--crop_size", CROP, "--target_base_size", f"{OW},{OH}",
            "--target_crop_size", CROP, "--iter_max", "200000", "--seed", "21", *extra]


def _expected_items(loader_cls, args, paths, count, wrap=None):
    """The first `count` training items as the host transform (utils/resample.py) gives them, from a
    second loader with the same arguments and seed."""
    ld = loader_cls(args, training=True, datasets_path=wrap(paths) if wrap else paths)
    out = []
    while len(out) < count:
        for rgb, ids, plan, ident, _ in ld.data_loader.host_items():
            out.append(ld.data_loader.dataset.host_transform(rgb, ids, plan) + (ident,))
            if len(out) == count:
                break
    ld.close()
    return out


def test_trainer_on_files(tmp_path):
    pytest.importorskip("PIL")
    from maxsquareloss_amd.datasets import City_DataLoader
    from maxsquareloss_amd.tools.train_source import Trainer, add_train_args, init_args
    paths, _ = write_tree(tmp_path, n=2, val_n=1, hw=SRC_HW)
    argv = _common(["--data_root_path", paths["data_root_path"], "--iter_stop", "2", "--data_loader_workers", "2"])
    args, _, _ = init_args(add_train_args(argparse.ArgumentParser()).parse_args(argv))
    args.seg_size = (OW, OH)
    tr = Trainer(args, cuda=True)
    assert tr.file_backed and tr.dataloader.num_iterations == 2 and tr.epoch_num == 1
    seen, step = [], tr.source_step

    def spy(x, y):
        seen.append((x.clone(), y.clone()))
        loss = step(x, y)
        seen.append(loss.detach().clone())
        return loss

    tr.source_step = spy
    tr.train()
    assert tr.current_iter == 2 and len(seen) == 4
    want = _expected_items(City_DataLoader, args, paths, 2, wrap=lambda p: {"Cityscapes": p})
    for n in range(2):
        x, y = seen[2 * n]
        assert x.is_cuda and x.shape == (1, 3, OH, OW) and y.dtype == torch.int64 and y.shape == (1, OH, OW)
        assert torch.equal(x.cpu(), want[n][0]) and torch.equal(y.cpu(), want[n][1]), n
        assert torch.isfinite(seen[2 * n + 1]).all()
    assert tr._validator is not None and tr._validator.valid_iterations == 1  # the val split was walked
    assert tr._validator.Eval.confusion_matrix.sum() > 0
    tr.dataloader.close()


@pytest.mark.parametrize("graph", [False, True])
def test_uda_trainer_on_files(tmp_path, graph):
    pytest.importorskip("PIL")
    from maxsquareloss_amd.datasets import City_DataLoader, GTA5_DataLoader
    from maxsquareloss_amd.tools.solve_gta5 import UDATrainer, build_parser
    from maxsquareloss_amd.tools.train_source import init_args
    import copy
    spaths, _ = write_tree(tmp_path / "gta", n=3, val_n=1, hw=SRC_HW, gta=True, seed=3)
    tpaths, _ = write_tree(tmp_path / "city", n=2, val_n=1, hw=SRC_HW, seed=4)
    argv = _common(["--source_data_path", spaths["data_root_path"], "--target_data_path", tpaths["data_root_path"],
                    "--graph", str(graph), "--data_loader_workers", "2", "--round_num", "1", "--epoch_each_round", "1"])
    args, _, _ = init_args(build_parser().parse_args(argv))
    args.seg_size = (OW, OH)
    tr = UDATrainer(args, cuda=True)
    assert tr.file_backed and tr.dataloader.num_iterations == 2 and len(tr.source_dataloader) == 3
    seen, step = [], tr.uda_step

    def spy(x_s, y_s, x_t):
        seen.append((x_s.clone(), y_s.clone(), x_t.clone()))
        step(x_s, y_s, x_t)
        seen.append((tr.loss_val.detach().clone(), tr.loss_target.detach().clone()))

    tr.uda_step = spy
    tr.optimizer.zero_grad()
    tr.train_one_epoch()
    torch.cuda.synchronize()
    assert tr.current_iter == 2 and len(seen) == 4
    src = _expected_items(GTA5_DataLoader, args, spaths, 2)
    targs = copy.copy(args)
    targs.base_size, targs.crop_size = args.target_base_size, args.target_crop_size
    tgt = _expected_items(City_DataLoader, targs, tpaths, 2, wrap=lambda p: {"Cityscapes": p})
    for n in range(2):
        x_s, y_s, x_t = seen[2 * n]
        assert x_s.shape == x_t.shape == (1, 3, OH, OW)
        assert torch.equal(x_s.cpu(), src[n][0]) and torch.equal(y_s.cpu(), src[n][1]), n
        assert torch.equal(x_t.cpu(), tgt[n][0]), n
        assert all(torch.isfinite(v).all() for v in seen[2 * n + 1])
    if graph:
        assert tr._graphed is not None
    tr.dataloader.close()
    tr.source_loader.close()


def test_evaluater_on_files_equals_host_transformed_items(tmp_path):
    pytest.importorskip("PIL")
    from maxsquareloss_amd.datasets import City_DataLoader
    from maxsquareloss_amd.tools import evaluate
    from maxsquareloss_amd.utils.validate import Validator
    paths, _ = write_tree(tmp_path, n=1, val_n=3, hw=SRC_HW)
    args, train_id, logger = evaluate.parse_args(_common(["--data_root_path", paths["data_root_path"], "--flip", "True"]))
    args.seg_size = (OW, OH)
    ev = evaluate.Evaluater(args, cuda=True, train_id=train_id, logger=logger)
    assert ev.valid_iterations == 3
    ev.validate()
    got = ev.Eval.confusion_matrix.copy()
    assert got.sum() > 0
    ld = City_DataLoader(args, training=False, datasets_path={"Cityscapes": paths})
    items = [ld.val_loader.dataset.host_transform(rgb, ids, plan) + (ident,)
             for rgb, ids, plan, ident, _ in ld.val_loader.host_items()]
    ld.close()
    assert len(items) == 3 and items[0][0].shape == (1, 3, OH, OW)
    ref = Validator(ev.model, args.num_classes, (OH, OW), 0, ev.device, flip=True, data=items)
    assert np.array_equal(ref.run().confusion_matrix, got)
    ev.dataloader.close()
