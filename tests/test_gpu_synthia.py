"""The device PNG unfilter (csrc/png.hip) byte for byte against the scalar restatement of the PNG
specification (png_ref.py), and file-backed SYNTHIA end to end on the GPU."""
import argparse

import numpy as np
import pytest
import torch

import png_ref

pytestmark = pytest.mark.gpu

GUARD = 0xA5
TIES = np.array([0, 1, 2, 254, 255], np.uint8)  # Paeth ties and their a, b, c order, mod-256 wrap, the 9-bit Average sum


def _lib():
    from maxsquareloss_amd import hip
    return hip, hip.load()


def band_rows():
    return _lib()[1].msl_png_unfilter_band_rows()


def run(scan, h, w, bpp, lane, stride=None, status=0):
    """msl_png_unfilter_lane on `scan` (numpy uint8, any shape holding the rows at `stride`) into rows
    1..h of an (h + 2, w) buffer of guard bytes; checks the status and the guard rows, returns (h, w)."""
    hip, lib = _lib()
    d_scan = torch.from_numpy(np.ascontiguousarray(scan)).cuda()
    stride = scan.shape[1] if stride is None else stride
    out = torch.full((h + 2, w), GUARD, dtype=torch.uint8, device="cuda")
    got = lib.msl_png_unfilter_lane(d_scan.data_ptr(), h, w, bpp, lane, stride, out[1].data_ptr(), hip.stream_ptr())
    assert got == status, (got, status)
    res = out.cpu().numpy()
    assert (res[0] == GUARD).all() and (res[-1] == GUARD).all(), "a guard row was written"
    return res[1:-1]


def raw_bytes(rng, kind, h, n):
    return rng.integers(0, 256, (h, n), dtype=np.uint8) if kind == "uniform" else TIES[rng.integers(0, 5, (h, n))]


def filter_sets(rng, h):
    return [[k] * h for k in range(5)] + [[r % 5 for r in range(h)], list(rng.integers(0, 5, h))]


def _shapes():
    heights = ["1", "2", "63", "64", "65", "129", "B-1", "B", "B+1", "2*B+1"]
    widths = [1, 2, 3, 63, 64, 65, 257]
    out = [(hh, w) for hh in heights for w in widths if not ("B" in hh and w > 65)]
    return out + [("1", 2000), ("2*B+1", 1)]


@pytest.mark.parametrize("hh,w", _shapes())
def test_unfilter_equals_the_scalar_oracle(hh, w):
    """A partial wave, the hand-over between waves and between bands, a row shorter than any skew and a width
    past any hand-over block; each filter type alone (long chains, row 0 and column 0 with their zero
    neighbours), cycling and random per row; uniform bytes and the tie / wrap set."""
    B = band_rows()
    h = eval(hh, {"B": B})
    rng = np.random.default_rng(h * 1000 + w)
    for kind in ("uniform", "ties"):
        raw = raw_bytes(rng, kind, h, w)
        for filters in filter_sets(rng, h):
            scan = png_ref.filter_rows(raw, 1, filters)
            want = png_ref.scalar_unfilter(scan, 1)
            assert np.array_equal(want, raw)
            got = run(scan, h, w, 1, 0)
            assert np.array_equal(got, want), (h, w, kind, filters[:5], np.argwhere(got != want)[:4])


def test_arbitrary_streams():
    """The unfilter is defined on any byte stream, not only on what an encoder writes."""
    rng = np.random.default_rng(77)
    for h, w in ((70, 130), (130, 67)):
        scan = rng.integers(0, 256, (h, 1 + w), dtype=np.uint8)
        scan[:, 0] = rng.integers(0, 5, h)
        assert np.array_equal(run(scan, h, w, 1, 0), png_ref.scalar_unfilter(scan, 1))


@pytest.mark.parametrize("bpp,lane", [(1, 0), (2, 0), (2, 1), (3, 2), (4, 3), (6, 1), (8, 7)])
def test_lanes_of_the_raw_stream(bpp, lane):
    from maxsquareloss_amd.utils import png
    rng = np.random.default_rng(bpp * 8 + lane)
    h, w = 67, 70
    for kind in ("uniform", "ties"):
        raw = raw_bytes(rng, kind, h, w * bpp)
        scan = png_ref.filter_rows(raw, bpp, rng.integers(0, 5, h))
        want = png_ref.scalar_lane(scan, bpp, lane)
        assert np.array_equal(want, raw[:, lane::bpp])
        assert np.array_equal(run(scan, h, w, bpp, lane), want)
        wide = np.full((h, 1 + w * bpp + 13), 0x5A, np.uint8)      # a row stride above 1 + w * bpp
        wide[:, :1 + w * bpp] = scan
        assert np.array_equal(run(wide, h, w, bpp, lane), want)
        if (bpp, lane) == (6, 1):
            assert np.array_equal(run(png.lane_plane(scan, 6, 1), h, w, 1, 0), want)


def test_a_filter_byte_above_4_is_none():
    """Defined behaviour of the C ABI (the host reader refuses such a file before any upload): the row is
    taken as None and the rows below follow from it."""
    rng = np.random.default_rng(4)
    h, w = 70, 66
    scan = png_ref.filter_rows(raw_bytes(rng, "uniform", h, w), 1, rng.integers(1, 5, h))
    scan[33, 0] = 7
    as_none = scan.copy()
    as_none[33, 0] = 0
    want = png_ref.scalar_unfilter(as_none, 1)
    got = run(scan, h, w, 1, 0)
    assert np.array_equal(got[33], scan[33, 1:]) and np.array_equal(got, want)


def test_bad_arguments_return_their_status_without_launching():
    hip, lib = _lib()
    scan = torch.zeros((4, 1 + 8 * 2), dtype=torch.uint8, device="cuda")
    out = torch.full((4, 8), GUARD, dtype=torch.uint8, device="cuda")
    s, o, st = scan.data_ptr(), out.data_ptr(), hip.stream_ptr()
    good = dict(scan=s, h=4, w=8, bpp=2, lane=1, stride=17, out=o)
    bad = [dict(scan=None), dict(out=None), dict(h=0), dict(w=0), dict(h=-1), dict(h=65536), dict(w=65536),
           dict(bpp=0), dict(bpp=9), dict(lane=2), dict(lane=-1), dict(stride=16), dict(stride=0)]
    for change in bad:
        a = dict(good, **change)
        got = lib.msl_png_unfilter_lane(a["scan"], a["h"], a["w"], a["bpp"], a["lane"], a["stride"], a["out"], st)
        assert got == -3, (change, got)
    torch.cuda.synchronize()
    assert (out == GUARD).all()
    a = good
    assert lib.msl_png_unfilter_lane(a["scan"], a["h"], a["w"], a["bpp"], a["lane"], a["stride"], a["out"], st) == 0
    torch.cuda.synchronize()
    assert not out.any()


def test_two_calls_back_to_back_on_one_stream():
    from maxsquareloss_amd.utils import preprocess
    rng = np.random.default_rng(9)
    B = band_rows()
    cases = []
    for h, w in ((B + 3, 40), (70, 300)):
        scan = png_ref.filter_rows(raw_bytes(rng, "uniform", h, w), 1, rng.integers(0, 5, h))
        cases.append((torch.from_numpy(scan).cuda(), png_ref.scalar_unfilter(scan, 1)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        outs = [preprocess.png_unfilter(d) for d, _ in cases]
    side.synchronize()
    for got, (_, want) in zip(outs, cases):
        assert got.dtype == torch.uint8 and got.is_cuda and np.array_equal(got.cpu().numpy(), want)


def test_python_entry_takes_strided_rows_and_refuses_the_rest():
    from maxsquareloss_amd.hip import MSLError
    from maxsquareloss_amd.utils import preprocess
    rng = np.random.default_rng(10)
    h, w = 66, 35
    raw = raw_bytes(rng, "uniform", h, w * 6)
    scan = png_ref.filter_rows(raw, 6, rng.integers(0, 5, h))
    wide = torch.zeros((h, 1 + w * 6 + 5), dtype=torch.uint8, device="cuda")
    wide[:, :1 + w * 6] = torch.from_numpy(scan).cuda()
    got = preprocess.png_unfilter(wide[:, :1 + w * 6], bpp=6, lane=1)      # a view: row stride above its width
    assert np.array_equal(got.cpu().numpy(), raw[:, 1::6])
    for bad, kw in ((torch.from_numpy(scan), {}), (wide[:, :1 + w * 6], dict(bpp=4)), (wide[0], {}),
                    (wide[:, :1 + w * 6].int(), {})):
        with pytest.raises(MSLError, match="png_unfilter"):
            preprocess.png_unfilter(bad, **kw)
    with pytest.raises(MSLError, match="msl_png_unfilter_lane failed"):
        preprocess.png_unfilter(wide[:, :1 + w * 6], bpp=6, lane=6)


# ------------------------------------------------------------------------------------ the tiny tree end to end
def _args(**kw):
    a = argparse.Namespace(base_size=(30, 20), crop_size=(24, 16), seg_size=(30, 20), random_mirror=True,
                           random_crop=True, resize=True, DA=False, seed=3, split="train", class_16=False,
                           class_13=False, batch_size=1, data_loader_workers=0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    pytest.importorskip("PIL")
    return png_ref.synthia_tree(tmp_path_factory.mktemp("synthia") / "S")


@pytest.mark.parametrize("class_16", [False, True])
@pytest.mark.parametrize("workers", [0, 3])
def test_loader_items_equal_the_host_transform(tree, class_16, workers):
    from maxsquareloss_amd.datasets import SYNTHIA_DataLoader
    paths, made = tree
    args = _args(class_16=class_16, data_loader_workers=workers)
    ld, ref = (SYNTHIA_DataLoader(args, training=True, datasets_path=paths) for _ in range(2))
    for which in ("data_loader", "val_loader"):                 # the train and the val transform
        want = [getattr(ref, which).dataset.host_transform(rgb, plane, plan) + (ident,)
                for rgb, plane, plan, ident, _ in getattr(ref, which).host_items()]
        got = list(getattr(ld, which))
        assert len(got) == len(want) == len(made["train" if which == "data_loader" else "val"])
        for (img, lab, ident), (wimg, wlab, wident) in zip(got, want):
            assert img.is_cuda and img.dtype == torch.float32 and lab.dtype == torch.int64 and ident == wident
            assert torch.equal(img.cpu(), wimg) and torch.equal(lab.cpu(), wlab), (which, ident)
        assert any((lab >= 0).any() for _, lab, _ in got)
    ds = ld.data_loader.dataset                                  # and one item by index
    img, lab, ident = ds[1]
    assert ident == 1 and img.shape == (1, 3, 20, 30) and lab.shape == (1, 20, 30)
    ld.close()
    ref.close()


# the sizes of the tiny-tree trainer tests (test_gpu_input_pipeline.py)
OW, OH, CROP, SRC_HW = 256, 128, "120,72", (96, 160)


def test_uda_trainer_on_synthia_files(tmp_path):
    pytest.importorskip("PIL")
    from test_input_pipeline import write_tree
    from maxsquareloss_amd.datasets import SYNTHIA_DataLoader
    from maxsquareloss_amd.tools.solve_gta5 import UDATrainer, build_parser
    from maxsquareloss_amd.tools.train_source import init_args
    spaths, _ = png_ref.synthia_tree(tmp_path / "S", n=3, val_n=1, hw=SRC_HW, seed=3)
    tpaths, _ = write_tree(tmp_path / "city", n=2, val_n=1, hw=SRC_HW, seed=4)
    argv = ["--imagenet_pretrained", "False", "--save_dir", "", "--random_crop", "True", "--resize", "True",
            "--base_size", f"{OW},{OH}", "--crop_size", CROP, "--target_base_size", f"{OW},{OH}",
            "--target_crop_size", CROP, "--iter_max", "200000", "--seed", "21",
            "--source_dataset", "synthia", "--num_classes", "16", "--source_data_path", spaths["data_root_path"],
            "--source_list_path", spaths["list_path"], "--target_data_path", tpaths["data_root_path"],
            "--data_loader_workers", "2", "--round_num", "1", "--epoch_each_round", "1"]

    def one_run():
        args, _, _ = init_args(build_parser().parse_args(argv))
        args.seg_size = (OW, OH)
        torch.manual_seed(5)
        tr = UDATrainer(args, cuda=True)
        assert tr.file_backed and isinstance(tr.source_loader, SYNTHIA_DataLoader) and len(tr.source_dataloader) == 3
        assert tr.source_dataloader.dataset.class_16 and tr.dataloader.num_iterations == 2
        seen, step = [], tr.uda_step

        def spy(x_s, y_s, x_t):
            step(x_s, y_s, x_t)
            seen.append((y_s.clone(), tr.loss_val.detach().clone(), tr.loss_target.detach().clone()))

        tr.uda_step = spy
        tr.optimizer.zero_grad()
        tr.train_one_epoch()
        torch.cuda.synchronize()
        assert tr.current_iter == 2 and len(seen) == 2
        params = [p.detach().clone() for p in tr.model.parameters()]
        tr.dataloader.close()
        tr.source_loader.close()
        return seen, params

    first, p1 = one_run()
    second, p2 = one_run()
    for (y1, a1, b1), (y2, a2, b2) in zip(first, second):
        assert torch.isfinite(a1).all() and torch.isfinite(b1).all()
        assert y1.shape == (1, OH, OW) and int(y1.max()) <= 15 and (y1 >= 0).any()
        assert torch.equal(y1, y2) and torch.equal(a1, a2) and torch.equal(b1, b2)
    assert all(torch.equal(a, b) for a, b in zip(p1, p2))
