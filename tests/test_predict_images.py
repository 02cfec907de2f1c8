"""CPU tests of the prediction images: the two new C entry points' declarations, the reference names of
datasets/cityscapes_Dataset.py against data recorded from the reference's own functions
(tests/golden/predict_images_kat.npz, scripts/gen_golden_predict_images.py), the host tables, the restatement the
GPU tests compare against (tests/predict_images_ref.py), the new flags, Client_dataset's list and the PNG writer."""
import argparse
import os
import re
import threading

import numpy as np
import pytest
import torch

import predict_images_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- C-ABI
@pytest.mark.parametrize("name,nargs", [("msl_predict_images", 19), ("msl_colorize", 7)])
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
        return {"int": hip.c_int, "float": hip.c_f, "long long": hip.c_ll}[p.rsplit(" ", 1)[0].replace("const ", "")]

    assert [ctype(p) for p in params] == args
    assert hasattr(hip.load(require_gpu=False), name)
    from maxsquareloss_amd import ops
    assert callable(ops.predict_images) and callable(ops.colorize)


def test_image_kernels_use_no_scratch():
    """The compiler's resource report of the last build (Makefile: predict.o.remarks): no instantiation of the
    prediction kernels spills or uses scratch, and the shared per-pixel decision left k_predict_up without any."""
    path = os.path.join(ROOT, "maxsquareloss_amd", "_lib", "obj", "predict.o.remarks")
    if not os.path.exists(path):
        pytest.skip("no resource report: build the library first (__graft_entry__.build())")
    kern, info = None, {}
    for line in open(path):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            kern = m.group(1)
            info[kern] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs Spill): (\d+)", line)
        if m and kern:
            info[kern][m.group(1)] = int(m.group(2))
    for stem, count in (("k_predict_images", 8), ("k_predict_up", 8), ("k_colorize", 2)):  # {flip} x {19, 16, 13, 32}
        ks = [k for k in info if stem in k]
        assert len(ks) == count, (stem, ks)
        for k in ks:
            assert info[k]["ScratchSize [bytes/lane]"] == 0 and info[k]["VGPRs Spill"] == 0, (k, info[k])


# ----------------------------------------------------------------------------- the reference's names
def test_reference_names_equal_the_golden():
    from maxsquareloss_amd.datasets import cityscapes_Dataset as cd
    g = ref.gold()
    assert np.array_equal(np.array(cd.label_colours, np.uint8), g["label_colours"])
    assert all(isinstance(c, tuple) for c in cd.label_colours) and len(cd.label_colours) == 20
    assert cd.NUM_CLASSES == 19 and list(g["name_classes"]) == cd.name_classes
    assert cd.IMG_MEAN.dtype == np.float32 and np.array_equal(cd.IMG_MEAN, g["img_mean"])


def _f(u8):
    return torch.from_numpy(u8.astype("float32")).div_(255.0)


def _rgb(out, y, x):
    return torch.round(out[0, :, y, x] * 255).int().tolist()


def test_decode_labels_on_cpu_equals_the_golden():
    from maxsquareloss_amd.datasets.cityscapes_Dataset import decode_labels
    g = ref.gold()
    ma, mb = g["mask_a"], g["mask_b"]
    assert ma.min() == -1 and max(ma.max(), mb.max()) == 20
    for mask, n, key in ((torch.from_numpy(ma), 2, "decode_a"), (mb, 1, "decode_b"), (ma, 1, "decode_a_n1"),
                         (torch.from_numpy(mb), 5, "decode_b_n5"), (torch.from_numpy(ma).int(), 2, "decode_a")):
        out = decode_labels(mask, n)
        assert out.dtype == torch.float32 and tuple(out.shape) == g[key].shape
        assert torch.equal(out, _f(g[key])), key
    assert decode_labels(ma).shape == (1, 3, 7, 9)  # num_images defaults to 1
    assert g["decode_a_n1"].shape[0] == 1 and g["decode_b_n5"].shape[0] == 1  # n < num_images: n images
    # fewer classes: class indices from num_classes on are black too
    out = decode_labels(np.array([[[0, 4, 5, 18]]]), 1, 5)
    assert torch.equal(out[0, :, 0, 2:], torch.zeros(3, 2)) and _rgb(out, 0, 1) == [190, 153, 153]


def test_decode_labels_maps_16_and_13_classes_through_the_trainid():
    """The documented deviation: class 9 of a 16-class model is sky (trainId 10), and is painted sky."""
    from maxsquareloss_amd.datasets.cityscapes_Dataset import decode_labels, label_colours
    out = decode_labels(np.array([[[9, 15, 16]]]), 1, 16)
    assert _rgb(out, 0, 0) == list(label_colours[10])
    assert _rgb(out, 0, 1) == list(label_colours[18]) and out[0, :, 0, 2].sum() == 0
    out = decode_labels(np.array([[[3, 12]]]), 1, 13)
    assert _rgb(out, 0, 0) == list(label_colours[6])
    assert _rgb(out, 0, 1) == list(label_colours[18])


@pytest.mark.parametrize("numpy_transform", [False, True])
def test_inv_preprocess_on_cpu_equals_the_golden(numpy_transform):
    from maxsquareloss_amd.datasets.cityscapes_Dataset import inv_preprocess
    g = ref.gold()
    want = g[f"inv_np{int(numpy_transform)}"]
    for imgs in (torch.from_numpy(g["img"].copy()), g["img"].copy()):
        out = inv_preprocess(imgs, 2, numpy_transform=numpy_transform)
        assert torch.is_tensor(out) and out.shape == want.shape
        assert np.abs(out.numpy() - want).max() <= 1e-6
        assert out.min() == 0 and 0.999 < out.max() < 1
    assert not np.array_equal(g["inv_np0"], g["inv_np1"])
    assert np.array_equal(g["inv_np0"][:, ::-1], g["inv_np1"])  # the channel flip and nothing else


# ----------------------------------------------------------------------------- host tables
@pytest.mark.parametrize("C", [19, 16, 13])
def test_shade_and_palette_tables(C):
    from maxsquareloss_amd.utils import palette
    pal, shade = palette.palette_table(C), palette.shade_table(C)
    assert pal.shape == (C, 3) and shade.shape == (4, C, 3) and pal.dtype == shade.dtype == np.uint8
    tid = palette.trainids_of(C)
    for b, r in enumerate((1.0, 0.8, 0.6, 0.3)):
        for k in range(C):
            assert pal[k].tolist() == list(palette.label_colours[tid[k]])
            assert shade[b, k].tolist() == [int(r * x) for x in palette.label_colours[tid[k]]], (b, k)
    assert np.array_equal(shade[0], pal)
    # the five shades of a class (black included) are distinct: a confidence pixel decodes to one bucket
    for k in range(C):
        assert len({tuple(shade[b, k]) for b in range(4)} | {(0, 0, 0)}) == 5
    assert palette.SPLITS == ref.SPLITS


def test_id_table_maps_to_cityscapes_label_ids():
    from maxsquareloss_amd.utils import palette
    from maxsquareloss_amd.utils.preprocess import CITYSCAPES_ID_TO_TRAINID
    t19, t16, t13 = (palette.id_table(c) for c in (19, 16, 13))
    assert t19.tolist() == [7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33]
    assert (t19[0], t16[0], t13[0]) == (7, 7, 7) and t19[18] == 33 and t16[9] == 23 and t13[3] == 19
    for t, C in ((t19, 19), (t16, 16), (t13, 13)):
        assert t.dtype == np.uint8 and len(t) == C
        assert [CITYSCAPES_ID_TO_TRAINID[int(i)] for i in t] == palette.trainids_of(C)  # the inverse table
    with pytest.raises(ValueError):
        palette.id_table(21)


# ----------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("shape", ref.SHAPES[:4])
@pytest.mark.parametrize("flip", [False, True])
def test_restatement_fills_every_bucket_with_a_small_edge_mask(shape, flip):
    r = ref.reference(shape, flip)
    npx = shape[3] * shape[4]
    counts = np.bincount(r["bucket"], minlength=5)
    print(f"{shape} flip={flip}: buckets {counts.tolist()}, kept {int(r['keep'].sum())}, near-edge "
          f"{int(r['near_edge'].sum())} of {npx}")
    assert (counts > 0).all(), counts
    assert 0 < r["keep"].sum() < npx
    assert r["near_edge"].sum() <= max(2, npx // 1000)
    assert (r["bucket"][r["keep"]] == 0).all()  # 0.95 lies in the top bucket


# ----------------------------------------------------------------------------- flags and tools
def test_new_flags_default_off():
    from maxsquareloss_amd.tools import evaluate, predict, solve_gta5
    from maxsquareloss_amd.tools.train_source import add_train_args
    a = evaluate.build_parser().parse_args([])
    assert a.save_predictions is None and a.save_kinds == ("color",) and a.image_summary is False
    assert a.threshold == solve_gta5.build_parser().parse_args([]).threshold == 0.95
    assert evaluate.output_request(a) is None
    assert add_train_args(argparse.ArgumentParser()).parse_args([]).val_save_predictions is None
    assert solve_gta5.build_parser().parse_args([]).val_save_predictions is None
    p = predict.build_parser().parse_args([])
    assert (p.out_size, p.save_predictions, p.flip, p.graph, p.list_path) == (None, None, False, False, None)
    a = evaluate.build_parser().parse_args(["--save_predictions", "d", "--save_kinds", "pseudo,color,pseudo",
                                            "--threshold", "0.9", "--data_loader_workers", "40"])
    req = evaluate.output_request(a)
    assert (req.directory, req.kinds, req.threshold, req.maps) == ("d", ("pseudo", "color"), 0.9, ("pseudo", "color"))
    assert all(req.selects(i, 50) for i in range(50))
    a = evaluate.build_parser().parse_args(["--image_summary", "True", "--save_dir", "log"])
    req = evaluate.output_request(a)
    assert req.directory == os.path.join("log", "images") and req.kinds == ("color",)
    assert [i for i in range(50) if req.selects(i, 50)] == [0, 20, 40, 49]  # every 20th item and the last


def test_save_kinds_rejects_unknown_kinds(capsys):
    from maxsquareloss_amd.tools import evaluate, predict
    from maxsquareloss_amd.utils.images import SAVE_KINDS, parse_save_kinds
    assert SAVE_KINDS == ("color", "trainids", "labelids", "confidence", "pseudo", "input")
    assert parse_save_kinds("color, input") == ("color", "input")
    for parser in (evaluate.build_parser(), predict.build_parser()):
        with pytest.raises(SystemExit):
            parser.parse_args(["--save_kinds", "color,heatmap"])
        assert "heatmap" in capsys.readouterr().err
    with pytest.raises(argparse.ArgumentTypeError):
        parse_save_kinds("")
    with pytest.raises(SystemExit):
        predict.build_parser().parse_args(["--out_size", "2048"])
    assert predict.build_parser().parse_args(["--out_size", "2048,1024"]).out_size == (2048, 1024)


def test_out_size_needs_unlabelled_data():
    from maxsquareloss_amd.hip import MSLError
    from maxsquareloss_amd.tools import evaluate
    from maxsquareloss_amd.utils.images import OutputRequest
    from maxsquareloss_amd.utils.validate import Validator
    assert not any("--out_size" in a.option_strings for a in evaluate.build_parser()._actions)
    req = OutputRequest("d", ("color",), out_size=(64, 32))
    with pytest.raises(MSLError, match="out_size"):
        Validator(None, 19, (33, 65), 1, torch.device("cpu"), data=[], outputs=req)
    v = Validator(None, 19, (33, 65), 1, torch.device("cpu"), data=[], outputs=req, labelled=False)
    assert v.outputs is req and v.valid_iterations == 0
    with pytest.raises(MSLError):  # unlabelled and nothing to write
        Validator(None, 19, (33, 65), 1, torch.device("cpu"), data=[], labelled=False)


# ----------------------------------------------------------------------------- Client_dataset
def test_client_dataset_lists_and_names(tmp_path):
    from maxsquareloss_amd.datasets import Client_dataset
    from maxsquareloss_amd.hip import MSLError
    Image = pytest.importorskip("PIL.Image")
    lists, imgs = tmp_path / "lists", tmp_path / "imgs" / "city"
    lists.mkdir()
    imgs.mkdir(parents=True)
    rng = np.random.default_rng(5)
    paths = []
    for k, (h, w) in enumerate(((6, 9), (5, 7))):
        arr = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        paths.append(str(imgs / f"city_{k:02d}_leftImg8bit.png"))
        Image.fromarray(arr).save(paths[-1])
    (lists / "test.txt").write_text("\n".join(paths) + "\n\n")
    args = argparse.Namespace(resize=True, seg_size=(8, 4), numpy_transform=True)
    ds = Client_dataset({"list_path": str(lists)}, args)
    assert len(ds) == 2 and ds.items == paths
    assert [ds.paths(i)[2] for i in range(2)] == ["city_00_leftImg8bit", "city_01_leftImg8bit"]
    rgb, ids = ds.decode(1)
    assert ids is None and rgb.shape == (5, 7, 3) and rgb.dtype == np.uint8
    assert np.array_equal(rgb, np.asarray(Image.open(paths[1]).convert("RGB")))
    assert ds.plan(7, 5) == (False, [((8, 4), None)])
    args.resize = False
    assert Client_dataset({"list_path": str(lists)}, args).plan(7, 5) == (False, [((7, 5), None)])
    with pytest.raises(MSLError, match="test.txt"):
        Client_dataset({"list_path": str(tmp_path / "imgs")}, args)


# ----------------------------------------------------------------------------- the writer
def test_writer_layout_round_trip_and_thread_bound(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from maxsquareloss_amd.hip import MSLError
    from maxsquareloss_amd.utils.images import MAX_WRITER_THREADS, SAVE_KINDS, ImageWriter
    rng = np.random.default_rng(11)
    rgb_kinds = ("color", "confidence", "input")

    def maps(h, w):
        return {k: rng.integers(0, 256, size=(h, w, 3) if k in rgb_kinds else (h, w), dtype=np.uint8)
                for k in SAVE_KINDS}

    before = threading.active_count()
    for workers in (0, 3, 40):
        d = tmp_path / f"w{workers}"
        sent = {}
        with ImageWriter(str(d), SAVE_KINDS, workers) as wr:
            assert wr.workers == min(workers, 16) <= MAX_WRITER_THREADS == 16 and len(wr._slots) >= 2
            for i in range(7):  # more saves than slots: a slot is reused only after its encode finished
                name = f"item_{i}"
                sent[name] = maps(5 + i, 8)
                wr.save(name, {k: (torch.from_numpy(v) if i % 2 else v) for k, v in sent[name].items()})
            assert threading.active_count() - before <= 16
        assert sorted(os.listdir(d)) == sorted(SAVE_KINDS)
        for name, m in sent.items():
            for k, arr in m.items():
                with Image.open(d / k / f"{name}.png") as im:
                    assert im.mode == ("RGB" if k in rgb_kinds else "L")
                    assert np.array_equal(np.asarray(im), arr), (workers, name, k)
        assert all(len(os.listdir(d / k)) == 7 for k in SAVE_KINDS)
    assert threading.active_count() == before  # close() joined the pool
    with ImageWriter(str(tmp_path / "one"), ("color",)) as wr:
        assert os.listdir(tmp_path / "one") == ["color"]
        with pytest.raises(MSLError):
            wr.save("x", {"pseudo": np.zeros((2, 2), np.uint8)})
