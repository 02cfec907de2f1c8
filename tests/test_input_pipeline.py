"""CPU tests of the file-backed input pipeline: the Pillow resampling tables (utils/resample.py)
against the reference loader's recorded outputs (tests/golden/input_pipeline_kat.npz, written by
scripts/gen_golden_input_pipeline.py from the reference's own transform code and real Pillow) and,
where Pillow is installed, against live Pillow; the datasets' file rules, draws and flags."""
import argparse
import importlib.util
import os
import random

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "input_pipeline_kat.npz")


def _gen():
    spec = importlib.util.spec_from_file_location("gen_golden_input_pipeline",
                                                  os.path.join(ROOT, "scripts", "gen_golden_input_pipeline.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fix():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def gen():
    return _gen()


def f32_of(fix, u8):
    """The fixture's fp32 (3, H, W) image of a recorded uint8 RGB output (its lossless encoding)."""
    t = fix["f32_of_byte"]
    return np.stack([t[c][u8[..., 2 - c]] for c in range(3)])


CASES = [(41, 67, 33, 20), (30, 50, 77, 45), (40, 60, 60, 17), (40, 60, 31, 40), (24, 36, 36, 24), (37, 1030, 515, 19)]


# ------------------------------------------------------------------------------------ tables
def test_fixture_has_the_issue_cases(fix):
    assert [tuple(int(v) for v in r) for r in fix["resize_cases"]] == CASES
    assert tuple(fix["crop_box"]) == (7, 5, 40, 30)
    assert os.path.getsize(GOLD) < 1 << 20


def test_bicubic_table_shape_and_ksize():
    from maxsquareloss_amd.utils import resample
    b, k, ks = resample.bicubic_table(41, 20)     # scale 2.05: support 4.1, ksize 11
    assert ks == 11 and b.shape == (20, 2) and k.shape == (20, 11) and b.dtype == k.dtype == np.int32
    b, k, ks = resample.bicubic_table(30, 45)     # upscale: filterscale 1, support 2, ksize 5
    assert ks == 5
    for n_in, n_out in ((1914, 1280), (1052, 720), (2048, 1024), (1024, 512)):
        b, k, ks = resample.bicubic_table(n_in, n_out)
        assert 7 <= ks <= 9 and b[:, 1].max() <= 8
        assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= n_in).all()
        for row, (_, n) in zip(k, b):
            assert not row[n:].any()
    # rows are used as they come: they need not sum to 2^22 and are never renormalised
    b, k, _ = resample.bicubic_table(1914, 1280)
    sums = k.sum(axis=1)
    assert (np.abs(sums - (1 << 22)) <= 8).all() and (sums != 1 << 22).any()


def test_nearest_table_keeps_the_incremental_sum():
    from maxsquareloss_amd.utils import resample
    for n_in, n_out in ((67, 33), (50, 77), (1030, 515), (1914, 1280), (1052, 720)):
        a = n_in / n_out
        xo, want = a * 0.5, []
        for _ in range(n_out):
            want.append(int(xo))
            xo += a
        assert resample.nearest_table(n_in, n_out).tolist() == want


@pytest.mark.parametrize("case", range(len(CASES)))
def test_numpy_two_pass_equals_the_reference_recording(fix, gen, case):
    from maxsquareloss_amd.utils import preprocess, resample
    h, w, ow, oh = CASES[case]
    ids = gen.kat_input(fix, f"c{case}_ids")
    assert ids.shape == (h, w)
    for m in (0, 1):
        for k in "us":
            rgb = gen.kat_input(fix, f"c{case}_{k}_rgb")
            got = resample.resize_bicubic(rgb, (ow, oh), mirror=bool(m))
            want = fix[f"c{case}_{k}_m{m}_u8"]
            assert got.shape == want.shape == (oh, ow, 3)
            assert np.array_equal(got, want), f"case {case} kind {k} mirror {m}: {(got != want).sum()} bytes differ"
            f32 = resample.bgr_minus_mean(got, fix["img_mean"])
            assert f32.tobytes() == f32_of(fix, want).tobytes()
        lab = resample.resize_nearest(ids, (ow, oh), mirror=bool(m))
        assert np.array_equal(lab, fix[f"c{case}_m{m}_ids"])
        for tag, (ds, c16) in {"city19": ("cityscapes", False), "city16": ("cityscapes", True), "gta19": ("gta5", False),
                               "gta16": ("gta5", True)}.items():
            if f"c{case}_m{m}_{tag}" in fix:
                assert np.array_equal(preprocess.build_lut(ds, class_16=c16)[lab], fix[f"c{case}_m{m}_{tag}"])
    if case == 0:
        assert fix["c0_s_m0_u8"].min() == 0 and fix["c0_s_m0_u8"].max() == 255  # the saturated kind hits both clamps


def test_crop_is_a_source_offset(fix, gen):
    from maxsquareloss_amd.utils import preprocess, resample
    box = tuple(int(v) for v in fix["crop_box"])
    ids = gen.kat_input(fix, "crop_ids")
    lut = preprocess.build_lut("cityscapes")
    for j, (ow, oh) in enumerate(fix["crop_sizes"]):
        for m in (0, 1):
            for k in "us":
                rgb = gen.kat_input(fix, f"crop_{k}_rgb")
                got = resample.resize_bicubic(rgb, (ow, oh), crop=box, mirror=bool(m))
                assert np.array_equal(got, fix[f"crop_{k}_o{j}_m{m}_u8"]), (j, m, k)
            lab = resample.resize_nearest(ids, (ow, oh), crop=box, mirror=bool(m))
            assert np.array_equal(lab, fix[f"crop_o{j}_m{m}_ids"])
            assert np.array_equal(lut[lab], fix[f"crop_o{j}_m{m}_city19"])
    with pytest.raises(ValueError):
        resample.resize_bicubic(gen.kat_input(fix, "crop_u_rgb"), (10, 10), crop=(60, 5, 40, 30))


def chain_args(fix, val=False, **kw):
    c = [int(v) for v in fix["chain_cfg"]]
    a = argparse.Namespace(base_size=(c[2], c[3]), crop_size=(c[0], c[1]), seg_size=(c[6], c[7]) if val else (c[4], c[5]),
                           random_mirror=True, random_crop=True, resize=True, DA=False, seed=0, split="train",
                           class_16=False, class_13=False, batch_size=1, data_loader_workers=0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def write_tree(root, n=3, hw=(60, 90), val_n=2, gta=False, seed=7):
    """A tiny dataset tree of PNGs; returns (paths dict, {list name: [(rgb, ids)]})."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    made = {}
    root = str(root)
    if gta:
        os.makedirs(os.path.join(root, "images"))
        os.makedirs(os.path.join(root, "labels"))
        num = 1
        for name, count in (("train", n), ("test", val_n)):
            made[name] = []
            with open(os.path.join(root, name + ".txt"), "w") as f:
                for _ in range(count):
                    rgb = rng.integers(0, 256, hw + (3,), dtype=np.uint8)
                    ids = rng.integers(0, 40, hw, dtype=np.uint8)
                    Image.fromarray(rgb).save(os.path.join(root, "images", f"{num:05d}.png"))
                    Image.fromarray(ids).save(os.path.join(root, "labels", f"{num:05d}.png"))
                    f.write(f"{num}\n")
                    made[name].append((rgb, ids))
                    num += 1
        return {"data_root_path": root, "list_path": root, "gt_path": os.path.join(root, "labels")}, made
    for name, count in (("train", n), ("val", val_n)):
        made[name] = []
        os.makedirs(os.path.join(root, "leftImg8bit", name, "aachen"))
        os.makedirs(os.path.join(root, "gtFine", name, "aachen"))
        with open(os.path.join(root, name + ".txt"), "w") as f:
            for i in range(count):
                rgb = rng.integers(0, 256, hw + (3,), dtype=np.uint8)
                ids = rng.integers(0, 40, hw, dtype=np.uint8)
                rel = f"/{name}/aachen/aachen_{i:06d}_000019_leftImg8bit.png"
                Image.fromarray(rgb).save(os.path.join(root, "leftImg8bit") + rel)
                Image.fromarray(ids).save(os.path.join(root, "gtFine") + rel.replace("leftImg8bit", "gtFine_labelIds"))
                f.write("leftImg8bit" + rel + "\n")
                made[name].append((rgb, ids))
    return {"data_root_path": root, "list_path": root, "gt_path": os.path.join(root, "gtFine")}, made


class _NoFiles:
    """A dataset object without files: the plan / host transform of City_Dataset on given arrays."""

    def __new__(cls, args, training=True):
        from maxsquareloss_amd.datasets import City_Dataset
        ds = City_Dataset.__new__(City_Dataset)
        ds.args, ds.split, ds.training = args, args.split, training
        ds._setup(args)
        ds.rsize = tuple(args.seg_size)
        from maxsquareloss_amd.utils import preprocess
        ds.lut = preprocess.build_lut("cityscapes")
        return ds


def test_chained_transforms_equal_the_reference(fix, gen):
    """mirror, crop, resize to base, resize to rsize (train) and resize, crop, resize to base (val): the
    dataset's own draws from random.Random(seed) are the reference's after random.seed(seed), and the
    plan run as exact resizes equals the reference's recorded output."""
    rgb, ids = gen.kat_input(fix, "crop_u_rgb"), gen.kat_input(fix, "crop_ids")
    for name, val in (("chain_train0", False), ("chain_train1", False), ("chain_val0", True)):
        ds = _NoFiles(chain_args(fix, val=val), training=not val)
        ds.rng = random.Random(int(fix[name + "_seed"]))
        mirror, steps = ds.plan(rgb.shape[1], rgb.shape[0])
        want = tuple(int(v) for v in fix[name + "_draw"])
        crop = next(c for _, c in steps if c is not None)
        assert (int(mirror), crop[0], crop[1]) == want
        assert len(steps) == 2 and (steps[0][1] is None) == val
        img, lab = ds.host_transform(rgb, ids, (mirror, steps))
        assert img.numpy()[0].tobytes() == f32_of(fix, fix[name + "_u8"]).tobytes(), name
        assert np.array_equal(lab.numpy()[0], fix[name + "_city19"].astype(np.int64)), name


# ------------------------------------------------------------------------------------ live Pillow
def test_tables_equal_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    from maxsquareloss_amd.utils import resample
    rng = np.random.default_rng(5)
    extra = [(100, 333, 7, 5), (13, 17, 200, 150), (60, 90, 45, 30)]
    for h, w, ow, oh in CASES + extra:
        for sat in (False, True):
            rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            if sat:
                rgb = ((rgb >> 7) * 255).astype(np.uint8)
            ids = rng.integers(0, 256, (h, w), dtype=np.uint8)
            for mirror in (False, True):
                im, lb = Image.fromarray(rgb), Image.fromarray(ids)
                if mirror:
                    im, lb = im.transpose(Image.FLIP_LEFT_RIGHT), lb.transpose(Image.FLIP_LEFT_RIGHT)
                assert np.array_equal(resample.resize_bicubic(rgb, (ow, oh), mirror=mirror),
                                      np.asarray(im.resize((ow, oh), Image.BICUBIC)))
                assert np.array_equal(resample.resize_nearest(ids, (ow, oh), mirror=mirror),
                                      np.asarray(lb.resize((ow, oh), Image.NEAREST)))
                if h >= 40 and w >= 50:
                    box = (7, 5, 40, 30)
                    pb = (7, 5, 47, 35)
                    assert np.array_equal(resample.resize_bicubic(rgb, (ow, oh), crop=box, mirror=mirror),
                                          np.asarray(im.crop(pb).resize((ow, oh), Image.BICUBIC)))
                    assert np.array_equal(resample.resize_nearest(ids, (ow, oh), crop=box, mirror=mirror),
                                          np.asarray(lb.crop(pb).resize((ow, oh), Image.NEAREST)))


def test_dataset_shape_tables_equal_live_pillow():
    """The two dataset shapes of the issue, one axis at a time (a full image per axis pair is slow in numpy)."""
    Image = pytest.importorskip("PIL.Image")
    from maxsquareloss_amd.utils import resample
    rng = np.random.default_rng(6)
    for (h, w), (ow, oh) in (((24, 1914), (1280, 24)), ((1052, 24), (24, 720)), ((16, 2048), (1024, 16)), ((1024, 16), (16, 512))):
        rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ids = rng.integers(0, 256, (h, w), dtype=np.uint8)
        assert np.array_equal(resample.resize_bicubic(rgb, (ow, oh)),
                              np.asarray(Image.fromarray(rgb).resize((ow, oh), Image.BICUBIC)))
        assert np.array_equal(resample.resize_nearest(ids, (ow, oh)),
                              np.asarray(Image.fromarray(ids).resize((ow, oh), Image.NEAREST)))


# ------------------------------------------------------------------------------------ datasets
def test_cityscapes_files_and_path_rule(tmp_path):
    pytest.importorskip("PIL")
    from maxsquareloss_amd.datasets import City_DataLoader, City_Dataset
    paths, made = write_tree(tmp_path, n=3, val_n=2)
    args = chain_args({"chain_cfg": [40, 30, 50, 36, 33, 20, 70, 44]})
    ds = City_Dataset(args, split="train", **paths)
    assert len(ds) == 3
    image_path, gt_path, ident = ds.paths(1)
    assert image_path.endswith("leftImg8bit/train/aachen/aachen_000001_000019_leftImg8bit.png")
    assert gt_path.endswith("gtFine/train/aachen/aachen_000001_000019_gtFine_labelIds.png") and ident == 1
    rgb, ids = ds.decode(1)
    assert np.array_equal(rgb, made["train"][1][0]) and np.array_equal(ids, made["train"][1][1])
    assert ds.rsize == (33, 20)
    args.DA = True
    assert City_Dataset(args, split="train", **paths).rsize == (50, 36)  # cityscapes_Dataset.py:111-114
    args.DA = False
    ld = City_DataLoader(args, training=True, datasets_path={"Cityscapes": paths})
    assert (ld.num_iterations, ld.valid_iterations) == (3, 2)
    assert len(ld.val_loader.dataset) == 2 and not ld.val_loader.dataset.is_train()
    assert ld.val_loader.order(0) == [0, 1] and sorted(ld.data_loader.order(0)) == [0, 1, 2]
    assert ld.data_loader.order(3) == ld.data_loader.order(3)
    ld.close()


def test_gta5_files_and_test_list(tmp_path):
    pytest.importorskip("PIL")
    from maxsquareloss_amd.datasets import GTA5_DataLoader, GTA5_Dataset
    paths, made = write_tree(tmp_path, n=2, val_n=1, gta=True)
    args = chain_args({"chain_cfg": [40, 30, 50, 36, 33, 20, 70, 44]})
    ds = GTA5_Dataset(args, split="train", **paths)
    assert ds.paths(1) == (os.path.join(paths["data_root_path"], "images", "00002.png"),
                           os.path.join(paths["gt_path"], "00002.png"), "2")
    assert ds.rsize == ds.base_size == (50, 36)  # the reference never sets rsize here: base_size
    val = GTA5_Dataset(args, split="val", training=False, **paths)  # gta5_Dataset.py:59-60: test.txt
    assert len(val) == 1 and val.paths(0)[2] == "3"
    assert np.array_equal(val.decode(0)[1], made["test"][0][1])
    ld = GTA5_DataLoader(args, training=True, datasets_path=paths)
    assert (ld.num_iterations, ld.valid_iterations) == (2, 1)
    ld.close()


def test_label_files_must_be_2d_uint8(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from maxsquareloss_amd.datasets import City_Dataset
    from maxsquareloss_amd.hip import MSLError
    paths, _ = write_tree(tmp_path, n=1, val_n=1)
    ds = City_Dataset(chain_args({"chain_cfg": [40, 30, 50, 36, 33, 20, 70, 44]}), split="train", **paths)
    gt = ds.paths(0)[1]
    Image.fromarray(np.zeros((60, 90), np.uint16) + 300).save(gt)  # a 16-bit label map, as SYNTHIA's
    with pytest.raises(MSLError, match="2-D uint8"):
        ds.decode(0)
    Image.fromarray(np.zeros((60, 90, 3), np.uint8)).save(gt)
    with pytest.raises(MSLError, match="2-D uint8"):
        ds.decode(0)
    with pytest.raises(MSLError, match="list file"):
        City_Dataset(ds.args, split="train", data_root_path=paths["data_root_path"], list_path=str(tmp_path / "nowhere"),
                     gt_path=paths["gt_path"])


@pytest.mark.parametrize("workers", [1, 3, 16])
def test_draws_do_not_depend_on_worker_count(tmp_path, workers):
    pytest.importorskip("PIL")
    from maxsquareloss_amd.datasets import City_DataLoader
    paths, made = write_tree(tmp_path, n=7, val_n=1)

    def epoch_plans(n_workers):
        args = chain_args({"chain_cfg": [40, 30, 50, 36, 33, 20, 70, 44]}, data_loader_workers=n_workers, seed=11)
        ld = City_DataLoader(args, training=True, datasets_path={"Cityscapes": paths})
        assert ld.data_loader.workers == min(n_workers, 16)
        got = []
        for _ in range(2):  # two epochs: two permutations
            for rgb, ids, plan, ident, _ in ld.data_loader.host_items():
                assert np.array_equal(rgb, made["train"][ident][0]) and np.array_equal(ids, made["train"][ident][1])
                got.append((ident, plan))
        ld.close()
        return got

    base = epoch_plans(0)
    assert sorted(i for i, _ in base[:7]) == list(range(7))
    assert [i for i, _ in base[:7]] != [i for i, _ in base[7:]]  # a new permutation per epoch
    assert len({p[0] for _, p in base}) == 2                      # both mirror values were drawn
    assert epoch_plans(workers) == base


def test_worker_count_is_capped():
    from maxsquareloss_amd.datasets import DeviceLoader
    ld = DeviceLoader([], shuffle=False, workers=64)
    assert ld.workers == 16
    ld.close()


def test_synthia_with_a_data_path_raises():
    from maxsquareloss_amd.datasets import build_loader
    from maxsquareloss_amd.hip import MSLError
    with pytest.raises(MSLError, match="FreeImage"):
        build_loader("synthia", argparse.Namespace(), True, {"data_root_path": "/x", "list_path": "/x", "gt_path": "/x"})


def test_flag_defaults_keep_the_synthetic_loaders():
    from maxsquareloss_amd.tools import evaluate, solve_gta5, train_source
    a = solve_gta5.build_parser().parse_args([])
    for k in ("data_root_path", "list_path", "gt_path", "source_data_path", "source_list_path", "source_gt_path",
              "target_data_path", "target_list_path", "target_gt_path"):
        assert getattr(a, k) is None, k
    assert a.data_loader_workers == 0
    assert evaluate.build_parser().parse_args([]).data_root_path is None
    # without a GPU the trainers cannot be built here; their loader choice is a method that needs none
    for cls in (train_source.Trainer, solve_gta5.UDATrainer):
        tr = cls.__new__(cls)
        args, _, _ = train_source.init_args(solve_gta5.build_parser().parse_args(["--crop_size", "64,32"]))
        tr.args, tr.rank = args, 0
        tr.build_dataloader()
        assert not tr.file_backed and type(tr.dataloader).__name__ == "SyntheticDomain"
        assert (tr.dataloader.h, tr.dataloader.w, len(tr.dataloader)) == (32, 64, args.synthetic_images)
    paths = train_source.dataset_paths("gta5", "/d/GTA5", None)
    assert paths == {"data_root_path": "/d/GTA5", "list_path": "/d/GTA5", "gt_path": "/d/GTA5/labels"}
    assert train_source.dataset_paths("Cityscapes", "/d/City", "/l")["gt_path"] == "/d/City/gtFine"


def test_uda_needs_both_roots():
    from maxsquareloss_amd.hip import MSLError
    from maxsquareloss_amd.tools import solve_gta5, train_source
    tr = solve_gta5.UDATrainer.__new__(solve_gta5.UDATrainer)
    args, _, _ = train_source.init_args(solve_gta5.build_parser().parse_args(["--source_data_path", "/nowhere"]))
    tr.args, tr.rank = args, 0
    with pytest.raises(MSLError, match="both"):
        tr.build_dataloader()
    args, _, _ = train_source.init_args(solve_gta5.build_parser().parse_args(
        ["--source_data_path", "/nowhere", "--target_data_path", "/nowhere", "--source_dataset", "synthia"]))
    tr.args = args
    with pytest.raises(MSLError, match="FreeImage"):
        tr.build_dataloader()
