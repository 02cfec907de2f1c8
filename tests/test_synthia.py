"""File-backed SYNTHIA without a GPU: the PNG scanline reader and its numpy unfilter against the scalar
restatement of the specification (png_ref.py) and against Pillow, the refusals, the dataset over a tiny
tree, and the C ABI of the device unfilter."""
import argparse
import io
import os
import re
import struct
import zlib

import numpy as np
import pytest

import png_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _png():
    from maxsquareloss_amd.utils import png
    return png


def _samples(rng, h, w, depth, colour):
    return rng.integers(0, 1 << depth, (h, w, png_ref.CHANNELS[colour]), dtype=np.uint16 if depth == 16 else np.uint8)


# ------------------------------------------------------------------------------------ reader + unfilter
@pytest.mark.parametrize("depth", [8, 16])
@pytest.mark.parametrize("colour", [0, 2, 4, 6])
@pytest.mark.parametrize("mode", ["cycle", "random"])
def test_reader_and_unfilter_equal_the_scalar_oracle(depth, colour, mode):
    png = _png()
    rng = np.random.default_rng(depth * 10 + colour + (mode == "random"))
    h, w = 29, 41
    samples = _samples(rng, h, w, depth, colour)
    filters = [r % 5 for r in range(h)] if mode == "cycle" else rng.integers(0, 5, h)
    data, scan = png_ref.png_bytes(samples, depth, colour, filters)
    info, got = png.read_scanlines(data)
    bpp = png_ref.CHANNELS[colour] * depth // 8
    assert (info.width, info.height, info.depth, info.colour, info.bpp) == (w, h, depth, colour, bpp)
    assert got.dtype == np.uint8 and got.shape == (h, 1 + w * bpp) and np.array_equal(got, scan)
    want = png_ref.scalar_unfilter(got, bpp)
    raw = (samples.astype(">u2") if depth == 16 else samples).tobytes()
    assert want.tobytes() == raw                                  # writer and oracle agree with each other
    for lane in range(bpp):
        plane = png.lane_plane(got, bpp, lane)
        assert plane.shape == (h, 1 + w) and plane.flags["C_CONTIGUOUS"]
        assert np.array_equal(png.unfilter_lane(plane), want[:, lane::bpp]), lane


def test_split_idat_and_ancillary_chunks(tmp_path):
    png = _png()
    rng = np.random.default_rng(3)
    samples = _samples(rng, 31, 45, 16, 2)
    extra = [png_ref.chunk(b"tEXt", b"Comment\0hello"), png_ref.chunk(b"pHYs", struct.pack(">IIB", 1, 1, 0))]
    data, scan = png_ref.png_bytes(samples, 16, 2, rng.integers(0, 5, 31), idat_chunks=4, extra=extra)
    assert data.count(b"IDAT") >= 3
    path = tmp_path / "split.png"
    path.write_bytes(data)
    info, got = png.read_scanlines(str(path))
    assert np.array_equal(got, scan) and info.bpp == 6
    one, _ = png_ref.png_bytes(samples, 16, 2, scan[:, 0], idat_chunks=1)
    assert np.array_equal(png.read_scanlines(one)[1], got)


def test_unfilter_lane_edge_shapes_and_tie_data():
    png = _png()
    rng = np.random.default_rng(11)
    for h, w in ((1, 1), (1, 9), (9, 1), (2, 2), (5, 64)):
        for vals in (None, np.array([0, 1, 2, 254, 255], np.uint8)):
            raw = rng.integers(0, 256, (h, w), dtype=np.uint8) if vals is None else vals[rng.integers(0, 5, (h, w))]
            for filters in ([k] * h for k in range(5)):
                scan = png_ref.filter_rows(raw, 1, filters)
                assert np.array_equal(png.unfilter_lane(scan), raw), (h, w, filters[0])
            # arbitrary filtered bytes too: the unfilter is defined on any stream, not just on encoder output
            scan = np.concatenate([rng.integers(0, 5, (h, 1)), raw.astype(np.int64)], axis=1).astype(np.uint8)
            assert np.array_equal(png.unfilter_lane(scan), png_ref.scalar_unfilter(scan, 1))


def test_unfilter_lane_is_usable_at_synthia_size():
    png = _png()
    rng = np.random.default_rng(0)
    raw = rng.integers(0, 23, (760, 1280), dtype=np.uint8)
    scan = png_ref.filter_rows(raw, 1, rng.integers(0, 5, 760))
    assert np.array_equal(png.unfilter_lane(scan), raw)


# ------------------------------------------------------------------------------------ against Pillow
@pytest.mark.parametrize("mode", ["L", "RGB", "RGBA", "I;16"])
def test_files_pillow_wrote_decode_as_pillow_reads_them(mode):
    Image = pytest.importorskip("PIL.Image")
    png = _png()
    rng = np.random.default_rng(5)
    h, w = 33, 47
    # smooth content, so that Pillow's adaptive encoder uses more than one filter type
    base = (np.add.outer(np.arange(h) * 3, np.arange(w) * 2) + rng.integers(0, 4, (h, w)))
    if mode == "I;16":
        arr = (base * 97 % 65536).astype(np.uint16)
    else:
        ch = {"L": 1, "RGB": 3, "RGBA": 4}[mode]
        arr = np.stack([(base * (k + 1) + 7 * k) % 256 for k in range(ch)], axis=-1).astype(np.uint8)
        arr = arr[..., 0] if ch == 1 else arr
    buf = io.BytesIO()
    Image.fromarray(arr, mode if mode != "I;16" else None).save(buf, format="PNG")
    info, scan = png.read_scanlines(buf.getvalue())
    assert len(set(scan[:, 0].tolist())) >= 2                     # the encoder chose filters row by row
    with Image.open(io.BytesIO(buf.getvalue())) as im:
        seen = np.asarray(im)
    assert np.array_equal(seen, arr)
    if mode == "I;16":
        assert info.depth == 16 and info.bpp == 2 and png.label_lane(info) == 1
        hi, lo = (png.unfilter_lane(png.lane_plane(scan, 2, k)) for k in (0, 1))
        assert np.array_equal(hi.astype(np.uint16) << 8 | lo, seen)
    else:
        assert info.depth == 8 and png.label_lane(info) == 0
        planes = seen.reshape(h, w, -1)
        for lane in range(info.bpp):
            assert np.array_equal(png.unfilter_lane(png.lane_plane(scan, info.bpp, lane)), planes[..., lane]), lane


def test_the_low_byte_of_r_holds_the_ids_and_pillow_loses_it():
    png = _png()
    rng = np.random.default_rng(8)
    h, w = 27, 40
    ids = rng.integers(0, 23, (h, w), dtype=np.uint8)
    lab = np.zeros((h, w, 3), np.uint16)
    lab[..., 0] = ids
    lab[..., 1] = rng.integers(256, 65536, (h, w))
    data, _ = png_ref.png_bytes(lab, 16, 2, rng.integers(0, 5, h))
    info, scan = png.read_scanlines(data)
    assert png.label_lane(info) == 1
    assert np.array_equal(png.unfilter_lane(png.lane_plane(scan, info.bpp, png.label_lane(info))), ids)
    Image = pytest.importorskip("PIL.Image")
    with Image.open(io.BytesIO(data)) as im:
        if im.mode != "RGB":
            pytest.skip(f"this Pillow opens 16-bit RGB as {im.mode}")
        seen = np.asarray(im.convert("RGB"))[..., 0]
    assert not np.array_equal(seen, ids) and not seen.any()       # the high byte: why the reader exists


# ------------------------------------------------------------------------------------ refusals
def _ihdr(w=4, h=3, depth=8, colour=0, interlace=0):
    return png_ref.chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour, 0, 0, interlace))


def _file(ihdr, scan_bytes, tail=True):
    return (b"\x89PNG\r\n\x1a\n" + ihdr + png_ref.chunk(b"IDAT", zlib.compress(scan_bytes))
            + (png_ref.chunk(b"IEND", b"") if tail else b""))


GOOD = bytes([0, 1, 2, 3, 4] * 3)   # 3 rows of filter None + 4 bytes


def test_refusals(tmp_path):
    png = _png()
    from maxsquareloss_amd.hip import MSLError
    assert png.read_scanlines(_file(_ihdr(), GOOD))[1].shape == (3, 5)
    cases = {
        "interlaced": _file(_ihdr(interlace=1), GOOD),
        "palette": _file(_ihdr(colour=3), GOOD),
        "bit depth 4": _file(_ihdr(depth=4), GOOD),
        "truncated stream": _file(_ihdr(), GOOD[:-2]),
        "over-long stream": _file(_ihdr(), GOOD + b"\0"),
        "filter byte 7 in row 1": _file(_ihdr(), GOOD[:5] + bytes([7]) + GOOD[6:]),
        "bad signature": b"\x89PNX" + _file(_ihdr(), GOOD)[4:],
        "truncated file": _file(_ihdr(), GOOD, tail=False),
    }
    broken = bytearray(_file(_ihdr(), GOOD))
    broken[8 + 8 + 13 + 4 + 8 + 3] ^= 0x40          # one bit inside the IDAT body
    cases["bad CRC in chunk b'IDAT'"] = bytes(broken)
    cut = _file(_ihdr(), GOOD)
    cases["runs past the end"] = cut[:-20]
    for why, data in cases.items():
        with pytest.raises(MSLError, match=re.escape(why)) as e:
            png.read_scanlines(data)
        assert "<png bytes>" in str(e.value)
    path = tmp_path / "bad.png"
    path.write_bytes(cases["palette"])
    with pytest.raises(MSLError, match=re.escape(str(path))):
        png.read_scanlines(str(path))
    with pytest.raises(MSLError, match="lane 2"):
        png.lane_plane(np.zeros((2, 5), np.uint8), 2, 2)


# ------------------------------------------------------------------------------------ the dataset
def _args(**kw):
    a = argparse.Namespace(base_size=(30, 20), crop_size=(24, 16), seg_size=(30, 20), random_mirror=True,
                           random_crop=True, resize=True, DA=False, seed=3, split="train", class_16=False,
                           class_13=False, batch_size=1, data_loader_workers=0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("class_16", [False, True])
def test_dataset_on_a_tiny_tree(tmp_path, class_16):
    pytest.importorskip("PIL")
    from maxsquareloss_amd.datasets import SYNTHIA_DataLoader, SYNTHIA_Dataset, build_loader
    from maxsquareloss_amd.utils import preprocess
    paths, made = png_ref.synthia_tree(tmp_path / "S")
    args = _args(class_16=class_16, random_crop=False, resize=False, random_mirror=False)
    ds = SYNTHIA_Dataset(args, split="train", training=True, class_16=class_16, **paths)
    assert ds.name == "synthia" and len(ds) == 3 and ds.items == ["7", "10", "13"] and ds.is_train()
    assert ds.rsize == ds.base_size == (30, 20)
    image_path, gt_path, ident = ds.paths(1)
    assert image_path == os.path.join(paths["data_root_path"], "RGB", "0000010.png")
    assert gt_path == os.path.join(paths["data_root_path"], "GT", "LABELS", "0000010.png") and ident == 1
    assert not SYNTHIA_Dataset(args, split="val", training=True, class_16=class_16, **paths).is_train()
    lut = preprocess.build_lut("synthia", class_16)
    assert np.array_equal(ds.lut, lut) and lut.max() == (15 if class_16 else 18)
    for item, (rgb, ids) in enumerate(made["train"]):
        got_rgb, plane = ds.decode(item)
        assert np.array_equal(got_rgb, rgb) and plane.dtype == np.uint8 and plane.shape == (23, 1 + 37)
        img, lab = ds.host_transform(got_rgb, plane, ds.plan(37, 23))
        assert img.shape == (1, 3, 23, 37) and lab.shape == (1, 23, 37)
        assert np.array_equal(lab[0].numpy(), lut[ids].astype(np.int64))
    ld = build_loader("synthia", args, True, paths)
    assert isinstance(ld, SYNTHIA_DataLoader) and (ld.num_iterations, ld.valid_iterations) == (3, 1)
    assert ld.data_loader.dataset.class_16 == class_16 and ld.val_loader.dataset.split == "val"
    ld.close()
    # augmented: the host transform of the decoded plane is the inherited transform of the ids
    aug = SYNTHIA_Dataset(_args(class_16=class_16), split="train", training=True, class_16=class_16, **paths)
    rgb, ids = made["train"][0]
    got_rgb, plane = aug.decode(0)
    plan = aug.plan(37, 23)
    img, lab = aug.host_transform(got_rgb, plane, plan)
    from maxsquareloss_amd.datasets import City_Dataset
    img2, lab2 = City_Dataset.host_transform(aug, rgb, ids, plan)
    assert lab.shape == (1, 20, 30) and (img == img2).all() and (lab == lab2).all()


def test_label_of_another_size_raises(tmp_path):
    pytest.importorskip("PIL")
    from maxsquareloss_amd.datasets import SYNTHIA_Dataset
    from maxsquareloss_amd.hip import MSLError
    paths, _ = png_ref.synthia_tree(tmp_path / "S", bad_size_item=10)
    ds = SYNTHIA_Dataset(_args(), split="train", training=True, **paths)
    ds.decode(0)
    with pytest.raises(MSLError, match="does not match its image"):
        ds.decode(1)


def test_missing_tree_says_what_is_expected(tmp_path):
    from maxsquareloss_amd.datasets import build_loader
    from maxsquareloss_amd.hip import MSLError
    os.makedirs(tmp_path / "RGB")
    paths = {"data_root_path": str(tmp_path), "list_path": str(tmp_path), "gt_path": str(tmp_path / "GT" / "LABELS")}
    with pytest.raises(MSLError) as e:
        build_loader("synthia", argparse.Namespace(), True, paths)
    msg = str(e.value)
    assert "GT/LABELS" in msg and "RGB/{id:07d}.png" in msg and "without imageio's FreeImage plugin" in msg
    assert "the image folder" not in msg                          # only what is missing is named


def test_default_gt_path():
    from maxsquareloss_amd.tools import train_source
    assert train_source.dataset_paths("synthia", "/d/S", None)["gt_path"] == "/d/S/GT/LABELS"
    assert train_source.dataset_paths("synthia", "/d/S", None, "/g")["gt_path"] == "/g"


# ------------------------------------------------------------------------------------ C ABI and build
def test_header_declares_and_library_exports_the_unfilter():
    import ctypes
    from maxsquareloss_amd import hip
    text = open(os.path.join(ROOT, "include", "msl_hip.h")).read()
    flat = " ".join(text.replace("\n * ", " ").split())
    assert ("int msl_png_unfilter_lane(const uint8_t* scan, int h, int w, int bpp, int lane, size_t row_stride, "
            "uint8_t* out, msl_stream_t stream);") in flat
    assert "int msl_png_unfilter_band_rows(void);" in flat
    assert "treats such a row as None" in flat
    res, argt = hip.SIGNATURES["msl_png_unfilter_lane"]
    assert res is ctypes.c_int and len(argt) == 8 and argt[5] is ctypes.c_size_t
    lib = hip.load(require_gpu=False)
    assert hasattr(lib, "msl_png_unfilter_lane")
    band = lib.msl_png_unfilter_band_rows()
    assert band >= 64 and band % 64 == 0
    # the argument checks run before any launch, so they answer without a GPU
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)
    assert lib.msl_png_unfilter_lane(None, 2, 2, 1, 0, 3, p, None) == -3
    assert lib.msl_png_unfilter_lane(p, 2, 2, 1, 1, 3, p, None) == -3


def test_png_kernel_uses_no_scratch():
    """The compiler's resource report of the last build (Makefile: png.o.remarks): one kernel, everything
    in registers - no scratch, no spilled vector or scalar registers."""
    path = os.path.join(ROOT, "maxsquareloss_amd", "_lib", "obj", "png.o.remarks")
    if not os.path.exists(path):
        pytest.skip("no resource report: build the library first (__graft_entry__.build())")
    kern, info = None, {}
    for line in open(path):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            kern = m.group(1)
            info[kern] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|SGPRs Spill|VGPRs Spill): (\d+)",
                      line)
        if m and kern:
            info[kern][m.group(1)] = int(m.group(2))
    assert len(info) == 1 and "k_png_unfilter_lane" in next(iter(info)), sorted(info)
    v = next(iter(info.values()))
    assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, v
