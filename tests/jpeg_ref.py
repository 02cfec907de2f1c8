"""Shared by the JPEG / cross-city tests: generated JPEG files (Pillow's own encoder), Pillow's decode as the
oracle, the truncated and corrupted streams of the robustness tests, and a tiny NTHU-style tree."""
import io
import os

import numpy as np

HEIGHTS = (1, 2, 3, 8, 9, 16, 17, 33)
WIDTHS = tuple(range(1, 10)) + (15, 16, 17, 31, 32, 33, 49)
SAMPLINGS = (0, 1, 2, "L")          # 4:4:4, 4:2:2, 4:2:0, grayscale
QUALITIES = (1, 50, 75, 100)
KINDS = ("noise", "two", "smooth")
# every way the scan is laid out: plain, optimised Huffman tables, a restart every 1 / 2 / 3 blocks and every MCU row
OPTIONS = ({}, {"optimize": True}, {"restart_marker_blocks": 1}, {"restart_marker_blocks": 2},
           {"restart_marker_blocks": 3}, {"restart_marker_rows": 1})


def picture(kind, h, w, rng):
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == "two":
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(xx * 5) % 256, (yy * 7) % 256, (xx + yy) * 3 % 256], -1).astype(np.uint8)


def photo(h, w, seed=1):
    """A photo-like image: gradients with noise on top."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([xx / 8 + yy / 16, yy / 4, (xx + yy) / 12], -1) % 256
    return (base + rng.normal(0, 12, (h, w, 3))).clip(0, 255).astype(np.uint8)


def encode(a, sampling=2, **kw):
    from PIL import Image
    im = Image.fromarray(a)
    if sampling == "L":
        im = im.convert("L")
    elif im.mode == "RGB":
        kw["subsampling"] = sampling
    b = io.BytesIO()
    im.save(b, "JPEG", **kw)
    return b.getvalue()


def pillow_rgb(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def sweep(h, widths=WIDTHS):
    """Every (width, sampling, quality, picture) at height h as (label, file bytes); the six scan layouts cycle
    so that each (size, sampling) meets each of them twice."""
    rng = np.random.default_rng(1000 + h)
    for w in widths:
        pics = {k: picture(k, h, w, rng) for k in KINDS}
        for s in SAMPLINGS:
            for qi, q in enumerate(QUALITIES):
                for ki, kind in enumerate(KINDS):
                    opt = OPTIONS[(qi * len(KINDS) + ki) % len(OPTIONS)]
                    yield (h, w, s, q, kind, tuple(opt)), encode(pics[kind], s, quality=q, **opt)


def unsupported():
    """(name, bytes): valid files the split decoder must refuse with MSL_ERR_SHAPE."""
    from PIL import Image
    a = photo(24, 40, 5)
    out = [("progressive", encode(a, 2, quality=80, progressive=True)),
           ("keep_rgb", encode(a, 0, quality=80, keep_rgb=True))]
    b = io.BytesIO()
    Image.fromarray(a).convert("CMYK").save(b, "JPEG", quality=80)
    return out + [("cmyk", b.getvalue())]


def fuzz_files():
    """Two small files, the second with restart markers."""
    return [encode(photo(19, 27, 2), 2, quality=60), encode(photo(17, 33, 3), 1, quality=85, restart_marker_blocks=2)]


def fuzz_streams(seed=0):
    """Every proper prefix of the two files and 200 seeded single-byte corruptions of each."""
    rng = np.random.default_rng(seed)
    for data in fuzz_files():
        for n in range(len(data)):
            yield data[:n]
        for _ in range(200):
            b = bytearray(data)
            b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
            yield bytes(b)


def golden_cases():
    """The six files of tests/golden/jpeg_kat.npz (scripts/gen_golden_jpeg.py)."""
    rng = np.random.default_rng(42)
    return [encode(picture("noise", 33, 49, rng), 0, quality=75),
            encode(picture("two", 17, 31, rng), 1, quality=100, restart_marker_rows=1),
            encode(picture("smooth", 33, 33, rng), 2, quality=50, optimize=True),
            encode(photo(40, 70, 9), 2, quality=92, restart_marker_blocks=2),
            encode(picture("noise", 17, 9, rng), "L", quality=75),
            encode(picture("noise", 3, 4, rng), 2, quality=1)]


def nthu_tree(root, city="Rome", n=3, val_n=2, hw=(40, 56), seed=5, png_item=None):
    """A tiny NTHU-style tree: <root>/<city>/Images/{Train,Test}/*.jpg, Labels/Test/*_eval.png and
    <root>/<city>/List/{train,test}.txt.  Returns (paths of the city, {list name: [(jpeg bytes, ids or None)]});
    `png_item` names a train item stored as .png instead of .jpg."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    croot = os.path.join(str(root), city)
    lists = os.path.join(croot, "List")
    for d in ("Images/Train", "Images/Test", "Labels/Test", "List"):
        os.makedirs(os.path.join(croot, d))
    made = {"train": [], "test": []}
    samplings = (2, 1, 0)
    for name, sub, count in (("train", "Train", n), ("test", "Test", val_n)):
        with open(os.path.join(lists, name + ".txt"), "w") as f:
            for i in range(count):
                ident = f"pano_{name}_{i:03d}"
                a = photo(hw[0], hw[1], seed * 100 + len(made["train"]) + 10 * len(made["test"]))
                if name == "train" and png_item == i:
                    Image.fromarray(a).save(os.path.join(croot, "Images", sub, ident + ".png"))
                    data = a
                else:
                    data = encode(a, samplings[i % 3], quality=90)
                    with open(os.path.join(croot, "Images", sub, ident + ".jpg"), "wb") as g:
                        g.write(data)
                ids = None
                if name == "test":
                    ids = rng.integers(0, 40, hw, dtype=np.uint8)
                    Image.fromarray(ids).save(os.path.join(croot, "Labels", sub, ident + "_eval.png"))
                f.write(ident + "\n")
                made[name].append((data, ids))
    return {"data_root_path": croot, "list_path": lists, "gt_path": os.path.join(croot, "Labels", "Test")}, made
