"""TEST INFRASTRUCTURE - writes tests/golden/input_pipeline_kat.npz from the reference's own loader code.

As oracle/gen_golden_preprocess.py does for the last transform, this script reads the source text of
the reference's datasets/cityscapes_Dataset.py, takes City_Dataset._train_sync_transform,
_val_sync_transform, _img_transform, _mask_transform and id2trainId out of it by AST and runs them,
unmodified, with real Pillow and the global `random` seeded per item, on generated uint8 images and
id maps.  It records the inputs (as generator arguments + checksum), the draws (mirror, x1, y1) - learnt by re-seeding and repeating
the reference's draws - and the outputs.  Only data is written; no reference source enters the
repository.  Needs the reference checkout and Pillow (skips without either).

Keys (k = noise kind: u uniform, s saturated 0/255; m = mirror 0/1; all sizes (w, h) as Pillow's):
  img_mean                                   the reference's IMG_MEAN
  resize_cases [n][4] = (h, w, ow, oh)       the plain resize cases
  c{i}_{k}_rgb_gen, c{i}_ids_gen             inputs of case i, as (seed, h, w, CRC-32 of the bytes): kat_input()
                                             regenerates them (noise() / id_map(), counter-based) and checks the CRC
  f32_of_byte [3][256]                       _img_transform of a byte ramp: plane c of a pixel whose byte is v
  c{i}_{k}_m{m}_u8                           _train_sync_transform's image, (oh, ow, 3) uint8 RGB: the fp32
                                             (3, oh, ow) BGR - mean output IS f32_of_byte[c][u8[..., 2 - c]], bit
                                             for bit (checked here before writing; fp32 noise does not compress,
                                             its 256 values per plane do)
  c{i}_m{m}_ids                              Pillow's NEAREST resize of the (mirrored) id map, raw ids
  c{i}_m{m}_city19                           _mask_transform's trainIds (int8, -1 = ignore)
  c{i}_m0_{city16,gta19,gta16}               the other tables, unmirrored
  crop_{k}_rgb_gen, crop_ids_gen, crop_box = (x1, y1, w, h), crop_sizes [j] = (ow, oh)
  crop_{k}_o{j}_m{m}_u8, crop_o{j}_m{m}_{ids,city19}    mirror, crop at crop_box, resize to size j
  chain_cfg = (crop w, h, base w, h, rsize w, h, val rsize w, h)
  chain_{train,val}{n}_draw = (mirror, x1, y1), _seed, _u8, _city19    the chained transforms on crop_u_rgb
"""
import argparse
import ast
import os
import random
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

CASES = [(41, 67, 33, 20), (30, 50, 77, 45), (40, 60, 60, 17), (40, 60, 31, 40), (24, 36, 36, 24), (37, 1030, 515, 19)]
CROP_SRC = (60, 90)          # (h, w)
CROP_BOX = (7, 5, 40, 30)    # (x1, y1, w, h)
CROP_SIZES = [(33, 20), (77, 45), (40, 30)]
CHAIN = dict(crop=(40, 30), base=(50, 36), rsize=(33, 20), val_rsize=(70, 44))


def load(ref_root):
    import torch
    from PIL import Image
    tree = ast.parse(open(os.path.join(ref_root, "datasets", "cityscapes_Dataset.py")).read())
    env = {"np": np, "torch": torch, "Image": Image, "random": random, "ttransforms": None}
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "IMG_MEAN" for t in node.targets):
            env["IMG_MEAN"] = eval(compile(ast.Expression(node.value), "<ref>", "eval"), dict(env))
    city = next(n for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and n.name == "City_Dataset")
    fns = {}
    for name in ("_train_sync_transform", "_val_sync_transform", "_img_transform", "_mask_transform", "id2trainId"):
        node = next(n for n in city.body if isinstance(n, ast.FunctionDef) and n.name == name)
        ns = dict(env)
        exec(compile(ast.Module(body=[node], type_ignores=[]), "<ref>", "exec"), ns)
        fns[name] = ns[name]
    init = next(n for n in city.body if isinstance(n, ast.FunctionDef) and n.name == "__init__")

    def assigned(match):
        for node in ast.walk(init):
            if isinstance(node, ast.Assign) and any(match(t) for t in node.targets):
                return eval(compile(ast.Expression(node.value), "<ref>", "eval"), dict(env, ignore_label=-1))
        raise KeyError

    table = assigned(lambda t: isinstance(t, ast.Attribute) and t.attr == "id_to_trainid")
    set16 = assigned(lambda t: isinstance(t, ast.Name) and t.id == "synthia_set_16")
    gtree = ast.parse(open(os.path.join(ref_root, "datasets", "gta5_Dataset.py")).read())
    gta = next(n for n in ast.walk(gtree) if isinstance(n, ast.ClassDef) and n.name == "GTA5_Dataset")
    ginit = next(n for n in gta.body if isinstance(n, ast.FunctionDef) and n.name == "__init__")
    gtable = next(eval(compile(ast.Expression(n.value), "<ref>", "eval"), {})
                  for n in ast.walk(ginit) if isinstance(n, ast.Assign)
                  and any(isinstance(t, ast.Attribute) and t.attr == "id_to_trainid" for t in n.targets))
    return env["IMG_MEAN"], fns, {"city": table, "gta": gtable}, set16


def dataset(fns, table, set16, class_16, **kw):
    """A stand-in `self` carrying the reference's methods and the attributes they read."""
    s = types.SimpleNamespace(args=types.SimpleNamespace(DA=False, numpy_transform=True), id_to_trainid=table,
                              class_16=class_16, class_13=False, trainid_to_16id={t: i for i, t in enumerate(set16)},
                              trainid_to_13id={}, **kw)
    for name, fn in fns.items():
        setattr(s, name, types.MethodType(fn, s))
    return s


def draws(seed, mirror_on, crop, w, h):
    """What the reference draws after random.seed(seed): (mirror, x1, y1)."""
    random.seed(seed)
    mirror = int(mirror_on and random.random() < 0.5)
    x1 = y1 = 0
    if crop:
        x1 = random.randint(0, w - crop[0])
        y1 = random.randint(0, h - crop[1])
    return mirror, x1, y1


def seed_for(want, mirror_on, crop, w, h):
    return next(s for s in range(10 ** 6) if draws(s, mirror_on, crop, w, h) == want)


def _uniform(seed, name, n):
    import sys
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from maxsquareloss_amd.utils.synthetic import counter_uniform  # splitmix64 counters: the same on every numpy
    return counter_uniform(seed, name, n)


def noise(seed, h, w, kind):
    """The generated image of (seed, kind): u = uniform bytes, s = saturated 0 / 255 bytes."""
    u = _uniform(seed, "kat_rgb_" + kind, h * w * 3)
    v = np.floor(u * 256.0) if kind == "u" else np.where(u < 0.5, 0, 255)
    return v.astype(np.uint8).reshape(h, w, 3)


def id_map(seed, h, w):
    """The generated id map: mostly the labelled range 0..34, the rest anywhere in 0..255; every low id appears."""
    n = h * w
    pick, low, any_ = (_uniform(seed, "kat_ids_" + t, n) for t in ("pick", "low", "any"))
    ids = np.where(pick < 0.7, np.floor(low * 35), np.floor(any_ * 256)).astype(np.uint8)
    ids[:64] = np.arange(64, dtype=np.uint8)
    return ids.reshape(h, w)


def kat_input(fix, key):
    """Input `key` of the fixture ('c3_u_rgb', 'crop_ids', ...): regenerated from its recorded
    (seed, h, w) and checked against its recorded CRC-32 - the inputs are uniform noise, which does not
    compress, so the file carries their generator's arguments and a checksum instead of the bytes."""
    import zlib
    seed, h, w, crc = (int(v) for v in fix[key + "_gen"])
    arr = id_map(seed, h, w) if key.endswith("_ids") else noise(seed, h, w, key.split("_")[-2])
    if zlib.crc32(arr.tobytes()) != crc:
        raise AssertionError(f"{key}: the regenerated input does not match the recorded checksum")
    return arr


def _record(out, key, seed, arr):
    import zlib
    out[key + "_gen"] = np.array([seed, arr.shape[0], arr.shape[1], zlib.crc32(arr.tobytes())], np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    try:
        from PIL import Image
    except ImportError:
        print("Pillow not present; the golden file is committed, nothing to do")
        return
    if not os.path.isdir(a.ref):
        print("reference not present; the golden file is committed, nothing to do")
        return
    mean, fns, tables, set16 = load(a.ref)
    luts = {"city19": ("city", False), "city16": ("city", True), "gta19": ("gta", False), "gta16": ("gta", True)}
    out = {"img_mean": np.asarray(mean, np.float32), "resize_cases": np.array(CASES, np.int32)}

    ramp = np.repeat(np.arange(256, dtype=np.uint8).reshape(1, 256, 1), 3, axis=2)
    f32_of_byte = dataset(fns, tables["city"], set16, False)._img_transform(Image.fromarray(ramp)).numpy()[:, 0, :]
    out["f32_of_byte"] = f32_of_byte

    def run(ds, rgb, ids, seed, train=True):
        """(image as uint8 RGB HWC, trainIds int8) of the reference's transform; the image's fp32 planes
        are re-encoded through f32_of_byte, losslessly (asserted)."""
        random.seed(seed)
        fn = ds._train_sync_transform if train else ds._val_sync_transform
        img, lab = fn(Image.fromarray(rgb), Image.fromarray(ids))
        img = img.numpy()
        bgr = np.rint(img + np.asarray(mean, np.float32).reshape(3, 1, 1)).astype(np.int64)
        assert bgr.min() >= 0 and bgr.max() <= 255
        back = np.stack([f32_of_byte[c][bgr[c]] for c in range(3)])
        assert back.dtype == np.float32 and back.tobytes() == img.tobytes(), "fp32 re-encoding is not lossless"
        return np.ascontiguousarray(bgr[::-1].transpose(1, 2, 0).astype(np.uint8)), lab.numpy().astype(np.int8)

    def resized_ids(ids, mirror, box, size):
        im = Image.fromarray(ids)
        if mirror:
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
        if box:
            im = im.crop((box[0], box[1], box[0] + box[2], box[1] + box[3]))
        return np.asarray(im.resize(size, Image.NEAREST))

    # plain resizes: random_mirror on (the seed picks the mirror), no crop, resize to (ow, oh)
    for i, (h, w, ow, oh) in enumerate(CASES):
        ids = id_map(100 + i, h, w)
        _record(out, f"c{i}_ids", 100 + i, ids)
        for k in "us":
            rgb = noise(100 + i, h, w, k)
            _record(out, f"c{i}_{k}_rgb", 100 + i, rgb)
            for m in (0, 1):
                seed = seed_for((m, 0, 0), True, None, w, h)
                for tag, (tab, c16) in luts.items():
                    ds = dataset(fns, tables[tab], set16, c16, random_mirror=True, random_crop=False, resize=True,
                                 rsize=(ow, oh))
                    img, lab = run(ds, rgb, ids, seed)
                    out[f"c{i}_{k}_m{m}_u8"] = img
                    if k == "u" and (m == 0 or tag == "city19"):
                        out[f"c{i}_m{m}_{tag}"] = lab
                out[f"c{i}_m{m}_ids"] = resized_ids(ids, m, None, (ow, oh))

    # mirror + crop at an odd offset + resize (the crop is a source offset, not Pillow's box=)
    h, w = CROP_SRC
    ids = id_map(200, h, w)
    _record(out, "crop_ids", 200, ids)
    out["crop_box"], out["crop_sizes"] = np.array(CROP_BOX, np.int32), np.array(CROP_SIZES, np.int32)
    for k in "us":
        rgb = noise(200, h, w, k)
        _record(out, f"crop_{k}_rgb", 200, rgb)
        for j, size in enumerate(CROP_SIZES):
            for m in (0, 1):
                seed = seed_for((m, CROP_BOX[0], CROP_BOX[1]), True, CROP_BOX[2:], w, h)
                ds = dataset(fns, tables["city"], set16, False, random_mirror=True, random_crop=True, resize=False,
                             crop_size=CROP_BOX[2:], base_size=size)
                img, lab = run(ds, rgb, ids, seed)
                out[f"crop_{k}_o{j}_m{m}_u8"] = img
                if k == "u":
                    out[f"crop_o{j}_m{m}_city19"] = lab
                    out[f"crop_o{j}_m{m}_ids"] = resized_ids(ids, m, CROP_BOX, size)

    # the chained transforms on crop_u_rgb: train = mirror, crop, resize to base, resize to rsize;
    # val = resize to rsize first, then crop and resize to base
    rgb = noise(200, h, w, "u")
    c = CHAIN
    out["chain_cfg"] = np.array(c["crop"] + c["base"] + c["rsize"] + c["val_rsize"], np.int32)
    for n, seed in enumerate((seed_for((0, 11, 3), True, c["crop"], w, h), seed_for((1, 24, 17), True, c["crop"], w, h))):
        ds = dataset(fns, tables["city"], set16, False, random_mirror=True, random_crop=True, resize=True,
                     crop_size=c["crop"], base_size=c["base"], rsize=c["rsize"])
        out[f"chain_train{n}_draw"] = np.array(draws(seed, True, c["crop"], w, h), np.int32)
        out[f"chain_train{n}_seed"] = np.array(seed, np.int64)
        out[f"chain_train{n}_u8"], out[f"chain_train{n}_city19"] = run(ds, rgb, ids, seed)
    vw, vh = c["val_rsize"]
    for n, seed in enumerate((seed_for((0, 13, 9), False, c["crop"], vw, vh),)):
        ds = dataset(fns, tables["city"], set16, False, random_mirror=True, random_crop=True, resize=True,
                     crop_size=c["crop"], base_size=c["base"], rsize=c["val_rsize"])
        out[f"chain_val{n}_draw"] = np.array(draws(seed, False, c["crop"], vw, vh), np.int32)
        out[f"chain_val{n}_seed"] = np.array(seed, np.int64)
        out[f"chain_val{n}_u8"], out[f"chain_val{n}_city19"] = run(ds, rgb, ids, seed, train=False)

    path = os.path.join(a.out, "input_pipeline_kat.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
