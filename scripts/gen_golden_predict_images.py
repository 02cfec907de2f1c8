"""TEST INFRASTRUCTURE - writes tests/golden/predict_images_kat.npz from the reference's own code.

As scripts/gen_golden_input_pipeline.py does for the loaders, this script reads the source text of the
reference's datasets/cityscapes_Dataset.py (which imports torchvision and so cannot be imported whole),
takes `label_colours`, `IMG_MEAN`, `name_classes`, `flip`, `inv_preprocess` and `decode_labels` out of it by
AST and runs them unmodified.  Only data is written; no reference source enters the repository.  Needs
the reference checkout (--ref) and Pillow.

Keys:
  label_colours [20][3] uint8, img_mean [3] float32, name_classes [20] str
  mask_a [2][7][9], mask_b [1][12][16]   int64 class maps with values from -1 to 20 (counter-based)
  decode_a, decode_b                     decode_labels(mask, num_images=n) * 255 as uint8 (n', 3, h, w); the
                                         float output IS uint8 / 255 in fp32, checked here before writing
  decode_a_n1                            decode_labels(mask_a, num_images=1): one image
  decode_b_n5                            decode_labels(mask_b, num_images=5): n < num_images, one image
  img [2][3][5][6] float32               a BGR - mean shaped batch
  inv_np0, inv_np1                       inv_preprocess(img.clone(), numpy_transform=False / True)
"""
import argparse
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SEED = 97
NAMES = ("IMG_MEAN", "NUM_CLASSES", "label_colours", "name_classes")
FUNCS = ("flip", "inv_preprocess", "decode_labels")


def load(ref_root):
    import torch
    from PIL import Image
    tree = ast.parse(open(os.path.join(ref_root, "datasets", "cityscapes_Dataset.py")).read())
    env = {"np": np, "torch": torch, "Image": Image}
    body = [n for n in tree.body
            if (isinstance(n, ast.Assign) and any(isinstance(t, ast.Name) and t.id in NAMES for t in n.targets))
            or (isinstance(n, ast.FunctionDef) and n.name in FUNCS)]
    exec(compile(ast.Module(body=body, type_ignores=[]), "<ref>", "exec"), env)
    return env


def class_map(n, h, w, tag):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from maxsquareloss_amd.utils.synthetic import counter_uniform
    u = counter_uniform(SEED, f"pi_mask_{tag}", n * h * w)
    m = (np.floor(u * 22).astype(np.int64) - 1).reshape(n, h, w)
    m[0, 0, :4] = (-1, 0, 19, 20)  # both ends, whatever the draw
    return m


def as_u8(t):
    f = t.numpy()
    u = np.rint(f * 255.0).astype(np.uint8)
    assert np.array_equal(u.astype(np.float32) / np.float32(255.0), f)
    return u


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    env = load(a.ref)
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from maxsquareloss_amd.utils.synthetic import counter_normal
    out = {"label_colours": np.array(env["label_colours"], np.uint8), "img_mean": np.asarray(env["IMG_MEAN"]),
           "name_classes": np.array(env["name_classes"])}
    assert env["NUM_CLASSES"] == 19
    ma, mb = class_map(2, 7, 9, "a"), class_map(1, 12, 16, "b")
    assert set(range(-1, 21)) <= set(np.unique(np.concatenate([ma.ravel(), mb.ravel()])).tolist())
    dl = env["decode_labels"]
    out.update(mask_a=ma, mask_b=mb, decode_a=as_u8(dl(torch.from_numpy(ma), 2)), decode_b=as_u8(dl(mb, 1)),
               decode_a_n1=as_u8(dl(ma, 1)), decode_b_n5=as_u8(dl(torch.from_numpy(mb), 5)))
    img = torch.from_numpy(counter_normal(SEED, "pi_img", 2 * 3 * 5 * 6, 60.0)).view(2, 3, 5, 6)
    out["img"] = img.numpy().copy()
    for flag in (False, True):
        out[f"inv_np{int(flag)}"] = env["inv_preprocess"](img.clone(), 2, env["IMG_MEAN"], flag).numpy()
    path = os.path.join(a.out, "predict_images_kat.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
