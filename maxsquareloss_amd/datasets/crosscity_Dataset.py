"""CrossCity_Dataset / CrossCity_DataLoader (datasets/crosscity_Dataset.py:16-124 of the reference), MI355X
path: City_Dataset's device transform over one city of the NTHU cross-city dataset (Rio, Rome, Tokyo, Taipei) -
Images/Train/{id}.jpg listed in <list_path>/train.txt, unlabelled; Images/Test/{id}.jpg with
Labels/Test/{id}_eval.png (8-bit Cityscapes ids) listed in <list_path>/test.txt; {id}.png where there is no
{id}.jpg.  `id_to_trainid` restates Cityscapes' table (crosscity_Dataset.py:56-58), with class_13 cut down to
the 13 classes the cities share.

The images are 2048x1024 JPEGs, and a host decode of one costs about as much as a training step.  decode()
therefore stops after the serial part: utils/jpeg.py parses the file and Huffman-decodes its scan on the
decoding thread, the coefficients travel through the pinned staging slot in place of the image, and the
dense rest - dequantisation, inverse DCT, chroma upsampling, YCbCr -> RGB - runs on the device
(utils/preprocess.py jpeg_reconstruct, csrc/jpeg.hip) ahead of the inherited mirror / crop / BICUBIC resize
chain, byte-exact against Pillow.  With --jpeg_decode pillow, and for a file the split decoder refuses
(progressive, CMYK, ...), Pillow decodes the whole file as for every other dataset; the item is the same bytes
either way.

Quirks: the reference's constructor cannot run as written - it reads `base_size` / `crop_size`, which it never
defines, and tools/solve_crosscity.py passes it base_size= / crop_size= keywords it does not accept; here both
come from `args`, as in City_Dataset (the trainer hands the target's sizes over in its copy of the arguments).
Like its GTA5 and SYNTHIA classes this class never sets `rsize`, so --resize True would raise AttributeError at
the first item; here that resize goes to base_size (as gta5_Dataset.py).  Its train items are (image, image,
item) and the trainer drops the second; here they are (image, None, id), as Client_dataset's.  Its loader builds
the val split from GTA5_Dataset, which it never imports; here the val split is this class's.  --gaussian_blur
is stored and never applied there; it is not read here."""
import os

import numpy as np
import torch

from ..hip import MSLError
from ..utils import jpeg, preprocess, resample
from ..utils.synthetic import IMG_MEAN
from .cityscapes_Dataset import City_DataLoader, City_Dataset, _pil, decode_rgb, image_of

CITIES = ("Rome", "Rio", "Tokyo", "Taipei")
LAYOUT = ("<root>/Images/Train/{id}.jpg (or .png) listed in <list_path>/train.txt, <root>/Images/Test/{id}.jpg "
          "with <root>/Labels/Test/{id}_eval.png (8-bit Cityscapes ids) listed in <list_path>/test.txt; <root> is "
          "one city of the NTHU dataset, <list_path> its List folder")


class CrossCity_Dataset(City_Dataset):
    name = "crosscity"

    def __init__(self, args, data_root_path="./datasets/NTHU_Datasets/Rio", list_path="./datasets/NTHU_list/Rio/List",
                 gt_path=None, split="train", training=True, class_13=False):
        self.args = args
        self.data_path, self.list_path = data_root_path, list_path
        self.split, self.training = split, training
        self._setup(args)
        self.rsize = self.base_size
        if split == "train":
            stem, sub = "train", "Train"
        elif split == "val":
            stem, sub = "test", "Test"
        else:
            raise Warning("split must be train/val")
        self.items = self._read_list(stem)
        self.image_filepath = os.path.join(self.data_path, "Images", sub)
        self.gt_filepath = gt_path if gt_path is not None else os.path.join(self.data_path, "Labels", sub)
        self.id_to_trainid = dict(preprocess.CITYSCAPES_ID_TO_TRAINID)
        self.class_16, self.class_13 = False, bool(class_13)
        self.lut = preprocess.build_lut("cityscapes", False, self.class_13)
        self.jpeg_decode = getattr(args, "jpeg_decode", "device")
        if self.jpeg_decode not in ("device", "pillow"):
            raise MSLError(f"--jpeg_decode {self.jpeg_decode!r}: device | pillow")

    def is_train(self):
        return self.split == "train" and self.training  # crosscity_Dataset.py:76

    def labelled(self):
        return not self.is_train()

    def paths(self, item):
        """(image path - {id}.jpg, else {id}.png - the label path or None, the id the item carries)."""
        ident = self.items[item]
        image = os.path.join(self.image_filepath, f"{ident}.jpg")
        if not os.path.exists(image):
            image = os.path.join(self.image_filepath, f"{ident}.png")
        gt = os.path.join(self.gt_filepath, f"{ident}_eval.png") if self.labelled() else None
        return image, gt, item

    def decode(self, item, alloc=None):
        """(the image: a JPEG's payload or Pillow's (H, W, 3) array (decode_rgb); the (H, W) ids or None).
        alloc(nbytes): where a payload goes - DeviceLoader passes its pinned staging slot (decode_into), so the
        Huffman decoder writes the coefficients where the H2D copy reads them."""
        image_path, gt_path, _ = self.paths(item)
        rgb = decode_rgb(image_path, self.jpeg_decode, alloc)
        if gt_path is None:
            return rgb, None
        with _pil().open(gt_path) as im:
            ids = np.asarray(im)
        if ids.ndim != 2 or ids.dtype != np.uint8:
            raise MSLError(f"{gt_path}: expected a 2-D uint8 label map, got shape {ids.shape} dtype {ids.dtype}")
        size = jpeg.size_of(rgb)
        if ids.shape != size:
            raise MSLError(f"{gt_path}: label map {ids.shape} does not match its image {size}")
        return rgb, ids

    decode_into = decode

    def host_transform(self, rgb, ids, plan):
        if jpeg.is_payload(rgb):
            rgb = jpeg.reconstruct(rgb.numpy() if hasattr(rgb, "numpy") else rgb)
        plan = plan[:2]
        if ids is not None:
            return super().host_transform(rgb, ids, plan)
        mirror, steps = plan
        for out_wh, crop in steps:
            rgb = resample.resize_bicubic(rgb, out_wh, crop, mirror)
            mirror = False
        return torch.from_numpy(resample.bgr_minus_mean(rgb, IMG_MEAN)).unsqueeze(0), None

    def device_transform(self, rgb, ids, plan):
        rgb, plan = image_of(rgb, plan)
        if ids is not None:
            return super().device_transform(rgb, ids, plan)
        mirror, steps = plan
        for k, (out_wh, crop) in enumerate(steps):
            rgb = preprocess.resize_image(rgb, out_wh, crop, mirror, as_uint8=k != len(steps) - 1)
            mirror = False
        return rgb, None


class CrossCity_DataLoader(City_DataLoader):
    """crosscity_Dataset.py:84-124: data_loader over the 'train' split (shuffled), val_loader over 'val' (test.txt)."""
    dataset_class = CrossCity_Dataset

    def _make(self, args, kw, extra, split, training):
        if split not in ("train", "val"):
            raise Warning("split must be train")
        return CrossCity_Dataset(args, split=split, training=training, class_13=extra["class_13"], **kw)


def check_tree(paths):
    """MSLError unless the city's tree of paths = {data_root_path, list_path, gt_path} is there; reads nothing but
    the file system."""
    root, lists = paths["data_root_path"], paths["list_path"]
    want = [(f"the image folder {os.path.join(root, 'Images', sub)}", os.path.join(root, "Images", sub))
            for sub in ("Train", "Test")]
    gt = paths.get("gt_path") or os.path.join(root, "Labels", "Test")
    want += [(f"the label folder {gt}", gt), (f"the list folder {lists}", lists)]
    missing = [what for what, p in want if not os.path.isdir(p)]
    missing += [f"the list {os.path.join(lists, f)}" for f in ("train.txt", "test.txt")
                if os.path.isdir(lists) and not os.path.exists(os.path.join(lists, f))]
    if missing:
        raise MSLError(f"file-backed NTHU cross-city: {', '.join(missing)} {'is' if len(missing) == 1 else 'are'} "
                       f"missing; the expected layout is {LAYOUT}")
