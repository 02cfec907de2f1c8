"""SYNTHIA_Dataset / SYNTHIA_DataLoader (datasets/synthia_Dataset.py:17-130 of the reference), MI355X
path: City_Dataset's device transform over SYNTHIA-RAND-CITYSCAPES' files - RGB/{id:07d}.png and
GT/LABELS/{id:07d}.png, ids listed in <list_path>/<split>.txt.

The labels are 16-bit RGB PNGs, R the class id and G the instance id; the reference keeps
`np.uint8(imageio.imread(path, format='PNG-FI')[:, :, 0])`, the low byte of R.  Pillow keeps the high
byte of a 16-bit sample, so the label file does not go through Pillow: utils/png.py inflates it on the
decoding thread and slices that one byte lane out (filter byte + one byte per pixel), the plane travels
through the pinned staging slot in place of the id map, and the PNG filters are undone on the device
(utils/preprocess.py png_unfilter, csrc/png.hip) ahead of the inherited mirror / crop / NEAREST resize /
id -> trainId chain.  8-bit label files take the same path (lane 0).

Quirks: like the reference's GTA5 class this class never sets `rsize`, so the reference's first item
raises AttributeError with --resize True; here that resize goes to base_size (as gta5_Dataset.py).
The reference's SYNTHIA_DataLoader never passes class_16 on to its dataset (its labels stay 19-class
trainIds whatever --num_classes says); here the loader passes args.class_16, which init_args derives from
--num_classes 16, so the labels match the 16-class head."""
import os

import numpy as np

from ..hip import MSLError
from ..utils import png, preprocess
from .cityscapes_Dataset import City_DataLoader, City_Dataset, _pil

LAYOUT = ("<root>/RGB/{id:07d}.png (images), <root>/GT/LABELS/{id:07d}.png (16-bit label PNGs, R = class id) "
          "and <list_path>/<split>.txt (one id per line)")


class SYNTHIA_Dataset(City_Dataset):
    name = "synthia"

    def __init__(self, args, data_root_path="./datasets/SYNTHIA", list_path="./datasets/SYNTHIA/list", gt_path=None,
                 split="train", training=True, class_16=False):
        self.args = args
        self.data_path, self.list_path = data_root_path, list_path
        self.split, self.training = split, training
        self._setup(args)
        self.rsize = self.base_size
        self.items = self._read_list(split)  # synthia_Dataset.py:44: the list is <split>.txt
        self.image_filepath = os.path.join(self.data_path, "RGB")
        self.gt_filepath = gt_path if gt_path is not None else os.path.join(self.data_path, "GT", "LABELS")
        self.class_16, self.class_13 = bool(class_16), False
        self.lut = preprocess.build_lut(self.name, self.class_16)

    def is_train(self):
        return self.split in ("train", "trainval", "all") and self.training  # synthia_Dataset.py:77

    def paths(self, item):
        name = "{:0>7d}.png".format(int(self.items[item]))
        return os.path.join(self.image_filepath, name), os.path.join(self.gt_filepath, name), item

    def decode(self, item):
        """(rgb (H, W, 3) uint8 from Pillow, plane (H, 1 + W) uint8): the label's inflated scanlines cut down
        to the byte lane the reference keeps, still PNG-filtered.  Host only, thread-safe."""
        Image = _pil()
        image_path, gt_path, _ = self.paths(item)
        with Image.open(image_path) as im:
            rgb = np.asarray(im.convert("RGB"), np.uint8)
        info, scan = png.read_scanlines(gt_path)
        if (info.height, info.width) != rgb.shape[:2]:
            raise MSLError(f"{gt_path}: label map {(info.height, info.width)} does not match its image "
                           f"{rgb.shape[:2]}")
        return rgb, png.lane_plane(scan, info.bpp, png.label_lane(info))

    def host_transform(self, rgb, plane, plan):
        return super().host_transform(rgb, png.unfilter_lane(plane), plan)

    def device_transform(self, rgb, plane, plan):
        return super().device_transform(rgb, preprocess.png_unfilter(plane), plan)


class SYNTHIA_DataLoader(City_DataLoader):
    """synthia_Dataset.py:84-130: data_loader over args.split (shuffled for train), val_loader over 'val'
    when training on 'train', else 'test'."""
    dataset_class = SYNTHIA_Dataset

    def _val_split(self, args):
        return "val" if args.split == "train" else "test"

    def _make(self, args, kw, extra, split, training):
        if "train" not in split and split not in ("val", "test", "all"):
            raise Warning("split must be train/val/trainavl/test/all")
        return SYNTHIA_Dataset(args, split=split, training=training, class_16=extra["class_16"], **kw)


def check_tree(paths):
    """MSLError unless the SYNTHIA tree of paths = {data_root_path, list_path, gt_path} is there; reads
    nothing but the file system."""
    root, lists, gt = paths["data_root_path"], paths["list_path"], paths["gt_path"]
    gt = gt if gt is not None else os.path.join(root, "GT", "LABELS")
    missing = [what for what, p in ((f"the image folder {os.path.join(root, 'RGB')}", os.path.join(root, "RGB")),
                                    (f"the label folder {gt}", gt), (f"the list folder {lists}", lists))
               if not os.path.isdir(p)]
    if missing:
        raise MSLError(f"file-backed SYNTHIA: {', '.join(missing)} {'is' if len(missing) == 1 else 'are'} missing; "
                       f"the expected layout is {LAYOUT}.  The 16-bit labels are decoded by this package's own "
                       "PNG reader (utils/png.py), without imageio's FreeImage plugin")
