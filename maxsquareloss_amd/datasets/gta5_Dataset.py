"""GTA5_Dataset / GTA5_DataLoader (datasets/gta5_Dataset.py:34-142 of the reference), MI355X path:
City_Dataset's device transform over GTA5's files - images/{id:05d}.png and gt_path/{id:05d}.png,
ids listed in train.txt, the val split in test.txt.

Quirk: the reference's GTA5 class never sets `rsize`, so its first item raises AttributeError
with --resize True; here that resize goes to base_size."""
import os

from ..utils import preprocess
from .cityscapes_Dataset import City_DataLoader, City_Dataset


class GTA5_Dataset(City_Dataset):
    name = "gta5"

    def __init__(self, args, data_root_path="./datasets/GTA5", list_path="./datasets/GTA5/list", gt_path=None,
                 split="train", training=True):
        self.args = args
        self.data_path, self.list_path = data_root_path, list_path
        self.split, self.training = split, training
        self._setup(args)
        self.rsize = self.base_size
        self.items = self._read_list("train" if "train" in split else "test")
        self.image_filepath = os.path.join(self.data_path, "images")
        self.gt_filepath = gt_path
        self.class_16 = self.class_13 = False
        self.lut = preprocess.build_lut(self.name)

    def paths(self, item):
        ident = int(self.items[item])
        name = "{:0>5d}.png".format(ident)
        return os.path.join(self.image_filepath, name), os.path.join(self.gt_filepath, name), str(ident)


class GTA5_DataLoader(City_DataLoader):
    """gta5_Dataset.py:98-142: data_loader over args.split (shuffled for train), val_loader over
    'val' (test.txt) when training on train, else 'test'."""
    dataset_class = GTA5_Dataset

    def _val_split(self, args):
        return "val" if "train" in args.split else "test"

    def _make(self, args, kw, extra, split, training):
        if "train" not in split and "val" not in split and "test" not in split:
            raise Warning("split must be train/val/trainavl/test/all")
        return GTA5_Dataset(args, split=split, training=training, **kw)
