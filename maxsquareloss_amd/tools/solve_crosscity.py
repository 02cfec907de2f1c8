"""Cityscapes -> NTHU cross-city UDA trainer (tools/solve_crosscity.py of the reference), MI355X path.

The iteration is solve_gta5.py's - the reference's solve_crosscity.py:144-271 restates it line for line - so
CrossCityTrainer is UDATrainer with other data: --pair, --graph, data-parallel exchange, --optim and every
--target_mode are inherited unchanged.  What differs (solve_crosscity.py:35-142):
  - the source is Cityscapes (--source_dataset cityscapes), cut down to the 13 classes the cities share
    (--num_classes 13, the default here: the reference's README runs it so);
  - the target is one city of the NTHU dataset (--city_name): <data_root_path>/<city_name> with its lists in
    <list_path>/<city_name>/List (datasets/crosscity_Dataset.py).  Its train images carry no labels; its
    2048x1024 JPEGs are Huffman-decoded on the decoding threads and finished on the device (--jpeg_decode);
  - main() validates on the city's test split and on the source's val split (validate_source) before it
    trains, and validates the source again after every epoch; the source numbers are logged only;
  - one run is --epoch_num epochs (no rounds), --lambda_target 0.1 and --threshold 0.98 by default; with
    --target_mode hard --threshold_mode class the per-class thresholds are regenerated before every epoch.
Without paths the source and target items are synthetic, as in every trainer here; validate_source then runs
on --val_images synthetic items of the source size.
"""
import argparse
import copy
import os

from ..datasets import build_loader
from ..datasets.crosscity_Dataset import CITIES
from ..hip import MSLError
from ..utils.synthetic import SyntheticDomain
from ..utils.validate import VAL_OFFSET, Validator, val_info
from .solve_gta5 import UDATrainer, add_UDA_train_args
from .train_source import Trainer, add_train_args, dataset_paths, init_args


class CrossCityTrainer(UDATrainer):
    def __init__(self, args, cuda=None, train_id="None", logger=None):
        self._source_validator = None
        super().__init__(args, cuda, train_id, logger)

    def build_dataloader(self):
        """solve_crosscity.py:38-90: the Cityscapes source loader (its val split is validate_source's) and the
        city's loader, self.dataloader, whose val split validate() walks.  The target dataset takes
        target_base_size / target_crop_size as its base / crop size."""
        a = self.args
        g = lambda k: getattr(a, k, None)  # noqa: E731
        root, src_root = g("target_data_path") or g("data_root_path"), g("source_data_path")
        if root is None and src_root is None:
            return Trainer.build_dataloader(self)
        if root is None or src_root is None:
            raise MSLError("file-backed cross-city UDA needs both --source_data_path (Cityscapes) and "
                           "--data_root_path (the NTHU root holding <city_name>/); give both, or neither for the "
                           "synthetic loaders")
        self.file_backed = True
        sargs = copy.copy(a)
        sargs.split = a.source_split
        self.source_loader = build_loader(a.source_dataset, sargs, True, dataset_paths(
            a.source_dataset, src_root, g("source_list_path"), g("source_gt_path")))
        targs = copy.copy(a)
        targs.base_size, targs.crop_size, targs.split = a.target_base_size, a.target_crop_size, "train"
        lists = os.path.join(g("target_list_path") or g("list_path") or root, a.city_name, "List")
        self.dataloader = build_loader("crosscity", targs, True, dataset_paths(
            "crosscity", os.path.join(root, a.city_name), lists, g("target_gt_path")))
        self.source_dataloader, self.target_dataloader = self.source_loader.data_loader, self.dataloader.data_loader
        self._source_items = self._target_items = None

    def validate_source(self):
        """solve_crosscity.py:139, :274 (train_source.py's validate_source): the source's val split through the
        validator, logged and returned as (PA, MPA, MIoU, FWIoU), nothing kept.  None where there is nothing to
        validate on (synthetic items and --val_images 0)."""
        if self._source_validator is None:
            if self.file_backed:
                data = self.source_loader.val_loader
            elif getattr(self.args, "val_images", 0) > 0:
                h, w = self.args.crop_size[1], self.args.crop_size[0]
                data = SyntheticDomain(h, w, self.args.num_classes, self.args.val_images, rank=self.rank,
                                       offset=VAL_OFFSET + 50)
            else:
                return None
            w, h = self.args.crop_size
            self._source_validator = Validator(self.model, self.args.num_classes, (h, w), len(data), self.device,
                                               rank=self.rank, data=data)
        self.logger.info("validating source domain...")
        return val_info(self._source_validator.run(), self.logger, self.current_epoch, "source")

    def main(self):
        """solve_crosscity.py:110-142."""
        if self.args.pretrained_ckpt_file is not None:
            path = self.args.pretrained_ckpt_file
            if os.path.isdir(path):
                path = os.path.join(self.args.checkpoint_dir, self.train_id + "best.pth")
            self.load_checkpoint(path)
        if not self.args.continue_training:
            self.best_MIou = self.best_iter = self.current_iter = self.current_epoch = 0
        else:
            self.load_checkpoint(os.path.join(self.args.checkpoint_dir, self.train_id + "best.pth"))
        self.args.iter_max = self.dataloader.num_iterations * self.args.epoch_num
        self.epoch_num = self.args.epoch_num
        self.optimizer.zero_grad()
        if self.validates():
            self.validate()
        self.validate_source()
        self.train()

    def train_one_epoch(self, epoch=0):
        # this trainer has no rounds: with --threshold_mode class the per-class thresholds are regenerated at
        # the top of every epoch (UDATrainer.generate_thresholds; nothing with `fixed`)
        if getattr(self, "threshold_pass", None) is not None:
            self.generate_thresholds(f"epoch {self.current_epoch}")
        super().train_one_epoch(epoch)
        self.validate_source()  # solve_crosscity.py:273-274


def add_crosscity_args(arg_parser):
    """solve_crosscity.py:276-295 over solve_gta5.py's flags: the defaults that differ, --city_name, --epoch_num."""
    add_UDA_train_args(arg_parser, source_datasets=("cityscapes",))
    arg_parser.set_defaults(num_classes=13, lambda_target=0.1, threshold=0.98)
    arg_parser.add_argument("--city_name", default="Rome", type=str, choices=list(CITIES),
                            help="the NTHU city: the target is <data_root_path>/<city_name>, its lists "
                                 "<list_path>/<city_name>/List")
    arg_parser.add_argument("--epoch_num", type=int, default=10, help="training epochs")
    return arg_parser


def build_parser():
    return add_crosscity_args(add_train_args(argparse.ArgumentParser()))


if __name__ == "__main__":
    args, train_id, logger = init_args(build_parser().parse_args())
    args.target_crop_size, args.target_base_size = args.crop_size, args.base_size  # solve_crosscity.py:312-313
    CrossCityTrainer(args=args, cuda=True, train_id="train_log", logger=logger).main()
