"""Evaluator (tools/evaluate.py of the reference), MI355X path.

Same surface: `Evaluater(args, cuda, train_id, logger)` with `main()`, `validate()` and
`load_checkpoint()`; `validate()` returns (PA, MPA, MIoU, FWIoU) - for 16 classes the 13-class
numbers -, logs the val_info lines and prints the per-class table (evaluate.py:99-202).  Run as

    python -m maxsquareloss_amd.tools.evaluate --pretrained_ckpt_file best.pth --flip True

What runs where (utils/validate.py): the eval-mode forward under torch.no_grad() down to the
low-resolution head logits, then one HIP kernel (msl_predict_up) for upsampling, the class and the
confusion matrix.  --flip (test-time augmentation, evaluate.py:120-135) runs the image and its
mirror through the trunk as one pair and averages the two softmaxes inside that kernel.
--scales 0.75,1.0,1.25 (not in the reference) also averages over input scales: each scale's forward - a flip
pair with --flip - feeds one fusion kernel (msl_predict_tta) that upsamples every low-resolution output
to the label size and sums the softmaxes (utils/validate.py).
--graph True replays the per-image work as a captured hipGraph.  Differences from the reference:
the val set is the val split of --dataset under --data_root_path (datasets/, transformed on the
device), or without a path synthetic (--val_images items at target_crop_size); batch size 1, at most 500;
tensorboard is out.  The reference's image summaries are files here: --save_predictions DIR writes every
item's prediction as PNGs, one sub-directory per --save_kinds entry (color, trainids, labelids,
confidence, pseudo, input; utils/images.py) - the maps come out of that same kernel launch
(msl_predict_images) and are encoded on --data_loader_workers host threads.  --image_summary True is
the reference's cadence: <save_dir>/images, every 20th item and the last.
"""
import argparse
import logging
import os

import torch

from .. import ops
from ..utils.synthetic import init_weights
from ..utils.thresholds import add_parse_check, load_class_thresholds
from ..utils.train_helper import get_model
from ..utils.images import SUMMARY_EVERY, OutputRequest, parse_save_kinds
from ..utils.validate import SINGLE_SCALE, Validator, scales_arg, val_info
from ..datasets import build_loader
from .train_source import add_train_args, dataset_paths, init_args, str2bool


class Evaluater:
    def __init__(self, args, cuda=None, train_id=None, logger=None):
        self.args = args
        self.cuda = bool(cuda) and torch.cuda.is_available()
        if not self.cuda:
            raise RuntimeError("the MI355X evaluator needs a GPU (no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.current_MIoU = self.best_MIou = 0
        self.current_epoch = self.current_iter = 0
        self.train_id = train_id
        self.logger = logger or logging.getLogger(__name__)

        ops.set_conv_math(getattr(args, "conv_math", "fp32"))
        if getattr(args, "f32_form", None):
            ops.set_f32_form(args.f32_form)
        self.model, _ = get_model(args)
        init_weights(self.model, seed=args.seed)
        self.model.to(self.device)

        # evaluate.py:53-62: --pretrained_ckpt_file, else <checkpoint_dir's parent>/<train_id>best.pth
        if args.pretrained_ckpt_file is not None:
            path = args.pretrained_ckpt_file
            if not os.path.exists(path):
                parent = os.path.dirname(str(args.checkpoint_dir or "").rstrip("/"))
                path = os.path.join(parent, str(train_id) + "best.pth")
                if not os.path.exists(path):
                    raise AssertionError("no pretrained_ckpt_file")
            self.load_checkpoint(path)

        self.validator = self.build_validator(args)
        self.Eval = self.validator.Eval
        self.valid_iterations = self.validator.valid_iterations

    def build_validator(self, args):
        w, h = args.target_crop_size
        images = getattr(args, "val_images", 0) or args.synthetic_images
        # evaluate.py:64-79: with --data_root_path the val split of --dataset from files (batch size 1)
        self.dataloader = None
        if getattr(args, "data_root_path", None) is not None:
            self.dataloader = build_loader(args.dataset, args, False, dataset_paths(
                args.dataset, args.data_root_path, args.list_path, getattr(args, "gt_path", None)))
        return Validator(self.model, args.num_classes, (h, w), images, self.device,
                         flip=bool(getattr(args, "flip", False)), graph=bool(getattr(args, "graph", False)),
                         data=self.dataloader.val_loader if self.dataloader else None,
                         outputs=output_request(args), scales=getattr(args, "scales", SINGLE_SCALE))

    def main(self):
        self.logger.info("This model will run on %s", torch.cuda.get_device_name(self.device))
        return self.validate()

    def validate(self):
        self.logger.info("validating one epoch...")
        ev = self.validator.run()
        out = val_info(ev, self.logger, self.current_epoch)
        ev.Print_Every_class_Eval()
        return out

    def load_checkpoint(self, filename):
        """evaluate.py:205-220: {'state_dict': ...} or a bare state dict ('module.' prefixes accepted);
        a missing file is logged and skipped.  Read as data only (torch.load(weights_only=True))."""
        try:
            self.logger.info("Loading checkpoint '%s'", filename)
            ckpt = torch.load(filename, map_location=self.device, weights_only=True)
        except OSError:
            self.logger.info("No checkpoint exists from '%s'. Skipping...", filename)
            return
        sd = ckpt["state_dict"] if "state_dict" in ckpt else ckpt
        self.model.load_state_dict({k[7:] if k.startswith("module.") else k: v for k, v in sd.items()})
        self.logger.info("Checkpoint loaded successfully from %s", filename)
        if "crop_size" in ckpt:
            self.args.crop_size = ckpt["crop_size"]


def output_request(args, out_size=None):
    """The OutputRequest of --save_predictions / --save_kinds / --threshold / --image_summary; None
    without either flag (today's runs)."""
    directory, every = getattr(args, "save_predictions", None), None
    if directory is None and getattr(args, "image_summary", False):
        directory, every = os.path.join(str(args.save_dir), "images"), SUMMARY_EVERY
    if directory is None:
        return None
    values = getattr(args, "class_threshold_values", None)
    if values is None and getattr(args, "class_thresholds", None) is not None:  # a namespace built by hand
        values = load_class_thresholds(args.class_thresholds, args.num_classes)
    return OutputRequest(directory, getattr(args, "save_kinds", ("color",)), getattr(args, "threshold", 0.95),
                         getattr(args, "data_loader_workers", 0), out_size=out_size, every=every,
                         class_thresholds=values)


def add_scales_arg(parser):
    parser.add_argument("--scales", type=scales_arg, default=SINGLE_SCALE, metavar="S[,S...]",
                        help="average the softmax over these input scales, each with its mirror under --flip: 1 to 8 "
                             "values in [0.25, 2.0], e.g. 0.75,1.0,1.25 (default 1.0: off; not in the reference)")
    return parser


def add_save_args(parser):
    a = parser.add_argument
    a("--save_predictions", type=str, default=None, metavar="DIR",
      help="write every item's prediction as PNGs under DIR, one sub-directory per kind (not in the reference)")
    a("--save_kinds", type=parse_save_kinds, default=("color",),
      help="comma-separated: color,trainids,labelids,confidence,pseudo,input (default color)")
    if not any("--threshold" in act.option_strings for act in parser._actions):
        a("--threshold", type=float, default=0.95, help="the pseudo kind keeps a class where its probability > this")
    a("--class_thresholds", type=str, default=None, metavar="FILE",
      help="a class_thresholds.json of tools/pseudo_thresholds.py: the pseudo kind then keeps a class where its "
           "probability > that class's own threshold (one more launch, msl_pseudo_classwise; not in the reference)")
    add_parse_check(parser, read_class_thresholds)
    return parser


def read_class_thresholds(ns):
    """--class_thresholds against --num_classes, known only once both are parsed (a parser error through
    utils/thresholds.py add_parse_check); the values go to ns.class_threshold_values."""
    ns.class_threshold_values = None
    if ns.class_thresholds is not None:
        ns.class_threshold_values = load_class_thresholds(ns.class_thresholds, ns.num_classes)


def build_parser():
    parser = add_train_args(argparse.ArgumentParser())  # --val_images is one of the train flags
    parser.add_argument("--flip", type=str2bool, default=False,
                        help="average the softmax of the image and of its horizontal mirror (evaluate.py:120-135)")
    parser.add_argument("--graph", type=str2bool, default=False,
                        help="replay each image after the first as one captured hipGraph (not in the reference)")
    add_scales_arg(parser)
    add_save_args(parser)
    parser.add_argument("--image_summary", type=str2bool, default=False,
                        help="the reference's image summaries as files: --save_predictions <save_dir>/images for "
                             "every 20th item and the last")
    return parser


def parse_args(argv=None):
    """evaluate.py:237-249: the val split, checkpoint_dir "none", crop = the target crop."""
    args = build_parser().parse_args(argv)
    if "train" in args.split:
        args.split = "val"
    if args.checkpoint_dir == "none":
        args.checkpoint_dir = str(args.pretrained_ckpt_file) + "/eval"
    args, train_id, logger = init_args(args)
    args.crop_size = args.target_crop_size
    args.base_size = args.target_base_size
    return args, train_id, logger


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    args, train_id, logger = parse_args()
    Evaluater(args=args, cuda=True, train_id=train_id, logger=logger).main()
