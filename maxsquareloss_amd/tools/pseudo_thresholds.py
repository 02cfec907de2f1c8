"""Class-balanced pseudo-label thresholds of a model over unlabelled images, as a tool - the statistics pass
the UDA trainer runs at the top of every round with --threshold_mode class (utils/thresholds.py), MI355X path.

    python -m maxsquareloss_amd.tools.pseudo_thresholds --list_path lists/ --pretrained_ckpt_file best.pth \\
        --flip True --pseudo_portion 0.5 --threshold 0.9 --save_dir out/
    python -m maxsquareloss_amd.tools.predict --list_path lists/ --pretrained_ckpt_file best.pth --flip True \\
        --save_predictions labels/ --save_kinds pseudo --class_thresholds out/class_thresholds.json

Built on the evaluator's parser like tools/predict.py: `<list_path>/test.txt` holds one image path per line;
without --list_path the tool runs on --val_images (or --synthetic_images) synthetic items.  Per image: the
eval-mode forward down to the low-resolution logits - the image and its mirror with --flip, every input scale
with --scales - then one kernel (msl_confidence_hist, msl_confidence_hist_tta with --scales) that upsamples,
takes the class and its winning probability exactly as the prediction kernels do, and counts the pair into a
[class][bin] histogram on the device; --graph True replays that body as a captured hipGraph.  One launch
(msl_class_thresholds) then gives every class the largest bin edge that still keeps --pseudo_portion of its
pixels, capped at --threshold.  Writes <save_dir>/class_thresholds.json (per class: name, pixels, share,
quantile, threshold, kept share; plus bins, portion, thr_max) and <save_dir>/confidence_hist.npy.
"""
import argparse
import logging

from ..datasets import Client_dataset, DeviceLoader
from ..hip import MSLError
from ..utils.images import parse_size
from ..utils.synthetic import SyntheticDomain
from ..utils.thresholds import ThresholdPass, add_parse_check, check_pass_flags
from ..utils.validate import SINGLE_SCALE, VAL_OFFSET
from .evaluate import Evaluater, add_scales_arg
from .train_source import add_train_args, init_args, str2bool


class ThresholdTool(Evaluater):
    def build_validator(self, args):
        """The evaluator builds its Validator here; this tool builds the statistics pass and its items, and
        hands the evaluator an object with the two attributes it reads."""
        w, h = args.target_crop_size
        self.dataloader = None
        if getattr(args, "list_path", None) is not None:
            self.dataloader = DeviceLoader(Client_dataset({"list_path": args.list_path}, args), shuffle=False,
                                           workers=getattr(args, "data_loader_workers", 0), seed=args.seed)
            self.items = self.dataloader
        else:
            images = getattr(args, "val_images", 0) or args.synthetic_images
            self.items = SyntheticDomain(h, w, args.num_classes, images, offset=VAL_OFFSET)
        n = len(self.items) if args.threshold_images <= 0 else min(args.threshold_images, len(self.items))
        self.passes = ThresholdPass(self.model, args.num_classes, args.threshold_bins, self.device,
                                    portion=args.pseudo_portion, thr_max=args.threshold, flip=bool(args.flip),
                                    scales=getattr(args, "scales", SINGLE_SCALE), graph=bool(args.graph))
        self.passes.valid_iterations, self.passes.Eval = n, None
        return self.passes

    def main(self):
        n = self.valid_iterations
        items = self.items
        walk = (items[i] for i in range(n)) if isinstance(items, SyntheticDomain) else \
            (item for _, item in zip(range(n), items))
        self.passes.run(walk)
        self.passes.log(self.logger)
        if not self.args.save_dir:
            raise MSLError("tools/pseudo_thresholds.py writes its result: give --save_dir DIR")
        path = self.passes.save(self.args.save_dir)
        self.logger.info("wrote %s", path)
        if self.dataloader is not None:
            self.dataloader.close()
        return path


def build_parser():
    parser = add_train_args(argparse.ArgumentParser())
    a = parser.add_argument
    a("--flip", type=str2bool, default=False, help="average the softmax of the image and of its horizontal mirror")
    a("--graph", type=str2bool, default=False, help="replay each image after the first as one captured hipGraph")
    add_scales_arg(parser)
    a("--threshold", type=float, default=0.95, help="the cap of the per-class thresholds (BDL: 0.9)")
    a("--pseudo_portion", type=float, default=0.5,
      help="the share of each class's pixels its threshold keeps at least")
    a("--threshold_bins", type=int, default=512,
      help="bins of the confidence histogram, a power of two in [16, 1024]")
    a("--threshold_images", type=int, default=0, help="use the first N images of the list (0 = all of it)")
    return add_parse_check(parser, check_pass_flags)


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    if args.checkpoint_dir == "none":
        args.checkpoint_dir = str(args.pretrained_ckpt_file) + "/eval"
    if isinstance(args.seg_size, str):
        args.seg_size = parse_size(args.seg_size)
    args, train_id, logger = init_args(args)
    args.crop_size = args.target_crop_size
    args.base_size = args.target_base_size
    return args, train_id, logger


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    args, train_id, logger = parse_args()
    ThresholdTool(args=args, cuda=True, train_id=train_id, logger=logger).main()
