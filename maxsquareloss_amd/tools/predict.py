"""Predict on unlabelled images and write the predictions as PNGs - the reference's --client path
(Client_dataset + validate_client) as a tool, MI355X path.

    python -m maxsquareloss_amd.tools.predict --list_path lists/ --pretrained_ckpt_file best.pth \\
        --flip True --save_predictions out/ --save_kinds color,labelids --out_size 2048,1024

`<list_path>/test.txt` holds one image path per line (datasets/ Client_dataset: decoded on
--data_loader_workers threads, with --resize resized to --seg_size on the device, byte-exact against
Pillow).  Per image: the eval-mode forward down to the low-resolution logits, then one kernel
(msl_predict_images) that upsamples, takes the class - with --flip of the averaged softmaxes - and writes
it as the --save_kinds maps; PNG encoding overlaps the next image.  --graph True replays that body as a
captured hipGraph.  --scales 0.5,1.0 (not in the reference) averages the softmax over those input scales as
tools/evaluate.py does, in one fusion kernel (msl_predict_tta_images) that upsamples every scale's output
straight to the size written.  --out_size W,H (not in the reference) upsamples the low-resolution logits straight to
that size - 2048,1024 for a Cityscapes submission - instead of the input's; it exists only here, where no
label has to match.  Without --list_path the tool runs on --val_images (or --synthetic_images) synthetic
items at target_crop_size, like every other tool, and names the files by index.
"""
import argparse
import logging

from ..datasets import Client_dataset, DeviceLoader
from ..hip import MSLError
from ..utils.images import parse_size
from ..utils.validate import SINGLE_SCALE, Validator
from .evaluate import Evaluater, add_save_args, add_scales_arg, output_request
from .train_source import add_train_args, init_args, str2bool


class Predictor(Evaluater):
    def build_validator(self, args):
        w, h = args.target_crop_size
        images = getattr(args, "val_images", 0) or args.synthetic_images
        outputs = output_request(args, out_size=getattr(args, "out_size", None))
        if outputs is None:
            raise MSLError("tools/predict.py writes predictions: give --save_predictions DIR")
        self.dataloader = None
        if getattr(args, "list_path", None) is not None:
            self.dataloader = DeviceLoader(Client_dataset({"list_path": args.list_path}, args), shuffle=False,
                                           workers=getattr(args, "data_loader_workers", 0), seed=args.seed)
        return Validator(self.model, args.num_classes, (h, w), images, self.device, flip=bool(args.flip),
                         graph=bool(args.graph), data=self.dataloader, outputs=outputs, labelled=False,
                         scales=getattr(args, "scales", SINGLE_SCALE))

    def main(self):
        self.validator.run()
        self.logger.info("wrote %d predictions (%s) under %s", self.valid_iterations,
                         ",".join(self.validator.outputs.kinds), self.validator.outputs.directory)
        if self.dataloader is not None:
            self.dataloader.close()


def build_parser():
    parser = add_train_args(argparse.ArgumentParser())
    parser.add_argument("--flip", type=str2bool, default=False,
                        help="average the softmax of the image and of its horizontal mirror")
    parser.add_argument("--graph", type=str2bool, default=False,
                        help="replay each image after the first as one captured hipGraph")
    add_scales_arg(parser)
    add_save_args(parser)
    parser.add_argument("--out_size", type=parse_size, default=None, metavar="W,H",
                        help="upsample the prediction to this size instead of the input's")
    return parser


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
    Predictor(args=args, cuda=True, train_id=train_id, logger=logger).main()
