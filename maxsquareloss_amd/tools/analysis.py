"""Per-image analysis (tools/analysis.py of the reference), MI355X path.

Same surface: `resultEvaluater(args, cuda, train_id, logger)` with `main()` and
`getvalResult(outputPath, threshold)`, which walks the val set, scores every image on its own (PA, MPA, MIoU,
FWIoU), saves the label, the prediction and the input of every image whose MIoU is below the threshold under
<save_dir>/savePics - named with the scores - and returns the reference's id2mIOU list.  Run as

    python -m maxsquareloss_amd.tools.analysis --pretrained_ckpt_file best.pth --graph True

What runs where (utils/analysis.py): the evaluator's forward and prediction kernel per image, then two small
launches - msl_image_metrics takes the image's scores and the save / don't-save decision on the device,
msl_analysis_maps writes the pictures of a selected image into a ring of device buffers and returns at once
for the others.  The host reads the scores once every --ring images.  The parser is tools/evaluate.py's (the
data paths, --flip, --scales, --graph, --data_loader_workers for the PNG threads; synthetic items without a
path) plus --miou_threshold, --analysis_kinds, --ring and --worst; the evaluator's --save_predictions and
--image_summary are refused here (--save_kinds and --threshold go with them and have no effect).  <save_dir>/per_image.csv holds every
image's row.

Differences from the reference: no nn.DataParallel (one device); style_img is the exact recovered input, not
the min-max-normalised one; its decode_labels unpacking bug and its hard-coded dataset path table are not
reproduced (the paths are the evaluator's flags); error_img (--analysis_kinds ...,error) is new.
"""
import logging
import os

from ..utils.analysis import (DEFAULT_KINDS, MIOU_THRESHOLD, RING_DEFAULT, SAVE_SUBDIR, Analyzer, parse_kinds,
                              ring_arg)
from ..utils.validate import SINGLE_SCALE
from ..datasets import build_loader
from . import evaluate
from .train_source import dataset_paths, init_args


class resultEvaluater(evaluate.Evaluater):
    def __init__(self, args, cuda=None, train_id=None, logger=None):
        super().__init__(args, cuda=cuda, train_id=train_id, logger=logger)
        self.totalEval = self.validator.totalEval
        self.resultOutPath = os.path.join(str(args.save_dir), SAVE_SUBDIR)

    def build_validator(self, args):
        """The Evaluater's data and options, as an Analyzer."""
        w, h = args.target_crop_size
        images = getattr(args, "val_images", 0) or args.synthetic_images
        self.dataloader = None
        if getattr(args, "data_root_path", None) is not None:
            self.dataloader = build_loader(args.dataset, args, False, dataset_paths(
                args.dataset, args.data_root_path, args.list_path, getattr(args, "gt_path", None)))
        return Analyzer(self.model, args.num_classes, (h, w), images, self.device, str(args.save_dir),
                        flip=bool(getattr(args, "flip", False)), scales=getattr(args, "scales", SINGLE_SCALE),
                        graph=bool(getattr(args, "graph", False)),
                        data=self.dataloader.val_loader if self.dataloader else None,
                        threshold=getattr(args, "miou_threshold", MIOU_THRESHOLD),
                        kinds=getattr(args, "analysis_kinds", DEFAULT_KINDS),
                        ring=getattr(args, "ring", RING_DEFAULT), workers=getattr(args, "data_loader_workers", 0))

    def main(self):
        import torch
        self.logger.info("This model will run on %s", torch.cuda.get_device_name(self.device))
        rows = self.getvalResult(self.resultOutPath, getattr(self.args, "miou_threshold", MIOU_THRESHOLD))
        n = int(getattr(self.args, "worst", 0) or 0)
        if n:
            print(f"##### the {min(n, len(rows))} images of lowest MIoU #####")
            for ident, PA, MPA, MIoU, FWIoU in self.validator.worst(n):
                print(ident, PA, MPA, MIoU, FWIoU)
        return rows

    def validate(self):
        """The Evaluater's surface: the analysis run, then the whole set's (PA, MPA, MIoU, FWIoU)."""
        self.getvalResult(self.resultOutPath, getattr(self.args, "miou_threshold", MIOU_THRESHOLD))
        return self.validator.total_scores()

    def getvalResult(self, outputPath, threshold):
        """tools/analysis.py:171-240: [(id, PA, MPA, MIoU, FWIoU)] over the val items; the pictures of the
        images below `threshold` go to `outputPath`."""
        self.logger.info('\nget result one epoch...')
        a = self.validator
        if float(threshold) != a.threshold:  # the captured graph holds the threshold of its capture
            a.threshold, a._graph = float(threshold), None
        a.out_dir = str(outputPath)
        return a.run()


def build_parser():
    parser = evaluate.build_parser()
    a = parser.add_argument
    a("--miou_threshold", type=float, default=MIOU_THRESHOLD,
      help="save the pictures of every image whose MIoU is strictly below this (the reference's constant 0.5)")
    a("--analysis_kinds", type=parse_kinds, default=DEFAULT_KINDS,
      help="comma-separated: label,pred,style,error (default label,pred,style: the reference's three)")
    a("--ring", type=ring_arg, default=RING_DEFAULT,
      help="images between two looks of the host at the device's scores, 1 to 64 (default 8)")
    a("--worst", type=int, default=0, metavar="N", help="also print the N rows of lowest MIoU")
    return parser


def parse_args(argv=None):
    """tools/evaluate.py's: the val split, checkpoint_dir "none", crop = the target crop."""
    parser = build_parser()
    args = parser.parse_args(argv)
    # the evaluator's own picture flags write every item's prediction: this tool writes the failures' pictures
    if args.save_predictions is not None or args.image_summary:
        parser.error("--save_predictions / --image_summary are the evaluator's (tools/evaluate.py); the analysis "
                     "writes <save_dir>/savePics, chosen by --miou_threshold and --analysis_kinds")
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
    resultEvaluater(args=args, cuda=True, train_id=train_id, logger=logger).main()
