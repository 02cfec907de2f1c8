"""AdaIN domain adaptation inside the MaxSquare training loop (tools/ADAIN.py of the reference, with the --DA,
--crop_trans and --rectification branches of its tools/train_source.py), MI355X path.

    python -m maxsquareloss_amd.tools.ADAIN --source_data_path datasets/GTA5 --target_data_path datasets/Cityscapes \\
        --target_list_path datasets/city_list --vgg vgg_normalised.pth --decoder decoder.pth --style styles/ \\
        --base_size 1280,720 --target_base_size 1280,640 --seg_size 1280,640 --graph True

One iteration: the source and the target item - uint8 RGB at base_size / target_base_size - are stylised
toward a fixed set of style images (tools/net.StyleNet, the statistics of the styles encoded once), turned
into the segmentation network's input at seg_size (utils/style_transform.stylise_for_seg; with --crop_trans
crop_trans: each quadrant magnified, stylised and stitched back), and solve_gta5's uda_step runs on that:
every --target_mode, --multi, --pair, --optim, data parallel.  No torch op touches an image-sized tensor
between the decoded item and the step.  With --graph True the style passes run eagerly on the stream the
step replays on and write straight into the captured step's static inputs.

The learning rate is the reference's: no poly schedule, ReduceLROnPlateau(mode='min', factor=0.9,
patience=3) stepped once per epoch on the mean source loss (ReduceLROnPlateau below, over the optimizer's
param_groups; a captured step reads its rates from device memory, so a reduction needs no new capture).

Validation stylises its items the same way (StylisedItems around the val loader, handed to the Validator);
validate_source walks the source's val split after every epoch.  With --rectification each target val image
also sends two half-size crops (x0 = 0 and W0 / 2, y0 drawn per image) magnified through the style network
and the model, and one kernel (ops.predict_rectify) takes the class, rectifies it and counts it.

The style network's weights and the style images are flags (--vgg, --decoder, --style): nothing has a default
path and nothing is downloaded.  Out of scope: the reference's tensorboard images (--val_save_predictions
writes the predictions as files instead), train_trans_only.py, the style network's training, coral,
analysis.py, and capturing the style pass itself.
"""
import argparse
import os
import random

import torch

from ..hip import MSLError
from ..utils import style_transform as st
from ..utils.eval import Eval
from ..utils.synthetic import IMG_MEAN
from ..utils.validate import Validator, val_info
from . import solve_gta5
from .stylize import IMAGE_EXTS, load_image, load_net
from .train_source import add_train_args, init_args


class ReduceLROnPlateau:
    """torch.optim.lr_scheduler.ReduceLROnPlateau(mode='min', threshold_mode='rel', cooldown=0, min_lr=0) over
    anything with param_groups: after more than `patience` epochs in a row without a metric below
    best * (1 - threshold), every group's lr is multiplied by `factor` (unless that changes it by less than
    eps) and the count restarts."""

    def __init__(self, optimizer, factor=0.9, patience=3, threshold=1e-4, eps=1e-8):
        if not 0.0 < factor < 1.0:
            raise ValueError("factor must lie in (0, 1)")
        self.optimizer, self.factor, self.patience, self.threshold, self.eps = optimizer, factor, patience, threshold, eps
        self.best = float("inf")
        self.num_bad_epochs = 0
        self.last_epoch = 0

    def step(self, metric):
        current = float(metric)
        self.last_epoch += 1
        if current < self.best * (1.0 - self.threshold):
            self.best = current
            self.num_bad_epochs = 0
        else:
            self.num_bad_epochs += 1
        if self.num_bad_epochs > self.patience:
            for g in self.optimizer.param_groups:
                old = float(g["lr"])
                new = max(old * self.factor, 0.0)
                if old - new > self.eps:
                    g["lr"] = new
            self.num_bad_epochs = 0


class StylisedItems:
    """A val loader's items as the segmentation network's input: (image (1,3,Hs,Ws), label at that size, id),
    stylised one by one as they are drawn.  Sized and re-iterable, as the Validator needs its data."""

    def __init__(self, loader, transform):
        self.loader, self.transform = loader, transform
        self.dataset = getattr(loader, "dataset", None)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for content, label, ident in self.loader:
            x, y = self.transform(content, label)
            yield x, y, ident


def _pair(v, name):
    if isinstance(v, str):
        parts = v.split(",")
        if len(parts) != 2:
            raise MSLError(f"--{name} takes W,H, got {v!r}")
        return int(parts[0]), int(parts[1])
    return int(v[0]), int(v[1])


def style_files(paths):
    """--style as files: the files themselves, or the image files of one directory in sorted order, the first
    four (the reference takes one batch of four from a folder)."""
    if len(paths) == 1 and os.path.isdir(paths[0]):
        names = sorted(n for n in os.listdir(paths[0]) if n.lower().endswith(IMAGE_EXTS))
        paths = [os.path.join(paths[0], n) for n in names[:4]]
    if not paths:
        raise MSLError("--style: no style images found")
    return list(paths)


def check_sizes(args):
    """The sizes the loop cannot run, refused before anything is built or launched."""
    seg, base, tbase, crop = args.seg_size, args.base_size, args.target_base_size, args.crop_size
    if args.crop_trans and (base[0] != 2 * crop[0] or base[1] != 2 * crop[1]):
        raise MSLError(f"--crop_trans: base_size {base} must be twice crop_size {crop} (the quadrants are magnified "
                       "to base_size; the reference asserts it)")
    if args.crop_trans and tuple(tbase) != tuple(base):
        raise MSLError(f"--crop_trans: target_base_size {tbase} must equal base_size {base} (the target's quadrants "
                       "are crop_size too)")
    for name, size in (("base_size", base), ("target_base_size", tbase)):
        if tuple(seg) == tuple(size) and (size[0] % 8 or size[1] % 8) and not args.crop_trans:
            raise MSLError(f"--{name} {size} equals seg_size but is no multiple of 8: the style network returns its "
                           "input rounded up to a multiple of 8 and nothing resizes it (the reference fails at the loss)")
    if args.rectification and (tbase[0] % 2 or tbase[1] % 2 or seg[0] % 2 or seg[1] % 2):
        raise MSLError(f"--rectification halves target_base_size {tbase} and seg_size {seg}: both must be even")


class UDATrainer(solve_gta5.UDATrainer):
    def __init__(self, args, cuda=None, train_id="None", logger=None):
        args.DA = True  # the datasets resize to base_size (not seg_size) and deliver RGB bytes
        args.seg_size = _pair(args.seg_size, "seg_size")
        check_sizes(args)
        if not args.vgg or not args.decoder or not args.style:
            raise MSLError("tools/ADAIN.py needs --vgg, --decoder and --style: the style network has no default "
                           "weights or images and nothing is downloaded")
        super().__init__(args, cuda, train_id, logger)
        if not self.file_backed:
            raise MSLError("tools/ADAIN.py stylises decoded images: give --source_data_path and --target_data_path")
        for loader in (self.source_loader, self.dataloader):
            for dl in (loader.data_loader, loader.val_loader):
                dl.dataset.deliver_uint8 = True
        self.network = load_net(args, self.device)
        files = style_files(args.style)
        weights = getattr(args, "weights", None)
        if weights is None:
            weights = [1.0 / len(files)] * len(files)
        if len(weights) != len(files):
            raise MSLError(f"{len(files)} style images but {len(weights)} interpolation weights")
        self.style_weights = tuple(float(w) for w in weights)
        with torch.no_grad():
            styles = [torch.from_numpy(load_image(p, args.base_size)) for p in files]
            self.style_stats = self.network.encode_style(styles)
        self.scheduler = ReduceLROnPlateau(self.optimizer, factor=0.9, patience=3)
        self.rect_rng = random.Random(args.seed)  # the y0 of --rectification, one draw per val image
        self.rect_draws = []                      # the last validation's draws, in item order
        self.rect_eval = None
        self._source_validator = None

    # ---------------------------------------------------------------- content -> segmentation input
    def poly_lr_scheduler(self, optimizer, init_lr=None, iter=None, max_iter=None, power=None):
        """The reference's ADAIN.py never calls it: the rates move only when the plateau scheduler moves them."""

    def seg_input(self, content, label=None, out=None, window=None):
        """A decoded item (uint8 (H, W, 3) RGB on the device) as the segmentation network's input at seg_size,
        with its label resized along: the style network or, with --crop_trans, cropTrans, then seg_transform.
        `window` (x0, y0, cw, ch) takes that part magnified to the item's size (rectification's crops, which
        never go through cropTrans).  `out`: a (1, 3, Hs, Ws) tensor to fill."""
        a = self.args
        kw = dict(alpha=a.alpha, weights=self.style_weights, mean=IMG_MEAN, out=out)
        with torch.no_grad():
            if a.crop_trans and window is None:
                x = st.crop_trans(self.network, content, self.style_stats, a.crop_size, a.base_size, a.seg_size, **kw)
            else:
                size = None if window is None else (content.size(0), content.size(1))
                x = st.stylise_for_seg(self.network, content, self.style_stats, a.seg_size, window=window, size=size,
                                       **kw)
            y = st._resize_label(label, tuple(x.shape[-2:]))
        return x, y

    # ---------------------------------------------------------------- loop
    def train_one_epoch(self, epoch=0):
        self.model.eval() if self.args.freeze_bn else self.model.train()
        self.iter_num = self.dataloader.num_iterations
        self.Eval.reset()
        self._reset_meters()
        if self._source_items is None:
            self._source_items, self._target_items = self.source_dataloader.cycle(), self.target_dataloader.cycle()
        for _ in range(self.iter_num):
            c_s, y_s, _ = next(self._source_items)
            c_t, _, _ = next(self._target_items)
            # a captured step's static inputs, once they exist: the style passes fill them in place
            static = self._graphed.static if self._graphed is not None and self._graphed.static else (None,) * 3
            x_s, y_s = self.seg_input(c_s, y_s, out=static[0])
            x_t, _ = self.seg_input(c_t, out=static[2])
            self.uda_step(x_s, y_s.to(dtype=torch.long), x_t)
        loss = float(self.loss_seg_value)
        if loss != loss:
            raise ValueError("Loss is nan during training...")
        self.scheduler.step(loss)
        self.logger.info("epoch %d: source loss %.6f target loss %.6f lr %s", self.current_epoch, loss,
                         float(self.loss_target_value), self.optimizer.group_lrs())
        self.validate_source(epoch)

    # ---------------------------------------------------------------- validation
    def val_data(self):
        return StylisedItems(self.dataloader.val_loader, self.seg_input)

    def validate(self, epoch=None):
        if not self.args.rectification:
            return super().validate(epoch)
        return self._validate_rectified(self.current_epoch if epoch is None else epoch)

    def _validate_rectified(self, epoch):
        """train_source.py:420-553 of the reference with --rectification: per target val image the stylised
        image and its two stylised, magnified crops through the model, then ops.predict_rectify."""
        a = self.args
        if self.rect_eval is None:
            self.rect_eval = Eval(a.num_classes)
        ev = self.rect_eval
        ev.reset()
        self.rect_draws = []
        self.model.eval()
        ws, hs = a.seg_size
        with torch.no_grad():
            for content, label, _ in self.dataloader.val_loader:
                h0, w0 = content.size(0), content.size(1)
                x, y = self.seg_input(content, label)
                low = self.model.predict_low(x)[0]
                y0 = self.rect_rng.randint(int(0.083 * h0), int(0.25 * h0))
                self.rect_draws.append(y0)
                crops = []
                for x0 in (0, int(0.5 * w0)):
                    xc, _ = self.seg_input(content, window=(x0, y0, w0 // 2, h0 // 2))
                    crops.append(self.model.predict_low(xc)[0])
                ev.add_batch_rectified(y, low, crops[0], crops[1], (hs, ws), int((y0 / h0) * hs))
        out = val_info(ev, self.logger, epoch)
        ev.Print_Every_class_Eval()
        return out

    def validate_source(self, epoch=None):
        """train_source.py:554-650 of the reference: the source's val split, stylised like the training items."""
        if self._source_validator is None:
            w, h = self.args.seg_size
            self._source_validator = Validator(self.model, self.args.num_classes, (h, w), 0, self.device, rank=self.rank,
                                               data=StylisedItems(self.source_loader.val_loader, self.seg_input))
        self.logger.info("validating source domain...")
        ev = self._source_validator.run()
        return val_info(ev, self.logger, self.current_epoch if epoch is None else epoch, name="source")


def add_UDA_train_args(arg_parser):
    """The reference's add_UDA_train_args (tools/ADAIN.py:386-411, its defaults) over solve_gta5's, and the
    style network's flags, which the reference hard-codes."""
    solve_gta5.add_UDA_train_args(arg_parser)
    arg_parser.set_defaults(round_num=40, target_mode="IW_maxsquare", lambda_target=0.09)
    a = arg_parser.add_argument
    a("--adain_lr", type=float, default=1e-4, help="accepted and unused, as in the reference")
    a("--vgg", default=None, help="the style encoder's state dict (vgg_normalised.pth); required")
    a("--decoder", default=None, help="the style decoder's state dict or training checkpoint; required")
    a("--style", nargs="+", default=None,
      help="the style images: files, or one directory whose first four image files in sorted order are used; required")
    a("--style_interpolation_weight", default="", help="one number per style, e.g. 1,1,2 (normalised); default equal")
    a("--alpha", type=float, default=1.0, help="stylisation strength in [0, 1]")
    return arg_parser


def build_parser():
    return add_UDA_train_args(add_train_args(argparse.ArgumentParser()))


def parse_args(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if not args.vgg or not args.decoder:
        parser.error("--vgg and --decoder are required: the style network has no default weights and nothing is "
                     "downloaded")
    if not args.style:
        parser.error("--style is required")
    if not 0.0 <= args.alpha <= 1.0:
        parser.error("--alpha must lie in [0, 1]")
    args.weights = None
    if args.style_interpolation_weight:
        try:
            raw = [float(v) for v in args.style_interpolation_weight.split(",")]
        except ValueError:
            parser.error("--style_interpolation_weight takes numbers separated by commas")
        if sum(raw) <= 0 or min(raw) < 0:
            parser.error("--style_interpolation_weight needs non-negative numbers with a positive sum")
        args.weights = [v / sum(raw) for v in raw]
    try:
        args.seg_size = _pair(args.seg_size, "seg_size")
    except (MSLError, ValueError) as e:
        parser.error(str(e))
    return args


if __name__ == "__main__":
    args, train_id, logger = init_args(parse_args())
    args.target_dataset = args.dataset
    train_id = str(args.source_dataset) + "2" + str(args.target_dataset) + "_" + args.target_mode
    UDATrainer(args=args, cuda=True, train_id=train_id, logger=logger).main()
