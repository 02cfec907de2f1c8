"""Class-balanced pseudo-label thresholds (--threshold_mode class; CBST's class-balanced thresholds, BDL's
"median confidence per class, capped at 0.9"; the reference's train_round() has the place - "# generate
threshold" - and assigns the constant).

A statistics pass walks target images through the eval-mode forward down to the low-resolution logits and
counts every pixel's (class, confidence bin) pair on the device (ops.confidence_hist, msl_confidence_hist: the
class and the winning probability of the evaluator's prediction kernels, the upsampled probabilities never
written).  One launch (ops.class_thresholds) then takes, per class, the largest bin edge that still keeps
`portion` of the class's pixels at or above it, capped at `thr_max`.  Nothing crosses to the host until the
table is read for the log.  The trainer (tools/solve_gta5.py) runs the pass at the top of every round; the
tool (tools/pseudo_thresholds.py) writes the result to a file that tools/predict.py and tools/evaluate.py take
as --class_thresholds.
"""
import json
import os

import numpy as np
import torch

from .. import ops
from ..hip import MSLError
from .eval import name_classes, synthia_set_13, synthia_set_16
from .validate import SINGLE_SCALE, GraphedPredict, parse_scales, tta_entries

FILE_NAME = "class_thresholds.json"
HIST_NAME = "confidence_hist.npy"


def check_bins(bins, num_classes):
    """msl_confidence_hist's size rule (hist_ok, csrc/predict.hip), the one statement of it in Python."""
    bins = int(bins)
    if bins < 16 or bins > 1024 or bins & (bins - 1) or int(num_classes) * bins > 16384:
        raise MSLError(f"--threshold_bins {bins} must be a power of two in [16, 1024] with num_classes * bins <= "
                       "16384")
    return bins


def check_pass(bins, num_classes, portion, thr_max):
    """The arguments of a statistics pass: (bins, portion, thr_max) checked, or an MSLError naming the flag."""
    bins, portion, thr_max = check_bins(bins, num_classes), float(portion), float(thr_max)
    if not 0.0 <= portion <= 1.0:
        raise MSLError(f"--pseudo_portion {portion} must lie in [0, 1]")
    if not 0.0 < thr_max <= 1.0:
        raise MSLError(f"--threshold {thr_max} must lie in (0, 1]: it caps the class thresholds")
    return bins, portion, thr_max


def check_pass_flags(ns):
    """check_pass on a parsed namespace (--threshold_bins, --num_classes, --pseudo_portion, --threshold)."""
    check_pass(ns.threshold_bins, ns.num_classes, ns.pseudo_portion, ns.threshold)


def add_parse_check(parser, check):
    """Have `parser` run check(namespace) after every parse and report an MSLError it raises as a parser error:
    for what only several parsed flags together can tell.  One hook per parser, however many checks are added:
    parse_args goes through parse_known_args, which is wrapped once and walks the parser's list."""
    checks = getattr(parser, "_msl_checks", None)
    if checks is None:
        checks = parser._msl_checks = []
        inner = parser.parse_known_args

        def parse_known_args(args=None, namespace=None):
            ns, rest = inner(args, namespace)
            for c in checks:
                try:
                    c(ns)
                except MSLError as e:
                    parser.error(str(e))
            return ns, rest

        parser.parse_known_args = parse_known_args
    checks.append(check)
    return parser


def pass_loader(train_loader, seed=12345):
    """A loader of a training loader's own list for the statistics pass: the dataset copied with the val
    transform (resize only: no mirror, no crop; the network input, not tools/ADAIN.py's uint8), a random
    stream of its own and the list order.  The training loader, its dataset's random stream and its epoch
    counter are not touched."""
    import copy
    import random
    from ..datasets import DeviceLoader
    ds = copy.copy(train_loader.dataset)
    ds.training, ds.random_mirror, ds.random_crop = False, False, False
    ds.deliver_uint8 = False
    ds.rng = random.Random(seed)
    if hasattr(ds, "labelled"):
        # an NTHU city's train list has no labels and its dataset decides that from `training`
        # (datasets/crosscity_Dataset.py labelled()): the copy reads the files the training dataset reads
        has_labels = bool(train_loader.dataset.labelled())
        ds.labelled = lambda: has_labels
    return DeviceLoader(ds, shuffle=False, workers=train_loader.workers, seed=train_loader.seed)


def first_items(loader, n):
    """The first n items of a loader (n <= 0: all of them)."""
    n = len(loader) if n <= 0 else min(int(n), len(loader))
    return (item for _, item in zip(range(n), loader))


def confidence_image(model, hist, x, hw, flip=False, scales=SINGLE_SCALE):
    """One image into the histogram: x (1,3,H,W) fp32 on the device, hw the size the prediction is upsampled
    to; the source - single scale, --flip, --scales - is utils/validate.py predict_image's."""
    if tuple(scales) != SINGLE_SCALE:
        return ops.confidence_hist(hist, hw, entries=tta_entries(model, x, scales, flip))
    if flip:
        (low, _), (low_f, _) = model.predict_low(x, flip=True)
        return ops.confidence_hist(hist, hw, low, low_f)
    return ops.confidence_hist(hist, hw, model.predict_low(x)[0])


class GraphedConfidence(GraphedPredict):
    """confidence_image as a captured graph, by GraphedPredict's rules (the image is copied into a static
    buffer; the histogram is the pass's own tensor)."""

    def __init__(self, model, hist, hw, flip, device, scales=SINGLE_SCALE):
        super().__init__(model, None, hw, flip, device, scales=scales)
        self.hist = hist

    def _body(self):
        confidence_image(self.model, self.hist, self.x, self.hw, self.flip, self.scales)


class ThresholdPass:
    """The statistics pass and its result.  `thr` (fp32 [C] on the device, allocated once: a captured training
    step reads it) starts at `thr_max` for every class."""

    def __init__(self, model, num_classes, bins, device, portion=0.5, thr_max=0.95, flip=False,
                 scales=SINGLE_SCALE, graph=False):
        self.model, self.num_classes, self.device = model, int(num_classes), device
        self.bins, self.portion, self.thr_max = check_pass(bins, num_classes, portion, thr_max)
        self.flip, self.use_graph = bool(flip), bool(graph)
        self.scales = parse_scales(scales, self.flip)
        self.hist, self.thr, self.kept = ops.confidence_buffers(self.num_classes, self.bins, device)
        self.thr.fill_(self.thr_max)
        self.quantile = torch.ones_like(self.thr)  # the uncapped bin edge of each class, for the report
        self.images = 0
        self._graphed = {}

    def add(self, x, hw=None):
        x = x.to(self.device, non_blocking=True)
        size = (int(x.shape[-2]), int(x.shape[-1]))
        hw = size if hw is None else (int(hw[0]), int(hw[1]))
        if self.use_graph:
            key = (size, hw)
            if key not in self._graphed:
                self._graphed[key] = GraphedConfidence(self.model, self.hist, hw, self.flip, self.device, self.scales)
            self._graphed[key](x, None)
        else:
            confidence_image(self.model, self.hist, x, hw, self.flip, self.scales)
        self.images += 1

    def run(self, items, hw=None):
        """Zero the histogram, count `items` ((image, label, id) triples; the label is not read) with the
        model in eval mode - BN on its running statistics - under no_grad, take the thresholds, and put the
        model back into the mode it was in.  Returns self.thr."""
        was_training = self.model.training
        self.model.eval()
        self.hist.zero_()
        self.images = 0
        try:
            with torch.no_grad():
                for x, _, _ in items:
                    self.add(x, hw)
                # the report's quantile is the kernel's own: the same launch with the cap at 1 gives b* / bins
                ops.class_thresholds(self.hist, self.portion, 1.0, self.quantile, self.kept)
                ops.class_thresholds(self.hist, self.portion, self.thr_max, self.thr, self.kept)
        finally:
            self.model.train(was_training)
        return self.thr

    def table(self):
        """The per-class rows (one device-to-host read): dict(name, pixels, share, quantile, threshold,
        kept_share).  quantile is the uncapped bin edge b* / bins, from msl_class_thresholds itself."""
        hist = self.hist.cpu().numpy()
        thr, kept, quant = self.thr.cpu().numpy(), self.kept.cpu().numpy(), self.quantile.cpu().numpy()
        n = hist.sum(axis=1)
        total = max(int(n.sum()), 1)
        ids = {19: range(19), 16: synthia_set_16, 13: synthia_set_13}.get(self.num_classes)
        names = [name_classes[i] for i in ids] if ids is not None else [str(k) for k in range(self.num_classes)]
        rows = []
        for k in range(self.num_classes):
            rows.append(dict(name=str(names[k]), pixels=int(n[k]), share=float(n[k]) / total, quantile=float(quant[k]),
                             threshold=float(thr[k]), kept_share=float(kept[k]) / int(n[k]) if n[k] else 0.0))
        return rows

    def log(self, logger, title="class thresholds"):
        rows = self.table()
        logger.info("%s: %d images, %d bins, portion %.3f, cap %.3f", title, self.images, self.bins, self.portion,
                    self.thr_max)
        logger.info("  %-14s %12s %8s %9s %10s %6s", "class", "pixels", "share", "quantile", "threshold", "kept")
        for r in rows:
            logger.info("  %-14s %12d %8.4f %9.4f %10.4f %6.3f", r["name"], r["pixels"], r["share"], r["quantile"],
                        r["threshold"], r["kept_share"])
        return rows

    def save(self, directory):
        """<directory>/class_thresholds.json and <directory>/confidence_hist.npy; returns the json path."""
        os.makedirs(directory, exist_ok=True)
        path = os.path.join(directory, FILE_NAME)
        with open(path, "w") as f:
            json.dump({"bins": self.bins, "portion": self.portion, "thr_max": self.thr_max, "images": self.images,
                       "classes": self.table()}, f, indent=1)
        np.save(os.path.join(directory, HIST_NAME), self.hist.cpu().numpy())
        return path


def load_class_thresholds(path, num_classes):
    """The thresholds of a class_thresholds.json as a tuple of floats; an MSLError when the file does not hold
    one threshold in (0, 1] - or 0 - for each of `num_classes` classes."""
    try:
        with open(path) as f:
            rows = json.load(f)["classes"]
        thr = tuple(float(r["threshold"]) for r in rows)
    except (OSError, ValueError, KeyError, TypeError) as e:
        raise MSLError(f"--class_thresholds {path}: not a class_thresholds.json ({e})") from None
    if len(thr) != int(num_classes):
        raise MSLError(f"--class_thresholds {path}: {len(thr)} classes, --num_classes is {num_classes}")
    if not all(0.0 <= t <= 1.0 for t in thr):
        raise MSLError(f"--class_thresholds {path}: a threshold outside [0, 1]")
    return thr
