"""Per-image analysis (the reference's tools/analysis.py: resultEvaluater.getvalResult), MI355X path.

Which images does a model fail on, and what do the failures look like?  The reference walks the val set with
two `Eval`s: one is filled and reset per image and gives that image's PA, MPA, MIoU and FWIoU, the other
keeps the whole set's matrix; every image whose MIoU is below a threshold is saved as three pictures named
with its scores.  It copies the full-resolution prediction to the host per image and computes everything in
numpy.

Here the per-image body is three launches after the forward and nothing crosses to the host:
  1. utils/validate.predict_image with images={"class": ...}: the class of every pixel, as a uint8 map, and
     the image's confusion matrix (self.Eval's device matrix) in one kernel (msl_predict_images; the
     multi-scale fusion kernel with --scales);
  2. ops.image_metrics (msl_image_metrics): the scores from that matrix into row `cursor % ring` of a device
     table, the decision MIoU < threshold into `state`, the matrix added to self.totalEval's and zeroed;
  3. ops.analysis_maps (msl_analysis_maps): the failure maps into slot `cursor % ring` of a ring of uint8
     buffers - a launch whose every thread first reads the decision and returns when it is 0.
With graph=True the forward and the three launches are one captured hipGraph (GraphedAnalysis, by
GraphedPredict's rules: static x, y, class map, rings and state), replayed per image.

The host looks once every `ring` images and at the end (a *drain*): one device-to-host copy of the filled
rows - the run's only host sync -, and for each selected row the slot's maps are handed to the ImageWriter
(pinned copy on the stream, PNG encoding on host threads).  Files, under <save_dir>/savePics, carry the
reference's names:
    {stem}_PA_{:.2f}_MPA_{:.2f}_MIoU_{:.2f}_FWIoU_{:.2f}_{label_img,pred_img,style_img,error_img}.png
`rows` is the reference's id2mIOU, per_image.csv the same table with the pixel count and whether the image was
saved, and the whole-set scores are printed as the reference prints them.

Differences from the reference: no nn.DataParallel (one device); style_img is the exact recovered input
(utils/images.py:recover_input's bytes), not the min-max-normalised one of inv_preprocess; error_img is new;
decode_labels' unpacking bug (the reference's call takes two results from a function that returns one) and
the hard-coded dataset path table are not reproduced; for 16 classes the scores are val_info's 13-class ones.
"""
import argparse
import csv
import os
from pathlib import Path

import numpy as np
import torch

from .. import ops
from ..hip import MSLError
from .eval import Eval, name_classes
from .images import ImageWriter
from .palette import trainids_of
from .validate import SINGLE_SCALE, GraphedPredict, Validator, predict_image

KINDS = ("label", "pred", "style", "error")
DEFAULT_KINDS = ("label", "pred", "style")  # the reference's three pictures
KIND_MAP = {"label": "label", "pred": "pred", "style": "input", "error": "error"}  # kind -> ops.ANALYSIS_MAPS
KIND_FILES = {"label": "label_img", "pred": "pred_img", "style": "style_img", "error": "error_img"}
MIOU_THRESHOLD = 0.5  # tools/analysis.py:169
RING_DEFAULT, RING_MAX = 8, 64
SAVE_SUBDIR = "savePics"


def parse_kinds(text):
    """'label,error' -> ('label', 'error'); an unknown or missing kind is an argparse error."""
    kinds = tuple(k.strip() for k in str(text).split(",") if k.strip())
    bad = [k for k in kinds if k not in KINDS]
    if bad or not kinds:
        raise argparse.ArgumentTypeError(f"unknown analysis kinds {bad}; choose from {','.join(KINDS)}")
    return tuple(dict.fromkeys(kinds))


def ring_arg(text):
    """--ring: how many images between two looks of the host, 1 to 64."""
    try:
        n = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--ring: {text!r} is not an integer") from None
    if not 1 <= n <= RING_MAX:
        raise argparse.ArgumentTypeError(f"--ring: {n} is outside [1, {RING_MAX}]")
    return n


def base_name(ident, PA, MPA, MIoU, FWIoU):
    """tools/analysis.py:211-212: the part of a saved picture's name before label_img.png etc."""
    return '{}_PA_{:.2f}_MPA_{:.2f}_MIoU_{:.2f}_FWIoU_{:.2f}_'.format(Path(str(ident)).stem, PA, MPA, MIoU, FWIoU)


def file_name(ident, scores, kind):
    return base_name(ident, *scores) + KIND_FILES[kind] + ".png"


def row_scores(row, num_classes):
    """(PA, MPA, MIoU, FWIoU) of one msl_image_metrics row as val_info returns them: the 13-class values for
    16 classes."""
    idx = (0, 4, 5, 6) if num_classes == 16 else (0, 1, 2, 3)
    return tuple(float(row[i]) for i in idx)


class GraphedAnalysis(GraphedPredict):
    """The per-image body of an Analyzer as one captured graph: GraphedPredict's prediction into the static
    class map, then the analyzer's two launches on the static x, y, rings and state."""

    def __init__(self, analyzer):
        super().__init__(analyzer.model, analyzer.Eval, analyzer.hw, analyzer.flip, analyzer.device,
                         maps=("class",), scales=analyzer.scales)
        self.analyzer = analyzer

    def _body(self):
        super()._body()
        self.analyzer.score_and_map(self.x, self.y, self.images["class"])


class Analyzer(Validator):
    def __init__(self, model, num_classes, hw, images, device, save_dir, flip=False, scales=SINGLE_SCALE,
                 graph=False, data=None, threshold=MIOU_THRESHOLD, kinds=DEFAULT_KINDS, ring=RING_DEFAULT,
                 workers=0, rank=0):
        """`data`, `images`, `flip`, `scales`, `graph` as the Validator's (every item of size hw, labelled).
        `threshold`: an image is saved when its MIoU is strictly below it.  `kinds`: the pictures of a saved
        image.  `ring`: the images between two drains, 1 to 64 - the depth of the row table and of the maps'
        rings.  `workers`: the ImageWriter's host threads."""
        super().__init__(model, num_classes, hw, images, device, flip=flip, graph=graph, rank=rank, data=data,
                         scales=scales)
        if not 1 <= int(ring) <= RING_MAX:
            raise MSLError(f"Analyzer: ring {ring} is outside [1, {RING_MAX}]")
        self.num_classes, self.threshold, self.ring = int(num_classes), float(threshold), int(ring)
        self.kinds = parse_kinds(",".join(kinds))
        self.save_dir, self.workers = str(save_dir), int(workers)
        self.out_dir = os.path.join(self.save_dir, SAVE_SUBDIR)
        self.totalEval = Eval(num_classes)
        self.rows, self.table = [], []
        self.drains = 0
        self._pending = []
        self._dev_ready = False
        self._graph = None

    @property
    def replays(self):
        return 0 if self._graph is None else self._graph.replays

    def _device_state(self):
        """The static device buffers (built once): both matrices, the row table, the state, the rings and,
        for the eager path, the class map."""
        if self._dev_ready:
            return
        c, dev = self.num_classes, self.device
        self.Eval._dev = torch.zeros(c * c, dtype=torch.int64, device=dev)       # this image's matrix
        self.totalEval._dev = torch.zeros(c * c, dtype=torch.int64, device=dev)  # total_cm
        self.rows_dev, self.state = ops.metrics_buffers(c, self.ring, dev)
        # the class map of the eager path; a captured body writes GraphedAnalysis' own static one
        self.cls = None if self.use_graph else ops.image_buffers(self.hw, ("class",), dev)
        self.rings = ops.analysis_buffers(self.hw, tuple(dict.fromkeys(KIND_MAP[k] for k in self.kinds)),
                                          self.ring, dev)
        self._dev_ready = True

    def score_and_map(self, x, y, cls):
        """The two launches after the prediction: the scores and the decision, then the gated maps."""
        ops.image_metrics(self.Eval._dev, self.totalEval._dev, self.threshold, self.rows_dev, self.state)
        ops.analysis_maps(x, y, cls, self.num_classes, state=self.state, out=self.rings)

    def _drain(self, writer):
        n = len(self._pending)
        if not n:
            return
        rows = self.rows_dev[:n].cpu().numpy()  # the one device-to-host copy, and the sync
        self.drains += 1
        for slot, ident in enumerate(self._pending):
            r = rows[slot]
            scores = row_scores(r, self.num_classes)
            saved = bool(r[8])
            self.rows.append((ident,) + scores)
            self.table.append((ident,) + scores + (int(r[7]), int(saved)))
            if saved:
                for k in self.kinds:
                    writer.save_as(file_name(ident, scores, k), self.rings[KIND_MAP[k]][slot])
        self._pending.clear()

    def run(self):
        """Walk the val items; fills `rows`, writes the pictures and per_image.csv, prints the whole-set
        scores; returns `rows` (the reference's id2mIOU)."""
        self._device_state()
        self.Eval.reset()
        self.totalEval.reset()
        self.rows_dev.zero_()
        self.state.zero_()
        self.rows, self.table, self.drains = [], [], 0
        self._pending.clear()
        self.model.eval()
        os.makedirs(self.out_dir, exist_ok=True)
        # a drain hands over up to ring x kinds maps at once: a host slot each, so that it only stages copies
        # and the encoding runs under the next images' forwards
        writer = ImageWriter(self.out_dir, (), self.workers,
                             slots=self.ring * len(self.kinds) if self.workers else None)
        try:
            with torch.no_grad():
                for index, (x, y, ident) in enumerate(self._items()):
                    if (int(x.shape[-2]), int(x.shape[-1])) != self.hw:
                        raise MSLError(f"Analyzer: item {index} is {tuple(x.shape[-2:])}, the rings are {self.hw}")
                    if self.use_graph:
                        if self._graph is None:
                            self._graph = GraphedAnalysis(self)
                        self._graph(x, y)
                    else:
                        if self.cls is None:  # use_graph was switched off after a graphed run
                            self.cls = ops.image_buffers(self.hw, ("class",), self.device)
                        x = x.to(self.device, non_blocking=True)
                        y = y.to(self.device, dtype=torch.long, non_blocking=True).reshape(-1)
                        predict_image(self.model, self.Eval, x, y, self.hw, self.flip, self.cls, 0.95, self.scales)
                        self.score_and_map(x, y, self.cls["class"])
                    self._pending.append(self.item_name(ident, index))
                    if len(self._pending) == self.ring:
                        self._drain(writer)
                self._drain(writer)
        finally:
            writer.close()
        self.write_csv()
        self.print_total()
        return self.rows

    def write_csv(self):
        os.makedirs(self.save_dir or ".", exist_ok=True)
        with open(os.path.join(self.save_dir, "per_image.csv"), "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(("id", "PA", "MPA", "MIoU", "FWIoU", "pixels", "saved"))
            for ident, PA, MPA, MIoU, FWIoU, pixels, saved in self.table:
                w.writerow((ident, repr(PA), repr(MPA), repr(MIoU), repr(FWIoU), pixels, saved))

    def total_scores(self):
        """(totalPA, totalMPA, totalMIoU, totalFWIoU) of the whole set, val_info's values."""
        ev = self.totalEval
        PA = ev.Pixel_Accuracy()
        out = (ev.Mean_Pixel_Accuracy(), ev.Mean_Intersection_over_Union(),
               ev.Frequency_Weighted_Intersection_over_Union())
        return (PA,) + tuple(v[1] if ev.synthia else v for v in out)

    def print_total(self):
        """tools/analysis.py:232-236."""
        ev = self.totalEval
        ious = ev._iou(ev.confusion_matrix)
        print('##### IOU for each class is #####')
        names = [name_classes[t] for t in trainids_of(self.num_classes)]
        for name, v in zip(names, ious):
            print(name, v)
        print('totalPA, totalMPA, totalMIoU, totalFWIoU', *self.total_scores())

    def worst(self, n):
        """The n rows of lowest MIoU (NaN last)."""
        key = lambda r: (np.isnan(r[3]), r[3])  # noqa: E731
        return sorted(self.rows, key=key)[:max(0, int(n))]
