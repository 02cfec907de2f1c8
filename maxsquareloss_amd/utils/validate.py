"""The validation loop of the reference (tools/evaluate.py:99-202; tools/train_source.py:420-553),
MI355X path, shared by tools/evaluate.py's Evaluater and Trainer.validate.

Per image: the eval-mode forward under torch.no_grad() down to the LOW-resolution head logits
(ResNetMulti.predict_low; with --flip the image and its mirror as one pair), then one kernel
(ops.predict_up, msl_predict_up) that re-interpolates every pixel, takes the reference's class -
np.argmax of the upsampled logits, or of (softmax + mirrored softmax of the flipped image) / 2 -
and counts it into the device confusion matrix.  The upsampled logits and probabilities are never
written and nothing crosses to the host until a metric is read.

`graph=True` captures that body once per shape as a hipGraph (GraphedPredict) and replays it with the
image and label copied into static buffers.  The data is whatever the caller hands the Validator - a
file-backed val loader (datasets/) - or, by default, synthetic (utils/synthetic.py) at a fixed offset
away from the training items.

With an output request (utils/images.py OutputRequest) the one kernel is ops.predict_images instead:
the same class and matrix, and the class written as the requested uint8 maps - static buffers in graph
mode - which an ImageWriter copies to pinned host slots and encodes as PNGs on host threads while the
next image runs.  An item's label may then be None (tools/predict.py: nothing to count).

`scales` other than (1.0,) (--scales, not in the reference) is multi-scale test-time augmentation: per
scale s the input is resized on the device to size_at(H, s) x size_at(W, s) (ops.resize_bilinear,
align_corners=True with torch-CPU's rounding; the scale that keeps the size takes the input as it is) and
run through predict_low - as a flip pair with --flip -, and ONE kernel (ops.predict_tta /
ops.predict_tta_images) upsamples every low-resolution output to the prediction size, sums the softmaxes in
the scales' order, each mirrored one mirrored back, and takes the class.  In graph mode the resizes, the
forwards and that launch are one captured graph.  (1.0,) is the single-scale path above, untouched.
"""
import argparse
import gc
import math
import os

import torch

from .. import ops
from ..hip import MSLError, load
from .eval import Eval
from .images import KIND_MAP, ImageWriter, recover_input
from .synthetic import SyntheticDomain

VAL_OFFSET = 900          # the val items' seed offset (train: 0, UDA target: 500)
VAL_ITER_MAX = 500        # evaluate.py:83: valid_iterations = min(num_iterations, 500)
SINGLE_SCALE = (1.0,)     # --scales' default: no multi-scale fusion
MAX_SCALES, MIN_SCALE, MAX_SCALE = 8, 0.25, 2.0


def size_at(n, s):
    """The side n at input scale s: round half up, at least 1 (Python floats)."""
    return max(1, int(math.floor(n * s + 0.5)))


def parse_scales(value, flip=False):
    """--scales: '0.75,1.0,1.25' or a sequence of numbers -> a tuple of floats, in the order given.  1 to 8
    values, each in [0.25, 2.0], no duplicates, and with `flip` twice as many entries as scales, at most
    what one fusion launch takes (msl_predict_tta_max_entries).  Anything else is an MSLError naming the
    value."""
    parts = [v.strip() for v in value.split(",")] if isinstance(value, str) else list(value)
    if not 1 <= len(parts) <= MAX_SCALES:
        raise MSLError(f"--scales takes 1 to {MAX_SCALES} values, got {len(parts)}: {value!r}")
    scales = []
    for v in parts:
        try:
            s = float(v)
        except (TypeError, ValueError):
            raise MSLError(f"--scales: {v!r} is not a number") from None
        if not MIN_SCALE <= s <= MAX_SCALE:  # a NaN fails both comparisons
            raise MSLError(f"--scales: {v!r} is outside [{MIN_SCALE}, {MAX_SCALE}]")
        if s in scales:
            raise MSLError(f"--scales: {v!r} is given twice")
        scales.append(s)
    if tuple(scales) != SINGLE_SCALE:  # the default takes no fusion launch
        n, cap = len(scales) * (2 if flip else 1), load(require_gpu=False).msl_predict_tta_max_entries()
        if n > cap:
            raise MSLError(f"--scales: {len(scales)} scales{' with --flip' if flip else ''} are {n} predictions, "
                           f"one launch fuses at most {cap}: {value!r}")
    return tuple(scales)


def scales_arg(text):
    """parse_scales as an argparse type: its refusals become argparse errors."""
    try:
        return parse_scales(text)
    except MSLError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def tta_entries(model, x, scales, flip):
    """The (low, mirror) entries of ops.predict_tta for x (1,3,H,W): per scale the resized input's
    low-resolution logits, followed with `flip` by those of its mirror (one image pair per scale)."""
    h, w = int(x.shape[-2]), int(x.shape[-1])
    entries = []
    for s in scales:
        hs, ws = size_at(h, s), size_at(w, s)
        xs = x if (hs, ws) == (h, w) else ops.resize_bilinear(x, (hs, ws))
        if flip:
            (low, _), (low_f, _) = model.predict_low(xs, flip=True)
            entries += [(low, 0), (low_f, 1)]
        else:
            entries.append((model.predict_low(xs)[0], 0))
    return entries


def predict_image(model, ev, x, y, hw, flip, images=None, thr=0.95, scales=SINGLE_SCALE):
    """One image into ev's matrix: x (1,3,H,W) fp32, y int64 (H*W labels), both on the device; hw is
    the size the prediction is upsampled to.  `images` (ops.image_buffers) also receives the prediction
    as uint8 maps, in the same launch; with them y may be None (an unlabelled image: no matrix).
    `scales` other than (1.0,): the multi-scale fusion of the module text.  `thr` as a device fp32 [C]
    tensor (--class_thresholds): the "pseudo" map comes from a launch of its own under one threshold per
    class (ops.pseudo_classwise), every other map and the matrix from the launch they always came from."""
    if torch.is_tensor(thr):
        pseudo = images.get("pseudo") if images else None
        if pseudo is None:
            thr = 0.95  # no map reads it
        else:
            rest = {k: v for k, v in images.items() if k != "pseudo"}
            entries = low = low_f = None
            if tuple(scales) != SINGLE_SCALE:
                entries = tta_entries(model, x, scales, flip)
            elif flip:
                (low, _), (low_f, _) = model.predict_low(x, flip=True)
            else:
                low = model.predict_low(x)[0]
            if y is not None and entries is not None:
                ev.add_batch_tta(y, entries, hw, images=rest or None)
            elif y is not None:
                ev.add_batch_low(y, low, hw, low_f, images=rest or None)
            elif rest and entries is not None:
                ops.predict_tta_images(entries, hw, out=rest)
            elif rest:
                ops.predict_images(low, hw, low_f, out=rest)
            ops.pseudo_classwise(thr, hw, low, low_f, entries, pseudo=pseudo)
            return
    if tuple(scales) != SINGLE_SCALE:
        if y is None and not images:
            if images is None:
                raise MSLError("predict_image: an unlabelled image and no output request - nothing to compute")
            return
        entries = tta_entries(model, x, scales, flip)
        if y is not None:
            ev.add_batch_tta(y, entries, hw, images=images, thr=thr)
        else:
            ops.predict_tta_images(entries, hw, out=images, thr=thr)
        return
    low_f = None
    if flip:
        (low, _), (low_f, _) = model.predict_low(x, flip=True)
    else:
        low = model.predict_low(x)[0]
    if y is not None:
        ev.add_batch_low(y, low, hw, low_f, images=images, thr=thr)
    elif images:
        ops.predict_images(low, hw, low_f, out=images, thr=thr)
    elif images is None:
        raise MSLError("predict_image: an unlabelled image and no output request - nothing to compute")


class GraphedPredict:
    """predict_image as a captured graph, by utils/graph.py's rules: the first call runs eagerly on
    the capture stream (that builds every weight pack and settles the allocator), then the body is
    captured once - own stream, no garbage collection while capturing - and later calls copy the
    image and label into the static buffers and replay.  The captured forward reads the weight packs
    (ops.PackCache, rewritten in place) and not the conv weights: before a replay, if any parameter's
    version differs from the versions the packs were built at, they are rebuilt eagerly first."""

    def __init__(self, model, ev, hw, flip, device, maps=None, thr=0.95, scales=SINGLE_SCALE):
        """`maps`: the ops.predict_images maps to write on every call, into the static buffers
        self.images (valid after the call, until the next one).  `scales`: predict_image's; the input
        resizes, every scale's forward and the fusion launch are then this one graph."""
        self.model, self.ev, self.hw, self.flip, self.device = model, ev, hw, flip, device
        self.scales = tuple(scales)
        self.images = None if maps is None else ops.image_buffers(hw, maps, device)
        self.thr = thr
        self.stream = torch.cuda.Stream(device=device)
        self.packer = ops.PackBatch(model)
        self.params = list(model.parameters())
        self.graph = None
        self.x = self.y = self.versions = None
        self.replays = 0
        self.eager_repacks = 0

    def _repack(self):
        self.packer.run()
        for c, d in self.packer._jobs():  # whatever the batched launch left stale: the per-conv path
            ws, cin, cout = c.meta[d]
            if c.key[d] != c.key_of(ws):
                c.get(ws, cin, cout, d)
        self.versions = [p._version for p in self.params]

    def __call__(self, x, y):
        if self.graph is None:
            return self._first(x, y)
        self.x.copy_(x, non_blocking=True)
        if self.y is not None:
            self.y.copy_(y.reshape(-1), non_blocking=True)
        if any(p._version != v for p, v in zip(self.params, self.versions)):
            self._repack()
            self.eager_repacks += 1
        self.graph.replay()
        self.replays += 1

    def _first(self, x, y):
        self.x = x.to(self.device, copy=True)
        self.y = None if y is None else y.to(self.device, dtype=torch.int64, copy=True).reshape(-1)
        s = self.stream
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            self._body()  # image 0, eager
        torch.cuda.current_stream(self.device).wait_stream(s)
        torch.cuda.synchronize(self.device)
        self._repack()  # nothing stale now; records the versions the packs were built at
        gc_was = gc.isenabled()
        gc.disable()
        try:
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=s):
                self._body()
        finally:
            if gc_was:
                gc.enable()
        torch.cuda.current_stream(self.device).wait_stream(s)


    def _body(self):
        predict_image(self.model, self.ev, self.x, self.y, self.hw, self.flip, self.images, self.thr,
                      self.scales)


def val_info(ev, logger, epoch, name=""):
    """The val_info lines of evaluate.py:170-195; returns (PA, MPA, MIoU, FWIoU), for 16 classes the
    13-class numbers."""
    PA = ev.Pixel_Accuracy()
    MPA, MIoU, FWIoU, PC = (ev.Mean_Pixel_Accuracy(), ev.Mean_Intersection_over_Union(),
                            ev.Frequency_Weighted_Intersection_over_Union(), ev.Mean_Precision())
    print("########## Eval{} ############".format(name))
    if ev.synthia:
        for k, tag in ((0, "16"), (1, "13")):
            logger.info('\nEpoch:{:.3f}, {} PA:{:.3f}, MPA_{t}:{:.3f}, MIoU_{t}:{:.3f}, FWIoU_{t}:{:.3f}, '
                        'PC_{t}:{:.3f}'.format(epoch, name, PA, MPA[k], MIoU[k], FWIoU[k], PC[k], t=tag))
        return PA, MPA[1], MIoU[1], FWIoU[1]
    logger.info('\nEpoch:{:.3f}, {} PA1:{:.3f}, MPA1:{:.3f}, MIoU1:{:.3f}, FWIoU1:{:.3f}, PC:{:.3f}'.format(
        epoch, name, PA, MPA, MIoU, FWIoU, PC))
    return PA, MPA, MIoU, FWIoU


class Validator:
    def __init__(self, model, num_classes, hw, images, device, flip=False, graph=False, rank=0, data=None,
                 outputs=None, labelled=True, scales=SINGLE_SCALE):
        """`data`: any iterable of (image (1,3,H,W), label, id) items with a length - a file-backed val
        loader (datasets/), a list of tensors; None = `images` synthetic items of size hw.  `outputs`: an
        OutputRequest (utils/images.py) - the selected items' predictions are also written as PNGs.  Its
        out_size upsamples to another size than the input's, so it needs `labelled=False`: the items'
        labels are then ignored and no matrix is filled.  `scales`: the input scales whose predictions are
        fused (parse_scales' rules; with `flip` each scale also runs mirrored); (1.0,) = none."""
        self.model, self.hw, self.device, self.flip, self.use_graph = model, (int(hw[0]), int(hw[1])), device, flip, graph
        self.scales = parse_scales(scales, flip)
        self.outputs, self.labelled = outputs, bool(labelled)
        if outputs is not None and outputs.out_size is not None and self.labelled:
            raise MSLError("--out_size upsamples the prediction to a size no label has: it is for unlabelled "
                           "images only (tools/predict.py), not for a labelled evaluator")
        if outputs is None and not self.labelled:
            raise MSLError("Validator: unlabelled data and no output request - nothing to compute")
        self.Eval = Eval(num_classes)
        self._class_thr = None  # --class_thresholds: the device fp32 [C] tensor the pseudo kind's launch reads
        if outputs is not None and getattr(outputs, "class_thresholds", None) is not None:
            if len(outputs.class_thresholds) != int(num_classes):
                raise MSLError(f"--class_thresholds holds {len(outputs.class_thresholds)} classes, the model has "
                               f"{num_classes}")
            self._class_thr = torch.tensor(outputs.class_thresholds, dtype=torch.float32, device=device)
        if data is None:
            data = SyntheticDomain(self.hw[0], self.hw[1], num_classes, images, rank=rank, offset=VAL_OFFSET)
        self.data = data
        self.valid_iterations = min(len(self.data), VAL_ITER_MAX)
        # flip [, image size when it is not hw] [, the scales when not (1.0,)] [, the output size, maps,
        # threshold and whether unlabelled of a body that writes images] -> GraphedPredict (one capture per
        # body and shape)
        self._graphed = {}

    def _items(self):
        if isinstance(self.data, SyntheticDomain):
            return (self.data[i] for i in range(self.valid_iterations))
        return (item for _, item in zip(range(self.valid_iterations), self.data))

    def item_name(self, ident, index):
        """The file name of an item's images: a name the item carries, the base name of a file-backed
        item's list entry, the index for synthetic ones."""
        if isinstance(ident, str):
            return ident
        items = getattr(getattr(self.data, "dataset", None), "items", None)
        if items is not None and isinstance(ident, int) and 0 <= ident < len(items):
            return os.path.splitext(os.path.basename(str(items[ident])))[0]
        return f"{index:06d}"

    def run(self):
        """Fill self.Eval over the val items (model.eval(), no_grad); the model stays in eval mode, as
        after the reference's validate()."""
        self.Eval.reset()
        self.model.eval()
        req = self.outputs
        writer = ImageWriter(req.directory, req.kinds, req.workers) if req is not None else None
        try:
            with torch.no_grad():
                for index, (x, y, ident) in enumerate(self._items()):
                    if not self.labelled:
                        y = None
                    size = (int(x.shape[-2]), int(x.shape[-1]))  # the item's own size (file-backed: the val resize)
                    hw = size if req is None or req.out_size is None else (req.out_size[1], req.out_size[0])
                    save = req is not None and req.selects(index, self.valid_iterations)
                    if y is None and not save:
                        continue
                    maps, thr = (req.maps, req.threshold) if save else (None, 0.95)
                    if save and self._class_thr is not None and "pseudo" in maps:
                        thr = self._class_thr
                    if self.use_graph:
                        key = self.flip if size == self.hw else (self.flip, size)
                        if self.scales != SINGLE_SCALE:
                            key = (key, "scales", self.scales)
                        if save or y is None:  # another body: its own capture and static output buffers
                            key = (key, hw, maps, "class" if torch.is_tensor(thr) else thr, y is None)
                        if key not in self._graphed:
                            self._graphed[key] = GraphedPredict(self.model, self.Eval, hw, self.flip, self.device,
                                                                maps, thr, self.scales)
                        self._graphed[key](x, y)
                        images = self._graphed[key].images
                    else:
                        x = x.to(self.device, non_blocking=True)
                        images = ops.image_buffers(hw, maps, self.device) if save else None
                        predict_image(self.model, self.Eval, x,
                                      None if y is None else y.to(self.device, dtype=torch.long,
                                                                  non_blocking=True).reshape(-1),
                                      hw, self.flip, images, thr, self.scales)
                    if save:
                        out = {k: images[KIND_MAP[k]] for k in req.kinds if k in KIND_MAP}
                        if "input" in req.kinds:
                            out["input"] = recover_input(x.to(self.device))
                        writer.save(self.item_name(ident, index), out)
        finally:
            if writer is not None:
                writer.close()
        return self.Eval
