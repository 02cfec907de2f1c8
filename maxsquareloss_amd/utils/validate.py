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
"""
import gc
import os

import torch

from .. import ops
from ..hip import MSLError
from .eval import Eval
from .images import KIND_MAP, ImageWriter, recover_input
from .synthetic import SyntheticDomain

VAL_OFFSET = 900          # the val items' seed offset (train: 0, UDA target: 500)
VAL_ITER_MAX = 500        # evaluate.py:83: valid_iterations = min(num_iterations, 500)


def predict_image(model, ev, x, y, hw, flip, images=None, thr=0.95):
    """One image into ev's matrix: x (1,3,H,W) fp32, y int64 (H*W labels), both on the device; hw is
    the size the prediction is upsampled to.  `images` (ops.image_buffers) also receives the prediction
    as uint8 maps, in the same launch; with them y may be None (an unlabelled image: no matrix)."""
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

    def __init__(self, model, ev, hw, flip, device, maps=None, thr=0.95):
        """`maps`: the ops.predict_images maps to write on every call, into the static buffers
        self.images (valid after the call, until the next one)."""
        self.model, self.ev, self.hw, self.flip, self.device = model, ev, hw, flip, device
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
        predict_image(self.model, self.ev, self.x, self.y, self.hw, self.flip, self.images, self.thr)


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
                 outputs=None, labelled=True):
        """`data`: any iterable of (image (1,3,H,W), label, id) items with a length - a file-backed val
        loader (datasets/), a list of tensors; None = `images` synthetic items of size hw.  `outputs`: an
        OutputRequest (utils/images.py) - the selected items' predictions are also written as PNGs.  Its
        out_size upsamples to another size than the input's, so it needs `labelled=False`: the items'
        labels are then ignored and no matrix is filled."""
        self.model, self.hw, self.device, self.flip, self.use_graph = model, (int(hw[0]), int(hw[1])), device, flip, graph
        self.outputs, self.labelled = outputs, bool(labelled)
        if outputs is not None and outputs.out_size is not None and self.labelled:
            raise MSLError("--out_size upsamples the prediction to a size no label has: it is for unlabelled "
                           "images only (tools/predict.py), not for a labelled evaluator")
        if outputs is None and not self.labelled:
            raise MSLError("Validator: unlabelled data and no output request - nothing to compute")
        self.Eval = Eval(num_classes)
        if data is None:
            data = SyntheticDomain(self.hw[0], self.hw[1], num_classes, images, rank=rank, offset=VAL_OFFSET)
        self.data = data
        self.valid_iterations = min(len(self.data), VAL_ITER_MAX)
        # flip [, image size when it is not hw] [, the output size, maps, threshold and whether unlabelled of a
        # body that writes images] -> GraphedPredict (one capture per body and shape)
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
                    if self.use_graph:
                        key = self.flip if size == self.hw else (self.flip, size)
                        if save or y is None:  # another body: its own capture and static output buffers
                            key = (key, hw, maps, thr, y is None)
                        if key not in self._graphed:
                            self._graphed[key] = GraphedPredict(self.model, self.Eval, hw, self.flip, self.device,
                                                                maps, thr)
                        self._graphed[key](x, y)
                        images = self._graphed[key].images
                    else:
                        x = x.to(self.device, non_blocking=True)
                        images = ops.image_buffers(hw, maps, self.device) if save else None
                        predict_image(self.model, self.Eval, x,
                                      None if y is None else y.to(self.device, dtype=torch.long,
                                                                  non_blocking=True).reshape(-1),
                                      hw, self.flip, images, thr)
                    if save:
                        out = {k: images[KIND_MAP[k]] for k in req.kinds if k in KIND_MAP}
                        if "input" in req.kinds:
                            out["input"] = recover_input(x.to(self.device))
                        writer.save(self.item_name(ident, index), out)
        finally:
            if writer is not None:
                writer.close()
        return self.Eval
