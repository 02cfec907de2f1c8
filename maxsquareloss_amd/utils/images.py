"""Predictions as PNG files: what to save (OutputRequest) and the writer that saves it (ImageWriter).

The maps themselves come out of the prediction kernel (ops.predict_images) as uint8 tensors on the
device.  The writer copies the requested ones into one of a few pinned host slots on the current stream
and hands the slot to a bounded pool of host threads that wait for the copy and encode with Pillow (which
releases the GIL), so the encoding of image i overlaps the forward of image i + 1.  With no threads it
encodes on the calling thread.

Layout under the directory, one sub-directory per kind:
  color/NAME.png       RGB   the class colours
  trainids/NAME.png    L     the class index (the trainId of a 19-class model)
  labelids/NAME.png    L     the Cityscapes labelId (the test server's encoding)
  confidence/NAME.png  RGB   the class colour shaded by the winning probability
  pseudo/NAME.png      L     the class where that probability passes the threshold, 255 = ignored
  input/NAME.png       RGB   the uint8 image recovered from the network input
"""
import argparse
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from ..hip import MSLError
from .synthetic import IMG_MEAN

SAVE_KINDS = ("color", "trainids", "labelids", "confidence", "pseudo", "input")
# kind -> the map of ops.predict_images it is ("input" comes from the network input instead)
KIND_MAP = {"color": "color", "trainids": "class", "labelids": "ids", "confidence": "confidence", "pseudo": "pseudo"}
MAX_WRITER_THREADS = 16
MAX_WRITER_SLOTS = 64
SUMMARY_EVERY = 20  # the reference's image-summary cadence (evaluate.py: every 20th item and the last)


def parse_save_kinds(text):
    """'color,pseudo' -> ('color', 'pseudo'); an unknown kind is an argparse error."""
    kinds = tuple(k.strip() for k in str(text).split(",") if k.strip())
    bad = [k for k in kinds if k not in SAVE_KINDS]
    if bad or not kinds:
        raise argparse.ArgumentTypeError(f"unknown save kinds {bad}; choose from {','.join(SAVE_KINDS)}")
    return tuple(dict.fromkeys(kinds))


def parse_size(text):
    """'W,H' -> (W, H), both positive."""
    try:
        w, h = (int(v) for v in str(text).split(","))
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected W,H, got {text!r}")
    if w < 1 or h < 1:
        raise argparse.ArgumentTypeError(f"expected a positive W,H, got {text!r}")
    return w, h


class OutputRequest:
    """What a validation run saves: `directory`, the `kinds`, the pseudo-label `threshold`, the writer's
    `workers`, optionally `out_size` (W, H) to upsample to instead of the input size (unlabelled data
    only), and which items: every one, the first `first` of them, or every `every`-th and the last."""

    def __init__(self, directory, kinds=("color",), threshold=0.95, workers=0, out_size=None, first=None, every=None,
                 class_thresholds=None):
        """`class_thresholds`: one threshold per class (--class_thresholds FILE); the pseudo kind then keeps a
        class where its probability > that class's own value instead of `threshold`."""
        self.directory, self.kinds = str(directory), parse_save_kinds(",".join(kinds))
        self.threshold, self.workers = float(threshold), int(workers)
        self.class_thresholds = None if class_thresholds is None else tuple(float(t) for t in class_thresholds)
        self.out_size = None if out_size is None else (int(out_size[0]), int(out_size[1]))
        self.first, self.every = first, every

    @property
    def maps(self):
        """The ops.predict_images maps the kinds need, in IMAGE_MAPS' names."""
        return tuple(dict.fromkeys(KIND_MAP[k] for k in self.kinds if k in KIND_MAP))

    def selects(self, index, total):
        if self.first is not None:
            return index < self.first
        if self.every:
            return index % self.every == 0 or index == total - 1
        return True


def recover_input(x, mean=IMG_MEAN):
    """The uint8 (H, W, 3) RGB image a network input x (1, 3, H, W) fp32 BGR - mean was made from."""
    m = torch.as_tensor(np.asarray(mean, np.float32), device=x.device).view(3, 1, 1)
    return (x[0] + m).round_().clamp_(0, 255).to(torch.uint8).flip(0).permute(1, 2, 0).contiguous()


def _encode(directory, name, arrays):
    from PIL import Image
    for kind, arr in arrays.items():
        Image.fromarray(arr).save(os.path.join(directory, kind, name + ".png"))


def _encode_file(path, arr):
    from PIL import Image
    Image.fromarray(arr).save(path)


class _Slot:
    def __init__(self):
        self.buf, self.future = {}, None

    def stage(self, kind, t):
        """Copy tensor / array t into this slot's buffer of `kind`; returns the numpy view to encode."""
        t = torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t
        if t.dtype != torch.uint8:
            raise MSLError(f"ImageWriter: {kind} must be uint8, got {t.dtype}")
        buf = self.buf.get(kind)
        if buf is None or buf.numel() < t.numel():
            buf = torch.empty(t.numel(), dtype=torch.uint8, pin_memory=t.is_cuda)
            self.buf[kind] = buf
        view = buf[:t.numel()].view(t.shape)
        view.copy_(t, non_blocking=True)
        return view.numpy()


class ImageWriter:
    """save(name, {kind: uint8 map}) writes <directory>/<kind>/<name>.png for every kind given; device
    tensors are copied on the current stream.  `workers` host threads (at most 16) encode; each save uses
    the next of max(2, workers + 1) host slots and first waits for the encode that last used it.
    save_as(relpath, map) writes one map to <directory>/<relpath> the same way (tools/stylize.py).  `slots`
    asks for more host slots than that (at most MAX_WRITER_SLOTS): a caller that hands over many maps at
    once (utils/analysis.py's drain) is then not held up by the encoders while it does."""

    def __init__(self, directory, kinds=SAVE_KINDS, workers=0, slots=None):
        try:
            from PIL import Image  # noqa: F401
        except ImportError as e:
            raise MSLError("saving predictions encodes PNGs with Pillow, which is not installed") from e
        # kinds () = no per-kind sub-directories: a writer of whole files (save_as) only
        self.directory, self.kinds = str(directory), parse_save_kinds(",".join(kinds)) if kinds else ()
        for k in self.kinds:
            os.makedirs(os.path.join(self.directory, k), exist_ok=True)
        self.workers = max(0, min(int(workers), MAX_WRITER_THREADS))
        self._pool = ThreadPoolExecutor(self.workers, thread_name_prefix="msl-png") if self.workers else None
        self._slots = [_Slot() for _ in range(max(2, self.workers + 1, min(int(slots or 0), MAX_WRITER_SLOTS)))]
        self._n = 0
        self.written = []

    def save(self, name, maps):
        bad = [k for k in maps if k not in self.kinds]
        if bad:
            raise MSLError(f"ImageWriter: kinds {bad} were not requested ({','.join(self.kinds)})")
        name = str(name)
        self._stage_and_encode(maps, lambda arrays: _encode(self.directory, name, arrays))
        self.written.append(name)

    def save_as(self, relpath, t):
        """Write one uint8 map to <directory>/<relpath>, in the format of the path's extension (the
        stylised datasets of tools/stylize: PNG or JPEG, any sub-directory)."""
        path = os.path.join(self.directory, str(relpath))
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        self._stage_and_encode({"file": t}, lambda arrays: _encode_file(path, arrays["file"]))
        self.written.append(str(relpath))

    def _stage_and_encode(self, maps, encode):
        slot = self._slots[self._n % len(self._slots)]
        self._n += 1
        if slot.future is not None:
            slot.future.result()
            slot.future = None
        on_device = [t for t in maps.values() if torch.is_tensor(t) and t.is_cuda]
        arrays = {k: slot.stage(k, t) for k, t in maps.items()}
        event = None
        if on_device:
            event = torch.cuda.Event()
            event.record(torch.cuda.current_stream(on_device[0].device))

        def job():
            if event is not None:
                event.synchronize()
            encode(arrays)

        if self._pool is None:
            job()
        else:
            slot.future = self._pool.submit(job)

    def flush(self):
        for slot in self._slots:
            if slot.future is not None:
                slot.future.result()
                slot.future = None

    def close(self):
        self.flush()
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
