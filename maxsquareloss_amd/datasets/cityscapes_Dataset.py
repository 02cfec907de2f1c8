"""City_Dataset / City_DataLoader (datasets/cityscapes_Dataset.py:86-171, 281-323 of the reference),
MI355X path.

Same constructor arguments, list files, path rule and `(image, label, id)` items.  What differs is
where the work runs: Pillow only decodes the two PNGs; the decoded uint8 arrays are uploaded as
they are and the whole of _train_sync_transform / _val_sync_transform (:173-243) - mirror, crop,
BICUBIC / NEAREST resize, BGR - mean, id -> trainId - runs on the device, byte-exact against Pillow
(utils/preprocess.py resize_image / resize_label).  An item is (1,3,H,W) fp32 + (1,H,W) int64 on
the GPU.

The augmentation draws (mirror, then x1, then y1, the reference's order) come from a
`random.Random` the dataset owns and are made by the consumer in item order, so they do not
depend on how many threads decode ahead (--data_loader_workers, at most 16; Pillow releases the
GIL while decoding).

A decoded image is an (H, W, 3) uint8 array - or, for a JPEG file (the NTHU cities of
crosscity_Dataset.py, the lists of Client_dataset), the 1-D uint8 payload of the decode's host half
(utils/jpeg.py: header, tables, Huffman-decoded coefficients), which goes through the same pinned
staging slot and is finished on the device ahead of the transform.  The loader therefore asks the
dataset for `item_plan(decoded)` and does not read a shape itself: for a payload the plan carries
the header, (mirror, steps, header), and device_transform starts with image_of().
"""
import collections
import os
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from ..hip import MSLError
from ..utils import jpeg, preprocess, resample
from ..utils.eval import name_classes  # noqa: F401  (the reference keeps the row names in this module)
from ..utils.palette import label_colours, palette_table
from ..utils.synthetic import IMG_MEAN

MAX_WORKERS = 16
NUM_CLASSES = 19


def _pil():
    try:
        from PIL import Image
    except ImportError as e:  # pragma: no cover - Pillow is present wherever the tests decode
        raise MSLError("the file-backed datasets decode PNGs with Pillow, which is not installed; install "
                       "Pillow or leave --data_root_path unset for the synthetic loaders") from e
    return Image


def decode_rgb(path, jpeg_decode="device", alloc=None):
    """One image file for the device: a JPEG as the payload of its host half (utils/jpeg.py decode_file; the
    device finishes it, utils/preprocess.py jpeg_reconstruct) - unless jpeg_decode is 'pillow' or the split
    decoder refuses the file - anything else as Pillow's uint8 (H, W, 3) RGB array.  Either way the item is the
    same bytes.  alloc(nbytes) -> a uint8 array: where a payload is decoded to (the loader's pinned staging slot;
    default a new array).  Host only, thread-safe."""
    if jpeg_decode == "device" and str(path).lower().endswith(jpeg.EXTENSIONS):
        payload = jpeg.decode_file(path, alloc)
        if payload is not None:
            return payload
    with _pil().open(path) as im:
        return np.asarray(im.convert("RGB"), np.uint8)


def image_of(rgb, plan):
    """(the decoded image on the device, (mirror, steps)): an item_plan that carries a JPEG header says `rgb` is
    the payload on the device, finished here."""
    if len(plan) == 3:
        return preprocess.jpeg_reconstruct(rgb, plan[2]), plan[:2]
    return rgb, plan


def _item_plan(self, rgb):
    """The plan of a decoded item.  An (H, W, 3) array says its own size; a JPEG payload (1-D) says it in
    its header, which then rides with the plan: (mirror, steps, header)."""
    if jpeg.is_payload(rgb):
        header = jpeg.header_of(rgb)
        return tuple(self.plan(header.width, header.height)) + (header,)
    return self.plan(rgb.shape[1], rgb.shape[0])


def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


class City_Dataset:
    name = "cityscapes"

    def __init__(self, args, data_root_path=os.path.abspath("./datasets/Cityscapes"),
                 list_path=os.path.abspath("./datasets/city_list"), gt_path=None, split="train", training=True,
                 class_16=False, class_13=False):
        self.args = args
        self.data_path, self.list_path, self.gt_path = data_root_path, list_path, gt_path
        self.split, self.training = split, training
        self._setup(args)
        # cityscapes_Dataset.py:111-114: seg_size unless --DA
        self.rsize = _pair(args.seg_size) if not getattr(args, "DA", False) else self.base_size
        self.items = self._read_list("train" if "train" in split else "val")
        self.class_16, self.class_13 = class_16, class_13
        self.lut = preprocess.build_lut(self.name, class_16, class_13)

    def _setup(self, args):
        self.base_size, self.crop_size = _pair(args.base_size), _pair(args.crop_size)
        self.random_mirror, self.random_crop, self.resize = args.random_mirror, args.random_crop, args.resize
        self.rng = random.Random(getattr(args, "seed", 12345))
        self.device = None

    def _read_list(self, stem):
        path = os.path.join(self.list_path, stem + ".txt")
        if not os.path.exists(path):
            raise MSLError(f"{type(self).__name__}: list file {path} is missing (split {self.split!r})")
        with open(path) as f:
            return [line.strip() for line in f if line.strip()]

    def __len__(self):
        return len(self.items)

    # ------------------------------------------------------------------ host: files
    def paths(self, item):
        """(image path, label path, the id the item carries) - cityscapes_Dataset.py:158-163."""
        rel = self.items[item]
        gt = self.gt_path + rel.replace("leftImg8bit", "", 1).replace("leftImg8bit", "gtFine_labelIds")
        return os.path.join(self.data_path, rel), gt, item

    def decode(self, item):
        """The two PNGs as uint8 arrays: (H, W, 3) RGB and (H, W) ids.  Host only, thread-safe."""
        Image = _pil()
        image_path, gt_path, _ = self.paths(item)
        with Image.open(image_path) as im:
            rgb = np.asarray(im.convert("RGB"), np.uint8)
        with Image.open(gt_path) as im:
            ids = np.asarray(im)
        if ids.ndim != 2 or ids.dtype != np.uint8:
            raise MSLError(f"{gt_path}: expected a 2-D uint8 label map, got shape {ids.shape} dtype {ids.dtype}")
        if ids.shape != rgb.shape[:2]:
            raise MSLError(f"{gt_path}: label map {ids.shape} does not match its image {rgb.shape[:2]}")
        return rgb, ids

    # ------------------------------------------------------------------ the transform as a plan
    def is_train(self):
        return ("train" in self.split or "trainval" in self.split) and self.training

    def plan(self, w, h):
        """Draw this item's augmentation and lay the transform out as (mirror, steps), steps =
        [(out (w, h), crop (x1, y1, w, h) or None), ...], each an exact Pillow crop + resize
        (_train_sync_transform / _val_sync_transform, :173-243; val resizes first, then crops)."""
        steps = []
        if self.is_train():
            mirror = bool(self.random_mirror and self.rng.random() < 0.5)
            if self.random_crop:
                steps.append((self.base_size, self._draw_crop(w, h)))
            if self.resize:
                steps.append((self.rsize, None))
        else:
            mirror = False
            if self.resize:
                steps.append((self.rsize, None))
                w, h = self.rsize
            if self.random_crop:
                steps.append((self.base_size, self._draw_crop(w, h)))
        return mirror, steps or [((w, h), None)]

    item_plan = _item_plan

    def _draw_crop(self, w, h):
        cw, ch = self.crop_size
        x1 = self.rng.randint(0, w - cw)
        y1 = self.rng.randint(0, h - ch)
        return x1, y1, cw, ch

    def host_transform(self, rgb, ids, plan):
        """The plan in numpy (utils/resample.py): what the device path must equal bit for bit."""
        mirror, steps = plan
        for out_wh, crop in steps:
            rgb = resample.resize_bicubic(rgb, out_wh, crop, mirror)
            ids = resample.resize_nearest(ids, out_wh, crop, mirror)
            mirror = False
        img = torch.from_numpy(resample.bgr_minus_mean(rgb, IMG_MEAN)).unsqueeze(0)
        lab = torch.from_numpy(self.lut[ids].astype(np.int64)).unsqueeze(0)
        return img, lab

    def device_transform(self, rgb, ids, plan):
        """rgb / ids: the decoded uint8 tensors on the GPU -> ((1,3,H,W) fp32, (1,H,W) int64).  With
        self.deliver_uint8 (set by tools/ADAIN.py, whose style network reads RGB bytes: the reference's
        adain_transform) the image stays the resized uint8 (H, W, 3) RGB."""
        mirror, steps = plan
        keep_u8 = getattr(self, "deliver_uint8", False)
        for k, (out_wh, crop) in enumerate(steps):
            last = k == len(steps) - 1
            rgb = preprocess.resize_image(rgb, out_wh, crop, mirror, as_uint8=keep_u8 or not last)
            ids = preprocess.resize_label(ids, out_wh, self.lut if last else None, crop, mirror)
            mirror = False
        return rgb, ids

    def _device(self):
        if self.device is None:
            if not torch.cuda.is_available():
                raise MSLError("the file-backed datasets transform on the GPU; no GPU is visible")
            self.device = torch.device("cuda", torch.cuda.current_device())
        return self.device

    def __getitem__(self, item):
        rgb, ids = self.decode(item)
        plan = self.item_plan(rgb)
        dev = self._device()
        img, lab = self.device_transform(torch.from_numpy(rgb).to(dev),
                                         None if ids is None else torch.from_numpy(ids).to(dev), plan)
        return img, lab, self.paths(item)[2]


class _Slot:
    """One pinned staging pair; `event` marks the end of the last H2D copy that read it, and a
    decoding thread waits for it before it writes the buffers again."""

    def __init__(self):
        self.rgb = self.ids = self.event = None

    def reserve(self, nbytes):
        """uint8 (nbytes,) numpy view of the pinned image buffer, for a decoder that writes its output in place
        (a dataset's decode_into); fill() then finds the item where it belongs and copies nothing."""
        if self.event is not None:
            self.event.synchronize()
        if self.rgb is None or self.rgb.numel() < nbytes:
            self.rgb = torch.empty(int(nbytes), dtype=torch.uint8).pin_memory()
        return self.rgb[:nbytes].numpy()

    def fill(self, rgb, ids):
        if self.event is not None:
            self.event.synchronize()
        out = []
        for name, arr in (("rgb", rgb), ("ids", ids)):
            if arr is None:  # an unlabelled item (Client_dataset)
                out.append(None)
                continue
            buf = getattr(self, name)
            if buf is None or buf.numel() < arr.size:
                buf = torch.empty(arr.size, dtype=torch.uint8).pin_memory()
                setattr(self, name, buf)
            view = buf[:arr.size].view(arr.shape)
            if arr.ctypes.data != buf.data_ptr():  # (else: decoded in place, reserve())
                np.copyto(view.numpy(), arr)
            out.append(view)
        return out


class DeviceLoader:
    """One dataset as an iterable of device items, batch size 1: an epoch is a seeded permutation
    (shuffle) or the list order; `workers` threads decode ahead of the consumer into pinned staging
    buffers, the consumer draws the augmentation, uploads and transforms on the current stream."""

    def __init__(self, dataset, shuffle, workers=0, seed=12345):
        self.dataset, self.shuffle, self.seed = dataset, bool(shuffle), int(seed)
        self.workers = max(0, min(int(workers), MAX_WORKERS))
        self.epoch = 0
        self._pool = ThreadPoolExecutor(self.workers, thread_name_prefix="msl-decode") if self.workers else None
        self._slots = None

    def __len__(self):
        return len(self.dataset)

    def order(self, epoch):
        idx = list(range(len(self.dataset)))
        if self.shuffle:
            random.Random(self.seed * 1000003 + epoch).shuffle(idx)
        return idx

    def _decode(self, item, slot):
        into = getattr(self.dataset, "decode_into", None)
        if slot is not None and into is not None:
            rgb, ids = into(item, slot.reserve)  # the image may already sit in the slot's pinned buffer
        else:
            rgb, ids = self.dataset.decode(item)
        return slot.fill(rgb, ids) if slot is not None else (rgb, ids)

    def host_items(self, staged=False):
        """One epoch of (rgb, ids, plan, id, slot): decoded arrays (pinned tensors with `staged`), the
        plan drawn in item order on the calling thread."""
        order = self.order(self.epoch)
        self.epoch += 1
        depth = 2 * self.workers
        if staged and self._slots is None:
            self._slots = [_Slot() for _ in range(depth + 1)]
        slot_of = (lambda s: self._slots[s % len(self._slots)]) if staged else (lambda s: None)
        pending = collections.deque()
        try:
            nxt = 0
            for seq, item in enumerate(order):
                if self._pool is None:
                    got = self._decode(item, slot_of(seq))
                else:
                    while nxt < len(order) and len(pending) < depth:
                        pending.append(self._pool.submit(self._decode, order[nxt], slot_of(nxt)))
                        nxt += 1
                    got = pending.popleft().result()
                rgb, ids = got
                plan = self.dataset.item_plan(rgb)
                yield rgb, ids, plan, self.dataset.paths(item)[2], slot_of(seq)
        finally:
            for f in pending:
                f.cancel()
            for f in pending:
                if not f.cancelled():
                    f.exception()  # wait: no thread writes a slot after the epoch is abandoned

    def __iter__(self):
        ds = self.dataset
        dev = ds._device()
        for rgb, ids, plan, ident, slot in self.host_items(staged=True):
            d_rgb = rgb.to(dev, non_blocking=True)
            d_ids = ids.to(dev, non_blocking=True) if ids is not None else None
            slot.event = torch.cuda.Event()
            slot.event.record(torch.cuda.current_stream(dev))
            img, lab = ds.device_transform(d_rgb, d_ids, plan)
            yield img, lab, ident

    def cycle(self):
        """Items for ever, epoch after epoch (the UDA loop pairs two loaders of different lengths)."""
        while True:
            yield from self

    def close(self):
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None
            self.workers = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class City_DataLoader:
    """cityscapes_Dataset.py:281-323: `data_loader` (args.split, shuffled when training),
    `val_loader` (the val split, in order), num_iterations / valid_iterations in items."""
    dataset_class = City_Dataset

    def __init__(self, args, training=True, datasets_path=None):
        self.args = args
        paths = datasets_path["Cityscapes"] if "Cityscapes" in datasets_path else datasets_path
        kw = dict(data_root_path=paths["data_root_path"], list_path=paths["list_path"], gt_path=paths["gt_path"])
        extra = dict(class_16=getattr(args, "class_16", False), class_13=getattr(args, "class_13", False))
        if int(getattr(args, "batch_size", 1)) != 1:
            raise MSLError("the file-backed loaders run batch size 1 (the reference's default)")
        workers, seed = getattr(args, "data_loader_workers", 0), getattr(args, "seed", 12345)
        data_set = self._make(args, kw, extra, args.split, training)
        if len(data_set) == 0:
            raise MSLError(f"{type(data_set).__name__}: the {args.split!r} list under {paths['list_path']} is empty")
        val_set = self._make(args, kw, extra, self._val_split(args), False)
        self.data_loader = DeviceLoader(data_set, shuffle=training and "train" in args.split, workers=workers, seed=seed)
        self.val_loader = DeviceLoader(val_set, shuffle=False, workers=workers, seed=seed)
        self.num_iterations = len(data_set)
        self.valid_iterations = len(val_set)

    def _val_split(self, args):
        return "val"

    def _make(self, args, kw, extra, split, training):
        return self.dataset_class(args, split=split, training=training, **kw, **extra)

    def close(self):
        self.data_loader.close()
        self.val_loader.close()


class Client_dataset:
    """cityscapes_Dataset.py:43-83: a list of unlabelled images to predict on.  `<list_path>/test.txt`
    holds one image path per line; with --resize the image is resized to seg_size (Pillow's BICUBIC,
    byte-exact on the device) before the image transform.  Items are (image (1,3,H,W) fp32, None, name),
    name the list entry's base name without its extension.  Decodes ahead through DeviceLoader like the
    labelled datasets."""
    name = "client"

    def __init__(self, dataset_path, args):
        self.args, self.dataset_path = args, dataset_path
        self.resize = bool(getattr(args, "resize", False))
        self.rsize = _pair(args.seg_size) if self.resize else None
        path = os.path.join(dataset_path["list_path"], "test.txt")
        if not os.path.exists(path):
            raise MSLError(f"Client_dataset: list file {path} is missing")
        with open(path) as f:
            self.items = [line.strip() for line in f if line.strip()]
        self.device = None

    def __len__(self):
        return len(self.items)

    def paths(self, item):
        path = self.items[item]
        return path, None, os.path.splitext(os.path.basename(path))[0]

    def decode(self, item, alloc=None):
        return decode_rgb(self.paths(item)[0], getattr(self.args, "jpeg_decode", "device"), alloc), None

    decode_into = decode  # (item, alloc): a JPEG's payload is decoded straight into the staging slot

    def plan(self, w, h):
        return False, [(self.rsize if self.resize else (w, h), None)]

    item_plan = _item_plan

    def device_transform(self, rgb, ids, plan):
        rgb, (mirror, steps) = image_of(rgb, plan)
        return preprocess.resize_image(rgb, steps[0][0], None, mirror), None

    _device = City_Dataset._device

    def __getitem__(self, item):
        rgb, _ = self.decode(item)
        img, _ = self.device_transform(torch.from_numpy(rgb).to(self._device()), None, self.item_plan(rgb))
        return img, None, self.paths(item)[2]


# ---------------------------------------------------------------------- looking at images and predictions
def _palette_of(num_classes):
    """uint8 [C, 3]: the colour of every class - through its trainId for the 16- and 13-class sets (a
    deviation from the reference, which paints class index k with colour k whatever the class count; the
    same for 19 classes), the first num_classes colours otherwise."""
    if num_classes in (19, 16, 13):
        return palette_table(num_classes)
    if not 1 <= num_classes <= len(label_colours):
        raise MSLError(f"decode_labels: no colours for {num_classes} classes")
    return np.array(label_colours[:num_classes], np.uint8)


_DEVICE_PALETTES = {}


def decode_labels(mask, num_images=1, num_classes=NUM_CLASSES):
    """cityscapes_Dataset.py:352-377: the first min(n, num_images) class maps of `mask` (n, h, w) as colour
    images, a float (n', 3, h, w) tensor in [0, 1]; values outside [0, num_classes), the ignored -1
    included, are black.  A device tensor is coloured on the device (msl_colorize) and the result stays
    there; numpy arrays and CPU tensors are coloured with numpy."""
    if torch.is_tensor(mask) and mask.is_cuda:
        from .. import ops
        n = min(int(mask.shape[0]), int(num_images))
        key = (int(num_classes), mask.device)
        if key not in _DEVICE_PALETTES:
            # the byte -> float table is divided on the host: the device's fp32 division by 255 rounds some
            # bytes one ulp away from the reference's
            _DEVICE_PALETTES[key] = (torch.from_numpy(_palette_of(int(num_classes))).to(mask.device),
                                     torch.arange(256, dtype=torch.float32).div_(255.0).to(mask.device))
        pal, unit = _DEVICE_PALETTES[key]
        m = mask[:n]
        if m.dtype not in (torch.int64, torch.int32):
            m = m.to(torch.int64)
        return unit[ops.colorize(m, pal).permute(0, 3, 1, 2).long()]
    if torch.is_tensor(mask):
        mask = mask.data.cpu().numpy()
    mask = np.asarray(mask)
    n = min(mask.shape[0], int(num_images))
    m = mask[:n].astype(np.int64)
    pal = np.concatenate([_palette_of(int(num_classes)), np.zeros((1, 3), np.uint8)])
    outputs = pal[np.where((m >= 0) & (m < num_classes), m, len(pal) - 1)]
    return torch.from_numpy(outputs.transpose([0, 3, 1, 2]).astype("float32")).div_(255.0)


def inv_preprocess(imgs, num_images=1, img_mean=IMG_MEAN, numpy_transform=False):
    """cityscapes_Dataset.py:332-350: the network input as something to look at - with numpy_transform
    the channels flipped back (BGR -> RGB), then the whole batch normalised to [0, 1) by its own minimum
    and maximum, (x - min) / (max - min + 1e-5).  As in the reference num_images and img_mean are not
    read and, without the channel flip, `imgs` is normalised in place.  Torch ops on the tensor's own
    device; numpy input is accepted."""
    if not torch.is_tensor(imgs):
        imgs = torch.from_numpy(np.asarray(imgs))
    if numpy_transform:
        imgs = imgs.flip(1)
    lo, hi = float(imgs.min()), float(imgs.max())
    imgs.clamp_(min=lo, max=hi)
    imgs.add_(-lo).div_(hi - lo + 1e-5)
    return imgs
