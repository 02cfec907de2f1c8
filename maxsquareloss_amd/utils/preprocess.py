"""Device-side input pipeline: the reference loaders' final transforms as HIP kernels (§8f row 4).

The reference converts every image and label on the host in numpy
(datasets/cityscapes_Dataset.py:245-264) and ships fp32 CHW images and fp32
labels; here the uint8 image / id map is copied as is (4x / 8x fewer PCIe
bytes) and converted on the GPU (csrc/preprocess.hip), bit-exact:
  image_transform:  RGB uint8 HWC -> BGR - IMG_MEAN fp32 (1,3,H,W)   (_img_transform, :245-251)
  label_transform:  ids uint8 HW  -> trainIds int64 (1,H,W), -1 = ignore
                    (id2trainId + the 16 / 13-class remaps, :124-155, 260-264)
both with the optional horizontal mirror of the random_mirror augmentation.

resize_image / resize_label run what comes before that in the reference's _train_sync_transform /
_val_sync_transform (:173-243) - Image.transpose, crop, resize with BICUBIC / NEAREST - byte-exact
against Pillow on the device (csrc/resample.hip, tables from utils/resample.py), ending in the same
two transforms.

png_unfilter undoes the PNG scanline filters of one byte lane on the device (csrc/png.hip): SYNTHIA's
16-bit label PNGs are inflated on the host (utils/png.py) and reconstructed here, ahead of resize_label.

jpeg_reconstruct finishes a baseline JPEG whose scan the host Huffman-decoded (utils/jpeg.py decode_file):
dequantisation, inverse DCT, chroma upsampling and YCbCr -> RGB on the device (csrc/jpeg.hip), the uint8
(H, W, 3) image Pillow decodes, ahead of resize_image.
"""
import ctypes

import numpy as np
import torch

from .. import hip
from . import jpeg, resample
from .synthetic import IMG_MEAN

# id -> trainId tables of the three loaders (values not listed map to the ignore label -1)
CITYSCAPES_ID_TO_TRAINID = {7: 0, 8: 1, 11: 2, 12: 3, 13: 4, 17: 5, 19: 6, 20: 7, 21: 8, 22: 9, 23: 10,
                            24: 11, 25: 12, 26: 13, 27: 14, 28: 15, 31: 16, 32: 17, 33: 18}  # cityscapes_Dataset.py:124-130
GTA5_ID_TO_TRAINID = dict(CITYSCAPES_ID_TO_TRAINID)  # gta5_Dataset.py:73-75 (the same 19 labelled ids)
SYNTHIA_ID_TO_TRAINID = {1: 10, 2: 2, 3: 0, 4: 1, 5: 4, 6: 8, 7: 5, 8: 13, 9: 7, 10: 11, 11: 18, 12: 17,
                         15: 6, 16: 9, 17: 12, 18: 14, 19: 15, 20: 16, 21: 3}  # synthia_Dataset.py:56-58
SET_16 = [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 15, 17, 18]  # cityscapes_Dataset.py:132
SET_13 = [0, 1, 2, 6, 7, 8, 10, 11, 12, 13, 15, 17, 18]            # cityscapes_Dataset.py:136


def build_lut(dataset, class_16=False, class_13=False):
    """int32[256]: uint8 label id -> the trainId the reference's id2trainId produces."""
    table = {"cityscapes": CITYSCAPES_ID_TO_TRAINID, "gta5": GTA5_ID_TO_TRAINID,
             "synthia": SYNTHIA_ID_TO_TRAINID}[dataset.lower()]
    lut = np.full(256, -1, np.int32)
    for k, v in table.items():
        lut[k] = v
    for on, sub in ((class_16, SET_16), (class_13, SET_13)):
        if on:
            remap = {t: i for i, t in enumerate(sub)}
            lut = np.array([remap.get(int(t), -1) for t in lut], np.int32)
    return lut


def image_transform(rgb, mirror=False, mean=IMG_MEAN):
    """rgb: uint8 (H, W, 3) on the GPU -> (1, 3, H, W) fp32 BGR - mean."""
    if not rgb.is_cuda or rgb.dtype != torch.uint8 or rgb.dim() != 3 or rgb.size(2) != 3:
        raise hip.MSLError(f"image_transform: expected a CUDA uint8 (H, W, 3) tensor, got {tuple(rgb.shape)} "
                           f"{rgb.dtype} {rgb.device}")
    rgb = rgb.contiguous()
    h, w = rgb.shape[:2]
    out = torch.empty((1, 3, h, w), dtype=torch.float32, device=rgb.device)
    m = [float(np.float32(v)) for v in mean]
    hip.check(hip.load().msl_image_transform(rgb.data_ptr(), h, w, int(bool(mirror)), m[0], m[1], m[2],
                                             out.data_ptr(), hip.stream_ptr()), "msl_image_transform")
    return out


_LUTS = {}


def label_transform(ids, lut, mirror=False):
    """ids: uint8 (H, W) on the GPU, lut: int32[256] (build_lut) -> (1, H, W) int64 trainIds."""
    if not ids.is_cuda or ids.dtype != torch.uint8 or ids.dim() != 2:
        raise hip.MSLError(f"label_transform: expected a CUDA uint8 (H, W) tensor, got {tuple(ids.shape)} "
                           f"{ids.dtype} {ids.device}")
    ids = ids.contiguous()
    key = (ids.device.index, np.asarray(lut, np.int32).tobytes())
    dlut = _LUTS.get(key)
    if dlut is None:
        dlut = torch.from_numpy(np.asarray(lut, np.int32).copy()).to(ids.device)
        if dlut.numel() != 256:
            raise hip.MSLError("label_transform: the table must have 256 entries")
        _LUTS[key] = dlut
    h, w = ids.shape
    out = torch.empty((1, h, w), dtype=torch.int64, device=ids.device)
    hip.check(hip.load().msl_label_transform(ids.data_ptr(), h, w, int(bool(mirror)), dlut.data_ptr(),
                                             out.data_ptr(), hip.stream_ptr()), "msl_label_transform")
    return out


# ---------------------------------------------------------------------------- Pillow-exact resampling
_TABLES = {}  # (device index, kind, in, out) -> (host bounds or None, device table, ksize)


def _bicubic_tables(in_size, out_size, device):
    """Host bounds + the device table of msl_resize_bicubic_rgb ([2 + ksize][out]: first taps, tap
    counts, coefficients), cached."""
    key = (device.index, "bicubic", int(in_size), int(out_size))
    got = _TABLES.get(key)
    if got is None:
        bounds, coeffs, ksize = resample.bicubic_table(in_size, out_size)
        if ksize > resample.MAX_KSIZE:
            raise hip.MSLError(f"resize_image: {in_size} -> {out_size} needs {ksize} taps per output; the "
                               f"kernels take at most {resample.MAX_KSIZE}")
        host = np.ascontiguousarray(bounds, np.int32)
        dev = torch.from_numpy(np.ascontiguousarray(np.concatenate([bounds, coeffs], axis=1).T, np.int32)).to(device)
        got = _TABLES[key] = (host, dev, ksize)
    return got


def _nearest_table(in_size, out_size, device):
    key = (device.index, "nearest", int(in_size), int(out_size))
    got = _TABLES.get(key)
    if got is None:
        got = _TABLES[key] = torch.from_numpy(np.array(resample.nearest_table(in_size, out_size), np.int32)).to(device)
    return got


def _crop_of(crop, h, w, what):
    if crop is None:
        return 0, 0, w, h
    x1, y1, cw, ch = (int(v) for v in crop)
    if x1 < 0 or y1 < 0 or cw < 1 or ch < 1 or x1 + cw > w or y1 + ch > h:
        raise hip.MSLError(f"{what}: crop {tuple(crop)} leaves the {w}x{h} source")
    return x1, y1, cw, ch


def resize_image(rgb, out_wh, crop=None, mirror=False, mean=IMG_MEAN, as_uint8=False):
    """Pillow's `img.transpose(FLIP_LEFT_RIGHT)` (if mirror), `img.crop((x1, y1, x1+w, y1+h))` (if
    crop = (x1, y1, w, h), in the mirrored image) and `img.resize(out_wh, Image.BICUBIC)`, byte-exact,
    on the device (csrc/resample.hip).  rgb: uint8 (H, W, 3) on the GPU; out_wh = (width, height).
    Returns (1, 3, oh, ow) fp32 BGR - mean (the reference's _img_transform, written by the last
    resampling pass), or with as_uint8 the resized uint8 (oh, ow, 3) image."""
    if not rgb.is_cuda or rgb.dtype != torch.uint8 or rgb.dim() != 3 or rgb.size(2) != 3:
        raise hip.MSLError(f"resize_image: expected a CUDA uint8 (H, W, 3) tensor, got {tuple(rgb.shape)} "
                           f"{rgb.dtype} {rgb.device}")
    rgb = rgb.contiguous()
    h, w = rgb.shape[:2]
    ow, oh = int(out_wh[0]), int(out_wh[1])
    x1, y1, cw, ch = _crop_of(crop, h, w, "resize_image")
    lib = hip.load()
    xb, xk, xks = _bicubic_tables(cw, ow, rgb.device) if ow != cw else (None, None, 0)
    yb, yk, yks = _bicubic_tables(ch, oh, rgb.device) if oh != ch else (None, None, 0)
    ws, ws_bytes = None, 0
    if xk is not None and yk is not None:
        ws_bytes = lib.msl_resize_workspace(ch, ow)
        ws = hip.workspace(ws_bytes, rgb.device)
    if as_uint8:
        out = torch.empty((oh, ow, 3), dtype=torch.uint8, device=rgb.device)
        out_u8, out_f32 = out.data_ptr(), None
    else:
        out = torch.empty((1, 3, oh, ow), dtype=torch.float32, device=rgb.device)
        out_u8, out_f32 = None, out.data_ptr()
    m = [float(np.float32(v)) for v in mean]
    hip.check(lib.msl_resize_bicubic_rgb(
        rgb.data_ptr(), h, w, x1, y1, cw, ch, int(bool(mirror)),
        None if xb is None else xb.ctypes.data, hip.ptr(xk), xks,
        None if yb is None else yb.ctypes.data, hip.ptr(yk), yks, ow, oh, out_u8, out_f32, m[0], m[1], m[2],
        hip.ptr(ws), ws_bytes, hip.stream_ptr()), "msl_resize_bicubic_rgb")
    return out


def _device_lut(lut, device):
    key = (device.index, np.asarray(lut, np.int32).tobytes())
    dlut = _LUTS.get(key)
    if dlut is None:
        dlut = torch.from_numpy(np.asarray(lut, np.int32).copy()).to(device)
        if dlut.numel() != 256:
            raise hip.MSLError("the id -> trainId table must have 256 entries")
        _LUTS[key] = dlut
    return dlut


def resize_label(ids, out_wh, lut, crop=None, mirror=False):
    """The label side of resize_image: mirror, crop, `mask.resize(out_wh, Image.NEAREST)`, byte-exact,
    then the id -> trainId table.  ids: uint8 (H, W) on the GPU.  With lut (int32[256], build_lut)
    returns (1, oh, ow) int64 trainIds; with lut=None the resized uint8 (oh, ow) id map."""
    if not ids.is_cuda or ids.dtype != torch.uint8 or ids.dim() != 2:
        raise hip.MSLError(f"resize_label: expected a CUDA uint8 (H, W) tensor, got {tuple(ids.shape)} "
                           f"{ids.dtype} {ids.device}")
    ids = ids.contiguous()
    h, w = ids.shape
    ow, oh = int(out_wh[0]), int(out_wh[1])
    x1, y1, cw, ch = _crop_of(crop, h, w, "resize_label")
    xtab = _nearest_table(cw, ow, ids.device) if ow != cw else None
    ytab = _nearest_table(ch, oh, ids.device) if oh != ch else None
    if lut is None:
        out = torch.empty((oh, ow), dtype=torch.uint8, device=ids.device)
        dlut, out_u8, out_i64 = None, out.data_ptr(), None
    else:
        out = torch.empty((1, oh, ow), dtype=torch.int64, device=ids.device)
        dlut, out_u8, out_i64 = _device_lut(lut, ids.device), None, out.data_ptr()
    hip.check(hip.load().msl_resize_nearest_label(
        ids.data_ptr(), h, w, x1, y1, cw, ch, int(bool(mirror)), hip.ptr(xtab), hip.ptr(ytab), ow, oh,
        hip.ptr(dlut), out_u8, out_i64, hip.stream_ptr()), "msl_resize_nearest_label")
    return out


# ---------------------------------------------------------------------------- PNG unfilter (SYNTHIA labels)
def png_unfilter(plane_or_scan, bpp=1, lane=0):
    """Inflated PNG scanlines -> byte `lane` of every reconstructed pixel (csrc/png.hip, one launch on the
    current stream).  plane_or_scan: CUDA uint8 (h, 1 + w * bpp), each row its filter byte and the filtered
    bytes (utils/png.py read_scanlines; with the defaults the compacted plane of lane_plane).  Returns CUDA
    uint8 (h, w), what utils/png.py unfilter_lane gives on the host."""
    t = plane_or_scan
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.uint8 or t.dim() != 2:
        raise hip.MSLError("png_unfilter: expected a CUDA uint8 (h, 1 + w * bpp) tensor of scanlines")
    bpp, lane = int(bpp), int(lane)
    if bpp < 1 or t.size(1) < 1 + bpp or (t.size(1) - 1) % bpp:
        raise hip.MSLError(f"png_unfilter: rows of {t.size(1)} bytes are not a filter byte and whole pixels of "
                           f"{bpp} bytes")
    if t.stride(1) != 1:
        t = t.contiguous()
    h, w = t.size(0), (t.size(1) - 1) // bpp
    out = torch.empty((h, w), dtype=torch.uint8, device=t.device)
    hip.check(hip.load().msl_png_unfilter_lane(t.data_ptr(), h, w, bpp, lane, t.stride(0), out.data_ptr(),
                                               hip.stream_ptr()), "msl_png_unfilter_lane")
    return out


# ---------------------------------------------------------------------------- JPEG reconstruction (NTHU images)
def jpeg_reconstruct(payload, header=None):
    """The device half of the JPEG decode (csrc/jpeg.hip, two launches on the current stream).  payload: the
    CUDA uint8 1-D tensor utils/jpeg.py decode_file made on the host - header, tables, coefficients.  header:
    the payload's hip.JpegHeader as read on the host (utils/jpeg.py header_of; the loaders pass it with the
    item's plan); without it the header's bytes are copied back from the device, which waits for the stream.
    Returns CUDA uint8 (H, W, 3) RGB, what utils/jpeg.py reconstruct gives on the host and Pillow for the file."""
    t = payload
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.uint8 or t.dim() != 1 or t.numel() <= jpeg.COEF_AT:
        raise hip.MSLError("jpeg_reconstruct: expected a CUDA uint8 1-D payload (utils/jpeg.py decode_file)")
    if not t.is_contiguous() or t.data_ptr() % 16:
        t = t.clone(memory_format=torch.contiguous_format)
    if header is None:
        header = jpeg.header_of(t[:jpeg.HEADER_BYTES].cpu())
    lib = hip.load()
    hp = ctypes.addressof(header)
    elems = lib.msl_jpeg_coef_elems(hp)
    if elems == 0 or t.numel() < jpeg.COEF_AT + 2 * elems:
        raise hip.MSLError(f"jpeg_reconstruct: a payload of {t.numel()} bytes does not hold the {elems} coefficients "
                           "of its header")
    ws_bytes = lib.msl_jpeg_workspace(hp)
    ws = hip.workspace(ws_bytes, t.device)
    out = torch.empty((header.height, header.width, 3), dtype=torch.uint8, device=t.device)
    hip.check(lib.msl_jpeg_reconstruct(t.data_ptr() + jpeg.COEF_AT, t.data_ptr() + jpeg.HEADER_BYTES, hp,
                                       out.data_ptr(), ws.data_ptr(), ws_bytes, hip.stream_ptr()),
              "msl_jpeg_reconstruct")
    return out
