"""Baseline JPEG decode for the NTHU cross-city images (crosscity_Dataset.py:74 of the reference:
`Image.open(image_path).convert("RGB")` on 2048x1024 JPEGs), split where the serial part ends.

  host    the marker parser and the Huffman decode (csrc/jpeg_host.h behind msl_jpeg_entropy_decode; ctypes
          releases the GIL, so the loaders' decoding threads run it in parallel) -> quantised coefficients in
          natural order, the quantisation tables, a header;
  device  dequantisation, libjpeg's JDCT_ISLOW inverse DCT, libjpeg-turbo's fancy chroma upsampling and the
          YCbCr -> RGB fixed point (csrc/jpeg.hip, utils/preprocess.py jpeg_reconstruct), byte-exact against
          Pillow.

decode_file packs what the host made into ONE uint8 array - the payload - that travels through the loaders'
pinned staging slot in place of the decoded image:
    [0, 256)                    the msl_jpeg_header (hip.JpegHeader), zero padded
    [256, 768)                  the tables, uint16 [4][64]
    [768, 768 + 2 * elems)      the coefficients, int16 [component][block row][block col][64]
reconstruct is the numpy restatement of the device half - the role utils/resample.py plays for the resize and
utils/png.py's unfilter_lane for the PNG filters: what the kernels must equal bit for bit, the tests and the
loaders' host_transform use it, no training path does.
"""
import ctypes

import numpy as np

from .. import hip

HEADER_BYTES, QUANT_BYTES = 256, 512
COEF_AT = HEADER_BYTES + QUANT_BYTES
OK, ERR_SHAPE, ERR_ARG = 0, -1, -3
EXTENSIONS = (".jpg", ".jpeg")

assert ctypes.sizeof(hip.JpegHeader) <= HEADER_BYTES


def _bytes_of(path_or_bytes):
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        return bytes(path_or_bytes)
    with open(path_or_bytes, "rb") as f:
        return f.read()


def info(path_or_bytes):
    """(status, header): msl_jpeg_info on a file or its bytes - MSL_OK, MSL_ERR_SHAPE for a valid file
    the split decoder does not take, MSL_ERR_ARG for a corrupt one."""
    data = _bytes_of(path_or_bytes)
    header = hip.JpegHeader()
    lib = hip.load(require_gpu=False)
    return lib.msl_jpeg_info(data, len(data), ctypes.addressof(header)), header


def decode_file(path_or_bytes, alloc=None):
    """The host half: the payload (uint8, layout above) of a JPEG file or its bytes, or None when the decoder
    refuses the file - unsupported (progressive, CMYK, RGB-coded, ...) or corrupt; the caller then decodes with
    Pillow, as before.  alloc(nbytes) -> a contiguous uint8 array of that size: the caller's buffer for the payload
    (the loaders pass their pinned staging slot, so nothing is copied afterwards); default a new array.  Host
    only, thread-safe."""
    data = _bytes_of(path_or_bytes)
    lib = hip.load(require_gpu=False)
    header = hip.JpegHeader()
    if lib.msl_jpeg_info(data, len(data), ctypes.addressof(header)) != OK:
        return None
    elems = lib.msl_jpeg_coef_elems(ctypes.addressof(header))
    if elems // 64 > 4 * len(data):
        # a block costs at least two bits (a DC code and an end-of-block code): the file cannot hold the blocks its
        # size field claims - a corrupt header, refused before it is given gigabytes
        return None
    payload = np.empty(COEF_AT + 2 * elems, np.uint8) if alloc is None else alloc(COEF_AT + 2 * elems)
    payload[:COEF_AT] = 0
    base = payload.ctypes.data
    if lib.msl_jpeg_entropy_decode(data, len(data), base, base + COEF_AT, elems, base + HEADER_BYTES) != OK:
        return None
    return payload


def is_payload(x):
    """Whether a decoded item is a payload (1-D) and not an (H, W, 3) image."""
    return getattr(x, "ndim", None) == 1 or (hasattr(x, "dim") and x.dim() == 1)


def size_of(decoded):
    """(height, width) of a decoded image: its header's if it is a payload, its own shape otherwise."""
    if is_payload(decoded):
        h = header_of(decoded)
        return h.height, h.width
    return tuple(decoded.shape[:2])


def header_of(payload):
    """A copy of the payload's header (payload: a numpy array or a CPU tensor)."""
    raw = payload[:HEADER_BYTES]
    raw = raw.numpy() if hasattr(raw, "numpy") else np.asarray(raw)
    return hip.JpegHeader.from_buffer_copy(np.ascontiguousarray(raw, np.uint8).tobytes()[:ctypes.sizeof(hip.JpegHeader)])


def split(payload):
    """(header, quant uint16 (4, 64), [coefficients int16 (blocks_h, blocks_w, 64) per component])."""
    payload = np.ascontiguousarray(payload, np.uint8)
    h = header_of(payload)
    quant = payload[HEADER_BYTES:COEF_AT].view(np.uint16).reshape(4, 64)
    coef = payload[COEF_AT:].view(np.int16)
    comps = []
    for c in range(h.ncomp):
        cc = h.comp[c]
        n = cc.blocks_w * cc.blocks_h * 64
        comps.append(coef[cc.offset:cc.offset + n].reshape(cc.blocks_h, cc.blocks_w, 64))
    return h, quant, comps


# ------------------------------------------------------------------------------------ the device half, in numpy
def _descale(x, n):
    """DESCALE of an int64 sum the way the kernel holds it: modulo 2^32 as int32, then the arithmetic shift (the
    wrap never happens on a block an encoder made: csrc/jpeg.hip)."""
    x = x + (1 << (n - 1))
    x = ((x + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
    return x >> n


def _pass(x, shift):
    """jidctint.c's 1-D pass along the last axis of int64 x (..., 8): CONST_BITS 13, the twelve constants."""
    i0, i1, i2, i3, i4, i5, i6, i7 = (x[..., k] for k in range(8))
    z1 = (i2 + i6) * 4433
    t2, t3 = z1 - i6 * 15137, z1 + i2 * 6270
    t0, t1 = (i0 + i4) << 13, (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i7, i5, i3, i1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, z5 - z3 * 16069, z5 - z4 * 3196
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    return np.stack([_descale(v, shift) for v in (t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1,
                                                  t11 - a2, t10 - a3)], -1)


def idct_plane(blocks, table):
    """blocks int16 (bh, bw, 64), table uint16 (64,) -> the uint8 plane (8 bh, 8 bw) of whole blocks: dequantise,
    the column pass descaled by 11, the row pass by 18, clamp(x + 128, 0, 255)."""
    x = (blocks.astype(np.int64) * table.astype(np.int64)).reshape(blocks.shape[:-1] + (8, 8))  # [row][col]
    ws = _pass(x.swapaxes(-1, -2), 11).swapaxes(-1, -2)
    out = np.clip(_pass(ws, 18) + 128, 0, 255).astype(np.uint8)
    bh, bw = out.shape[:2]
    return out.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _upsample_h2v1(p):
    """libjpeg-turbo's h2v1_fancy_upsample on int64 (h, w) -> (h, 2 w)."""
    prev = np.concatenate([p[:, :1], p[:, :-1]], 1)
    nxt = np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out = np.empty((p.shape[0], 2 * p.shape[1]), np.int64)
    out[:, 0::2] = (3 * p + prev + 1) >> 2
    out[:, 1::2] = (3 * p + nxt + 2) >> 2
    out[:, 0], out[:, -1] = p[:, 0], p[:, -1]
    return out


def _upsample_h2v2(p):
    """libjpeg-turbo's h2v2_fancy_upsample on int64 (h, w) -> (2 h, 2 w)."""
    h, w = p.shape
    out = np.empty((2 * h, 2 * w), np.int64)
    for v, far in ((0, np.concatenate([p[:1], p[:-1]])), (1, np.concatenate([p[1:], p[-1:]]))):
        cs = 3 * p + far
        last = np.concatenate([cs[:, :1], cs[:, :-1]], 1)
        nxt = np.concatenate([cs[:, 1:], cs[:, -1:]], 1)
        even, odd = (3 * cs + last + 8) >> 4, (3 * cs + nxt + 7) >> 4
        even[:, 0], odd[:, -1] = (4 * cs[:, 0] + 8) >> 4, (4 * cs[:, -1] + 7) >> 4
        out[v::2, 0::2], out[v::2, 1::2] = even, odd
    return out


def _fix(x):
    return int(x * 65536 + 0.5)


def reconstruct(payload):
    """The payload -> uint8 (H, W, 3) RGB: what Pillow's `Image.open(f).convert("RGB")` gives for the file."""
    h, quant, comps = split(payload)
    W, H = h.width, h.height
    planes = []
    for c, blocks in enumerate(comps):
        cc = h.comp[c]
        p = idct_plane(blocks, quant[cc.tq]).astype(np.int64)
        if h.ncomp == 3 and c > 0 and (h.hmax, h.vmax) != (1, 1):
            cw, ch = -(-W * cc.h // h.hmax), -(-H * cc.v // h.vmax)
            p = p[:ch, :cw]                      # padding samples never enter a filter
            if cw <= 2:                          # libjpeg selects the box upsamplers for such a plane
                p = p.repeat(2, axis=1)
                p = p.repeat(2, axis=0) if h.vmax == 2 else p
            else:
                p = _upsample_h2v2(p) if h.vmax == 2 else _upsample_h2v1(p)
        planes.append(p[:H, :W])
    if h.ncomp == 1:
        return np.ascontiguousarray(np.stack([planes[0]] * 3, -1).astype(np.uint8))
    y, cb, cr = planes[0], planes[1] - 128, planes[2] - 128
    r = y + ((_fix(1.402) * cr + 32768) >> 16)
    b = y + ((_fix(1.772) * cb + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb + 32768 - _fix(0.71414) * cr) >> 16)
    return np.ascontiguousarray(np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8))


def decode(path_or_bytes):
    """uint8 (H, W, 3): decode_file + reconstruct, all on the host; None for a file the decoder refuses."""
    payload = decode_file(path_or_bytes)
    return None if payload is None else reconstruct(payload)
