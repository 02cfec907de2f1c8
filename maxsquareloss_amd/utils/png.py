"""A minimal PNG scanline reader for SYNTHIA's 16-bit label PNGs (synthia_Dataset.py:73-75 of the
reference: `np.uint8(imageio.imread(path, format='PNG-FI')[:, :, 0])`, the LOW byte of R).

Pillow opens a 16-bit RGB PNG as 8-bit RGB and keeps the high byte of every sample, so the class ids
are lost; imageio's FreeImage plugin is not a dependency.  Two facts about PNG make a reader of a
few lines enough:
  - inflate is in the standard library (zlib.decompress releases the GIL, so it runs on the
    decode-ahead threads);
  - the scanline filters work on bytes bpp apart - byte i of a row from byte i - bpp of the same row
    and bytes i, i - bpp of the row above - so the bytes of one lane (byte k of every pixel) depend
    only on that lane.  One byte per pixel is a bpp = 1 problem on one bpp-th of the data.
read_scanlines parses and inflates, lane_plane slices the lane out, and the unfilter runs on the device
(utils/preprocess.py png_unfilter, csrc/png.hip).  unfilter_lane is its numpy restatement, the role
utils/resample.py plays for the resize: the loaders' host_transform and the tests use it, no training
path does.
"""
import collections
import struct
import zlib

import numpy as np

from ..hip import MSLError

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}  # colour type -> samples per pixel (3 = palette, refused)

PNGInfo = collections.namedtuple("PNGInfo", "width height depth colour channels bpp")


def _fail(name, why):
    raise MSLError(f"{name}: {why}")


def read_scanlines(path_or_bytes):
    """(info, scan): the IHDR fields as a PNGInfo and the inflated scanlines as uint8 (h, 1 + w * bpp),
    each row its filter byte followed by its filtered bytes.  Checks the signature and every chunk's CRC,
    concatenates all IDAT chunks, skips ancillary chunks.  MSLError (naming the file and the reason) for an
    interlaced file, a palette image, a bit depth under 8, a truncated or over-long stream, a bad CRC and a
    filter byte above 4."""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        name, data = "<png bytes>", bytes(path_or_bytes)
    else:
        name = str(path_or_bytes)
        with open(path_or_bytes, "rb") as f:
            data = f.read()
    if data[:8] != SIGNATURE:
        _fail(name, "not a PNG file (bad signature)")
    pos, info, idat, ended = 8, None, [], False
    while pos < len(data):
        if pos + 8 > len(data):
            _fail(name, "truncated file: a chunk header is cut short")
        length, ctype = struct.unpack(">I4s", data[pos:pos + 8])
        end = pos + 12 + length
        if end > len(data):
            _fail(name, f"truncated file: chunk {ctype!r} runs past the end")
        body = data[pos + 8:pos + 8 + length]
        if zlib.crc32(data[pos + 4:pos + 8 + length]) != struct.unpack(">I", data[end - 4:end])[0]:
            _fail(name, f"bad CRC in chunk {ctype!r}")
        pos = end
        if info is None and ctype != b"IHDR":
            _fail(name, "the first chunk is not IHDR")
        if ctype == b"IHDR":
            if info is not None or length != 13:
                _fail(name, "malformed IHDR")
            w, h, depth, colour, comp, filt, interlace = struct.unpack(">IIBBBBB", body)
            if colour == 3:
                _fail(name, "palette images (colour type 3) are not supported")
            if colour not in CHANNELS:
                _fail(name, f"unknown colour type {colour}")
            if depth < 8:
                _fail(name, f"bit depth {depth} is not supported (8 or 16 only)")
            if depth not in (8, 16):
                _fail(name, f"bad bit depth {depth}")
            if interlace != 0:
                _fail(name, "interlaced (Adam7) files are not supported")
            if comp != 0 or filt != 0 or w < 1 or h < 1:
                _fail(name, "malformed IHDR")
            ch = CHANNELS[colour]
            info = PNGInfo(w, h, depth, colour, ch, ch * depth // 8)
        elif ctype == b"IDAT":
            idat.append(body)
        elif ctype == b"IEND":
            ended = True
            break
        elif not ctype[0] & 0x20:
            _fail(name, f"unknown critical chunk {ctype!r}")
    if info is None or not ended:
        _fail(name, "truncated file: no IEND chunk")
    if not idat:
        _fail(name, "no IDAT chunk")
    row = 1 + info.width * info.bpp
    want = info.height * row
    z = zlib.decompressobj()
    try:
        raw = z.decompress(b"".join(idat), want + 1)
    except zlib.error as e:
        raise MSLError(f"{name}: the image data does not inflate ({e})") from e
    if len(raw) > want:
        _fail(name, f"over-long stream: more than the {want} bytes of {info.height} scanlines")
    if len(raw) < want or not z.eof:
        _fail(name, f"truncated stream: {len(raw)} of {want} scanline bytes")
    scan = np.frombuffer(raw, np.uint8).reshape(info.height, row)
    worst = int(scan[:, 0].max())
    if worst > 4:
        _fail(name, f"filter byte {worst} in row {int(np.argmax(scan[:, 0] > 4))} (0..4 are defined)")
    return info, scan


def lane_plane(scan, bpp, lane):
    """uint8 (h, 1 + w), contiguous: the filter byte and byte `lane` of every pixel of scan (h, 1 + w * bpp)."""
    bpp, lane = int(bpp), int(lane)
    if scan.ndim != 2 or bpp < 1 or not 0 <= lane < bpp or (scan.shape[1] - 1) % bpp or scan.shape[1] < 1 + bpp:
        raise MSLError(f"lane_plane: scanlines {scan.shape} do not hold lane {lane} of {bpp}-byte pixels")
    out = np.empty((scan.shape[0], 1 + (scan.shape[1] - 1) // bpp), np.uint8)
    out[:, 0] = scan[:, 0]
    out[:, 1:] = scan[:, 1 + lane::bpp]
    return out


def label_lane(info):
    """The lane `np.uint8(imread(...)[:, :, 0])` keeps: the low byte of the first channel - PNG samples are
    big-endian, so byte 1 at depth 16 and byte 0 at depth 8."""
    return 1 if info.depth == 16 else 0


def unfilter_lane(plane):
    """plane uint8 (h, 1 + w) (lane_plane) -> the reconstructed bytes uint8 (h, w), per the PNG specification
    (None, Sub, Up, Average = floor((a + b) / 2), Paeth with ties in the order a, b, c; mod 256; neighbours
    outside the image 0; a filter byte above 4 as None, like the device kernel).  numpy, one vector op set
    per anti-diagonal: pixel (r, x) sits on diagonal r + x and needs only the two diagonals before it."""
    plane = np.asarray(plane, np.uint8)
    h, w = plane.shape[0], plane.shape[1] - 1
    ft = plane[:, 0].astype(np.int32)
    ft[ft > 4] = 0
    # skewed storage: S[r, r + x + 1] = pixel (r, x), one leading zero column (the left neighbour of x = 0)
    # and one leading zero row (the row above row 0); diagonal t is then column t + 1 of rows 1..h
    F = np.zeros((h + 1, w + h + 1), np.int32)
    rows = np.arange(h)
    cols = rows[:, None] + np.arange(w)[None, :] + 1
    F[rows[:, None] + 1, cols] = plane[:, 1:]
    S = np.zeros_like(F)
    live = np.zeros((h + 1, w + h + 1), bool)
    live[rows[:, None] + 1, cols] = True
    ftc = np.concatenate([[0], ft])
    is1, is2, is3, is4 = (ftc == k for k in (1, 2, 3, 4))
    for t in range(1, w + h):
        a = S[1:, t - 1]                 # (r, x - 1): same row, previous diagonal
        b = S[:-1, t - 1]                # (r - 1, x): row above, previous diagonal
        c = S[:-1, t - 2] if t >= 2 else np.zeros(h, np.int32)  # (r - 1, x - 1): two diagonals back
        pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        pred = np.where(is1[1:], a, np.where(is2[1:], b, np.where(is3[1:], (a + b) >> 1,
                                                                  np.where(is4[1:], paeth, 0))))
        S[1:, t] = np.where(live[1:, t], (F[1:, t] + pred) & 0xff, 0)
    return np.ascontiguousarray(S[rows[:, None] + 1, cols].astype(np.uint8))
