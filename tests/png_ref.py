"""Helpers of the SYNTHIA / PNG tests (not collected): a scalar restatement of the PNG specification's
unfilter - the oracle of test_synthia.py and test_gpu_synthia.py, a plain double loop that shares nothing
with utils/png.py - a small PNG writer that applies a chosen filter type per row (forward filtering reads
original bytes only, so it cannot share a bug with a decoder), and a tiny SYNTHIA tree."""
import os
import struct
import zlib

import numpy as np

CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}


def scalar_unfilter(scan, bpp):
    """scan uint8 (h, 1 + n) -> the reconstructed bytes uint8 (h, n), PNG specification section 9.2/9.4.
    A filter byte above 4 is taken as None (the device kernel's defined behaviour)."""
    rows = [bytes(r) for r in np.asarray(scan, np.uint8)]
    n = len(rows[0]) - 1
    prev = bytearray(n)
    out = []
    for r in rows:
        ft, line = r[0], bytearray(r[1:])
        for i in range(n):
            a = line[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            if ft == 1:
                pred = a
            elif ft == 2:
                pred = b
            elif ft == 3:
                pred = (a + b) // 2
            elif ft == 4:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            else:
                pred = 0
            line[i] = (line[i] + pred) & 0xff
        out.append(bytes(line))
        prev = line
    return np.frombuffer(b"".join(out), np.uint8).reshape(len(rows), n)


def scalar_lane(scan, bpp, lane):
    return np.ascontiguousarray(scalar_unfilter(scan, bpp)[:, lane::bpp])


def filter_rows(raw, bpp, filters):
    """raw uint8 (h, n) original bytes -> scanlines uint8 (h, 1 + n) with filters[r] applied to row r."""
    raw = np.asarray(raw, np.uint8).astype(np.int32)
    h, n = raw.shape
    a = np.zeros_like(raw)
    a[:, bpp:] = raw[:, :-bpp] if n > bpp else 0
    b = np.zeros_like(raw)
    b[1:] = raw[:-1]
    c = np.zeros_like(raw)
    c[1:, bpp:] = raw[:-1, :-bpp] if n > bpp else 0
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    preds = [np.zeros_like(raw), a, b, (a + b) // 2, paeth]
    scan = np.empty((h, 1 + n), np.uint8)
    for r, ft in enumerate(filters):
        scan[r, 0] = ft
        scan[r, 1:] = (raw[r] - preds[ft][r]) & 0xff
    return scan


def chunk(ctype, body):
    return struct.pack(">I", len(body)) + ctype + body + struct.pack(">I", zlib.crc32(ctype + body))


def png_bytes(samples, depth, colour, filters, idat_chunks=1, interlace=0, extra=()):
    """A PNG file: samples (h, w, channels) uint8 / uint16 (big-endian on file), filters[r] per row, the
    compressed stream split into idat_chunks IDAT chunks, `extra` chunks between IHDR and IDAT."""
    samples = np.asarray(samples)
    h, w, ch = samples.shape
    assert ch == CHANNELS[colour]
    raw = (samples.astype(">u2") if depth == 16 else samples.astype(np.uint8)).tobytes()
    bpp = ch * depth // 8
    scan = filter_rows(np.frombuffer(raw, np.uint8).reshape(h, w * bpp), bpp, filters)
    z = zlib.compress(scan.tobytes(), 6)
    cuts = [len(z) * k // idat_chunks for k in range(idat_chunks + 1)]
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour, 0, 0, interlace))
    for e in extra:
        out += e
    for lo, hi in zip(cuts, cuts[1:]):
        out += chunk(b"IDAT", z[lo:hi])
    return out + chunk(b"IEND", b""), scan


def synthia_tree(root, n=3, val_n=1, hw=(23, 37), seed=5, bad_size_item=None):
    """<root>/RGB, <root>/GT/LABELS (16-bit RGB: R = class id 0..22, G = an instance id above 255, B = 0,
    random filter per row), <root>/list/{train,val}.txt.  Returns (paths, {split: [(rgb, ids)]})."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    root = str(root)
    os.makedirs(os.path.join(root, "RGB"))
    os.makedirs(os.path.join(root, "GT", "LABELS"))
    os.makedirs(os.path.join(root, "list"))
    made, num = {}, 7
    for name, count in (("train", n), ("val", val_n)):
        made[name] = []
        with open(os.path.join(root, "list", name + ".txt"), "w") as f:
            for _ in range(count):
                rgb = rng.integers(0, 256, hw + (3,), dtype=np.uint8)
                ids = rng.integers(0, 23, hw, dtype=np.uint8)
                lhw = (hw[0] + 1, hw[1]) if num == bad_size_item else hw
                lab = np.zeros(lhw + (3,), np.uint16)
                lab[:hw[0], :, 0] = ids
                lab[..., 1] = rng.integers(256, 65536, lhw)
                data, _ = png_bytes(lab, 16, 2, rng.integers(0, 5, lhw[0]), idat_chunks=2)
                Image.fromarray(rgb).save(os.path.join(root, "RGB", f"{num:07d}.png"))
                with open(os.path.join(root, "GT", "LABELS", f"{num:07d}.png"), "wb") as g:
                    g.write(data)
                f.write(f"{num}\n")
                made[name].append((rgb, ids))
                num += 3
    return {"data_root_path": root, "list_path": os.path.join(root, "list"),
            "gt_path": os.path.join(root, "GT", "LABELS")}, made
