"""Times of the prediction images at 1024x512, C = 19 (low-res 65x129): HIP events after warm-up, medians, the
variants of a comparison alternated in one process.

(a) msl_predict_images with all five maps against
      predict_up   msl_predict_up alone (class map only) - with --parent_lib from a libmsl_hip.so built from the
                   parent commit, loaded beside this build's (whose own is then timed as predict_up_new), else
                   this build's;
      composed     the same maps without the new kernel: msl_predict_up's class map, torch indexing of the id
                   table and the palette, msl_upsample_fwd + torch softmax (x2, flip and average with flip) for
                   the winning probability, torch comparisons for the shade and the pseudo-label, uint8 casts.
    Bytes are computed from the shapes.  No bar is set: the numbers are recorded.
(b) one whole saved image - Validator.run() with an output request for the color and labelids kinds: forward,
    kernel, device-to-host copy, PNG encode - per image, eager and replayed, with 0 and 8 writer threads, against the
    same run without the request.

    python scripts/time_predict_images.py [--out profiles/predict_images_times.txt] [--parent_lib PATH]
"""
import argparse
import ctypes
import os
import shutil
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from maxsquareloss_amd import hip, ops  # noqa: E402
from maxsquareloss_amd.graphs.models.deeplab_multi import DeeplabMulti  # noqa: E402
from maxsquareloss_amd.utils.images import OutputRequest  # noqa: E402
from maxsquareloss_amd.utils.palette import SPLITS  # noqa: E402
from maxsquareloss_amd.utils.synthetic import counter_normal, init_weights  # noqa: E402
from maxsquareloss_amd.utils.validate import Validator  # noqa: E402

C, HI, WI, HW = 19, 65, 129, (512, 1024)
P = HW[0] * HW[1]
MAPS = tuple(ops.IMAGE_MAPS)


def alternate(fns, warmup=20, reps=200):
    """{name: (median, min) microseconds}; one call of each variant per round, round after round.  A round starts
    one variant later than the one before, so that every variant follows every other equally often (what ran
    before decides whether the low-res logits are still in L2)."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    order = list(fns.items())
    for r in range(reps):
        for k, fn in order[r % len(order):] + order[:r % len(order)]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    return {k: (sorted(v)[len(v) // 2], min(v)) for k, v in times.items()}


def kernel_part(lines, parent_lib):
    low = torch.from_numpy(counter_normal(81, "time_low", C * HI * WI, 6.0)).view(1, C, HI, WI).cuda()
    lowf = (low.flip(-1) + torch.from_numpy(counter_normal(82, "time_lowf", C * HI * WI, 1.0)).view(1, C, HI, WI).cuda())
    lowf = lowf.contiguous()
    idl, pal, shade = ops.image_tables(C, low.device)
    pal, shade = pal.view(C, 3), shade.view(4, C, 3)
    bufs = ops.image_buffers(HW, MAPS, low.device)
    arg = torch.empty(P, dtype=torch.int32, device=low.device)
    up = hip.load().msl_predict_up
    if parent_lib:
        up = ctypes.CDLL(parent_lib).msl_predict_up
        up.restype, up.argtypes = hip.SIGNATURES["msl_predict_up"]

    def predict_up(flip, up=up):
        hip.check(up(low.data_ptr(), lowf.data_ptr() if flip else None, C, HI, WI, HW[0], HW[1], None, None,
                     arg.data_ptr(), hip.stream_ptr()), "msl_predict_up")

    def composed(flip):
        with torch.no_grad():
            cls = ops.predict_up(low, HW, lowf if flip else None, want_argmax=True).long()
            out = {"class": cls.to(torch.uint8), "ids": idl[cls], "color": pal[cls]}
            p = torch.softmax(ops.upsample_bilinear(low, HW), dim=1)
            if flip:
                p = (p + torch.softmax(ops.upsample_bilinear(lowf, HW), dim=1).flip(-1)) / 2
            top = p[0].max(dim=0).values.reshape(-1)
            bucket = (top <= SPLITS[0]).long() + (top <= SPLITS[1]) + (top <= SPLITS[2]) + (top <= SPLITS[3])
            conf = torch.cat([shade, shade.new_zeros(1, C, 3)])[bucket, cls]
            out["confidence"] = conf
            out["pseudo"] = torch.where(top > 0.95, cls, cls.new_full((), 255)).to(torch.uint8)
            return out

    fns = {}
    for flip in (False, True):
        tag = "_flip" if flip else ""
        fns["predict_up" + tag] = lambda f=flip: predict_up(f)
        if parent_lib:  # the refactored kernel of this build next to the parent's
            fns["predict_up_new" + tag] = lambda f=flip: predict_up(f, hip.load().msl_predict_up)
        fns["images" + tag] = lambda f=flip: ops.predict_images(low, HW, lowf if f else None, out=bufs)
        fns["composed" + tag] = lambda f=flip: composed(f)
    # the composed path computes what the kernel computes (off the rounding edges of the probability)
    for flip in (False, True):
        want = composed(flip)
        ops.predict_images(low, HW, lowf if flip else None, out=bufs)
        diff = {k: int((bufs[k].reshape(-1) != want[k].reshape(-1)).sum()) for k in MAPS}
        lines.append(f"# flip {'on ' if flip else 'off'}: bytes that differ between the kernel and the composed path "
                     f"(probability rounding at a cut): {diff}")
    res = alternate(fns)
    lo, hi = 4 * C * HI * WI, 4 * C * P
    nbytes = {"predict_up": lo + 4 * P, "predict_up_flip": 2 * lo + 4 * P, "predict_up_new": lo + 4 * P,
              "predict_up_new_flip": 2 * lo + 4 * P, "images": lo + 9 * P,
              "images_flip": 2 * lo + 9 * P,
              # predict_up (low -> int32), casts and gathers (r int64 + w), upsample (low -> hi), softmax (r + w),
              # max (r hi + w), four compares and sums, gather, where
              "composed": (lo + 4 * P) + (4 + 8) * P + 3 * (8 + 1) * P + (lo + hi) + 2 * hi + hi + 4 * P,
              "composed_flip": (2 * lo + 4 * P) + (4 + 8) * P + 3 * (8 + 1) * P + 2 * (lo + hi) + 4 * hi + 7 * hi
              + hi + 4 * P}
    lines.append(f"# (a) all five maps of one image, C={C}, low {HI}x{WI} -> {HW[0]}x{HW[1]}, HIP events, median / min "
                 f"of 200 alternated rounds after 20 warm-up; predict_up from "
                 f"{'the parent commit (--parent_lib)' if parent_lib else 'this build'}")
    for k, (med, mn) in res.items():
        lines.append(f"{k:16s} median {med:8.1f} us   min {mn:8.1f} us   {nbytes[k] / 1e6:8.2f} MB moved at least "
                     f"(from shapes)")
    for tag in ("", "_flip"):
        lines.append(f"images{tag} / predict_up{tag} = {res['images' + tag][0] / res['predict_up' + tag][0]:.3f} time; "
                     f"images{tag} / composed{tag} = {res['images' + tag][0] / res['composed' + tag][0]:.3f} time")


def saved_part(lines, images):
    dev = torch.device("cuda", 0)
    model = init_weights(DeeplabMulti(num_classes=C, pretrained=False)).to(dev)
    tmp = tempfile.mkdtemp(prefix="msl_predict_images_")
    res = {}
    try:
        for graph in (False, True):
            for workers in (None, 0, 8):
                req = None if workers is None else OutputRequest(tmp, ("color", "labelids"), workers=workers)
                v = Validator(model, C, HW, images, dev, graph=graph, outputs=req)
                v.data = [(x.pin_memory(), y.pin_memory(), i) for x, y, i in (v.data[k] for k in range(images))]
                v.run()  # warm-up: packs, allocator, the capture
                v.run()
                torch.cuda.synchronize()
                per = []
                for _ in range(5):
                    t0 = time.perf_counter()
                    v.run()  # returns after the last file is written
                    torch.cuda.synchronize()
                    per.append((time.perf_counter() - t0) * 1e3 / images)
                res[(graph, workers)] = sorted(per)[len(per) // 2]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    lines.append(f"# (b) Validator.run() per image at {HW[1]}x{HW[0]}, wall clock to the last file on disk, median of 5 "
                 f"runs over {images} images; saved = color + labelids PNGs (forward, msl_predict_images, D2H, encode)")
    for (graph, workers), ms in res.items():
        what = "no images saved " if workers is None else f"saved, {workers} threads"
        lines.append(f"{'replayed' if graph else 'eager':9s} {what:18s} {ms:8.2f} ms / image")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_images_times.txt"))
    ap.add_argument("--images", type=int, default=8, help="images per run of part (b); 0 skips it")
    ap.add_argument("--parent_lib", default=None, help="a libmsl_hip.so built from the parent commit")
    a = ap.parse_args()
    lines = [f"# {torch.cuda.get_device_name(0)}"]
    kernel_part(lines, a.parent_lib)
    if a.images > 0:
        saved_part(lines, a.images)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
