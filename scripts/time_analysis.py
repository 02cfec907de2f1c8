"""Times of the per-image analysis (utils/analysis.py) at 1024x512, C = 19, on synthetic items: wall clock per
image to the last file on disk, the variants of the comparison run one after the other in one process on the
same box, median of --runs runs after two warm-up runs (packs, allocator, the capture).

  validator   Validator.run(): the evaluator without any per-image score (the floor), eager and replayed;
  analyzer    Analyzer.run(), eager and replayed, the three default pictures, with --miou_threshold at -1 (no
              image saved), at the median of the per-image MIoUs (half of them) and at 2 (all of them);
  naive       the same result without the two new kernels: per image msl_predict_images (colour for every image,
              the decision is not known before the launch) into a fresh matrix, a .cpu() of the matrix, the host
              Eval's scores, and for an image below the threshold msl_colorize of the label and recover_input.

No bar is set: the numbers are recorded, each with its ratio to the Validator of the same run.

    python scripts/time_analysis.py [--out profiles/analysis_times.txt] [--images 16] [--ring 8] [--workers 8]
"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from maxsquareloss_amd import ops  # noqa: E402
from maxsquareloss_amd.graphs.models.deeplab_multi import DeeplabMulti  # noqa: E402
from maxsquareloss_amd.utils import analysis as an  # noqa: E402
from maxsquareloss_amd.utils.eval import Eval  # noqa: E402
from maxsquareloss_amd.utils.images import ImageWriter, recover_input  # noqa: E402
from maxsquareloss_amd.utils.synthetic import init_weights  # noqa: E402
from maxsquareloss_amd.utils.validate import Validator  # noqa: E402

C, HW = 19, (512, 1024)


def timed(run, images, runs):
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    per = []
    for _ in range(runs):
        t0 = time.perf_counter()
        run()  # returns after the last file is written
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) * 1e3 / images)
    return sorted(per)[len(per) // 2]


def naive(model, data, thr, out_dir, workers, dev):
    pal = ops.image_tables(C, dev)[1].view(C, 3)
    total, rows = np.zeros((C, C)), []
    shutil.rmtree(out_dir, ignore_errors=True)
    os.makedirs(out_dir)
    with ImageWriter(out_dir, (), workers) as writer, torch.no_grad():
        for i, (x, y, _) in enumerate(data):
            x = x.to(dev, non_blocking=True)
            yd = y.to(dev, dtype=torch.long, non_blocking=True).reshape(-1)
            cm = torch.zeros(C * C, dtype=torch.int64, device=dev)
            maps = ops.predict_images(model.predict_low(x)[0], HW, None, yd, cm, want=("color",))
            ev = Eval(C)
            ev.confusion_matrix = cm.view(C, C).cpu().numpy()  # the per-image sync
            scores = (ev.Pixel_Accuracy(), ev.Mean_Pixel_Accuracy(), ev.Mean_Intersection_over_Union(),
                      ev.Frequency_Weighted_Intersection_over_Union())
            total += ev.confusion_matrix
            rows.append((f"{i:06d}",) + scores)
            if scores[2] < thr:
                writer.save_as(an.file_name(rows[-1][0], scores, "label"), ops.colorize(yd.view(*HW), pal))
                writer.save_as(an.file_name(rows[-1][0], scores, "pred"), maps["color"])
                writer.save_as(an.file_name(rows[-1][0], scores, "style"), recover_input(x))
    return rows, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "analysis_times.txt"))
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--ring", type=int, default=8)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    model = init_weights(DeeplabMulti(num_classes=C, pretrained=False)).to(dev).eval()
    tmp = tempfile.mkdtemp(prefix="msl_analysis_")
    lines = [f"# {torch.cuda.get_device_name(0)}",
             f"# {a.images} synthetic items at {HW[1]}x{HW[0]}, C={C}, ring {a.ring}, {a.workers} PNG threads, kinds "
             f"{','.join(an.DEFAULT_KINDS)}; wall clock per image to the last file on disk, median of {a.runs} runs "
             f"after 2 warm-up runs; ratio = against the Validator of the same mode in this run"]
    res, order = {}, []
    sink = open(os.devnull, "w")
    try:
        base = Validator(model, C, HW, a.images, dev)
        data = [(x.pin_memory(), y.pin_memory(), i) for x, y, i in (base.data[k] for k in range(a.images))]
        rows, total = naive(model, data, -1.0, os.path.join(tmp, "probe"), 0, dev)
        mious = sorted(r[3] for r in rows)
        mid = 0.5 * (mious[len(mious) // 2 - 1] + mious[len(mious) // 2]) if len(mious) > 1 else mious[0] + 1.0
        thresholds = (("none saved (-1)", -1.0), (f"half saved ({mid:.4f})", mid), ("all saved (2)", 2.0))
        lines.append(f"# per-image MIoU {mious[0]:.4f} .. {mious[-1]:.4f}; the median threshold saves "
                     f"{sum(1 for v in mious if v < mid)} of {len(mious)}")
        for graph in (False, True):
            mode = "replayed" if graph else "eager"
            v = Validator(model, C, HW, a.images, dev, graph=graph)
            v.data = data
            res[("validator", mode, "")] = timed(v.run, a.images, a.runs)
            order.append(("validator", mode, ""))
            assert np.array_equal(v.Eval.confusion_matrix, total)
            for what, thr in thresholds:
                z = an.Analyzer(model, C, HW, a.images, dev, os.path.join(tmp, f"{mode}_{thr}"), graph=graph,
                                threshold=thr, ring=a.ring, workers=a.workers)
                z.data = data

                def run(z=z):
                    shutil.rmtree(z.out_dir, ignore_errors=True)
                    stdout, sys.stdout = sys.stdout, sink  # the per-class table of every run
                    try:
                        z.run()
                    finally:
                        sys.stdout = stdout

                res[("analyzer", mode, what)] = timed(run, a.images, a.runs)
                order.append(("analyzer", mode, what))
                assert np.array_equal(z.totalEval.confusion_matrix, total)
                assert sum(t[6] for t in z.table) == sum(1 for m in mious if m < thr)
                assert len(os.listdir(z.out_dir)) == 3 * sum(t[6] for t in z.table)
        for what, thr in thresholds:
            res[("naive", "eager", what)] = timed(
                lambda thr=thr: naive(model, data, thr, os.path.join(tmp, "naive"), a.workers, dev), a.images, a.runs)
            order.append(("naive", "eager", what))
    finally:
        sink.close()
        shutil.rmtree(tmp, ignore_errors=True)
    for key in order:
        kind, mode, what = key
        ratio = res[key] / res[("validator", mode, "")]
        lines.append(f"{kind:9s} {mode:9s} {what:24s} {res[key]:8.2f} ms / image   x{ratio:.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
