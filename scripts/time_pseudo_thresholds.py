"""Times the class-balanced threshold kernels on the GPU against the launch they share their per-pixel work with.

    python scripts/time_pseudo_thresholds.py [--what kernels,step,pass] [--images 500] [--out FILE]

kernels: msl_confidence_hist[_tta] (64 and 512 bins) and msl_pseudo_classwise[_tta] against
         msl_predict_images / msl_predict_tta_images writing only pseudo_out, from the same inputs, at 1024 x 512,
         C = 19, low resolution 65 x 129 (the TTA table: scales 0.75, 1.0, 1.25, each with its mirror).  Two
         inputs: std 6 counter_normal logits (the tests') and a skewed map - one class with p > 0.99 on about 80 %
         of the pixels, the case in which the lanes of a wave meet on one histogram cell.
step:    the captured `hard` UDA step with --threshold_mode class against fixed (one more launch, a 4 MB label map).
pass:    the statistics pass over --images synthetic images against as many iterations of the evaluator, both as
         captured graphs.

Device events around windows of many launches, the two sides alternated, the median of the windows reported.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from maxsquareloss_amd import ops  # noqa: E402
from maxsquareloss_amd.utils.synthetic import counter_normal  # noqa: E402

C, HO, WO = 19, 512, 1024
DEV = "cuda"


def logits(tag, hi, wi, std):
    return torch.from_numpy(counter_normal(7, f"tpt_{tag}_{hi}x{wi}", C * hi * wi, std)).view(1, C, hi, wi).clone()


def skewed(tag, hi, wi):
    """std 6 logits with the left 80 % of the map pushed to class 0 (std 1 noise under a margin of 14)."""
    t = logits(tag, hi, wi, 6.0)
    cut = int(round(0.8 * wi))
    t[:, :, :, :cut] = logits(tag + "n", hi, wi, 1.0)[:, :, :, :cut]
    t[:, 0, :, :cut] += 14.0
    return t


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps  # us per call


def compare(sides, reps=200, windows=7):
    """{name: median us} of callables timed in alternating windows after a warm-up of each."""
    for fn in sides.values():
        window(fn, 20)
    got = {k: [] for k in sides}
    for _ in range(windows):
        for k, fn in sides.items():
            got[k].append(window(fn, reps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}


def kernels(say):
    sizes = {0.75: (49, 97), 1.0: (65, 129), 1.25: (81, 161)}
    for name, make in (("std6", lambda tag, hi, wi: logits(tag, hi, wi, 6.0)), ("skewed", skewed)):
        low = make("a", 65, 129).to(DEV)
        lowf = (make("a", 65, 129).flip(-1) + logits("f", 65, 129, 1.0)).to(DEV)
        entries = []
        for s, (hi, wi) in sizes.items():
            base = make(f"s{s}", hi, wi)
            entries += [(base.to(DEV), 0), ((base.flip(-1) + logits(f"sf{s}", hi, wi, 1.0)).to(DEV), 1)]
        buf = ops.image_buffers((HO, WO), ("pseudo",), DEV)
        lab = torch.empty(HO * WO, dtype=torch.int64, device=DEV)
        thr = torch.full((C,), 0.9, device=DEV)
        hist = {b: ops.confidence_buffers(C, b, DEV)[0] for b in (64, 512)}
        share = float((ops.predict_images(low, (HO, WO), want=("pseudo",), thr=0.99)["pseudo"] == 0).float().mean())
        say(f"input {name}: class 0 with p > 0.99 on {100 * share:.1f} % of the pixels")
        for src, kw in (("no flip", dict(low=low)), ("flip", dict(low=low, low_flip=lowf)), ("tta6", dict(entries=entries))):
            if "entries" in kw:
                base = lambda: ops.predict_tta_images(entries, (HO, WO), out=buf, thr=0.9)  # noqa: E731
            else:
                base = lambda kw=kw: ops.predict_images(kw["low"], (HO, WO), kw.get("low_flip"), out=buf, thr=0.9)  # noqa: E731
            sides = {"images(pseudo)": base}
            for b in (64, 512):
                sides[f"hist{b}"] = lambda b=b, kw=kw: ops.confidence_hist(hist[b], (HO, WO), **kw)
            sides["classwise(label+pseudo)"] = lambda kw=kw: ops.pseudo_classwise(thr, (HO, WO), label=lab,
                                                                                 pseudo=buf["pseudo"], **kw)
            sides["classwise(pseudo)"] = lambda kw=kw: ops.pseudo_classwise(thr, (HO, WO), pseudo=buf["pseudo"], **kw)
            res = compare(sides)
            ref = res["images(pseudo)"][0]
            for k, (med, lo, hi) in res.items():
                say(f"  {name:7s} {src:8s} {k:24s} {med:8.1f} us  (windows {lo:.1f} .. {hi:.1f})  x{med / ref:.3f}")
    h = ops.confidence_buffers(C, 512, DEV)[0]
    res = compare({"class_thresholds(19x512)": lambda: ops.class_thresholds(h, 0.5, 0.9)})
    say(f"  msl_class_thresholds 19 x 512: {res['class_thresholds(19x512)'][0]:.1f} us (launch included)")


def step(say, steps=30):
    from maxsquareloss_amd.tools.solve_gta5 import UDATrainer, build_parser
    from maxsquareloss_amd.tools.train_source import init_args
    from maxsquareloss_amd.utils.synthetic import synthetic_image, synthetic_labels
    xs, ys, xt = synthetic_image(HO, WO, 40).cuda(), synthetic_labels(HO, WO, C, 40).cuda(), synthetic_image(HO, WO, 540).cuda()
    trainers = {}
    for mode in ("fixed", "class"):
        argv = ["--imagenet_pretrained", "False", "--save_dir", "", "--target_mode", "hard", "--threshold_mode", mode,
                "--threshold", "0.9", "--threshold_images", "2", "--synthetic_images", "2", "--graph", "True",
                "--iter_max", "100000"]
        args, _, _ = init_args(build_parser().parse_args(argv))
        tr = UDATrainer(args, cuda=True)
        tr.optimizer.zero_grad()
        tr.generate_thresholds()
        tr.model.train()
        for _ in range(3):
            tr.uda_step(xs, ys, xt)
        torch.cuda.synchronize()
        trainers[mode] = tr
    res = compare({m: (lambda tr=tr: tr.uda_step(xs, ys, xt)) for m, tr in trainers.items()}, reps=steps, windows=5)
    for m, (med, lo, hi) in res.items():
        say(f"  hard step, --threshold_mode {m:5s} (graph): {med / 1e3:8.3f} ms  (windows {lo / 1e3:.3f} .. {hi / 1e3:.3f})"
            f"  x{med / res['fixed'][0]:.4f}")


def stats_pass(say, images):
    from maxsquareloss_amd.tools import evaluate
    from maxsquareloss_amd.utils.synthetic import SyntheticDomain
    from maxsquareloss_amd.utils.thresholds import ThresholdPass
    from maxsquareloss_amd.utils.validate import Validator
    args, train_id, logger = evaluate.parse_args(["--imagenet_pretrained", "False", "--save_dir", "", "--val_images", "3"])
    m = evaluate.Evaluater(args, cuda=True, train_id=train_id, logger=logger).model
    # the same device-resident items for both sides: the host's synthetic generator is not what is measured
    dom = SyntheticDomain(HO, WO, C, 8, offset=900)
    items = [tuple(t.to(DEV) if torch.is_tensor(t) else t for t in dom[i]) for i in range(8)]
    data = [items[i % 8] for i in range(images)]
    val = Validator(m, C, (HO, WO), images, torch.device(DEV), graph=True, data=data)
    tp = ThresholdPass(m, C, 512, torch.device(DEV), portion=0.5, thr_max=0.9, graph=True)
    val.run(), tp.run(data[:4])
    times = {"evaluator": [], "statistics pass": []}
    for _ in range(3):
        for name, fn in (("evaluator", val.run), ("statistics pass", lambda: tp.run(data))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    base = statistics.median(times["evaluator"])
    for name, v in times.items():
        med = statistics.median(v)
        say(f"  {name:16s} {images} images (graph): {med:7.3f} s  ({1e3 * med / images:.3f} ms per image; runs "
            f"{min(v):.3f} .. {max(v):.3f})  x{med / base:.4f}")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--what", default="kernels,step,pass")
    p.add_argument("--images", type=int, default=500)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_pseudo_thresholds.py measures on the GPU; none is visible")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say(f"{torch.cuda.get_device_name(0)}; 1024 x 512, C = 19, low resolution 65 x 129; us per call, median of "
        "alternating windows")
    if "kernels" in a.what:
        kernels(say)
    if "step" in a.what:
        step(say)
    if "pass" in a.what:
        stats_pass(say, a.images)


if __name__ == "__main__":
    main()
