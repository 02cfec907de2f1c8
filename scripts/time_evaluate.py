"""Times of the evaluator at 1024x512, C = 19 (low-res 65x129): HIP events after warm-up, medians, the
variants of a comparison alternated in one process.

(a) msl_predict_up (ops.predict_up: upsampling, class and confusion matrix in one kernel) against the same
    result composed from the older entry points: msl_upsample_fwd (x2 with --flip), torch softmax / flip / add,
    msl_confusion_accumulate.  The fused kernel must not be slower.  Bytes are computed from the shapes.
(b) Validator.run() per image (utils/validate.py: eval-mode forward + msl_predict_up), eager and as a captured
    graph, flip off and on, on images already on the host.  The flip pair must cost no more than two single
    forwards.  --step_ms records the same box's `python bench.py` step time next to it.

    python scripts/time_evaluate.py [--out profiles/evaluate_times.txt] [--step_ms MS]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from maxsquareloss_amd import ops  # noqa: E402
from maxsquareloss_amd.graphs.models.deeplab_multi import DeeplabMulti  # noqa: E402
from maxsquareloss_amd.utils.eval import Eval  # noqa: E402
from maxsquareloss_amd.utils.synthetic import counter_normal, init_weights, synthetic_labels  # noqa: E402
from maxsquareloss_amd.utils.validate import Validator  # noqa: E402

C, HI, WI, HW = 19, 65, 129, (512, 1024)
P = HW[0] * HW[1]


def alternate(fns, warmup=20, reps=200):
    """{name: (median, min) microseconds}; one call of each variant per round, round after round."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    return {k: (sorted(v)[len(v) // 2], min(v)) for k, v in times.items()}


def kernel_part(lines):
    low = torch.from_numpy(counter_normal(81, "time_low", C * HI * WI, 3.0)).view(1, C, HI, WI).cuda()
    lowf = torch.from_numpy(counter_normal(82, "time_lowf", C * HI * WI, 3.0)).view(1, C, HI, WI).cuda()
    lab = synthetic_labels(HW[0], HW[1], C, 5).cuda()
    fused, comp = Eval(C), Eval(C)

    def composed(flip):
        with torch.no_grad():
            pred = ops.upsample_bilinear(low, HW)
            if flip:
                pf = torch.softmax(ops.upsample_bilinear(lowf, HW), dim=1).flip(-1)
                pred = (torch.softmax(pred, dim=1) + pf) / 2
            comp.add_batch(lab, pred)

    fns = {"fused": lambda: fused.add_batch_low(lab, low, HW), "composed": lambda: composed(False),
           "fused_flip": lambda: fused.add_batch_low(lab, low, HW, lowf), "composed_flip": lambda: composed(True)}
    res = alternate(fns)
    counted = (int(fused.confusion_matrix.sum()), int(comp.confusion_matrix.sum()))
    lo, hi, lb = 4 * C * HI * WI, 4 * C * P, 8 * P
    nbytes = {"fused": lo + lb + 8 * C * C, "fused_flip": 2 * lo + lb + 8 * C * C,
              # upsample: low -> hi; confusion: hi + label
              "composed": (lo + hi) + (hi + lb),
              # 2 upsamples, 2 softmaxes (r + w), flip (r + w), add (2r + w), halve (r + w), confusion
              "composed_flip": 2 * (lo + hi) + 2 * 2 * hi + 2 * hi + 3 * hi + 2 * hi + (hi + lb)}
    lines.append(f"# (a) class + confusion matrix of one image, C={C}, low {HI}x{WI} -> {HW[0]}x{HW[1]}, HIP events, "
                 f"median / min of 200 alternated rounds after 20 warm-up")
    for k, (med, mn) in res.items():
        lines.append(f"{k:14s} median {med:8.1f} us   min {mn:8.1f} us   {nbytes[k] / 1e6:8.2f} MB moved (from shapes)")
    for new, base in (("fused", "composed"), ("fused_flip", "composed_flip")):
        ratio = res[new][0] / res[base][0]
        lines.append(f"{new} / {base} = {ratio:.3f} time, {nbytes[new] / nbytes[base]:.4f} bytes "
                     f"(bar 1.0: {'met' if ratio <= 1.0 else 'MISSED'})")
    lines.append(f"# the two matrices counted {counted[0]} and {counted[1]} pixels over the same calls")


def forward_part(lines, images, step_ms):
    dev = torch.device("cuda", 0)
    model = init_weights(DeeplabMulti(num_classes=C, pretrained=False)).to(dev)
    res = {}
    for graph in (False, True):
        for flip in (False, True):
            v = Validator(model, C, HW, images, dev, flip=flip, graph=graph)
            v.data = [(x.pin_memory(), y.pin_memory(), i) for x, y, i in (v.data[k] for k in range(images))]
            v.run()  # warm-up: packs, allocator, the capture
            v.run()
            torch.cuda.synchronize()
            per = []
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                v.run()
                e1.record()
                e1.synchronize()
                per.append(e0.elapsed_time(e1) / images)
            res[(graph, flip)] = sorted(per)[len(per) // 2]
    lines.append(f"# (b) Validator.run() per image at {HW[1]}x{HW[0]} (eval-mode forward + msl_predict_up; host-to-device "
                 f"copy of the image and label included), HIP events, median of 5 runs over {images} images")
    for (graph, flip), ms in res.items():
        lines.append(f"{'replayed' if graph else 'eager':9s} flip {'on ' if flip else 'off'}  {ms:8.2f} ms / image")
    for graph in (False, True):
        ratio = res[(graph, True)] / res[(graph, False)]
        lines.append(f"{'replayed' if graph else 'eager'}: flip on / flip off = {ratio:.3f} "
                     f"(bar 2.0, two single forwards: {'met' if ratio <= 2.0 else 'MISSED'})")
    if step_ms is not None:
        lines.append(f"# the same box's `python bench.py` training step: {step_ms:.2f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evaluate_times.txt"))
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--step_ms", type=float, default=None)
    a = ap.parse_args()
    lines = [f"# {torch.cuda.get_device_name(0)}"]
    kernel_part(lines)
    forward_part(lines, a.images, a.step_ms)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
