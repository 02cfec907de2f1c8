"""Times of multi-scale test-time augmentation (--scales) at 1024x512, C = 19: HIP events after warm-up, the
variants of a comparison alternated in one process, round after round.

(a) The fusion alone (msl_predict_tta through Eval.add_batch_tta): the low-resolution outputs of scales 0.75, 1.0,
    1.25 (49x97, 65x129, 81x161), each with its mirror, to 512x1024 with the confusion matrix, against
      - the same rule composed from torch ops on the same GPU (msl_upsample_fwd, softmax, flip, add,
        msl_confusion_accumulate): bar 1.0;
      - three msl_predict_up --flip calls at those low sizes, timed as one unit: the fused launch must not exceed
        them by more than their run-to-run spread (max - min over the rounds).
    The 16-entry launch and C = 32 are recorded without a bar.  Bytes are computed from the shapes.
(b) Validator.run() per image with --scales 0.75,1.0,1.25 --flip True, eager and replayed, against the sum of
    three single-scale --flip runs at 768x384, 1024x512 and 1280x640 through the single-scale path.  Bar: that sum
    plus its spread (the new work is two three-channel resizes).

    python scripts/time_tta.py [--out profiles/tta_times.txt]
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
from maxsquareloss_amd.utils.validate import Validator, size_at  # noqa: E402

C, HW, SCALES = 19, (512, 1024), (0.75, 1.0, 1.25)
LOWS = ((49, 97), (65, 129), (81, 161))
P = HW[0] * HW[1]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def alternate(fns, warmup=20, reps=200):
    """{name: sorted microseconds}; one call of each variant per round, round after round."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            times[k].append(timed(fn))
    return {k: sorted(v) for k, v in times.items()}


def logits(c, hi, wi, tag):
    return torch.from_numpy(counter_normal(81, f"tta_{tag}_{c}", c * hi * wi, 3.0)).view(1, c, hi, wi).cuda()


def kernel_part(lines):
    ents = [(logits(C, hi, wi, f"{k}{m}"), m) for k, (hi, wi) in enumerate(LOWS) for m in (0, 1)]
    lab = synthetic_labels(HW[0], HW[1], C, 5).cuda()
    fused, comp, three = Eval(C), Eval(C), Eval(C)

    def composed():
        with torch.no_grad():
            acc = 0
            for low, m in ents:
                p = torch.softmax(ops.upsample_bilinear(low, HW), dim=1)
                acc = acc + (p.flip(-1) if m else p)
            comp.add_batch(lab, acc)

    def three_flip():
        for k in range(3):
            three.add_batch_low(lab, ents[2 * k][0], HW, ents[2 * k + 1][0])

    worst = [(ents[k % 6][0], k % 2) for k in range(16)]
    ents32 = [(logits(32, hi, wi, f"c32_{k}{m}"), m) for k, (hi, wi) in enumerate(LOWS) for m in (0, 1)]
    lab32, ev16, ev32 = synthetic_labels(HW[0], HW[1], 32, 5).cuda(), Eval(C), Eval(32)
    res = alternate({"fused": lambda: fused.add_batch_tta(lab, ents, HW), "composed": composed,
                     "three_flip": three_flip, "fused_16": lambda: ev16.add_batch_tta(lab, worst, HW),
                     "fused_c32": lambda: ev32.add_batch_tta(lab32, ents32, HW)})
    lo = [4 * C * hi * wi for hi, wi in LOWS]
    hi, lb, mat = 4 * C * P, 8 * P, 8 * C * C
    nbytes = {"fused": 2 * sum(lo) + lb + mat, "three_flip": 2 * sum(lo) + 3 * (lb + mat),
              # per entry an upsample (low -> hi), a softmax (r + w) and an add (2r + w), per mirror a flip (r + w);
              # then the confusion pass (hi + label)
              "composed": 2 * sum(lo) + 6 * (hi + 2 * hi + 3 * hi) + 3 * 2 * hi + (hi + lb),
              "fused_16": sum(4 * C * t.shape[2] * t.shape[3] for t, _ in worst) + lb + mat,
              "fused_c32": 2 * sum(4 * 32 * a * b for a, b in LOWS) + lb + 8 * 32 * 32}
    lines.append(f"# (a) class + confusion matrix of one image from {len(ents)} entries (low {', '.join('%dx%d' % s for s in LOWS)}, "
                 f"each with its mirror), C={C}, -> {HW[0]}x{HW[1]}, HIP events, 200 alternated rounds after 20 warm-up")
    for k, v in res.items():
        lines.append(f"{k:11s} median {v[len(v) // 2]:8.1f} us   min {v[0]:8.1f} us   max {v[-1]:8.1f} us   "
                     f"{nbytes[k] / 1e6:8.2f} MB moved (from shapes)")
    med = {k: v[len(v) // 2] for k, v in res.items()}
    ratio = med["fused"] / med["composed"]
    lines.append(f"fused / composed = {ratio:.3f} time, {nbytes['fused'] / nbytes['composed']:.4f} bytes "
                 f"(bar 1.0: {'met' if ratio <= 1.0 else 'MISSED'})")
    spread = res["three_flip"][-1] - res["three_flip"][0]
    ok = med["fused"] <= med["three_flip"] + spread
    lines.append(f"fused {med['fused']:.1f} us against three msl_predict_up flip calls {med['three_flip']:.1f} us + their spread "
                 f"{spread:.1f} us (max - min): {'met' if ok else 'MISSED'}; fused / three_flip = {med['fused'] / med['three_flip']:.3f}")
    lines.append(f"# fused_16 ({len(worst)} entries) and fused_c32 (C=32, {len(ents32)} entries): recorded, no bar")
    lines.append(f"# the matrices counted {int(fused.confusion_matrix.sum())} (fused), {int(comp.confusion_matrix.sum())} "
                 f"(composed) and {int(three.confusion_matrix.sum())} / 3 (three calls) pixels over the same calls")


def forward_part(lines, images, rounds):
    dev = torch.device("cuda", 0)
    model = init_weights(DeeplabMulti(num_classes=C, pretrained=False)).to(dev)

    def validator(hw, graph, scales=(1.0,)):
        v = Validator(model, C, hw, images, dev, flip=True, graph=graph, scales=scales)
        v.data = [(x.pin_memory(), y.pin_memory(), i) for x, y, i in (v.data[k] for k in range(images))]
        v.run()  # warm-up: packs, allocator, the capture
        v.run()
        return v

    lines.append(f"# (b) Validator.run() per image, --flip True (host-to-device copy of the image and label included), HIP "
                 f"events, median of {rounds} alternated rounds over {images} images")
    for graph in (False, True):
        tta = validator(HW, graph, SCALES)
        singles = [validator((size_at(HW[0], s), size_at(HW[1], s)), graph) for s in SCALES]
        torch.cuda.synchronize()
        t_tta, t_sum, t_each = [], [], [[] for _ in singles]
        for _ in range(rounds):
            t_tta.append(timed(tta.run) / 1e3 / images)
            each = [timed(v.run) / 1e3 / images for v in singles]
            for acc, t in zip(t_each, each):
                acc.append(t)
            t_sum.append(sum(each))
        mode = "replayed" if graph else "eager"
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        for s, v, t in zip(SCALES, singles, t_each):
            lines.append(f"{mode:9s} single scale {v.hw[1]}x{v.hw[0]} ({s})  {med(t):8.2f} ms / image")
        spread = max(t_sum) - min(t_sum)
        ok = med(t_tta) <= med(t_sum) + spread
        lines.append(f"{mode:9s} --scales {','.join(str(s) for s in SCALES)}  {med(t_tta):8.2f} ms / image against the sum "
                     f"{med(t_sum):.2f} ms + its spread {spread:.2f} ms: {'met' if ok else 'MISSED'} "
                     f"(ratio {med(t_tta) / med(t_sum):.3f})")
    px = [3 * size_at(HW[0], s) * size_at(HW[1], s) * 4 for s in SCALES if s != 1.0]
    lines.append(f"# new bytes per image: two input resizes read {2 * 3 * P * 4 / 1e6:.2f} MB and write {sum(px) / 1e6:.2f} MB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tta_times.txt"))
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    lines = [f"# {torch.cuda.get_device_name(0)}"]
    kernel_part(lines)
    forward_part(lines, a.images, a.rounds)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
