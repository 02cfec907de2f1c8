"""Forward + backward time of the fused target-mode losses at 1024x512, C = 19 (low-res 65x129), HIP events
after warm-up.  The yardsticks are the MaxSquare / IW-MaxSquare / multi-level CE ops:
    entropy    <= 1.5 x maxsquare_up
    IW_entropy <= 1.5 x iw_maxsquare_up
    hard       <= multi_ce_up (the same kernel with one head fewer)

    python scripts/time_target_losses.py [--out profiles/target_modes_loss_times.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from maxsquareloss_amd import ops  # noqa: E402
from maxsquareloss_amd.utils.synthetic import counter_normal  # noqa: E402

C, HI, WI, HW = 19, 65, 129, (512, 1024)


def time_op(fn, low, warmup=20, reps=200):
    """Median and minimum microseconds of one forward + backward."""
    def once():
        lg = low.detach().requires_grad_()
        out = fn(lg)
        (out[0] if isinstance(out, tuple) else out).backward()
    for _ in range(warmup):
        once()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        once()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    times.sort()
    return times[len(times) // 2], times[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "target_modes_loss_times.txt"))
    a = ap.parse_args()
    low = torch.from_numpy(counter_normal(81, "time_low", C * HI * WI, 4.0)).view(1, C, HI, WI).cuda()
    low2 = torch.from_numpy(counter_normal(82, "time_low2", C * HI * WI, 4.0)).view(1, C, HI, WI).cuda()
    fns = {
        "maxsquare_up": lambda t: ops.maxsquare_up(t, HW),
        "iw_maxsquare_up": lambda t: ops.iw_maxsquare_up(t, HW, 0.2),
        "multi_ce_up": lambda t: ops.multi_ce_up(t, low2, HW, 0.95),
        "entropy_up": lambda t: ops.entropy_up(t, HW),
        "iw_entropy_up": lambda t: ops.iw_entropy_up(t, HW, 0.2),
        "hard_ce_up": lambda t: ops.hard_ce_up(t, HW, 0.95),
    }
    res = {k: time_op(fn, low) for k, fn in fns.items()}
    lines = [f"# fused loss forward + backward, C={C}, low {HI}x{WI} -> {HW[0]}x{HW[1]}, HIP events, "
             f"median / min of 200 after 20 warm-up, {torch.cuda.get_device_name(0)}"]
    for k, (med, mn) in res.items():
        lines.append(f"{k:18s} median {med:8.1f} us   min {mn:8.1f} us")
    for new, base, bar in (("entropy_up", "maxsquare_up", 1.5), ("iw_entropy_up", "iw_maxsquare_up", 1.5),
                           ("hard_ce_up", "multi_ce_up", 1.0)):
        ratio = res[new][0] / res[base][0]
        lines.append(f"{new} / {base} = {ratio:.3f} (bar {bar:.1f}: {'met' if ratio <= bar else 'MISSED'})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
