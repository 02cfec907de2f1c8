"""Time of the fused optimizer steps on the full model's launch table (DeeplabMulti, 19 classes: every
live parameter, the duplicated group-0 entries with their multiplicities), HIP events after warm-up:
msl_sgd_step (one launch) and msl_adam_step (coefficient launch + element launch), called through
the C-ABI in windows of --calls calls so the host's per-call cost is not what is timed, the two
alternating over --rounds rounds.  Then, with --uda, one UDA step at 1024x512 (IW_maxsquare, multi,
hipGraph) with --optim SGD and --optim Adam, alternating.

Expectation checked: Adam <= 1.4 x SGD (28 B against 20 B per element) plus 25 % for the second
launch and the sqrt / divide work, i.e. <= 1.75 x the SGD time of the same run.

    python scripts/time_adam.py [--uda] [--out profiles/adam_step_times.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from maxsquareloss_amd import hip  # noqa: E402
from maxsquareloss_amd.graphs.models.deeplab_multi import DeeplabMulti  # noqa: E402
from maxsquareloss_amd.utils.optim import SGD, Adam  # noqa: E402
from maxsquareloss_amd.utils.synthetic import init_weights, synthetic_image, synthetic_labels  # noqa: E402


class _A:
    lr = 2.5e-4


def _optimizer(kind):
    """An optimizer over a model of its own with every live parameter marked as having a gradient
    (the dead ASPP branches, quirk Q1, excluded), its launch table built.  Returns (opt, elements)."""
    model = init_weights(DeeplabMulti(19, pretrained=False), 1).cuda()
    if kind == "SGD":
        opt = SGD(model.optim_parameters(_A), lr=2.5e-4, momentum=0.9, weight_decay=5e-4)
    else:
        opt = Adam(model.optim_parameters(_A), betas=(0.9, 0.99), weight_decay=5e-4)
    opt.grads.flat.normal_(generator=torch.Generator("cuda").manual_seed(3)).mul_(1e-3)
    dead = {id(p) for n, p in model.named_parameters() if "conv2d_list.2" in n or "conv2d_list.3" in n}
    elems = 0
    for i, p in enumerate(opt.grads.params):
        opt.grads.used[i] = id(p) not in dead
        elems += p.numel() if id(p) not in dead else 0
    opt.step()  # builds the table and the state (SGD: its first-step rule is behind it)
    opt.step()
    return opt, elems, model


def _call(kind, opt):
    lib = hip.load()
    _dev, p_ent, p_be, p_bo, nblocks = opt._table
    st = hip.stream_ptr()
    if kind == "SGD":
        return lambda: hip.check(lib.msl_sgd_step(p_ent, p_be, p_bo, nblocks, 2.5e-4, 2.5e-3, 0.9, 5e-4, 1.0, st),
                                 "msl_sgd_step")
    coef, n = opt._coef.data_ptr(), opt._table_rows
    return lambda: hip.check(lib.msl_adam_step(p_ent, n, p_be, p_bo, nblocks, 2.5e-4, 2.5e-3, 0.9, 0.99, 1e-8, 5e-4,
                                               1.0, coef, st), "msl_adam_step")


def _window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls  # us per call


def _uda_trainer(optim, graph):
    from maxsquareloss_amd.tools.solve_gta5 import UDATrainer, build_parser
    from maxsquareloss_amd.tools.train_source import init_args
    argv = ["--crop_size", "1024,512", "--target_crop_size", "1024,512", "--imagenet_pretrained", "False",
            "--save_dir", "", "--target_mode", "IW_maxsquare", "--multi", "True", "--graph", str(graph),
            "--optim", optim]
    args, _, _ = init_args(build_parser().parse_args(argv))
    tr = UDATrainer(args, cuda=True)
    tr.optimizer.zero_grad()
    return tr


def _uda_ms(tr, inputs, iters):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        tr.uda_step(*inputs)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_step_times.txt"))
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--uda", action="store_true", help="also time one UDA step per optimizer at 1024x512")
    ap.add_argument("--uda_iters", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_adam.py measures on the GPU; none is visible")
    kinds = ("SGD", "Adam")
    opts = {k: _optimizer(k) for k in kinds}
    calls = {k: _call(k, opts[k][0]) for k in kinds}
    for k in kinds:  # warm-up: code objects loaded, clocks up
        _window(calls[k], a.calls)
    times = {k: [] for k in kinds}
    for _ in range(a.rounds):
        for k in kinds:
            times[k].append(_window(calls[k], a.calls))
    elems = opts["SGD"][1]
    assert elems == opts["Adam"][1]
    bytes_per = {"SGD": 20, "Adam": 28}
    lines = [f"# optimizer step on the full model's launch table: {elems} live elements, "
             f"{opts['SGD'][0]._table_rows} entries, {opts['SGD'][0]._table[4]} blocks; HIP events around "
             f"{a.calls} calls, {a.rounds} alternating rounds after warm-up, {torch.cuda.get_device_name(0)}"]
    med = {}
    for k in kinds:
        t = sorted(times[k])
        med[k] = statistics.median(t)
        tbs = elems * bytes_per[k] / (med[k] * 1e-6) / 1e12
        lines.append(f"{'msl_' + k.lower() + '_step':14s} median {med[k]:7.1f} us   min {t[0]:7.1f}   max {t[-1]:7.1f}   "
                     f"{bytes_per[k]} B/element -> {tbs:.2f} TB/s at the median"
                     + ("   (coefficient launch included)" if k == "Adam" else ""))
    ratio = med["Adam"] / med["SGD"]
    lines.append(f"Adam / SGD = {ratio:.3f} (expectation <= 1.4 x 1.25 = 1.75: {'met' if ratio <= 1.75 else 'MISSED'})")
    if a.uda:
        del opts, calls
        torch.cuda.empty_cache()
        inputs = (synthetic_image(512, 1024, 0).cuda(), synthetic_labels(512, 1024, 19, 0).cuda(),
                  synthetic_image(512, 1024, 500).cuda())
        trs = {k: _uda_trainer(k, True) for k in kinds}
        for k in kinds:
            _uda_ms(trs[k], inputs, 5)  # eager first iteration, capture, first replays
        uda = {k: [] for k in kinds}
        for _ in range(3):
            for k in kinds:
                uda[k].append(_uda_ms(trs[k], inputs, a.uda_iters))
        lines.append(f"# one UDA step at 1024x512 (IW_maxsquare, multi, --graph True), ms per iteration over "
                     f"{a.uda_iters} replays, 3 alternating rounds")
        for k in kinds:
            lines.append(f"--optim {k:5s} " + "  ".join(f"{t:7.3f}" for t in uda[k]) +
                         f"   median {statistics.median(uda[k]):7.3f} ms")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
