"""Times of in-loop AdaIN domain adaptation (tools/ADAIN.py), HIP events after warm-up, seeded He-initialised
style network (times do not depend on the values), random images.

(a) Each of the four kernels between the style network and the segmentation network on its own, at its shape
    in one iteration / one rectified validation image, through the C-ABI on preallocated buffers in windows
    of --calls calls; beside each the bytes it must move (from shapes), the time those bytes take at
    6.3 TB/s, and the same transform done with torch ops on the same GPU.
(b) One whole iteration box to box - two decoded uint8 items on the device in, the optimizer step done -
    eager and with --graph True; and what it is held against: the plain UDA step (solve_gta5's uda_step on
    ready fp32 tensors of seg_size, the same code before this loop existed) plus the plain style pass
    (StyleNet.stylize + the uint8 output, as scripts/time_style.py times it) at the source and the target
    base size.  The iteration does strictly less than that sum - the fused output replaces the uint8
    output and nothing is resampled by torch - so the bar is: iteration <= sum + the run-to-run spread
    (max - min over the rounds) of those measurements.

    python scripts/time_da_step.py [--base_size 1280,720] [--target_base_size 1280,640] [--seg_size 1280,640]
        [--out profiles/da_step_times.txt]
"""
import argparse
import os
import statistics
import sys
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from maxsquareloss_amd import hip, ops  # noqa: E402
from maxsquareloss_amd.tools import ADAIN, net  # noqa: E402
from maxsquareloss_amd.tools.train_source import init_args  # noqa: E402
from maxsquareloss_amd.utils.synthetic import IMG_MEAN  # noqa: E402
from time_style import he_init, window  # noqa: E402

STREAM_TBS = 6.3
MEAN = [float(m) for m in IMG_MEAN]


def write_trees(root, base, tbase):
    """The smallest GTA5 and Cityscapes trees the loaders accept (one image per list): the trainer is built on
    files, the timed loops run on device-resident items."""
    from PIL import Image
    rng = np.random.default_rng(1)
    g, c = os.path.join(root, "gta"), os.path.join(root, "city")
    for d in ("images", "labels"):
        os.makedirs(os.path.join(g, d))
    for num, name in ((1, "train"), (2, "test")):
        Image.fromarray(rng.integers(0, 256, (base[1], base[0], 3), dtype=np.uint8)).save(f"{g}/images/{num:05d}.png")
        Image.fromarray(rng.integers(0, 34, (base[1], base[0]), dtype=np.uint8)).save(f"{g}/labels/{num:05d}.png")
        open(f"{g}/{name}.txt", "w").write(f"{num}\n")
    for name in ("train", "val"):
        os.makedirs(f"{c}/leftImg8bit/{name}/a")
        os.makedirs(f"{c}/gtFine/{name}/a")
        rel = f"/{name}/a/a_000000_000019_leftImg8bit.png"
        Image.fromarray(rng.integers(0, 256, (tbase[1], tbase[0], 3), dtype=np.uint8)).save(f"{c}/leftImg8bit{rel}")
        Image.fromarray(rng.integers(0, 34, (tbase[1], tbase[0]), dtype=np.uint8)).save(
            f"{c}/gtFine{rel}".replace("leftImg8bit.png", "gtFine_labelIds.png"))
        open(f"{c}/{name}.txt", "w").write(rel + "\n")
    vgg, dec = he_init(net.make_vgg(), 21), he_init(net.make_decoder(), 22)
    torch.save(vgg.state_dict(), f"{root}/vgg.pth")
    torch.save(dec.state_dict(), f"{root}/decoder.pth")
    Image.fromarray(rng.integers(0, 256, (64, 96, 3), dtype=np.uint8)).save(f"{root}/style.png")
    return g, c


def kernel_rows(base, seg, low_shape):
    """[(label, fn, bytes, torch fn)] of the four kernels at their shapes."""
    lib, dev, s = hip.load(), "cuda", hip.stream_ptr()
    (bw, bh), (ws, hs) = base, seg
    oh, ow = net.out_hw(bh, bw)
    img = torch.randint(0, 256, (hs, ws, 3), dtype=torch.uint8, device=dev)
    w1, b1 = torch.randn(3, 3, 1, 1, device=dev), torch.randn(3, device=dev)
    grid = torch.empty((1, 3, hs + 2, ws + 2), device=dev)
    chw = img.permute(2, 0, 1)[None].float().div(255)
    rows = [(f"input_window  {ws // 2}x{hs // 2} of u8 {ws}x{hs} -> grid {ws}x{hs}",
             lambda: hip.check(lib.msl_style_input_window(img.data_ptr(), None, hs, ws, ws // 2, hs // 4, ws // 2, hs // 2,
                                                          hs, ws, w1.data_ptr(), b1.data_ptr(), grid.data_ptr(), 3, s), "a"),
             (ws // 2) * (hs // 2) * 3 + grid.numel() * 4,
             lambda: F.pad(F.conv2d(F.interpolate(chw[:, :, hs // 4:hs // 4 + hs // 2, ws // 2:], size=(hs, ws)), w1, b1),
                           (1, 1, 1, 1), mode="reflect"))]
    y = torch.rand((1, 3, oh + 2, ow + 2), device=dev)
    out = torch.empty((1, 3, hs, ws), device=dev)
    mean_rgb = torch.tensor(IMG_MEAN[::-1].copy(), device=dev).reshape(3, 1, 1)
    rows.append((f"output_resampled  grid {ow}x{oh} -> seg {ws}x{hs}",
                 lambda: ops.style_output_resampled(y, out, grid=True, mean=MEAN), 2 * out.numel() * 4,
                 lambda: (F.interpolate(y[:, :, 1:-1, 1:-1], size=(hs, ws)).mul(255).add(0.5).clamp(0, 255)[0]
                          - mean_rgb).flip(0).unsqueeze(0).contiguous()))
    lab = torch.randint(-1, 19, (bh, bw), dtype=torch.int64, device=dev)
    lout = torch.empty((hs, ws), dtype=torch.int64, device=dev)
    rows.append((f"label_resize  {bw}x{bh} -> {ws}x{hs}",
                 lambda: hip.check(lib.msl_label_resize_nearest(lab.data_ptr(), bh, bw, lout.data_ptr(), hs, ws, s), "c"),
                 2 * lout.numel() * 8, lambda: F.interpolate(lab.float()[None, None], size=(hs, ws))[0].long()))
    c, hi, wi = low_shape
    lows = [torch.randn((1, c, hi, wi), device=dev) * 3 for _ in range(3)]
    gt = torch.randint(-1, c, (hs * ws,), dtype=torch.int64, device=dev)
    cm = torch.zeros(c * c, dtype=torch.int64, device=dev)

    def torch_rectify():
        pred = F.interpolate(lows[0], size=(hs, ws), mode="bilinear", align_corners=True)[0]
        m, cls = pred.max(0)
        for k in (0, 1):
            new = F.interpolate(F.interpolate(lows[1 + k], size=(hs, ws), mode="bilinear", align_corners=True),
                                size=(hs // 2, ws // 2))[0]
            nm, ncls = new.max(0)
            reg = (slice(hs // 8, hs // 8 + hs // 2), slice(k * ws // 2, (k + 1) * ws // 2))
            cls[reg] = torch.where(nm > m[reg], ncls, cls[reg])
        keep = (gt >= 0) & (gt < c)
        return torch.bincount(c * gt[keep] + cls.reshape(-1)[keep], minlength=c * c)

    rows.append((f"predict_rectify  3 x {c}x{hi}x{wi} -> {ws}x{hs} + matrix",
                 lambda: ops.predict_rectify(lows[0], lows[1], lows[2], (hs, ws), hs // 8, gt, cm),
                 3 * c * hi * wi * 4 + hs * ws * 8, torch_rectify))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "da_step_times.txt"))
    ap.add_argument("--base_size", default="1280,720")
    ap.add_argument("--target_base_size", default="1280,640")
    ap.add_argument("--seg_size", default="1280,640")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3, help="iterations per timed window")
    ap.add_argument("--modes", default="eager,graph", help="the step modes of (b)")
    ap.add_argument("--kernels", type=int, default=1, help="0 skips (a)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_da_step.py measures on the GPU; none is visible")
    base, tbase, seg = (tuple(int(v) for v in s.split(",")) for s in (a.base_size, a.target_base_size, a.seg_size))
    tmp = tempfile.TemporaryDirectory()
    g, c = write_trees(tmp.name, base, tbase)
    argv = ["--imagenet_pretrained", "False", "--save_dir", "", "--resize", "True", "--base_size", a.base_size,
            "--target_base_size", a.target_base_size, "--seg_size", a.seg_size, "--source_data_path", g,
            "--target_data_path", c, "--vgg", f"{tmp.name}/vgg.pth", "--decoder", f"{tmp.name}/decoder.pth",
            "--style", f"{tmp.name}/style.png", "--target_mode", "maxsquare", "--lambda_target", "0.1"]
    gen = torch.Generator().manual_seed(5)
    c_s = torch.randint(0, 256, (base[1], base[0], 3), dtype=torch.uint8, generator=gen).cuda()
    c_t = torch.randint(0, 256, (tbase[1], tbase[0], 3), dtype=torch.uint8, generator=gen).cuda()
    y_s = torch.randint(-1, 19, (1, base[1], base[0]), dtype=torch.int64, generator=gen).cuda()
    lines = [f"# in-loop AdaIN domain adaptation, base {a.base_size}, target base {a.target_base_size}, seg {a.seg_size}, "
             f"{torch.cuda.get_device_name(0)}; HIP events, medians over {a.rounds} rounds after warm-up",
             f"# (a) each new kernel on its own, windows of {a.calls} calls on the same buffers; floor = bytes / "
             f"{STREAM_TBS} TB/s; torch = the same transform with torch ops on this GPU"]

    def trainer(mode):
        """A fresh trainer per mode: a captured step wants its first iteration on the capture stream."""
        args, _, _ = init_args(ADAIN.parse_args(argv + ["--graph", str(mode == "graph")]))
        tr = ADAIN.UDATrainer(args, cuda=True, train_id="time")
        tr.optimizer.zero_grad()
        tr.model.train()
        tr.iter_num = 1
        return tr

    modes = a.modes.split(",")
    if a.kernels:
        tr = trainer("eager")
        with torch.no_grad():
            x0, _ = tr.seg_input(c_t)
            tr.model.eval()
            low_shape = tuple(tr.model.predict_low(x0)[0].shape[1:])
            for label, fn, nbytes, tfn in kernel_rows(tbase, seg, low_shape)[:1] + kernel_rows(base, seg, low_shape)[1:]:
                window(fn, 3), window(tfn, 3)
                t = statistics.median(window(fn, a.calls) for _ in range(a.rounds))
                tt = statistics.median(window(tfn, a.calls) for _ in range(a.rounds))
                floor = nbytes / (STREAM_TBS * 1e12) * 1e6
                lines.append(f"{label:62s} {t:8.1f} us   {nbytes / 1e6:7.2f} MB   floor {floor:6.1f} us   torch {tt:8.1f} us")
                print(lines[-1], flush=True)
        tr.dataloader.close()
        tr.source_loader.close()
        del tr
        torch.cuda.empty_cache()

    times = {}
    for mode in modes:
        tr = trainer(mode)
        x_s, y_seg = tr.seg_input(c_s, y_s)
        x_t, _ = tr.seg_input(c_t)
        x_s, x_t = x_s.clone(), x_t.clone()

        def plain_step():
            tr.uda_step(x_s, y_seg, x_t)

        def da_step():
            static = tr._graphed.static if tr._graphed is not None and tr._graphed.static else (None,) * 3
            xs, ys = tr.seg_input(c_s, y_s, out=static[0])
            xt, _ = tr.seg_input(c_t, out=static[2])
            tr.uda_step(xs, ys, xt)

        def style_pass(content):
            return lambda: ops.style_output(tr.network.stylize(content, tr.style_stats, 1.0, tr.style_weights), grid=True)[0]

        runs = {f"plain UDA step at seg size, {mode}": plain_step,
                f"style pass, source base {a.base_size} (u8 out), beside {mode}": style_pass(c_s),
                f"style pass, target base {a.target_base_size} (u8 out), beside {mode}": style_pass(c_t),
                f"DA iteration, {mode}": da_step}
        for k, fn in runs.items():
            window(fn, 2)
            print(f"warmed up: {k}", flush=True)
        for _ in range(a.rounds):
            for k, fn in runs.items():
                times.setdefault(k, []).append(window(fn, a.iters) / 1e3)
        tr.dataloader.close()
        tr.source_loader.close()
        del tr, runs
        torch.cuda.empty_cache()
    lines.append(f"# (b) box to box, ms per iteration, windows of {a.iters}, alternating; spread = max - min over the rounds")
    med = {k: statistics.median(t) for k, t in times.items()}
    spread = {k: max(t) - min(t) for k, t in times.items()}
    for k, t in times.items():
        lines.append(f"{k:52s} median {med[k]:8.3f} ms   min {min(t):8.3f}   max {max(t):8.3f}   spread {spread[k]:6.3f}")
    for mode in modes:
        styles = [k for k in times if k.startswith("style pass") and k.endswith(mode)]
        step = f"plain UDA step at seg size, {mode}"
        total = med[step] + sum(med[k] for k in styles)
        slack = spread[step] + sum(spread[k] for k in styles)
        da = med[f"DA iteration, {mode}"]
        lines.append(f"{mode}: plain step + two style passes = {total:.3f} ms, spread {slack:.3f} ms; DA iteration {da:.3f} ms: "
                     f"{'within' if da <= total + slack else 'ABOVE'} the bar ({da - total:+.3f} ms)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    tmp.cleanup()


if __name__ == "__main__":
    main()
