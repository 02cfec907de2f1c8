"""Times the device input pipeline against the reference's host pipeline, on the GPU box, and
writes profiles/input_pipeline_times.txt.

Per dataset shape (GTA5 1914x1052 -> 1280x720, Cityscapes 2048x1024 -> 1024x512), one item =
image + label:
  device path   pinned uint8 H2D + resize_image (fp32 BGR - mean out) + resize_label (int64 out);
                the kernels alone with the source resident (device events); bytes the kernels must
                move, from the shapes, over the kernel time, against the achievable HBM rate
  host path     what the reference's loader does after decoding, on this host, one thread: Pillow
                BICUBIC / NEAREST resize, numpy fp32 BGR - mean CHW, id -> trainId, fp32 / int64
                H2D.  (The id -> trainId step is timed as one table gather, which is faster than
                the reference's 35 masked assignments: the host path is given the benefit.)
  gate          device path < host path, per item (exit status 1 otherwise)
and one file-backed UDATrainer step (--data_loader_workers 8, PNGs of the two source shapes
written to a temporary tree) next to the synthetic step at the same network sizes: recorded
only, PNG decoding is the host's.

Times are host clocks around work that ends in a device synchronise, or device events; every
shape is warmed up first.  Needs a GPU (no fallback) and Pillow.
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12  # bytes/s a streaming copy reaches on an MI355X (8 TB/s peak)
SHAPES = [("GTA5", (1052, 1914), (1280, 720)), ("Cityscapes", (1024, 2048), (1024, 512))]


def sync_time(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def event_time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def kernel_bytes(h, w, ow, oh):
    """Bytes the two passes and the label gather must move (each operand once)."""
    image = h * w * 3 + 2 * h * ow * 3 + oh * ow * 12     # source, intermediate written + read, fp32 planes
    label = oh * ow * (1 + 8)                             # gathered ids, int64 trainIds
    return image + label


def items(args, iters, warm):
    import PIL
    from PIL import Image
    from maxsquareloss_amd.utils.preprocess import build_lut, resize_image, resize_label
    from maxsquareloss_amd.utils.synthetic import IMG_MEAN
    lines, ok = [], True
    rng = np.random.default_rng(0)
    lut = build_lut("cityscapes")
    dev = torch.device("cuda")
    for name, (h, w), (ow, oh) in SHAPES:
        rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ids = rng.integers(0, 35, (h, w), dtype=np.uint8)
        p_rgb, p_ids = torch.from_numpy(rgb).pin_memory(), torch.from_numpy(ids).pin_memory()
        d_rgb, d_ids = p_rgb.to(dev), p_ids.to(dev)

        def kernels():
            return resize_image(d_rgb, (ow, oh)), resize_label(d_ids, (ow, oh), lut)

        def device_item():
            x, y = p_rgb.to(dev, non_blocking=True), p_ids.to(dev, non_blocking=True)
            return resize_image(x, (ow, oh)), resize_label(y, (ow, oh), lut)

        im, lb = Image.fromarray(rgb), Image.fromarray(ids)
        parts = {}

        def host_item():
            t0 = time.perf_counter()
            r = im.resize((ow, oh), Image.BICUBIC)
            m = lb.resize((ow, oh), Image.NEAREST)
            t1 = time.perf_counter()
            x = np.asarray(r, np.float32)[:, :, ::-1] - IMG_MEAN
            x = torch.from_numpy(x.transpose(2, 0, 1).copy())
            y = torch.from_numpy(lut[np.asarray(m)].astype(np.int64))
            t2 = time.perf_counter()
            out = x.to(dev), y.to(dev)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            for k, v in (("pillow", t1 - t0), ("numpy", t2 - t1), ("h2d", t3 - t2)):
                parts[k] = parts.get(k, 0.0) + v
            return out

        # the two paths give the same tensors
        got, want = device_item(), host_item()
        assert torch.equal(got[0][0].cpu(), want[0].cpu()) and torch.equal(got[1][0].cpu(), want[1].cpu()), name
        for _ in range(warm):
            kernels(), device_item(), host_item()
        parts.clear()
        t_k = event_time(kernels, iters)
        t_d = sync_time(device_item, iters)
        t_h = sync_time(host_item, max(iters // 4, 3))
        n_h = max(iters // 4, 3)
        nbytes = kernel_bytes(h, w, ow, oh)
        rate = nbytes / t_k
        lines += [
            f"{name} {w}x{h} -> {ow}x{oh}  (one item = image + label; {iters} timed iterations, {warm} warm-up)",
            f"  device path  uint8 H2D + kernels   {t_d * 1e3:8.3f} ms",
            f"               kernels alone         {t_k * 1e3:8.3f} ms   ({nbytes / 1e6:.1f} MB moved, {rate / 1e12:.3f} TB/s = "
            f"{100 * rate / HBM_ACHIEVABLE:.1f} % of the achievable {HBM_ACHIEVABLE / 1e12:.1f} TB/s; recorded, not gated)",
            f"  host path    Pillow + numpy + H2D  {t_h * 1e3:8.3f} ms   (Pillow {parts['pillow'] / n_h * 1e3:.2f}, numpy "
            f"{parts['numpy'] / n_h * 1e3:.2f}, fp32/int64 H2D {parts['h2d'] / n_h * 1e3:.2f}; one thread, "
            f"Pillow {PIL.__version__})",
            f"  gate         device < host: {'PASS' if t_d < t_h else 'FAIL'}  ({t_h / t_d:.1f}x)", ""]
        ok = ok and t_d < t_h
    return lines, ok


def write_trees(root, n):
    from PIL import Image
    rng = np.random.default_rng(1)
    g, c = os.path.join(root, "gta"), os.path.join(root, "city")
    os.makedirs(os.path.join(g, "images")), os.makedirs(os.path.join(g, "labels"))
    for name in ("train", "test"):
        with open(os.path.join(g, name + ".txt"), "w") as f:
            for i in range(n):
                num = i + 1 + (n if name == "test" else 0)
                if name == "train":
                    Image.fromarray(rng.integers(0, 256, (1052, 1914, 3), dtype=np.uint8)).save(
                        os.path.join(g, "images", f"{num:05d}.png"), compress_level=1)
                    Image.fromarray(rng.integers(0, 35, (1052, 1914), dtype=np.uint8)).save(
                        os.path.join(g, "labels", f"{num:05d}.png"), compress_level=1)
                    f.write(f"{num}\n")
    for name in ("train", "val"):
        os.makedirs(os.path.join(c, "leftImg8bit", name, "x")), os.makedirs(os.path.join(c, "gtFine", name, "x"))
        with open(os.path.join(c, name + ".txt"), "w") as f:
            for i in range(n if name == "train" else 0):
                rel = f"/{name}/x/x_{i:06d}_leftImg8bit.png"
                Image.fromarray(rng.integers(0, 256, (1024, 2048, 3), dtype=np.uint8)).save(
                    os.path.join(c, "leftImg8bit") + rel, compress_level=1)
                Image.fromarray(rng.integers(0, 35, (1024, 2048), dtype=np.uint8)).save(
                    os.path.join(c, "gtFine") + rel.replace("leftImg8bit", "gtFine_labelIds"), compress_level=1)
                f.write("leftImg8bit" + rel + "\n")
    return g, c


def uda_steps(steps, warm, n_files=8):
    """A file-backed UDATrainer step (decode ahead with 8 threads, device transform, the captured
    step) next to the synthetic step, both at 1024x512 for both domains."""
    from maxsquareloss_amd.tools.solve_gta5 import UDATrainer, build_parser
    from maxsquareloss_amd.tools.train_source import init_args
    base = ["--crop_size", "1024,512", "--target_crop_size", "1024,512", "--base_size", "1024,512",
            "--target_base_size", "1024,512", "--imagenet_pretrained", "False", "--save_dir", "", "--multi", "False",
            "--lambda_target", "0.1", "--graph", "True", "--resize", "True", "--random_crop", "False"]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        g, c = write_trees(tmp, n_files)
        t_write = time.perf_counter() - t0
        for kind, extra in (("synthetic", ["--synthetic_images", str(n_files)]),
                            ("files", ["--source_data_path", g, "--target_data_path", c, "--data_loader_workers", "8"])):
            args, _, _ = init_args(build_parser().parse_args(base + extra))
            args.seg_size = (1024, 512)
            tr = UDATrainer(args, cuda=True)
            tr.optimizer.zero_grad()
            tr.model.train()
            if kind == "files":
                src, tgt = tr.source_dataloader.cycle(), tr.target_dataloader.cycle()
                nxt = lambda: (next(src), next(tgt))  # noqa: E731
            else:
                # resident on the device before the clock starts: the step as bench.py times it
                it = iter(range(10 ** 9))
                held = [tuple((d[i][0].to(tr.device), d[i][1].to(tr.device), 0)
                              for d in (tr.source_dataloader, tr.target_dataloader)) for i in range(n_files)]
                nxt = lambda: held[next(it) % n_files]  # noqa: E731

            def step():
                (x_s, y_s, _), (x_t, _, _) = nxt()
                tr.uda_step(x_s, y_s.to(torch.long), x_t)

            for _ in range(warm):
                step()
            out[kind] = sync_time(step, steps)
            if kind == "files":
                del src, tgt
                tr.dataloader.close(), tr.source_loader.close()
            del tr
            torch.cuda.empty_cache()
    return [f"UDATrainer step at 1024x512 / 1024x512, --graph True, {steps} timed steps after {warm} (recorded only):",
            f"  synthetic items, resident on the device (the step alone)   {out['synthetic'] * 1e3:8.2f} ms / step",
            f"  file-backed, --data_loader_workers 8, {n_files} + {n_files} noise PNGs   {out['files'] * 1e3:8.2f} ms / step"
            f"   (PNG decode is host work; writing the PNGs took {t_write:.1f} s, not timed)", ""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "input_pipeline_times.txt"))
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--no-uda", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_input_pipeline.py measures on the GPU; none is visible")
    head = [f"input pipeline, {torch.cuda.get_device_name(0)}, torch {torch.__version__}, host threads for the host path: 1", ""]
    torch.set_num_threads(1)
    lines, ok = items(a, a.iters, a.warmup)
    if not a.no_uda:
        lines += uda_steps(a.steps, a.warmup)
    text = "\n".join(head + lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
