"""Times file-backed SYNTHIA on the GPU box and writes profiles/synthia_pipeline_times.txt (recorded, not
gated; DESIGN 3.11 reads the numbers).

  kernel   msl_png_unfilter_lane at 1280x760 on the compacted plane, per filter: all rows None / Sub / Up /
           Average / Paeth and the mix Pillow's adaptive encoder chose for the same label map (a 16-bit
           greyscale file Pillow wrote; its low-byte lane).  Device events around single calls, the median
           of --iters of them after warm-up, min and max beside it.
  host     read_scanlines (CRC, inflate) + lane_plane of a 16-bit RGB label file of that map, one thread.
  item     one SYNTHIA item (pinned uint8 H2D of image + plane, unfilter, image / label transform) beside
           one GTA5 item (H2D, BICUBIC / NEAREST resize 1914x1052 -> 1280x720), host clock around work that
           ends in a synchronise.
  step     a config-5-shaped UDATrainer step (1280x760, IW_maxsquare + multi, fp16 convs, --graph True)
           from temporary PNG trees against the same step on resident synthetic items, for SYNTHIA (16
           classes) and for GTA5 (19 classes) as the source; each timed --repeats times, the spread of the
           repeats beside the medians.

Needs a GPU (no fallback) and Pillow.
"""
import argparse
import io
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import png_ref  # noqa: E402  (tests/png_ref.py: the PNG writer with a chosen filter per row)

H, W = 760, 1280


def label_map(rng, h=H, w=W):
    """A compressible label map: class ids 0..22 in blocks, as a rendered scene has them."""
    coarse = rng.integers(0, 23, (h // 40 + 1, w // 64 + 1), dtype=np.uint8)
    return np.ascontiguousarray(np.kron(coarse, np.ones((40, 64), np.uint8))[:h, :w])


def label_file(rng, ids, filters):
    lab = np.zeros(ids.shape + (3,), np.uint16)
    lab[..., 0] = ids
    lab[..., 1] = np.kron(rng.integers(256, 65536, (ids.shape[0] // 40 + 1, ids.shape[1] // 64 + 1)),
                          np.ones((40, 64), np.int64))[:ids.shape[0], :ids.shape[1]]
    return png_ref.png_bytes(lab, 16, 2, filters, idat_chunks=8)[0]


def event_times(fn, iters, warm):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def sync_time(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def kernel_lines(rng, ids, iters, warm):
    from PIL import Image
    from maxsquareloss_amd import hip
    from maxsquareloss_amd.utils import png, preprocess
    planes = {name: png_ref.filter_rows(ids, 1, [k] * H) for k, name in enumerate(("None", "Sub", "Up", "Average", "Paeth"))}
    buf = io.BytesIO()
    Image.fromarray(ids.astype(np.uint16)).save(buf, format="PNG")
    info, scan = png.read_scanlines(buf.getvalue())
    mix = png.lane_plane(scan, info.bpp, png.label_lane(info))
    counts = np.bincount(mix[:, 0], minlength=5)
    planes["Pillow-adaptive"] = mix
    band = hip.load().msl_png_unfilter_band_rows()
    lines = [f"msl_png_unfilter_lane, {W}x{H} compacted plane (bpp 1), one workgroup of {band} threads; device events "
             f"around single calls, {iters} timed after {warm} warm-up:"]
    for name, plane in planes.items():
        d = torch.from_numpy(np.ascontiguousarray(plane)).cuda()
        assert np.array_equal(preprocess.png_unfilter(d).cpu().numpy(), ids), name
        t = event_times(lambda: preprocess.png_unfilter(d), iters, warm)
        extra = f"   (rows per filter 0..4: {counts.tolist()})" if name == "Pillow-adaptive" else ""
        lines.append(f"  {name:<16} median {statistics.median(t):7.3f} ms   min {min(t):7.3f}   max {max(t):7.3f}{extra}")
    return lines + [""]


def host_lines(data, iters):
    from maxsquareloss_amd.utils import png
    t_read, t_lane = [], []
    for _ in range(iters):
        t0 = time.perf_counter()
        info, scan = png.read_scanlines(data)
        t1 = time.perf_counter()
        png.lane_plane(scan, info.bpp, png.label_lane(info))
        t_lane.append(time.perf_counter() - t1)
        t_read.append(t1 - t0)
    return [f"host, one thread, 16-bit RGB label file of the same map ({len(data)} bytes, 8 IDAT chunks), median of {iters}:",
            f"  read_scanlines (CRC + inflate of {H * (1 + 6 * W)} bytes)   {statistics.median(t_read) * 1e3:7.3f} ms",
            f"  lane_plane (1 of 6 byte lanes)                     {statistics.median(t_lane) * 1e3:7.3f} ms", ""]


def item_lines(rng, ids, data, iters, warm):
    from maxsquareloss_amd.utils import png, preprocess
    dev = torch.device("cuda")
    lut16, lut19 = preprocess.build_lut("synthia", True), preprocess.build_lut("gta5")
    info, scan = png.read_scanlines(data)
    plane = png.lane_plane(scan, info.bpp, png.label_lane(info))
    p_rgb = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).pin_memory()
    p_plane = torch.from_numpy(plane).pin_memory()
    g_rgb = torch.from_numpy(rng.integers(0, 256, (1052, 1914, 3), dtype=np.uint8)).pin_memory()
    g_ids = torch.from_numpy(rng.integers(0, 35, (1052, 1914), dtype=np.uint8)).pin_memory()

    def synthia_item():
        x, y = p_rgb.to(dev, non_blocking=True), p_plane.to(dev, non_blocking=True)
        return preprocess.resize_image(x, (W, H)), preprocess.resize_label(preprocess.png_unfilter(y), (W, H), lut16)

    def synthia_without():
        x, y = p_rgb.to(dev, non_blocking=True), p_plane.to(dev, non_blocking=True)
        return preprocess.resize_image(x, (W, H)), preprocess.resize_label(y[:, 1:], (W, H), lut16)

    def gta5_item():
        x, y = g_rgb.to(dev, non_blocking=True), g_ids.to(dev, non_blocking=True)
        return preprocess.resize_image(x, (1280, 720)), preprocess.resize_label(y, (1280, 720), lut19)

    assert np.array_equal(synthia_item()[1][0].cpu().numpy(), lut16[ids].astype(np.int64))
    out = {}
    for name, fn in (("synthia", synthia_item), ("without", synthia_without), ("gta5", gta5_item)):
        for _ in range(warm):
            fn()
        out[name] = [sync_time(fn, iters) * 1e3 for _ in range(3)]
    fmt = lambda v: f"{statistics.median(v):7.3f} ms   (three runs of {iters}: " + ", ".join(f"{t:.3f}" for t in v) + ")"  # noqa: E731
    return ["one item = image + label, pinned uint8 H2D + device work, host clock, synchronised:",
            f"  SYNTHIA {W}x{H} (H2D, unfilter, image / label transform)    {fmt(out['synthia'])}",
            f"  the same item, a strided copy in place of the unfilter     {fmt(out['without'])}",
            f"  GTA5 1914x1052 -> 1280x720 (H2D, BICUBIC / NEAREST resize)   {fmt(out['gta5'])}", ""]


def write_trees(root, rng, n):
    from PIL import Image
    s, g, c = (os.path.join(root, k) for k in ("synthia", "gta", "city"))
    for d in ("RGB", "GT/LABELS", "list"):
        os.makedirs(os.path.join(s, d))
    os.makedirs(os.path.join(g, "images")), os.makedirs(os.path.join(g, "labels"))
    noise = lambda h, w: Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))  # noqa: E731
    for name in ("train", "val"):
        with open(os.path.join(s, "list", name + ".txt"), "w") as f:
            for i in range(n if name == "train" else 0):
                noise(H, W).save(os.path.join(s, "RGB", f"{i:07d}.png"), compress_level=1)
                with open(os.path.join(s, "GT", "LABELS", f"{i:07d}.png"), "wb") as out:
                    out.write(label_file(rng, label_map(rng), rng.integers(0, 5, H)))
                f.write(f"{i}\n")
    for name in ("train", "test"):
        with open(os.path.join(g, name + ".txt"), "w") as f:
            for i in range(n if name == "train" else 0):
                noise(1052, 1914).save(os.path.join(g, "images", f"{i + 1:05d}.png"), compress_level=1)
                Image.fromarray(label_map(rng, 1052, 1914)).save(os.path.join(g, "labels", f"{i + 1:05d}.png"))
                f.write(f"{i + 1}\n")
    for name in ("train", "val"):
        os.makedirs(os.path.join(c, "leftImg8bit", name, "x")), os.makedirs(os.path.join(c, "gtFine", name, "x"))
        with open(os.path.join(c, name + ".txt"), "w") as f:
            for i in range(n if name == "train" else 0):
                rel = f"/{name}/x/x_{i:06d}_leftImg8bit.png"
                noise(1024, 2048).save(os.path.join(c, "leftImg8bit") + rel, compress_level=1)
                Image.fromarray(label_map(rng, 1024, 2048)).save(
                    os.path.join(c, "gtFine") + rel.replace("leftImg8bit", "gtFine_labelIds"))
                f.write("leftImg8bit" + rel + "\n")
    return s, g, c


def step_lines(rng, steps, warm, repeats, n_files=8):
    from maxsquareloss_amd.tools.solve_gta5 import UDATrainer, build_parser
    from maxsquareloss_amd.tools.train_source import init_args
    size = f"{W},{H}"
    base = ["--crop_size", size, "--target_crop_size", size, "--base_size", size, "--target_base_size", size,
            "--imagenet_pretrained", "False", "--save_dir", "", "--multi", "True", "--target_mode", "IW_maxsquare",
            "--lambda_target", "0.1", "--conv_math", "fp16", "--graph", "True", "--resize", "True",
            "--random_crop", "False"]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        s, g, c = write_trees(tmp, rng, n_files)
        t_write = time.perf_counter() - t0
        runs = []
        for source, root, classes in (("synthia", s, "16"), ("gta5", g, "19")):
            common = base + ["--source_dataset", source, "--num_classes", classes]
            lists = ["--source_list_path", os.path.join(root, "list")] if source == "synthia" else []
            runs += [((source, "resident"), common + ["--synthetic_images", str(n_files)]),
                     ((source, "files"), common + lists + ["--source_data_path", root, "--target_data_path", c,
                                                           "--data_loader_workers", "8"])]
        for key, argv in runs:
            args, _, _ = init_args(build_parser().parse_args(argv))
            args.seg_size = (W, H)
            tr = UDATrainer(args, cuda=True)
            tr.optimizer.zero_grad()
            tr.model.train()
            if key[1] == "files":
                src, tgt = tr.source_dataloader.cycle(), tr.target_dataloader.cycle()
                nxt = lambda: (next(src), next(tgt))  # noqa: E731
            else:
                it = iter(range(10 ** 9))
                held = [tuple((d[i][0].to(tr.device), d[i][1].to(tr.device), 0)
                              for d in (tr.source_dataloader, tr.target_dataloader)) for i in range(n_files)]
                nxt = lambda: held[next(it) % n_files]  # noqa: E731

            def step():
                (x_s, y_s, _), (x_t, _, _) = nxt()
                tr.uda_step(x_s, y_s.to(torch.long), x_t)

            for _ in range(warm):
                step()
            out[key] = [sync_time(step, steps) * 1e3 for _ in range(repeats)]
            if key[1] == "files":
                del src, tgt
                tr.dataloader.close(), tr.source_loader.close()
            del tr
            torch.cuda.empty_cache()
    lines = [f"UDATrainer step, config 5's shape ({W}x{H} both domains, IW_maxsquare + multi, fp16 convs, --graph True), "
             f"{repeats} runs of {steps} steps after {warm} warm-up; files = {n_files} + {n_files} temporary PNGs, "
             f"--data_loader_workers 8 (writing them took {t_write:.1f} s, not timed):"]
    for source in ("synthia", "gta5"):
        r, f = out[(source, "resident")], out[(source, "files")]
        lines += [f"  source {source:<8} resident synthetic items   median {statistics.median(r):7.2f} ms / step   "
                  f"(runs: {', '.join(f'{t:.2f}' for t in r)}; spread {max(r) - min(r):.2f})",
                  f"  source {source:<8} file-backed                median {statistics.median(f):7.2f} ms / step   "
                  f"(runs: {', '.join(f'{t:.2f}' for t in f)}; spread {max(f) - min(f):.2f})",
                  f"  source {source:<8} file-backed - resident     {statistics.median(f) - statistics.median(r):+7.2f} ms"]
    d = {k: statistics.median(out[(k, "files")]) - statistics.median(out[(k, "resident")]) for k in ("synthia", "gta5")}
    lines += [f"  SYNTHIA's difference - GTA5's difference      {d['synthia'] - d['gta5']:+7.2f} ms   (held against the "
              "unfilter's kernel time above, within the spreads)", ""]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "synthia_pipeline_times.txt"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-uda", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_synthia_pipeline.py measures on the GPU; none is visible")
    torch.set_num_threads(1)
    rng = np.random.default_rng(0)
    ids = label_map(rng)
    data = label_file(rng, ids, rng.integers(0, 5, H))
    lines = [f"SYNTHIA input pipeline, {torch.cuda.get_device_name(0)}, torch {torch.__version__}", ""]
    lines += kernel_lines(rng, ids, a.iters, a.warmup)
    lines += host_lines(data, max(a.iters // 3, 5))
    lines += item_lines(rng, ids, data, a.iters, a.warmup)
    if not a.no_uda:
        lines += step_lines(rng, a.steps, a.warmup, a.repeats)
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
