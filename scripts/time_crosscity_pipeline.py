"""Times the cross-city JPEG path on the GPU box and writes profiles/crosscity_pipeline_times.txt (recorded,
not gated; DESIGN 3.13 reads the numbers and the default of --jpeg_decode follows from them).

One 2048x1024 4:2:0 quality-92 file, made by Pillow's encoder from a synthetic photo-like image:
  pillow   Pillow's whole decode, `np.asarray(Image.open(f).convert("RGB"))`, one thread, per image.
  host     the host half alone: msl_jpeg_entropy_decode into a buffer that exists, and utils/jpeg.py
           decode_file into a buffer the caller hands it (as the loader's staging slot does), one thread, per image.
  device   msl_jpeg_reconstruct: device events around single calls (both launches), and each kernel's own time
           from `rocprofv3 --kernel-trace --stats` over a child process of this script that only runs the call
           (--kernels-only); bytes moved, computed from the shapes, over that time against the achievable HBM
           rate (6.3 TB/s).
  loader   CrossCity_DataLoader items per second over a temporary tree of such files with 8 decoding threads,
           --jpeg_decode device and pillow alternating in the same run, host clock around epochs that end in a
           synchronise.

Needs a GPU (no fallback) and Pillow.
"""
import argparse
import csv
import ctypes
import glob
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import jpeg_ref  # noqa: E402  (tests/jpeg_ref.py: the generated pictures and Pillow's encoder)

H, W = 1024, 2048
HBM = 6.3e12  # achievable bytes / s


def the_file(seed=1):
    return jpeg_ref.encode(jpeg_ref.photo(H, W, seed), 2, quality=92)


def host_clock(fn, iters):
    out = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def traffic(header):
    """(bytes of launch 1, bytes of launch 2), from the shapes: coefficients in and planes out; planes in (each
    sample once) and RGB out."""
    blocks = sum(c.blocks_w * c.blocks_h for c in list(header.comp)[:header.ncomp])
    planes = blocks * 64
    return blocks * 128 + planes, planes + header.width * header.height * 3


def reconstruct_call(data):
    from maxsquareloss_amd.utils import jpeg, preprocess
    payload = jpeg.decode_file(data)
    header = jpeg.header_of(payload)
    dev = torch.from_numpy(payload).cuda()
    return (lambda: preprocess.jpeg_reconstruct(dev, header)), header, payload


def kernels_only(iters):
    """The child process rocprofv3 traces: nothing but the call."""
    fn, _, _ = reconstruct_call(the_file())
    for _ in range(iters + 5):
        fn()
    torch.cuda.synchronize()


def kernel_stats(iters, keep):
    """{kernel substring: (mean us, min us, max us, calls)} from a rocprofv3 --kernel-trace --stats child run."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
               os.path.abspath(__file__), "--kernels-only", "--iters", str(iters)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise SystemExit(f"rocprofv3 failed ({r.returncode}):\n{r.stderr[-2000:]}")
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            raise SystemExit("rocprofv3 wrote no kernel_stats.csv")
        out = {}
        with open(found[0]) as f:
            rows = list(csv.DictReader(f))
        for row in rows:
            for key in ("k_jpeg_idct", "k_jpeg_rgb"):
                if key in row["Name"]:
                    out[key] = (float(row["AverageNs"]) / 1e3, float(row["MinNs"]) / 1e3, float(row["MaxNs"]) / 1e3,
                                int(row["Calls"]))
        if keep:
            with open(keep, "w") as f:
                w = csv.DictWriter(f, fieldnames=list(rows[0].keys()), quoting=csv.QUOTE_NONNUMERIC)
                w.writeheader()
                w.writerows(row for row in rows if "k_jpeg" in row["Name"])
        return out


def device_lines(data, iters, warm, stats):
    fn, header, payload = reconstruct_call(data)
    want = jpeg_ref.pillow_rgb(data)
    assert np.array_equal(fn().cpu().numpy(), want), "the device decode differs from Pillow's"
    for _ in range(warm):
        fn()
    t = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b) * 1e3)
    b1, b2 = traffic(header)
    lines = [f"device, msl_jpeg_reconstruct on that file's {payload.size} payload bytes (equal to Pillow's decode on every "
             "byte):",
             f"  both launches, device events around single calls, {iters} after {warm} warm-up:   median "
             f"{statistics.median(t):7.1f} us   min {min(t):7.1f}   max {max(t):7.1f}",
             f"  per kernel, rocprofv3 --kernel-trace --stats over a child process that runs only the call; bytes from "
             f"the shapes; achievable HBM {HBM / 1e12:.1f} TB/s:"]
    for key, nbytes, what in (("k_jpeg_idct", b1, "dequantise + IDCT + clamp"), ("k_jpeg_rgb", b2, "upsample + colour")):
        if key not in stats:
            lines.append(f"  {key:<12} not measured")
            continue
        mean, lo, hi, calls = stats[key]
        rate = nbytes / (mean * 1e-6)
        lines.append(f"  {key:<12} ({what})   mean {mean:7.1f} us   min {lo:7.1f}   max {hi:7.1f}   ({calls} calls)   "
                     f"{nbytes / 1e6:5.1f} MB -> {rate / 1e9:7.1f} GB/s = {100 * rate / HBM:4.1f} % of achievable HBM")
    return lines + [""]


def host_lines(data, iters):
    from PIL import Image
    import io
    from maxsquareloss_amd import hip
    from maxsquareloss_amd.utils import jpeg
    lib = hip.load()
    header = hip.JpegHeader()
    assert lib.msl_jpeg_info(data, len(data), ctypes.addressof(header)) == 0
    elems = lib.msl_jpeg_coef_elems(ctypes.addressof(header))
    coef, quant = np.empty(elems, np.int16), np.empty(256, np.uint16)
    args = (data, len(data), ctypes.addressof(header), coef.ctypes.data, elems, quant.ctypes.data)
    t_pil = host_clock(lambda: np.asarray(Image.open(io.BytesIO(data)).convert("RGB")), iters)
    t_raw = host_clock(lambda: lib.msl_jpeg_entropy_decode(*args), iters)
    slot = np.empty(jpeg.COEF_AT + 2 * elems, np.uint8)
    t_file = host_clock(lambda: jpeg.decode_file(data, lambda n: slot[:n]), iters)
    fmt = lambda v: f"median {statistics.median(v):7.2f} ms   min {min(v):7.2f}   max {max(v):7.2f}"  # noqa: E731
    import PIL
    from PIL import features
    return [f"host, one thread, {W}x{H} 4:2:0 quality 92 ({len(data)} bytes; Pillow {PIL.__version__}, libjpeg-turbo "
            f"{features.version('libjpeg_turbo')}), {iters} decodes each:",
            f"  Pillow, the whole decode to an RGB array            {fmt(t_pil)}",
            f"  msl_jpeg_entropy_decode into an existing buffer      {fmt(t_raw)}",
            f"  utils/jpeg.py decode_file into the caller's buffer   {fmt(t_file)}", ""]


def loader_lines(n_files, epochs, repeats, workers=8):
    from maxsquareloss_amd.datasets import CrossCity_DataLoader
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "Rome")
        for d in ("Images/Train", "Images/Test", "Labels/Test", "List"):
            os.makedirs(os.path.join(root, d))
        with open(os.path.join(root, "List", "train.txt"), "w") as f:
            for i in range(n_files):
                with open(os.path.join(root, "Images", "Train", f"im_{i:03d}.jpg"), "wb") as g:
                    g.write(the_file(10 + i))
                f.write(f"im_{i:03d}\n")
        open(os.path.join(root, "List", "test.txt"), "w").close()
        paths = {"data_root_path": root, "list_path": os.path.join(root, "List"), "gt_path": None}

        def make(mode):
            a = argparse.Namespace(base_size=(1024, 512), crop_size=(1024, 512), seg_size=(1024, 512), random_mirror=True,
                                   random_crop=False, resize=True, DA=False, seed=3, split="train", class_16=False,
                                   class_13=True, batch_size=1, data_loader_workers=workers, jpeg_decode=mode)
            return CrossCity_DataLoader(a, training=True, datasets_path=paths)

        loaders = {mode: make(mode) for mode in ("device", "pillow")}

        def epoch_rate(ld):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 0
            for _ in range(epochs):
                for img, _, _ in ld.data_loader:
                    n += 1
            torch.cuda.synchronize()
            return n / (time.perf_counter() - t0)

        first = {m: next(iter(ld.data_loader))[0] for m, ld in loaders.items()}
        for ld in loaders.values():
            ld.data_loader.epoch = 0
        same = torch.equal(first["device"], first["pillow"])
        rates = {m: [] for m in loaders}
        for m, ld in loaders.items():
            epoch_rate(ld)  # warm-up: staging slots, tables, code objects
        for _ in range(repeats):  # alternating
            for m, ld in loaders.items():
                rates[m].append(epoch_rate(ld))
        for ld in loaders.values():
            ld.close()
    lines = [f"loader, CrossCity_DataLoader over {n_files} such files (2048x1024 -> 1024x512 BICUBIC, mirror drawn), "
             f"{workers} decoding threads of the 16 CPUs a job gets, {repeats} alternating runs of {epochs} epochs each "
             f"after one warm-up epoch; first items bit-identical: {same}:"]
    for m in ("device", "pillow"):
        r = rates[m]
        lines.append(f"  --jpeg_decode {m:<7} median {statistics.median(r):7.1f} items/s   (runs: "
                     f"{', '.join(f'{v:.1f}' for v in r)}; spread {max(r) - min(r):.1f})")
    d, p = statistics.median(rates["device"]), statistics.median(rates["pillow"])
    lines += [f"  device / pillow = {d / p:.2f}: the default of --jpeg_decode stays `device` only if this is not below 1", ""]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crosscity_pipeline_times.txt"))
    ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "crosscity_kernel_stats.csv"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_crosscity_pipeline.py measures on the GPU; none is visible")
    if a.kernels_only:
        return kernels_only(a.iters)
    stats = kernel_stats(a.iters, a.stats_out)
    torch.set_num_threads(1)
    data = the_file()
    lines = [f"Cross-city JPEG input pipeline, {torch.cuda.get_device_name(0)}, torch {torch.__version__}", ""]
    lines += host_lines(data, max(a.iters // 2, 8))
    lines += device_lines(data, a.iters, a.warmup, stats)
    lines += loader_lines(a.files, a.epochs, a.repeats)
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
