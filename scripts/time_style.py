"""Times of the AdaIN style pass (tools/net.StyleNet over csrc/style.hip and msl_dconv_fwd), HIP events
after warm-up, seeded He-initialised weights (times do not depend on the values).

(a) Every launch of csrc/style.hip on its own, at its shape in one --size W,H stylisation, called through
    the C-ABI on preallocated buffers in windows of --calls calls; beside each the bytes it must move (from
    shapes) and the time those bytes take at 6.3 TB/s, what a streaming kernel reaches on an MI355X.
(b) One stylisation box to box - uint8 HWC image on the device in, uint8 HWC image on the device out, the
    style encoded once before - with --conv_math fp32 (the f16x3 form) and fp16, against torch running the
    same nn.Sequential stack on the same GPU (the reference's path on this hardware; --torch), alternating.

    python scripts/time_style.py [--torch] [--size 1024,512] [--out profiles/style_transfer_times.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from maxsquareloss_amd import hip, ops  # noqa: E402
from maxsquareloss_amd.tools import net  # noqa: E402

STREAM_TBS = 6.3


def he_init(seq, seed):
    g = torch.Generator().manual_seed(seed)
    for m in seq:
        if isinstance(m, nn.Conv2d):
            fan_in = m.in_channels * m.kernel_size[0] * m.kernel_size[1]
            with torch.no_grad():
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.05)
    return seq


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls  # us per call


def kernel_calls(sn, h, w):
    """[(label, fn, bytes)] of every csrc/style.hip launch of one stylisation of an h x w image."""
    lib, dev = hip.load(), "cuda"
    st = hip.stream_ptr()
    out = []
    img = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device=dev)
    grid = torch.empty((1, 3, h + 2, w + 2), device=dev)
    out.append((f"input   u8 {h}x{w} -> 3ch grid", lambda: hip.check(lib.msl_style_input(
        img.data_ptr(), None, h, w, sn.w1.data_ptr(), sn.b1.data_ptr(), grid.data_ptr(), 3, st), "input"),
        img.numel() + grid.numel() * 4))
    keep = [img, grid]
    ch, cw, cc = h, w, sn.enc_stages[0].cout
    ab = torch.rand((2, 512), device=dev)
    for name, stages in (("enc", sn.enc_stages[1:]), ("dec", sn.dec_stages)):
        for i, s in enumerate(stages):
            first_dec = name == "dec" and i == 0
            if first_dec:  # the statistics and the coefficients sit between the encoder and the decoder
                x = torch.randn((1, cc, ch + 2, cw + 2), device=dev)
                stats, sstats = torch.empty((2, cc), device=dev), torch.rand((1, 2, cc), device=dev)
                wsb = lib.msl_style_stats_workspace(cc, ch, cw)
                ws = hip.workspace(wsb, dev)
                out.append((f"stats   {cc}ch {ch}x{cw}", lambda x=x, stats=stats, ws=ws, wsb=wsb, c=cc, hh=ch, ww=cw:
                            hip.check(lib.msl_style_stats(x.data_ptr(), 1, c, hh, ww, 1, stats.data_ptr(), ws.data_ptr(),
                                                          wsb, st), "stats"), cc * ch * cw * 4))
                one = (ctypes.c_float * 1)(1.0)
                out.append((f"coef    {cc}ch", lambda stats=stats, sstats=sstats, c=cc, one=one: hip.check(
                    lib.msl_style_adain_coef(stats.data_ptr(), sstats.data_ptr(), ctypes.addressof(one), 1, c, 1.0, 1e-5,
                                             ab[0].data_ptr(), ab[1].data_ptr(), st), "coef"), cc * 6 * 4))
                keep += [x, stats, sstats, ws, one]
            ho, wo = ops.style_out_hw(ch, cw, s.resample)
            x = torch.randn((1, cc, ch + 2, cw + 2), device=dev)
            y = torch.empty((1, cc, ho + 2, wo + 2), device=dev)
            act = 2 if first_dec else ops.STYLE_ACT[s.act]
            a, b = (ab[0].data_ptr(), ab[1].data_ptr()) if first_dec else (None, None)
            read = cc * ch * cw * 4
            out.append((f"pad {name}{i + (1 if name == 'enc' else 0)} {cc}ch {ch}x{cw} {s.act if not first_dec else 'adain'}"
                        f"/{s.resample}", lambda x=x, y=y, c=cc, hh=ch, ww=cw, act=act, rs=ops.STYLE_RESAMPLE[s.resample],
                        a=a, b=b: hip.check(lib.msl_style_pad(x.data_ptr(), 1, c, hh, ww, act, rs, a, b, y.data_ptr(), c, st),
                                            "pad"), read + y.numel() * 4))
            keep += [x, y]
            ch, cw, cc = ho, wo, s.cout
    x = torch.rand((1, 3, ch + 2, cw + 2), device=dev)
    u8 = torch.empty((ch, cw, 3), dtype=torch.uint8, device=dev)
    seg = torch.empty((1, 3, ch, cw), device=dev)
    out.append((f"output  {ch}x{cw} -> u8", lambda: hip.check(lib.msl_style_output(
        x.data_ptr(), 1, ch, cw, u8.data_ptr(), None, 0.0, 0.0, 0.0, st), "output"), 3 * ch * cw * 5))
    out.append((f"output  {ch}x{cw} -> seg", lambda: hip.check(lib.msl_style_output(
        x.data_ptr(), 1, ch, cw, None, seg.data_ptr(), 104.0, 116.7, 122.7, st), "output"), 3 * ch * cw * 8))
    keep += [x, u8, seg, ab]
    return out, keep


class TorchPass:
    """The reference's path: the same stacks as torch modules on the GPU, fp32."""

    def __init__(self, vgg, dec, style_u8):
        self.enc = nn.Sequential(*list(vgg.children())[:net.ENCODER_CHILDREN]).cuda()
        self.dec = dec.cuda()
        with torch.no_grad():
            self.sm, self.ss = self.mean_std(self.enc(self.to_tensor(style_u8)))

    @staticmethod
    def to_tensor(u8):
        return u8.permute(2, 0, 1)[None].float().div(255)

    @staticmethod
    def mean_std(f):
        n, c = f.shape[:2]
        return (f.reshape(n, c, -1).mean(2).reshape(n, c, 1, 1),
                (f.reshape(n, c, -1).var(2) + 1e-5).sqrt().reshape(n, c, 1, 1))

    def __call__(self, u8):
        with torch.no_grad():
            cf = self.enc(self.to_tensor(u8))
            cm, cs = self.mean_std(cf)
            y = self.dec((cf - cm) / cs * self.ss + self.sm)
            return y[0].mul(255).add(0.5).clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "style_transfer_times.txt"))
    ap.add_argument("--size", default="1024,512", help="W,H of the content and the style image")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=5, help="stylisations per timed window")
    ap.add_argument("--torch", action="store_true", help="also time torch's own stack on the GPU")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_style.py measures on the GPU; none is visible")
    w, h = (int(v) for v in a.size.split(","))
    vgg, dec = he_init(net.make_vgg(), 21), he_init(net.make_decoder(), 22)
    sn = net.StyleNet(vgg.state_dict(), dec.state_dict(), "cuda")
    lines = [f"# AdaIN style pass at {w}x{h}, {torch.cuda.get_device_name(0)}; HIP events, medians over {a.rounds} rounds "
             f"after warm-up",
             f"# (a) each csrc/style.hip launch on its own, windows of {a.calls} calls on the same buffers (up to 256 MiB of "
             f"them can stay in the Infinity Cache between calls); floor = bytes / {STREAM_TBS} TB/s"]
    calls, keep = kernel_calls(sn, h, w)
    for _, fn, _ in calls:
        window(fn, 3)
    total_us = total_floor = 0.0
    for label, fn, nbytes in calls:
        t = statistics.median(window(fn, a.calls) for _ in range(a.rounds))
        floor = nbytes / (STREAM_TBS * 1e12) * 1e6
        if not label.endswith("-> seg"):
            total_us, total_floor = total_us + t, total_floor + floor
        lines.append(f"{label:44s} {t:8.1f} us   {nbytes / 1e6:8.2f} MB   floor {floor:7.1f} us   "
                     f"{nbytes / t / 1e6:5.2f} TB/s")
        print(lines[-1], flush=True)
    lines.append(f"sum over one stylisation (u8 output)          {total_us:8.1f} us   floor {total_floor:7.1f} us")
    del calls, keep
    torch.cuda.empty_cache()

    g = torch.Generator().manual_seed(5)
    content = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g).cuda()
    style = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g).cuda()
    stats = sn.encode_style([style])

    def ours():
        return ops.style_output(sn.stylize(content, stats), grid=True)[0]

    runs = {}
    for math in ("fp32", "fp16"):
        def run(math=math):
            ops.set_conv_math(math)
            return ours()
        runs["HIP pass, conv math " + math + (" (f16x3)" if math == "fp32" else "")] = run
    if a.torch:
        print("building torch's pass (its conv library may tune on first use) ...", flush=True)
        tp = TorchPass(vgg, dec, style)
        runs["torch nn.Sequential, fp32"] = lambda: tp(content)
    outs = {}
    for k, fn in runs.items():
        outs[k] = fn()
        window(fn, 2)
        print(f"warmed up: {k}", flush=True)
    times = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():
            times[k].append(window(fn, a.iters) / 1e3)
    ops.set_conv_math("fp32")
    lines.append(f"# (b) one stylisation box to box (uint8 HWC on the device in and out, style encoded once), ms, windows of "
                 f"{a.iters}, alternating")
    for k, t in times.items():
        t = sorted(t)
        lines.append(f"{k:36s} median {statistics.median(t):8.3f} ms   min {t[0]:8.3f}   max {t[-1]:8.3f}")
    ref = next(iter(outs.values())).int()
    for k, o in outs.items():
        d = (o.int() - ref).abs()
        lines.append(f"# output of '{k}' against the first: {tuple(o.shape)}, max |diff| {d.max().item()} levels, "
                     f"{(d > 0).float().mean().item() * 100:.3f} % of bytes differ")
    if a.torch:
        ks = list(times)
        lines.append(f"HIP (f16x3) / torch = {statistics.median(times[ks[0]]) / statistics.median(times[ks[-1]]):.3f} time")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
