"""Stylise a set of images with the AdaIN network - the reference's style_transfer_AdaIN
(utils/style_transform.py) as a tool, MI355X path.

    python -m maxsquareloss_amd.tools.stylize --content_dir datasets/GTA5/images --style ambulance.jpg \\
        --vgg vgg_normalised.pth --decoder decoder.pth --content_size 1024,512 --style_size 1024,512 \\
        --output_path out/ --save_ext png

The content images are the image files under --content_dir (searched recursively, sorted), or the paths
listed one per line in --content_list, relative to --content_root.  Pillow decodes them on
--data_loader_workers threads and resizes them to --content_size W,H with Image.BILINEAR (what
torchvision's Resize does to a PIL image); the device does the rest: /255, the encoder, AdaIN toward the
style statistics (encoded once, before the loop), the decoder, the 8-bit quantisation of torchvision's
save_image.  Files are encoded by utils/images.ImageWriter while the next image runs.

Several --style files are mixed by --style_interpolation_weight (integers, normalised to sum 1, as the
reference does).  Output names are the reference's: {content stem}_{H}r{W}_{style stem}.{ext} for one
style, {content stem}stylized.{ext} for a mix.  --keep_tree True instead writes each output under the
content's own relative path and file name (its extension decides the format), so that GTA5_Dataset /
City_Dataset read the stylised copy when --source_data_path / --target_data_path points at --output_path.
The output is the content size rounded up to multiples of 8 (tools/net.out_hw), as in the reference.

There is no default for --vgg / --decoder and no download: without them the tool stops.
"""
import argparse
import logging
import os
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .. import ops
from ..hip import MSLError
from ..utils.images import MAX_WRITER_THREADS, ImageWriter, parse_size
from .train_source import str2bool

IMAGE_EXTS = (".png", ".jpg", ".jpeg")


def build_parser():
    p = argparse.ArgumentParser(description="AdaIN stylisation of a set of images on the HIP kernels")
    p.add_argument("--content_dir", default=None, help="stylise every image file under this directory")
    p.add_argument("--content_list", default=None, help="a file of image paths, one per line, relative to --content_root")
    p.add_argument("--content_root", default=None, help="the directory --content_list's paths are relative to")
    p.add_argument("--style", nargs="+", default=None, help="the style image; several are interpolated")
    p.add_argument("--style_interpolation_weight", default="", help="integers, one per style, e.g. 1,1,2")
    p.add_argument("--vgg", default=None, help="the encoder's state dict (vgg_normalised.pth)")
    p.add_argument("--decoder", default=None, help="the decoder's state dict or training checkpoint")
    p.add_argument("--content_size", type=parse_size, default=None, metavar="W,H", help="resize contents to this size")
    p.add_argument("--style_size", type=parse_size, default=None, metavar="W,H", help="resize styles to this size")
    p.add_argument("--alpha", type=float, default=1.0, help="stylisation strength in [0, 1]")
    p.add_argument("--output_path", default=None, help="the directory the stylised images go under")
    p.add_argument("--save_ext", choices=("png", "jpg"), default="jpg")
    p.add_argument("--keep_tree", type=str2bool, default=False,
                   help="keep each content's relative path and file name under --output_path")
    p.add_argument("--data_loader_workers", type=int, default=4, help="host threads that decode and that encode")
    p.add_argument("--conv_math", choices=("fp32", "fp16", "bf16"), default="fp32")
    return p


def parse_args(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if not args.vgg or not args.decoder:
        parser.error("--vgg and --decoder are required: the style network has no default weights and nothing is "
                     "downloaded")
    if (args.content_dir is None) == (args.content_list is None):
        parser.error("give exactly one of --content_dir and --content_list")
    if args.content_list is not None and args.content_root is None:
        parser.error("--content_list needs --content_root")
    if not args.style:
        parser.error("--style is required")
    if not args.output_path:
        parser.error("--output_path is required")
    if not 0.0 <= args.alpha <= 1.0:
        parser.error("--alpha must lie in [0, 1]")
    args.weights = None
    if len(args.style) > 1:
        try:
            raw = [int(v) for v in args.style_interpolation_weight.split(",")]
        except ValueError:
            raw = []
        if len(raw) != len(args.style) or sum(raw) <= 0 or min(raw) < 0:
            parser.error(f"{len(args.style)} styles need --style_interpolation_weight with as many non-negative integers")
        args.weights = [v / sum(raw) for v in raw]
    return args


def content_items(args):
    """[(file, path relative to the content root)] in the order they are processed."""
    if args.content_list is not None:
        with open(args.content_list) as f:
            rel = [line.strip() for line in f if line.strip()]
        root = args.content_root
    else:
        root, rel = args.content_dir, []
        for d, _, files in os.walk(root):
            rel += [os.path.relpath(os.path.join(d, n), root) for n in files if n.lower().endswith(IMAGE_EXTS)]
        rel.sort()
    return [(os.path.join(root, r), r) for r in rel]


def output_name(relpath, h, w, styles, ext, keep_tree=False):
    """The output file, relative to --output_path, of the content at `relpath` resized to h x w."""
    if keep_tree:
        return relpath
    stem = os.path.splitext(os.path.basename(relpath))[0]
    if len(styles) > 1:
        return f"{stem}stylized.{ext}"
    return f"{stem}_{h}r{w}_{os.path.splitext(os.path.basename(styles[0]))[0]}.{ext}"


def load_image(path, size=None):
    """uint8 (H, W, 3) RGB of a file, resized to size = (W, H) as torchvision's Resize resizes a PIL image."""
    from PIL import Image
    with Image.open(path) as im:
        im = im.convert("RGB")
        if size is not None and im.size != tuple(size):
            im = im.resize(tuple(size), Image.BILINEAR)
        return np.asarray(im, dtype=np.uint8).copy()


def load_net(args, device="cuda"):
    from .net import StyleNet
    return StyleNet(torch.load(args.vgg, map_location="cpu"), torch.load(args.decoder, map_location="cpu"), device)


def run(args, logger=None):
    """Stylise every content item; returns the written paths, relative to --output_path."""
    logger = logger or logging.getLogger(__name__)
    if not torch.cuda.is_available():
        raise MSLError("tools/stylize.py runs the style network on the GPU; none is visible")
    items = content_items(args)
    if not items:
        raise MSLError("tools/stylize.py: no content images found")
    ops.set_conv_math(args.conv_math)
    net = load_net(args)
    workers = max(1, min(int(args.data_loader_workers), MAX_WRITER_THREADS))
    with torch.no_grad(), ThreadPoolExecutor(workers, thread_name_prefix="msl-decode") as pool, \
            ImageWriter(args.output_path, kinds=(), workers=workers) as writer:
        styles = list(pool.map(lambda p: load_image(p, args.style_size), args.style))
        style_stats = net.encode_style([torch.from_numpy(s) for s in styles])
        pending = deque()
        todo = iter(items)

        def submit():
            item = next(todo, None)
            if item is not None:
                pending.append((item[1], pool.submit(load_image, item[0], args.content_size)))

        for _ in range(workers + 1):
            submit()
        while pending:
            rel, fut = pending.popleft()
            img = torch.from_numpy(fut.result()).to(net.device, non_blocking=True)
            submit()
            y = net.stylize(img, style_stats, args.alpha, args.weights)
            u8, _ = ops.style_output(y[:, :3], grid=True)
            writer.save_as(output_name(rel, img.size(0), img.size(1), args.style, args.save_ext, args.keep_tree), u8)
        written = list(writer.written)
    logger.info("wrote %d stylised images under %s", len(written), args.output_path)
    return written


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    run(parse_args())
