"""The reference's style-transfer interface (utils/style_transform.py, tools/function.py,
Trainer.seg_transform of tools/train_source.py) over the HIP style pass (tools/net.StyleNet).

  calc_mean_std, adaptive_instance_normalization   the reference's functions on device tensors
  style_transfer(net, content, style, alpha, interpolation_weights)
                                                   the reference's inner style_transfer: (1, 3, H', W')
  seg_transform(tensor, label, size, mean)         a stylised tensor as the segmentation network's input, resized
                                                   to seg_size with its label
  stylise_for_seg(net, content, style_stats, seg_size)
                                                   content -> style pass -> segmentation input, no torch op between
  crop_trans(net, content, style_stats, crop_size, base_size, seg_size)
                                                   the reference's cropTrans (tools/ADAIN.py) + seg_transform

Content and style may differ in size: only the (S, 2, 512) statistics of relu4_1 cross from one to the
other, so a run over a dataset encodes its style once (net.encode_style) and passes the statistics instead
of the images.  The output is H' x W' = the content size rounded up to multiples of 8 (tools/net.out_hw),
as in the reference, whose ceil-mode pools and x2 up-samplings do the same.

Not here: preserve_color (the reference's coral(), an SVD on the host) raises NotImplementedError; the
style network's training is out of scope.  The in-loop trainer over these functions is tools/ADAIN.py.
"""
import functools

import numpy as np
import torch

from .. import ops
from ..hip import MSLError
from .synthetic import IMG_MEAN


def _images(feat, name):
    if feat.dim() != 4:
        raise ValueError(f"{name}: expected (N, C, H, W), got {tuple(feat.shape)}")
    return [feat[n:n + 1].float().contiguous() for n in range(feat.size(0))]


def calc_mean_std(feat, eps=1e-5):
    """((N, C, 1, 1) mean, (N, C, 1, 1) sqrt(unbiased variance + eps)) of a device tensor (N, C, H, W)."""
    stats = torch.stack([ops.style_stats(x, relu=False) for x in _images(feat, "calc_mean_std")])  # (N, 2, C)
    n, c = feat.shape[:2]
    return stats[:, 0].reshape(n, c, 1, 1), (stats[:, 1] + eps).sqrt().reshape(n, c, 1, 1)


def adaptive_instance_normalization(content_feat, style_feat):
    """content_feat normalised per channel to style_feat's mean and standard deviation, image by image."""
    if content_feat.shape[:2] != style_feat.shape[:2]:
        raise ValueError(f"adaptive_instance_normalization: {tuple(content_feat.shape)} vs {tuple(style_feat.shape)}")
    out = []
    for x, s in zip(_images(content_feat, "adaptive_instance_normalization"),
                    _images(style_feat, "adaptive_instance_normalization")):
        a, b = ops.style_adain_coef(ops.style_stats(x, relu=False), ops.style_stats(s, relu=False)[None])
        out.append(ops.style_pad(x, a=a, b=b)[:, :, 1:-1, 1:-1])
    return torch.cat(out).contiguous()


def style_transfer(net, content, style, alpha=1.0, interpolation_weights=None, preserve_color=False):
    """The decoder's output (1, 3, H', W') for `content` (1, 3, H, W) in the style of `style`: a float
    (S, 3, h, w) tensor in [0, 1], or the (S, 2, 512) statistics net.encode_style returned for it.  With
    several styles `interpolation_weights` (summing to 1, as the reference normalises them) mixes them."""
    if preserve_color:
        raise NotImplementedError("preserve_color (coral) is not part of the HIP style pass")
    if content.dim() != 4 or content.size(0) != 1:
        raise ValueError(f"style_transfer: content must be (1, 3, H, W), got {tuple(content.shape)}")
    stats = style if style.dim() == 3 else net.encode_style(style)
    weights = None if interpolation_weights is None else [float(w) for w in interpolation_weights]
    y = net.stylize(content.to(net.device).float(), stats, alpha, weights)
    return y[:, :3, 1:-1, 1:-1].contiguous()


def _resize_label(label, hw):
    """An int64 label map (..., H, W) on the device at hw = (H', W'), torch's nearest rule; its leading
    dimensions are kept."""
    if label is None or tuple(label.shape[-2:]) == tuple(hw):
        return label
    lead = tuple(label.shape[:-2])
    out = ops.label_resize_nearest(label.reshape(label.shape[-2:]).to(torch.int64), hw)
    return out.reshape(lead + tuple(hw))


def seg_transform(tensor, label=None, size=None, mean=IMG_MEAN):
    """Trainer.seg_transform: a stylised (1, 3, H, W) RGB tensor as the segmentation network's input,
    clamp(x * 255 + 0.5, 0, 255) in B, G, R order minus `mean` (B, G, R), not truncated to integers.
    With `size` = (W, H), the reference's seg_size, the image is first resized to it by torch's nearest rule
    (F.interpolate's default), in the same launch.  With `label` (int64 trainIds (..., H, W) on the device)
    returns (image, label resized with it), else the image alone."""
    mean = [float(m) for m in mean]
    tensor = tensor.float()
    if size is None or (int(size[1]), int(size[0])) == tuple(tensor.shape[-2:]):
        img = ops.style_output(tensor, rgb=False, seg=True, mean=mean)[1]
    else:
        img = torch.empty((1, 3, int(size[1]), int(size[0])), dtype=torch.float32, device=tensor.device)
        ops.style_output_resampled(tensor, img, mean=mean)
    if label is None:
        return img
    return img, _resize_label(label, tuple(img.shape[-2:]))


def _seg_out(out, hs, ws, device, name):
    """The (1, 3, hs, ws) fp32 tensor a function fills: `out` (a captured step's static input), or a new one."""
    if out is None:
        return torch.empty((1, 3, hs, ws), dtype=torch.float32, device=device)
    if tuple(out.shape) != (1, 3, hs, ws):
        raise MSLError(f"{name}: out is {tuple(out.shape)}, the result (1, 3, {hs}, {ws})")
    return out


def stylise_for_seg(net, content, style_stats, seg_size=None, alpha=1.0, weights=None, mean=IMG_MEAN, window=None,
                    size=None, out=None):
    """content -> style pass -> the segmentation network's input (1, 3, Hs, Ws), seg_size = (Ws, Hs): the
    reference's self.network(content, batch_style) followed by seg_transform, with no torch op on an
    image-sized tensor - the decoder's grid goes through one launch that resamples, quantises, reorders
    and subtracts `mean`.  `content`, `window`, `size` as StyleNet.encode takes them; seg_size None keeps
    the style pass's own size (tools/net.out_hw); `out` receives the result in place."""
    y = net.stylize(content, style_stats, alpha, weights, window, size)
    h, w = y.size(2) - 2, y.size(3) - 2
    mean = [float(m) for m in mean]
    hs, ws = (h, w) if seg_size is None else (int(seg_size[1]), int(seg_size[0]))
    if out is None and (hs, ws) == (h, w):
        return ops.style_output(y[:, :3], grid=True, rgb=False, seg=True, mean=mean)[1]
    return ops.style_output_resampled(y[:, :3], _seg_out(out, hs, ws, y.device, "stylise_for_seg"), grid=True, mean=mean)


def nearest_index(n_in, n_out):
    """torch's nearest source index of every destination cell of an axis resized from n_in to n_out cells, as
    the kernels form it: min(floor(d * scale), n_in - 1) with scale = n_in / n_out and the product in fp32."""
    scale = np.float32(n_in) / np.float32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n_in - 1)


@functools.lru_cache(maxsize=64)
def _quadrant_span(full, dest, off, mid):
    """(first, count) of the destination cells whose nearest source in a stitched axis of `full` cells lies
    in [off, off + mid): a contiguous run, the map being monotone."""
    src = nearest_index(full, dest)
    hit = np.nonzero((src >= off) & (src < off + mid))[0]
    return (int(hit[0]), int(hit.size)) if hit.size else (0, 0)


def crop_trans(net, content, style_stats, crop_size, base_size, seg_size=None, alpha=1.0, weights=None,
               mean=IMG_MEAN, out=None):
    """The reference's cropTrans followed by seg_transform, as the segmentation network's input (1, 3, Hs, Ws):
    each quadrant of `content` (uint8 (H, W, 3) or float (1, 3, H, W) of 2 * crop_size) is magnified to
    base_size, stylised, resized to crop_size, the four are stitched and the whole resized to seg_size
    (default: 2 * crop_size, no second resize).  Sizes are (W, H) as the reference's flags.  The magnified
    quadrant and the stitched image are never written: the first launch of a pass gathers from the content
    (ops.style_input_window) and its last one fills the quadrant's share of the result through the two
    composed index maps (ops.style_output_resampled).  `out` receives the result in place."""
    cw, ch = int(crop_size[0]), int(crop_size[1])
    bw, bh = int(base_size[0]), int(base_size[1])
    if (bw, bh) != (2 * cw, 2 * ch):
        raise MSLError(f"crop_trans: base_size {bw},{bh} must be twice crop_size {cw},{ch}")
    ih, iw = (content.size(0), content.size(1)) if content.dtype == torch.uint8 else tuple(content.shape[-2:])
    if (ih, iw) != (2 * ch, 2 * cw):
        raise MSLError(f"crop_trans: the content is {iw},{ih} but its quadrants must be crop_size {cw},{ch}")
    ws, hs = (2 * cw, 2 * ch) if seg_size is None else (int(seg_size[0]), int(seg_size[1]))
    mean = [float(m) for m in mean]
    out = _seg_out(out, hs, ws, net.device, "crop_trans")
    for qy in (0, 1):
        for qx in (0, 1):
            y = net.stylize(content, style_stats, alpha, weights, window=(qx * cw, qy * ch, cw, ch), size=(bh, bw))
            dy0, dh = _quadrant_span(2 * ch, hs, qy * ch, ch)
            dx0, dw = _quadrant_span(2 * cw, ws, qx * cw, cw)
            if dh and dw:
                ops.style_output_resampled(y[:, :3], out, (dx0, dy0, dw, dh), grid=True, mid=(ch, cw),
                                           full=(2 * ch, 2 * cw), off=(qy * ch, qx * cw), mean=mean)
    return out


def to_uint8(tensor):
    """torchvision save_image's quantisation of a (1, 3, H, W) RGB tensor: uint8 (H, W, 3)."""
    return ops.style_output(tensor.float(), rgb=True, seg=False)[0]
