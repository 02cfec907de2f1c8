"""The reference's style-transfer interface (utils/style_transform.py, tools/function.py,
Trainer.seg_transform of tools/train_source.py) over the HIP style pass (tools/net.StyleNet).

  calc_mean_std, adaptive_instance_normalization   the reference's functions on device tensors
  style_transfer(net, content, style, alpha, interpolation_weights)
                                                   the reference's inner style_transfer: (1, 3, H', W')
  seg_transform(tensor, mean)                      a stylised tensor as the segmentation network's input

Content and style may differ in size: only the (S, 2, 512) statistics of relu4_1 cross from one to the
other, so a run over a dataset encodes its style once (net.encode_style) and passes the statistics instead
of the images.  The output is H' x W' = the content size rounded up to multiples of 8 (tools/net.out_hw),
as in the reference, whose ceil-mode pools and x2 up-samplings do the same.

Not here: preserve_color (the reference's coral(), an SVD on the host) raises NotImplementedError; the
style network's training and the trainer's source_aug / target_aug loops are out of scope.
"""
import torch

from .. import ops
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


def seg_transform(tensor, mean=IMG_MEAN):
    """Trainer.seg_transform: a stylised (1, 3, H, W) RGB tensor as the segmentation network's input,
    clamp(x * 255 + 0.5, 0, 255) in B, G, R order minus `mean` (B, G, R), not truncated to integers."""
    return ops.style_output(tensor.float(), rgb=False, seg=True, mean=[float(m) for m in mean])[1]


def to_uint8(tensor):
    """torchvision save_image's quantisation of a (1, 3, H, W) RGB tensor: uint8 (H, W, 3)."""
    return ops.style_output(tensor.float(), rgb=True, seg=False)[0]
