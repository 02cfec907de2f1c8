"""The AdaIN style network written out in torch.nn, independently of maxsquareloss_amd/tools/net.py: the
stacks whose index keys the reference's checkpoints carry, and the reference's style pass over them
(utils/style_transform.py: style_transfer inside style_transfer_AdaIN) in any dtype on the CPU.  Plain
helpers shared by test_style.py and test_gpu_style.py; no fixtures.
"""
import torch
import torch.nn as nn


def _pad_conv(cin, cout, relu=True):
    return [nn.ReflectionPad2d(1), nn.Conv2d(cin, cout, 3)] + ([nn.ReLU()] if relu else [])


def _pool():
    return nn.MaxPool2d((2, 2), (2, 2), (0, 0), ceil_mode=True)


def _up():
    return nn.Upsample(scale_factor=2, mode="nearest")


def ref_vgg():
    """VGG-19 with reflection-padded convs behind a 1x1 colour conv (53 children)."""
    return nn.Sequential(
        nn.Conv2d(3, 3, 1), *_pad_conv(3, 64), *_pad_conv(64, 64), _pool(),
        *_pad_conv(64, 128), *_pad_conv(128, 128), _pool(),
        *_pad_conv(128, 256), *_pad_conv(256, 256), *_pad_conv(256, 256), *_pad_conv(256, 256), _pool(),
        *_pad_conv(256, 512), *_pad_conv(512, 512), *_pad_conv(512, 512), *_pad_conv(512, 512), _pool(),
        *_pad_conv(512, 512), *_pad_conv(512, 512), *_pad_conv(512, 512), *_pad_conv(512, 512))


def ref_decoder():
    """The mirrored decoder from relu4_1 (29 children)."""
    return nn.Sequential(
        *_pad_conv(512, 256), _up(), *_pad_conv(256, 256), *_pad_conv(256, 256), *_pad_conv(256, 256),
        *_pad_conv(256, 128), _up(), *_pad_conv(128, 128), *_pad_conv(128, 64), _up(), *_pad_conv(64, 64),
        *_pad_conv(64, 3, relu=False))


def he_init(seq, seed):
    """Seeded He-normal weights and small biases: activations keep their scale through the stack."""
    g = torch.Generator().manual_seed(seed)
    for m in seq:
        if isinstance(m, nn.Conv2d):
            fan_in = m.in_channels * m.kernel_size[0] * m.kernel_size[1]
            with torch.no_grad():
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.05)
    return seq


def mean_std(feat, eps=1e-5):
    n, c = feat.shape[:2]
    var = feat.reshape(n, c, -1).var(dim=2) + eps
    return feat.reshape(n, c, -1).mean(dim=2).reshape(n, c, 1, 1), var.sqrt().reshape(n, c, 1, 1)


def adain(content_feat, style_feat):
    sm, ss = mean_std(style_feat)
    cm, cs = mean_std(content_feat)
    return (content_feat - cm) / cs * ss + sm


def mix(content_feat, style_feats, alpha, weights):
    """sum_i w_i adain(content, style_i) * alpha + content * (1 - alpha)."""
    feat = sum(w * adain(content_feat, s) for w, s in zip(weights, style_feats))
    return feat * alpha + content_feat * (1 - alpha)


def style_pass(vgg, dec, content, styles, alpha, weights, dtype):
    """The reference's pass in `dtype` on the CPU: content (1, 3, H, W), styles a list of (1, 3, h, w)."""
    enc = nn.Sequential(*list(vgg.children())[:31]).to(dtype)
    dec = dec.to(dtype)
    with torch.no_grad():
        cf = enc(content.to(dtype))
        out = dec(mix(cf, [enc(s.to(dtype)) for s in styles], alpha, weights))
    enc.float(), dec.float()
    return out
