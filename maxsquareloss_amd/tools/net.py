"""The AdaIN style network of the reference (tools/net.py): a VGG-19 encoder and a mirrored decoder as
nn.Sequential stacks whose index keys ("0.weight", "2.weight", ...) are the ones its checkpoints carry
(vgg_normalised.pth, decoder.pth / decoder_iter_*.pth.tar), and StyleNet, which runs them on the HIP
kernels (ops.style_* and ops.conv3x3_reflect; csrc/style.hip).

The two stacks exist to load and check state dicts and to say what the network is; StyleNet never calls
them.  It walks them once into stages - "make this conv's input grid out of the previous output (ReLU,
pool or up-sample, reflection border: one launch), then the conv" - and runs the stages.

Sizes: the encoder pools three times with ceil_mode=True and the decoder doubles three times, so a content
image of H x W comes out as H' x W' with H' = 8 * ceil(ceil(ceil(H / 2) / 2) / 2) (out_hw): H rounded up
to a multiple of 8, exactly as the reference's stacks behave.
"""
import torch
import torch.nn as nn

from .. import ops

# VGG-19's 3x3 convs in order; "M" a 2x2 ceil-mode max-pool.  Every conv is reflection-padded and followed
# by a ReLU; a 1x1 conv 3 -> 3 (the checkpoint's colour transform) leads.
_VGG_PLAN = (64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512)
# The decoder mirrors the encoder from relu4_1 (512 channels) down; "U" nearest x2; no ReLU after the last conv.
_DECODER_PLAN = (256, "U", 256, 256, 256, 128, "U", 128, 64, "U", 64, 3)
ENCODER_CHILDREN = 31  # the encoder up to relu4_1, all the style pass uses


def _conv_block(cin, cout, relu=True):
    block = [nn.ReflectionPad2d((1, 1, 1, 1)), nn.Conv2d(cin, cout, (3, 3))]
    return block + [nn.ReLU()] if relu else block


def make_vgg():
    layers, cin = [nn.Conv2d(3, 3, (1, 1))], 3
    for v in _VGG_PLAN:
        if v == "M":
            layers.append(nn.MaxPool2d((2, 2), (2, 2), (0, 0), ceil_mode=True))
        else:
            layers += _conv_block(cin, v)
            cin = v
    return nn.Sequential(*layers)


def make_decoder():
    layers, cin = [], 512
    for i, v in enumerate(_DECODER_PLAN):
        if v == "U":
            layers.append(nn.Upsample(scale_factor=2, mode="nearest"))
        else:
            layers += _conv_block(cin, v, relu=i + 1 < len(_DECODER_PLAN))
            cin = v
    return nn.Sequential(*layers)


vgg = make_vgg()
decoder = make_decoder()


def out_hw(h, w):
    """The size the style pass returns for an h x w content image."""
    def up8(n):
        for _ in range(3):
            n = (n + 1) // 2
        return 8 * n
    return up8(h), up8(w)


class Stage:
    """One 3x3 conv of the network and how its input grid is made from the previous output: `act` "relu" or
    "none", `resample` "none", "pool" or "up" (ops.style_pad's names)."""

    def __init__(self, conv, act, resample):
        self.cin, self.cout = conv.in_channels, conv.out_channels
        self.weight, self.bias = conv.weight.detach(), conv.bias.detach()
        self.act, self.resample = act, resample
        self.cache = ops.PackCache()


def stages_of(seq, act="none"):
    """(stages, the activation still pending after the last conv) of a stack that starts with a reflection-
    padded 3x3 conv; `act` is the activation pending from what came before."""
    stages, resample = [], "none"
    for m in seq:
        if isinstance(m, nn.ReLU):
            act = "relu"
        elif isinstance(m, nn.MaxPool2d):
            resample = "pool"
        elif isinstance(m, nn.Upsample):
            resample = "up"
        elif isinstance(m, nn.Conv2d):
            stages.append(Stage(m, act, resample))
            act, resample = "none", "none"
        elif not isinstance(m, nn.ReflectionPad2d):
            raise TypeError(f"style network: unexpected layer {m!r}")
    return stages, act


class StyleNet:
    """The encoder up to relu4_1 and the decoder, weights on `device`, run on the HIP kernels.

    vgg_state is the reference's vgg_normalised.pth state dict (all 53 children's keys; the first 31
    children are kept), decoder_state a decoder state dict, bare or as the reference's training saves it
    ({'state_dict': ..., 'loss_c_best': ...}).  A dict that does not fit the stacks raises (load_state_dict).
    """
    CHANNELS = 512  # of relu4_1, where the statistics cross

    def __init__(self, vgg_state, decoder_state, device="cuda"):
        enc, dec = make_vgg(), make_decoder()
        if "loss_c_best" in decoder_state:
            decoder_state = decoder_state["state_dict"]
        enc.load_state_dict(vgg_state)
        dec.load_state_dict(decoder_state)
        self.device = torch.device(device)
        enc = nn.Sequential(*list(enc.children())[:ENCODER_CHILDREN]).to(self.device).float()
        dec = dec.to(self.device).float()
        first = enc[0]
        self.w1, self.b1 = first.weight.detach().contiguous(), first.bias.detach().contiguous()
        self.enc_stages, pending = stages_of(list(enc.children())[1:])
        assert pending == "relu"  # relu4_1: the statistics and the AdaIN affine read relu(the last conv)
        self.dec_stages, pending = stages_of(dec.children())
        assert pending == "none" and self.dec_stages[-1].cout == 3

    # ------------------------------------------------------------------ geometry (no device needed)
    def conv_calls(self, h, w, decode=True):
        """(cin, cout, grid rows, grid columns) of every conv call of a pass over an h x w image, in order:
        the encoder's and, with `decode`, the decoder's."""
        calls = []
        for st in self.enc_stages + (self.dec_stages if decode else []):
            h, w = ops.style_out_hw(h, w, st.resample)
            calls.append((st.cin, st.cout, h + 2, w + 2))
        return calls

    # ------------------------------------------------------------------ the pass
    def encode(self, img, window=None, size=None):
        """relu4_1's conv output (before its ReLU) as a grid (1, 512, h+2, w+2) whose interior is valid, from
        a uint8 (H, W, 3) RGB image or a float (1, 3, H, W) tensor in [0, 1] on the device.  With `window`
        (x0, y0, cw, ch) and `size` (h, w): of that window of the image magnified to h x w by torch's nearest
        rule (ops.style_input_window: the reference's F.interpolate(crop, size) ahead of the network)."""
        y = None
        for i, st in enumerate(self.enc_stages):
            if i == 0 and window is not None:
                g = ops.style_input_window(img, window, size, self.w1, self.b1, cpad=st.cin)
            elif i == 0:
                g = ops.style_input(img, self.w1, self.b1, cpad=st.cin)
            else:
                g = ops.style_pad(y, grid=True, act=st.act, resample=st.resample)
            y = ops.conv3x3_reflect(g, st.weight, st.bias, st.cache)
        return y

    def stats(self, img):
        """(2, 512): mean and unbiased variance per channel of relu4_1 of one image."""
        return ops.style_stats(self.encode(img), grid=True, relu=True)

    def encode_style(self, style):
        """The style statistics (S, 2, 512) of S style images: a float (S, 3, h, w) tensor in [0, 1] or a
        list of uint8 (h, w, 3) images.  Encode once, pass to style_transfer for every content image."""
        imgs = [style[i:i + 1] for i in range(style.size(0))] if torch.is_tensor(style) else list(style)
        return torch.stack([self.stats(im.to(self.device)) for im in imgs])

    def decode(self, feat, a, b):
        """The decoder over a * relu(feat) + b (feat: encode()'s grid): the last conv's grid (1, 3, H'+2,
        W'+2), interior valid."""
        y = feat
        for i, st in enumerate(self.dec_stages):
            if i == 0:
                g = ops.style_pad(y, grid=True, act="relu_in", resample=st.resample, a=a, b=b)
            else:
                g = ops.style_pad(y, grid=True, act=st.act, resample=st.resample)
            y = ops.conv3x3_reflect(g, st.weight, st.bias, st.cache)
        return y

    def stylize(self, content, style_stats, alpha=1.0, weights=None, window=None, size=None):
        """The stylised image as the decoder's last grid (see decode): `content` (and `window`, `size`) as
        encode() takes it, `style_stats` from encode_style, `weights` the interpolation weights of several
        styles."""
        if weights is None:
            if style_stats.size(0) != 1:
                raise ValueError("several styles need interpolation weights")
            weights = (1.0,)
        if len(weights) != style_stats.size(0):
            raise ValueError(f"{len(weights)} interpolation weights for {style_stats.size(0)} styles")
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f"alpha must lie in [0, 1], got {alpha}")
        feat = self.encode(content, window, size)
        a, b = ops.style_adain_coef(ops.style_stats(feat, grid=True, relu=True), style_stats, weights, alpha)
        return self.decode(feat, a, b)
