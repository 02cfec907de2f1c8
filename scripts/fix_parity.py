"""Outputs, data gradients and weight gradients of the conv GEMMs at the step's shapes, saved for a
bitwise comparison of two library builds (MSL_LIB_PATH) or settings that must agree bit for bit
(r04: k_sk_reduce vs an in-launch fix-up of split stream-K tiles, profiles/r04_sk_fixup_ab.txt).

    fix_parity.py save OUT.pt [--conv-math fp32|fp16|bf16] [--f32-form mfma_f32|bf16x6|f16x3]
    fix_parity.py compare A.pt B.pt

Covered: the 3x3 and pointwise convs (y, dx, dW; dW also accumulated into a flat gradient buffer, one
pointwise case per weight-gradient orientation and one 3x3 case), the ASPP head (ops.aspp2, 2048 -> 19,
d 6 / 12), the stem (also with an accumulating weight), a residual BN + ReLU whose affine parameters
accumulate into a flat buffer, the 2048 -> 512 data gradient with the masked residual in its epilogue,
and every loss of ops (loss, IW outputs and the logits' gradient): the host wrappers of ops.py issue
these calls, so two versions of the package over one library must agree bit for bit too."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

if sys.argv[1] == "compare":
    a, b = torch.load(sys.argv[2], weights_only=True), torch.load(sys.argv[3], weights_only=True)
    bad = [k for k in a if k not in b or not torch.equal(a[k], b[k])] + [k for k in b if k not in a]
    for k in a:
        print(f"{k:48s} {'DIFFERENT' if k in bad else 'bit-identical'}")
    sys.exit(1 if bad else 0)

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["save"])
ap.add_argument("out")
ap.add_argument("--conv-math", default="fp32", choices=["fp32", "fp16", "bf16"])
ap.add_argument("--f32-form", default="f16x3", choices=["mfma_f32", "bf16x6", "f16x3"])
args = ap.parse_args()

from maxsquareloss_amd import ops  # noqa: E402
from maxsquareloss_amd.graphs.models import deeplab_multi as dm  # noqa: E402
from maxsquareloss_amd.utils.optim import FlatGrads  # noqa: E402

ops.set_f32_form(args.f32_form)
ops.set_conv_math(args.conv_math)
torch.manual_seed(0)
dev = "cuda"
out = {}


def act(c, nimg, h, w):
    return torch.randn(1, c, nimg, h, w, device=dev).requires_grad_()


def weight(*shape, acc=False):
    """A leaf weight; with `acc`, its .grad is a non-zero slice of a flat gradient buffer, so the weight
    gradient kernels accumulate into it in place (ops.grad_sink)."""
    wt = torch.nn.Parameter(torch.randn(*shape, device=dev) * 0.02)
    if acc:
        wt.flat = FlatGrads([wt], dev)
        wt.flat.flat.normal_()
    return wt


def record(name, y, x, wts):
    y.backward(torch.randn_like(y))
    out[name + " y"] = y.detach().cpu()
    out[name + " dx"] = x.grad.cpu()
    for i, wt in enumerate(wts):
        out[f"{name} dw{i}"] = wt.grad.detach().cpu()


for nimg in (1, 2):
    for (cin, cout, h, w, d, acc) in [(256, 256, 65, 129, 2, False), (64, 64, 129, 257, 1, False),
                                      (512, 512, 65, 129, 4, False), (2048, 19, 65, 129, 6, False),
                                      (256, 256, 65, 129, 2, True)]:
        x, wt = act(cin, nimg, h, w), weight(cout, cin, 3, 3, acc=acc)
        record(f"dconv {cin}->{cout} d{d} n{nimg}{' acc' if acc else ''}",
               ops.dconv3x3(x, wt, d, ops.PackCache()), x, [wt])
    for (cin, cout, h, w, acc) in [(1024, 256, 65, 129, False), (256, 1024, 65, 129, False),
                                   (2048, 512, 65, 129, False), (64, 256, 129, 257, False),
                                   (1024, 256, 65, 129, True), (256, 1024, 65, 129, True)]:
        x, wt = act(cin, nimg, h, w), weight(cout, cin, 1, 1, acc=acc)
        record(f"pconv {cin}->{cout} n{nimg}{' acc' if acc else ''}",
               ops.pconv(x, wt, ops.PackCache(pointwise=True)), x, [wt])
    # the ASPP head: two dilated branches with biases in one call
    x = act(2048, nimg, 65, 129)
    prm = [weight(19, 2048, 3, 3), weight(19), weight(19, 2048, 3, 3), weight(19)]
    record(f"aspp2 2048->19 d6/12 n{nimg}", ops.aspp2(x, prm[0], prm[1], prm[2], prm[3], 6, 12, ops.PackCache()),
           x, prm)
    # the stem: 7x7 stride 2 on the raw image (im2col + the pointwise GEMM)
    x = torch.randn(1, 3, nimg, 257, 513, device=dev).mul_(60).requires_grad_()
    wt = weight(64, 3, 7, 7)
    record(f"stem 3->64 n{nimg}", ops.stem_conv(x, wt, 2, 3, ops.PackCache(pointwise=True)), x, [wt])
    x = torch.randn(1, 3, nimg, 257, 513, device=dev).mul_(60).requires_grad_()
    wt = weight(64, 3, 7, 7, acc=True)
    record(f"stem 3->64 n{nimg} acc", ops.stem_conv(x, wt, 2, 3, ops.PackCache(pointwise=True)), x, [wt])
    # a residual BN + ReLU whose affine parameters accumulate in place into a flat gradient buffer
    bn = torch.nn.BatchNorm2d(256).to(dev).train()
    bn.flat = FlatGrads([bn.weight, bn.bias], dev)
    bn.flat.flat.normal_()
    x, res = act(256, nimg, 65, 129), act(256, nimg, 65, 129)
    record(f"bn_act 256 res relu n{nimg} acc", ops.bn_act(bn, x, residual=res, relu=True), x,
           [res, bn.weight, bn.bias])
    # a layer4 identity block: conv1's 2048 -> 512 data gradient applies bn3's ReLU mask to the residual
    # gradient in its epilogue (ops.MaskedResidual; the bf16 math materialises it)
    blk = dm.Bottleneck(2048, 512, dilation=4).to(dev).train()
    x = act(2048, nimg, 65, 129) if nimg > 1 else torch.randn(1, 2048, 65, 129, device=dev).requires_grad_()
    record(f"block 2048/512 d4 n{nimg}", blk(x), x, list(blk.parameters()))

# the losses: C = 19, the fused ones from 9 x 17 logits upsampled to 33 x 65, the others at 33 x 65
C, LOW, UP = 19, (9, 17), (33, 65)
labels = torch.randint(-1, C, (UP[0] * UP[1],), device=dev)
low2 = torch.randn(1, C, *LOW, device=dev) * 4
target = torch.softmax(torch.randn(1, C, *UP, device=dev) * 3, 1)
LOSSES = {
    "ce_up": (LOW, lambda t: ops.ce_up(t, labels, UP)),
    "maxsquare_up": (LOW, lambda t: ops.maxsquare_up(t, UP)),
    "iw_maxsquare_up": (LOW, lambda t: ops.iw_maxsquare_up(t, UP, 0.2)),
    "multi_ce_up": (LOW, lambda t: ops.multi_ce_up(t, low2, UP, 0.5)),
    "entropy_up": (LOW, lambda t: ops.entropy_up(t, UP)),
    "iw_entropy_up": (LOW, lambda t: ops.iw_entropy_up(t, UP, 0.2)),
    "hard_ce_up": (LOW, lambda t: ops.hard_ce_up(t, UP, 0.5)),
    "soft_ce": (UP, lambda t: ops.soft_ce(t, target)),
    "iw_soft_ce": (UP, lambda t: ops.iw_soft_ce(t, target, 0.2)),
    "maxsquare_prob": (UP, lambda t: ops.maxsquare_prob(torch.softmax(t, 1))),
    "iw_maxsquare_prob": (UP, lambda t: ops.iw_maxsquare_prob(torch.softmax(t, 1), labels, 0.2)),
}
for name, (hw, fn) in LOSSES.items():
    low = (torch.randn(1, C, *hw, device=dev) * 4).requires_grad_()
    res = fn(low)
    loss, iw = (res[0], res[1:]) if isinstance(res, tuple) else (res, ())
    (loss * 0.75).backward()
    out[name + " loss"] = loss.detach().cpu()
    out[name + " d low"] = low.grad.cpu()
    for tag, t in zip(("hist", "weights"), iw):
        out[f"{name} {tag}"] = t.cpu()
torch.save(out, args.out)
print(len(out), "tensors saved")
