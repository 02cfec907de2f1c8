"""The evaluator on the GPU: msl_predict_up against the torch-CPU restatement (tests/evaluate_ref.py), the
eval-mode forward (running statistics) and the flip pair against the oracle, Evaluater.validate() eager and as a
captured graph, and the trainers' --val_images.

Kernel level (counter_normal logits, std 3, one NaN low-res logit, labels with -1, C and 255):
  - no flip: the class map and the matrix match exactly (the upsample is bit-exact against torch-CPU);
  - flip: the class equals the restatement's wherever its near-tie mask (top-2 gap of the averaged probability
    < 1e-5) is clear and is one of its two leading classes elsewhere; the mask may cover 0.1 % of the pixels.
    Measured on CPU for these inputs (SHAPES order): 1 of 2145 pixels (4.7e-4), 0, 0, 0, 45 of 524288 (8.6e-5).
Model level at 128 x 256 (low-res 17 x 33): the project's 1e-3 normwise bound on the logits (test_gpu_configs).
"""
import argparse
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import evaluate_ref as ref  # noqa: E402
from oracle import msl_oracle as orc  # noqa: E402
from maxsquareloss_amd import hip, ops  # noqa: E402
from maxsquareloss_amd.utils.eval import Eval  # noqa: E402
from maxsquareloss_amd.utils.synthetic import synthetic_image  # noqa: E402

H, W = 128, 256


# ----------------------------------------------------------------------------- kernel level
def _case(C, hi, wi, ho, wo):
    return (ref.logits(C, hi, wi, nan=True), ref.logits(C, hi, wi, tag="Lf"), ref.labels(C, ho, wo))


def _device_run(low, lowf, lab, hw):
    """(class map, matrix) of one ops.predict_up call with both outputs."""
    C = low.size(1)
    cm = torch.zeros(C * C, dtype=torch.int64, device="cuda")
    arg = ops.predict_up(low.cuda(), hw, None if lowf is None else lowf.cuda(), lab.cuda().reshape(-1), cm,
                         want_argmax=True)
    torch.cuda.synchronize()
    return arg.cpu().numpy().astype(np.int64), cm.view(C, C).cpu().numpy()


@pytest.mark.parametrize("C,hi,wi,ho,wo", ref.SHAPES)
def test_predict_up_no_flip_is_exact(C, hi, wi, ho, wo):
    low, _, lab = _case(C, hi, wi, ho, wo)
    hw = (ho, wo)
    cls, _, _ = ref.predict_ref(low, hw)
    want = ref.confusion_ref(lab.numpy(), cls, C)
    arg, cm = _device_run(low, None, lab, hw)
    assert np.array_equal(arg, cls)
    assert np.array_equal(cm, want) and cm.sum() == int(((lab >= 0) & (lab < C)).sum())
    # a second call accumulates; the predict-only and the matrix-only forms agree with the full call
    dev_cm = torch.from_numpy(cm.reshape(-1).copy()).cuda()
    assert ops.predict_up(low.cuda(), hw, None, lab.cuda().reshape(-1), dev_cm) is None
    only_arg = ops.predict_up(low.cuda(), hw, want_argmax=True)
    torch.cuda.synchronize()
    assert np.array_equal(dev_cm.view(C, C).cpu().numpy(), 2 * want)
    assert np.array_equal(only_arg.cpu().numpy().astype(np.int64), cls)


@pytest.mark.parametrize("C,hi,wi,ho,wo", ref.SHAPES)
def test_predict_up_flip_matches_off_the_near_ties(C, hi, wi, ho, wo):
    low, lowf, lab = _case(C, hi, wi, ho, wo)
    hw = (ho, wo)
    cls, near, top2 = ref.predict_ref(low, hw, lowf)
    share = near.mean()
    print(f"flip C={C} {hi}x{wi} -> {ho}x{wo}: near-tie share {share:.2e} ({int(near.sum())} pixels)")
    assert share <= 1e-3
    arg, cm = _device_run(low, lowf, lab, hw)
    assert np.array_equal(arg[~near], cls[~near])
    assert ((arg[near] == top2[0][near]) | (arg[near] == top2[1][near])).all()
    g = lab.numpy().reshape(-1)
    keep = (g >= 0) & (g < C)
    assert cm.sum() == int(keep.sum())  # every labelled pixel counted once
    assert np.array_equal(cm, ref.confusion_ref(g, arg, C))  # the matrix is the one of the class map written
    assert np.abs(cm - ref.confusion_ref(g, cls, C)).sum() <= 2 * int((near & keep).sum())
    only_arg = ops.predict_up(low.cuda(), hw, lowf.cuda(), want_argmax=True)
    assert np.array_equal(only_arg.cpu().numpy().astype(np.int64), arg)


def test_predict_up_rejects_bad_arguments():
    lib = hip.load()
    low = torch.zeros(1, 33, 3, 3, device="cuda")
    with pytest.raises(hip.MSLError, match=r"status -3"):  # MSL_ERR_ARG: the register arrays hold 32 classes
        ops.predict_up(low, (7, 9), want_argmax=True)
    low = torch.zeros(1, 19, 3, 3, device="cuda")
    arg = torch.zeros(63, dtype=torch.int32, device="cuda")
    lab = torch.zeros(63, dtype=torch.int64, device="cuda")
    s = hip.stream_ptr()
    assert lib.msl_predict_up(low.data_ptr(), None, 19, 3, 3, 7, 9, None, None, None, s) == -3  # no output
    assert lib.msl_predict_up(low.data_ptr(), None, 19, 3, 3, 7, 9, lab.data_ptr(), None, arg.data_ptr(), s) == -3
    assert lib.msl_predict_up(None, None, 19, 3, 3, 7, 9, None, None, arg.data_ptr(), s) == -3
    assert lib.msl_predict_up(low.data_ptr(), None, 19, 3, 3, 0, 9, None, None, arg.data_ptr(), s) == -3  # geometry
    assert lib.msl_predict_up(low.data_ptr(), None, 19, 3, 3, 7, 9, None, None, arg.data_ptr(), s) == 0
    torch.cuda.synchronize()
    with pytest.raises(hip.MSLError):
        ops.predict_up(low, (7, 9))  # nothing to compute
    with pytest.raises(hip.MSLError):
        ops.predict_up(low, (7, 9), label=lab)  # label without a matrix


@pytest.mark.parametrize("ho,wo", [(33, 65), (40, 70)])
def test_predict_up_ties_take_the_lowest_class(ho, wo):
    """Planes 3 and 7 identical and dominant, in L and in Lf: np.argmax's first maximum is class 3 at every pixel,
    for the logits (no flip) and for the averaged probabilities (equal inputs give equal exponentials)."""
    C, hi, wi = 19, 9, 17
    low, lowf = ref.logits(C, hi, wi), ref.logits(C, hi, wi, tag="Lf")
    for t in (low, lowf):
        t[0, 3] += 40.0
        t[0, 7] = t[0, 3]
    for flip in (None, lowf):
        arg = ops.predict_up(low.cuda(), (ho, wo), None if flip is None else flip.cuda(), want_argmax=True)
        assert (arg == 3).all().item()
        assert (torch.from_numpy(ref.predict_ref(low, (ho, wo), flip)[0]) == 3).all().item()


@pytest.mark.parametrize("C,hi,wi,ho,wo", ref.SHAPES[:4])
def test_add_batch_low_equals_add_batch_on_the_upsampled_logits(C, hi, wi, ho, wo):
    low, _, lab = _case(C, hi, wi, ho, wo)
    a, b = Eval(C), Eval(C)
    a.add_batch_low(lab.cuda(), low.cuda(), (ho, wo))
    b.add_batch(lab.cuda().view(1, ho, wo), ops.upsample_bilinear(low.cuda(), (ho, wo)))
    assert a.confusion_matrix.sum() > 0 and np.array_equal(a.confusion_matrix, b.confusion_matrix)


# ----------------------------------------------------------------------------- model level
def _argv(*extra):
    return ["--crop_size", f"{W},{H}", "--target_crop_size", f"{W},{H}", "--imagenet_pretrained", "False",
            "--save_dir", "", *extra]


def _normwise(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max()).item()


class _World:
    """One Evaluater (its model in eval mode with filled running statistics and spread logits), the oracle's
    copy of its state, and the oracle's eval-mode logits of one image and of its mirror - built once."""

    def __init__(self):
        from maxsquareloss_amd.tools import evaluate
        args, train_id, logger = evaluate.parse_args(_argv("--val_images", "3"))
        self.ev = evaluate.Evaluater(args, cuda=True, train_id=train_id, logger=logger)
        m = self.model = self.ev.model
        # running statistics = one image's batch statistics: a train-mode forward with momentum 1
        bns = [b for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d)]
        moms = [b.momentum for b in bns]
        for b in bns:
            b.momentum = 1.0
        m.train()
        with torch.no_grad():
            m._heads(synthetic_image(H, W, 70).cuda())
        for b, mo in zip(bns, moms):
            b.momentum = mo
        m.eval()
        # random-init logits have tiny class margins: scale layer6's two live head convs (the head is
        # linear in them, so the logits scale exactly) to a spread of std 2 over the classes
        self.x = synthetic_image(H, W, 71)
        low = m.predict_low(self.x.cuda())[0]
        k = 2.0 / ops.upsample_bilinear(low, (H, W)).std().item()
        with torch.no_grad():
            for conv in list(m.layer6.conv2d_list)[:2]:
                conv.weight.mul_(k)
                conv.bias.mul_(k)
        self.buffers = {n: b.detach().clone() for n, b in m.named_buffers()}
        self.oracle = orc.Model({n: v.detach().cpu() for n, v in m.state_dict().items()})
        with torch.no_grad():
            o = self.oracle
            self.ref = orc.forward_low(o.params, o.buffers, self.x, training=False)
            self.ref_flip = orc.forward_low(o.params, o.buffers, self.x.flip(-1), training=False)


@pytest.fixture(scope="module")
def world():
    return _World()


def test_eval_mode_forward_matches_the_oracle(world):
    m = world.model
    assert not m.training
    x2, x1 = m.predict_low(world.x.cuda())
    assert x2.shape == (1, 19, 17, 33) and not x2.requires_grad
    assert ops.upsample_bilinear(x2, (H, W)).std().item() >= 1.0
    for tag, g, r in zip(("x2", "x1"), (x2, x1), world.ref):
        e = _normwise(g, r)
        print(f"eval-mode {tag}: max|gpu - oracle| / max|oracle| = {e:.2e}")
        assert e < 1e-3, (tag, e)
    for n, b in m.named_buffers():  # running statistics and num_batches_tracked untouched
        assert torch.equal(b, world.buffers[n]), n
    # eval mode reads the running statistics: moving the stem BN's running mean moves its output (batch
    # statistics would not notice)
    bn, z = m.bn1, m.conv1(world.x.cuda()).detach()
    with torch.no_grad():
        y0 = ops.bn_act(bn, z, relu=True)
        bn.running_mean.add_(1.0)
        y1 = ops.bn_act(bn, z, relu=True)
        bn.running_mean.copy_(world.buffers["bn1.running_mean"])
        assert torch.equal(ops.bn_act(bn, z, relu=True), y0) and not torch.equal(y1, y0)


def test_flip_pair_matches_two_single_forwards(world):
    m = world.model
    (a2, a1), (f2, f1) = m.predict_low(world.x.cuda(), flip=True)
    for tag, g, r in zip(("x2", "x1"), (f2, f1), world.ref_flip):
        e = _normwise(g, r)
        print(f"flip pair, mirrored image {tag}: vs oracle {e:.2e}")
        assert e < 1e-3, (tag, e)
    for tag, g, r in zip(("x2", "x1"), (a2, a1), m.predict_low(world.x.cuda())):
        e = _normwise(g, r)  # the f16x3 operand scales span the pair: close, not bit-equal
        print(f"flip pair, first image {tag}: vs the single forward {e:.2e}")
        assert e < 1e-3, (tag, e)
    for n, b in m.named_buffers():
        assert torch.equal(b, world.buffers[n]), n


def _reference_matrix(world, flip):
    """The restatement run on the device's own low-res logits of the validator's items."""
    v, m = world.ev.validator, world.model
    C = 19
    cm, near_lab, labelled = np.zeros((C, C), dtype=np.int64), 0, 0
    for i in range(v.valid_iterations):
        x, y, _ = v.data[i]
        g = y.numpy().reshape(-1)
        keep = (g >= 0) & (g < C)
        if flip:
            (low, _), (lowf, _) = m.predict_low(x.cuda(), flip=True)
            cls, near, _ = ref.predict_ref(low.cpu(), (H, W), lowf.cpu())
        else:
            cls, near, _ = ref.predict_ref(m.predict_low(x.cuda())[0].cpu(), (H, W))
        cm += ref.confusion_ref(g, cls, C)
        near_lab += int((near & keep).sum())
        labelled += int(keep.sum())
    return cm, near_lab, labelled


@pytest.mark.parametrize("flip", [False, True])
def test_evaluater_validate(world, flip, capsys):
    ev = world.ev
    ev.validator.flip = flip
    PA, MPA, MIoU, FWIoU = ev.validate()
    out = capsys.readouterr().out
    assert "########## Eval" in out and out.count("===>") == 20  # the header and 19 class rows
    got = ev.Eval.confusion_matrix
    want, near_lab, labelled = _reference_matrix(world, flip)
    share = near_lab / labelled
    print(f"validate flip={flip}: near-tie share of the labelled pixels {share:.2e}; |diff| {np.abs(got - want).sum()}")
    assert ev.valid_iterations == 3 and got.sum() == labelled
    assert share <= 1e-2
    assert np.abs(got - want).sum() <= 2 * near_lab
    r = orc.eval_metrics(got)
    assert (PA, MPA, MIoU, FWIoU) == pytest.approx((r["PA"], r["MPA"], r["MIoU"], r["FWIoU"]), rel=1e-12)
    assert 0 < PA < 1 and np.isfinite(MIoU)


@pytest.mark.parametrize("flip", [False, True])
def test_graphed_validate_is_bit_identical_and_sees_weight_edits(world, flip):
    from maxsquareloss_amd.utils.validate import Validator
    m = world.model
    eager = Validator(m, 19, (H, W), 2, torch.device("cuda", 0), flip=flip)
    graphed = Validator(m, 19, (H, W), 2, torch.device("cuda", 0), flip=flip, graph=True)
    a = eager.run().confusion_matrix
    b = graphed.run().confusion_matrix
    gp = graphed._graphed[flip]
    assert gp.replays == 1 and a.sum() > 0 and np.array_equal(a, b)  # image 0 eager, image 1 replayed
    bias, weight = m.layer6.conv2d_list[0].bias, m.layer4[0].conv1.weight
    saved = (bias.detach().clone(), weight.detach().clone())
    try:
        with torch.no_grad():  # a bias the captured kernels read directly, and a weight they read as a pack
            bias[::2] += 1.5
            weight.mul_(1.25)
        b2 = graphed.run().confusion_matrix
        a2 = eager.run().confusion_matrix
        assert gp.replays == 3 and gp.eager_repacks == 1
        assert np.array_equal(a2, b2) and not np.array_equal(a2, a)
    finally:
        with torch.no_grad():
            bias.copy_(saved[0])
            weight.copy_(saved[1])
    assert np.array_equal(graphed.run().confusion_matrix, a)  # and back (another repack)


def test_trainer_validates_and_keeps_the_best(tmp_path):
    from maxsquareloss_amd.tools.train_source import Trainer, add_train_args, init_args
    argv = _argv("--synthetic_images", "2", "--iter_max", "200000", "--iter_stop", "2", "--val_images", "2")
    argv[argv.index("--save_dir") + 1] = str(tmp_path)
    args, _, _ = init_args(add_train_args(argparse.ArgumentParser()).parse_args(argv))
    tr = Trainer(args, cuda=True, train_id="t_")
    assert tr.epoch_num == 1 and tr.best_MIou == 0
    tr.train()
    assert tr.current_iter == 2 and tr.best_iter == 2
    assert np.isfinite(tr.current_MIoU) and tr.current_MIoU > 0 and tr.best_MIou == tr.current_MIoU
    assert tr._validator.Eval.confusion_matrix.sum() > 0
    best = os.path.join(str(tmp_path), "t_best.pth")
    assert os.path.exists(best) and os.path.exists(os.path.join(str(tmp_path), "t_final.pth"))
    kept, tr.best_MIou = tr.best_MIou, 0
    tr.load_checkpoint(best)
    assert tr.best_MIou == kept
