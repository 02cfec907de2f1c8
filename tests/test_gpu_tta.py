"""GPU: multi-scale / mirror test-time augmentation (--scales): msl_predict_tta / msl_predict_tta_images against
the torch-CPU restatement (tests/tta_ref.py) and against today's --flip kernels, the input resize against
torch-CPU, and the scaled evaluator and prediction tool against hand-composed calls.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import evaluate_ref as er  # noqa: E402
import tta_ref as tr  # noqa: E402
from oracle import msl_oracle as orc  # noqa: E402
from maxsquareloss_amd import hip, ops  # noqa: E402
from maxsquareloss_amd.utils import palette, validate  # noqa: E402
from maxsquareloss_amd.utils.eval import Eval  # noqa: E402
from maxsquareloss_amd.utils.synthetic import synthetic_image  # noqa: E402

MAPS = ("class", "ids", "color", "confidence", "pseudo")


def _dev(ents):
    return [(L.cuda(), m) for L, m in ents]


def _run(ents, hw, lab):
    """(class map, matrix) of one ops.predict_tta call with both outputs."""
    C = ents[0][0].size(1)
    cm = torch.zeros(C * C, dtype=torch.int64, device="cuda")
    arg = ops.predict_tta(_dev(ents), hw, lab.cuda().reshape(-1), cm, want_argmax=True)
    torch.cuda.synchronize()
    return arg.cpu().numpy().astype(np.int64), cm.view(C, C).cpu().numpy()


# ----------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize("nan", [False, True], ids=["plain", "nan"])
@pytest.mark.parametrize("index", range(len(tr.CASES)), ids=tr.IDS)
def test_predict_tta_matches_the_restatement(index, nan):
    case = tr.CASES[index]
    C, _, hw, _ = case
    ents, ref = tr.entries(case, nan), tr.case_ref(index, nan)
    lab = er.labels(C, *hw)
    arg, cm = _run(ents, hw, lab)
    near = ref[1]
    print(f"tta {tr.IDS[index]} nan={nan}: {len(ents)} entries, near-tie share {near.mean():.2e}, "
          f"device differs from the restatement at {int((arg != ref[0]).sum())} pixels")
    assert near.mean() <= 1e-3
    assert tr.agrees(arg, ref)
    if nan:  # the pixels the planted NaN reaches are class 0 for the device too
        hit = np.isnan(tr.fuse(ents[1:2], hw)[0])
        assert hit.any() and not hit.all() and (arg[hit] == 0).all()
    g = lab.numpy().reshape(-1)
    keep = (g >= 0) & (g < C)
    assert cm.sum() == int(keep.sum())  # every labelled pixel counted once
    assert np.array_equal(cm, er.confusion_ref(g, arg, C))  # the matrix is the one of the class map written
    # a second call accumulates; the predict-only and the matrix-only forms agree with the full call
    dev_cm = torch.from_numpy(cm.reshape(-1).copy()).cuda()
    assert ops.predict_tta(_dev(ents), hw, lab.cuda().reshape(-1), dev_cm) is None
    only_arg = ops.predict_tta(_dev(ents), hw, want_argmax=True)
    torch.cuda.synchronize()
    assert np.array_equal(dev_cm.view(C, C).cpu().numpy(), 2 * cm)
    assert np.array_equal(only_arg.cpu().numpy().astype(np.int64), arg)


@pytest.mark.parametrize("C,hi,wi,ho,wo", er.SHAPES)
def test_two_entries_are_the_flip_rule_bit_for_bit(C, hi, wi, ho, wo):
    low, lowf, lab = er.logits(C, hi, wi, nan=True), er.logits(C, hi, wi, tag="Lf"), er.labels(C, ho, wo)
    hw = (ho, wo)
    arg, cm = _run([(low, 0), (lowf, 1)], hw, lab)
    want_cm = torch.zeros(C * C, dtype=torch.int64, device="cuda")
    want = ops.predict_up(low.cuda(), hw, lowf.cuda(), lab.cuda().reshape(-1), want_cm, want_argmax=True)
    assert np.array_equal(arg, want.cpu().numpy().astype(np.int64))
    assert np.array_equal(cm, want_cm.view(C, C).cpu().numpy()) and cm.sum() > 0


@pytest.mark.parametrize("C,hi,wi,ho,wo", [er.SHAPES[3], er.SHAPES[0], er.SHAPES[1]], ids=["wo%4==0", "odd_wo", "c16"])
def test_two_entries_write_the_flip_images_byte_for_byte(C, hi, wi, ho, wo):
    """The mirrored entry is close to the mirror of the first, as a network's is: the averaged probability then
    reaches every confidence bucket and both sides of both thresholds (two unrelated entries average below 0.9)."""
    low = er.logits(C, hi, wi, nan=True).cuda()
    lowf = (er.logits(C, hi, wi).flip(-1) + 0.3 * er.logits(C, hi, wi, tag="Lf")).cuda()
    lab = er.labels(C, ho, wo)
    hw = (ho, wo)
    for thr in (0.6, 0.95):
        cm_a, cm_b = (torch.zeros(C * C, dtype=torch.int64, device="cuda") for _ in range(2))
        got = ops.predict_tta_images([(low, 0), (lowf, 1)], hw, lab.cuda().reshape(-1), cm_a, want=MAPS, thr=thr)
        want = ops.predict_images(low, hw, lowf, lab.cuda().reshape(-1), cm_b, want=MAPS, thr=thr)
        for k in MAPS:
            assert torch.equal(got[k], want[k]), (k, thr)
        assert torch.equal(cm_a, cm_b) and cm_a.sum().item() > 0
    assert (got["pseudo"] == 255).any() and (got["pseudo"] != 255).any()
    assert len(torch.unique(got["confidence"].view(-1, 3), dim=0)) > 2
    # one map alone, no label: the same bytes
    alone = ops.predict_tta_images([(low, 0), (lowf, 1)], hw, want=("confidence",), thr=0.95)
    assert torch.equal(alone["confidence"], want["confidence"])


@pytest.mark.parametrize("index", [0, 2, 3], ids=[tr.IDS[i] for i in (0, 2, 3)])
def test_tta_images_follow_the_class_and_its_summed_probability(index):
    """More than two entries: the maps are the tables at the class predict_tta writes, and the confidence /
    pseudo maps follow acc[cls] / n of the restatement away from their thresholds."""
    case = tr.CASES[index]
    C, _, hw, _ = case
    ents = tr.entries(case)
    thr = 0.3  # unrelated entries: their averaged winning probability lies around it
    got = {k: v.cpu().numpy() for k, v in ops.predict_tta_images(_dev(ents), hw, want=MAPS, thr=thr).items()}
    arg = ops.predict_tta(_dev(ents), hw, want_argmax=True).cpu().numpy().astype(np.int64).reshape(hw)
    assert np.array_equal(got["class"], arg)
    assert np.array_equal(got["ids"], palette.id_table(C)[arg]) and np.array_equal(got["color"], palette.palette_table(C)[arg])
    prob = (tr.fuse(ents, hw).max(axis=0) / np.float32(len(ents))).reshape(hw)
    shade = palette.shade_table(C).reshape(4, C, 3)
    clear = np.ones(hw, dtype=bool)
    for t in (0.9, 0.8, 0.7, 0.5, thr):
        clear &= np.abs(prob - t) > 1e-5
    bucket = np.where(prob > 0.9, 0, np.where(prob > 0.8, 1, np.where(prob > 0.7, 2, np.where(prob > 0.5, 3, -1))))
    want_conf = np.where((bucket >= 0)[..., None], shade[np.maximum(bucket, 0), arg], 0)
    assert np.array_equal(got["confidence"][clear], want_conf[clear])
    assert np.array_equal(got["pseudo"][clear], np.where(prob > thr, arg, 255)[clear])
    assert clear.mean() > 0.99


@pytest.mark.parametrize("ho,wo", [(33, 65), (40, 70)])
def test_ties_take_the_lowest_class(ho, wo):
    """Planes 3 and 7 identical and dominant in every entry: equal inputs give equal probabilities and equal
    sums, and np.argmax's first maximum is class 3 at every pixel."""
    C = 19
    ents = []
    for k, (hi, wi) in enumerate(((9, 17), (5, 9), (12, 22))):
        for m in (0, 1):
            t = er.logits(C, hi, wi, tag=f"tie{k}{m}")
            t[0, 3] += 40.0
            t[0, 7] = t[0, 3]
            ents.append((t, m))
    arg = ops.predict_tta(_dev(ents), (ho, wo), want_argmax=True)
    assert (arg == 3).all().item()
    assert (tr.tta_ref(ents, (ho, wo))[0] == 3).all()


def test_entry_order_matters_only_on_near_ties():
    C, hw = 19, (64, 128)
    same = [(er.logits(C, 9, 17, tag=f"perm{k}"), m) for k, m in enumerate((0, 0, 0, 1, 1))]
    _, near, _ = tr.tta_ref(same, hw)
    base = ops.predict_tta(_dev(same), hw, want_argmax=True).cpu().numpy()
    for order in ((2, 0, 1, 4, 3), (1, 2, 0, 3, 4), (0, 1, 2, 4, 3)):  # entries of equal size and mirror swapped
        got = ops.predict_tta(_dev([same[i] for i in order]), hw, want_argmax=True).cpu().numpy()
        assert np.array_equal(got[~near], base[~near])
    assert near.mean() <= 1e-3 and len(np.unique(base)) > 5


def test_python_refusals():
    low = torch.zeros(1, 19, 3, 3, device="cuda")
    with pytest.raises(hip.MSLError):
        ops.predict_tta([], (7, 9), want_argmax=True)
    with pytest.raises(hip.MSLError):
        ops.predict_tta([(low, 0)] * 17, (7, 9), want_argmax=True)
    with pytest.raises(hip.MSLError):
        ops.predict_tta([(low, 2)], (7, 9), want_argmax=True)
    with pytest.raises(hip.MSLError):
        ops.predict_tta([(low, 0), (torch.zeros(1, 16, 3, 3, device="cuda"), 0)], (7, 9), want_argmax=True)
    with pytest.raises(hip.MSLError):
        ops.predict_tta([(low, 0)], (7, 9))  # nothing to compute
    with pytest.raises(hip.MSLError, match=r"status -3"):  # the register arrays hold 32 classes
        ops.predict_tta([(torch.zeros(1, 33, 3, 3, device="cuda"), 0)], (7, 9), want_argmax=True)
    with pytest.raises(hip.MSLError):
        Eval(16).add_batch_tta(torch.zeros(63, dtype=torch.int64), [(low, 0)], (7, 9))
    assert ops.predict_tta([(low, 0)] * 16, (7, 9), want_argmax=True).shape == (63,)


# ----------------------------------------------------------------------------- the input resize
@pytest.mark.parametrize("hi,wi,ho,wo", [(128, 256, 96, 192), (37, 53, 28, 40), (128, 256, 160, 320), (128, 256, 40, 88),
                                         (128, 256, 41, 88)])
def test_input_resize_is_torch_cpu_bit_for_bit(hi, wi, ho, wo):
    """Down and up, on both sides of ho + wo = 128, where torch-CPU changes from summing four taps to
    interpolating per axis (28 x 40 and 40 x 88: four taps)."""
    x = synthetic_image(hi, wi, 5)
    want = F.interpolate(x, size=(ho, wo), mode="bilinear", align_corners=True)
    got = ops.resize_bilinear(x.cuda(), (ho, wo)).cpu()
    assert torch.equal(got, want)
    if ho + wo > 128:  # there the loss kernels' upsample is the same arithmetic
        assert torch.equal(ops.upsample_bilinear(x.cuda(), (ho, wo)).cpu(), want)


# ----------------------------------------------------------------------------- model level
H, W = 128, 256
SCALES = (0.75, 1.0, 1.25)
LOW = {0.75: (13, 25), 1.0: (17, 33), 1.25: (21, 41)}


@pytest.fixture(scope="module")
def model():
    """An eval-mode model with filled running statistics and logits spread to std 2 over the classes, as
    tests/test_gpu_evaluate.py builds it."""
    from maxsquareloss_amd.tools import evaluate
    args, train_id, logger = evaluate.parse_args(["--crop_size", f"{W},{H}", "--target_crop_size", f"{W},{H}",
                                                  "--imagenet_pretrained", "False", "--save_dir", "",
                                                  "--val_images", "3"])
    m = evaluate.Evaluater(args, cuda=True, train_id=train_id, logger=logger).model
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
    with torch.no_grad():
        low = m.predict_low(synthetic_image(H, W, 71).cuda())[0]
        k = 2.0 / ops.upsample_bilinear(low, (H, W)).std().item()
        for conv in list(m.layer6.conv2d_list)[:2]:
            conv.weight.mul_(k)
            conv.bias.mul_(k)
    return m


def _normwise(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max()).item()


def test_scaled_forwards_match_the_oracle_and_the_fusion_its_restatement(model):
    x = synthetic_image(H, W, 71)
    ents = validate.tta_entries(model, x.cuda(), SCALES, True)
    assert [(tuple(L.shape[2:]), m) for L, m in ents] == [(LOW[s], m) for s in SCALES for m in (0, 1)]
    o = orc.Model({n: v.detach().cpu() for n, v in model.state_dict().items()})
    for k, s in enumerate(SCALES):
        hs, ws = validate.size_at(H, s), validate.size_at(W, s)
        xs = x if s == 1.0 else F.interpolate(x, size=(hs, ws), mode="bilinear", align_corners=True)
        for m in ((0, 1) if k == 0 else (0,)):  # the mirror at the smallest size only: an oracle forward takes a second
            with torch.no_grad():
                want = orc.forward_low(o.params, o.buffers, xs.flip(-1) if m else xs, training=False)[0]
            e = _normwise(ents[2 * k + m][0], want)
            print(f"scale {s} mirror {m}: low-res logits {tuple(want.shape[2:])} vs the oracle {e:.2e}")
            assert e < 1e-3, (s, m, e)
    host = [(L.cpu(), m) for L, m in ents]
    ref = tr.tta_ref(host, (H, W))
    arg = ops.predict_tta(ents, (H, W), want_argmax=True).cpu().numpy()
    print(f"model fusion: near-tie share {ref[1].mean():.2e}, classes {len(np.unique(arg))}")
    assert ref[1].mean() <= 1e-2 and len(np.unique(arg)) > 1
    assert tr.agrees(arg, ref)


def _hand_matrix(model, items, scales, flip, hw=None):
    cm = torch.zeros(19 * 19, dtype=torch.int64, device="cuda")
    maps = []
    with torch.no_grad():
        for x, y, _ in items:
            ents = validate.tta_entries(model, x.cuda(), scales, flip)
            maps.append(ops.predict_tta(ents, hw or x.shape[-2:], y.cuda().reshape(-1), cm, want_argmax=True).cpu())
    return cm.view(19, 19).cpu().numpy(), maps


def test_validator_equals_hand_composed_calls_eager_and_graphed(model):
    from maxsquareloss_amd.utils.images import OutputRequest
    dev = torch.device("cuda", 0)
    eager = validate.Validator(model, 19, (H, W), 3, dev, flip=True, scales=SCALES)
    graphed = validate.Validator(model, 19, (H, W), 3, dev, flip=True, graph=True, scales=SCALES)
    items = [eager.data[i] for i in range(3)]
    want, want_maps = _hand_matrix(model, items, SCALES, True)
    a = eager.run().confusion_matrix
    b = graphed.run().confusion_matrix
    assert a.sum() > 0 and np.array_equal(a, want) and np.array_equal(b, want)
    (key, gp), = graphed._graphed.items()
    assert key == (True, "scales", SCALES) and gp.replays == 2  # image 0 eager, then two replays of one graph
    single = validate.Validator(model, 19, (H, W), 3, dev, flip=True).run().confusion_matrix
    assert not np.array_equal(single, want)  # the scales change the prediction
    # the class maps: the body that writes images, eager and captured
    for graph in (False, True):
        ev = Eval(19)
        bufs = ops.image_buffers((H, W), ("class",), dev)
        body = validate.GraphedPredict(model, ev, (H, W), True, dev, ("class",), 0.95, SCALES) if graph else None
        for (x, y, _), want_map in zip(items, want_maps):
            with torch.no_grad():
                if graph:
                    body(x.cuda(), y.cuda())
                    got = body.images["class"]
                else:
                    validate.predict_image(model, ev, x.cuda(), y.cuda().reshape(-1), (H, W), True, bufs, 0.95, SCALES)
                    got = bufs["class"]
            assert torch.equal(got.cpu().reshape(-1).to(torch.int32), want_map)
        assert np.array_equal(ev.confusion_matrix, want)
    # a weight edit between replays is seen
    bias, weight = model.layer6.conv2d_list[0].bias, model.layer4[0].conv1.weight
    saved = (bias.detach().clone(), weight.detach().clone())
    try:
        with torch.no_grad():  # a bias the captured kernels read directly, and a weight they read as a pack
            bias[::2] += 1.5
            weight.mul_(1.25)
        b2 = graphed.run().confusion_matrix
        a2 = eager.run().confusion_matrix
        assert gp.replays == 5 and gp.eager_repacks == 1
        assert np.array_equal(a2, b2) and not np.array_equal(a2, a)
    finally:
        with torch.no_grad():
            bias.copy_(saved[0])
            weight.copy_(saved[1])
    assert np.array_equal(graphed.run().confusion_matrix, a)  # and back (another repack)


# ----------------------------------------------------------------------------- the tools
def _files(d):
    out = {}
    for kind in sorted(os.listdir(d)):
        for name in sorted(os.listdir(os.path.join(d, kind))):
            out[kind + "/" + name] = open(os.path.join(d, kind, name), "rb").read()
    return out


def test_evaluate_tool_reports_the_hand_composed_metrics(model, tmp_path):
    pytest.importorskip("PIL")
    from test_input_pipeline import write_tree
    from maxsquareloss_amd.tools import evaluate
    paths, _ = write_tree(tmp_path, n=1, val_n=2, hw=(96, 160))
    args, train_id, logger = evaluate.parse_args([
        "--imagenet_pretrained", "False", "--save_dir", "", "--resize", "True", "--base_size", f"{W},{H}",
        "--crop_size", f"{W},{H}", "--target_base_size", f"{W},{H}", "--target_crop_size", f"{W},{H}",
        "--data_root_path", paths["data_root_path"], "--scales", "0.75,1.0,1.25", "--flip", "True"])
    args.seg_size = (W, H)
    ev = evaluate.Evaluater(args, cuda=True, train_id=train_id, logger=logger)
    ev.model.load_state_dict(model.state_dict())
    assert ev.validator.scales == SCALES and ev.valid_iterations == 2
    PA, MPA, MIoU, FWIoU = ev.validate()
    got = ev.Eval.confusion_matrix.copy()
    items = [(x, y, i) for x, y, i in ev.dataloader.val_loader]
    assert len(items) == 2 and tuple(items[0][0].shape) == (1, 3, H, W)
    want, _ = _hand_matrix(ev.model.eval(), items, SCALES, True)
    ev.dataloader.close()
    assert got.sum() > 0 and np.array_equal(got, want)
    r = orc.eval_metrics(want)
    assert (PA, MPA, MIoU, FWIoU) == pytest.approx((r["PA"], r["MPA"], r["MIoU"], r["FWIoU"]), rel=1e-12)


def _predict_run(model, tmp_path, tag, lists, extra):
    from maxsquareloss_amd.tools import predict
    out = tmp_path / tag
    args, train_id, logger = predict.parse_args([
        "--list_path", str(lists), "--imagenet_pretrained", "False", "--save_dir", "", "--resize", "True",
        "--save_predictions", str(out), "--save_kinds", "labelids,color", "--data_loader_workers", "2", *extra])
    args.seg_size = (W, H)
    p = predict.Predictor(args, cuda=True, train_id=train_id, logger=logger)
    p.model.load_state_dict(model.state_dict())
    p.main()
    return p, out


def test_predict_tool_writes_the_fused_files(model, tmp_path):
    pytest.importorskip("PIL.Image")
    from PIL import Image
    from maxsquareloss_amd.utils.preprocess import resize_image
    lists = tmp_path / "lists"
    lists.mkdir()
    rng = np.random.default_rng(3)
    paths = []
    for k in range(2):
        paths.append(str(tmp_path / f"frame_{k}.png"))
        Image.fromarray(rng.integers(0, 256, size=(40, 70, 3), dtype=np.uint8)).save(paths[-1])
    (lists / "test.txt").write_text("\n".join(paths) + "\n")
    OW, OH = 96, 52
    p, out = _predict_run(model, tmp_path, "fused", lists, ["--scales", "0.5,1.0", "--out_size", f"{OW},{OH}"])
    assert p.validator.scales == (0.5, 1.0)
    assert sorted(os.listdir(out)) == ["color", "labelids"]
    for k in range(2):
        rgb = torch.from_numpy(np.asarray(Image.open(paths[k]).convert("RGB")).copy()).cuda()
        with torch.no_grad():
            ents = validate.tta_entries(p.model.eval(), resize_image(rgb, (W, H)), (0.5, 1.0), False)
        assert [tuple(L.shape[2:]) for L, _ in ents] == [(9, 17), (17, 33)]
        want = ops.predict_tta_images(ents, (OH, OW), want=("ids", "color"))
        for kind, name in (("labelids", "ids"), ("color", "color")):
            got = np.asarray(Image.open(out / kind / f"frame_{k}.png"))
            assert np.array_equal(got, want[name].cpu().numpy()), (kind, k)
    # --scales 1.0 is today's path: the same bytes as a run without the flag
    _, plain = _predict_run(model, tmp_path, "plain", lists, ["--flip", "True"])
    _, one = _predict_run(model, tmp_path, "one", lists, ["--flip", "True", "--scales", "1.0"])
    assert _files(plain) == _files(one) and len(_files(plain)) == 4
