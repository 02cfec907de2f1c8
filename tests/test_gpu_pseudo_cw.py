"""Class-balanced pseudo-label thresholds on the GPU: msl_confidence_hist, msl_class_thresholds and
msl_pseudo_classwise against the torch-CPU / numpy restatement (tests/pseudo_cw_ref.py) and against the kernels
whose decision they share (msl_pseudo_labels_up, msl_predict_images, msl_predict_tta_images); the loss
(utils/loss.py PseudoLabelCEClasswise) against pseudo_label_ce and fp64 torch-CPU; the UDA trainer with
--threshold_mode class over two rounds, eager and as a captured graph.

Inputs: tests/predict_images_ref.py's (std 6 logits; for flip the mirror plus std 1 noise) at its five shapes.
A pixel whose reference probability lies within 1e-5 of a bin edge (or of its class's threshold) may fall on
either side: per class and edge, the count at or above the edge may differ from the restatement's by the number
of that class's pixels near that edge; such pixels are at most 2 % of an image (three pixels for the 63-pixel
one, pseudo_cw_ref.near_cap).  Near-tie pixels of the flip rule may be counted in either of their two leading
classes.

The loss with a uniform threshold vector is bit-equal to pseudo_label_ce (loss and gradient): both are the CE sum
over the same labels.  The trainer runs at a 128 x 256 crop (17 x 33 logits), the smallest size the suite holds
the whole model to.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import predict_images_ref as pir  # noqa: E402
import pseudo_cw_ref as ref  # noqa: E402
import target_modes_ref as tm  # noqa: E402
from maxsquareloss_amd import hip, ops  # noqa: E402
from maxsquareloss_amd.utils import loss as L  # noqa: E402

DEV = "cuda"
PORTION, THR_MAX = 0.5, 0.9
HIST_CASES = [(s, f, b) for s in ref.SHAPES for f in (False, True) for b in ref.BINS]
HIST_CASES += [(ref.LIMIT_SHAPE, f, ref.LIMIT_BINS) for f in (False, True)]  # the 64 KB tile, 32 classes


def _lows(shape, flip, nan=False):
    C, hi, wi, ho, wo = shape
    low, lowf = pir.inputs(C, hi, wi, flip, nan)
    return low.to(DEV), None if lowf is None else lowf.to(DEV)


def _hist(shape, flip, bins, nan=False, into=None, tta=False):
    C, hi, wi, ho, wo = shape
    low, lowf = _lows(shape, flip, nan)
    hist = ops.confidence_buffers(C, bins, DEV)[0] if into is None else into
    if tta:
        ops.confidence_hist(hist, (ho, wo), entries=[(low, 0), (lowf, 1)])
    else:
        ops.confidence_hist(hist, (ho, wo), low, lowf)
    torch.cuda.synchronize()
    return hist


# ----------------------------------------------------------------------------- the histogram
@pytest.mark.parametrize("shape,flip,bins", HIST_CASES)
def test_confidence_hist(shape, flip, bins):
    C, hi, wi, ho, wo = shape
    npx = ho * wo
    r = ref.hist_ref(shape, flip, bins)
    hist = _hist(shape, flip, bins)
    got = hist.cpu().numpy()
    assert got.shape == (C, bins) and (got >= 0).all()
    assert got.sum() == r["valid"] == npx
    assert r["near"] <= ref.near_cap(npx)  # the allowance below cannot hide a wrong bin rule
    diff = ref.suffix(got) - ref.suffix(r["hist_off_tie"])  # [C, bins + 1], per class and edge
    edge, tie = r["edge_count"], r["tie_count"][:, None]
    print(f"{shape} flip={flip} bins={bins}: near-edge {r['near']} of {npx} (most on one edge "
          f"{int(edge.sum(axis=0).max())}), near-tie pixels {int(r['tie_count'].sum()) // 2}, cells off "
          f"{int((got != r['hist']).sum())}, largest cumulative difference {int(np.abs(diff).max())}")
    assert (diff >= -edge).all() and (diff <= edge + tie).all()
    assert np.array_equal(got.sum(axis=1) == 0, r["hist"].sum(axis=1) == 0) or tie.any()
    # it accumulates: a second call into the same buffer doubles every cell; a second run gives the same bytes
    _hist(shape, flip, bins, into=hist)
    assert np.array_equal(hist.cpu().numpy(), 2 * got)
    assert np.array_equal(_hist(shape, flip, bins).cpu().numpy(), got)
    if flip:  # a two-entry table is the flip rule bit for bit
        assert np.array_equal(_hist(shape, flip, bins, tta=True).cpu().numpy(), got)


@pytest.mark.parametrize("flip", [False, True])
def test_confidence_hist_skips_nan_pixels(flip):
    shape = ref.SHAPES[0]
    r = ref.hist_ref(shape, flip, 64, True)
    npx = shape[3] * shape[4]
    assert 0 < r["valid"] < npx
    got = _hist(shape, flip, 64, nan=True).cpu().numpy()
    assert got.sum() == r["valid"]
    if flip:
        assert np.array_equal(_hist(shape, flip, 64, nan=True, tta=True).cpu().numpy(), got)


# ----------------------------------------------------------------------------- the thresholds
def _thresholds(hist_np, portion, thr_max):
    hist = torch.from_numpy(np.ascontiguousarray(hist_np, np.int64)).to(DEV)
    thr, kept = ops.class_thresholds(hist, portion, thr_max)
    torch.cuda.synchronize()
    return thr.cpu().numpy(), kept.cpu().numpy()


@pytest.mark.parametrize("case", ref.hand_cases(), ids=lambda c: c[0])
def test_class_thresholds_on_hand_built_histograms(case):
    name, hist, portion, thr_max, want = case
    thr, kept = _thresholds(hist, portion, thr_max)
    rthr, rkept, _ = ref.thresholds_ref(hist, portion, thr_max)
    assert thr.dtype == np.float32 and np.array_equal(thr, rthr), (name, thr, rthr)
    assert np.array_equal(kept, rkept), (name, kept, rkept)
    if want is not None:
        assert np.array_equal(thr, np.asarray(want, np.float32))


@pytest.mark.parametrize("shape,flip,bins", [(s, f, b) for s in ref.SHAPES[:4] for f in (False, True)
                                             for b in ref.BINS] + [(ref.SHAPES[4], True, 512)])
def test_class_thresholds_on_the_kernels_own_histogram(shape, flip, bins):
    got = _hist(shape, flip, bins).cpu().numpy()
    for portion, thr_max in ((PORTION, THR_MAX), (0.2, 1.0), (1.0, 0.95), (0.0, 0.5)):
        thr, kept = _thresholds(got, portion, thr_max)
        rthr, rkept, _ = ref.thresholds_ref(got, portion, thr_max)
        assert np.array_equal(thr, rthr) and np.array_equal(kept, rkept), (portion, thr_max)
        n = got.sum(axis=1)
        assert (kept >= np.ceil(portion * n)).all() and (thr <= np.float32(thr_max)).all()
    assert (got.sum(axis=1) == 0).any() or shape not in ref.SHAPES[:2] or flip


# ----------------------------------------------------------------------------- the labels
def _classwise(shape, flip, thr, tta=False, unaligned=False):
    """(label int64 numpy, pseudo uint8 numpy) of one msl_pseudo_classwise call; `unaligned`: the byte map starts
    one byte, the label map one element into its allocation, with guard values around both."""
    C, hi, wi, ho, wo = shape
    npx = ho * wo
    low, lowf = _lows(shape, flip)
    t = torch.as_tensor(np.asarray(thr, np.float32)).to(DEV)
    raw_l = torch.full((npx + 2,), -7, dtype=torch.int64, device=DEV)
    raw_p = torch.full((npx + 8,), 77, dtype=torch.uint8, device=DEV)
    off = 1 if unaligned else 0
    lab, ps = raw_l[1:1 + npx], raw_p[4 * (1 - off) + off:4 * (1 - off) + off + npx]
    assert ps.data_ptr() % 4 == off
    if tta:
        ops.pseudo_classwise(t, (ho, wo), entries=[(low, 0), (lowf, 1)], label=lab, pseudo=ps)
    else:
        ops.pseudo_classwise(t, (ho, wo), low, lowf, label=lab, pseudo=ps)
    torch.cuda.synchronize()
    start = 4 * (1 - off) + off
    rl, rp = raw_l.cpu().numpy(), raw_p.cpu().numpy()
    assert rl[0] == -7 and rl[-1] == -7 and (rp[:start] == 77).all() and (rp[start + npx:] == 77).all()
    return rl[1:1 + npx].copy(), rp[start:start + npx].copy()


@pytest.mark.parametrize("shape", ref.SHAPES)
@pytest.mark.parametrize("flip", [False, True])
def test_uniform_thresholds_are_the_scalar_rule(shape, flip):
    C, hi, wi, ho, wo = shape
    low, lowf = _lows(shape, flip)
    for thr in (pir.THR, 0.5):
        if flip:
            want = ops.predict_images(low, (ho, wo), lowf, want=("pseudo",), thr=thr)["pseudo"].cpu().numpy().reshape(-1)
            also = ops.predict_tta_images([(low, 0), (lowf, 1)], (ho, wo), want=("pseudo",), thr=thr)["pseudo"]
            assert np.array_equal(also.cpu().numpy().reshape(-1), want)
        else:
            lab32 = ops.pseudo_labels_up(low, (ho, wo), thr).cpu().numpy()
            want = np.where(lab32 < 0, 255, lab32).astype(np.uint8)
            img = ops.predict_images(low, (ho, wo), want=("pseudo",), thr=thr)["pseudo"].cpu().numpy().reshape(-1)
            assert np.array_equal(img, want)
        for unaligned in (False, True):
            lab, ps = _classwise(shape, flip, np.full(C, thr, np.float32), unaligned=unaligned)
            assert np.array_equal(ps, want), (thr, unaligned)
            assert np.array_equal(lab, np.where(want == 255, -1, want.astype(np.int64))), (thr, unaligned)
        if flip:
            lab, ps = _classwise(shape, flip, np.full(C, thr, np.float32), tta=True)
            assert np.array_equal(ps, want)
        assert 0 < (want != 255).sum() < want.size


@pytest.mark.parametrize("shape", ref.SHAPES)
@pytest.mark.parametrize("flip", [False, True])
def test_labels_under_the_cases_own_thresholds(shape, flip):
    C, hi, wi, ho, wo = shape
    r = pir.reference(shape, flip)
    thr = ref.thresholds_ref(ref.hist_ref(shape, flip, 512)["hist"], PORTION, THR_MAX)[0]
    assert len(np.unique(thr)) > 2  # the classes really have different thresholds
    want = ref.labels_ref(r["cls"], r["top"], thr)
    skip = ref.near_threshold(r["cls"], r["top"], thr) | r["near_tie"]
    for unaligned in (False, True):
        lab, ps = _classwise(shape, flip, thr, unaligned=unaligned)
        print(f"{shape} flip={flip}: kept {int((want >= 0).sum())} of {want.size}, near a threshold or a tie "
              f"{int(skip.sum())}, differing {int((lab != want).sum())}")
        assert skip.sum() <= ref.near_cap(want.size)
        assert np.array_equal(lab[~skip], want[~skip])
        assert np.array_equal(ps, np.where(lab < 0, 255, lab).astype(np.uint8))  # the two outputs agree everywhere
        assert ((lab[skip] == -1) | (lab[skip] == r["cls"][skip]) | r["near_tie"][skip]).all()
    # each output alone gives the same values
    low, lowf = _lows(shape, flip)
    t = torch.from_numpy(thr).to(DEV)
    only_l, none = ops.pseudo_classwise(t, (ho, wo), low, lowf, want=("label",))
    none2, only_p = ops.pseudo_classwise(t, (ho, wo), low, lowf, want=("pseudo",))
    assert none is None and none2 is None and only_p.shape == (ho, wo)
    assert np.array_equal(only_l.cpu().numpy(), lab) and np.array_equal(only_p.cpu().numpy().reshape(-1), ps)


def test_nan_pixels_get_no_label():
    shape = ref.SHAPES[0]
    C, hi, wi, ho, wo = shape
    low, _ = pir.inputs(C, hi, wi, False, True)
    r = pir.reference(shape, False, True)
    lab, ps = ops.pseudo_classwise(torch.zeros(C, device=DEV), (ho, wo), low.to(DEV), want=("label", "pseudo"))
    nanpx = np.isnan(r["top"])
    assert nanpx.any() and (lab.cpu().numpy()[nanpx] == -1).all() and (ps.cpu().numpy().reshape(-1)[nanpx] == 255).all()
    assert (lab.cpu().numpy()[~nanpx] == r["cls"][~nanpx]).all()  # threshold 0: every other pixel keeps its class


# ----------------------------------------------------------------------------- the loss
def _run(fn, low):
    lg = low.clone().requires_grad_()
    out = fn(ops.upsample_bilinear(lg, HW[tuple(low.shape)]))
    out.backward()
    torch.cuda.synchronize()
    return out.detach(), lg.grad


HW = {}
LOSS_SHAPES = [ref.SHAPES[3], ref.SHAPES[1], ref.SHAPES[2]]


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


@pytest.mark.parametrize("shape", LOSS_SHAPES)
def test_loss_with_a_uniform_vector_is_pseudo_label_ce(shape):
    C, hi, wi, ho, wo = shape
    low = _lows(shape, False)[0]
    HW[tuple(low.shape)] = (ho, wo)
    for thr in (pir.THR, 0.5):
        vec = torch.full((C,), thr, dtype=torch.float32, device=DEV)
        a, da = _run(lambda p: L.pseudo_label_ce_classwise(p, vec), low)
        b, db = _run(lambda p: L.pseudo_label_ce(p, thr), low)
        print(f"{shape} thr={thr}: loss {a.item()!r} vs {b.item()!r}, gradient difference {_rel(da, db):.3e}")
        assert np.isfinite(b.item()) and db.abs().max().item() > 0
        assert a.item() == b.item() and torch.equal(da, db)


@pytest.mark.parametrize("shape", LOSS_SHAPES)
def test_loss_with_class_thresholds_against_fp64(shape):
    C, hi, wi, ho, wo = shape
    low_cpu = pir.inputs(C, hi, wi, False)[0]
    low = low_cpu.to(DEV)
    HW[tuple(low.shape)] = (ho, wo)
    r = pir.reference(shape, False)
    thr = ref.thresholds_ref(ref.hist_ref(shape, False, 512)["hist"], PORTION, THR_MAX)[0]
    skip = ref.near_threshold(r["cls"], r["top"], thr)
    want = ref.labels_ref(r["cls"], r["top"], thr)
    want[skip] = -1
    # the reference: fp64 CE of the upsampled logits with the restatement's labels
    l64 = low_cpu.double().requires_grad_()
    loss64 = F.cross_entropy(tm.up(l64, (ho, wo)), torch.from_numpy(want).view(1, ho, wo), ignore_index=-1)
    (d64,) = torch.autograd.grad(loss64, l64)
    # the device: the kernel's label map with the same pixels removed, through the same fused CE
    t = torch.from_numpy(thr).to(DEV)
    lab, _ = ops.pseudo_classwise(t, (ho, wo), low)
    lab[torch.from_numpy(skip).to(DEV)] = -1
    assert np.array_equal(lab.cpu().numpy(), want)
    got, dgot = _run(lambda p: ops.ce_up(ops.low_of(p), lab, (ho, wo)), low)
    print(f"{shape}: kept {int((want >= 0).sum())} of {want.size}, near a threshold {int(skip.sum())}, loss "
          f"{got.item():.7f} vs {loss64.item():.7f}, gradient {_rel(dgot, d64):.3e}")
    assert (want >= 0).sum() > 0
    assert got.item() == pytest.approx(loss64.item(), rel=1e-5)
    assert _rel(dgot, d64) < 1e-5
    # the loss object: the same numbers when no pixel had to be removed, within the removed pixels' share else
    obj = L.PseudoLabelCEClasswise()
    a, da = _run(lambda p: obj(p, t), low)
    assert obj.labels.dtype == torch.int64 and obj.labels.numel() == ho * wo
    if not skip.any():
        assert a.item() == got.item() and torch.equal(da, dgot)
    else:
        assert np.array_equal(obj.labels.cpu().numpy()[~skip], want[~skip])
    b, db = _run(lambda p: obj(p, t), low)  # the buffer is reused; the result is reproducible
    assert a.item() == b.item() and torch.equal(da, db)


# ----------------------------------------------------------------------------- argument errors
def test_entry_points_reject_bad_arguments():
    lib = hip.load()
    low = torch.zeros(1, 19, 3, 3, device=DEV)
    hist = torch.zeros(19 * 64, dtype=torch.int64, device=DEV)
    big = torch.zeros(32 * 1024, dtype=torch.int64, device=DEV)
    thr = torch.full((32,), 0.5, device=DEV)
    kept = torch.zeros(32, dtype=torch.int64, device=DEV)
    lab = torch.full((63,), -9, dtype=torch.int64, device=DEV)
    ps = torch.full((64,), 9, dtype=torch.uint8, device=DEV)
    s, Lp, H = hip.stream_ptr(), low.data_ptr(), hist.data_ptr()
    ERR = -3

    def h(logits=Lp, c=19, hi=3, wi=3, ho=7, wo=9, bins=64, out=H):
        return lib.msl_confidence_hist(logits, None, c, hi, wi, ho, wo, bins, out, s)

    assert h(logits=None) == ERR and h(out=None) == ERR
    assert h(c=0) == ERR and h(c=33) == ERR
    for bins in (0, 8, 48, 100, 2048):
        assert h(bins=bins) == ERR, bins
    assert h(c=19, bins=1024, out=big.data_ptr()) == ERR      # 19 * 1024 cells > 16384
    assert h(ho=0) == ERR and h(wi=0) == ERR and h(ho=1 << 16, wo=1 << 15) == ERR
    ent = (hip.TtaEntry * 2)(hip.TtaEntry(Lp, 3, 3, 0), hip.TtaEntry(Lp, 3, 3, 1))

    def ht(entries=ent, n=2, c=19, bins=64, out=H):
        return lib.msl_confidence_hist_tta(entries, n, c, 7, 9, bins, out, s)

    assert ht(entries=None) == ERR and ht(n=0) == ERR and ht(n=17) == ERR and ht(bins=48) == ERR and ht(out=None) == ERR
    assert ht(entries=(hip.TtaEntry * 1)(hip.TtaEntry(Lp, 3, 3, 2)), n=1) == ERR   # mirror outside {0, 1}
    assert ht(entries=(hip.TtaEntry * 1)(hip.TtaEntry(None, 3, 3, 0)), n=1) == ERR

    def t(hist=H, c=19, bins=64, portion=0.5, thr_max=0.9, out=thr.data_ptr(), k=kept.data_ptr()):
        return lib.msl_class_thresholds(hist, c, bins, portion, thr_max, out, k, s)

    assert t(hist=None) == ERR and t(out=None) == ERR and t(c=0) == ERR and t(c=33) == ERR and t(bins=48) == ERR
    assert t(c=32, bins=1024, hist=big.data_ptr()) == ERR
    for portion in (-0.1, 1.5, float("nan")):
        assert t(portion=portion) == ERR
    for thr_max in (0.0, -0.5, 1.5, float("nan")):
        assert t(thr_max=thr_max) == ERR

    def p(logits=Lp, c=19, ho=7, th=thr.data_ptr(), label=lab.data_ptr(), pseudo=ps.data_ptr()):
        return lib.msl_pseudo_classwise(logits, None, c, 3, 3, ho, 9, th, label, pseudo, s)

    assert p(logits=None) == ERR and p(th=None) == ERR and p(label=None, pseudo=None) == ERR
    assert p(c=33) == ERR and p(ho=0) == ERR
    assert lib.msl_pseudo_classwise_tta(None, 2, 19, 7, 9, thr.data_ptr(), lab.data_ptr(), None, s) == ERR
    assert lib.msl_pseudo_classwise_tta(ent, 2, 19, 7, 9, None, lab.data_ptr(), None, s) == ERR
    assert lib.msl_pseudo_classwise_tta(ent, 2, 19, 7, 9, thr.data_ptr(), None, None, s) == ERR
    torch.cuda.synchronize()
    # nothing was launched: every buffer is as it was
    assert hist.sum().item() == 0 and kept.sum().item() == 0 and (thr == 0.5).all()
    assert (lab == -9).all() and (ps == 9).all()
    # the same calls with good arguments do run
    assert h() == 0 and ht() == 0 and t() == 0 and p() == 0 and p(label=None) == 0 and p(pseudo=None) == 0
    torch.cuda.synchronize()
    assert hist.sum().item() == 2 * 63 and (lab >= -1).all()
    with pytest.raises(hip.MSLError):
        ops.confidence_hist(torch.zeros(16, 64, dtype=torch.int64, device=DEV), (7, 9), low)   # 16 rows, 19 classes
    with pytest.raises(hip.MSLError):
        ops.pseudo_classwise(thr[:16].contiguous(), (7, 9), low)
    with pytest.raises(hip.MSLError):
        ops.pseudo_classwise(thr[:19].contiguous(), (7, 9), low, want=())


# ----------------------------------------------------------------------------- the tools
H, W = 128, 256


def _spread_logits(m):
    """An eval-mode model with filled running statistics and logits spread to std 2 over the classes (random-init
    logits have tiny margins), as tests/test_gpu_predict_images.py builds its model."""
    from maxsquareloss_amd.utils.synthetic import synthetic_image
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


def test_threshold_tool_and_the_class_thresholds_flag(tmp_path):
    """tools/pseudo_thresholds.py eager and as a captured graph (--flip), its files, and a Validator that takes
    them as --class_thresholds: the pseudo map is msl_pseudo_classwise's, the other kinds are unchanged."""
    import json
    import os
    pytest.importorskip("PIL.Image")
    from PIL import Image
    from maxsquareloss_amd.tools import pseudo_thresholds as tool
    from maxsquareloss_amd.utils.images import OutputRequest
    from maxsquareloss_amd.utils.synthetic import SyntheticDomain
    from maxsquareloss_amd.utils.thresholds import ThresholdPass, load_class_thresholds
    from maxsquareloss_amd.utils.validate import VAL_OFFSET, Validator
    hists, model = {}, None
    for graph in (False, True):
        out = tmp_path / f"thr{int(graph)}"
        args, train_id, logger = tool.parse_args([
            "--crop_size", f"{W},{H}", "--target_crop_size", f"{W},{H}", "--imagenet_pretrained", "False",
            "--save_dir", str(out), "--val_images", "3", "--threshold_bins", "64", "--threshold", "0.9",
            "--pseudo_portion", "0.5", "--flip", "True", "--graph", str(graph)])
        t = tool.ThresholdTool(args, cuda=True, train_id=train_id, logger=logger)
        if model is None:
            model = _spread_logits(t.model)
        else:
            t.model.load_state_dict(model.state_dict())
            t.model.eval()
        path = t.main()
        assert path == str(out / "class_thresholds.json") and not t.model.training  # the mode it was found in
        hists[graph] = np.load(out / "confidence_hist.npy")
        if graph:
            assert [g.replays for g in t.passes._graphed.values()] == [2]
    assert np.array_equal(hists[False], hists[True]) and hists[False].sum() == 3 * H * W
    doc = json.load(open(tmp_path / "thr0" / "class_thresholds.json"))
    assert (doc["bins"], doc["portion"], doc["thr_max"], doc["images"], len(doc["classes"])) == (64, 0.5, 0.9, 3, 19)
    assert sorted(doc["classes"][0]) == ["kept_share", "name", "pixels", "quantile", "share", "threshold"]
    assert doc["classes"][0]["name"] == "road" and [r["pixels"] for r in doc["classes"]] == hists[False].sum(axis=1).tolist()
    thr = load_class_thresholds(str(tmp_path / "thr0" / "class_thresholds.json"), 19)
    rthr, rkept, rq = ref.thresholds_ref(hists[False], 0.5, 0.9)
    assert np.array_equal(np.asarray(thr, np.float32), rthr)
    assert [r["quantile"] for r in doc["classes"]] == [float(q) for q in rq]
    # the histogram is that of the items' flip predictions, and of a two-entry table through --scales' path
    dom = SyntheticDomain(H, W, 19, 3, offset=VAL_OFFSET)
    direct = ops.confidence_buffers(19, 64, DEV)[0]
    with torch.no_grad():
        for i in range(3):
            (low, _), (low_f, _) = model.predict_low(dom[i][0].to(DEV), flip=True)
            ops.confidence_hist(direct, (H, W), low, low_f)
        lows = [model.predict_low(dom[i][0].to(DEV), flip=True) for i in range(3)]
    assert np.array_equal(direct.cpu().numpy(), hists[False])
    tp = ThresholdPass(model, 19, 64, torch.device(DEV), thr_max=0.9, flip=True, scales=(1.0, 0.75))
    tp.run(dom[i] for i in range(2))
    assert tp.hist.sum().item() == 2 * H * W and tp.images == 2
    # --class_thresholds: eager and graphed files are the same bytes; pseudo follows the per-class rule
    files = {}
    for graph in (False, True):
        d = tmp_path / f"pred{int(graph)}"
        req = OutputRequest(str(d), ("pseudo", "trainids"), threshold=0.9, class_thresholds=thr)
        Validator(model, 19, (H, W), 3, torch.device(DEV, 0), flip=True, graph=graph, outputs=req).run()
        files[graph] = {k: [open(d / k / n, "rb").read() for n in sorted(os.listdir(d / k))] for k in ("pseudo", "trainids")}
    assert files[False] == files[True] and len(files[False]["pseudo"]) == 3
    plain = tmp_path / "plain"
    Validator(model, 19, (H, W), 3, torch.device(DEV, 0), flip=True,
              outputs=OutputRequest(str(plain), ("pseudo", "trainids"), threshold=0.9)).run()
    t_dev = torch.tensor(thr, dtype=torch.float32, device=DEV)
    kept = kept_plain = 0
    for i in range(3):
        (low, _), (low_f, _) = lows[i]
        want = ops.pseudo_classwise(t_dev, (H, W), low, low_f, want=("pseudo",))[1].cpu().numpy()
        got = np.asarray(Image.open(tmp_path / "pred0" / "pseudo" / f"{i:06d}.png"))
        assert np.array_equal(got, want)
        kept += int((got != 255).sum())
        assert np.array_equal(np.asarray(Image.open(tmp_path / "pred0" / "trainids" / f"{i:06d}.png")),
                              np.asarray(Image.open(plain / "trainids" / f"{i:06d}.png")))
        kept_plain += int((np.asarray(Image.open(plain / "pseudo" / f"{i:06d}.png")) != 255).sum())
    assert kept_plain < kept < 3 * H * W  # the scalar 0.9 keeps fewer pixels than the per-class medians below it


# ----------------------------------------------------------------------------- the trainer


def _trainer(graph, extra):
    from maxsquareloss_amd.tools.solve_gta5 import UDATrainer, build_parser
    from maxsquareloss_amd.tools.train_source import init_args
    argv = ["--crop_size", f"{W},{H}", "--target_crop_size", f"{W},{H}", "--imagenet_pretrained", "False",
            "--save_dir", "", "--target_mode", "hard", "--synthetic_images", "2", "--round_num", "2",
            "--epoch_each_round", "1", "--multi", "False", "--graph", str(graph)] + extra
    args, _, _ = init_args(build_parser().parse_args(argv))
    return UDATrainer(args, cuda=True)


def _state(tr):
    return ([p.detach().clone() for p in tr.model.parameters()] + [b.detach().clone() for b in tr.model.buffers()] +
            [tr.optimizer.state[p]["momentum_buffer"].detach().clone() for p in tr.optimizer._uniq
             if p in tr.optimizer.state])


def test_trainer_two_rounds_eager_and_graphed():
    """Two rounds of one epoch of two iterations each, the thresholds regenerated from two target items at the top
    of each: the eager and the --graph trainer agree bit for bit after each round, the thresholds of round 1
    differ from round 0's, and the captured step - one GraphedStep for the whole run - follows them."""
    runs = {}
    for graph in (False, True):
        tr = _trainer(graph, ["--threshold_mode", "class", "--threshold_images", "2", "--threshold_bins", "512",
                              "--threshold", "0.9"])
        assert tr.class_thresholds.dtype == torch.float32 and tr.class_thresholds.shape == (19,)
        thr_tensor, snaps, steps = tr.class_thresholds, [], []
        inner = tr.train

        def train(tr=tr, inner=inner, snaps=snaps, steps=steps):
            assert tr.model.training  # the pass put the training mode back
            # main() keeps the reference's epoch arithmetic (solve_gta5.py:277), under which a second round runs
            # past iter_max and the poly rate runs out: one epoch per round here, iter_max = 4 iterations
            tr.epoch_num = tr.current_epoch + 1
            inner()
            torch.cuda.synchronize()
            snaps.append((_state(tr), tr.class_thresholds.clone(), tr.threshold_pass.hist.clone(),
                          float(tr.loss_target_value)))
            steps.append(tr._graphed)

        tr.train = train
        tr.main()
        assert tr.class_thresholds is thr_tensor and len(snaps) == 2 and tr.current_iter == 4
        if graph:
            assert steps[0] is not None and steps[0] is steps[1] and steps[0].replays == 3  # no second capture
        runs[graph] = snaps
    for rnd, (e, g) in enumerate(zip(runs[False], runs[True])):
        assert torch.equal(e[1], g[1]) and torch.equal(e[2], g[2]), rnd      # thresholds and histogram
        assert all(torch.equal(a, b) for a, b in zip(e[0], g[0])), rnd      # weights, buffers, momentum
        assert e[3] == g[3] and np.isfinite(e[3]) and e[3] > 0, (rnd, e[3], g[3])
        assert e[2].sum().item() == 2 * H * W                               # two images were counted
    assert not torch.equal(runs[False][0][1], runs[False][1][1])            # round 1 has thresholds of its own
    assert (runs[False][0][1] <= 0.9).all()


def test_crosscity_trainer_regenerates_the_thresholds_every_epoch():
    """tools/solve_crosscity.py has no rounds: its main() must still run the pass, before every epoch."""
    from maxsquareloss_amd.tools.solve_crosscity import CrossCityTrainer, build_parser
    from maxsquareloss_amd.tools.train_source import init_args
    argv = ["--crop_size", f"{W},{H}", "--target_crop_size", f"{W},{H}", "--imagenet_pretrained", "False",
            "--save_dir", "", "--target_mode", "hard", "--threshold_mode", "class", "--threshold_images", "2",
            "--synthetic_images", "2", "--epoch_num", "2", "--multi", "False"]
    args, _, _ = init_args(build_parser().parse_args(argv))
    tr = CrossCityTrainer(args, cuda=True)
    assert args.num_classes == 13 and (tr.class_thresholds == 0.98).all()  # the cap, until a pass has run
    seen, inner = [], tr.generate_thresholds

    def generate(when=None):
        rows = inner(when)
        torch.cuda.synchronize()
        seen.append((tr.class_thresholds.clone(), rows, when))
        return rows

    tr.generate_thresholds = generate
    tr.main()
    assert len(seen) == 2 and tr.current_iter == 4
    assert [when for _, _, when in seen] == ["epoch 0", "epoch 1"]  # the table's title: this tool has no rounds
    for thr, rows, _ in seen:
        assert len(rows) == 13 and sum(r["pixels"] for r in rows) == 2 * H * W
        assert (thr < 0.98).any() and (thr <= 0.98).all()  # a pass ran: not the cap everywhere
    assert not torch.equal(seen[0][0], seen[1][0]) and np.isfinite(float(tr.loss_target_value))


def test_every_rank_counts_the_same_synthetic_items():
    from maxsquareloss_amd.utils.synthetic import SyntheticDomain
    tr = _trainer(False, ["--threshold_mode", "class", "--threshold_images", "2"])
    tr.target_dataloader = SyntheticDomain(H, W, 19, 2, rank=1, offset=500)  # as rank 1 of a data-parallel run
    items = list(tr.threshold_items())
    rank0 = SyntheticDomain(H, W, 19, 2, rank=0, offset=500)
    assert len(items) == 2 and all(torch.equal(items[i][0], rank0[i][0]) for i in range(2))
    assert not torch.equal(items[0][0], tr.target_dataloader[0][0])  # the rank's own training items differ


def test_trainer_fixed_mode_is_the_scalar_hard_step():
    tr = _trainer(False, ["--threshold_mode", "fixed", "--threshold", "0.5"])
    assert tr.threshold_pass is None and tr.class_thresholds is None and tr.generate_thresholds() is None
    shape = ref.SHAPES[3]
    low = _lows(shape, False)[0]
    HW[tuple(low.shape)] = shape[3:]
    a, da = _run(tr.target_loss, low)
    b, db = _run(lambda p: L.pseudo_label_ce(p, 0.5), low)
    assert np.isfinite(a.item()) and a.item() == b.item() and torch.equal(da, db)
