"""The per-image analysis on the GPU: msl_image_metrics and msl_analysis_maps against the numpy restatement
(tests/analysis_ref.py), and the Analyzer end to end, eager and as a captured graph.

Metrics: per-class IoU, PA and the pixel count are bit-equal to numpy, the NaN pattern is identical, the
nan-means and FWIoU are within 1e-12 absolute (two summation orders of <= 32 fp64 terms in [0, 1] differ by at
most 2 * 31 * 32 * 2^-53 ~ 2.2e-13).  Maps: byte-exact.

End to end at 128 x 256 (the smallest size tests/test_gpu_evaluate.py forwards), 5 synthetic items, ring 2.
The threshold splits the plain loop's per-image MIoUs at their median: the midpoint of the second and third
lowest, so that two of the five images lie below it and every MIoU is >= 1e-9 away (the median itself IS one of
five values, so a distance to each of them could not be asserted of it).  With --scales the plain loop's one
launch is ops.predict_tta over the same entries, the multi-scale form of ops.predict_up.
"""
import itertools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import analysis_ref as ref  # noqa: E402
from maxsquareloss_amd import hip, ops  # noqa: E402
from maxsquareloss_amd.utils import palette  # noqa: E402


# ----------------------------------------------------------------------------- msl_image_metrics
def _same_row(got, want):
    H = ref.HEAD
    assert np.array_equal(got[H:], want[H:], equal_nan=True)            # per-class IoU, bit for bit
    assert got[0] == want[0] and got[7] == want[7] and got[8] == want[8]  # PA, pixels, selected
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want[1:7])
    d = np.abs(got[1:7][ok] - want[1:7][ok])
    assert (d <= ref.MEAN_TOL).all(), (got[:H], want[:H])
    return float(d.max()) if d.size else 0.0


@pytest.mark.parametrize("C", [1, 13, 16, 19, 32])
def test_image_metrics(C):
    CAP = 3
    mats = ref.matrices(C)
    assert len(mats) >= 5  # the cursor wraps at capacity 3
    rows, state = ops.metrics_buffers(C, CAP, "cuda")
    image = torch.zeros(C * C, dtype=torch.int64, device="cuda")
    total = torch.zeros(C * C, dtype=torch.int64, device="cuda")
    shadow, sum_cm, worst, picked = np.zeros((CAP, ref.HEAD + C)), np.zeros((C, C), np.int64), 0.0, []
    for i, (name, m) in enumerate(mats.items()):
        miou = ref.val_miou(ref.metrics_row(m, 0.5), C)
        if name == "half" or np.isnan(miou):
            thr = 0.5
        else:
            thr = miou + (0.01 if i % 2 else -0.01)
            assert abs(thr - miou) >= 1e-6
        want = ref.metrics_row(m, thr)
        image.copy_(torch.from_numpy(m.reshape(-1).copy()))
        ops.image_metrics(image, total, thr, rows, state)
        got_rows, st = rows.cpu().numpy(), state.cpu().numpy().tolist()
        slot = i % CAP
        worst = max(worst, _same_row(got_rows[slot], want))
        shadow[slot] = got_rows[slot]
        assert np.array_equal(got_rows, shadow, equal_nan=True), name  # only that row was written
        assert st == [i + 1, int(want[8]), slot], (name, st)
        sum_cm += m
        assert np.array_equal(total.view(C, C).cpu().numpy(), sum_cm) and not image.any().item(), name
        picked.append(int(want[8]))
        if C != 16:
            assert np.isnan(got_rows[slot][4:7]).all()
        if name == "half" and C > 1:  # every IoU exactly 0.5, threshold 0.5: strict, not selected
            assert (got_rows[slot][ref.HEAD:] == 0.5).all() and ref.val_miou(got_rows[slot], C) == 0.5
            assert st[1] == 0
        if name == "zero":
            assert got_rows[slot][0] == 0.0 and np.isnan(got_rows[slot][1:4]).all() and st[1] == 0
    print(f"C={C}: max |mean - restatement| = {worst:.2e}; selected {picked}")
    assert 0 < sum(picked) < len(picked) or C == 1


def test_image_metrics_strict_threshold_and_wrapper_checks():
    C = 19
    m = ref.matrices(C)["half"]
    rows, state = ops.metrics_buffers(C, 2, "cuda")
    total = torch.zeros(C * C, dtype=torch.int64, device="cuda")
    for thr, want in ((0.5, 0), (float(np.nextafter(0.5, 1)), 1), (float("nan"), 0)):
        image = torch.from_numpy(m.reshape(-1).copy()).cuda()
        ops.image_metrics(image, total, thr, rows, state)
        assert state.cpu().tolist()[1] == want, thr
    with pytest.raises(hip.MSLError):
        ops.image_metrics(total[:-1], total, 0.5, rows, state)
    with pytest.raises(hip.MSLError):
        ops.image_metrics(total, total, 0.5, rows[:, :-1], state)
    with pytest.raises(hip.MSLError):
        ops.image_metrics(total, total, 0.5, rows, state.long())


# ----------------------------------------------------------------------------- msl_analysis_maps
C_MAPS = 19
SUBSETS = [s for n in range(1, 5) for s in itertools.combinations(ops.ANALYSIS_MAPS, n)]


def _map_case(h, w):
    x, label, cls = ref.map_inputs(h, w, C_MAPS)
    want = ref.maps(x, label, cls, palette.palette_table(C_MAPS), C_MAPS)
    dev = (torch.from_numpy(x)[None].cuda(), torch.from_numpy(label).cuda().reshape(-1),
           torch.from_numpy(cls).cuda())
    return want, dev


@pytest.mark.parametrize("h,w", [(3, 4), (5, 7), (8, 12), (33, 64)])  # dword, byte, dword, three blocks
def test_analysis_maps_every_output_subset(h, w):
    want, (x, label, cls) = _map_case(h, w)
    for subset in SUBSETS:
        out = ops.analysis_maps(x, label, cls, C_MAPS, want=subset)
        assert tuple(out) == subset
        for k in subset:
            assert out[k].shape == (1, h, w, 3)
            assert np.array_equal(out[k][0].cpu().numpy(), want[k]), (subset, k)


def test_analysis_maps_unaligned_outputs_take_the_byte_path():
    """w % 4 == 0 but maps that do not start on a dword: the kernel must not store dwords."""
    h, w = 8, 12
    want, (x, label, cls) = _map_case(h, w)
    n = h * w * 3
    raws = {k: torch.full((n + 8,), 0xA5, dtype=torch.uint8, device="cuda") for k in ops.ANALYSIS_MAPS}
    out = {k: r[1:1 + n].view(1, h, w, 3) for k, r in raws.items()}
    assert all(t.data_ptr() % 4 == 1 and t.is_contiguous() for t in out.values())
    ops.analysis_maps(x, label, cls, C_MAPS, out=out)
    for k, r in raws.items():
        r = r.cpu().numpy()
        assert np.array_equal(r[1:1 + n].reshape(h, w, 3), want[k]), k
        assert r[0] == 0xA5 and (r[1 + n:] == 0xA5).all()  # nothing written around it


@pytest.mark.parametrize("shift_x,shift_cls", [(True, False), (False, True), (True, True)])
def test_analysis_maps_unaligned_inputs_take_the_scalar_path(shift_x, shift_cls):
    """w % 4 == 0 and aligned outputs, but an x that is not on 16 bytes or a class map that is not on a dword:
    no float4 / dword load may be issued (it would fault or read the neighbouring pixels)."""
    h, w = 8, 12
    want, (x, label, cls) = _map_case(h, w)
    if shift_x:
        raw = torch.zeros(3 * h * w + 4, dtype=torch.float32, device="cuda")
        raw[1:1 + 3 * h * w] = x.reshape(-1)
        x = raw[1:1 + 3 * h * w].view(1, 3, h, w)
        assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    if shift_cls:
        raw_c = torch.zeros(h * w + 4, dtype=torch.uint8, device="cuda")
        raw_c[1:1 + h * w] = cls.reshape(-1)
        cls = raw_c[1:1 + h * w].view(h, w)
        assert cls.data_ptr() % 4 == 1 and cls.is_contiguous()
    out = ops.analysis_maps(x, label, cls, C_MAPS, want=ops.ANALYSIS_MAPS)
    for k in ops.ANALYSIS_MAPS:
        assert np.array_equal(out[k][0].cpu().numpy(), want[k]), k


@pytest.mark.parametrize("h,w", [(5, 7), (8, 12)])
def test_analysis_maps_gate_and_slot(h, w):
    want, (x, label, cls) = _map_case(h, w)
    SLOTS = 3

    def rings():
        r = ops.analysis_buffers((h, w), ops.ANALYSIS_MAPS, SLOTS, "cuda")
        for t in r.values():
            t.fill_(0xA5)
        return r

    out = rings()  # gate 0: nothing is written, whatever the slot says
    state = torch.tensor([4, 0, 1], dtype=torch.int32, device="cuda")
    ops.analysis_maps(x, label, cls, C_MAPS, state=state, out=out)
    assert all((t == 0xA5).all().item() for t in out.values())
    for slot in range(SLOTS):  # gate 1: slot k and only slot k
        out = rings()
        state = torch.tensor([9, 1, slot], dtype=torch.int32, device="cuda")
        ops.analysis_maps(x, label, cls, C_MAPS, state=state, out=out)
        for k, t in out.items():
            t = t.cpu().numpy()
            assert np.array_equal(t[slot], want[k]), (slot, k)
            assert all((t[s] == 0xA5).all() for s in range(SLOTS) if s != slot), (slot, k)
    out = rings()  # no state: always, slot 0
    ops.analysis_maps(x, label, cls, C_MAPS, out=out)
    for k, t in out.items():
        t = t.cpu().numpy()
        assert np.array_equal(t[0], want[k]) and (t[1:] == 0xA5).all()
    assert state.cpu().tolist() == [9, 1, SLOTS - 1]  # the launch only reads it


def test_analysis_maps_wrapper_checks():
    _, (x, label, cls) = _map_case(3, 4)
    with pytest.raises(hip.MSLError):
        ops.analysis_maps(x, label, cls, C_MAPS, want=())
    with pytest.raises(hip.MSLError):
        ops.analysis_maps(x, label, cls, C_MAPS, want=("heat",))
    with pytest.raises(hip.MSLError):
        ops.analysis_maps(x, label[:-1], cls, C_MAPS)
    with pytest.raises(hip.MSLError):
        ops.analysis_maps(x, label, cls.int(), C_MAPS)
    with pytest.raises(hip.MSLError, match=r"status -3"):  # error needs the label
        ops.analysis_maps(x, None, cls, C_MAPS, want=("error",))
    out = ops.analysis_maps(x, None, None, C_MAPS, want=("input",))  # the input alone needs neither
    assert np.array_equal(out["input"][0].cpu().numpy(), ref.input_image(x[0].cpu().numpy()))


# ----------------------------------------------------------------------------- end to end
H, W = 128, 256
ITEMS, RING = 5, 2
KINDS = ("label", "pred", "style", "error")


@pytest.fixture(scope="module")
def model():
    """An eval-mode model with filled running statistics and logits spread to std 2 over the classes, as
    tests/test_gpu_evaluate.py builds it."""
    from maxsquareloss_amd.tools import evaluate
    from maxsquareloss_amd.utils.synthetic import synthetic_image
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


def _plain_loop(model, data, flip, scales):
    """Per item: one prediction launch into a fresh matrix, the host Eval's scores of it, the class map."""
    from maxsquareloss_amd.utils.eval import Eval
    from maxsquareloss_amd.utils.validate import SINGLE_SCALE, tta_entries
    out = []
    with torch.no_grad():
        for i in range(len(data)):
            x, y, _ = data[i]
            xd, yd = x.cuda(), y.cuda().reshape(-1)
            cm = torch.zeros(19 * 19, dtype=torch.int64, device="cuda")
            if tuple(scales) != SINGLE_SCALE:
                arg = ops.predict_tta(tta_entries(model, xd, scales, flip), (H, W), yd, cm, want_argmax=True)
            elif flip:
                (low, _), (low_f, _) = model.predict_low(xd, flip=True)
                arg = ops.predict_up(low, (H, W), low_f, yd, cm, want_argmax=True)
            else:
                arg = ops.predict_up(model.predict_low(xd)[0], (H, W), None, yd, cm, want_argmax=True)
            ev = Eval(19)
            ev.confusion_matrix = cm.view(19, 19).cpu().numpy()
            scores = (ev.Pixel_Accuracy(), ev.Mean_Pixel_Accuracy(), ev.Mean_Intersection_over_Union(),
                      ev.Frequency_Weighted_Intersection_over_Union())
            out.append((scores, arg.cpu().numpy().astype(np.uint8).reshape(H, W), x[0].numpy(), y[0].numpy()))
    return out


def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


@pytest.mark.parametrize("tag,flip,scales", [("plain", False, (1.0,)), ("flip", True, (1.0,)),
                                             ("scales", False, (0.75, 1.0))])
def test_analyzer_end_to_end(model, tag, flip, scales, tmp_path, capsys):
    import PIL.Image  # noqa: F401  the pictures are PNGs: a missing Pillow fails here, it does not skip
    from PIL import Image
    from maxsquareloss_amd.utils import analysis as an
    from maxsquareloss_amd.utils.validate import Validator
    dev = torch.device("cuda", 0)
    plain = Validator(model, 19, (H, W), ITEMS, dev, flip=flip, scales=scales)
    total_want = plain.run().confusion_matrix
    loop = _plain_loop(model, plain.data, flip, scales)
    mious = sorted(s[2] for s, *_ in loop)
    thr = 0.5 * (mious[1] + mious[2])
    gaps = [abs(thr - v) for v in mious]
    print(f"{tag}: per-image MIoU {mious}, threshold {thr!r}, min distance {min(gaps):.3e}")
    assert min(gaps) >= 1e-9
    below = [i for i, (s, *_) in enumerate(loop) if s[2] < thr]
    assert len(below) == 2

    def run(name, graph, threshold, workers=0):
        a = an.Analyzer(model, 19, (H, W), ITEMS, dev, str(tmp_path / name), flip=flip, scales=scales, graph=graph,
                        threshold=threshold, kinds=KINDS, ring=RING, workers=workers)
        rows = a.run()
        assert rows is a.rows and len(rows) == ITEMS and a.drains == 3  # 2 + 2 + 1
        assert a.replays == (ITEMS - 1 if graph else 0)                 # image 0 runs eagerly, then is captured
        assert np.array_equal(a.totalEval.confusion_matrix, total_want)
        assert not a.Eval._dev.any().item()
        return a

    eager, graphed = run("eager", False, thr), run("graph", True, thr, workers=2)
    assert eager.rows == graphed.rows and eager.table == graphed.table
    worst = 0.0
    for i, (ident, PA, MPA, MIoU, FWIoU) in enumerate(eager.rows):
        want = loop[i][0]
        assert ident == f"{i:06d}" and PA == want[0]
        d = max(abs(a - b) for a, b in zip((MPA, MIoU, FWIoU), want[1:]))
        worst = max(worst, d)
        assert d <= ref.MEAN_TOL
        assert eager.table[i][5] == int(total_pixels(loop[i][3])) and eager.table[i][6] == int(i in below)
    print(f"{tag}: max |row - host Eval| = {worst:.2e}")
    assert sum(t[5] for t in eager.table) == int(total_want.sum())

    # exactly the images below the threshold have files, and they hold the restatement's bytes
    names = sorted(an.file_name(eager.rows[i][0], eager.rows[i][1:], k) for i in below for k in KINDS)
    files_e, files_g = _files(eager.out_dir), _files(graphed.out_dir)
    assert sorted(files_e) == names and files_e == files_g
    pal = palette.palette_table(19)
    for i in below:
        _, cls, x, y = loop[i]
        want = ref.maps(x, y, cls, pal, 19)
        for k in KINDS:
            got = np.asarray(Image.open(os.path.join(eager.out_dir, an.file_name(eager.rows[i][0], eager.rows[i][1:], k))))
            assert np.array_equal(got, want[an.KIND_MAP[k]]), (i, k)
    for a in (eager, graphed):
        lines = open(os.path.join(a.save_dir, "per_image.csv")).read().splitlines()
        assert lines[0] == "id,PA,MPA,MIoU,FWIoU,pixels,saved" and len(lines) == 1 + ITEMS
        assert [ln.rsplit(",", 1)[1] for ln in lines[1:]] == [str(int(i in below)) for i in range(ITEMS)]
    out = capsys.readouterr().out
    assert out.count("totalPA, totalMPA, totalMIoU, totalFWIoU") == 2 and "##### IOU for each class is #####" in out

    # threshold -1 writes no file, threshold 2 writes all
    none, every = run("none", False, -1.0), run("all", True, 2.0)
    assert os.listdir(none.out_dir) == [] and all(t[6] == 0 for t in none.table)
    assert len(os.listdir(every.out_dir)) == ITEMS * len(KINDS) and all(t[6] == 1 for t in every.table)
    assert none.rows == eager.rows == every.rows
    assert [r[0] for r in eager.worst(2)] == [f"{i:06d}" for i in sorted(below, key=lambda i: loop[i][0][2])]
    capsys.readouterr()


def total_pixels(label):
    return ((label >= 0) & (label < 19)).sum()


def test_analysis_tool_runs_on_synthetic_items(model, tmp_path):
    import PIL.Image  # noqa: F401  the pictures are PNGs: a missing Pillow fails here, it does not skip
    from maxsquareloss_amd.tools import analysis
    args, train_id, logger = analysis.parse_args([
        "--crop_size", f"{W},{H}", "--target_crop_size", f"{W},{H}", "--imagenet_pretrained", "False",
        "--save_dir", str(tmp_path), "--val_images", "4", "--graph", "True", "--ring", "3", "--worst", "2"])
    agent = analysis.resultEvaluater(args, cuda=True, train_id=train_id, logger=logger)
    agent.model.load_state_dict(model.state_dict())
    rows = agent.main()
    assert len(rows) == 4 and agent.validator.drains == 2 and agent.validator.replays == 3
    saved = [t for t in agent.validator.table if t[6]]
    assert len(os.listdir(tmp_path / "savePics")) == 3 * len(saved) and (tmp_path / "per_image.csv").exists()
    assert len(saved) == sum(1 for r in rows if r[3] < 0.5)
