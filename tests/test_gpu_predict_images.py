"""The prediction images on the GPU: msl_predict_images against msl_predict_up (the class and the matrix, bit
for bit), against itself (every map is a table lookup of the class map written) and against the torch-CPU
restatement (tests/predict_images_ref.py) for what is decided from the winning probability; msl_colorize and
decode_labels against data recorded from the reference; the Validator with an output request, eager and as a
captured graph; tools/predict.py on a list of PNGs.

Inputs: counter_normal logits of std 6; for flip the mirrored image's logits are the mirror of those plus std 1
noise, which fills all five confidence buckets at every shape (asserted on the restatement).  Bucket and
pseudo-label decisions must equal the restatement's wherever its near-edge mask (the reference probability within
1e-5 of 0.9, 0.8, 0.7, 0.5 or the 0.95 threshold) is clear; on it the neighbouring bucket / the other decision is
accepted too.  The mask may hold max(2, 0.1 %) of the pixels; measured on the CPU for these inputs it holds 1 of 192
pixels at 12 x 16, 2 of 2840 at 40 x 71, none at the other small shapes and 1.6e-4 of the pixels at 1028 x 1032.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import evaluate_ref as ev  # noqa: E402
import predict_images_ref as ref  # noqa: E402
from maxsquareloss_amd import hip, ops  # noqa: E402
from maxsquareloss_amd.utils import palette  # noqa: E402

MAPS = tuple(ops.IMAGE_MAPS)
CASES = [(s, f, False) for s in ref.SHAPES for f in (False, True)] + [(ref.SHAPES[0], f, True) for f in (False, True)]


def _run(shape, flip, nan, want=MAPS, with_label=True):
    """One ops.predict_images call -> ({map: numpy}, matrix or None)."""
    C, hi, wi, ho, wo = shape
    low, lowf = ref.inputs(C, hi, wi, flip, nan)
    lab = cm = None
    if with_label:
        lab = ev.labels(C, ho, wo).cuda().reshape(-1)
        cm = torch.zeros(C * C, dtype=torch.int64, device="cuda")
    out = ops.predict_images(low.cuda(), (ho, wo), None if lowf is None else lowf.cuda(), lab, cm, want=want,
                             thr=ref.THR)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, None if cm is None else cm.view(C, C).cpu().numpy()


def _predict_up(shape, flip, nan):
    C, hi, wi, ho, wo = shape
    low, lowf = ref.inputs(C, hi, wi, flip, nan)
    cm = torch.zeros(C * C, dtype=torch.int64, device="cuda")
    arg = ops.predict_up(low.cuda(), (ho, wo), None if lowf is None else lowf.cuda(),
                         ev.labels(C, ho, wo).cuda().reshape(-1), cm, want_argmax=True)
    torch.cuda.synchronize()
    return arg.cpu().numpy().astype(np.int64), cm.view(C, C).cpu().numpy()


@pytest.mark.parametrize("shape,flip,nan", CASES)
def test_predict_images(shape, flip, nan):
    C, hi, wi, ho, wo = shape
    npx = ho * wo
    out, cm = _run(shape, flip, nan)
    cls = out["class"].reshape(-1).astype(np.int64)
    assert out["class"].shape == (ho, wo) and out["color"].shape == (ho, wo, 3) and cls.max() < C

    # the class and the matrix are msl_predict_up's, bit for bit
    arg, cm_up = _predict_up(shape, flip, nan)
    assert np.array_equal(cls, arg)
    assert np.array_equal(cm, cm_up) and cm.sum() > 0

    # the class against the restatement: exact off the near-tie mask, one of the two leading classes on it
    r = ref.reference(shape, flip, nan)
    near = r["near_tie"]
    assert np.array_equal(cls[~near], r["cls"][~near])
    if near.any():
        assert ((cls[near] == r["top2"][0][near]) | (cls[near] == r["top2"][1][near])).all()
    if nan:
        assert np.isnan(r["top"]).any()

    # every map is a lookup of the class map written: exact everywhere
    ids, pal, shade = palette.id_table(C), palette.palette_table(C), palette.shade_table(C)
    assert np.array_equal(out["ids"].reshape(-1), ids[cls])
    assert np.array_equal(out["color"].reshape(-1, 3), pal[cls])
    conf, pseudo = out["confidence"].reshape(-1, 3), out["pseudo"].reshape(-1).astype(np.int64)
    shades = np.concatenate([shade, np.zeros((1, C, 3), np.uint8)])[:, cls]  # [5][npx][3]
    hit = (shades == conf[None]).all(axis=2)
    assert (hit.sum(axis=0) == 1).all()  # one of the five shades of the class's colour
    bucket = hit.argmax(axis=0)
    assert ((pseudo == cls) | (pseudo == 255)).all()
    kept = pseudo != 255

    # the decisions against the restatement
    edge = r["near_edge"]
    counts = np.bincount(r["bucket"], minlength=5)
    print(f"{shape} flip={flip} nan={nan}: buckets {counts.tolist()}, kept {int(r['keep'].sum())}, near-edge "
          f"{int(edge.sum())} of {npx}, bucket diffs {int((bucket != r['bucket']).sum())}, pseudo diffs "
          f"{int((kept != r['keep']).sum())}")
    assert edge.sum() <= max(2, npx // 1000)
    if not nan:
        assert (counts > 0).all() and 0 < r["keep"].sum() < npx
    assert np.array_equal(bucket[~edge], r["bucket"][~edge])
    assert (np.abs(bucket[edge] - r["bucket"][edge]) <= 1).all()
    assert np.array_equal(kept[~edge], r["keep"][~edge])
    nanpx = np.isnan(r["top"])
    assert (bucket[nanpx] == 4).all() and not kept[nanpx].any()


@pytest.mark.parametrize("shape", [ref.SHAPES[2], ref.SHAPES[1]])  # the byte path and the dword path
@pytest.mark.parametrize("flip", [False, True])
def test_each_output_alone_gives_the_same_bytes(shape, flip):
    C = shape[0]
    full, cm = _run(shape, flip, False)
    for k in MAPS:
        one, none = _run(shape, flip, False, want=(k,), with_label=False)
        assert none is None and list(one) == [k] and np.array_equal(one[k], full[k]), k
    # the matrix alone, and buffers handed in
    only, cm2 = _run(shape, flip, False, want=())
    assert only == {} and np.array_equal(cm2, cm)
    low, lowf = ref.inputs(C, shape[1], shape[2], flip)
    bufs = ops.image_buffers(shape[3:], ("pseudo", "color"), "cuda")
    got = ops.predict_images(low.cuda(), shape[3:], None if lowf is None else lowf.cuda(), out=bufs, thr=ref.THR)
    assert got is bufs and np.array_equal(bufs["pseudo"].cpu().numpy(), full["pseudo"])
    assert np.array_equal(bufs["color"].cpu().numpy(), full["color"])


def test_unaligned_outputs_take_the_byte_path():
    """wo % 4 == 0 but a map that does not start on a dword: the kernel must not store dwords."""
    shape = ref.SHAPES[1]
    C, hi, wi, ho, wo = shape
    full, _ = _run(shape, False, False)
    low = ref.inputs(C, hi, wi, False)[0].cuda()
    idl, pal, shade = ops.image_tables(C, low.device)
    raw = torch.full((ho * wo * 3 + 8,), 77, dtype=torch.uint8, device="cuda")
    col = raw[1:1 + ho * wo * 3]
    assert col.data_ptr() % 4 == 1
    hip.check(hip.load().msl_predict_images(low.data_ptr(), None, C, hi, wi, ho, wo, None, None, 0.95, idl.data_ptr(),
                                            pal.data_ptr(), shade.data_ptr(), None, None, col.data_ptr(), None, None,
                                            hip.stream_ptr()), "msl_predict_images")
    torch.cuda.synchronize()
    raw = raw.cpu().numpy()
    assert np.array_equal(raw[1:1 + ho * wo * 3].reshape(ho, wo, 3), full["color"])
    assert raw[0] == 77 and (raw[1 + ho * wo * 3:] == 77).all()  # nothing written around it


def test_predict_images_rejects_bad_arguments():
    lib = hip.load()
    low = torch.zeros(1, 19, 3, 3, device="cuda")
    u8 = torch.zeros(63 * 3, dtype=torch.uint8, device="cuda")
    lab = torch.zeros(63, dtype=torch.int64, device="cuda")
    cm = torch.zeros(19 * 19, dtype=torch.int64, device="cuda")
    idl, pal, shade = (t.data_ptr() for t in ops.image_tables(19, low.device))
    s, L, o = hip.stream_ptr(), low.data_ptr(), u8.data_ptr()

    def call(c=19, label=None, conf=None, tables=(idl, pal, shade), outs=(o, None, None, None, None), ho=7):
        return lib.msl_predict_images(L, None, c, 3, 3, ho, 9, label, conf, 0.95, *tables, *outs, s)

    assert call(outs=(None,) * 5) == -3                                   # no output
    assert call(label=lab.data_ptr()) == -3                               # label without confusion
    assert call(conf=cm.data_ptr()) == -3                                 # confusion without label
    assert call(c=33) == -3                                               # the register arrays hold 32 classes
    assert call(ho=0) == -3                                               # geometry
    assert call(tables=(None, pal, shade), outs=(None, o, None, None, None)) == -3   # ids without id_lut
    assert call(tables=(idl, None, shade), outs=(None, None, o, None, None)) == -3   # color without palette
    assert call(tables=(idl, pal, None), outs=(None, None, None, o, None)) == -3     # confidence without shade
    assert call(tables=(None, None, None), outs=(o, None, None, None, o)) == 0       # class and pseudo need no table
    assert call(outs=(None,) * 5, label=lab.data_ptr(), conf=cm.data_ptr()) == 0     # the matrix alone
    assert lib.msl_colorize(None, 1, 4, pal, 19, o, s) == -3 and lib.msl_colorize(lab.data_ptr(), 1, 4, None, 19, o, s) == -3
    assert lib.msl_colorize(lab.data_ptr(), 1, 4, pal, 257, o, s) == -3 and lib.msl_colorize(lab.data_ptr(), 2, 4, pal, 19, o, s) == -3
    assert lib.msl_colorize(lab.data_ptr(), 1, 0, pal, 19, o, s) == 0
    torch.cuda.synchronize()
    assert cm.sum().item() == 63
    with pytest.raises(hip.MSLError):
        ops.predict_images(low, (7, 9), want=())  # nothing to compute
    with pytest.raises(hip.MSLError):
        ops.predict_images(low, (7, 9), want=("heat",))
    with pytest.raises(hip.MSLError):
        ops.predict_images(low, (7, 9), label=lab)
    with pytest.raises(hip.MSLError):  # no tables for 21 classes
        ops.predict_images(torch.zeros(1, 21, 3, 3, device="cuda"), (7, 9))


# ----------------------------------------------------------------------------- colorize / the reference names
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_colorize_equals_the_golden(dtype):
    g = ref.gold()
    pal = torch.from_numpy(g["label_colours"][:19].copy()).cuda()
    for key, want in (("mask_a", "decode_a"), ("mask_b", "decode_b")):
        out = ops.colorize(torch.from_numpy(g[key]).to(dtype).cuda(), pal)
        assert out.dtype == torch.uint8 and tuple(out.shape) == g[key].shape + (3,)
        assert np.array_equal(out.permute(0, 3, 1, 2).cpu().numpy(), g[want])
    # an odd pixel count: the partial last quad stores bytes
    m = torch.from_numpy(g["mask_a"][0, :, :7]).to(dtype).cuda()  # 49 pixels
    assert np.array_equal(ops.colorize(m, pal).permute(2, 0, 1).cpu().numpy(), g["decode_a"][0][:, :, :7])


def test_decode_labels_and_inv_preprocess_on_device_tensors():
    from maxsquareloss_amd.datasets.cityscapes_Dataset import decode_labels, inv_preprocess
    g = ref.gold()
    for key, n, want in (("mask_a", 2, "decode_a"), ("mask_a", 1, "decode_a_n1"), ("mask_b", 5, "decode_b_n5")):
        out = decode_labels(torch.from_numpy(g[key]).cuda(), n)
        assert out.is_cuda and out.dtype == torch.float32
        assert torch.equal(out.cpu(), torch.from_numpy(g[want].astype("float32")).div_(255.0)), want
    out = decode_labels(torch.from_numpy(g["mask_b"]).cuda().to(torch.uint8), 1)  # 255-style maps: any integer type
    assert out.shape == (1, 3, 12, 16)
    for flag in (False, True):
        out = inv_preprocess(torch.from_numpy(g["img"].copy()).cuda(), 2, numpy_transform=flag)
        assert out.is_cuda and (out.cpu().numpy() - g[f"inv_np{int(flag)}"]).__abs__().max() <= 1e-6


# ----------------------------------------------------------------------------- model level
H, W = 128, 256  # the smallest size the suite holds the whole model to (tests/test_gpu_evaluate.py)
KINDS = ("color", "trainids", "labelids", "confidence", "pseudo", "input")


@pytest.fixture(scope="module")
def model():
    """An eval-mode model with filled running statistics and logits spread to std 2 over the classes (random-init
    logits have tiny margins), as tests/test_gpu_evaluate.py builds it."""
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


def _files(d):
    out = {}
    for kind in sorted(os.listdir(d)):
        for name in sorted(os.listdir(os.path.join(d, kind))):
            out[kind + "/" + name] = open(os.path.join(d, kind, name), "rb").read()
    return out


@pytest.mark.parametrize("flip", [False, True])
def test_validator_writes_the_same_files_eager_and_graphed(model, flip, tmp_path):
    pytest.importorskip("PIL.Image")
    from PIL import Image
    from maxsquareloss_amd.utils.images import OutputRequest
    from maxsquareloss_amd.utils.synthetic import synthetic_rgb
    from maxsquareloss_amd.utils.validate import VAL_OFFSET, Validator
    dev = torch.device("cuda", 0)
    plain = Validator(model, 19, (H, W), 3, dev, flip=flip).run().confusion_matrix
    runs = {}
    for tag, graph, workers in (("eager", False, 0), ("graph", True, 2)):
        req = OutputRequest(str(tmp_path / tag), KINDS, threshold=0.6, workers=workers)
        v = Validator(model, 19, (H, W), 3, dev, flip=flip, graph=graph, outputs=req)
        runs[tag] = (v.run().confusion_matrix, _files(tmp_path / tag))
        if graph:
            assert [g.replays for g in v._graphed.values()] == [2]  # image 0 eager, then two replays
    (cm_e, files_e), (cm_g, files_g) = runs["eager"], runs["graph"]
    assert np.array_equal(cm_e, plain) and np.array_equal(cm_g, plain) and plain.sum() > 0  # the metrics' matrix
    assert sorted(files_e) == [f"{k}/{i:06d}.png" for k in sorted(KINDS) for i in range(3)]
    assert files_e == files_g  # byte for byte
    # what is in them: the recovered input is the synthetic image, the maps are consistent with each other
    for i in range(3):
        def png(kind):
            return np.asarray(Image.open(tmp_path / "eager" / kind / f"{i:06d}.png"))
        assert np.array_equal(png("input"), synthetic_rgb(H, W, VAL_OFFSET + i))
        cls = png("trainids").astype(np.int64)
        assert cls.shape == (H, W) and len(np.unique(cls)) > 1
        assert np.array_equal(png("labelids"), palette.id_table(19)[cls])
        assert np.array_equal(png("color"), palette.palette_table(19)[cls])
        ps = png("pseudo")
        assert ((ps == cls) | (ps == 255)).all()


def test_predict_tool_writes_out_size_files(model, tmp_path):
    pytest.importorskip("PIL.Image")
    from PIL import Image
    from maxsquareloss_amd.tools import predict
    from maxsquareloss_amd.utils.preprocess import resize_image
    lists, out = tmp_path / "lists", tmp_path / "out"
    lists.mkdir()
    rng = np.random.default_rng(3)
    paths = []
    for k in range(3):
        paths.append(str(tmp_path / f"frame_{k}.png"))
        Image.fromarray(rng.integers(0, 256, size=(40, 70, 3), dtype=np.uint8)).save(paths[-1])
    (lists / "test.txt").write_text("\n".join(paths) + "\n")
    OW, OH = 96, 52
    args, train_id, logger = predict.parse_args([
        "--list_path", str(lists), "--imagenet_pretrained", "False", "--save_dir", "", "--resize", "True",
        "--save_predictions", str(out), "--save_kinds", "trainids,color", "--out_size", f"{OW},{OH}",
        "--data_loader_workers", "2"])
    args.seg_size = (W, H)
    p = predict.Predictor(args, cuda=True, train_id=train_id, logger=logger)
    p.model.load_state_dict(model.state_dict())
    p.main()
    assert sorted(os.listdir(out)) == ["color", "trainids"]
    assert sorted(os.listdir(out / "trainids")) == [f"frame_{k}.png" for k in range(3)]
    for k in range(3):
        got = np.asarray(Image.open(out / "trainids" / f"frame_{k}.png"))
        assert got.shape == (OH, OW) and Image.open(out / "color" / f"frame_{k}.png").size == (OW, OH)
        rgb = torch.from_numpy(np.asarray(Image.open(paths[k]).convert("RGB")).copy()).cuda()
        with torch.no_grad():
            low = p.model.eval().predict_low(resize_image(rgb, (W, H)))[0]
        want = ops.predict_images(low, (OH, OW), want=("class",))["class"].cpu().numpy()
        assert np.array_equal(got, want)
        assert np.array_equal(np.asarray(Image.open(out / "color" / f"frame_{k}.png")),
                              palette.palette_table(19)[want.astype(np.int64)])
