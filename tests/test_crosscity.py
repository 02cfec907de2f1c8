"""CPU tests of the cross-city feature: the host half of the JPEG decoder (csrc/jpeg_host.h behind the library's
host entry points) with the numpy restatement of the device half (utils/jpeg.py) byte for byte against Pillow's
decoder, its behaviour on unsupported, truncated and corrupted files, CrossCity_Dataset on a tiny tree, and the
C ABI."""
import argparse
import ctypes
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "jpeg_kat.npz")
OK, ERR_SHAPE, ERR_ARG = 0, -1, -3
GUARD = 0x5A5A
MAX_ELEMS = 1 << 26  # a corrupted size field can ask for gigabytes: such a header is not decoded


def _lib():
    from maxsquareloss_amd import hip
    return hip, hip.load(require_gpu=False)


# ------------------------------------------------------------------------------------ the decode against Pillow
@pytest.mark.parametrize("h", jpeg_ref.HEIGHTS)
def test_numpy_decode_equals_pillow(h):
    """Widths 1..9 and the 15/16/17, 31/32/33 block edges, the three samplings and grayscale, quality 1..100,
    noise, two-level and smooth pictures, optimised tables and every restart layout; widths 3..4 under 4:2:x are
    the box-replicated chroma planes."""
    pytest.importorskip("PIL")
    from maxsquareloss_amd.utils import jpeg
    n = 0
    for label, data in jpeg_ref.sweep(h):
        want = jpeg_ref.pillow_rgb(data)
        got = jpeg.decode(data)
        assert got is not None, label
        assert got.dtype == np.uint8 and got.shape == want.shape, label
        assert np.array_equal(got, want), (label, np.argwhere(got != want)[:4])
        n += 1
    assert n == len(jpeg_ref.WIDTHS) * 4 * 4 * 3


def test_sweep_covers_what_it_says():
    labels = [label for h in (3, 16) for label, _ in jpeg_ref.sweep(h, widths=(3, 33))]
    for s in jpeg_ref.SAMPLINGS:
        assert {lab[5] for lab in labels if lab[2] == s} == {tuple(o) for o in jpeg_ref.OPTIONS}
    assert {lab[3] for lab in labels} == set(jpeg_ref.QUALITIES) and {lab[4] for lab in labels} == set(jpeg_ref.KINDS)


def test_payload_layout_and_header():
    pytest.importorskip("PIL")
    from maxsquareloss_amd.utils import jpeg
    data = jpeg_ref.encode(jpeg_ref.photo(33, 50), 2, quality=80, restart_marker_blocks=3)
    st, h = jpeg.info(data)
    assert st == OK and (h.width, h.height, h.ncomp, h.hmax, h.vmax, h.restart_interval) == (50, 33, 3, 2, 2, 3)
    assert (h.mcus_w, h.mcus_h) == (4, 3)
    assert [(c.h, c.v, c.blocks_w, c.blocks_h, c.offset) for c in h.comp] == [
        (2, 2, 8, 6, 0), (1, 1, 4, 3, 48 * 64), (1, 1, 4, 3, 60 * 64)]
    payload = jpeg.decode_file(data)
    assert payload.dtype == np.uint8 and payload.ndim == 1 and jpeg.is_payload(payload)
    assert payload.size == jpeg.COEF_AT + 2 * 72 * 64
    h2, quant, comps = jpeg.split(payload)
    assert bytes(h2) == bytes(h) and quant.shape == (4, 64) and quant[0].min() >= 1 and not quant[2:].any()
    assert [c.shape for c in comps] == [(6, 8, 64), (3, 4, 64), (3, 4, 64)]
    gray = jpeg.split(jpeg.decode_file(jpeg_ref.encode(jpeg_ref.photo(9, 17), "L", quality=80)))[0]
    assert (gray.ncomp, gray.hmax, gray.vmax, gray.comp[0].blocks_w, gray.comp[0].blocks_h) == (1, 1, 1, 3, 2)


def test_sixteen_bit_tables_and_extended_sequential():
    """A DQT with 16-bit entries and the SOF1 marker: the same coefficients as the 8-bit SOF0 file."""
    pytest.importorskip("PIL")
    from maxsquareloss_amd.utils import jpeg
    data = jpeg_ref.encode(jpeg_ref.photo(20, 30), 2, quality=70)
    out, i = bytearray(data[:2]), 2
    while data[i + 1] != 0xDA:
        m, L = data[i + 1], struct.unpack(">H", data[i + 2:i + 4])[0]
        seg = data[i + 4:i + 2 + L]
        if m == 0xDB:
            wide, p = bytearray(), 0
            while p < len(seg):
                assert seg[p] >> 4 == 0
                wide += bytes([0x10 | seg[p]]) + b"".join(struct.pack(">H", v) for v in seg[p + 1:p + 65])
                p += 65
            seg = bytes(wide)
        out += bytes([0xFF, 0xC1 if m == 0xC0 else m]) + struct.pack(">H", len(seg) + 2) + seg
        i += 2 + L
    out += data[i:]
    assert bytes(out) != data and np.array_equal(jpeg.decode(bytes(out)), jpeg_ref.pillow_rgb(data))
    assert np.array_equal(jpeg_ref.pillow_rgb(bytes(out)), jpeg_ref.pillow_rgb(data))


def test_unsupported_files_are_refused_and_the_dataset_still_equals_pillow(tmp_path):
    pytest.importorskip("PIL")
    from maxsquareloss_amd.datasets import CrossCity_Dataset
    from maxsquareloss_amd.utils import jpeg
    paths, _ = jpeg_ref.nthu_tree(tmp_path / "N", n=3, val_n=1)
    ds = CrossCity_Dataset(_args(), split="train", training=True, **{k: paths[k] for k in ("data_root_path", "list_path")})
    for item, (name, data) in enumerate(jpeg_ref.unsupported()):
        st, _ = jpeg.info(data)
        assert st == ERR_SHAPE, (name, st)
        assert jpeg.decode_file(data) is None
        with open(ds.paths(item)[0], "wb") as f:
            f.write(data)
        rgb, ids = ds.decode(item)
        assert ids is None and rgb.ndim == 3 and np.array_equal(rgb, jpeg_ref.pillow_rgb(data)), name


def test_a_size_field_the_file_cannot_hold_is_refused_before_any_allocation():
    """A corrupt SOF claiming 65535 x 65535 asks for 26 GB of coefficients; a block costs at least two bits, so the
    file cannot hold them and decode_file says so without asking for the memory."""
    pytest.importorskip("PIL")
    from maxsquareloss_amd.utils import jpeg
    data = bytearray(jpeg_ref.encode(jpeg_ref.photo(16, 16), 0, quality=70))
    at = data.index(b"\xff\xc0") + 5
    data[at:at + 4] = b"\xff\xff\xff\xff"
    st, h = jpeg.info(bytes(data))
    assert st == OK and (h.width, h.height) == (65535, 65535)
    assert jpeg.decode_file(bytes(data)) is None
    honest = jpeg_ref.encode(np.zeros((1024, 2048, 3), np.uint8), 2, quality=1, optimize=True)   # the densest file
    assert jpeg.decode_file(honest) is not None


def _decode_guarded(lib, hip, data):
    """msl_jpeg_info, then msl_jpeg_entropy_decode into a buffer with a guard block on either side; returns
    the status."""
    header = hip.JpegHeader()
    st = lib.msl_jpeg_info(data, len(data), ctypes.addressof(header))
    if st != OK:
        return st
    elems = lib.msl_jpeg_coef_elems(ctypes.addressof(header))
    assert elems > 0
    if elems > MAX_ELEMS:
        return OK
    buf = np.full(elems + 128, GUARD, np.uint16)
    quant = np.full(256 + 128, GUARD, np.uint16)
    h2 = hip.JpegHeader()
    st = lib.msl_jpeg_entropy_decode(data, len(data), ctypes.addressof(h2), buf.ctypes.data + 128, elems,
                                     quant.ctypes.data + 128)
    assert (buf[:64] == GUARD).all() and (buf[-64:] == GUARD).all(), "a guard word of the coefficient buffer"
    assert (quant[:64] == GUARD).all() and (quant[-64:] == GUARD).all(), "a guard word of the tables"
    if st == OK:
        assert bytes(h2) == bytes(header)
        assert lib.msl_jpeg_entropy_decode(data, len(data), ctypes.addressof(h2), buf.ctypes.data + 128, elems - 1,
                                           quant.ctypes.data + 128) == -2  # MSL_ERR_WORKSPACE: a short buffer
    return st


def test_truncated_and_corrupted_streams():
    """Every proper prefix of two small files (one with restarts) and 200 single-byte corruptions of each: a
    status, never a write outside the buffers, and the process lives."""
    pytest.importorskip("PIL")
    hip, lib = _lib()
    seen = {OK: 0, ERR_SHAPE: 0, ERR_ARG: 0}
    for data in jpeg_ref.fuzz_streams():
        st = _decode_guarded(lib, hip, data)
        assert st in seen, st
        seen[st] += 1
    assert seen[ERR_ARG] > 1000 and seen[OK] > 0, seen
    files = jpeg_ref.fuzz_files()
    for data in files:
        assert _decode_guarded(lib, hip, data) == OK
        assert _decode_guarded(lib, hip, data[:len(data) - 40]) == ERR_ARG   # the scan is cut short
    assert lib.msl_jpeg_info(None, 0, ctypes.addressof(hip.JpegHeader())) == ERR_ARG
    assert lib.msl_jpeg_info(files[0], len(files[0]), None) == ERR_ARG


def _sanitizer_env():
    """The environment as it is, less the two variables that change what a sanitizer reports."""
    return {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}


def _sanitizer_compiler(tmp_path):
    """(compiler, flags) that build a program with -fsanitize=address,undefined which starts under the
    environment as given, or None.  The sanitizer runtime is linked statically into the program (clang does so by
    default, gcc with -static-libasan), so it comes first whatever else the environment has loaded."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    tried = []
    for cxx in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("c++"), shutil.which("g++")):
        if not cxx or not os.path.exists(cxx) or cxx in tried:
            continue
        tried.append(cxx)
        for extra in ([], ["-static-libasan", "-static-libubsan"], ["-static-libasan"]):
            flags = ["-fsanitize=address,undefined"] + extra
            exe = tmp_path / "probe"
            r = subprocess.run([cxx] + flags + [str(probe), "-o", str(exe)], capture_output=True)
            if r.returncode == 0 and subprocess.run([str(exe)], capture_output=True, env=_sanitizer_env()).returncode == 0:
                return cxx, flags
    return None


def test_host_decoder_under_sanitizers(tmp_path):
    """tests/jpeg_host_main.cpp - its own main over csrc/jpeg_host.h alone, no HIP, no Python - built with
    AddressSanitizer and UBSan, on the same prefixes and corruptions: exit 0 and no report."""
    pytest.importorskip("PIL")
    found = _sanitizer_compiler(tmp_path)
    if found is None:
        pytest.skip("no compiler here links a sanitised program that starts under this environment")
    cxx, flags = found
    exe = tmp_path / "jpeg_host_main"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + flags +
                           ["-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "jpeg_host_main.cpp"), "-o",
                            str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    cases = tmp_path / "cases.bin"
    n = 0
    with open(cases, "wb") as f:
        for data in list(jpeg_ref.fuzz_streams()) + jpeg_ref.fuzz_files() + [d for _, d in jpeg_ref.unsupported()]:
            f.write(struct.pack("<I", len(data)) + data)
            n += 1
    run = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, env=_sanitizer_env())
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-2000:]
    m = re.fullmatch(r"ok (\d+) shape (\d+) arg (\d+)\s*", run.stdout)
    assert m and sum(int(v) for v in m.groups()) == n and int(m.group(1)) >= 2 and int(m.group(2)) >= 3, run.stdout


def test_host_header_builds_with_a_plain_host_compiler(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host compiler")
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only",
                        os.path.join(ROOT, "tests", "jpeg_host_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src = open(os.path.join(ROOT, "maxsquareloss_amd", "csrc", "jpeg_host.h")).read()
    assert "hip/" not in src and "static " in src and not re.search(r"^\s*(static|thread_local)\s+(?!const|inline)\w", src, re.M)


# ------------------------------------------------------------------------------------ the golden recording
def test_golden_recording():
    pytest.importorskip("PIL")
    from maxsquareloss_amd.utils import jpeg
    gold = np.load(GOLD)
    assert os.path.getsize(GOLD) < 64 * 1024
    for k, data in enumerate(jpeg_ref.golden_cases()):
        rec = gold[f"file_{k}"].tobytes()
        want = gold[f"rgb_{k}"]
        assert np.array_equal(jpeg.decode(rec), want), k                  # the decode equals the recording
        assert np.array_equal(jpeg_ref.pillow_rgb(rec), want), (k, "this Pillow decodes the recorded file differently")
        assert jpeg.decode(data) is not None and np.array_equal(jpeg.decode(data), jpeg_ref.pillow_rgb(data))
    kinds = [(h.ncomp, h.hmax, h.vmax, h.restart_interval > 0)
             for h in (jpeg.info(gold[f"file_{k}"].tobytes())[1] for k in range(6))]
    assert kinds == [(3, 1, 1, False), (3, 2, 1, True), (3, 2, 2, False), (3, 2, 2, True), (1, 1, 1, False),
                     (3, 2, 2, False)]


def test_idct_wraps_as_the_kernel_does():
    """Outside the range an encoder produces, the restatement is 32-bit modular arithmetic - defined, the
    kernel's - and inside it the plain integer result."""
    from maxsquareloss_amd.utils import jpeg
    rng = np.random.default_rng(3)
    x = rng.integers(-2048, 2048, (500, 8)).astype(np.int64)
    exact = jpeg._pass(x, 11)
    big = jpeg._pass(x + (1 << 32), 11)     # the same values modulo 2^32
    assert np.array_equal(exact, big)
    assert np.array_equal(jpeg._descale(np.array([5, -5, (1 << 31) + 7], np.int64), 2), [1, -1, -(1 << 29) + 2])


# ------------------------------------------------------------------------------------ the dataset
def _args(**kw):
    a = argparse.Namespace(base_size=(48, 32), crop_size=(40, 24), seg_size=(48, 32), random_mirror=True,
                           random_crop=True, resize=True, DA=False, seed=3, split="train", class_16=False,
                           class_13=True, batch_size=1, data_loader_workers=0, jpeg_decode="device")
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_dataset_on_a_tiny_tree(tmp_path):
    pytest.importorskip("PIL")
    from maxsquareloss_amd.datasets import CrossCity_DataLoader, CrossCity_Dataset, build_loader
    from maxsquareloss_amd.utils import jpeg, preprocess
    paths, made = jpeg_ref.nthu_tree(tmp_path / "N", n=3, val_n=2, png_item=1)
    args = _args(random_crop=False, resize=False, random_mirror=False)
    ds = CrossCity_Dataset(args, split="train", training=True, class_13=True, **paths)
    assert ds.name == "crosscity" and len(ds) == 3 and ds.is_train() and ds.rsize == ds.base_size == (48, 32)
    assert ds.items == ["pano_train_000", "pano_train_001", "pano_train_002"]
    root = paths["data_root_path"]
    assert ds.paths(0) == (os.path.join(root, "Images", "Train", "pano_train_000.jpg"), None, 0)
    assert ds.paths(1) == (os.path.join(root, "Images", "Train", "pano_train_001.png"), None, 1)   # no .jpg: the .png
    lut = preprocess.build_lut("cityscapes", class_13=True)
    assert np.array_equal(ds.lut, lut) and lut.max() == 12 and ds.class_13 and not ds.class_16
    assert ds.id_to_trainid == preprocess.CITYSCAPES_ID_TO_TRAINID
    pil = CrossCity_Dataset(_args(random_crop=False, resize=False, random_mirror=False, jpeg_decode="pillow"),
                            split="train", training=True, class_13=True, **paths)
    for item, (data, _) in enumerate(made["train"]):
        want = data if item == 1 else jpeg_ref.pillow_rgb(data)
        rgb, ids = ds.decode(item)
        assert ids is None and jpeg.is_payload(rgb) == (item != 1)
        rgb_p, _ = pil.decode(item)
        assert rgb_p.ndim == 3 and np.array_equal(rgb_p, want)
        plan = ds.item_plan(rgb)
        assert len(plan) == (3 if item != 1 else 2) and plan[:2] == pil.item_plan(rgb_p)
        img, lab = ds.host_transform(rgb, None, plan)
        img_p, lab_p = pil.host_transform(rgb_p, None, pil.item_plan(rgb_p))
        assert lab is None and lab_p is None and img.shape == (1, 3, 40, 56) and (img == img_p).all()
    val = CrossCity_Dataset(args, split="val", training=True, class_13=True, **paths)
    assert not val.is_train() and len(val) == 2
    assert val.paths(1) == (os.path.join(root, "Images", "Test", "pano_test_001.jpg"),
                            os.path.join(root, "Labels", "Test", "pano_test_001_eval.png"), 1)
    for item, (data, ids) in enumerate(made["test"]):
        rgb, got_ids = val.decode(item)
        assert np.array_equal(got_ids, ids)
        img, lab = val.host_transform(rgb, got_ids, val.item_plan(rgb))
        assert np.array_equal(lab[0].numpy(), lut[ids].astype(np.int64)) and int(lab.max()) <= 12
    with pytest.raises(Warning, match="train/val"):
        CrossCity_Dataset(args, split="test", **paths)
    ld = build_loader("crosscity", _args(), True, paths)
    assert isinstance(ld, CrossCity_DataLoader) and (ld.num_iterations, ld.valid_iterations) == (3, 2)
    assert ld.data_loader.dataset.class_13 and ld.val_loader.dataset.split == "val" and ld.data_loader.shuffle
    ld.close()


def test_label_of_another_size_raises(tmp_path):
    pytest.importorskip("PIL")
    from PIL import Image
    from maxsquareloss_amd.datasets import CrossCity_Dataset
    from maxsquareloss_amd.hip import MSLError
    paths, _ = jpeg_ref.nthu_tree(tmp_path / "N", n=1, val_n=2)
    Image.fromarray(np.zeros((40, 55), np.uint8)).save(os.path.join(paths["gt_path"], "pano_test_001_eval.png"))
    ds = CrossCity_Dataset(_args(), split="val", training=False, **paths)
    ds.decode(0)
    with pytest.raises(MSLError, match="does not match its image"):
        ds.decode(1)


@pytest.mark.parametrize("workers", [1, 4])
def test_draws_do_not_depend_on_worker_count(tmp_path, workers):
    pytest.importorskip("PIL")
    from maxsquareloss_amd.datasets import CrossCity_DataLoader
    from maxsquareloss_amd.utils import jpeg
    paths, made = jpeg_ref.nthu_tree(tmp_path / "N", n=7, val_n=1)

    def epoch_plans(n_workers, mode):
        ld = CrossCity_DataLoader(_args(data_loader_workers=n_workers, seed=11, jpeg_decode=mode), training=True,
                                  datasets_path=paths)
        got = []
        for _ in range(2):
            for rgb, ids, plan, ident, _ in ld.data_loader.host_items():
                assert ids is None and jpeg.is_payload(rgb) == (mode == "device")
                if mode == "device":
                    assert np.array_equal(jpeg.reconstruct(rgb), jpeg_ref.pillow_rgb(made["train"][ident][0]))
                got.append((ident, plan[:2]))
        ld.close()
        return got

    base = epoch_plans(0, "device")
    assert sorted(i for i, _ in base[:7]) == list(range(7)) and [i for i, _ in base[:7]] != [i for i, _ in base[7:]]
    assert len({p[0] for _, p in base}) == 2
    assert epoch_plans(workers, "device") == base and epoch_plans(workers, "pillow") == base


def test_client_dataset_takes_jpegs(tmp_path):
    pytest.importorskip("PIL")
    from maxsquareloss_amd.datasets import Client_dataset
    from maxsquareloss_amd.utils import jpeg
    data = jpeg_ref.encode(jpeg_ref.photo(24, 40), 2, quality=85)
    (tmp_path / "a.jpg").write_bytes(data)
    (tmp_path / "b.JPEG").write_bytes(data)
    (tmp_path / "test.txt").write_text(f"{tmp_path / 'a.jpg'}\n{tmp_path / 'b.JPEG'}\n")
    for mode in ("device", "pillow"):
        ds = Client_dataset({"list_path": str(tmp_path)}, argparse.Namespace(resize=False, seg_size=(40, 24),
                                                                              jpeg_decode=mode))
        for item in range(2):
            rgb, ids = ds.decode(item)
            assert ids is None and jpeg.is_payload(rgb) == (mode == "device")
            plan = ds.item_plan(rgb)
            assert plan[:2] == (False, [((40, 24), None)]) and len(plan) == (3 if mode == "device" else 2)
            if mode == "device":
                assert np.array_equal(jpeg.reconstruct(rgb), jpeg_ref.pillow_rgb(data))


def test_missing_tree_says_what_is_expected(tmp_path):
    from maxsquareloss_amd.datasets import build_loader
    from maxsquareloss_amd.hip import MSLError
    os.makedirs(tmp_path / "Rome" / "Images" / "Train")
    paths = {"data_root_path": str(tmp_path / "Rome"), "list_path": str(tmp_path / "Rome" / "List"), "gt_path": None}
    with pytest.raises(MSLError) as e:
        build_loader("crosscity", argparse.Namespace(), True, paths)
    msg = str(e.value)
    assert "Images/Test" in msg and "Labels/Test" in msg and "the list folder" in msg and "{id}_eval.png" in msg
    assert "Images/Train is" not in msg and os.path.join("Images", "Train") + "," not in msg   # only what is missing
    with pytest.raises(MSLError, match="crosscity"):
        build_loader("nthu", argparse.Namespace(), True, paths)


def test_trainer_flags_and_paths():
    from maxsquareloss_amd.tools import solve_crosscity, train_source
    a = solve_crosscity.build_parser().parse_args([])
    assert (a.source_dataset, a.city_name, a.num_classes, a.jpeg_decode, a.epoch_num) == ("cityscapes", "Rome", 13,
                                                                                          "device", 10)
    assert (a.lambda_target, a.threshold, a.target_mode, a.graph, a.pair) == (0.1, 0.98, "maxsquare", False, True)
    with pytest.raises(SystemExit):
        solve_crosscity.build_parser().parse_args(["--city_name", "Paris"])
    with pytest.raises(SystemExit):
        solve_crosscity.build_parser().parse_args(["--jpeg_decode", "cpu"])
    assert train_source.dataset_paths("crosscity", "/d/Rome", "/l")["gt_path"] == "/d/Rome/Labels/Test"
    assert issubclass(solve_crosscity.CrossCityTrainer, __import__(
        "maxsquareloss_amd.tools.solve_gta5", fromlist=["UDATrainer"]).UDATrainer)
    # the other trainers' flags are as they were
    from maxsquareloss_amd.tools import solve_gta5
    b = solve_gta5.build_parser().parse_args([])
    assert (b.source_dataset, b.num_classes, b.lambda_target, b.threshold, b.jpeg_decode) == ("gta5", 19, 1, 0.95, "device")


# ------------------------------------------------------------------------------------ C ABI
def test_header_signatures_and_exports():
    from maxsquareloss_amd import hip
    text = open(os.path.join(ROOT, "include", "msl_hip.h")).read()
    flat = " ".join(text.split())
    for decl in ("int msl_jpeg_info(const uint8_t* file, size_t n, msl_jpeg_header* header);",
                 "size_t msl_jpeg_coef_elems(const msl_jpeg_header* header);",
                 "int msl_jpeg_entropy_decode(const uint8_t* file, size_t n, msl_jpeg_header* header, int16_t* coef, "
                 "size_t coef_elems, uint16_t* quant);",
                 "size_t msl_jpeg_workspace(const msl_jpeg_header* header);",
                 "int msl_jpeg_reconstruct(const int16_t* coef, const uint16_t* quant, const msl_jpeg_header* header, "
                 "uint8_t* rgb, void* ws, size_t ws_bytes, msl_stream_t stream);",
                 "int msl_jpeg_tile_blocks(void);", "int msl_jpeg_tile_pixels(void);"):
        assert decl in flat, decl
    names = ["msl_jpeg_info", "msl_jpeg_coef_elems", "msl_jpeg_entropy_decode", "msl_jpeg_workspace",
             "msl_jpeg_reconstruct", "msl_jpeg_tile_blocks", "msl_jpeg_tile_pixels"]
    lib = hip.load(require_gpu=False)
    for name in names:
        assert name in hip.SIGNATURES and hasattr(lib, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], capture_output=True, text=True).stdout
    assert set(names) <= set(re.findall(r" T (msl_\w+)", out))
    assert lib.msl_abi_version() == 3 and hip.ABI_VERSION == 3
    assert ctypes.sizeof(hip.JpegHeader) == 8 * 4 + 3 * 32 and ctypes.sizeof(hip.JpegComp) == 32
    assert lib.msl_jpeg_tile_blocks() == 32 and lib.msl_jpeg_tile_pixels() % 256 == 0
    assert "jpeg.hip" in open(os.path.join(ROOT, "maxsquareloss_amd", "csrc", "Makefile")).read()


def test_reconstruct_checks_its_arguments_before_any_launch():
    """The checks answer without a GPU: nothing is launched."""
    pytest.importorskip("PIL")
    from maxsquareloss_amd import hip
    from maxsquareloss_amd.utils import jpeg
    lib = hip.load(require_gpu=False)
    _, h = jpeg.info(jpeg_ref.encode(jpeg_ref.photo(20, 30), 2, quality=70))
    hp = ctypes.addressof(h)
    ws = lib.msl_jpeg_workspace(hp)
    assert ws == 32 * 32 + 2 * 256 and lib.msl_jpeg_coef_elems(hp) == (16 + 4 + 4) * 64
    buf = (ctypes.c_uint8 * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    good = [p, p, hp, p, p, ws, None]
    for k in (0, 1, 2, 3, 4):
        bad = list(good)
        bad[k] = None
        assert lib.msl_jpeg_reconstruct(*bad) == ERR_ARG, k
    assert lib.msl_jpeg_reconstruct(p, p, hp, p, p, ws - 1, None) == ERR_ARG          # a short workspace
    assert lib.msl_jpeg_reconstruct(p + 2, p, hp, p, p, ws, None) == ERR_ARG          # misaligned coefficients
    for field, value in (("width", 33), ("height", 40), ("ncomp", 2), ("hmax", 1), ("mcus_w", 3)):
        h2 = hip.JpegHeader.from_buffer_copy(bytes(h))
        setattr(h2, field, value)
        assert lib.msl_jpeg_reconstruct(p, p, ctypes.addressof(h2), p, p, 1 << 20, None) == ERR_ARG, field
        assert lib.msl_jpeg_workspace(ctypes.addressof(h2)) == 0 and lib.msl_jpeg_coef_elems(ctypes.addressof(h2)) == 0
    for field, value in (("blocks_w", 5), ("blocks_h", 1), ("offset", 64), ("tq", 4), ("h", 1)):
        h2 = hip.JpegHeader.from_buffer_copy(bytes(h))
        setattr(h2.comp[1 if field != "h" else 0], field, value)
        assert lib.msl_jpeg_reconstruct(p, p, ctypes.addressof(h2), p, p, 1 << 20, None) == ERR_ARG, field


def test_jpeg_kernels_use_no_scratch():
    path = os.path.join(ROOT, "maxsquareloss_amd", "_lib", "obj", "jpeg.o.remarks")
    assert os.path.exists(path), "no resource report: the build (__graft_entry__.build()) writes it beside jpeg.o"
    text = open(path).read()
    names = re.findall(r"remark: Function Name: (\S+)", text)
    assert len(names) == 2 and "k_jpeg_idct" in names[0] + names[1] and "k_jpeg_rgb" in names[0] + names[1]
    assert [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)] == [0, 0]
    assert [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", text)] == [0, 0]
