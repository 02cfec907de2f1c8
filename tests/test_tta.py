"""CPU: the host side of multi-scale test-time augmentation (--scales): the C ABI of msl_predict_tta /
msl_predict_tta_images / msl_resize_bilinear and their refusals, the flag's parsing, the torch-CPU restatement
(tests/tta_ref.py) against the same rule in fp64, and the conv plans of every size the default scales reach.

Nothing here launches a kernel: the entry points are called with arguments they must refuse before any launch.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import conv_form_cases as cf
import evaluate_ref as er
import tta_ref as tr
from maxsquareloss_amd import hip
from maxsquareloss_amd.hip import MSLError
from maxsquareloss_amd.utils import validate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK_PTR = 0x1000  # never dereferenced: the checks refuse the call before any launch
ERR_ARG = -3
NEW_SYMBOLS = ("msl_predict_tta_max_entries", "msl_predict_tta", "msl_predict_tta_images", "msl_resize_bilinear")


# ------------------------------------------------------------------------------------------ the C ABI
def test_header_signatures_and_library_agree_on_the_entry_points():
    src = open(os.path.join(ROOT, "include", "msl_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = hip.load(require_gpu=False)
    out = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (msl_\w+)", out))
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, code), s
        assert s in hip.SIGNATURES and hasattr(lib, s) and s in exported, s
    struct = re.search(r"typedef struct msl_tta_entry \{(.*?)\} msl_tta_entry;", code, flags=re.S)
    assert struct and re.sub(r"\s+", " ", struct.group(1)).strip() == "const float* logits; int hi, wi, mirror;"
    assert [n for n, _ in hip.TtaEntry._fields_] == ["logits", "hi", "wi", "mirror"]
    assert ctypes.sizeof(hip.TtaEntry) == 24  # pointer, three ints, padded to the pointer's alignment
    assert hip.ABI_VERSION == 3 and lib.msl_abi_version() == 3
    assert lib.msl_predict_tta_max_entries() == 16


def _table(*ents):
    t = (hip.TtaEntry * max(1, len(ents)))()
    for k, e in enumerate(ents):
        t[k] = hip.TtaEntry(*e)
    return t


GOOD = (OK_PTR, 9, 17, 0)


def _tta(entries=None, n=None, c=19, ho=33, wo=65, label=OK_PTR, cm=OK_PTR, arg=OK_PTR, null_table=False):
    entries = [GOOD, (OK_PTR, 5, 9, 1)] if entries is None else entries
    t = None if null_table else _table(*entries)
    return hip.load(require_gpu=False).msl_predict_tta(t, len(entries) if n is None else n, c, ho, wo, label, cm, arg,
                                                       None)


def _img(entries=None, n=None, c=19, ho=33, wo=65, label=OK_PTR, cm=OK_PTR, thr=0.95, id_lut=OK_PTR, pal=OK_PTR,
         shade=OK_PTR, outs=(OK_PTR,) * 5, null_table=False):
    entries = [GOOD, (OK_PTR, 5, 9, 1)] if entries is None else entries
    t = None if null_table else _table(*entries)
    return hip.load(require_gpu=False).msl_predict_tta_images(t, len(entries) if n is None else n, c, ho, wo, label, cm,
                                                              thr, id_lut, pal, shade, *outs, None)


BAD_COMMON = [
    dict(null_table=True),
    dict(n=0), dict(n=-1), dict(entries=[GOOD] * 16, n=17),
    dict(entries=[GOOD, (None, 9, 17, 0)]), dict(entries=[(OK_PTR, 0, 17, 0)]), dict(entries=[GOOD, (OK_PTR, 9, 0, 1)]),
    dict(entries=[(OK_PTR, -2, 17, 0)]), dict(entries=[GOOD, (OK_PTR, 9, 17, 2)]), dict(entries=[(OK_PTR, 9, 17, -1)]),
    dict(c=0), dict(c=33), dict(c=-4),
    dict(ho=0), dict(wo=0), dict(ho=-1), dict(ho=46341, wo=46341), dict(ho=1 << 16, wo=1 << 15),
    dict(label=None), dict(cm=None),
]


@pytest.mark.parametrize("kw", BAD_COMMON, ids=lambda kw: ",".join(sorted(kw)))
def test_predict_tta_refuses_before_any_launch(kw):
    assert _tta(**kw) == ERR_ARG
    assert _img(**kw) == ERR_ARG


def test_predict_tta_refuses_a_call_without_output_or_table():
    assert _tta(label=None, cm=None, arg=None) == ERR_ARG
    assert _img(label=None, cm=None, outs=(None,) * 5) == ERR_ARG
    some = (OK_PTR,) * 5
    assert _img(id_lut=None, outs=some) == ERR_ARG   # ids_out without its table
    assert _img(pal=None, outs=some) == ERR_ARG      # color_out
    assert _img(shade=None, outs=some) == ERR_ARG    # conf_out


def test_resize_bilinear_refuses_before_any_launch():
    f = hip.load(require_gpu=False).msl_resize_bilinear
    ok = OK_PTR
    assert f(None, ok, 3, 8, 8, 4, 4, None) == ERR_ARG and f(ok, None, 3, 8, 8, 4, 4, None) == ERR_ARG
    for c, hi, wi, ho, wo in ((0, 8, 8, 4, 4), (5, 8, 8, 4, 4), (3, 0, 8, 4, 4), (3, 8, 0, 4, 4), (3, 8, 8, 0, 4),
                              (3, 8, 8, 4, 0), (4, 8, 8, 1 << 15, 1 << 14)):
        assert f(ok, ok, c, hi, wi, ho, wo, None) == ERR_ARG, (c, hi, wi, ho, wo)


def test_fusion_kernels_use_no_scratch():
    """The compiler's resource report of the last build (Makefile: predict.o.remarks, and loss.o.remarks for
    k_resize_four): the by-value entry table, indexed with the loop variable, puts nothing in scratch and nothing
    spills, in any instantiation."""
    paths = [os.path.join(ROOT, "maxsquareloss_amd", "_lib", "obj", o + ".remarks") for o in ("predict.o", "loss.o")]
    if not all(os.path.exists(p) for p in paths):
        pytest.skip("no resource report: build the library first (__graft_entry__.build())")
    kern, info = None, {}
    for line in (line for p in paths for line in open(p)):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            kern = m.group(1)
            info[kern] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill): (\d+)", line)
        if m and kern:
            info[kern][m.group(1)] = int(m.group(2))
    for stem, count in (("k_predict_ttaI", 4), ("k_predict_tta_imagesI", 4), ("k_resize_four", 1)):  # C in {19, 16, 13, 32}
        ks = [k for k in info if stem in k]
        assert len(ks) == count, (stem, ks)
        for k in ks:
            assert info[k]["ScratchSize [bytes/lane]"] == 0 and info[k]["VGPRs Spill"] == 0, (k, info[k])
            print(k, info[k])


# ------------------------------------------------------------------------------------------ the flag
def test_size_at_rounds_half_up():
    table = {(65, 0.5): 33, (128, 0.75): 96, (128, 1.25): 160, (512, 0.75): 384, (1024, 1.25): 1280, (7, 0.5): 4,
             (5, 0.5): 3, (3, 0.25): 1, (1, 0.25): 1, (2, 0.25): 1, (513, 1.0): 513, (33, 1.5): 50, (31, 1.5): 47}
    for (n, s), want in table.items():
        assert validate.size_at(n, s) == want == tr.size_at(n, s), (n, s)


def test_scales_parse():
    assert validate.parse_scales("1.0") == validate.SINGLE_SCALE == (1.0,)
    assert validate.parse_scales("0.75,1.0,1.25") == (0.75, 1.0, 1.25)
    assert validate.parse_scales(" 1.25, 0.5 ") == (1.25, 0.5)  # the order given
    assert validate.parse_scales((0.5, 1, 2)) == (0.5, 1.0, 2.0)
    eight = "0.25,0.5,0.75,1.0,1.25,1.5,1.75,2.0"
    assert len(validate.parse_scales(eight, flip=True)) == 8  # 16 entries: the launch's limit
    for bad, word in (("", "''"), ("0.2", "0.2"), ("2.01", "2.01"), ("1.0,abc", "abc"), ("0.5,1.0,0.5", "0.5"),
                      ("1,1.0", "1.0"), ("nan", "nan"), ("-1", "-1"), (eight + ",1.1", "9"), ("0.5,,1", "''")):
        with pytest.raises(MSLError) as e:
            validate.parse_scales(bad)
        assert word in str(e.value), (bad, str(e.value))
    with pytest.raises(MSLError):
        validate.parse_scales(())


def test_tools_take_the_flag():
    from maxsquareloss_amd.tools import evaluate, predict
    for tool in (evaluate, predict):
        p = tool.build_parser()
        assert p.parse_args([]).scales == (1.0,)
        assert p.parse_args(["--scales", "0.75,1.0,1.25", "--flip", "True"]).scales == (0.75, 1.0, 1.25)
        for bad in ("3.0", "1.0,1.0", "x"):
            with pytest.raises(SystemExit):
                p.parse_args(["--scales", bad])


def test_validator_takes_scales_without_a_gpu():
    v = validate.Validator(None, 19, (8, 16), 1, "cpu", flip=True, scales=(0.5, 1.0))
    assert v.scales == (0.5, 1.0)
    assert validate.Validator(None, 19, (8, 16), 1, "cpu").scales == (1.0,)
    with pytest.raises(MSLError):
        validate.Validator(None, 19, (8, 16), 1, "cpu", scales=(0.5, 0.5))


# ------------------------------------------------------------------------------------------ the restatement
NEAR_COUNT = [0, 0, 0, 2, 110]  # near-tie pixels of each case, measured with this restatement on the CPU


@pytest.mark.parametrize("index", range(len(tr.CASES)), ids=tr.IDS)
def test_restatement_against_fp64(index):
    """The fp32 restatement and the same rule in fp64 choose the same class wherever the top-2 gap is clear;
    the near-tie share stays under the evaluator tests' cap."""
    case = tr.CASES[index]
    cls, near, top2 = tr.case_ref(index)
    cls64, _, _ = tr.tta_ref(tr.entries(case), case[2], torch.float64)
    share = near.mean()
    differ = cls != cls64
    print("case %s: %d near-tie pixels of %d (share %.2e), fp32 and fp64 differ at %d" %
          (tr.IDS[index], near.sum(), near.size, share, differ.sum()))
    assert share <= 1e-3
    assert not (differ & ~near).any()
    assert near.sum() == NEAR_COUNT[index]
    n = len(tr.entries(case))
    assert n == len(case[1]) * (2 if case[3] else 1) and cls.shape == (case[2][0] * case[2][1],)
    assert np.array_equal(top2[0], cls)


def test_two_entries_restate_the_flip_rule():
    C, hi, wi, ho, wo = er.SHAPES[0]
    low, lowf = er.logits(C, hi, wi, "L"), er.logits(C, hi, wi, "F")
    cls, near, _ = er.predict_ref(low, (ho, wo), lowf)
    mine, mnear, _ = tr.tta_ref([(low, 0), (lowf, 1)], (ho, wo))
    assert np.array_equal(cls, mine) and np.array_equal(near, mnear)


# ------------------------------------------------------------------------------------------ the plan gate
def eval_conv_cases(h, w, nimg, family, num_classes=19):
    """Every conv GEMM of the eval forward of one H x W image (nimg = 2: a flip pair) as conv_form_cases Cases,
    by the dispatch of ops.py: the stem as im2col + the pointwise GEMM (fp32 under every family), 1x1 convs on
    the pointwise GEMM, the bottlenecks' 3x3 on the dilated GEMM and each ASPP head as one pointwise GEMM with
    18 * C rows (ASPP_FORM "shift")."""
    from oracle import msl_oracle as orc
    sh, sw = (h + 6 - 7) // 2 + 1, (w + 6 - 7) // 2 + 1
    stem_family = "fp32" if family in ("bf16", "fp16") else family
    cases = [cf.Case("pconv_fwd", stem_family, "f16x3", 1, 1, 147, 64, sh, sw, nimg, 0, 0)]
    dil = {64: 1, 128: 1, 256: 2, 512: 4}
    heads = {}
    for cin, cout, k, ho, wo in orc.conv_calls(h, w, num_classes):
        if k == 1:
            cases.append(cf.Case("pconv_fwd", family, "f16x3", 1, 1, cin, cout, ho, wo, nimg, 0, 0))
        elif cout == num_classes and cin in (1024, 2048):
            heads[cin] = (ho, wo)
        else:
            assert k == 3 and cin == cout
            cases.append(cf.Case("dconv_fwd", family, "f16x3", 1, 1, cin, cout, ho, wo, nimg, dil[cin], 0))
    assert sorted(heads) == [1024, 2048]
    for cin, (ho, wo) in heads.items():
        cases.append(cf.Case("pconv_fwd", family, "f16x3", 1, 1, cin, 18 * num_classes, ho, wo, nimg, 0, 0))
    return cases


@pytest.mark.parametrize("family", ["fp32", "fp16"])
@pytest.mark.parametrize("w,h", [(192, 96), (320, 160), (768, 384), (1280, 640), (1536, 768), (2560, 1280)])
def test_every_conv_call_of_a_scaled_forward_lands_on_a_kernel_held_to_fp64(family, w, h):
    """Every conv call of the eval forward at the sizes --scales reaches (0.75 / 1.25 of 128 x 256 and of
    1024 x 512, 0.75 / 1.25 of 2048 x 1024), as one image and as a flip pair: planned with MSL_OK onto a
    (kernel, schedule class) conv_form_cases.TABLE has a case of, or onto a flat schedule."""
    table = {(k, c) for k, c, _ in cf.TABLE}
    keys = cf.all_form_keys(hip)
    n = 0
    for nimg in (1, 2):
        for case in eval_conv_cases(h, w, nimg, family):
            pl = cf.plan_of(hip, case)
            assert pl.status == cf.MSL_OK, (case, pl.status)
            cls = cf.schedule_class(pl)
            key = keys[pl.row] if pl.stream_k else "tile"
            assert cls == "flat" or (key, cls) in table, (case, key, cls)
            n += 1
    assert n == 2 * (1 + 103 + 2)  # the stem, 33 bottlenecks of three convs and four downsamples, two heads
