"""The coverage gate of the forward-form conv kernels (CPU only: msl_conv_fwd_plan launches nothing).

plan_fwd / plan_sk (csrc/dconv.hip) send every forward and data-gradient conv GEMM to one instantiation of
the stream-K kernel and one schedule.  This module plans a committed grid of calls (conv_form_cases.grid)
through the library itself and holds tests/conv_form_cases.py TABLE - the cases test_gpu_conv_forms.py
compares with fp64 - against it: a plan edit that sends some shape to a kernel or schedule no case runs fails
here, before any GPU is involved.
"""
import ctypes
import itertools

import pytest

import conv_form_cases as cf
from maxsquareloss_amd import hip

# The refused calls of the grid (MSL_ERR_SHAPE): the split-K tile kernel (M <= 32 with an odd K-step count)
# has no bf16 form and no accumulate epilogue.  (family, entry) of every refusal; none runs stream-K.
REFUSED = {
    ("bf16", "dconv_fwd"), ("bf16", "dconv_dgrad"), ("bf16", "pconv_fwd"), ("bf16", "pconv_dgrad"),
    ("fp32", "pconv_dgrad_acc"), ("fp32", "pconv_dgrad_resmask"), ("fp16", "pconv_dgrad_acc"),
    ("fp16", "pconv_dgrad_resmask"),
}


@pytest.fixture(scope="module")
def swept():
    return cf.reached(hip, cf.grid())


def test_every_reachable_kernel_and_schedule_has_a_case(swept):
    found, _ = swept
    need = {kc for kc in found if kc[1] in cf.CLASSES}
    have = {(k, c) for k, c, _ in cf.TABLE}
    missing = sorted(need - have)
    hint = ["%s %s: e.g. %s" % (k, c, tuple(cf.suggest(found, k, c))) for k, c in missing]
    assert not missing, "reachable (kernel, schedule) pairs without a numeric case:\n" + "\n".join(hint)
    assert {c for _, c in need} == set(cf.CLASSES)  # the grid itself reaches every class, both tile ones too
    print("%d (kernel, schedule) pairs reachable on the grid, all with a case" % len(need))


def test_every_built_kernel_is_reached(swept):
    """The table holds only launchable rows: the grid reaches every one through an entry point."""
    found, _ = swept
    keys = cf.all_form_keys(hip)
    assert len(set(keys)) == len(keys)
    hit = {k for k, _ in found} - {"tile"}  # ("tile": the split-K tile kernel, no row of the table)
    assert set(keys) == hit
    # Every argument plan_fwd can be given (accumulate on every geometry and family).  No entry point passes
    # accumulate to the bf16 family or to a 3x3 conv; there plan_fwd names a form that is not built - accumulate in
    # the bf16 math, or on a 128-row f16x3 / fp16 tile that is not pointwise - and the call is refused
    raw, unbuilt = set(), set()
    for (fam, form), taps, acc, hyb in itertools.product((("fp32", "mfma_f32"), ("fp32", "bf16x6"), ("fp32", "f16x3"),
                                                         ("bf16", "f16x3"), ("fp16", "f16x3")), (9, 1), (0, 1), (1, 0)):
        forms = hip.Forms(cf.F32_FORMS[form], hyb, 1, 1)
        for nb, cimg, m, (n, h, w) in itertools.product((1, 2) if taps == 9 else (1,), cf.GRID_CIMG, cf.GRID_M,
                                                        cf.GRID_PIXELS):
            pl = hip.conv_fwd_plan(cf.FAMILIES[fam], nb, taps, cimg, m, n * h * w, acc, 2 if taps == 9 else 0, forms_=forms)
            if not pl.stream_k:  # the split-K tile kernel: test_refusals_are_the_pinned_ones
                assert pl.row == -1 and pl.status == (cf.MSL_ERR_SHAPE if acc or fam == "bf16" else cf.MSL_OK)
            elif acc and (fam == "bf16" or (taps == 9 and m > 64 and form == "f16x3")):
                assert (pl.status, pl.row, pl.stream_k) == (cf.MSL_ERR_SHAPE, -1, 1), (fam, form, taps, cimg, m)
                unbuilt.add((fam, cf.MATHS[pl.math]))
            else:
                assert pl.status == cf.MSL_OK and pl.row >= 0, (fam, form, taps, acc, cimg, m)
                raw.add(keys[pl.row])
    assert raw == set(keys)
    assert unbuilt == {("bf16", "bf16"), ("fp32", "h3p"), ("fp16", "h1p")}


def test_refusals_are_the_pinned_ones(swept):
    _, refused = swept
    assert {(c.family, c.entry) for c, _ in refused} == REFUSED
    for c, pl in refused:
        assert pl.status == cf.MSL_ERR_SHAPE and not pl.stream_k and pl.row == -1, c
        assert c.family == "bf16" or cf.ENTRIES[c.entry][2], c


def test_plans_are_consistent_with_their_kernel(swept):
    """What the query reports of a plan agrees with the instantiation it names."""
    found, _ = swept
    lib = hip.load(require_gpu=False)
    f = hip.ConvForm()
    for (key, cls), cases in found.items():
        for c in cases[:: max(1, len(cases) // 50)]:
            pl = cf.plan_of(hip, c)
            _, nb, taps, cimg, m, p, acc, _ = cf.plan_args(c)
            assert pl.ksteps == nb * taps * -(-cimg // 16) and pl.tiles_n == -(-p // 128)
            if not pl.stream_k:
                assert pl.row == -1 and pl.math == 0 and m <= 32 and pl.ksteps % 2 == 1
                assert pl.tiles_m == 1 and pl.S == -(-pl.ksteps // pl.kps) and pl.reduce == (pl.S > 1)
                assert (pl.tdp, pl.NW, pl.T, pl.split_img) == (0, 0, 0, 0)
                continue
            assert lib.msl_conv_fwd_form_describe(pl.row, ctypes.addressof(f)) == cf.MSL_OK
            assert (f.math, f.acc, pl.split_img) == (pl.math, acc, int(f.bform == 2))
            assert pl.tiles_m == -(-m // f.bm) and pl.kps * f.G == pl.ksteps and pl.S == 1
            tiles = pl.tiles_m * pl.tiles_n
            assert pl.tdp % 512 == 0 and pl.tdp <= tiles and pl.T == (tiles - pl.tdp) * pl.kps
            assert pl.reduce == (pl.T > 0) and pl.NW <= min(512, max(pl.T, 1))
            if not c.sk_hybrid:
                assert pl.tdp == 0


@pytest.mark.parametrize("key,cls,case", cf.TABLE, ids=[str(i) for i in range(len(cf.TABLE))])
def test_table_case_lands_where_it_is_filed(key, cls, case):
    assert cf.entry_exists(case.entry, case.family) and cf.family_runs(case.family, case.f32_form)
    pl = cf.plan_of(hip, case)
    assert pl.status == cf.MSL_OK
    assert ((cf.form_key(hip, pl.row) if pl.stream_k else "tile"), cf.schedule_class(pl)) == (key, cls)
    assert cf.macs(case) <= cf.CASE_MAX_MACS
    if case.entry == "pconv_dgrad_resmask":
        assert (case.h * case.w) % 64 != 0


def test_table_has_no_duplicates():
    cases = [c for _, _, c in cf.TABLE]
    assert len(set(cases)) == len(cases)


def test_form_describe_and_bad_arguments():
    lib = hip.load(require_gpu=False)
    n = lib.msl_conv_fwd_form_count()
    f = hip.ConvForm()
    seen = set()
    for row in range(n):
        assert lib.msl_conv_fwd_form_describe(row, ctypes.addressof(f)) == cf.MSL_OK
        assert f.bm in (32, 64, 128, 256) and f.math in cf.MATHS and f.bform in cf.BFORMS
        seen.add(tuple(getattr(f, name) for name, _ in f._fields_))
    assert len(seen) == n == 39
    for row in (-1, n, n + 1000):
        assert lib.msl_conv_fwd_form_describe(row, ctypes.addressof(f)) == cf.MSL_ERR_ARG
    assert lib.msl_conv_fwd_form_describe(0, None) == cf.MSL_ERR_ARG
    out = hip.ConvFwdPlan()
    ok = dict(family=0, nbranch=1, taps=9, cimg=80, M=67, P=1675, accumulate=0, dil0=2)
    forms = {name: hip.Forms(v, 1, 1, 1) for name, v in cf.F32_FORMS.items()}

    def plan(fm=forms["f16x3"], o=out, **kw):
        a = dict(ok, **kw)
        return lib.msl_conv_fwd_plan(a["family"], a["nbranch"], a["taps"], a["cimg"], a["M"], a["P"], a["accumulate"],
                                     a["dil0"], None if fm is None else ctypes.addressof(fm),
                                     None if o is None else ctypes.addressof(o))

    assert plan() == cf.MSL_OK and plan(fm=None) == cf.MSL_OK  # NULL forms: the defaults
    bad = [dict(family=-1), dict(family=3), dict(nbranch=0), dict(nbranch=3), dict(taps=3), dict(cimg=0), dict(M=0),
           dict(P=0), dict(P=2 ** 30 + 1), dict(dil0=0), dict(taps=1, dil0=1), dict(taps=1, dil0=0, nbranch=2)]
    for kw in bad:
        assert plan(**kw) == cf.MSL_ERR_ARG, kw
    assert plan(o=None) == cf.MSL_ERR_ARG
    assert plan(fm=hip.Forms(1, 1, 1, 1)) == cf.MSL_ERR_ARG  # no such f32_form
    for name in ("mfma_f32", "bf16x6"):  # the fp16 family reads the f16x3 packs
        assert plan(fm=forms[name], family=2) == cf.MSL_ERR_ARG
        assert plan(fm=forms[name], family=1) == cf.MSL_OK
    assert plan(taps=1, dil0=0) == cf.MSL_OK
