"""The coverage gate of the weight-gradient conv kernels (CPU only: msl_conv_wgrad_plan launches nothing).

plan_wgrad / plan_chunks / wgrad_swaps / wgrad_reduce (csrc/dconv.hip) send every weight-gradient conv GEMM to one
GEMM instantiation, one schedule and one piece reduce.  This module plans a committed grid of calls
(conv_wgrad_cases.grid) through the library itself - msl_conv_wgrad_plan calls the functions launch_wgrad calls -
and holds tests/conv_wgrad_cases.py TABLE and EDGES, the cases test_gpu_conv_wgrad_forms.py compares with fp64,
against it: a plan edit that sends some shape to a kernel, reduce or schedule no case runs fails here, before any
GPU is involved.
"""
import ctypes
import itertools

import pytest

import conv_wgrad_cases as cw
from maxsquareloss_amd import hip

# Every GEMM instantiation and every piece reduce launch_wgrad names is reached by the grid (ten and five): nothing
# is pinned as unreachable.  Should a plan edit strand one, it goes here with the reason.
UNREACHED_GEMMS = set()
UNREACHED_REDUCES = set()
ALL_GEMMS = {"x6.x6", "x6.h3p", "x6.h1p", "sk128x128.f32", "sk128x128.bf16", "sk128x128.x6", "sk64x64.f32",
             "sk64x64.bf16", "sk32x128.f32", "sk32x128.bf16"}
# k_wgrad_x6's scalar mask cursor (a run of more than kWxMaskTab - 3 = 2045 K-steps) IS reachable under the guards of
# launch_wgrad: plan_chunks bounds the items (tiles x chunks <= 4096), not the chunk length, so a plan of few chunks
# on many pixels has chunks that long (72 tiles x 7 chunks of 2049 K-steps at 229 414 pixels;
# test_scalar_cursor_is_reachable_only_above_the_cap).  On the sweep the long runs are all chunked, never stream-K
# ranges.  A run that long is 32 736 pixels of one tile, a chunked plan has at least 0.75 * 512 items, and a tile of
# k_wgrad_x6 (>= 128 channels a side) holds on average more than 64 x 64 channel pairs: over 5e10 MACs, thirty times
# CASE_MAX_MACS.  No grid point (<= 20 000 pixels) gets there; EDGES carries the one case, over the cap.
SCALAR_CURSOR_MIN_PIXELS = (cw.kWxMaskTab - 2) * 16 - 15
# The refused calls of the grid (MSL_ERR_SHAPE): the two-branch 515 -> 515 3x3 gradient on k_wgrad_x6's chunked plan
# from 19 881 pixels - T * NW >= 2^31 with NW = 450 tiles x 9 chunks (the guard of the stream-K index arithmetic).
REFUSED = {(2, 9, 515, 515, 1, 141, 141), (2, 9, 515, 515, 2, 100, 100)}


@pytest.fixture(scope="module")
def swept():
    return cw.reached(hip, cw.grid())


def _gemm(key):
    return key.split("/")[0]


def test_every_reachable_key_and_class_has_a_case(swept):
    found, _, _ = swept
    keys = {k for k, _ in found}
    need = {kc for kc in found if kc[1] in cw.CLASSES}
    need |= {(k, "flat") for k in keys if not any((k, c) in found for c in cw.CLASSES)}  # reachable only as flat
    have = {(k, c) for k, c, _ in cw.ALL_CASES}
    missing = sorted(need - have)
    hint = ["%s %s: e.g. %s" % (k, c, tuple(cw.suggest(hip, found[(k, c)]))) for k, c in missing]
    assert not missing, "reachable (key, class) pairs without a numeric case:\n" + "\n".join(hint)
    assert {c for _, c in need} == set(cw.CLASSES) | {"flat"}
    print("%d keys, %d (key, class) pairs needing a case on the grid (%d with flat), all with one" % (
        len(keys), len(need), len(found)))


def test_every_key_has_a_case_in_each_swizzle_state(swept):
    _, swz, _ = swept
    have = set()
    for key, _, c in cw.ALL_CASES:
        have.add((key, cw.plan_of(hip, c).swizzle))
    missing = sorted(set(swz) - have)
    hint = ["%s swizzle %d: e.g. %s" % (k, s, tuple(cw.suggest(hip, swz[(k, s)]))) for k, s in missing]
    assert not missing, "reachable (key, worker swizzle) states without a numeric case:\n" + "\n".join(hint)


def test_unreached_kernels_are_the_pinned_ones(swept):
    found, _, _ = swept
    keys = {k for k, _ in found}
    assert ALL_GEMMS - {_gemm(k) for k in keys} == UNREACHED_GEMMS
    assert set(cw.REDUCES.values()) - {k.split("/")[1] for k in keys} == UNREACHED_REDUCES
    # the transposed tiles: pointwise only, k_wgrad_x6 only
    assert all(k.endswith("/1") and k.startswith("x6.") for k in keys if "/t/" in k)
    assert {k.split("/")[2] for k in keys} == {"n", "t"}
    # the math launched is not the family's: the fp16 family on every kernel without an fp16 form
    by_family = {}
    for (k, _), cases in found.items():
        for c in cases:
            by_family.setdefault(c.family, set()).add(_gemm(k))
    assert by_family["fp16"] == {"x6.h1p", "sk128x128.x6", "sk64x64.f32", "sk32x128.f32"}
    assert by_family["bf16"] == {"sk128x128.bf16", "sk64x64.bf16", "sk32x128.bf16"}


def test_refusals_are_the_pinned_ones(swept):
    _, _, refused = swept
    assert {(c.nbranch, c.taps, c.cin, c.cout, c.nimg, c.h, c.w) for c, _ in refused} == REFUSED
    for c, pl in refused:
        assert pl.status == cw.MSL_ERR_SHAPE and pl.gemm == 1 and pl.nchunk > 0 and pl.T * pl.NW >= 2 ** 31, c


def test_refusal_bounds():
    """MSL_ERR_SHAPE exactly from P + 64 >= 2^22 and from max(cin, cout) * P >= 2^29, MSL_OK just below each."""
    for fam, form in cw.MATH_PAIRS:
        fm = hip.Forms(cw.F32_FORMS[form], 1, 1, 1)

        def status(taps, cin, cout, p):
            return hip.conv_wgrad_plan(cw.FAMILIES[fam], 1, taps, cin, cout, 1, p, 1, int(taps == 9), forms_=fm).status

        for taps in (9, 1):
            assert status(taps, 4, 4, 2 ** 22 - 65) == cw.MSL_OK
            assert status(taps, 4, 4, 2 ** 22 - 64) == cw.MSL_ERR_SHAPE
            # 2^29 = 2048 * 2^18: far under the pixel bound, and the plan's other guards hold on both sides
            assert status(taps, 2048, 19, 2 ** 18 - 1) == cw.MSL_OK
            assert status(taps, 2048, 19, 2 ** 18) == cw.MSL_ERR_SHAPE
            assert status(taps, 19, 2048, 2 ** 18 - 1) == cw.MSL_OK
            assert status(taps, 19, 2048, 2 ** 18) == cw.MSL_ERR_SHAPE


def test_scalar_cursor_is_reachable_only_above_the_cap():
    """The longest run of every permitted k_wgrad_x6 plan on a sweep to the pixel bound: the mask table holds
    every run below SCALAR_CURSOR_MIN_PIXELS, and every plan that takes the scalar cursor is over thirty times CASE_MAX_MACS."""
    pixels, p = [], 4096
    while p < 2 ** 22 - 64:
        pixels.append(p)
        p = p * 9 // 8 + 1
    pixels += [2 ** 22 - 65, 2 ** 21, 2 ** 20 + 1]
    scalar, ok = [], 0
    for (fam, form), (taps, nb) in itertools.product(cw.MATH_PAIRS[1:3] + cw.MATH_PAIRS[4:], ((9, 1), (9, 2), (1, 1))):
        fm = hip.Forms(cw.F32_FORMS[form], 1, 1, 1)
        for cin, cout, p in itertools.product((128, 129, 131, 256, 257, 384, 512, 515, 1024, 2048), (128, 129, 256, 512, 2048),
                                              pixels):
            pl = hip.conv_wgrad_plan(cw.FAMILIES[fam], nb, taps, cin, cout, 1, p, 1, int(taps == 9), forms_=fm)
            if pl.status != cw.MSL_OK or not pl.gemm:
                continue
            ok += 1
            assert pl.mask_tab == int(pl.max_run + 3 <= cw.kWxMaskTab)
            if not pl.mask_tab:
                assert pl.nchunk > 0  # chunked, never a stream-K range
                scalar.append((nb * taps * cin * cout * p, p))
    assert ok > 1000 and scalar
    assert min(p for _, p in scalar) >= SCALAR_CURSOR_MIN_PIXELS
    assert min(m for m, _ in scalar) > 30 * cw.CASE_MAX_MACS
    # and the table carries a case of it, on shifted taps (a pointwise run has no border to mask)
    assert any(c.taps == 9 and not cw.plan_of(hip, c).mask_tab for _, _, c in cw.ALL_CASES)


def test_plans_are_consistent_with_their_kernel(swept):
    """What the query reports of a plan agrees with the kernel it names."""
    found, _, _ = swept
    for (key, cls), cases in found.items():
        for c in cases[:: max(1, len(cases) // 60)]:
            pl = cw.plan_of(hip, c)
            p = c.nimg * c.h * c.w
            m, n = (c.cin, c.cout) if pl.trans else (c.cout, c.cin)
            assert pl.trans == int(c.taps == 1 and c.cout > c.cin and pl.gemm == 1)
            assert (pl.bm, pl.bn) in ((128, 128), (64, 64), (32, 128)) and pl.bk == (16 if pl.gemm else 64)
            assert pl.split_rows == pl.gemm and (pl.gemm == 0 or (pl.bm == 128 and min(m, n) >= 128))
            assert pl.tiles_m == -(-m // pl.bm) and pl.tiles_n == -(-n // pl.bn) and pl.ntap == c.nbranch * c.taps
            tiles = pl.tiles_m * pl.tiles_n * pl.ntap
            assert pl.KS == -(-p // pl.bk) and pl.T == tiles * pl.KS
            assert pl.swizzle == int(pl.NW % 8 == 0)
            assert cw.REDUCES[pl.reduce].endswith("%dx%d" % (pl.bm, pl.bn))
            if pl.nchunk > 0:
                assert pl.gemm == 1 and pl.kchunk >= 8 and pl.nchunk == -(-pl.KS // pl.kchunk)
                assert pl.NW == tiles * pl.nchunk <= 4096 and pl.slots == 1 and pl.max_run == pl.kchunk
                assert pl.NW / (-(-pl.NW // 512) * 512) >= 0.75
                assert (pl.reduce == 4) == (pl.nchunk >= 16)
            else:
                assert pl.kchunk == 0 and pl.NW == min(pl.T, 512 if pl.gemm or pl.bm == 64 and max(m, n) > 128 else 256)
                assert pl.slots == (-(-pl.T // pl.NW) + pl.KS - 2) // pl.KS + 1
                assert 1 <= pl.max_run <= min(pl.KS, -(-pl.T // pl.NW))
                if pl.gemm:
                    assert (pl.reduce == 4) == (-(-pl.NW // tiles) >= 16)
            assert pl.mask_tab == pl.gemm  # every grid point is far below the scalar cursor
            # the math launched: the fp16 planes only on k_wgrad_x6, a split form only on a 128-row tile
            fam_math = {"mfma_f32": "f32", "bf16x6": "x6", "f16x3": "h3p"}[c.f32_form] if c.family == "fp32" else \
                {"bf16": "bf16", "fp16": "h1p"}[c.family]
            math = cw.MATHS[pl.math]
            if pl.gemm:
                assert math == fam_math and fam_math in ("x6", "h3p", "h1p")
            elif pl.bm == 128:
                assert math == ("x6" if fam_math in ("h3p", "h1p") else fam_math)
            else:
                assert math == ("bf16" if fam_math == "bf16" else "f32")
            assert pl.rowscale == int(pl.gemm == 1 and math in ("h3p", "h1p"))  # no partials given: per row


def test_rowscale_follows_the_partial_counts():
    """rowscale = 1 only when both operands come with one maximum per row (or none: the call reduces them so)."""
    pw = cw.Case("fp32", "f16x3", 1, 1, 131, 257, 2, 45, 91, 0, 0, 0)  # swapped: the counts trade places with it
    for c in (cw.Case("fp32", "f16x3", 1, 9, 131, 257, 2, 25, 33, 2, 0, 0), pw, pw._replace(family="fp16")):
        assert cw.plan_of(hip, c).gemm == 1
        for xn, dn, want in ((0, 0, 1), (c.cin, c.cout, 1), (c.cin, 0, 1), (0, c.cout, 1), (1, 1, 0), (1, 0, 0),
                             (0, 1, 0), (c.cout, c.cin, 0), (c.cin, c.cout + 1, 0), (64, 64, 0)):
            assert cw.plan_of(hip, c, xn, dn).rowscale == want, (c, xn, dn)
    for c in (pw._replace(f32_form="bf16x6"), pw._replace(f32_form="mfma_f32"), pw._replace(family="bf16")):
        assert cw.plan_of(hip, c, 1, 1).rowscale == 0 and cw.plan_of(hip, c).rowscale == 0  # no scales in these maths


def test_wgrad_split_agrees_with_the_query(swept):
    """msl_conv_wgrad_split (the fp16-operand emulation of the tests asks it) == "the call runs k_wgrad_x6" in the
    x6-capable maths, over the whole grid."""
    lib = hip.load(require_gpu=False)
    n = 0
    for c in cw.grid():
        if (c.family, c.f32_form) in (("fp32", "mfma_f32"), ("bf16", "f16x3")):
            continue
        split = lib.msl_conv_wgrad_split(c.nbranch, c.taps, c.cin, c.cout, c.h, c.w, c.nimg)
        assert split == cw.plan_of(hip, c).gemm, c
        n += 1
    assert n > 10000


@pytest.mark.parametrize("key,cls,case", cw.ALL_CASES, ids=[str(i) for i in range(len(cw.ALL_CASES))])
def test_table_case_lands_where_it_is_filed(key, cls, case):
    assert (case.family, case.f32_form) in cw.MATH_PAIRS
    assert case.taps == 9 or (case.nbranch == 1 and case.dil0 == 0 and case.dil1 == 0)
    pl = cw.plan_of(hip, case)
    assert pl.status == cw.MSL_OK
    assert (cw.plan_key(pl, case.taps), cw.schedule_class(pl)) == (key, cls)
    assert (cw.macs(case) <= cw.CASE_MAX_MACS) != (case in cw.OVER_CAP)


def test_table_has_no_duplicates_and_covers_the_flags():
    cases = [c for _, _, c in cw.ALL_CASES]
    assert len(set(cases)) == len(cases)
    plans = [(c, cw.plan_of(hip, c)) for c in cases]
    # accumulate once per reduce kernel and orientation, the transposed split reduce included, and on a 3x3 call of
    # either branch count (dbias accumulates too)
    acc = {(pl.reduce, pl.trans) for c, pl in plans if c.accumulate}
    assert acc == {(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (3, 1), (4, 1)}
    assert {c.nbranch for c, _ in plans if c.accumulate and c.taps == 9} == {1, 2}
    # k_wgrad_x6 at dilations 1..5 on one image, and at w = 16 and 17 on a pair of odd height
    assert {c.dil0 for c, pl in plans if pl.gemm and c.taps == 9 and c.nimg == 1} >= {1, 2, 3, 4, 5}
    assert {c.w for c, pl in plans if pl.gemm and c.taps == 9 and c.nimg == 2 and c.h % 2} >= {16, 17}
    # a dilation that reaches past the image, per GEMM kernel family: columns and rows
    assert {pl.gemm for c, pl in plans if c.taps == 9 and c.dil0 >= c.w} == {0, 1}
    assert {pl.gemm for c, pl in plans if c.taps == 9 and c.dil0 >= c.h} == {0, 1}


def test_bad_arguments():
    lib = hip.load(require_gpu=False)
    out = hip.ConvWgradPlan()
    ok = dict(family=0, nbranch=1, taps=9, cin=131, cout=257, h=25, w=33, nimg=2, has_dbias=1, x_npart=0, dy_npart=0)
    forms = {name: hip.Forms(v, 1, 1, 1) for name, v in cw.F32_FORMS.items()}

    def plan(fm=forms["f16x3"], o=out, **kw):
        a = dict(ok, **kw)
        return lib.msl_conv_wgrad_plan(a["family"], a["nbranch"], a["taps"], a["cin"], a["cout"], a["h"], a["w"], a["nimg"],
                                       a["has_dbias"], a["x_npart"], a["dy_npart"],
                                       None if fm is None else ctypes.addressof(fm), None if o is None else ctypes.addressof(o))

    assert plan() == cw.MSL_OK and plan(fm=None) == cw.MSL_OK  # NULL forms: the defaults
    assert plan(has_dbias=0) == cw.MSL_OK and plan(nbranch=2) == cw.MSL_OK
    assert plan(taps=1, has_dbias=0) == cw.MSL_OK
    bad = [dict(family=-1), dict(family=3), dict(nbranch=0), dict(nbranch=3), dict(taps=3), dict(cin=0), dict(cout=0),
           dict(h=0), dict(w=0), dict(nimg=0), dict(h=2 ** 15, w=2 ** 15, nimg=2), dict(x_npart=-1), dict(dy_npart=-1),
           dict(taps=1), dict(taps=1, has_dbias=0, nbranch=2)]  # a pointwise call has neither dbias nor a second branch
    for kw in bad:
        assert plan(**kw) == cw.MSL_ERR_ARG, kw
    assert plan(o=None) == cw.MSL_ERR_ARG
    assert plan(fm=hip.Forms(1, 1, 1, 1)) == cw.MSL_ERR_ARG  # no such f32_form
    for name in ("mfma_f32", "bf16x6"):  # the fp16 family reads the f16x3 packs
        assert plan(fm=forms[name], family=2) == cw.MSL_ERR_ARG
        assert plan(fm=forms[name], family=1) == cw.MSL_OK
