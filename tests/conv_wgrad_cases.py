"""The weight-gradient conv cases shared by the CPU gate (test_conv_wgrad_forms.py) and the fp64 parity tests
(test_gpu_conv_wgrad_forms.py): plain data and helpers, no fixtures.

plan_wgrad / plan_chunks / wgrad_swaps (csrc/dconv.hip) send every weight-gradient conv GEMM to one of ten GEMM
instantiations (k_wgrad_x6 or k_wgrad_sk, by tile and math) under a chunked split-K or stream-K schedule, and
wgrad_reduce to one of five piece reduces.  The library answers which through msl_conv_wgrad_plan (host only,
the functions the launch itself calls).  A case here is one call of a C-ABI entry point (msl_dconv_wgrad* /
msl_pconv_wgrad*), filed under the (key, schedule class) the query says it runs; GRID is the sweep the gate
holds the table against.
"""
import itertools
from collections import namedtuple

from conv_form_cases import CASE_MAX_MACS, F32_FORMS, FAMILIES, MATHS, MSL_ERR_ARG, MSL_ERR_SHAPE, MSL_OK  # noqa: F401

Case = namedtuple("Case", "family f32_form nbranch taps cin cout nimg h w dil0 dil1 accumulate")

# the five (family, fp32 form) pairs with a plan of their own: the fp32 entry points in each form, the bf16 ones
# (their plan does not depend on the form) and the fp16 ones (which need the f16x3 form)
MATH_PAIRS = (("fp32", "mfma_f32"), ("fp32", "bf16x6"), ("fp32", "f16x3"), ("bf16", "f16x3"), ("fp16", "f16x3"))
GEMMS = {0: "sk", 1: "x6"}
REDUCES = {0: "r32x128", 1: "r64x64", 2: "wide64x64", 3: "r128x128", 4: "split128x128"}
CLASSES = ("chunk", "chunk_ragged", "sk")  # the classes a reachable key needs a case of ("flat": only if alone)
kWxMaskTab = 2048  # k_wgrad_x6's border-mask table, K-steps (csrc/dconv_kernels.h)


def plan_of(hip, case, x_npart=0, dy_npart=0):
    """The library's plan of the case (hip.ConvWgradPlan) under the case's own forms; every 3x3 case passes
    dbias, no pointwise one has it."""
    forms = hip.Forms(F32_FORMS[case.f32_form], 1, 1, 1)
    return hip.conv_wgrad_plan(FAMILIES[case.family], case.nbranch, case.taps, case.cin, case.cout, case.h, case.w,
                               case.nimg, int(case.taps == 9), x_npart, dy_npart, forms_=forms)


def plan_key(pl, taps):
    """(GEMM kernel with its tile and math, reduce kernel, orientation, taps) as one string."""
    gemm = "x6" if pl.gemm else "sk%dx%d" % (pl.bm, pl.bn)  # k_wgrad_x6 has the one tile, 128 x 128
    return "%s.%s/%s/%s/%d" % (gemm, MATHS[pl.math], REDUCES[pl.reduce], "t" if pl.trans else "n", taps)


def schedule_class(pl):
    """chunk / chunk_ragged: k_wgrad_x6's chunked split-K, the last chunk whole or short; sk: stream-K worker
    ranges that straddle tiles; flat: everything else (at most one K-step per worker, or ranges that end on tile
    boundaries)."""
    if pl.nchunk > 0:
        return "chunk_ragged" if pl.KS % pl.kchunk else "chunk"
    if pl.T > pl.NW and pl.T % pl.NW != 0 and pl.slots >= 2:
        return "sk"
    return "flat"


def macs(case):
    return case.nbranch * case.taps * case.cin * case.cout * case.nimg * case.h * case.w


# ------------------------------------------------------------------------------------------ the grid
# Channels on both sides of 32, 64, 128, 256 and 512 (the thresholds of plan_wgrad), the ragged ones and the
# thresholds themselves; every (cin, cout) pair, so both cout > cin (the pointwise swap) and cin > cout
GRID_CH = (5, 19, 32, 33, 64, 65, 127, 128, 131, 256, 257, 342, 512, 515)
# (nimg, h, w): 203 to 20 000 pixels as one image and as a pair; widths 7 (< 16: no k_wgrad_x6), 16 and 17 (a
# 16-pixel K-step spans two rows) and 33 among them
GRID_PIXELS = ((1, 29, 7), (2, 119, 7), (1, 7, 33), (2, 17, 16), (2, 17, 17), (1, 63, 16), (1, 67, 17), (1, 25, 33),
               (2, 25, 33), (1, 25, 67), (2, 105, 17), (2, 33, 65), (2, 45, 91), (1, 91, 91), (1, 141, 141),
               (2, 100, 100))


def grid():
    """Every call the gate plans: math pair x geometry (3x3 with one and two branches, pointwise) x cin x cout
    x pixels."""
    for (family, f32_form), (taps, nb) in itertools.product(MATH_PAIRS, ((9, 1), (9, 2), (1, 1))):
        for cin, cout, (n, h, w) in itertools.product(GRID_CH, GRID_CH, GRID_PIXELS):
            d0, d1 = (2, 5 if nb == 2 else 0) if taps == 9 else (0, 0)
            yield Case(family, f32_form, nb, taps, cin, cout, n, h, w, d0, d1, 0)


def reached(hip, cases):
    """{(key, class): [cases]}, {key: {swizzle values}} and the refused cases over `cases`, by the library's plan."""
    found, swz, refused = {}, {}, []
    for c in cases:
        pl = plan_of(hip, c)
        if pl.status != MSL_OK:
            refused.append((c, pl))
            continue
        key = plan_key(pl, c.taps)
        found.setdefault((key, schedule_class(pl)), []).append(c)
        swz.setdefault((key, pl.swizzle), []).append(c)
    return found, swz, refused


def rank(hip, c):
    """The case rules, in order: channels off the tile size on both sides; a pair of images for 3x3; an odd P
    for pointwise; more K-steps per run than the pipeline is deep (two stages of one or two K-steps); under
    CASE_MAX_MACS; then the fewest MACs."""
    pl = plan_of(hip, c)
    p = c.nimg * c.h * c.w
    m, n = (c.cin, c.cout) if pl.trans else (c.cout, c.cin)
    return (macs(c) > CASE_MAX_MACS, not (m % pl.bm and n % pl.bn), c.taps == 9 and c.nimg != 2,
            c.taps == 1 and p % 2 == 0, pl.max_run <= 4, macs(c))


def suggest(hip, cases):
    return min(cases, key=lambda c: rank(hip, c))


# ------------------------------------------------------------------------------------------ the table
# (key, class, Case).  First, per reachable (key, class) with a class of CLASSES - and "flat" where a key is
# reachable no other way - the grid point rank() puts first, then a second case per key for the swizzle state the
# first does not have (where the grid reaches both).  Then the edges no plan number shows (EDGES below).
def _c(*a):
    return Case(*a)


TABLE = [
    ("sk128x128.bf16/r128x128/n/1", "sk", _c("bf16", "f16x3", 1, 1, 515, 515, 1, 25, 33, 0, 0, 0)),
    ("sk128x128.bf16/r128x128/n/1", "flat", _c("bf16", "f16x3", 1, 1, 515, 515, 1, 29, 7, 0, 0, 0)),
    ("sk128x128.bf16/r128x128/n/9", "sk", _c("bf16", "f16x3", 1, 9, 515, 515, 2, 17, 16, 2, 0, 0)),
    ("sk128x128.f32/r128x128/n/1", "sk", _c("fp32", "mfma_f32", 1, 1, 515, 515, 1, 25, 33, 0, 0, 0)),
    ("sk128x128.f32/r128x128/n/1", "flat", _c("fp32", "mfma_f32", 1, 1, 515, 515, 1, 29, 7, 0, 0, 0)),
    ("sk128x128.f32/r128x128/n/9", "sk", _c("fp32", "mfma_f32", 1, 9, 515, 515, 2, 17, 16, 2, 0, 0)),
    ("sk128x128.x6/r128x128/n/1", "sk", _c("fp32", "bf16x6", 1, 1, 131, 515, 1, 25, 67, 0, 0, 0)),
    ("sk128x128.x6/r128x128/n/1", "flat", _c("fp32", "bf16x6", 1, 1, 131, 131, 1, 25, 33, 0, 0, 0)),
    ("sk128x128.x6/r128x128/n/9", "sk", _c("fp32", "bf16x6", 1, 9, 131, 257, 2, 119, 7, 2, 0, 0)),
    ("sk128x128.x6/r128x128/n/9", "flat", _c("fp32", "bf16x6", 1, 9, 128, 128, 2, 17, 16, 2, 0, 0)),
    ("sk32x128.bf16/r32x128/n/1", "sk", _c("bf16", "f16x3", 1, 1, 515, 5, 1, 141, 141, 0, 0, 0)),
    ("sk32x128.bf16/r32x128/n/1", "flat", _c("bf16", "f16x3", 1, 1, 5, 5, 1, 29, 7, 0, 0, 0)),
    ("sk32x128.bf16/r32x128/n/9", "sk", _c("bf16", "f16x3", 1, 9, 5, 5, 2, 45, 91, 2, 0, 0)),
    ("sk32x128.bf16/r32x128/n/9", "flat", _c("bf16", "f16x3", 1, 9, 5, 5, 2, 17, 16, 2, 0, 0)),
    ("sk32x128.f32/r32x128/n/1", "sk", _c("fp32", "mfma_f32", 1, 1, 515, 5, 1, 141, 141, 0, 0, 0)),
    ("sk32x128.f32/r32x128/n/1", "flat", _c("fp32", "mfma_f32", 1, 1, 5, 5, 1, 29, 7, 0, 0, 0)),
    ("sk32x128.f32/r32x128/n/9", "sk", _c("fp32", "mfma_f32", 1, 9, 5, 5, 2, 45, 91, 2, 0, 0)),
    ("sk32x128.f32/r32x128/n/9", "flat", _c("fp32", "mfma_f32", 1, 9, 5, 5, 2, 17, 16, 2, 0, 0)),
    ("sk64x64.bf16/r64x64/n/1", "sk", _c("bf16", "f16x3", 1, 1, 342, 342, 1, 91, 91, 0, 0, 0)),
    ("sk64x64.bf16/r64x64/n/1", "flat", _c("bf16", "f16x3", 1, 1, 5, 33, 1, 29, 7, 0, 0, 0)),
    ("sk64x64.bf16/r64x64/n/9", "sk", _c("bf16", "f16x3", 1, 9, 5, 65, 2, 33, 65, 2, 0, 0)),
    ("sk64x64.bf16/r64x64/n/9", "flat", _c("bf16", "f16x3", 1, 9, 5, 33, 2, 17, 16, 2, 0, 0)),
    ("sk64x64.bf16/wide64x64/n/1", "sk", _c("bf16", "f16x3", 1, 1, 5, 515, 1, 141, 141, 0, 0, 0)),
    ("sk64x64.bf16/wide64x64/n/1", "flat", _c("bf16", "f16x3", 1, 1, 5, 33, 1, 67, 17, 0, 0, 0)),
    ("sk64x64.bf16/wide64x64/n/9", "sk", _c("bf16", "f16x3", 1, 9, 5, 33, 2, 45, 91, 2, 0, 0)),
    ("sk64x64.bf16/wide64x64/n/9", "flat", _c("bf16", "f16x3", 1, 9, 5, 33, 2, 25, 33, 2, 0, 0)),
    ("sk64x64.f32/r64x64/n/1", "sk", _c("fp32", "mfma_f32", 1, 1, 342, 342, 1, 91, 91, 0, 0, 0)),
    ("sk64x64.f32/r64x64/n/1", "flat", _c("fp32", "mfma_f32", 1, 1, 5, 33, 1, 29, 7, 0, 0, 0)),
    ("sk64x64.f32/r64x64/n/9", "sk", _c("fp32", "mfma_f32", 1, 9, 5, 65, 2, 33, 65, 2, 0, 0)),
    ("sk64x64.f32/r64x64/n/9", "flat", _c("fp32", "mfma_f32", 1, 9, 5, 33, 2, 17, 16, 2, 0, 0)),
    ("sk64x64.f32/wide64x64/n/1", "sk", _c("fp32", "mfma_f32", 1, 1, 5, 515, 1, 141, 141, 0, 0, 0)),
    ("sk64x64.f32/wide64x64/n/1", "flat", _c("fp32", "mfma_f32", 1, 1, 5, 33, 1, 67, 17, 0, 0, 0)),
    ("sk64x64.f32/wide64x64/n/9", "sk", _c("fp32", "mfma_f32", 1, 9, 5, 33, 2, 45, 91, 2, 0, 0)),
    ("sk64x64.f32/wide64x64/n/9", "flat", _c("fp32", "mfma_f32", 1, 9, 5, 33, 2, 25, 33, 2, 0, 0)),
    ("x6.h1p/r128x128/n/1", "flat", _c("fp16", "f16x3", 1, 1, 257, 257, 1, 29, 7, 0, 0, 0)),
    ("x6.h1p/r128x128/n/1", "flat", _c("fp16", "f16x3", 1, 1, 512, 256, 1, 29, 7, 0, 0, 0)),
    ("x6.h1p/r128x128/n/9", "chunk", _c("fp16", "f16x3", 1, 9, 131, 131, 2, 25, 33, 2, 0, 0)),
    ("x6.h1p/r128x128/n/9", "chunk_ragged", _c("fp16", "f16x3", 2, 9, 131, 257, 2, 17, 16, 2, 5, 0)),
    ("x6.h1p/r128x128/n/9", "sk", _c("fp16", "f16x3", 1, 9, 257, 257, 2, 17, 16, 2, 0, 0)),
    ("x6.h1p/r128x128/t/1", "flat", _c("fp16", "f16x3", 1, 1, 257, 342, 1, 29, 7, 0, 0, 0)),
    ("x6.h1p/r128x128/t/1", "flat", _c("fp16", "f16x3", 1, 1, 256, 512, 1, 29, 7, 0, 0, 0)),
    ("x6.h1p/split128x128/n/1", "chunk", _c("fp16", "f16x3", 1, 1, 257, 257, 1, 141, 141, 0, 0, 0)),
    ("x6.h1p/split128x128/n/1", "chunk_ragged", _c("fp16", "f16x3", 1, 1, 257, 131, 1, 91, 91, 0, 0, 0)),
    ("x6.h1p/split128x128/n/1", "sk", _c("fp16", "f16x3", 1, 1, 515, 515, 1, 25, 67, 0, 0, 0)),
    ("x6.h1p/split128x128/n/9", "chunk", _c("fp16", "f16x3", 1, 9, 131, 257, 2, 105, 17, 2, 0, 0)),
    ("x6.h1p/split128x128/n/9", "chunk_ragged", _c("fp16", "f16x3", 1, 9, 128, 131, 2, 33, 65, 2, 0, 0)),
    ("x6.h1p/split128x128/t/1", "chunk", _c("fp16", "f16x3", 1, 1, 131, 257, 2, 45, 91, 0, 0, 0)),
    ("x6.h1p/split128x128/t/1", "chunk_ragged", _c("fp16", "f16x3", 1, 1, 131, 257, 1, 91, 91, 0, 0, 0)),
    ("x6.h1p/split128x128/t/1", "sk", _c("fp16", "f16x3", 1, 1, 257, 342, 1, 67, 17, 0, 0, 0)),
    ("x6.h3p/r128x128/n/1", "flat", _c("fp32", "f16x3", 1, 1, 257, 257, 1, 29, 7, 0, 0, 0)),
    ("x6.h3p/r128x128/n/1", "flat", _c("fp32", "f16x3", 1, 1, 512, 256, 1, 29, 7, 0, 0, 0)),
    ("x6.h3p/r128x128/n/9", "chunk", _c("fp32", "f16x3", 1, 9, 131, 131, 2, 25, 33, 2, 0, 0)),
    ("x6.h3p/r128x128/n/9", "chunk_ragged", _c("fp32", "f16x3", 2, 9, 131, 257, 2, 17, 16, 2, 5, 0)),
    ("x6.h3p/r128x128/n/9", "sk", _c("fp32", "f16x3", 1, 9, 257, 257, 2, 17, 16, 2, 0, 0)),
    ("x6.h3p/r128x128/t/1", "flat", _c("fp32", "f16x3", 1, 1, 257, 342, 1, 29, 7, 0, 0, 0)),
    ("x6.h3p/r128x128/t/1", "flat", _c("fp32", "f16x3", 1, 1, 256, 512, 1, 29, 7, 0, 0, 0)),
    ("x6.h3p/split128x128/n/1", "chunk", _c("fp32", "f16x3", 1, 1, 257, 257, 1, 141, 141, 0, 0, 0)),
    ("x6.h3p/split128x128/n/1", "chunk_ragged", _c("fp32", "f16x3", 1, 1, 257, 131, 1, 91, 91, 0, 0, 0)),
    ("x6.h3p/split128x128/n/1", "sk", _c("fp32", "f16x3", 1, 1, 515, 515, 1, 25, 67, 0, 0, 0)),
    ("x6.h3p/split128x128/n/9", "chunk", _c("fp32", "f16x3", 1, 9, 131, 257, 2, 105, 17, 2, 0, 0)),
    ("x6.h3p/split128x128/n/9", "chunk_ragged", _c("fp32", "f16x3", 1, 9, 128, 131, 2, 33, 65, 2, 0, 0)),
    ("x6.h3p/split128x128/t/1", "chunk", _c("fp32", "f16x3", 1, 1, 131, 257, 2, 45, 91, 0, 0, 0)),
    ("x6.h3p/split128x128/t/1", "chunk_ragged", _c("fp32", "f16x3", 1, 1, 131, 257, 1, 91, 91, 0, 0, 0)),
    ("x6.h3p/split128x128/t/1", "sk", _c("fp32", "f16x3", 1, 1, 257, 342, 1, 67, 17, 0, 0, 0)),
    ("x6.x6/r128x128/n/1", "flat", _c("fp32", "bf16x6", 1, 1, 257, 257, 1, 29, 7, 0, 0, 0)),
    ("x6.x6/r128x128/n/1", "flat", _c("fp32", "bf16x6", 1, 1, 512, 256, 1, 29, 7, 0, 0, 0)),
    ("x6.x6/r128x128/n/9", "chunk", _c("fp32", "bf16x6", 1, 9, 131, 131, 2, 25, 33, 2, 0, 0)),
    ("x6.x6/r128x128/n/9", "chunk_ragged", _c("fp32", "bf16x6", 2, 9, 131, 257, 2, 17, 16, 2, 5, 0)),
    ("x6.x6/r128x128/n/9", "sk", _c("fp32", "bf16x6", 1, 9, 257, 257, 2, 17, 16, 2, 0, 0)),
    ("x6.x6/r128x128/t/1", "flat", _c("fp32", "bf16x6", 1, 1, 257, 342, 1, 29, 7, 0, 0, 0)),
    ("x6.x6/r128x128/t/1", "flat", _c("fp32", "bf16x6", 1, 1, 256, 512, 1, 29, 7, 0, 0, 0)),
    ("x6.x6/split128x128/n/1", "chunk", _c("fp32", "bf16x6", 1, 1, 257, 257, 1, 141, 141, 0, 0, 0)),
    ("x6.x6/split128x128/n/1", "chunk_ragged", _c("fp32", "bf16x6", 1, 1, 257, 131, 1, 91, 91, 0, 0, 0)),
    ("x6.x6/split128x128/n/1", "sk", _c("fp32", "bf16x6", 1, 1, 515, 515, 1, 25, 67, 0, 0, 0)),
    ("x6.x6/split128x128/n/9", "chunk", _c("fp32", "bf16x6", 1, 9, 131, 257, 2, 105, 17, 2, 0, 0)),
    ("x6.x6/split128x128/n/9", "chunk_ragged", _c("fp32", "bf16x6", 1, 9, 128, 131, 2, 33, 65, 2, 0, 0)),
    ("x6.x6/split128x128/t/1", "chunk", _c("fp32", "bf16x6", 1, 1, 131, 257, 2, 45, 91, 0, 0, 0)),
    ("x6.x6/split128x128/t/1", "chunk_ragged", _c("fp32", "bf16x6", 1, 1, 131, 257, 1, 91, 91, 0, 0, 0)),
    ("x6.x6/split128x128/t/1", "sk", _c("fp32", "bf16x6", 1, 1, 257, 342, 1, 67, 17, 0, 0, 0)),
]

# The edges no plan number shows, each filed under the (key, class) it lands on.  The near-2^22-pixel case runs 32 x
# 128 tiles on 4 x 4 channels: its MACs stay under CASE_MAX_MACS in the reference; only the tile padding exceeds it.
EDGES = [
    # k_wgrad_x6 3x3, one image (tile n0 = 0, the run from K-step 0), dilations 1..5: the first 16-byte load of X's
    # row 0 starts 1-3 elements before X (shifted into place) or exactly 4 before (masked whole), by d % 4
    ("x6.h3p/r128x128/n/9", "chunk_ragged", _c("fp32", "f16x3", 1, 9, 131, 131, 1, 39, 33, 1, 0, 0)),
    ("x6.h3p/r128x128/n/9", "chunk_ragged", _c("fp32", "f16x3", 1, 9, 131, 131, 1, 39, 33, 2, 0, 0)),
    ("x6.h3p/r128x128/n/9", "chunk_ragged", _c("fp32", "f16x3", 1, 9, 131, 131, 1, 39, 33, 3, 0, 0)),
    ("x6.h3p/r128x128/n/9", "chunk_ragged", _c("fp32", "f16x3", 1, 9, 131, 131, 1, 39, 33, 4, 0, 0)),
    ("x6.h3p/r128x128/n/9", "chunk_ragged", _c("fp32", "f16x3", 1, 9, 131, 131, 1, 39, 33, 5, 0, 0)),
    ("x6.x6/r128x128/n/9", "chunk_ragged", _c("fp32", "bf16x6", 1, 9, 131, 131, 1, 39, 33, 3, 0, 0)),
    ("x6.h1p/r128x128/n/9", "chunk_ragged", _c("fp16", "f16x3", 1, 9, 131, 131, 1, 39, 33, 3, 0, 0)),
    # k_wgrad_x6, w = 17 and 16 (a 16-pixel K-step spans two rows), a pair with h odd (a K-step crosses the image
    # seam), at a dilation >= w (every outer column tap exactly 0, or dw0 when accumulating) and at 2; then one
    # image shorter than its dilation (every outer row tap)
    ("x6.h3p/r128x128/n/9", "chunk_ragged", _c("fp32", "f16x3", 1, 9, 131, 131, 2, 39, 17, 17, 0, 0)),
    ("x6.h3p/r128x128/n/9", "chunk_ragged", _c("fp32", "f16x3", 1, 9, 131, 131, 2, 39, 17, 20, 0, 1)),
    ("x6.x6/r128x128/n/9", "chunk_ragged", _c("fp32", "bf16x6", 1, 9, 131, 131, 2, 39, 17, 17, 0, 0)),
    ("x6.h1p/r128x128/n/9", "chunk_ragged", _c("fp16", "f16x3", 1, 9, 131, 131, 2, 39, 17, 2, 0, 0)),
    ("x6.h3p/r128x128/n/9", "chunk_ragged", _c("fp32", "f16x3", 1, 9, 131, 131, 2, 39, 17, 2, 0, 0)),
    ("x6.h3p/r128x128/n/9", "chunk_ragged", _c("fp32", "f16x3", 1, 9, 131, 131, 2, 41, 16, 16, 0, 0)),
    ("x6.h3p/r128x128/n/9", "chunk_ragged", _c("fp32", "f16x3", 1, 9, 131, 131, 2, 41, 16, 19, 0, 1)),
    ("x6.x6/r128x128/n/9", "chunk_ragged", _c("fp32", "bf16x6", 1, 9, 131, 131, 2, 41, 16, 16, 0, 0)),
    ("x6.h1p/r128x128/n/9", "chunk_ragged", _c("fp16", "f16x3", 1, 9, 131, 131, 2, 41, 16, 2, 0, 0)),
    ("x6.h3p/r128x128/n/9", "chunk_ragged", _c("fp32", "f16x3", 1, 9, 131, 131, 2, 41, 16, 2, 0, 0)),
    ("x6.h3p/r128x128/n/9", "chunk_ragged", _c("fp32", "f16x3", 1, 9, 131, 131, 1, 9, 143, 12, 0, 0)),
    ("x6.x6/r128x128/n/9", "chunk_ragged", _c("fp32", "bf16x6", 1, 9, 131, 131, 1, 9, 143, 12, 0, 1)),
    # small images (as in the forward table): a pair narrower than the dilation (2 x 119 x 7 at d = 9), one image
    # shorter than it (1 x 9 x 187 at d = 12), per k_wgrad_sk kernel; w < 16 at channel counts that would
    # otherwise run k_wgrad_x6 (131, 512 / 515); the wide images land on k_wgrad_x6 where its channels allow
    ("sk64x64.f32/r64x64/n/9", "sk", _c("fp32", "mfma_f32", 1, 9, 33, 65, 2, 119, 7, 9, 0, 0)),
    ("sk64x64.f32/r64x64/n/9", "sk", _c("fp32", "mfma_f32", 1, 9, 33, 65, 1, 9, 187, 12, 0, 0)),
    ("sk32x128.f32/r32x128/n/9", "sk", _c("fp32", "mfma_f32", 2, 9, 72, 19, 2, 119, 7, 9, 12, 0)),
    ("sk32x128.f32/r32x128/n/9", "sk", _c("fp32", "mfma_f32", 2, 9, 72, 19, 1, 9, 187, 12, 15, 0)),
    ("sk128x128.f32/r128x128/n/9", "sk", _c("fp32", "mfma_f32", 1, 9, 512, 515, 2, 45, 7, 9, 0, 0)),
    ("sk128x128.f32/r128x128/n/9", "sk", _c("fp32", "mfma_f32", 1, 9, 515, 512, 1, 9, 69, 12, 0, 0)),
    ("sk128x128.x6/r128x128/n/9", "sk", _c("fp32", "bf16x6", 1, 9, 131, 131, 2, 119, 7, 9, 0, 0)),
    ("x6.x6/r128x128/n/9", "chunk_ragged", _c("fp32", "bf16x6", 1, 9, 131, 131, 1, 9, 187, 12, 0, 0)),
    ("sk128x128.x6/r128x128/n/9", "sk", _c("fp32", "f16x3", 1, 9, 131, 131, 2, 119, 7, 9, 0, 0)),
    ("x6.h3p/r128x128/n/9", "chunk_ragged", _c("fp32", "f16x3", 1, 9, 131, 131, 1, 9, 187, 12, 0, 0)),
    ("sk128x128.x6/r128x128/n/9", "sk", _c("fp32", "f16x3", 1, 9, 512, 515, 2, 45, 7, 9, 0, 0)),
    ("x6.h3p/r128x128/n/9", "chunk_ragged", _c("fp32", "f16x3", 1, 9, 515, 512, 1, 9, 69, 12, 0, 0)),
    ("sk64x64.bf16/r64x64/n/9", "sk", _c("bf16", "f16x3", 1, 9, 33, 65, 2, 119, 7, 9, 0, 0)),
    ("sk64x64.bf16/r64x64/n/9", "sk", _c("bf16", "f16x3", 1, 9, 33, 65, 1, 9, 187, 12, 0, 0)),
    ("sk32x128.bf16/r32x128/n/9", "sk", _c("bf16", "f16x3", 2, 9, 72, 19, 2, 119, 7, 9, 12, 0)),
    ("sk32x128.bf16/r32x128/n/9", "sk", _c("bf16", "f16x3", 2, 9, 72, 19, 1, 9, 187, 12, 15, 0)),
    ("sk128x128.bf16/r128x128/n/9", "sk", _c("bf16", "f16x3", 1, 9, 512, 515, 2, 45, 7, 9, 0, 0)),
    ("sk128x128.bf16/r128x128/n/9", "sk", _c("bf16", "f16x3", 1, 9, 515, 512, 1, 9, 69, 12, 0, 0)),
    ("sk64x64.f32/r64x64/n/9", "sk", _c("fp16", "f16x3", 1, 9, 33, 65, 2, 119, 7, 9, 0, 0)),
    ("sk64x64.f32/r64x64/n/9", "sk", _c("fp16", "f16x3", 1, 9, 33, 65, 1, 9, 187, 12, 0, 0)),
    ("sk32x128.f32/r32x128/n/9", "sk", _c("fp16", "f16x3", 2, 9, 72, 19, 2, 119, 7, 9, 12, 0)),
    ("sk32x128.f32/r32x128/n/9", "sk", _c("fp16", "f16x3", 2, 9, 72, 19, 1, 9, 187, 12, 15, 0)),
    ("sk128x128.x6/r128x128/n/9", "sk", _c("fp16", "f16x3", 1, 9, 131, 131, 2, 119, 7, 9, 0, 0)),
    ("x6.h1p/r128x128/n/9", "chunk_ragged", _c("fp16", "f16x3", 1, 9, 131, 131, 1, 9, 187, 12, 0, 0)),
    # k_wgrad_sk's float pixel-to-row division ((p + 0.5f) * invW) close under the 2^22-pixel refusal, a width that
    # is no power of two, few channels
    ("sk32x128.f32/r32x128/n/9", "sk", _c("fp32", "mfma_f32", 1, 9, 4, 4, 1, 1023, 4099, 2, 0, 0)),
    # k_wgrad_x6's scalar mask cursor: a run of more than kWxMaskTab - 3 K-steps.  plan_chunks allows it from about
    # 229 000 pixels (72 tiles x 7 chunks of 2049 K-steps: 71 GMAC), far above CASE_MAX_MACS - the one case over the
    # cap (OVER_CAP), its reference computed in fp64 on the GPU; a pair, so the cursor crosses the image seam
    ("x6.h3p/r128x128/n/9", "chunk_ragged", _c("fp32", "f16x3", 2, 9, 131, 131, 2, 457, 251, 2, 5, 0)),
    # the fp16 family on the kernels without an fp16 form: bf16x6 on the 128-row stream-K tile (the fill too low
    # for k_wgrad_x6), exact f32 on the 64- and 32-row tiles
    ("sk128x128.x6/r128x128/n/1", "sk", _c("fp16", "f16x3", 1, 1, 131, 131, 2, 33, 65, 0, 0, 0)),
    ("sk128x128.x6/r128x128/n/9", "sk", _c("fp16", "f16x3", 2, 9, 131, 131, 1, 7, 33, 2, 5, 0)),
    ("sk64x64.f32/r64x64/n/9", "sk", _c("fp16", "f16x3", 1, 9, 33, 65, 2, 25, 33, 2, 0, 0)),
    ("sk32x128.f32/r32x128/n/9", "sk", _c("fp16", "f16x3", 2, 9, 5, 5, 2, 25, 33, 2, 5, 0)),
    # accumulate = 1 (dw and, for 3x3, dbias), once per reduce kernel, orientation and geometry
    ("sk128x128.f32/r128x128/n/1", "sk", _c("fp32", "mfma_f32", 1, 1, 515, 515, 1, 25, 33, 0, 0, 1)),
    ("sk128x128.x6/r128x128/n/9", "sk", _c("fp32", "bf16x6", 1, 9, 131, 257, 2, 119, 7, 2, 0, 1)),
    ("sk32x128.f32/r32x128/n/1", "sk", _c("fp32", "mfma_f32", 1, 1, 515, 5, 1, 141, 141, 0, 0, 1)),
    ("sk32x128.f32/r32x128/n/9", "sk", _c("fp32", "mfma_f32", 1, 9, 5, 5, 2, 45, 91, 2, 0, 1)),
    ("sk64x64.f32/r64x64/n/1", "flat", _c("fp32", "mfma_f32", 1, 1, 5, 33, 1, 29, 7, 0, 0, 1)),
    ("sk64x64.f32/r64x64/n/9", "sk", _c("fp32", "mfma_f32", 1, 9, 5, 65, 2, 33, 65, 2, 0, 1)),
    ("sk64x64.f32/wide64x64/n/1", "sk", _c("fp32", "mfma_f32", 1, 1, 5, 515, 1, 141, 141, 0, 0, 1)),
    ("sk64x64.f32/wide64x64/n/9", "sk", _c("fp32", "mfma_f32", 1, 9, 5, 33, 2, 45, 91, 2, 0, 1)),
    ("x6.h3p/r128x128/n/9", "chunk_ragged", _c("fp32", "f16x3", 2, 9, 131, 257, 2, 17, 16, 2, 5, 1)),
    ("x6.h3p/r128x128/t/1", "flat", _c("fp32", "f16x3", 1, 1, 257, 342, 1, 29, 7, 0, 0, 1)),
    ("x6.h3p/split128x128/n/1", "chunk_ragged", _c("fp32", "f16x3", 1, 1, 257, 131, 1, 91, 91, 0, 0, 1)),
    ("x6.h3p/split128x128/n/9", "chunk_ragged", _c("fp32", "f16x3", 1, 9, 128, 131, 2, 33, 65, 2, 0, 1)),
    ("x6.h3p/split128x128/t/1", "chunk", _c("fp32", "f16x3", 1, 1, 131, 257, 2, 45, 91, 0, 0, 1)),
]

ALL_CASES = TABLE + EDGES
OVER_CAP = {Case("fp32", "f16x3", 2, 9, 131, 131, 2, 457, 251, 2, 5, 0)}  # the scalar-cursor case (see EDGES)
GPU_REFERENCE_PIXELS = 1 << 18  # from here the fp64 reference is computed on the GPU (two cases)


def case_id(key, cls, c):
    return "%s-%s-%s-%s-b%d-%dx%d-%dx%dx%d-d%d.%d-a%d" % (key, cls, c.family, c.f32_form, c.nbranch, c.cin, c.cout, c.nimg,
                                                         c.h, c.w, c.dil0, c.dil1, c.accumulate)
