"""The forward-form conv cases shared by the CPU gate (test_conv_forms.py) and the fp64 parity tests
(test_gpu_conv_forms.py): plain data and helpers, no fixtures.

plan_fwd (csrc/dconv.hip) picks, for every forward and data-gradient conv GEMM, one instantiation of the
stream-K kernel (a row of kSkKernels) or the split-K tile kernel, and plan_sk its schedule.  The library
answers which through msl_conv_fwd_plan (host only).  A case here is one call of a C-ABI entry point, filed
under the (kernel, schedule class) the query says it runs; GRID is the sweep the gate holds the table
against: every (kernel, class) some grid point reaches needs a case.
"""
import ctypes
import itertools
from collections import namedtuple

Case = namedtuple("Case", "entry family f32_form sk_hybrid nbranch cin cout h w nimg dil0 dil1")

# entry point -> (taps, data gradient, accumulate)
ENTRIES = {
    "dconv_fwd": (9, False, 0), "dconv_dgrad": (9, True, 0),
    "pconv_fwd": (1, False, 0), "pconv_dgrad": (1, True, 0),
    "pconv_dgrad_acc": (1, True, 1), "pconv_dgrad_resmask": (1, True, 1),
}
FAMILIES = {"fp32": 0, "bf16": 1, "fp16": 2}
F32_FORMS = {"mfma_f32": 0, "bf16x6": 2, "f16x3": 5}
# msl_conv_form.math / msl_conv_fwd_plan_info.math
MATHS = {0: "f32", 1: "bf16", 2: "x6", 3: "x6p", 5: "h3p", 8: "h1p"}
BFORMS = {0: "lds", 1: "bd", 2: "bp"}
CLASSES = ("sk", "hybrid", "dp_only", "tile_split", "tile_single")  # the classes a reachable kernel needs a case of
MSL_OK, MSL_ERR_SHAPE, MSL_ERR_ARG = 0, -1, -3


def entry_exists(entry, family):
    """The bf16 entry points have no accumulate epilogue of either kind (include/msl_hip.h)."""
    return not (family == "bf16" and ENTRIES[entry][2])


def family_runs(family, f32_form):
    """The _f16 entry points need the f16x3 packs; the bf16 ones read the fp32 part of any pack (one form
    is enough: its plan does not depend on f32_form)."""
    return f32_form == "f16x3" or family == "fp32"


def plan_args(case):
    """(family, nbranch, taps, cimg, M, P, accumulate, dil0) of msl_conv_fwd_plan: a data gradient's image
    operand is dy (cout channels) and its rows are cin."""
    taps, dgrad, acc = ENTRIES[case.entry]
    cimg, m = (case.cout, case.cin) if dgrad else (case.cin, case.cout)
    return (FAMILIES[case.family], case.nbranch, taps, cimg, m, case.nimg * case.h * case.w, acc,
            case.dil0 if taps == 9 else 0)


def plan_of(hip, case):
    """The library's plan of the case (hip.ConvFwdPlan) under the case's own forms."""
    forms = hip.Forms(F32_FORMS[case.f32_form], case.sk_hybrid, 1, 1)
    return hip.conv_fwd_plan(*plan_args(case), forms_=forms)


def form_key(hip, row):
    """A row of the kernel table by its own template arguments (stable if the table is reordered)."""
    if row < 0:
        return "tile"
    f = hip.ConvForm()
    assert hip.load(require_gpu=False).msl_conv_fwd_form_describe(row, ctypes.addressof(f)) == MSL_OK
    return "%d.g%d.s%d.%dx%d.%s.%s.%s.%s" % (f.bm, f.G, f.stages, f.wm, f.wn, "pw" if f.pw else "xy", MATHS[f.math],
                                              "acc" if f.acc else "set", BFORMS[f.bform])


def all_form_keys(hip):
    n = hip.load(require_gpu=False).msl_conv_fwd_form_count()
    return [form_key(hip, r) for r in range(n)]


def schedule_class(pl):
    """The schedule class of a plan; "flat" is a stream-K schedule that exercises no tile-straddling worker
    range (at most one stage per worker, or ranges that end on tile boundaries): the gate asks no case of it."""
    if not pl.stream_k:
        return "tile_split" if pl.S > 1 else "tile_single"
    if pl.tdp > 0:
        return "hybrid" if pl.T > 0 else "dp_only"
    if pl.T > pl.NW and pl.T % pl.NW != 0:
        return "sk"
    return "flat"


def macs(case):
    return case.nbranch * ENTRIES[case.entry][0] * case.cin * case.cout * case.nimg * case.h * case.w


# ------------------------------------------------------------------------------------------ the grid
# Channels of the image operand: 1 / 2 / 5 / 6 full 16-channel blocks (odd and even K-step counts), the ragged
# 72 (5 blocks), 147 (10, the stem's im2col rows) and 234 = 18 * 13 (15 blocks: the ASPP shift data gradient);
# 8 / 24 (one / two ragged blocks: the LDS image form at the sizes of whole data-parallel rounds);
# 256 / 272 (16 / 17 blocks): deep enough that 65 pixel tiles of one row block outnumber the 512 workers' stages
GRID_CIMG = (8, 16, 24, 32, 72, 80, 96, 147, 234, 256, 272)
# Rows: both sides of 32, 64, 128 (the fp16 BP form), 512 (the f16x3 BP form) and the 256-row tile's
# M >= 2048, M % 256 == 0
GRID_M = (19, 29, 32, 33, 48, 61, 64, 65, 67, 100, 127, 128, 131, 342, 511, 512, 1024, 1920, 2048, 2176)
# (nimg, h, w): 14 ragged pixel tiles with P odd (the pointwise dwordx4 rows then start off 16 bytes) and a pair
# of 13 tiles; 64 and 65 pixel tiles (x 8 row blocks of 128 = 512 and 520 tiles); 512 and 515 pixel tiles for the
# single-row-block forms; each as one image with P odd and as a pair (whose images are no multiple of 64 px: the
# residual mask's rows end inside a word)
GRID_PIXELS = ((1, 25, 67), (2, 25, 33), (2, 45, 91), (1, 91, 91), (2, 50, 83), (1, 255, 257), (2, 181, 181),
               (1, 219, 301), (2, 181, 182))
CASE_MAX_MACS = 1.5e9  # of a table case (its fp64 reference); the gate plans every grid point, whatever its size


def grid():
    """Every call the gate plans: entry point x family x fp32 form x schedule form x channels x rows x pixels
    (the two-branch 3x3 forward and data gradient included)."""
    for entry, family, f32_form in itertools.product(ENTRIES, FAMILIES, F32_FORMS):
        if not entry_exists(entry, family) or not family_runs(family, f32_form):
            continue
        taps, dgrad, _ = ENTRIES[entry]
        for nb in ((1, 2) if taps == 9 else (1,)):
            for hyb, cimg, m, (n, h, w) in itertools.product((1, 0), GRID_CIMG, GRID_M, GRID_PIXELS):
                cin, cout = (m, cimg) if dgrad else (cimg, m)
                d0, d1 = (2, 5 if nb == 2 else 0) if taps == 9 else (0, 0)
                yield Case(entry, family, f32_form, hyb, nb, cin, cout, h, w, n, d0, d1)


def reached(hip, cases):
    """{(form key, class): [cases]} and the refused cases over `cases`, by the library's own plan."""
    keys = all_form_keys(hip)
    found, refused = {}, []
    for c in cases:
        pl = plan_of(hip, c)
        if pl.status != MSL_OK:
            refused.append((c, pl))
            continue
        cls = schedule_class(pl)
        key = keys[pl.row] if pl.stream_k else "tile"
        found.setdefault((key, cls), []).append(c)
    return found, refused


def suggest(found, key, cls):
    """A grid point for (key, cls) out of reached()'s `found`: the cheapest under the default schedule form."""
    return min(found[(key, cls)], key=lambda c: (c.sk_hybrid != 1, macs(c) > CASE_MAX_MACS, macs(c)))


# ------------------------------------------------------------------------------------------ the table
# (form key, class, Case).  First, per reachable (kernel, class), a grid point chosen by these rules in order: the
# default schedule form; M off the tile size; at most CASE_MAX_MACS and 2^25 outputs; the data-gradient entry for
# the hybrid class and the forward one elsewhere (accumulating kernels: the masked residual for hybrid - its
# epilogue then runs in the GEMM and in the reduce - and the plain accumulate elsewhere); more K stages per tile
# than the kernel's pipeline is deep; a pair for 3x3 and masked-residual calls, an odd pixel count for the other
# pointwise ones; then the fewest MACs.  Then the edges no plan number shows, per 3x3 kernel: one image shorter
# than its dilation (forward) and a pair narrower than it (data gradient), so every outer tap of a row or column
# falls outside and a tap that crossed the image seam would show.  Last, pure stream-K (sk_hybrid 0) on a call
# large enough for data-parallel rounds, once per math.  suggest() names the grid point for a pair the gate misses.
def _c(*a):
    return Case(*a)


TABLE = [
    ("128.g1.s3.2x2.xy.bf16.set.lds", "dp_only", _c("dconv_fwd", "bf16", "f16x3", 1, 1, 8, 65, 181, 181, 2, 2, 0)),
    ("128.g1.s3.2x2.xy.bf16.set.lds", "hybrid", _c("dconv_dgrad", "bf16", "f16x3", 1, 1, 65, 8, 181, 182, 2, 2, 0)),
    ("128.g1.s3.2x2.xy.bf16.set.lds", "sk", _c("dconv_fwd", "bf16", "f16x3", 1, 1, 8, 65, 45, 91, 2, 2, 0)),
    ("128.g1.s3.2x2.xy.f32.acc.lds", "dp_only", _c("pconv_dgrad_acc", "fp32", "mfma_f32", 1, 1, 65, 72, 255, 257, 1, 0, 0)),
    ("128.g1.s3.2x2.xy.f32.acc.lds", "hybrid", _c("pconv_dgrad_resmask", "fp32", "mfma_f32", 1, 1, 65, 72, 181, 182, 2, 0, 0)),
    ("128.g1.s3.2x2.xy.f32.acc.lds", "sk", _c("pconv_dgrad_acc", "fp32", "mfma_f32", 1, 1, 131, 72, 91, 91, 1, 0, 0)),
    ("128.g1.s3.2x2.xy.f32.set.lds", "dp_only", _c("dconv_fwd", "fp32", "mfma_f32", 1, 1, 8, 65, 181, 181, 2, 2, 0)),
    ("128.g1.s3.2x2.xy.f32.set.lds", "hybrid", _c("dconv_dgrad", "fp32", "mfma_f32", 1, 1, 65, 8, 181, 182, 2, 2, 0)),
    ("128.g1.s3.2x2.xy.f32.set.lds", "sk", _c("dconv_fwd", "fp32", "mfma_f32", 1, 1, 8, 65, 45, 91, 2, 2, 0)),
    ("128.g1.s4.1x4.pw.h1p.acc.lds", "dp_only", _c("pconv_dgrad_acc", "fp16", "f16x3", 1, 1, 65, 72, 255, 257, 1, 0, 0)),
    ("128.g1.s4.1x4.pw.h1p.acc.lds", "hybrid", _c("pconv_dgrad_resmask", "fp16", "f16x3", 1, 1, 65, 72, 181, 182, 2, 0, 0)),
    ("128.g1.s4.1x4.pw.h1p.acc.lds", "sk", _c("pconv_dgrad_acc", "fp16", "f16x3", 1, 1, 131, 72, 91, 91, 1, 0, 0)),
    ("128.g1.s4.1x4.pw.h1p.set.lds", "dp_only", _c("pconv_fwd", "fp16", "f16x3", 1, 1, 72, 65, 255, 257, 1, 0, 0)),
    ("128.g1.s4.1x4.pw.h1p.set.lds", "hybrid", _c("pconv_dgrad", "fp16", "f16x3", 1, 1, 65, 72, 219, 301, 1, 0, 0)),
    ("128.g1.s4.1x4.pw.h1p.set.lds", "sk", _c("pconv_fwd", "fp16", "f16x3", 1, 1, 72, 131, 91, 91, 1, 0, 0)),
    ("128.g1.s4.1x4.pw.h3p.acc.lds", "dp_only", _c("pconv_dgrad_acc", "fp32", "f16x3", 1, 1, 65, 72, 255, 257, 1, 0, 0)),
    ("128.g1.s4.1x4.pw.h3p.acc.lds", "hybrid", _c("pconv_dgrad_resmask", "fp32", "f16x3", 1, 1, 65, 72, 181, 182, 2, 0, 0)),
    ("128.g1.s4.1x4.pw.h3p.acc.lds", "sk", _c("pconv_dgrad_acc", "fp32", "f16x3", 1, 1, 131, 72, 91, 91, 1, 0, 0)),
    ("128.g1.s4.1x4.pw.h3p.set.lds", "dp_only", _c("pconv_fwd", "fp32", "f16x3", 1, 1, 72, 65, 255, 257, 1, 0, 0)),
    ("128.g1.s4.1x4.pw.h3p.set.lds", "hybrid", _c("pconv_dgrad", "fp32", "f16x3", 1, 1, 65, 72, 219, 301, 1, 0, 0)),
    ("128.g1.s4.1x4.pw.h3p.set.lds", "sk", _c("pconv_fwd", "fp32", "f16x3", 1, 1, 72, 131, 91, 91, 1, 0, 0)),
    ("128.g1.s4.1x4.xy.h1p.set.bd", "dp_only", _c("dconv_fwd", "fp16", "f16x3", 1, 1, 16, 65, 181, 181, 2, 2, 0)),
    ("128.g1.s4.1x4.xy.h1p.set.bd", "hybrid", _c("dconv_dgrad", "fp16", "f16x3", 1, 1, 65, 16, 181, 182, 2, 2, 0)),
    ("128.g1.s4.1x4.xy.h1p.set.bd", "sk", _c("dconv_fwd", "fp16", "f16x3", 1, 1, 16, 65, 45, 91, 2, 2, 0)),
    ("128.g1.s4.1x4.xy.h1p.set.bp", "dp_only", _c("dconv_fwd", "fp16", "f16x3", 1, 1, 8, 131, 181, 181, 2, 2, 0)),
    ("128.g1.s4.1x4.xy.h1p.set.bp", "hybrid", _c("dconv_dgrad", "fp16", "f16x3", 1, 1, 131, 8, 181, 182, 2, 2, 0)),
    ("128.g1.s4.1x4.xy.h1p.set.bp", "sk", _c("dconv_fwd", "fp16", "f16x3", 1, 1, 8, 131, 45, 91, 2, 2, 0)),
    ("128.g1.s4.1x4.xy.h1p.set.lds", "dp_only", _c("dconv_fwd", "fp16", "f16x3", 1, 1, 8, 65, 181, 181, 2, 2, 0)),
    ("128.g1.s4.1x4.xy.h1p.set.lds", "hybrid", _c("dconv_dgrad", "fp16", "f16x3", 1, 1, 65, 8, 181, 182, 2, 2, 0)),
    ("128.g1.s4.1x4.xy.h1p.set.lds", "sk", _c("dconv_fwd", "fp16", "f16x3", 1, 1, 8, 65, 45, 91, 2, 2, 0)),
    ("128.g1.s4.1x4.xy.h3p.set.bd", "dp_only", _c("dconv_fwd", "fp32", "f16x3", 1, 1, 16, 65, 181, 181, 2, 2, 0)),
    ("128.g1.s4.1x4.xy.h3p.set.bd", "hybrid", _c("dconv_dgrad", "fp32", "f16x3", 1, 1, 65, 16, 181, 182, 2, 2, 0)),
    ("128.g1.s4.1x4.xy.h3p.set.bd", "sk", _c("dconv_fwd", "fp32", "f16x3", 1, 1, 16, 65, 45, 91, 2, 2, 0)),
    ("128.g1.s4.1x4.xy.h3p.set.bp", "dp_only", _c("dconv_fwd", "fp32", "f16x3", 1, 1, 8, 1024, 45, 91, 2, 2, 0)),
    ("128.g1.s4.1x4.xy.h3p.set.bp", "hybrid", _c("dconv_dgrad", "fp32", "f16x3", 1, 1, 1024, 8, 50, 83, 2, 2, 0)),
    ("128.g1.s4.1x4.xy.h3p.set.bp", "sk", _c("dconv_fwd", "fp32", "f16x3", 1, 1, 8, 1024, 25, 33, 2, 2, 0)),
    ("128.g1.s4.1x4.xy.h3p.set.lds", "dp_only", _c("dconv_fwd", "fp32", "f16x3", 1, 1, 8, 65, 181, 181, 2, 2, 0)),
    ("128.g1.s4.1x4.xy.h3p.set.lds", "hybrid", _c("dconv_dgrad", "fp32", "f16x3", 1, 1, 65, 8, 181, 182, 2, 2, 0)),
    ("128.g1.s4.1x4.xy.h3p.set.lds", "sk", _c("dconv_fwd", "fp32", "f16x3", 1, 1, 8, 65, 45, 91, 2, 2, 0)),
    ("128.g1.s4.2x2.xy.x6p.acc.lds", "dp_only", _c("pconv_dgrad_acc", "fp32", "bf16x6", 1, 1, 65, 72, 255, 257, 1, 0, 0)),
    ("128.g1.s4.2x2.xy.x6p.acc.lds", "hybrid", _c("pconv_dgrad_resmask", "fp32", "bf16x6", 1, 1, 65, 72, 181, 182, 2, 0, 0)),
    ("128.g1.s4.2x2.xy.x6p.acc.lds", "sk", _c("pconv_dgrad_acc", "fp32", "bf16x6", 1, 1, 131, 72, 91, 91, 1, 0, 0)),
    ("128.g1.s4.2x2.xy.x6p.set.lds", "dp_only", _c("dconv_fwd", "fp32", "bf16x6", 1, 1, 8, 65, 181, 181, 2, 2, 0)),
    ("128.g1.s4.2x2.xy.x6p.set.lds", "hybrid", _c("dconv_dgrad", "fp32", "bf16x6", 1, 1, 65, 8, 181, 182, 2, 2, 0)),
    ("128.g1.s4.2x2.xy.x6p.set.lds", "sk", _c("dconv_fwd", "fp32", "bf16x6", 1, 1, 8, 65, 45, 91, 2, 2, 0)),
    ("128.g2.s2.2x2.xy.bf16.set.lds", "dp_only", _c("pconv_fwd", "bf16", "f16x3", 1, 1, 96, 65, 255, 257, 1, 0, 0)),
    ("128.g2.s2.2x2.xy.bf16.set.lds", "hybrid", _c("pconv_dgrad", "bf16", "f16x3", 1, 1, 65, 96, 219, 301, 1, 0, 0)),
    ("128.g2.s2.2x2.xy.bf16.set.lds", "sk", _c("dconv_fwd", "bf16", "f16x3", 1, 2, 8, 65, 45, 91, 2, 2, 5)),
    ("128.g2.s2.2x2.xy.f32.acc.lds", "dp_only", _c("pconv_dgrad_acc", "fp32", "mfma_f32", 1, 1, 65, 96, 255, 257, 1, 0, 0)),
    ("128.g2.s2.2x2.xy.f32.acc.lds", "hybrid", _c("pconv_dgrad_resmask", "fp32", "mfma_f32", 1, 1, 65, 96, 181, 182, 2, 0, 0)),
    ("128.g2.s2.2x2.xy.f32.acc.lds", "sk", _c("pconv_dgrad_acc", "fp32", "mfma_f32", 1, 1, 65, 256, 91, 91, 1, 0, 0)),
    ("128.g2.s2.2x2.xy.f32.set.lds", "dp_only", _c("pconv_fwd", "fp32", "mfma_f32", 1, 1, 96, 65, 255, 257, 1, 0, 0)),
    ("128.g2.s2.2x2.xy.f32.set.lds", "hybrid", _c("pconv_dgrad", "fp32", "mfma_f32", 1, 1, 65, 96, 219, 301, 1, 0, 0)),
    ("128.g2.s2.2x2.xy.f32.set.lds", "sk", _c("dconv_fwd", "fp32", "mfma_f32", 1, 2, 8, 65, 45, 91, 2, 2, 5)),
    ("128.g2.s3.1x4.pw.h1p.acc.lds", "dp_only", _c("pconv_dgrad_acc", "fp16", "f16x3", 1, 1, 65, 147, 255, 257, 1, 0, 0)),
    ("128.g2.s3.1x4.pw.h1p.acc.lds", "hybrid", _c("pconv_dgrad_resmask", "fp16", "f16x3", 1, 1, 65, 147, 181, 182, 2, 0, 0)),
    ("128.g2.s3.1x4.pw.h1p.acc.lds", "sk", _c("pconv_dgrad_acc", "fp16", "f16x3", 1, 1, 65, 256, 91, 91, 1, 0, 0)),
    ("128.g2.s3.1x4.pw.h1p.set.lds", "dp_only", _c("pconv_fwd", "fp16", "f16x3", 1, 1, 147, 65, 255, 257, 1, 0, 0)),
    ("128.g2.s3.1x4.pw.h1p.set.lds", "hybrid", _c("pconv_dgrad", "fp16", "f16x3", 1, 1, 65, 147, 219, 301, 1, 0, 0)),
    ("128.g2.s3.1x4.pw.h1p.set.lds", "sk", _c("pconv_fwd", "fp16", "f16x3", 1, 1, 256, 65, 91, 91, 1, 0, 0)),
    ("256.g1.s3.1x4.pw.h3p.acc.lds", "dp_only", _c("pconv_dgrad_acc", "fp32", "f16x3", 1, 1, 2048, 72, 45, 91, 2, 0, 0)),
    ("256.g1.s3.1x4.pw.h3p.acc.lds", "hybrid", _c("pconv_dgrad_resmask", "fp32", "f16x3", 1, 1, 2048, 72, 50, 83, 2, 0, 0)),
    ("256.g1.s3.1x4.pw.h3p.acc.lds", "sk", _c("pconv_dgrad_acc", "fp32", "f16x3", 1, 1, 2048, 72, 25, 67, 1, 0, 0)),
    ("256.g1.s3.1x4.pw.h3p.set.lds", "dp_only", _c("pconv_fwd", "fp32", "f16x3", 1, 1, 72, 2048, 45, 91, 2, 0, 0)),
    ("256.g1.s3.1x4.pw.h3p.set.lds", "hybrid", _c("pconv_dgrad", "fp32", "f16x3", 1, 1, 2048, 72, 91, 91, 1, 0, 0)),
    ("256.g1.s3.1x4.pw.h3p.set.lds", "sk", _c("pconv_fwd", "fp32", "f16x3", 1, 1, 72, 2048, 25, 67, 1, 0, 0)),
    ("32.g2.s2.1x4.xy.bf16.set.lds", "dp_only", _c("pconv_fwd", "bf16", "f16x3", 1, 1, 96, 19, 255, 257, 1, 0, 0)),
    ("32.g2.s2.1x4.xy.bf16.set.lds", "hybrid", _c("pconv_dgrad", "bf16", "f16x3", 1, 1, 19, 96, 219, 301, 1, 0, 0)),
    ("32.g2.s2.1x4.xy.bf16.set.lds", "sk", _c("dconv_fwd", "bf16", "f16x3", 1, 2, 8, 19, 45, 91, 2, 2, 5)),
    ("32.g2.s2.1x4.xy.f32.acc.lds", "dp_only", _c("pconv_dgrad_acc", "fp32", "mfma_f32", 1, 1, 19, 96, 255, 257, 1, 0, 0)),
    ("32.g2.s2.1x4.xy.f32.acc.lds", "hybrid", _c("pconv_dgrad_resmask", "fp32", "mfma_f32", 1, 1, 19, 96, 181, 182, 2, 0, 0)),
    ("32.g2.s2.1x4.xy.f32.acc.lds", "sk", _c("pconv_dgrad_acc", "fp32", "mfma_f32", 1, 1, 19, 256, 91, 91, 1, 0, 0)),
    ("32.g2.s2.1x4.xy.f32.set.lds", "dp_only", _c("pconv_fwd", "fp32", "mfma_f32", 1, 1, 96, 19, 255, 257, 1, 0, 0)),
    ("32.g2.s2.1x4.xy.f32.set.lds", "hybrid", _c("pconv_dgrad", "fp32", "mfma_f32", 1, 1, 19, 96, 219, 301, 1, 0, 0)),
    ("32.g2.s2.1x4.xy.f32.set.lds", "sk", _c("dconv_fwd", "fp32", "mfma_f32", 1, 2, 8, 19, 45, 91, 2, 2, 5)),
    ("64.g1.s3.2x2.xy.bf16.set.lds", "dp_only", _c("dconv_fwd", "bf16", "f16x3", 1, 1, 8, 33, 181, 181, 2, 2, 0)),
    ("64.g1.s3.2x2.xy.bf16.set.lds", "hybrid", _c("dconv_dgrad", "bf16", "f16x3", 1, 1, 33, 8, 181, 182, 2, 2, 0)),
    ("64.g1.s3.2x2.xy.bf16.set.lds", "sk", _c("dconv_fwd", "bf16", "f16x3", 1, 1, 8, 33, 45, 91, 2, 2, 0)),
    ("64.g1.s3.2x2.xy.f32.acc.lds", "dp_only", _c("pconv_dgrad_acc", "fp32", "mfma_f32", 1, 1, 33, 72, 255, 257, 1, 0, 0)),
    ("64.g1.s3.2x2.xy.f32.acc.lds", "hybrid", _c("pconv_dgrad_resmask", "fp32", "mfma_f32", 1, 1, 33, 72, 181, 182, 2, 0, 0)),
    ("64.g1.s3.2x2.xy.f32.acc.lds", "sk", _c("pconv_dgrad_acc", "fp32", "mfma_f32", 1, 1, 33, 234, 91, 91, 1, 0, 0)),
    ("64.g1.s3.2x2.xy.f32.set.lds", "dp_only", _c("dconv_fwd", "fp32", "mfma_f32", 1, 1, 8, 33, 181, 181, 2, 2, 0)),
    ("64.g1.s3.2x2.xy.f32.set.lds", "hybrid", _c("dconv_dgrad", "fp32", "mfma_f32", 1, 1, 33, 8, 181, 182, 2, 2, 0)),
    ("64.g1.s3.2x2.xy.f32.set.lds", "sk", _c("dconv_fwd", "fp32", "mfma_f32", 1, 1, 8, 33, 45, 91, 2, 2, 0)),
    ("64.g1.s4.1x4.xy.h1p.acc.bd", "dp_only", _c("pconv_dgrad_acc", "fp16", "f16x3", 1, 1, 19, 96, 255, 257, 1, 0, 0)),
    ("64.g1.s4.1x4.xy.h1p.acc.bd", "hybrid", _c("pconv_dgrad_resmask", "fp16", "f16x3", 1, 1, 19, 96, 181, 182, 2, 0, 0)),
    ("64.g1.s4.1x4.xy.h1p.acc.bd", "sk", _c("pconv_dgrad_acc", "fp16", "f16x3", 1, 1, 19, 256, 91, 91, 1, 0, 0)),
    ("64.g1.s4.1x4.xy.h1p.acc.lds", "dp_only", _c("pconv_dgrad_acc", "fp16", "f16x3", 1, 1, 33, 72, 255, 257, 1, 0, 0)),
    ("64.g1.s4.1x4.xy.h1p.acc.lds", "hybrid", _c("pconv_dgrad_resmask", "fp16", "f16x3", 1, 1, 33, 72, 181, 182, 2, 0, 0)),
    ("64.g1.s4.1x4.xy.h1p.acc.lds", "sk", _c("pconv_dgrad_acc", "fp16", "f16x3", 1, 1, 19, 147, 91, 91, 1, 0, 0)),
    ("64.g1.s4.1x4.xy.h1p.set.bd", "dp_only", _c("pconv_fwd", "fp16", "f16x3", 1, 1, 96, 19, 255, 257, 1, 0, 0)),
    ("64.g1.s4.1x4.xy.h1p.set.bd", "hybrid", _c("pconv_dgrad", "fp16", "f16x3", 1, 1, 19, 96, 219, 301, 1, 0, 0)),
    ("64.g1.s4.1x4.xy.h1p.set.bd", "sk", _c("dconv_fwd", "fp16", "f16x3", 1, 1, 96, 19, 25, 33, 2, 2, 0)),
    ("64.g1.s4.1x4.xy.h1p.set.lds", "dp_only", _c("dconv_fwd", "fp16", "f16x3", 1, 1, 8, 33, 181, 181, 2, 2, 0)),
    ("64.g1.s4.1x4.xy.h1p.set.lds", "hybrid", _c("dconv_dgrad", "fp16", "f16x3", 1, 1, 33, 8, 181, 182, 2, 2, 0)),
    ("64.g1.s4.1x4.xy.h1p.set.lds", "sk", _c("dconv_fwd", "fp16", "f16x3", 1, 1, 8, 33, 45, 91, 2, 2, 0)),
    ("64.g1.s4.1x4.xy.h3p.acc.bd", "dp_only", _c("pconv_dgrad_acc", "fp32", "f16x3", 1, 1, 19, 96, 255, 257, 1, 0, 0)),
    ("64.g1.s4.1x4.xy.h3p.acc.bd", "hybrid", _c("pconv_dgrad_resmask", "fp32", "f16x3", 1, 1, 19, 96, 181, 182, 2, 0, 0)),
    ("64.g1.s4.1x4.xy.h3p.acc.bd", "sk", _c("pconv_dgrad_acc", "fp32", "f16x3", 1, 1, 19, 256, 91, 91, 1, 0, 0)),
    ("64.g1.s4.1x4.xy.h3p.acc.lds", "dp_only", _c("pconv_dgrad_acc", "fp32", "f16x3", 1, 1, 33, 72, 255, 257, 1, 0, 0)),
    ("64.g1.s4.1x4.xy.h3p.acc.lds", "hybrid", _c("pconv_dgrad_resmask", "fp32", "f16x3", 1, 1, 33, 72, 181, 182, 2, 0, 0)),
    ("64.g1.s4.1x4.xy.h3p.acc.lds", "sk", _c("pconv_dgrad_acc", "fp32", "f16x3", 1, 1, 19, 147, 91, 91, 1, 0, 0)),
    ("64.g1.s4.1x4.xy.h3p.set.bd", "dp_only", _c("pconv_fwd", "fp32", "f16x3", 1, 1, 96, 19, 255, 257, 1, 0, 0)),
    ("64.g1.s4.1x4.xy.h3p.set.bd", "hybrid", _c("pconv_dgrad", "fp32", "f16x3", 1, 1, 19, 96, 219, 301, 1, 0, 0)),
    ("64.g1.s4.1x4.xy.h3p.set.bd", "sk", _c("dconv_fwd", "fp32", "f16x3", 1, 1, 96, 19, 25, 33, 2, 2, 0)),
    ("64.g1.s4.1x4.xy.h3p.set.lds", "dp_only", _c("dconv_fwd", "fp32", "f16x3", 1, 1, 8, 33, 181, 181, 2, 2, 0)),
    ("64.g1.s4.1x4.xy.h3p.set.lds", "hybrid", _c("dconv_dgrad", "fp32", "f16x3", 1, 1, 33, 8, 181, 182, 2, 2, 0)),
    ("64.g1.s4.1x4.xy.h3p.set.lds", "sk", _c("dconv_fwd", "fp32", "f16x3", 1, 1, 8, 33, 45, 91, 2, 2, 0)),
    ("64.g2.s2.2x2.xy.bf16.set.lds", "dp_only", _c("pconv_fwd", "bf16", "f16x3", 1, 1, 96, 33, 255, 257, 1, 0, 0)),
    ("64.g2.s2.2x2.xy.bf16.set.lds", "hybrid", _c("pconv_dgrad", "bf16", "f16x3", 1, 1, 33, 96, 219, 301, 1, 0, 0)),
    ("64.g2.s2.2x2.xy.bf16.set.lds", "sk", _c("dconv_fwd", "bf16", "f16x3", 1, 2, 8, 33, 45, 91, 2, 2, 5)),
    ("64.g2.s2.2x2.xy.f32.acc.lds", "dp_only", _c("pconv_dgrad_acc", "fp32", "mfma_f32", 1, 1, 33, 96, 255, 257, 1, 0, 0)),
    ("64.g2.s2.2x2.xy.f32.acc.lds", "hybrid", _c("pconv_dgrad_resmask", "fp32", "mfma_f32", 1, 1, 33, 96, 181, 182, 2, 0, 0)),
    ("64.g2.s2.2x2.xy.f32.acc.lds", "sk", _c("pconv_dgrad_acc", "fp32", "mfma_f32", 1, 1, 33, 256, 91, 91, 1, 0, 0)),
    ("64.g2.s2.2x2.xy.f32.set.lds", "dp_only", _c("pconv_fwd", "fp32", "mfma_f32", 1, 1, 96, 33, 255, 257, 1, 0, 0)),
    ("64.g2.s2.2x2.xy.f32.set.lds", "hybrid", _c("pconv_dgrad", "fp32", "mfma_f32", 1, 1, 33, 96, 219, 301, 1, 0, 0)),
    ("64.g2.s2.2x2.xy.f32.set.lds", "sk", _c("dconv_fwd", "fp32", "mfma_f32", 1, 2, 8, 33, 45, 91, 2, 2, 5)),
    ("tile", "tile_single", _c("pconv_fwd", "fp32", "f16x3", 1, 1, 8, 19, 25, 67, 1, 0, 0)),
    ("tile", "tile_split", _c("dconv_fwd", "fp32", "f16x3", 1, 1, 8, 19, 25, 33, 2, 2, 0)),
    ("128.g1.s3.2x2.xy.bf16.set.lds", "sk", _c("dconv_fwd", "bf16", "f16x3", 1, 1, 72, 65, 9, 187, 1, 12, 0)),
    ("128.g1.s3.2x2.xy.bf16.set.lds", "sk", _c("dconv_dgrad", "bf16", "f16x3", 1, 1, 65, 72, 119, 7, 2, 9, 0)),
    ("128.g1.s3.2x2.xy.f32.set.lds", "sk", _c("dconv_fwd", "fp32", "mfma_f32", 1, 1, 72, 65, 9, 187, 1, 12, 0)),
    ("128.g1.s3.2x2.xy.f32.set.lds", "sk", _c("dconv_dgrad", "fp32", "mfma_f32", 1, 1, 65, 72, 119, 7, 2, 9, 0)),
    ("128.g1.s4.1x4.xy.h1p.set.bd", "sk", _c("dconv_fwd", "fp16", "f16x3", 1, 1, 80, 65, 9, 187, 1, 12, 0)),
    ("128.g1.s4.1x4.xy.h1p.set.bd", "sk", _c("dconv_dgrad", "fp16", "f16x3", 1, 1, 65, 80, 119, 7, 2, 9, 0)),
    ("128.g1.s4.1x4.xy.h1p.set.bp", "sk", _c("dconv_fwd", "fp16", "f16x3", 1, 1, 72, 131, 9, 187, 1, 12, 0)),
    ("128.g1.s4.1x4.xy.h1p.set.bp", "sk", _c("dconv_dgrad", "fp16", "f16x3", 1, 1, 131, 72, 119, 7, 2, 9, 0)),
    ("128.g1.s4.1x4.xy.h1p.set.lds", "sk", _c("dconv_fwd", "fp16", "f16x3", 1, 1, 72, 65, 9, 187, 1, 12, 0)),
    ("128.g1.s4.1x4.xy.h1p.set.lds", "sk", _c("dconv_dgrad", "fp16", "f16x3", 1, 1, 65, 72, 119, 7, 2, 9, 0)),
    ("128.g1.s4.1x4.xy.h3p.set.bd", "sk", _c("dconv_fwd", "fp32", "f16x3", 1, 1, 80, 65, 9, 187, 1, 12, 0)),
    ("128.g1.s4.1x4.xy.h3p.set.bd", "sk", _c("dconv_dgrad", "fp32", "f16x3", 1, 1, 65, 80, 119, 7, 2, 9, 0)),
    ("128.g1.s4.1x4.xy.h3p.set.bp", "sk", _c("dconv_fwd", "fp32", "f16x3", 1, 1, 8, 1024, 9, 187, 1, 12, 0)),
    ("128.g1.s4.1x4.xy.h3p.set.bp", "sk", _c("dconv_dgrad", "fp32", "f16x3", 1, 1, 1024, 8, 119, 7, 2, 9, 0)),
    ("128.g1.s4.1x4.xy.h3p.set.lds", "sk", _c("dconv_fwd", "fp32", "f16x3", 1, 1, 72, 65, 9, 187, 1, 12, 0)),
    ("128.g1.s4.1x4.xy.h3p.set.lds", "sk", _c("dconv_dgrad", "fp32", "f16x3", 1, 1, 65, 72, 119, 7, 2, 9, 0)),
    ("128.g1.s4.2x2.xy.x6p.set.lds", "sk", _c("dconv_fwd", "fp32", "bf16x6", 1, 1, 72, 65, 9, 187, 1, 12, 0)),
    ("128.g1.s4.2x2.xy.x6p.set.lds", "sk", _c("dconv_dgrad", "fp32", "bf16x6", 1, 1, 65, 72, 119, 7, 2, 9, 0)),
    ("128.g2.s2.2x2.xy.bf16.set.lds", "sk", _c("dconv_fwd", "bf16", "f16x3", 1, 2, 72, 65, 9, 187, 1, 12, 15)),
    ("128.g2.s2.2x2.xy.bf16.set.lds", "sk", _c("dconv_dgrad", "bf16", "f16x3", 1, 2, 65, 72, 119, 7, 2, 9, 12)),
    ("128.g2.s2.2x2.xy.f32.set.lds", "sk", _c("dconv_fwd", "fp32", "mfma_f32", 1, 2, 72, 65, 9, 187, 1, 12, 15)),
    ("128.g2.s2.2x2.xy.f32.set.lds", "sk", _c("dconv_dgrad", "fp32", "mfma_f32", 1, 2, 65, 72, 119, 7, 2, 9, 12)),
    ("32.g2.s2.1x4.xy.bf16.set.lds", "sk", _c("dconv_fwd", "bf16", "f16x3", 1, 2, 72, 19, 9, 187, 1, 12, 15)),
    ("32.g2.s2.1x4.xy.bf16.set.lds", "sk", _c("dconv_dgrad", "bf16", "f16x3", 1, 2, 19, 72, 119, 7, 2, 9, 12)),
    ("32.g2.s2.1x4.xy.f32.set.lds", "sk", _c("dconv_fwd", "fp32", "mfma_f32", 1, 2, 72, 19, 9, 187, 1, 12, 15)),
    ("32.g2.s2.1x4.xy.f32.set.lds", "sk", _c("dconv_dgrad", "fp32", "mfma_f32", 1, 2, 19, 72, 119, 7, 2, 9, 12)),
    ("64.g1.s3.2x2.xy.bf16.set.lds", "sk", _c("dconv_fwd", "bf16", "f16x3", 1, 1, 72, 33, 9, 187, 1, 12, 0)),
    ("64.g1.s3.2x2.xy.bf16.set.lds", "sk", _c("dconv_dgrad", "bf16", "f16x3", 1, 1, 33, 72, 119, 7, 2, 9, 0)),
    ("64.g1.s3.2x2.xy.f32.set.lds", "sk", _c("dconv_fwd", "fp32", "mfma_f32", 1, 1, 72, 33, 9, 187, 1, 12, 0)),
    ("64.g1.s3.2x2.xy.f32.set.lds", "sk", _c("dconv_dgrad", "fp32", "mfma_f32", 1, 1, 33, 72, 119, 7, 2, 9, 0)),
    ("64.g1.s4.1x4.xy.h1p.set.bd", "sk", _c("dconv_fwd", "fp16", "f16x3", 1, 1, 96, 19, 9, 187, 1, 12, 0)),
    ("64.g1.s4.1x4.xy.h1p.set.bd", "sk", _c("dconv_dgrad", "fp16", "f16x3", 1, 1, 19, 96, 119, 7, 2, 9, 0)),
    ("64.g1.s4.1x4.xy.h1p.set.lds", "sk", _c("dconv_fwd", "fp16", "f16x3", 1, 1, 72, 33, 9, 187, 1, 12, 0)),
    ("64.g1.s4.1x4.xy.h1p.set.lds", "sk", _c("dconv_dgrad", "fp16", "f16x3", 1, 1, 33, 72, 119, 7, 2, 9, 0)),
    ("64.g1.s4.1x4.xy.h3p.set.bd", "sk", _c("dconv_fwd", "fp32", "f16x3", 1, 1, 96, 19, 9, 187, 1, 12, 0)),
    ("64.g1.s4.1x4.xy.h3p.set.bd", "sk", _c("dconv_dgrad", "fp32", "f16x3", 1, 1, 19, 96, 119, 7, 2, 9, 0)),
    ("64.g1.s4.1x4.xy.h3p.set.lds", "sk", _c("dconv_fwd", "fp32", "f16x3", 1, 1, 72, 33, 9, 187, 1, 12, 0)),
    ("64.g1.s4.1x4.xy.h3p.set.lds", "sk", _c("dconv_dgrad", "fp32", "f16x3", 1, 1, 33, 72, 119, 7, 2, 9, 0)),
    ("64.g2.s2.2x2.xy.bf16.set.lds", "sk", _c("dconv_fwd", "bf16", "f16x3", 1, 2, 72, 33, 9, 187, 1, 12, 15)),
    ("64.g2.s2.2x2.xy.bf16.set.lds", "sk", _c("dconv_dgrad", "bf16", "f16x3", 1, 2, 33, 72, 119, 7, 2, 9, 12)),
    ("64.g2.s2.2x2.xy.f32.set.lds", "sk", _c("dconv_fwd", "fp32", "mfma_f32", 1, 2, 72, 33, 9, 187, 1, 12, 15)),
    ("64.g2.s2.2x2.xy.f32.set.lds", "sk", _c("dconv_dgrad", "fp32", "mfma_f32", 1, 2, 33, 72, 119, 7, 2, 9, 12)),
    ("32.g2.s2.1x4.xy.bf16.set.lds", "sk", _c("pconv_dgrad", "bf16", "f16x3", 0, 1, 19, 96, 219, 301, 1, 0, 0)),
    ("32.g2.s2.1x4.xy.f32.acc.lds", "sk", _c("pconv_dgrad_resmask", "fp32", "mfma_f32", 0, 1, 19, 96, 181, 182, 2, 0, 0)),
    ("64.g1.s4.1x4.xy.h1p.acc.bd", "sk", _c("pconv_dgrad_resmask", "fp16", "f16x3", 0, 1, 19, 96, 181, 182, 2, 0, 0)),
    ("64.g1.s4.1x4.xy.h3p.acc.bd", "sk", _c("pconv_dgrad_resmask", "fp32", "f16x3", 0, 1, 19, 96, 181, 182, 2, 0, 0)),
]
