"""The BatchNorm cases shared by the CPU gate (test_bn_forms.py) and the fp64 parity test (test_gpu_bn_forms.py):
plain data and helpers, no fixtures.

csrc/bn.hip sends every BN call to one of 13 fused instantiations (k_bn_fwd_fused / k_bn_bwd_fused at 4, 9, 16 and
33 elements per lane, the joint two-image forms among them) or to the flat kernels in their float4 or scalar
alignment, by thresholds in p, c and nimg; what a kernel does then depends on which pointers the call gives.  The
library answers which kernel through msl_bn_plan (host only, the functions the launch itself calls).  A case here
is one call of a C-ABI entry point with its options, filed under the kernel key, shape class and image class the
query says it runs; GRID is the sweep the gate holds the table against.
"""
import itertools
from collections import namedtuple

MSL_OK, MSL_ERR_WORKSPACE, MSL_ERR_ARG = 0, -2, -3
CASE_MAX_ELEMS = 9_000_000  # c * nimg * p of a case (the forward fused.16 loop2 cases: 257 x 2 x 16384)

# dir: "fwd" (msl_bn_fwd_mask) or "bwd" (msl_bn_bwd_am / _am_beta / _mask by `src`); bn_fused: msl_forms.bn_fused;
# aligned 0: every tensor operand from a buffer sliced at [1:], 4 bytes off 16-byte alignment; far: x = 3 randn + 40
# (the cancellation case), else 3 randn + 1.
# Forward options: relu, residual, affine (gamma and beta given, else both NULL), absmax, mask (the ReLU bits), upd
# (update_running), nbt (num_batches_tracked given).
# Backward options: src (the ReLU source: none = no ReLU, y, bits, recompute), residual (the forward had one; never
# with recompute), affine (gamma - and beta for recompute - given), dx, dres, dparams (dgamma and dbeta given), acc
# (accumulate_params, onto random previous contents), absmax (absmax_dx).
Case = namedtuple("Case", "dir c nimg p training bn_fused aligned far relu residual affine absmax mask upd nbt src dx "
                          "dres dparams acc")

FWD_KEYS = ("fused.4", "fused.9", "fused.16", "fused.33", "joint.4", "joint.9", "joint.16", "flat.train.vec",
            "flat.train.scalar", "flat.eval.vec", "flat.eval.scalar")
BWD_KEYS = tuple(k for k in FWD_KEYS if k != "joint.16")  # kBnJoint16Bwd is false: that instantiation is not built
ALL_KEYS = tuple("fwd:" + k for k in FWD_KEYS) + tuple("bwd:" + k for k in BWD_KEYS)  # 21
PREV_BLOCKS = {4: 0, 9: 4, 16: 9, 33: 16}  # the 1024-element blocks of the next smaller form
FUSED_SHAPES = ("low", "full", "ragged")
FLAT_SHAPES = ("single", "split", "s16", "rows", "shrunk")
SOURCES = ("none", "y", "bits", "recompute")


def F(c, nimg, p, training=1, bn_fused=1, aligned=1, far=0, relu=0, residual=0, affine=1, absmax=0, mask=0, upd=1,
      nbt=1):
    return Case("fwd", c, nimg, p, training, bn_fused, aligned, far, relu, residual, affine, absmax, mask, upd, nbt,
                "none", 0, 0, 0, 0)


def B(c, nimg, p, training=1, bn_fused=1, aligned=1, far=0, src="none", residual=0, affine=1, absmax=0, dx=1, dres=0,
      dparams=1, acc=0):
    return Case("bwd", c, nimg, p, training, bn_fused, aligned, far, int(src != "none"), residual, affine, absmax, 0, 0,
                0, src, dx, dres, dparams, acc)


def elems(case):
    return case.c * case.nimg * case.p


def entry_of(src):
    """The backward entry point a ReLU source goes through."""
    return {"bits": "mask", "recompute": "am_beta"}.get(src, "am")


def plan_of(hip, case, src=None, ws_bytes=None):
    """The library's plan of the case (hip.BnPlan) under the case's own forms; src: another ReLU source."""
    forms = hip.Forms(5, 1, 1, case.bn_fused)
    if case.dir == "fwd":
        return hip.bn_plan(0, case.c, case.p, case.nimg, case.training, case.relu, case.aligned, has_absmax=case.absmax,
                           has_mask=case.mask, ws_bytes=ws_bytes, forms_=forms)
    src = case.src if src is None else src
    return hip.bn_plan(1, case.c, case.p, case.nimg, case.training, int(src != "none"), case.aligned, entry_of(src), src,
                       case.dx, case.absmax, 0, ws_bytes=ws_bytes, forms_=forms)


def plan_key(case, pl):
    if pl.fused:
        return "%s:%s.%d" % (case.dir, "joint" if pl.joint else "fused", pl.ept)
    return "%s:flat.%s.%s" % (case.dir, "train" if case.training else "eval", "vec" if pl.vec else "scalar")


def shape_class(case, pl):
    """The class of the row length p under the plan; "other" needs no case of its own.
    fused / joint: low (the first element of the form's last block; at 4 elements a row under one wave), full,
    ragged (strictly inside, p no multiple of 4 or 64).  flat: s16 (16 statistics parts), split (2..15 parts),
    shrunk (bn_flat_chunk halved the chunk: p <= 16), rows (a block stages 4 rows or more), single (one part, p at
    least a chunk)."""
    p = case.p
    if pl.fused:
        lo, hi = PREV_BLOCKS[pl.ept] * 1024 + 1, pl.ept * 1024
        if p == hi:
            return "full"
        if p == lo or (pl.ept == 4 and p <= 63):
            return "low"
        if lo < p < hi and p % 64 and p % 4:
            return "ragged"
        return "other"
    if pl.S == 16:
        return "s16"
    if pl.S > 1:
        return "split"
    if pl.chunk < 4096:
        return "shrunk"
    if pl.max_rows >= 4:
        return "rows"
    return "single" if p >= pl.chunk else "other"


def image_class(case, pl):
    if pl.fused:
        return "pair" if pl.joint else ("one", "loop2", "loop3")[case.nimg - 1]
    return "img%d" % case.nimg


def option_values(case, key):
    """{(option, value)} the case covers for its key."""
    fused = "flat" not in key
    if case.dir == "fwd":
        names = ["residual", "relu", "absmax", "upd", "affine", "nbt"] + (["mask"] if fused else [])
        return {(n, getattr(case, n)) for n in names}
    return {(n, getattr(case, n)) for n in ("src", "dx", "dres", "dparams", "acc", "absmax", "affine")}


def options_needed(key):
    """{(option, value)} every key needs across its cases: both values of each flag, every ReLU source it takes."""
    d, k = key.split(":")
    fused = "flat" not in k
    if d == "fwd":
        names = ["residual", "relu", "absmax", "upd", "affine", "nbt"] + (["mask"] if fused else [])
        return {(n, v) for n in names for v in (0, 1)}
    srcs = ["none", "y"] + (["bits"] if fused else []) + (["recompute"] if fused and not k.endswith(".33") else [])
    need = {(n, v) for n in ("dx", "dres", "dparams", "acc", "absmax", "affine") for v in (0, 1)}
    return need | {("src", s) for s in srcs}


# ------------------------------------------------------------------------------------------ the grid
GRID_C = (1, 3, 127, 128, 256, 257, 300)
# both sides of every threshold (4096 | 4097, 9216 | 9217, 16384 | 16385, 33792 | 33793; bn_splits at 8192 | 8193;
# bn_flat_chunk at 16 | 17), rows under a wave (1, 5, 37, 63), ragged rows inside each form (2145, 6001, 12345,
# 20001) and the 16-part row (122881, at c = 1 only)
GRID_P = (1, 5, 16, 17, 37, 63, 2145, 4096, 4097, 6001, 8193, 9216, 9217, 12345, 16384, 16385, 20001, 33792, 33793,
          122881)


def grid():
    for d, c, p, nimg, tr, fu, al in itertools.product(("fwd", "bwd"), GRID_C, GRID_P, (1, 2, 3), (0, 1), (0, 1), (0, 1)):
        if c * nimg * p > CASE_MAX_ELEMS or (p == 122881 and c > 1):
            continue
        yield (F if d == "fwd" else B)(c, nimg, p, training=tr, bn_fused=fu, aligned=al)


def reached(hip, cases):
    """{(key, shape class): [cases]} and {(key, image class): [cases]} over `cases`, by the library's plan."""
    shapes, images = {}, {}
    for cs in cases:
        pl = plan_of(hip, cs)
        assert pl.status == MSL_OK, cs
        key = plan_key(cs, pl)
        shapes.setdefault((key, shape_class(cs, pl)), []).append(cs)
        images.setdefault((key, image_class(cs, pl)), []).append(cs)
    return shapes, images


def suggest(cases):
    """The cheapest grid point of a (key, class) the table lacks."""
    return min(cases, key=elems)


def case_id(key, shape, image, c):
    if c.dir == "fwd":
        opts = "r%dres%da%dam%dm%du%dn%d" % (c.relu, c.residual, c.affine, c.absmax, c.mask, c.upd, c.nbt)
    else:
        opts = "%s-res%da%dam%ddx%ddr%ddp%dacc%d" % (c.src, c.residual, c.affine, c.absmax, c.dx, c.dres, c.dparams, c.acc)
    return "%s-%s-%s-%dx%dx%d-t%df%dal%dfar%d-%s" % (key, shape, image, c.c, c.nimg, c.p, c.training, c.bn_fused, c.aligned,
                                                   c.far, opts)


# ------------------------------------------------------------------------------------------ the table
# (key, shape class, image class, Case): per key every shape class and image class the grid reaches, the options
# cycled so that every key sees every value of every option (pairwise, no cross product).
TABLE = [
    ("fwd:fused.4", "low", "loop2", F(257, 2, 5, relu=1, residual=1, absmax=1, mask=1)),
    ("fwd:fused.4", "full", "loop3", F(3, 3, 4096, far=1, affine=0, upd=0, nbt=0)),
    ("fwd:fused.4", "ragged", "one", F(3, 1, 2145, relu=1, mask=1, nbt=0)),
    ("fwd:fused.4", "low", "loop2", F(257, 2, 5, aligned=0, far=1, relu=1, residual=1, affine=0, absmax=1, upd=0)),
    ("fwd:fused.4", "low", "one", F(3, 1, 37, relu=1, residual=1, absmax=1, mask=1)),
    ("fwd:fused.4", "low", "loop3", F(3, 3, 1, far=1, affine=0, upd=0, nbt=0)),
    ("fwd:fused.9", "low", "loop2", F(257, 2, 4097, relu=1, residual=1, absmax=1, mask=1)),
    ("fwd:fused.9", "full", "loop3", F(3, 3, 9216, far=1, affine=0, upd=0, nbt=0)),
    ("fwd:fused.9", "ragged", "one", F(3, 1, 6001, relu=1, mask=1, nbt=0)),
    ("fwd:fused.9", "low", "loop2", F(257, 2, 4097, aligned=0, far=1, relu=1, residual=1, affine=0, absmax=1, upd=0)),
    ("fwd:fused.16", "low", "loop2", F(257, 2, 9217, relu=1, residual=1, absmax=1, mask=1)),
    ("fwd:fused.16", "full", "loop3", F(3, 3, 16384, far=1, affine=0, upd=0, nbt=0)),
    ("fwd:fused.16", "ragged", "one", F(3, 1, 12345, relu=1, mask=1, nbt=0)),
    ("fwd:fused.16", "low", "loop2", F(257, 2, 9217, aligned=0, far=1, relu=1, residual=1, affine=0, absmax=1, upd=0)),
    ("fwd:fused.33", "low", "loop2", F(128, 2, 16385, relu=1, residual=1, absmax=1, mask=1)),
    ("fwd:fused.33", "full", "one", F(128, 1, 33792, far=1, affine=0, upd=0, nbt=0)),
    ("fwd:fused.33", "low", "loop3", F(128, 3, 16385, relu=1, mask=1, nbt=0)),
    ("fwd:fused.33", "ragged", "one", F(128, 1, 20001, far=1, relu=1, residual=1, affine=0, absmax=1, upd=0)),
    ("fwd:fused.33", "low", "loop2", F(128, 2, 16385, aligned=0, relu=1, residual=1, absmax=1, mask=1)),
    ("fwd:joint.4", "low", "pair", F(3, 2, 5, relu=1, residual=1, absmax=1, mask=1)),
    ("fwd:joint.4", "full", "pair", F(3, 2, 4096, far=1, affine=0, upd=0, nbt=0)),
    ("fwd:joint.4", "ragged", "pair", F(3, 2, 2145, relu=1, mask=1, nbt=0)),
    ("fwd:joint.4", "low", "pair", F(3, 2, 5, aligned=0, far=1, relu=1, residual=1, affine=0, absmax=1, upd=0)),
    ("fwd:joint.4", "ragged", "pair", F(256, 2, 2145, relu=1, residual=1, absmax=1, mask=1)),
    ("fwd:joint.4", "low", "pair", F(1, 2, 1, far=1, affine=0, upd=0, nbt=0)),
    ("fwd:joint.9", "low", "pair", F(3, 2, 4097, relu=1, residual=1, absmax=1, mask=1)),
    ("fwd:joint.9", "full", "pair", F(3, 2, 9216, far=1, affine=0, upd=0, nbt=0)),
    ("fwd:joint.9", "ragged", "pair", F(3, 2, 6001, relu=1, mask=1, nbt=0)),
    ("fwd:joint.9", "low", "pair", F(3, 2, 4097, aligned=0, far=1, relu=1, residual=1, affine=0, absmax=1, upd=0)),
    ("fwd:joint.9", "ragged", "pair", F(256, 2, 6001, relu=1, residual=1, absmax=1, mask=1)),
    ("fwd:joint.9", "low", "pair", F(1, 2, 4097, far=1, affine=0, upd=0, nbt=0)),
    ("fwd:joint.16", "low", "pair", F(3, 2, 9217, relu=1, residual=1, absmax=1, mask=1)),
    ("fwd:joint.16", "full", "pair", F(3, 2, 16384, far=1, affine=0, upd=0, nbt=0)),
    ("fwd:joint.16", "ragged", "pair", F(3, 2, 12345, relu=1, mask=1, nbt=0)),
    ("fwd:joint.16", "low", "pair", F(3, 2, 9217, aligned=0, far=1, relu=1, residual=1, affine=0, absmax=1, upd=0)),
    ("fwd:joint.16", "ragged", "pair", F(256, 2, 12345, relu=1, residual=1, absmax=1, mask=1)),
    ("fwd:joint.16", "low", "pair", F(1, 2, 9217, far=1, affine=0, upd=0, nbt=0)),
    ("fwd:flat.train.vec", "single", "img1", F(3, 1, 4096, bn_fused=0, relu=1, residual=1, absmax=1)),
    ("fwd:flat.train.vec", "split", "img2", F(3, 2, 8193, bn_fused=0, far=1, affine=0, upd=0, nbt=0)),
    ("fwd:flat.train.vec", "s16", "img3", F(2, 3, 122881, bn_fused=0, relu=1, nbt=0)),
    ("fwd:flat.train.vec", "rows", "img1", F(300, 1, 63, bn_fused=0, far=1, relu=1, residual=1, affine=0, absmax=1, upd=0)),
    ("fwd:flat.train.vec", "shrunk", "img2", F(256, 2, 5, bn_fused=0, relu=1, residual=1, absmax=1)),
    ("fwd:flat.train.scalar", "single", "img1", F(3, 1, 4096, bn_fused=0, aligned=0, relu=1, residual=1, absmax=1)),
    ("fwd:flat.train.scalar", "split", "img2", F(3, 2, 8193, bn_fused=0, aligned=0, far=1, affine=0, upd=0, nbt=0)),
    ("fwd:flat.train.scalar", "s16", "img3", F(2, 3, 122881, bn_fused=0, aligned=0, relu=1, nbt=0)),
    ("fwd:flat.train.scalar", "rows", "img1", F(300, 1, 63, bn_fused=0, aligned=0, far=1, relu=1, residual=1, affine=0, absmax=1, upd=0)),
    ("fwd:flat.train.scalar", "shrunk", "img2", F(256, 2, 5, bn_fused=0, aligned=0, relu=1, residual=1, absmax=1)),
    ("fwd:flat.eval.vec", "single", "img1", F(3, 1, 4096, training=0, bn_fused=0, relu=1, residual=1, absmax=1)),
    ("fwd:flat.eval.vec", "split", "img2", F(3, 2, 8193, training=0, bn_fused=0, far=1, affine=0, upd=0, nbt=0)),
    ("fwd:flat.eval.vec", "s16", "img3", F(2, 3, 122881, training=0, bn_fused=0, relu=1, nbt=0)),
    ("fwd:flat.eval.vec", "rows", "img1", F(300, 1, 63, training=0, bn_fused=0, far=1, relu=1, residual=1, affine=0, absmax=1, upd=0)),
    ("fwd:flat.eval.vec", "shrunk", "img2", F(256, 2, 5, training=0, bn_fused=0, relu=1, residual=1, absmax=1)),
    ("fwd:flat.eval.scalar", "single", "img1", F(3, 1, 4096, training=0, bn_fused=0, aligned=0, relu=1, residual=1, absmax=1)),
    ("fwd:flat.eval.scalar", "split", "img2", F(3, 2, 8193, training=0, bn_fused=0, aligned=0, far=1, affine=0, upd=0, nbt=0)),
    ("fwd:flat.eval.scalar", "s16", "img3", F(2, 3, 122881, training=0, bn_fused=0, aligned=0, relu=1, nbt=0)),
    ("fwd:flat.eval.scalar", "rows", "img1", F(300, 1, 63, training=0, bn_fused=0, aligned=0, far=1, relu=1, residual=1, affine=0, absmax=1, upd=0)),
    ("fwd:flat.eval.scalar", "shrunk", "img2", F(256, 2, 5, training=0, bn_fused=0, aligned=0, relu=1, residual=1, absmax=1)),
    ("bwd:fused.4", "low", "loop2", B(257, 2, 5, absmax=1)),
    ("bwd:fused.4", "full", "loop3", B(3, 3, 4096, far=1, affine=0, src="y", dx=0, dres=1, dparams=0, acc=1)),
    ("bwd:fused.4", "ragged", "one", B(3, 1, 2145, src="bits", dres=1, acc=1)),
    ("bwd:fused.4", "low", "loop2", B(257, 2, 5, aligned=0, far=1, affine=0, absmax=1, src="recompute", dres=1)),
    ("bwd:fused.4", "low", "one", B(3, 1, 37, absmax=1)),
    ("bwd:fused.4", "low", "loop3", B(3, 3, 1, far=1, src="y", dx=0, dres=1, dparams=0, acc=1)),
    ("bwd:fused.9", "low", "loop2", B(257, 2, 4097, absmax=1)),
    ("bwd:fused.9", "full", "loop3", B(3, 3, 9216, far=1, affine=0, src="y", dx=0, dres=1, dparams=0, acc=1)),
    ("bwd:fused.9", "ragged", "one", B(3, 1, 6001, src="bits", dres=1, acc=1)),
    ("bwd:fused.9", "low", "loop2", B(257, 2, 4097, aligned=0, far=1, affine=0, absmax=1, src="recompute", dres=1)),
    ("bwd:fused.16", "low", "loop2", B(3, 2, 9217, absmax=1)),
    ("bwd:fused.16", "full", "loop3", B(3, 3, 16384, far=1, affine=0, src="y", dx=0, dres=1, dparams=0, acc=1)),
    ("bwd:fused.16", "ragged", "one", B(3, 1, 12345, src="bits", dres=1, acc=1)),
    ("bwd:fused.16", "low", "loop2", B(3, 2, 9217, aligned=0, far=1, affine=0, absmax=1, src="recompute", dres=1)),
    ("bwd:fused.33", "low", "loop2", B(128, 2, 16385, absmax=1)),
    ("bwd:fused.33", "full", "one", B(128, 1, 33792, far=1, affine=0, src="y", dx=0, dres=1, dparams=0, acc=1)),
    ("bwd:fused.33", "low", "loop3", B(128, 3, 16385, src="bits", dres=1, acc=1)),
    ("bwd:fused.33", "ragged", "one", B(128, 1, 20001, far=1, affine=0, absmax=1, dres=1)),
    ("bwd:fused.33", "low", "loop2", B(128, 2, 16385, aligned=0, absmax=1, src="y")),
    ("bwd:joint.4", "low", "pair", B(3, 2, 5, absmax=1)),
    ("bwd:joint.4", "full", "pair", B(3, 2, 4096, far=1, affine=0, src="y", dx=0, dres=1, dparams=0, acc=1)),
    ("bwd:joint.4", "ragged", "pair", B(3, 2, 2145, src="bits", dres=1, acc=1)),
    ("bwd:joint.4", "low", "pair", B(3, 2, 5, aligned=0, far=1, affine=0, absmax=1, src="recompute", dres=1)),
    ("bwd:joint.4", "ragged", "pair", B(256, 2, 2145, absmax=1)),
    ("bwd:joint.4", "low", "pair", B(1, 2, 1, far=1, src="y", dx=0, dres=1, dparams=0, acc=1)),
    ("bwd:joint.9", "low", "pair", B(3, 2, 4097, absmax=1)),
    ("bwd:joint.9", "full", "pair", B(3, 2, 9216, far=1, affine=0, src="y", dx=0, dres=1, dparams=0, acc=1)),
    ("bwd:joint.9", "ragged", "pair", B(3, 2, 6001, src="bits", dres=1, acc=1)),
    ("bwd:joint.9", "low", "pair", B(3, 2, 4097, aligned=0, far=1, affine=0, absmax=1, src="recompute", dres=1)),
    ("bwd:joint.9", "ragged", "pair", B(256, 2, 6001, absmax=1)),
    ("bwd:joint.9", "low", "pair", B(1, 2, 4097, far=1, affine=0, src="y", dx=0, dres=1, dparams=0, acc=1)),
    ("bwd:flat.train.vec", "single", "img1", B(3, 1, 4096, bn_fused=0, absmax=1)),
    ("bwd:flat.train.vec", "split", "img2", B(3, 2, 8193, bn_fused=0, far=1, affine=0, src="y", dx=0, dres=1, dparams=0, acc=1)),
    ("bwd:flat.train.vec", "s16", "img3", B(2, 3, 122881, bn_fused=0, dres=1, acc=1)),
    ("bwd:flat.train.vec", "rows", "img1", B(300, 1, 63, bn_fused=0, far=1, residual=1, affine=0, absmax=1, src="y", dres=1)),
    ("bwd:flat.train.vec", "shrunk", "img2", B(256, 2, 5, bn_fused=0, absmax=1)),
    ("bwd:flat.train.scalar", "single", "img1", B(3, 1, 4096, bn_fused=0, aligned=0, absmax=1)),
    ("bwd:flat.train.scalar", "split", "img2", B(3, 2, 8193, bn_fused=0, aligned=0, far=1, affine=0, src="y", dx=0, dres=1, dparams=0, acc=1)),
    ("bwd:flat.train.scalar", "s16", "img3", B(2, 3, 122881, bn_fused=0, aligned=0, dres=1, acc=1)),
    ("bwd:flat.train.scalar", "rows", "img1", B(300, 1, 63, bn_fused=0, aligned=0, far=1, residual=1, affine=0, absmax=1, src="y", dres=1)),
    ("bwd:flat.train.scalar", "shrunk", "img2", B(256, 2, 5, bn_fused=0, aligned=0, absmax=1)),
    ("bwd:flat.eval.vec", "single", "img1", B(3, 1, 4096, training=0, bn_fused=0, absmax=1)),
    ("bwd:flat.eval.vec", "split", "img2", B(3, 2, 8193, training=0, bn_fused=0, far=1, affine=0, src="y", dx=0, dres=1, dparams=0, acc=1)),
    ("bwd:flat.eval.vec", "s16", "img3", B(2, 3, 122881, training=0, bn_fused=0, dres=1, acc=1)),
    ("bwd:flat.eval.vec", "rows", "img1", B(300, 1, 63, training=0, bn_fused=0, far=1, residual=1, affine=0, absmax=1, src="y", dres=1)),
    ("bwd:flat.eval.vec", "shrunk", "img2", B(256, 2, 5, training=0, bn_fused=0, absmax=1)),
    ("bwd:flat.eval.scalar", "single", "img1", B(3, 1, 4096, training=0, bn_fused=0, aligned=0, absmax=1)),
    ("bwd:flat.eval.scalar", "split", "img2", B(3, 2, 8193, training=0, bn_fused=0, aligned=0, far=1, affine=0, src="y", dx=0, dres=1, dparams=0, acc=1)),
    ("bwd:flat.eval.scalar", "s16", "img3", B(2, 3, 122881, training=0, bn_fused=0, aligned=0, dres=1, acc=1)),
    ("bwd:flat.eval.scalar", "rows", "img1", B(300, 1, 63, training=0, bn_fused=0, aligned=0, far=1, residual=1, affine=0, absmax=1, src="y", dres=1)),
    ("bwd:flat.eval.scalar", "shrunk", "img2", B(256, 2, 5, training=0, bn_fused=0, aligned=0, absmax=1)),
    # the flat kernels under bn_fused = 1: train mode past the fused shapes (c < 128 beyond 16384 px), and eval mode
    # at a size the fused kernels would take in train mode (a row length no class asks for: "other")
    ("fwd:flat.train.vec", "split", "img2", F(3, 2, 16385, relu=1, residual=1, absmax=1)),
    ("bwd:flat.train.vec", "split", "img2", B(3, 2, 16385, src="y", absmax=1, dres=1)),
    ("fwd:flat.eval.vec", "other", "img2", F(3, 2, 2145, training=0, far=1, relu=1, absmax=1)),
    ("bwd:flat.eval.vec", "other", "img2", B(3, 2, 2145, training=0, far=1, src="y", absmax=1)),
]
