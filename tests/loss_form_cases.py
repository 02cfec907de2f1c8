"""The fused-loss, upsample and resize cases shared by the CPU gate (test_loss_forms.py) and the fp64 parity test
(test_gpu_loss_forms.py): plain data and helpers, no fixtures.

csrc/loss.hip builds every loss kernel four times (MSL_DISPATCH_C: 19, 16, 13 classes and a generic 32-wide body
for every other count), splits the backward's rows into column chunks whose LDS the host sizes (rows_chunks,
rows_wmax), opts in to more than 64 KB of LDS or refuses above 160 KB, caps every flat grid (grid-stride beyond the
cap) and switches msl_resize_bilinear's kernel at ho + wo = 128.  The library answers all of that through
msl_loss_plan (host only, the functions the launches themselves call).  A case here is one operation of
maxsquareloss_amd.ops with its data recipe, filed under the name and the geometry classes the plan gives it;
grid() is the lattice the gate holds the table against.
"""
import itertools
from collections import namedtuple

import numpy as np
import torch

import loss_ref as lr

MSL_OK, MSL_ERR_SHAPE, MSL_ERR_WORKSPACE, MSL_ERR_ARG = 0, -1, -2, -3
MARGIN = 1e-4  # the least decision margin of every case, outside its deliberately tied pixels

# Gradient bars |d - ref| <= K 2^-24 A per element (loss_ref: A = Wy^T M Wx, M the pixel's coefficient).
# The upsample's K are derived: the backward's weights are exact, its sums fp64 and it rounds twice (T, then
# dlow) - 3 with the weights' own fp32 add at a clamped tap; the forward rounds twice per axis - 4.  The losses'
# K are measured, not derived: 4 x the worst ratio of torch-CPU fp32 autograd of the same operation over TABLE,
# rounded up to a power of two (profiles/loss_forms_errors.txt holds those ratios and the GPU's).
K_UPSAMPLE_BWD, K_UPSAMPLE_FWD = 3, 4
# ce's K is that large because its kind carries the 513 x 513 case, where torch's fp32 backward adds 4096 pixels per
# low-res element in fp32; the kernels add in fp64 and stay under 4 (the profile file).
K = {"ce": 512, "maxsquare": 32, "iw_maxsquare": 32, "multi_ce": 32, "entropy": 16, "iw_entropy": 32, "hard_ce": 16,
     "prob": 16, "soft": 128}

# op: up (a fused loss, forward and backward), upsample (forward and backward), resize, labels (loss_labels_up),
# pseudo (pseudo_labels_up + logits_argmax_up), prob, soft.  kind: the loss (lr.UP_KINDS; ms / iw for prob; plain /
# iw for soft), else "-".  For the flat ops the tensor is (1, c, ho, wo) and hi = wi = 1.
# data: "+"-joined tokens.  Logits: x4 (4 randn, the default scale), x40 (p rounds to 0 or 1; the second head stays
# at 4: two one-hot heads that disagree would average to a near tie at every pixel), x400 (the grid-stride cases of
# the deciding kernels: among 263 169 or 1 050 625 independent pixels only logits this far apart keep every decision
# MARGIN clear; same-size geometry, every pixel a node), solo (loss_labels_up without the second head), off (+1e4:
# the max subtraction; on same-size geometry, where the fp32 interpolation of values near 1e4 is exact), empty
# (classes 1 and c-1 never win: IW weights of empty classes), tie (two classes tied for the maximum at isolated
# low-res nodes).  CE labels:
# rand (-1 .. c-1), over (values >= c too), one (one valid pixel), first / last (one class), none (all ignored).
# prob: lab / nolab (the histogram's source).  soft: keep / part / all (the ignored share of the target) and
# di / dt / both (which gradients are asked).
Case = namedtuple("Case", "op kind c hi wi ho wo data gout thr ratio seed")

KINDS = lr.UP_KINDS
BUCKETS = (19, 16, 13, 32)
ALL_KEYS = tuple(
    ["k_loss_fwd:%s:%d" % (k, b) for k in KINDS for b in BUCKETS] +
    ["k_bwd_rows:%s:%d" % (k, b) for k in KINDS + ("upsample",) for b in BUCKETS] +
    ["k_bwd_cols:%s" % k for k in KINDS + ("upsample",)] + ["k_loss_finalize:%s" % k for k in KINDS] +
    ["k_loss_labels:%d" % b for b in BUCKETS] + ["k_pseudo_labels:%d" % b for b in BUCKETS] +
    ["k_prob_%s:%s:%d" % (d, k, b) for d in ("fwd", "bwd") for k in ("ms", "iw") for b in BUCKETS] +
    ["k_soft_%s:%s:%d" % (d, k, b) for d in ("fwd", "bwd") for k in ("plain", "iw") for b in BUCKETS] +
    ["k_upsample_fwd:vec", "k_upsample_fwd:scalar", "k_resize_four"])  # 118
GENERIC_C = (1, 2, 12, 14, 20, 32)  # class counts the generic body serves, every one with a case

AXIS = ("in1", "out1", "same", "up_pow2", "up", "down")
BWD_FAMILIES = ("up_bwd", "upsample_bwd")


def geo(case):
    return case.c, case.hi, case.wi, case.ho, case.wo


def plans(hip, case):
    """{family: LossPlan} of the library calls the case makes."""
    g = geo(case)
    fam = {"up": ("up_fwd", "up_bwd"), "upsample": ("upsample_fwd", "upsample_bwd"), "resize": ("resize",),
           "labels": ("labels",), "pseudo": ("labels",), "prob": ("prob_fwd", "prob_bwd"),
           "soft": ("soft_fwd", "soft_bwd")}[case.op]
    return {f: hip.loss_plan(f, *g) for f in fam}


def keys_of(case, pl):
    """The kernel instantiations the case runs, by the plan."""
    k = case.kind
    if case.op == "up":
        out = ["k_loss_fwd:%s:%d" % (k, pl["up_fwd"].cm), "k_loss_finalize:%s" % k]
        if pl["up_bwd"].status == MSL_OK:
            out += ["k_bwd_rows:%s:%d" % (k, pl["up_bwd"].cm), "k_bwd_cols:%s" % k]
        return out
    if case.op == "upsample":
        out = ["k_upsample_fwd:%s" % ("vec" if pl["upsample_fwd"].vec else "scalar")]
        if pl["upsample_bwd"].status == MSL_OK:
            out += ["k_bwd_rows:upsample:%d" % pl["upsample_bwd"].cm, "k_bwd_cols:upsample"]
        return out
    if case.op == "resize":
        p = pl["resize"]
        return ["k_resize_four"] if p.four_tap else ["k_upsample_fwd:%s" % ("vec" if p.vec else "scalar")]
    if case.op == "labels":
        return ["k_loss_labels:%d" % pl["labels"].cm]
    if case.op == "pseudo":
        return ["k_pseudo_labels:%d" % pl["labels"].cm]
    if case.op == "prob":
        fin = "k_loss_finalize:%s" % ("maxsquare" if k == "ms" else "iw_maxsquare")
        return ["k_prob_fwd:%s:%d" % (k, pl["prob_fwd"].cm), "k_prob_bwd:%s:%d" % (k, pl["prob_bwd"].cm), fin]
    fin = "k_loss_finalize:%s" % ("ce" if k == "plain" else "iw_entropy")
    return ["k_soft_fwd:%s:%d" % (k, pl["soft_fwd"].cm), "k_soft_bwd:%s:%d" % (k, pl["soft_bwd"].cm), fin]


def axis_class(n_in, n_out):
    if n_in == 1:
        return "in1"
    if n_out == 1:
        return "out1"
    if n_in == n_out:
        return "same"
    if n_in > n_out:
        return "down"
    q, r = divmod(n_out - 1, n_in - 1)
    return "up_pow2" if r == 0 and q & (q - 1) == 0 else "up"  # every low-res node is hit exactly


def bwd_classes(case, p):
    """The geometry classes of a backward plan p (up_bwd or upsample_bwd)."""
    out = ["W:" + axis_class(case.wi, case.wo), "H:" + axis_class(case.hi, case.ho)]
    n = p.rows_chunks
    out.append("chunks1" if n == 1 else "chunks8" if n == 8 else "chunks2..7")
    if n > 1 and case.wi - (n - 1) * p.per < p.per:
        out.append("last_chunk_short")
    if p.status == MSL_ERR_SHAPE:
        return out + ["lds_refused"]
    out.append("lds_optin" if p.lds_optin else "lds_small")
    if p.cols_trips > 1:
        out.append("cols_stride")
    return out


def classes_of(case, pl):
    """The geometry classes the case is filed under, as one sorted, comma-joined string."""
    out = []
    for f in BWD_FAMILIES:
        if f in pl:
            out += bwd_classes(case, pl[f])
    for f in ("up_fwd", "upsample_fwd", "resize", "labels", "prob_fwd", "prob_bwd", "soft_fwd", "soft_bwd"):
        if f in pl and pl[f].status == MSL_OK:
            out.append("%s_%s" % (f, "stride" if pl[f].fwd_trips > 1 else "one_trip"))
    return ",".join(sorted(out))


def name_of(case, pl):
    first = next(iter(pl.values()))
    return "%s:%s:%d" % (case.op, case.kind, first.cm)


# ------------------------------------------------------------------------------------------ the grid
GRID_W = ((1, 9), (5, 1), (33, 33), (5, 17), (17, 100), (65, 130), (100, 333), (257, 300), (70, 40), (33, 9),
          (17, 1024), (2, 1400), (64, 65), (255, 256), (256, 300), (31, 500))
GRID_H = ((1, 5), (5, 1), (5, 5), (3, 9), (3, 7), (33, 9), (65, 9))
GRID_C = (1, 13, 16, 19, 32)


def grid():
    """(family, Case) over the lattice: every backward family at every geometry."""
    for fam, (wi, wo), (hi, ho), c in itertools.product(BWD_FAMILIES, GRID_W, GRID_H, GRID_C):
        op = "up" if fam == "up_bwd" else "upsample"
        yield fam, Case(op, "ce" if op == "up" else "-", c, hi, wi, ho, wo, "x4", 1.0, None, None, 0)


def reached(hip, cases):
    """{(family, class): [cases]} over (family, case) pairs, by the library's plan."""
    out = {}
    for fam, cs in cases:
        p = hip.loss_plan(fam, *geo(cs))
        assert p.status in (MSL_OK, MSL_ERR_SHAPE), cs
        for cl in bwd_classes(cs, p):
            out.setdefault((fam, cl), []).append(cs)
    return out


def suggest(cases):
    """The cheapest grid point of a (family, class) the table lacks."""
    return min(cases, key=lambda c: c.c * (c.hi * c.wi + c.ho * c.wo))


# ------------------------------------------------------------------------------------------ the host bound
def chunk_ranges(wi, wo, chunks):
    """k_bwd_rows' pixel range [ox_lo, ox_hi) of every column chunk, from the fp32 lin(): [(ixa, ixb, lo, hi)]."""
    i0 = lr.lin_taps(wi, wo)[0]
    per = -(-wi // chunks)
    out = []
    for j in range(chunks):
        ixa, ixb = j * per, min(wi, (j + 1) * per)
        lo = int(np.searchsorted(i0, ixa - 1, side="left"))
        hi = wo if ixb >= wi else int(np.searchsorted(i0, ixb, side="left"))
        out.append((ixa, ixb, lo, hi))
    return out


def bound_grid():
    """(wi, wo) of the host-bound sweep: every wi up to 300 against a dense set of wo, and seeded random pairs."""
    pow2 = sorted({v for k in range(1, 12) for v in (2 ** k - 1, 2 ** k, 2 ** k + 1)})
    wos = sorted(set(range(1, 41)) | set(pow2) | {100, 130, 300, 333, 513, 1000, 1400})
    for wi in range(1, 301):
        for wo in wos:
            yield wi, wo
    rng = np.random.RandomState(20240)
    for _ in range(3000):
        yield int(rng.randint(1, 2050)), int(rng.randint(1, 4097))


# ------------------------------------------------------------------------------------------ the inputs
def tie_nodes(case):
    """Low-res nodes (iy, ix) whose two top classes are tied, isolated from each other; their hi-res pixels."""
    nodes = [(0, 1), (case.hi - 1, 3)]
    sy = (case.ho - 1) // max(case.hi - 1, 1)
    sx = (case.wo - 1) // max(case.wi - 1, 1)
    return nodes, [(iy * sy, ix * sx) for iy, ix in nodes]


def logits(case, which=0):
    """The low-resolution logits (1, c, hi, wi) of an up / labels / pseudo case; which = 1: the second head."""
    tok = case.data.split("+")
    g = torch.Generator().manual_seed(1000 * case.seed + which)
    scale = 400.0 if "x400" in tok else 40.0 if "x40" in tok and which == 0 else 4.0
    x = torch.randn(1, case.c, case.hi, case.wi, generator=g) * scale
    if "off" in tok:
        x = x + 1e4
    if "empty" in tok and case.c > 2:
        x[:, [1, case.c - 1]] -= 60.0
    if "tie" in tok:
        a, b = case.c // 3, case.c - 1
        for iy, ix in tie_nodes(case)[0]:
            x[0, a, iy, ix] = x[0, b, iy, ix] = x[0, :, iy, ix].max() + 3.0
    return x


def ce_labels(case):
    tok = case.data.split("+")
    g = torch.Generator().manual_seed(1000 * case.seed + 7)
    n, c = case.ho * case.wo, case.c
    if "over" in tok:
        return torch.randint(-1, c + 3, (n,), generator=g)
    if "one" in tok:
        y = torch.full((n,), -1, dtype=torch.int64)
        y[n // 2] = c - 1
        return y
    if "first" in tok:
        return torch.zeros(n, dtype=torch.int64)
    if "last" in tok:
        return torch.full((n,), c - 1, dtype=torch.int64)
    if "none" in tok:
        return torch.full((n,), -1, dtype=torch.int64)
    return torch.randint(-1, c, (n,), generator=g)


def flat_inputs(case):
    """prob: (prob, label or None).  soft: (inputs, target).  Tensors (1, c, ho, wo)."""
    tok = case.data.split("+")
    g = torch.Generator().manual_seed(1000 * case.seed + 3)
    shape = (1, case.c, case.ho, case.wo)
    x = torch.randn(shape, generator=g) * 3.0
    if case.op == "prob":
        lab = torch.randint(-1, case.c, (1, case.ho, case.wo), generator=g) if "lab" in tok else None
        return torch.softmax(x, 1), lab
    t = torch.softmax(torch.randn(shape, generator=g) * 2.0, 1)
    if "part" in tok:
        flat = t.reshape(-1)
        flat[3::7] = -1.0
    if "all" in tok:
        t = torch.full(shape, -1.0)
    return x, t


def upsample_inputs(case):
    """(x (1, c, hi, wi), gy (1, c, ho, wo)) of an upsample / resize case."""
    g = torch.Generator().manual_seed(1000 * case.seed + 5)
    return (torch.randn(1, case.c, case.hi, case.wi, generator=g) * 3.0,
            torch.randn(1, case.c, case.ho, case.wo, generator=g))


def reference(case):
    """The fp64 reference of an up case (loss_ref.up_loss)."""
    low2 = logits(case, 1) if case.kind == "multi_ce" else None
    labels = ce_labels(case) if case.kind == "ce" else None
    return lr.up_loss(case.kind, logits(case), (case.ho, case.wo), low2, labels, case.thr, case.ratio, case.gout)


def run_reference(case):
    """The fp64 reference of any case with a gradient: (K's kind, {output name: (ref, A)}, the full reference)."""
    if case.op == "up":
        r = reference(case)
        return case.kind, {"dlow": (r["dlow"], r["A"])}, r
    if case.op == "prob":
        p, lab = flat_inputs(case)
        r = lr.prob_loss(p, case.kind == "iw", lab, case.ratio, case.gout)
        return "prob", {"dprob": (r["dprob"], r["A"])}, r
    x, t = flat_inputs(case)
    r = lr.soft_loss(x, t, -1.0, case.ratio, case.gout)
    return "soft", {"dinputs": (r["dinputs"], r["A_inputs"]), "dtarget": (r["dtarget"], r["A_target"])}, r


def cpu_fp32_ratio(case):
    """(K's kind, worst |d32 - ref| / (2^-24 A)) of torch-CPU fp32 autograd of the case's operation."""
    kind, outs, r = run_reference(case)
    if case.op == "up":
        got = {"dlow": lr.up_loss_fp32(case.kind, logits(case), (case.ho, case.wo), r, case.gout)[1]}
    elif case.op == "prob":
        got = {"dprob": lr.prob_loss_fp32(flat_inputs(case)[0], case.kind == "iw", r, case.gout)[1]}
    else:
        _, dx, dt = lr.soft_loss_fp32(*flat_inputs(case), -1.0, case.ratio, case.gout)
        got = {"dinputs": dx, "dtarget": dt}
    return kind, max(lr.local_ratio(got[n], ref, a)[0] for n, (ref, a) in outs.items())


def k_rule(ratio):
    """4 x the measured ratio, rounded up to a power of two."""
    k = 1
    while k < 4.0 * ratio:
        k *= 2
    return k


def case_id(row):
    name, _, c = row
    return "%s-%dx%d-%dx%d-%s-g%s-t%s-r%s-s%d" % (name, c.hi, c.wi, c.ho, c.wo, c.data, c.gout, c.thr, c.ratio, c.seed)


# ------------------------------------------------------------------------------------------ the table
# (name = op:kind:CM bucket, geometry classes, Case): every key of ALL_KEYS once, every (backward family, class)
# pair once, every data edge once per kind; the kinds, gout and class counts cycled over the geometries (no cross
# product).  The seeds are picked so that the margin condition holds (test_loss_forms.py asserts it).
TABLE = [
    ("up:ce:19", "H:up,W:in1,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'ce', 19, 3, 1, 7, 9, 'x4', 1.0, None, None, 0)),
    ("up:ce:16", "H:same,W:out1,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'ce', 16, 5, 5, 5, 1, 'x4', 0.37, None, None, 0)),
    ("up:ce:13", "H:up_pow2,W:same,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'ce', 13, 3, 33, 9, 33, 'x4', -2.0, None, None, 0)),
    ("up:ce:32", "H:same,W:up_pow2,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'ce', 1, 3, 5, 3, 17, 'x4', 1.0, None, None, 0)),
    ("up:maxsquare:19", "H:up,W:up,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'maxsquare', 19, 4, 17, 9, 100, 'x4', 0.37, None, None, 0)),
    ("up:maxsquare:16", "H:in1,W:up,chunks2..7,last_chunk_short,lds_small,up_fwd_one_trip",
     Case('up', 'maxsquare', 16, 1, 65, 5, 130, 'x4', -2.0, None, None, 0)),
    ("up:maxsquare:13", "H:out1,W:up,chunks2..7,last_chunk_short,lds_small,up_fwd_one_trip",
     Case('up', 'maxsquare', 13, 5, 100, 1, 333, 'x4', 1.0, None, None, 0)),
    ("up:maxsquare:32", "H:down,W:up,chunks8,last_chunk_short,lds_small,up_fwd_one_trip",
     Case('up', 'maxsquare', 2, 33, 257, 9, 300, 'x4', 0.37, None, None, 0)),
    ("up:iw_maxsquare:19", "H:up_pow2,W:down,chunks2..7,lds_small,up_fwd_one_trip",
     Case('up', 'iw_maxsquare', 19, 3, 70, 5, 40, 'x4', -2.0, None, 0.2, 1)),
    ("up:iw_maxsquare:16", "H:down,W:down,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'iw_maxsquare', 16, 33, 33, 9, 9, 'x4', 1.0, None, 0.2, 0)),
    ("up:iw_maxsquare:13", "H:up,W:in1,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'iw_maxsquare', 13, 3, 1, 7, 9, 'x4', 0.37, None, 0.2, 0)),
    ("up:iw_maxsquare:32", "H:same,W:out1,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'iw_maxsquare', 12, 5, 5, 5, 1, 'x4', -2.0, None, 0.2, 0)),
    ("up:multi_ce:19", "H:up_pow2,W:same,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'multi_ce', 19, 3, 33, 9, 33, 'x4', 1.0, 0.5, None, 0)),
    ("up:multi_ce:16", "H:same,W:up_pow2,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'multi_ce', 16, 3, 5, 3, 17, 'x4', 0.37, 0.5, None, 0)),
    ("up:multi_ce:13", "H:up,W:up,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'multi_ce', 13, 4, 17, 9, 100, 'x4', -2.0, 0.5, None, 0)),
    ("up:multi_ce:32", "H:in1,W:up,chunks2..7,last_chunk_short,lds_small,up_fwd_one_trip",
     Case('up', 'multi_ce', 14, 1, 65, 5, 130, 'x4', 1.0, 0.5, None, 0)),
    ("up:entropy:19", "H:out1,W:up,chunks2..7,last_chunk_short,lds_small,up_fwd_one_trip",
     Case('up', 'entropy', 19, 5, 100, 1, 333, 'x4', 0.37, None, None, 0)),
    ("up:entropy:16", "H:down,W:up,chunks8,last_chunk_short,lds_small,up_fwd_one_trip",
     Case('up', 'entropy', 16, 33, 257, 9, 300, 'x4', -2.0, None, None, 0)),
    ("up:entropy:13", "H:up_pow2,W:down,chunks2..7,lds_small,up_fwd_one_trip",
     Case('up', 'entropy', 13, 3, 70, 5, 40, 'x4', 1.0, None, None, 0)),
    ("up:entropy:32", "H:down,W:down,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'entropy', 20, 33, 33, 9, 9, 'x4', 0.37, None, None, 0)),
    ("up:iw_entropy:19", "H:up,W:in1,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'iw_entropy', 19, 3, 1, 7, 9, 'x4', -2.0, None, 0.2, 0)),
    ("up:iw_entropy:16", "H:same,W:out1,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'iw_entropy', 16, 5, 5, 5, 1, 'x4', 1.0, None, 0.2, 0)),
    ("up:iw_entropy:13", "H:up_pow2,W:same,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'iw_entropy', 13, 3, 33, 9, 33, 'x4', 0.37, None, 0.2, 0)),
    ("up:iw_entropy:32", "H:same,W:up_pow2,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'iw_entropy', 32, 3, 5, 3, 17, 'x4', -2.0, None, 0.2, 0)),
    ("up:hard_ce:19", "H:up,W:up,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'hard_ce', 19, 4, 17, 9, 100, 'x4', 1.0, 0.5, None, 0)),
    ("up:hard_ce:16", "H:in1,W:up,chunks2..7,last_chunk_short,lds_small,up_fwd_one_trip",
     Case('up', 'hard_ce', 16, 1, 65, 5, 130, 'x4', 0.37, 0.5, None, 0)),
    ("up:hard_ce:13", "H:out1,W:up,chunks2..7,last_chunk_short,lds_small,up_fwd_one_trip",
     Case('up', 'hard_ce', 13, 5, 100, 1, 333, 'x4', -2.0, 0.5, None, 0)),
    ("up:hard_ce:32", "H:down,W:up,chunks8,last_chunk_short,lds_small,up_fwd_one_trip",
     Case('up', 'hard_ce', 1, 33, 257, 9, 300, 'x4', 1.0, 0.5, None, 0)),
    ("up:ce:19", "H:up_pow2,W:up,chunks1,lds_optin,up_fwd_one_trip",
     Case('up', 'ce', 19, 3, 17, 5, 1024, 'x4', 0.37, None, None, 0)),
    ("up:maxsquare:32", "H:up_pow2,W:up,chunks1,lds_refused,up_fwd_one_trip",
     Case('up', 'maxsquare', 32, 3, 2, 5, 1400, 'x4', 1.0, None, None, 0)),
    ("up:iw_entropy:32", "H:down,W:up,chunks8,cols_stride,last_chunk_short,lds_small,up_fwd_one_trip",
     Case('up', 'iw_entropy', 32, 65, 257, 9, 300, 'x4', -2.0, None, 0.2, 0)),
    ("up:ce:19", "H:up_pow2,W:up_pow2,chunks1,lds_small,up_fwd_stride",
     Case('up', 'ce', 19, 9, 9, 513, 513, 'x4', 0.37, None, None, 0)),
    ("up:ce:19", "H:up,W:up,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'ce', 19, 4, 17, 9, 100, 'x40', 0.37, None, None, 0)),
    ("up:ce:13", "H:same,W:same,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'ce', 13, 5, 33, 5, 33, 'off', -2.0, None, None, 0)),
    ("up:maxsquare:32", "H:up,W:up,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'maxsquare', 12, 4, 17, 9, 100, 'x40', -2.0, None, None, 0)),
    ("up:maxsquare:32", "H:same,W:same,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'maxsquare', 20, 5, 33, 5, 33, 'off', 1.0, None, None, 0)),
    ("up:iw_maxsquare:19", "H:up,W:up,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'iw_maxsquare', 19, 4, 17, 9, 100, 'x40', 1.0, None, 0.2, 0)),
    ("up:iw_maxsquare:13", "H:same,W:same,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'iw_maxsquare', 13, 5, 33, 5, 33, 'off', 0.37, None, 0.2, 0)),
    ("up:multi_ce:32", "H:up,W:up,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'multi_ce', 12, 4, 17, 9, 100, 'x40', 0.37, 0.95, None, 0)),
    ("up:multi_ce:32", "H:same,W:same,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'multi_ce', 20, 5, 33, 5, 33, 'off', -2.0, 0.5, None, 0)),
    ("up:entropy:19", "H:up,W:up,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'entropy', 19, 4, 17, 9, 100, 'x40', -2.0, None, None, 0)),
    ("up:entropy:13", "H:same,W:same,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'entropy', 13, 5, 33, 5, 33, 'off', 1.0, None, None, 0)),
    ("up:iw_entropy:32", "H:up,W:up,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'iw_entropy', 12, 4, 17, 9, 100, 'x40', 1.0, None, 0.2, 0)),
    ("up:iw_entropy:32", "H:same,W:same,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'iw_entropy', 20, 5, 33, 5, 33, 'off', 0.37, None, 0.2, 0)),
    ("up:hard_ce:19", "H:up,W:up,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'hard_ce', 19, 4, 17, 9, 100, 'x40', 0.37, 0.95, None, 1)),
    ("up:hard_ce:13", "H:same,W:same,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'hard_ce', 13, 5, 33, 5, 33, 'off', -2.0, 0.5, None, 0)),
    ("up:ce:19", "H:up,W:up,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'ce', 19, 3, 5, 7, 11, 'x4+over', 1.0, None, None, 0)),
    ("up:ce:32", "H:up,W:up,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'ce', 14, 3, 5, 7, 11, 'x4+one', 0.37, None, None, 0)),
    ("up:ce:16", "H:up,W:up,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'ce', 16, 3, 5, 7, 11, 'x4+first', -2.0, None, None, 0)),
    ("up:ce:32", "H:up,W:up,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'ce', 2, 3, 5, 7, 11, 'x4+last', 1.0, None, None, 0)),
    ("up:ce:13", "H:up,W:up,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'ce', 13, 3, 5, 7, 11, 'x4+none', 0.37, None, None, 0)),
    ("up:iw_maxsquare:19", "H:up,W:up,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'iw_maxsquare', 19, 4, 17, 9, 100, 'x4+empty', 1.0, None, 0.0, 0)),
    ("up:iw_maxsquare:32", "H:up,W:up,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'iw_maxsquare', 32, 4, 17, 9, 100, 'x4+empty', 0.37, None, 0.2, 0)),
    ("up:iw_maxsquare:16", "H:up,W:up,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'iw_maxsquare', 16, 4, 17, 9, 100, 'x4+empty', -2.0, None, 1.0, 0)),
    ("up:iw_entropy:19", "H:up,W:up,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'iw_entropy', 19, 4, 17, 9, 100, 'x4+empty', 1.0, None, 0.0, 0)),
    ("up:iw_entropy:32", "H:up,W:up,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'iw_entropy', 32, 4, 17, 9, 100, 'x4+empty', 0.37, None, 0.2, 0)),
    ("up:iw_entropy:16", "H:up,W:up,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'iw_entropy', 16, 4, 17, 9, 100, 'x4+empty', -2.0, None, 1.0, 0)),
    ("up:hard_ce:19", "H:up,W:up,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'hard_ce', 19, 3, 5, 7, 11, 'x4', 0.37, 1.001, None, 0)),
    ("up:hard_ce:32", "H:up,W:up,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'hard_ce', 14, 3, 5, 7, 11, 'x4', -2.0, 0.0, None, 0)),
    ("up:multi_ce:19", "H:up,W:up,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'multi_ce', 19, 3, 5, 7, 11, 'x4', 0.37, 1.001, None, 0)),
    ("up:multi_ce:32", "H:up,W:up,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'multi_ce', 14, 3, 5, 7, 11, 'x4', -2.0, 0.0, None, 0)),
    ("up:iw_maxsquare:19", "H:same,W:up_pow2,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'iw_maxsquare', 19, 3, 5, 3, 17, 'x4+tie', 1.0, None, 0.2, 0)),
    ("up:iw_entropy:19", "H:same,W:up_pow2,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'iw_entropy', 19, 3, 5, 3, 17, 'x4+tie', 1.0, None, 0.2, 0)),
    ("up:multi_ce:32", "H:same,W:up_pow2,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'multi_ce', 12, 3, 5, 3, 17, 'x4+tie', 1.0, 0.3, None, 0)),
    ("up:hard_ce:19", "H:same,W:up_pow2,chunks1,lds_small,up_fwd_one_trip",
     Case('up', 'hard_ce', 19, 3, 5, 3, 17, 'x4+tie', 1.0, 0.3, None, 0)),
    ("upsample:-:0", "H:up,W:in1,chunks1,lds_small,upsample_fwd_one_trip",
     Case('upsample', '-', 19, 3, 1, 7, 9, 'x4', 1.0, None, None, 0)),
    ("upsample:-:0", "H:same,W:out1,chunks1,lds_small,upsample_fwd_one_trip",
     Case('upsample', '-', 16, 5, 5, 5, 1, 'x4', 1.0, None, None, 0)),
    ("upsample:-:0", "H:up_pow2,W:same,chunks1,lds_small,upsample_fwd_one_trip",
     Case('upsample', '-', 13, 3, 33, 9, 33, 'x4', 1.0, None, None, 0)),
    ("upsample:-:0", "H:same,W:up_pow2,chunks1,lds_small,upsample_fwd_one_trip",
     Case('upsample', '-', 3, 3, 5, 3, 17, 'x4', 1.0, None, None, 0)),
    ("upsample:-:0", "H:up,W:up,chunks1,lds_small,upsample_fwd_one_trip",
     Case('upsample', '-', 1, 4, 17, 9, 100, 'x4', 1.0, None, None, 0)),
    ("upsample:-:0", "H:in1,W:up,chunks2..7,last_chunk_short,lds_small,upsample_fwd_one_trip",
     Case('upsample', '-', 20, 1, 65, 5, 130, 'x4', 1.0, None, None, 0)),
    ("upsample:-:0", "H:out1,W:up,chunks2..7,last_chunk_short,lds_small,upsample_fwd_one_trip",
     Case('upsample', '-', 2, 5, 100, 1, 333, 'x4', 1.0, None, None, 0)),
    ("upsample:-:0", "H:down,W:up,chunks8,last_chunk_short,lds_small,upsample_fwd_one_trip",
     Case('upsample', '-', 12, 33, 257, 9, 300, 'x4', 1.0, None, None, 0)),
    ("upsample:-:0", "H:up_pow2,W:down,chunks2..7,lds_small,upsample_fwd_one_trip",
     Case('upsample', '-', 14, 3, 70, 5, 40, 'x4', 1.0, None, None, 0)),
    ("upsample:-:0", "H:down,W:down,chunks1,lds_small,upsample_fwd_one_trip",
     Case('upsample', '-', 19, 33, 33, 9, 9, 'x4', 1.0, None, None, 0)),
    ("upsample:-:0", "H:up_pow2,W:up,chunks1,lds_optin,upsample_fwd_one_trip",
     Case('upsample', '-', 19, 3, 17, 5, 1024, 'x4', 1.0, None, None, 0)),
    ("upsample:-:0", "H:up_pow2,W:up,chunks1,lds_refused,upsample_fwd_one_trip",
     Case('upsample', '-', 32, 3, 2, 5, 1400, 'x4', 1.0, None, None, 0)),
    ("upsample:-:0", "H:down,W:up,chunks8,cols_stride,last_chunk_short,lds_small,upsample_fwd_one_trip",
     Case('upsample', '-', 32, 65, 257, 9, 300, 'x4', 1.0, None, None, 0)),
    ("upsample:-:0", "H:up,W:up,chunks1,lds_small,upsample_fwd_one_trip",
     Case('upsample', '-', 16, 3, 5, 7, 11, 'x4', 1.0, None, None, 0)),
    ("resize:-:0", "resize_one_trip",
     Case('resize', '-', 3, 20, 30, 60, 68, 'x4', 1.0, None, None, 0)),
    ("resize:-:0", "resize_one_trip",
     Case('resize', '-', 3, 20, 30, 60, 69, 'x4', 1.0, None, None, 0)),
    ("resize:-:0", "resize_one_trip",
     Case('resize', '-', 4, 20, 30, 60, 68, 'x4', 1.0, None, None, 0)),
    ("resize:-:0", "resize_one_trip",
     Case('resize', '-', 4, 20, 30, 60, 69, 'x4', 1.0, None, None, 0)),
    ("resize:-:0", "resize_one_trip",
     Case('resize', '-', 3, 40, 50, 17, 23, 'x4', 1.0, None, None, 0)),
    ("labels:-:19", "labels_one_trip",
     Case('labels', '-', 19, 3, 33, 9, 33, 'x4', 1.0, 0.5, None, 0)),
    ("pseudo:-:19", "labels_one_trip",
     Case('pseudo', '-', 19, 4, 17, 9, 100, 'x4', 1.0, 0.5, None, 0)),
    ("labels:-:16", "labels_one_trip",
     Case('labels', '-', 16, 4, 17, 9, 100, 'x4', 1.0, 0.5, None, 4)),
    ("pseudo:-:16", "labels_one_trip",
     Case('pseudo', '-', 16, 3, 33, 9, 33, 'x4', 1.0, 0.5, None, 1)),
    ("labels:-:13", "labels_one_trip",
     Case('labels', '-', 13, 3, 70, 5, 40, 'x4', 1.0, 0.5, None, 1)),
    ("pseudo:-:13", "labels_one_trip",
     Case('pseudo', '-', 13, 3, 5, 3, 17, 'x4', 1.0, 0.5, None, 0)),
    ("labels:-:32", "labels_one_trip",
     Case('labels', '-', 20, 3, 5, 3, 17, 'x4', 1.0, 0.5, None, 0)),
    ("pseudo:-:32", "labels_one_trip",
     Case('pseudo', '-', 20, 3, 70, 5, 40, 'x4', 1.0, 0.5, None, 1)),
    ("prob:ms:19", "prob_bwd_one_trip,prob_fwd_one_trip",
     Case('prob', 'ms', 19, 1, 1, 5, 51, 'nolab', 1.0, None, None, 0)),
    ("prob:ms:16", "prob_bwd_one_trip,prob_fwd_one_trip",
     Case('prob', 'ms', 16, 1, 1, 5, 51, 'lab', 0.37, None, None, 0)),
    ("prob:ms:13", "prob_bwd_one_trip,prob_fwd_one_trip",
     Case('prob', 'ms', 13, 1, 1, 5, 51, 'nolab', -2.0, None, None, 0)),
    ("prob:ms:32", "prob_bwd_one_trip,prob_fwd_one_trip",
     Case('prob', 'ms', 12, 1, 1, 5, 51, 'lab', 1.0, None, None, 0)),
    ("prob:ms:32", "prob_bwd_one_trip,prob_fwd_one_trip",
     Case('prob', 'ms', 2, 1, 1, 5, 51, 'nolab', 0.37, None, None, 0)),
    ("prob:iw:32", "prob_bwd_one_trip,prob_fwd_one_trip",
     Case('prob', 'iw', 2, 1, 1, 5, 51, 'lab', -2.0, None, 0.2, 0)),
    ("prob:iw:19", "prob_bwd_one_trip,prob_fwd_one_trip",
     Case('prob', 'iw', 19, 1, 1, 5, 51, 'nolab', 0.37, None, 0.2, 0)),
    ("prob:iw:16", "prob_bwd_one_trip,prob_fwd_one_trip",
     Case('prob', 'iw', 16, 1, 1, 5, 51, 'lab', -2.0, None, 0.2, 0)),
    ("prob:iw:13", "prob_bwd_one_trip,prob_fwd_one_trip",
     Case('prob', 'iw', 13, 1, 1, 5, 51, 'nolab', 1.0, None, 0.2, 0)),
    ("prob:iw:32", "prob_bwd_one_trip,prob_fwd_one_trip",
     Case('prob', 'iw', 12, 1, 1, 5, 51, 'lab', 0.37, None, 0.2, 0)),
    ("prob:ms:32", "prob_bwd_one_trip,prob_fwd_one_trip",
     Case('prob', 'ms', 2, 1, 1, 1, 1, 'lab', 0.37, None, None, 0)),
    ("prob:ms:32", "prob_bwd_one_trip,prob_fwd_one_trip",
     Case('prob', 'ms', 2, 1, 1, 1, 257, 'nolab', -2.0, None, None, 0)),
    ("prob:ms:32", "prob_bwd_one_trip,prob_fwd_stride",
     Case('prob', 'ms', 2, 1, 1, 300, 1000, 'lab', 1.0, None, None, 0)),
    ("prob:iw:32", "prob_bwd_one_trip,prob_fwd_one_trip",
     Case('prob', 'iw', 2, 1, 1, 1, 1, 'nolab', 0.37, None, 0.0, 0)),
    ("prob:iw:32", "prob_bwd_one_trip,prob_fwd_one_trip",
     Case('prob', 'iw', 2, 1, 1, 1, 257, 'lab', -2.0, None, 0.2, 0)),
    ("prob:iw:32", "prob_bwd_one_trip,prob_fwd_stride",
     Case('prob', 'iw', 2, 1, 1, 300, 1000, 'nolab', 1.0, None, 1.0, 0)),
    ("soft:plain:19", "soft_bwd_one_trip,soft_fwd_one_trip",
     Case('soft', 'plain', 19, 1, 1, 5, 51, 'keep+both', 1.0, None, None, 0)),
    ("soft:plain:16", "soft_bwd_one_trip,soft_fwd_one_trip",
     Case('soft', 'plain', 16, 1, 1, 5, 51, 'part+di', 0.37, None, None, 0)),
    ("soft:plain:13", "soft_bwd_one_trip,soft_fwd_one_trip",
     Case('soft', 'plain', 13, 1, 1, 5, 51, 'part+dt', -2.0, None, None, 0)),
    ("soft:plain:32", "soft_bwd_one_trip,soft_fwd_one_trip",
     Case('soft', 'plain', 14, 1, 1, 5, 51, 'keep+di', 1.0, None, None, 0)),
    ("soft:iw:19", "soft_bwd_one_trip,soft_fwd_one_trip",
     Case('soft', 'iw', 19, 1, 1, 5, 51, 'keep+both', 0.37, None, 0.2, 0)),
    ("soft:iw:16", "soft_bwd_one_trip,soft_fwd_one_trip",
     Case('soft', 'iw', 16, 1, 1, 5, 51, 'part+di', -2.0, None, 0.2, 0)),
    ("soft:iw:13", "soft_bwd_one_trip,soft_fwd_one_trip",
     Case('soft', 'iw', 13, 1, 1, 5, 51, 'part+dt', 1.0, None, 0.2, 0)),
    ("soft:iw:32", "soft_bwd_one_trip,soft_fwd_one_trip",
     Case('soft', 'iw', 14, 1, 1, 5, 51, 'keep+di', 0.37, None, 0.2, 0)),
    ("soft:plain:32", "soft_bwd_one_trip,soft_fwd_one_trip",
     Case('soft', 'plain', 2, 1, 1, 1, 1, 'part+both', 0.37, None, None, 0)),
    ("soft:plain:32", "soft_bwd_one_trip,soft_fwd_one_trip",
     Case('soft', 'plain', 2, 1, 1, 1, 257, 'keep+dt', -2.0, None, None, 0)),
    ("soft:plain:32", "soft_bwd_one_trip,soft_fwd_stride",
     Case('soft', 'plain', 2, 1, 1, 300, 1000, 'keep+both', 1.0, None, None, 0)),
    ("soft:iw:32", "soft_bwd_one_trip,soft_fwd_one_trip",
     Case('soft', 'iw', 2, 1, 1, 1, 1, 'part+both', 0.37, None, 0.0, 0)),
    ("soft:iw:32", "soft_bwd_one_trip,soft_fwd_one_trip",
     Case('soft', 'iw', 2, 1, 1, 1, 257, 'keep+dt', -2.0, None, 1.0, 0)),
    ("soft:iw:32", "soft_bwd_one_trip,soft_fwd_stride",
     Case('soft', 'iw', 2, 1, 1, 300, 1000, 'keep+both', 1.0, None, 0.2, 0)),
    ("soft:plain:32", "soft_bwd_one_trip,soft_fwd_one_trip",
     Case('soft', 'plain', 2, 1, 1, 5, 51, 'all+both', 1.0, None, None, 0)),
    ("soft:iw:32", "soft_bwd_one_trip,soft_fwd_one_trip",
     Case('soft', 'iw', 2, 1, 1, 5, 51, 'all+both', 0.37, None, 0.2, 0)),
    ("soft:plain:32", "soft_bwd_stride,soft_fwd_stride",
     Case('soft', 'plain', 1, 1, 1, 1, 1048833, 'keep+both', -2.0, None, None, 0)),
    ("soft:iw:32", "soft_bwd_stride,soft_fwd_stride",
     Case('soft', 'iw', 1, 1, 1, 1, 1048833, 'part+di', 0.37, None, 0.2, 0)),
    # the grid-stride trips of the kernels that decide: 513 x 513 and 1025 x 1025 independent pixels
    ("up:iw_maxsquare:19", "H:same,W:same,chunks8,cols_stride,last_chunk_short,lds_small,up_fwd_stride",
     Case('up', 'iw_maxsquare', 19, 513, 513, 513, 513, 'x400', 0.37, None, 0.2, 0)),
    ("up:iw_entropy:32", "H:same,W:same,chunks8,cols_stride,last_chunk_short,lds_small,up_fwd_stride",
     Case('up', 'iw_entropy', 20, 513, 513, 513, 513, 'x400', -2.0, None, 0.2, 0)),
    ("pseudo:-:32", "labels_stride",
     Case('pseudo', '-', 2, 1025, 1025, 1025, 1025, 'x400', 1.0, 0.5, None, 1)),
    ("labels:-:32", "labels_stride",
     Case('labels', '-', 2, 1025, 1025, 1025, 1025, 'x400+solo', 1.0, 0.5, None, 0)),
]
