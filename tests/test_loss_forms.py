"""The coverage gate of the fused-loss, upsample and resize kernels (CPU only: msl_loss_plan launches nothing).

csrc/loss.hip picks a class-count instantiation, the backward's column chunks and LDS, every grid and
msl_resize_bilinear's kernel by thresholds on the host.  This module plans a committed lattice of geometries
(loss_form_cases.grid) through the library itself - msl_loss_plan calls the functions the launches call - and holds
tests/loss_form_cases.py TABLE, the cases test_gpu_loss_forms.py compares with fp64, against it: a threshold edit
that sends some shape where no case goes, or a case that no longer runs what it is filed under, fails here, before
any GPU is involved.  It also checks the host's LDS bound against the fp32 index arithmetic over a wide sweep,
the fp64 reference (loss_ref.py) against torch in double, and each case's decision margins.
"""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_form_cases as lc
import loss_ref as lr
from maxsquareloss_amd import hip

ROWS = [pytest.param(row, id=lc.case_id(row)) for row in lc.TABLE]
UP_ROWS = [pytest.param(row, id=lc.case_id(row)) for row in lc.TABLE
           if row[2].op == "up" and row[2].ho * row[2].wo <= 5000]


@pytest.fixture(scope="module")
def swept():
    return lc.reached(hip, lc.grid())


def _filed():
    """{(family, class)} and {key} of the table, by the plan."""
    pairs, keys = set(), set()
    for _, _, cs in lc.TABLE:
        pl = lc.plans(hip, cs)
        keys |= set(lc.keys_of(cs, pl))
        for f in lc.BWD_FAMILIES:
            if f in pl:
                pairs |= {(f, cl) for cl in lc.bwd_classes(cs, pl[f])}
    return pairs, keys


def test_every_key_and_every_reachable_class_has_a_case(swept):
    pairs, keys = _filed()
    assert len(lc.ALL_KEYS) == 118 and len(set(lc.ALL_KEYS)) == 118
    missing = sorted(set(lc.ALL_KEYS) - keys)
    assert not missing, "kernel instantiations no case runs: %s" % missing
    assert keys <= set(lc.ALL_KEYS), sorted(keys - set(lc.ALL_KEYS))
    missing = sorted(set(swept) - pairs)
    hint = ["%s %s: e.g. %s" % (f, c, tuple(lc.suggest(swept[(f, c)]))) for f, c in missing]
    assert not missing, "reachable (family, class) pairs without a case:\n" + "\n".join(hint)
    # every class is reached where it can be, in both families
    every = {"W:" + a for a in lc.AXIS} | {"H:" + a for a in lc.AXIS} | {
        "chunks1", "chunks2..7", "chunks8", "last_chunk_short", "lds_small", "lds_optin", "lds_refused", "cols_stride"}
    for f in lc.BWD_FAMILIES:
        assert {c for g, c in swept if g == f} == every, f
    # the generic body of the losses at every class count it is asked to serve
    assert {cs.c for _, _, cs in lc.TABLE if cs.op == "up"} >= set(lc.GENERIC_C) | {19, 16, 13}
    print("%d keys, %d (family, class) pairs on the grid, all with a case; %d cases" % (
        len(keys), len(swept), len(lc.TABLE)))


@pytest.mark.parametrize("row", ROWS)
def test_table_case_lands_where_it_is_filed(row):
    name, classes, cs = row
    pl = lc.plans(hip, cs)
    assert (lc.name_of(cs, pl), lc.classes_of(cs, pl)) == (name, classes)
    for f, p in pl.items():
        assert p.status == lc.MSL_OK or (f in lc.BWD_FAMILIES and "lds_refused" in classes), (f, p.status)
    assert cs.gout in (1.0, 0.37, -2.0)
    if "off" in cs.data:  # values near 1e4 interpolate exactly only on the nodes
        assert (cs.hi, cs.wi) == (cs.ho, cs.wo)
    if "tie" in cs.data:
        assert lc.axis_class(cs.wi, cs.wo) in ("up_pow2", "same") and lc.axis_class(cs.hi, cs.ho) in ("up_pow2", "same")


def test_table_has_no_duplicates_and_holds_the_named_edges():
    cases = [row[2] for row in lc.TABLE]
    assert len(set(cases)) == len(cases)
    up = [c for c in cases if c.op == "up"]
    for kind in lc.KINDS:
        mine = [c for c in up if c.kind == kind]
        assert {c.gout for c in mine} == {1.0, 0.37, -2.0}, kind
        assert {t for c in mine for t in c.data.split("+")} >= {"x4", "x40", "off"}, kind
    for kind in ("iw_maxsquare", "iw_entropy"):
        assert {c.ratio for c in up if c.kind == kind and "empty" in c.data} == {0.0, 0.2, 1.0}
    for kind in ("hard_ce", "multi_ce"):
        assert {c.thr for c in up if c.kind == kind} >= {0.0, 0.5, 1.001}  # all pass, some, none
    assert {c.kind for c in up if "tie" in c.data} == {"iw_maxsquare", "iw_entropy", "multi_ce", "hard_ce"}
    ce = {t for c in up if c.kind == "ce" for t in c.data.split("+")}
    assert ce >= {"over", "one", "first", "last", "none"}
    assert any(c.wo % 4 for c in up)
    ups = [c for c in cases if c.op == "upsample"]
    assert {c.wo % 4 for c in ups} >= {0, 1, 3}
    rs = [c for c in cases if c.op == "resize"]
    assert {(c.c, c.ho + c.wo) for c in rs} >= {(3, 128), (3, 129), (4, 128), (4, 129)}
    flat = [c for c in cases if c.op in ("prob", "soft")]
    for op in ("prob", "soft"):
        assert {c.ho * c.wo for c in flat if c.op == op and c.c == 2} >= {1, 255, 257, 300000}
    assert any(c.op == "soft" and c.c == 1 and c.ho * c.wo > 4096 * 256 for c in flat)
    soft = {t for c in flat if c.op == "soft" for t in c.data.split("+")}
    assert soft >= {"keep", "part", "all", "di", "dt", "both"}


def test_thresholds_from_both_sides():
    """rows_chunks, MSL_DISPATCH_C, the 128 switch, the grid caps and the LDS limits, each from both sides."""
    bwd = lambda c, wi, wo, hi=3, ho=5: hip.loss_plan("up_bwd", c, hi, wi, ho, wo)  # noqa: E731
    for wi, n in ((1, 1), (63, 1), (64, 2), (95, 2), (96, 3), (255, 7), (256, 8), (257, 8), (1000, 8)):
        p = bwd(19, wi, 2 * wi)
        assert (p.rows_chunks, p.per) == (n, -(-wi // n)), wi
    for c in range(1, 33):
        cm = c if c in (19, 16, 13) else 32
        for fam in ("up_fwd", "up_bwd", "upsample_bwd", "labels", "prob_fwd", "prob_bwd", "soft_fwd", "soft_bwd"):
            assert hip.loss_plan(fam, c, 3, 5, 7, 11).cm == cm, (fam, c)
    assert hip.loss_plan("upsample_fwd", 19, 3, 5, 7, 11).cm == 0
    for c in (3, 4):
        for ho, wo, four in ((64, 64, 1), (60, 68, 1), (1, 127, 1), (60, 69, 0), (64, 65, 0), (1, 128, 0)):
            p = hip.loss_plan("resize", c, 20, 30, ho, wo)
            assert (p.status, p.four_tap) == (lc.MSL_OK, four), (c, ho, wo)
            if four:
                assert (p.fwd_blocks, p.fwd_trips, p.vec) == (-(-c * ho * wo // 256), 1, 0)
            else:
                assert p.vec == int(wo % 4 == 0) and p.fwd_blocks == min(8192, -(-c * ho * -(-wo // 4) // 256))
    # the grid caps: 1024 forward blocks, 2048 of k_bwd_cols, 4096 of the flat backward and the label kernels
    for fam, cap in (("up_fwd", 1024), ("labels", 4096)):
        n = cap * 256
        assert hip.loss_plan(fam, 19, 3, 5, 1, n).fwd_trips == 1 and hip.loss_plan(fam, 19, 3, 5, 1, n + 1).fwd_trips == 2
        assert hip.loss_plan(fam, 19, 3, 5, 1, n + 1).fwd_blocks == cap
    for fam, cap in (("prob_fwd", 1024), ("soft_fwd", 1024), ("prob_bwd", 4096), ("soft_bwd", 4096)):
        n = cap * 256
        assert hip.loss_plan(fam, 2, 1, 1, 1, n).fwd_trips == 1 and hip.loss_plan(fam, 2, 1, 1, 1, n + 1).fwd_trips == 2
    assert bwd(32, 128, 130, hi=128).cols_trips == 1 and bwd(32, 129, 130, hi=128).cols_trips == 2  # 32 * 128 * 128
    assert bwd(32, 129, 130, hi=128).cols_blocks == 2048
    # LDS: wmax * (4 c + 12) bytes; opt-in above 64 KB, refused above 160 KB
    for c, wo, optin, status in ((19, 744, 0, 0), (19, 745, 1, 0), (19, 1861, 1, 0), (19, 1862, 1, lc.MSL_ERR_SHAPE)):
        p = bwd(c, 1, wo)  # wi = 1: the whole row
        assert p.rows_wmax == wo and p.lds_bytes == wo * (4 * c + 12)
        assert (p.lds_optin, p.status) == (optin, status), (c, wo, p.lds_bytes)
    p = bwd(19, 17, 1024)
    assert (p.lds_bytes, p.lds_optin, p.status) == (90112, 1, lc.MSL_OK)
    p = bwd(32, 2, 1400)
    assert p.status == lc.MSL_ERR_SHAPE and hip.loss_plan("up_fwd", 32, 3, 2, 5, 1400).status == lc.MSL_OK


def test_refusals():
    ok, arg, wsp = lc.MSL_OK, lc.MSL_ERR_ARG, lc.MSL_ERR_WORKSPACE
    lib = hip.load(require_gpu=False)
    for fam in ("up_fwd", "up_bwd", "upsample_bwd", "labels", "prob_fwd", "prob_bwd", "soft_fwd", "soft_bwd"):
        assert hip.loss_plan(fam, 32, 3, 5, 7, 11, ws_bytes=1 << 30).status == ok, fam
        assert hip.loss_plan(fam, 33, 3, 5, 7, 11, ws_bytes=1 << 30).status == arg, fam
        assert hip.loss_plan(fam, 0, 3, 5, 7, 11, ws_bytes=1 << 30).status == arg, fam
    assert hip.loss_plan("upsample_fwd", 33, 3, 5, 7, 11).status == ok  # no class limit: C is a run-time count
    assert hip.loss_plan("resize", 4, 3, 5, 7, 11).status == ok and hip.loss_plan("resize", 5, 3, 5, 7, 11).status == arg
    for fam in ("up_fwd", "up_bwd", "upsample_bwd", "upsample_fwd", "resize", "labels"):
        for g in ((0, 5, 7, 11), (3, 0, 7, 11), (3, 5, 0, 11), (3, 5, 7, 0)):
            assert hip.loss_plan(fam, 3, *g, ws_bytes=1 << 30).status == arg, (fam, g)
    assert hip.loss_plan("up_fwd", 19, 3, 5, 46341, 46341, ws_bytes=1 << 30).status == arg  # 2^31 pixels and more
    assert hip.loss_plan("upsample_fwd", 2, 3, 5, 32768, 32768).status == arg  # c * ho * wo
    # a workspace one byte short
    for fam, g in (("up_fwd", (19, 3, 5, 7, 11)), ("up_bwd", (19, 3, 5, 7, 11)), ("upsample_bwd", (3, 3, 5, 7, 11)),
                   ("prob_fwd", (2, 1, 1, 5, 51)), ("soft_fwd", (32, 1, 1, 5, 51))):
        need = hip.loss_plan(fam, *g).ws_required
        assert need > 0 and hip.loss_plan(fam, *g, ws_bytes=need).status == ok
        assert hip.loss_plan(fam, *g, ws_bytes=need - 1).status == wsp
    for fam in ("upsample_fwd", "resize", "labels", "prob_bwd", "soft_bwd"):
        assert hip.loss_plan(fam, 3, 3, 5, 7, 11, ws_bytes=0).status == ok
    # the query itself refuses no out and a family it does not know; out untouched
    out = hip.LossPlan()
    out.status = 77
    assert lib.msl_loss_plan(0, 19, 3, 5, 7, 11, 1 << 30, None) == arg
    for fam in (-1, 10):
        assert lib.msl_loss_plan(fam, 19, 3, 5, 7, 11, 1 << 30, ctypes.addressof(out)) == arg
    assert out.status == 77


def test_host_bound_holds_over_the_sweep():
    """rows_wmax against the fp32 lin(): every chunk non-empty and within the planned range, i0 monotone, the
    160 KB refusal where the plan says, msl_loss_workspace enough for both passes."""
    lib = hip.load(require_gpu=False)
    n = 0
    for wi, wo in lc.bound_grid():
        i0 = lr.lin_taps(wi, wo)[0]
        assert (np.diff(i0) >= 0).all() and i0[0] == 0 and i0[-1] <= wi - 1, (wi, wo)
        for c in (1, 19, 32):
            p = hip.loss_plan("up_bwd", c, 3, wi, 5, wo)
            assert p.status in (lc.MSL_OK, lc.MSL_ERR_SHAPE)
            assert (p.lds_bytes > 160 * 1024) == (p.status == lc.MSL_ERR_SHAPE), (c, wi, wo)
            assert p.lds_bytes == p.rows_wmax * (4 * c + 12) and p.lds_optin == int(p.lds_bytes > 64 * 1024)
            assert lib.msl_loss_workspace(c, 3, wi, 5, wo) >= max(p.ws_required,
                                                                  hip.loss_plan("up_fwd", c, 3, wi, 5, wo).ws_required)
        assert p.per == -(-wi // p.rows_chunks) and p.rows_wmax <= wo
        # the bound's own arithmetic: (per + 1) columns of at most ceil(1 / sw) + 2 pixels each, clamped to the row.
        # Over this sweep no chunk needs the + 2 (the count per column never exceeds ceil(1 / sw)); it is the margin
        # against an fp32 product landing on the other side of an integer, so its value is pinned here, not found
        # by an overflow.
        each = math.ceil(1.0 / float(np.float32(wi - 1) / np.float32(wo - 1))) + 2 if wi >= 2 and wo >= 2 else wo
        assert p.rows_wmax == min(wo, (p.per + 1) * each), (wi, wo, p.rows_wmax)
        for ixa, ixb, lo, hi in lc.chunk_ranges(wi, wo, p.rows_chunks):
            assert ixa < ixb, "empty chunk: wi %d wo %d chunks %d" % (wi, wo, p.rows_chunks)
            assert hi - lo <= p.rows_wmax, "chunk [%d, %d) of wi %d wo %d needs %d pixels, planned %d" % (
                ixa, ixb, wi, wo, hi - lo, p.rows_wmax)
        n += 1
    assert n >= 20000


# ------------------------------------------------------------------------------------------ the reference itself
def _torch_loss(kind, up, dec, c):
    """The formulas tests/test_gpu_ops.py::test_fused_losses and utils/loss.py use, on torch's own upsample."""
    if kind in ("ce", "multi_ce", "hard_ce"):
        return F.cross_entropy(up, dec["label"].unsqueeze(0), ignore_index=-1)
    prob = F.softmax(up, 1)
    if kind == "maxsquare":
        return -torch.mean(prob ** 2) / 2
    if kind == "iw_maxsquare":
        return -torch.sum(prob ** 2 * dec["w"][dec["arg"]]) / c
    terms = -F.log_softmax(up, 1) * prob
    return terms.mean() if kind == "entropy" else torch.sum(terms.sum(1) * dec["w"][dec["arg"]]) / c


@pytest.mark.parametrize("row", UP_ROWS)
def test_reference_agrees_with_torch_in_double(row):
    """With its weights taken in fp64 too, loss_ref is F.interpolate + torch's losses in double: 1e-12 on the loss,
    1e-10 on the gradient.  With the fp32 weights it differs by the weights' rounding alone."""
    cs = row[2]
    ref32 = lc.reference(cs)
    lr.WEIGHTS[0] = np.float64
    try:
        ref = lc.reference(cs)
    finally:
        lr.WEIGHTS[0] = np.float32
    low = lc.logits(cs).double().requires_grad_()
    up = F.interpolate(low, size=(cs.ho, cs.wo), mode="bilinear", align_corners=True)
    loss = _torch_loss(cs.kind, up, ref, cs.c)
    if not np.isfinite(ref["loss"]):
        assert torch.isnan(loss) and ref["dlow"].abs().max() == 0 and ref["A"].abs().max() == 0
        return
    (d,) = torch.autograd.grad(loss * cs.gout, low)
    assert abs(loss.item() - ref["loss"]) <= 1e-12 * max(abs(ref["loss"]), 1e-300) or loss.item() == ref["loss"]
    assert lr.rel(ref["dlow"], d) <= 1e-10 or d.abs().max() == 0
    # fp32 weights: each differs from the exact one by at most 2^-23 of the source index (the scale and the
    # product each round once); the loss is Lipschitz in the logits, which move by that times their own size
    for n_in, n_out in ((cs.hi, cs.ho), (cs.wi, cs.wo)):
        w32, w64 = lr.dense(n_in, n_out), None
        lr.WEIGHTS[0] = np.float64
        try:
            w64 = lr.dense(n_in, n_out)
        finally:
            lr.WEIGHTS[0] = np.float32
        assert (w32 - w64).abs().max().item() <= 2.0 ** -23 * n_in
    if "tie" not in cs.data:  # (a tie's decision may legitimately fall either way between the two weightings)
        shift = 2.0 ** -22 * (cs.hi + cs.wi) * low.detach().abs().max().item()
        assert abs(ref32["loss"] - ref["loss"]) <= 4 * shift * max(1.0, abs(cs.gout)) + 1e-12


def test_reference_upsample_agrees_with_torch_in_double():
    for hi, wi, ho, wo in ((3, 5, 7, 11), (33, 33, 9, 9), (5, 100, 1, 333), (3, 1, 7, 9)):
        g = torch.Generator().manual_seed(wo)
        x, gy = torch.randn(1, 3, hi, wi, generator=g), torch.randn(1, 3, ho, wo, generator=g)
        lr.WEIGHTS[0] = np.float64
        try:
            y, _ = lr.upsample_fwd(x, (ho, wo))
            dx, _ = lr.upsample_bwd(gy, hi, wi)
        finally:
            lr.WEIGHTS[0] = np.float32
        xd = x.double().requires_grad_()
        yt = F.interpolate(xd, size=(ho, wo), mode="bilinear", align_corners=True)
        assert torch.allclose(y, yt.detach(), rtol=1e-12, atol=1e-12)
        assert torch.allclose(dx, torch.autograd.grad(yt, xd, gy.double())[0], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("row", [r for r in ROWS if r.values[0][2].op in ("up", "labels", "pseudo")])
def test_decision_margins(row):
    """No pixel's decision is within MARGIN of flipping, except the deliberately tied node pixels, which are tied
    exactly.  (The prob and soft forms decide on the fp32 values they are given: nothing is computed before the
    comparison, so there is nothing to keep clear of.)  A condition on the inputs; no pixel is excluded from any
    comparison."""
    cs = row[2]
    hw = (cs.ho, cs.wo)
    if cs.op == "up":
        m = lc.reference(cs)["margin"].clone()
    elif cs.op == "labels" and "solo" in cs.data:
        m = lr.up_labels(lc.logits(cs), None, hw, cs.thr)[1]
    elif cs.op == "labels":
        _, g1, _, g2 = lr.up_labels(lc.logits(cs), lc.logits(cs, 1), hw, cs.thr)
        m = torch.minimum(g1, g2)
    else:
        _, g1, _, g2 = lr.pseudo_labels(lc.logits(cs), hw, cs.thr)
        m = torch.minimum(g1, g2)
    if "tie" in cs.data:
        for oy, ox in lc.tie_nodes(cs)[1]:
            assert m[oy, ox] == 0
            m[oy, ox] = float("inf")
    assert m.min().item() >= lc.MARGIN


def test_k_follows_the_cpu_fp32_measurement():
    """K of every loss kind is 4 x the worst ratio of torch-CPU fp32 autograd over TABLE, rounded up to a power of
    two (the figures: profiles/loss_forms_errors.txt).  The measurement's last digits depend on torch's own fp32
    summation order, so this holds K to the rule within one doubling instead of to the digit."""
    worst = {}
    for _, _, cs in lc.TABLE:
        if cs.op in ("up", "prob", "soft"):
            kind, r = lc.cpu_fp32_ratio(cs)
            worst[kind] = max(worst.get(kind, 0.0), r)
    assert set(worst) == set(lc.K)
    for kind, r in sorted(worst.items()):
        print("%-13s cpu-fp32 worst ratio %8.3f  rule %4d  K %4d" % (kind, r, lc.k_rule(r), lc.K[kind]))
        assert lc.k_rule(r) // 2 <= lc.K[kind] <= 2 * lc.k_rule(r), kind
