"""The coverage gate of the BatchNorm kernels (CPU only: msl_bn_plan launches nothing).

csrc/bn.hip sends every BN call to a fused instantiation or to the flat kernels by thresholds in p, c and nimg, and
refuses some combinations of its nullable operands.  This module plans a committed grid of calls
(bn_form_cases.grid) through the library itself - msl_bn_plan calls the functions the launch calls - and holds
tests/bn_form_cases.py TABLE, the cases test_gpu_bn_forms.py compares with fp64, against it: a threshold edit that
sends some shape to a kernel no case runs, or a case that no longer runs the kernel it is filed under, fails here,
before any GPU is involved.  It also checks the fp64 reference (bn_ref.py) against torch's own batch norm.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import bn_form_cases as bc
import bn_ref
from maxsquareloss_amd import hip

# Built instantiations no call reaches, with the reason.  k_bn_bwd_fused<16, true> is not built at all
# (kBnJoint16Bwd = false: the joint backward spills at 16 elements), so "bwd:joint.16" is no key; that no backward
# plan is joint at 16 is pinned below, so flipping the constant fails here until a case is added.
UNREACHED = set()


@pytest.fixture(scope="module")
def swept():
    return bc.reached(hip, bc.grid())


def _table(kind):
    i = {"shape": 1, "image": 2}[kind]
    return {(row[0], row[i]) for row in bc.TABLE}


def test_every_reachable_key_and_class_has_a_case(swept):
    shapes, images = swept
    need = {kc for kc in shapes if kc[1] != "other"}
    missing = sorted(need - _table("shape"))
    hint = ["%s %s: e.g. %s" % (k, c, tuple(bc.suggest(shapes[(k, c)]))) for k, c in missing]
    assert not missing, "reachable (key, shape class) pairs without a case:\n" + "\n".join(hint)
    missing = sorted(set(images) - _table("image"))
    hint = ["%s %s: e.g. %s" % (k, c, tuple(bc.suggest(images[(k, c)]))) for k, c in missing]
    assert not missing, "reachable (key, image class) pairs without a case:\n" + "\n".join(hint)
    # every class is reached where it can be: the fused forms in all three shapes (fused.33 included), the flat
    # vec kernels in all five, the scalar ones at least in single and rows
    for key in bc.ALL_KEYS:
        got = {c for k, c in need if k == key}
        if "flat" not in key:
            assert got == set(bc.FUSED_SHAPES), key
            assert {c for k, c in images if k == key} == ({"pair"} if "joint" in key else {"one", "loop2", "loop3"}), key
        else:
            assert got == set(bc.FLAT_SHAPES), key
            assert {c for k, c in images if k == key} == {"img1", "img2", "img3"}, key
    print("%d keys, %d (key, shape) and %d (key, image) pairs on the grid, all with a case; %d cases" % (
        len({k for k, _ in shapes}), len(need), len(images), len(bc.TABLE)))


def test_every_built_instantiation_is_reached(swept):
    shapes, _ = swept
    keys = {k for k, _ in shapes}
    assert len(bc.ALL_KEYS) == 21
    assert set(bc.ALL_KEYS) - keys == UNREACHED and keys <= set(bc.ALL_KEYS)
    assert "bwd:joint.16" not in keys  # kBnJoint16Bwd
    assert {row[0] for row in bc.TABLE} == set(bc.ALL_KEYS)


def test_every_key_sees_every_option_value():
    have = {}
    for key, _, _, case in bc.TABLE:
        have.setdefault(key, set()).update(bc.option_values(case, key))
    for key in bc.ALL_KEYS:
        missing = sorted(bc.options_needed(key) - have[key], key=str)
        assert not missing, "%s never runs with %s" % (key, missing)
    # accumulate_params onto given buffers (the trainer's call), per backward key
    acc = {key for key, _, _, c in bc.TABLE if c.dir == "bwd" and c.acc and c.dparams}
    assert acc == {k for k in bc.ALL_KEYS if k.startswith("bwd:")}


@pytest.mark.parametrize("key,shape,image,case", bc.TABLE, ids=[str(i) for i in range(len(bc.TABLE))])
def test_table_case_lands_where_it_is_filed(key, shape, image, case):
    pl = bc.plan_of(hip, case)
    assert pl.status == bc.MSL_OK
    assert (bc.plan_key(case, pl), bc.shape_class(case, pl), bc.image_class(case, pl)) == (key, shape, image)
    assert bc.elems(case) <= bc.CASE_MAX_ELEMS
    if case.dir == "fwd":
        assert (case.src, case.dx, case.dres, case.dparams, case.acc) == ("none", 0, 0, 0, 0)  # the backward's fields
        assert not case.mask or (case.relu and pl.fused)
    else:
        assert (case.mask, case.upd, case.nbt) == (0, 0, 0)  # the forward's fields
        assert case.src in bc.SOURCES and case.relu == int(case.src != "none")
        assert not (case.src == "recompute" and case.residual)
        assert case.dx or not case.absmax
        assert case.dx or case.dres or case.dparams  # the call writes something
    if not case.aligned:
        assert pl.fused or not pl.vec


def test_table_has_no_duplicates_and_holds_the_named_edges():
    cases = [row[3] for row in bc.TABLE]
    assert len(set(cases)) == len(cases)
    plans = [(key, c, bc.plan_of(hip, c)) for key, _, _, c in bc.TABLE]
    for d in ("fwd", "bwd"):
        mine = [(k, c, pl) for k, c, pl in plans if c.dir == d]
        # one-wave rows and the one-element row on the smallest form, in the image loop
        assert any(pl.fused and pl.ept == 4 and not pl.joint and c.p == 1 for _, c, pl in mine)
        assert any(pl.fused and pl.ept == 4 and not pl.joint and 1 < c.p <= 63 for _, c, pl in mine)
        # the joint forms at the last channel count that takes them and at one channel, per size
        for e in (4, 9) + ((16,) if d == "fwd" else ()):
            assert {c.c for _, c, pl in mine if pl.joint and pl.ept == e} >= {1, 256}, (d, e)
        # the pair in the image loop: from 257 channels (any count for the backward at 16 elements)
        for e in (4, 9, 16):
            loop2 = [c for _, c, pl in mine if pl.fused and not pl.joint and pl.ept == e and c.nimg == 2]
            assert loop2 and all(c.c == 257 or (d == "bwd" and e == 16) for c in loop2), (d, e)
        # the 33-element form at exactly 128 channels, at both ends
        assert {c.p for _, c, pl in mine if pl.fused and pl.ept == 33 and c.c == 128} >= {16385, 33792}
        assert all(c.c == 128 for _, c, pl in mine if pl.fused and pl.ept == 33)
        # the float4 body on rows that start off 16 bytes
        assert any(not pl.fused and pl.vec and c.p % 4 and c.nimg >= 2 for _, c, pl in mine)
        # a shrunk chunk that stages close to 256 rows, and the scalar kernels on whole rows and on many rows
        assert any(not pl.fused and pl.chunk < 4096 and c.c * c.nimg >= 300 and pl.max_rows >= 200 for _, c, pl in mine)
        assert any(not pl.fused and pl.S == 16 and c.c <= 2 and c.p == 122881 for _, c, pl in mine)
        # x around 40 (the cancellation case) on half of the cases, around 1 on the rest
        far = sum(c.far for _, c, _ in mine)
        assert abs(2 * far - len(mine)) <= 0.2 * len(mine), (d, far, len(mine))


def _fwd(c, p, nimg=1, training=1, fused=1, ws_bytes=None, **kw):
    return bc.plan_of(hip, bc.F(c, nimg, p, training=training, bn_fused=fused, **kw), ws_bytes=ws_bytes)


def _bwd(c, p, nimg=1, training=1, fused=1, ws_bytes=None, **kw):
    return bc.plan_of(hip, bc.B(c, nimg, p, training=training, bn_fused=fused, **kw), ws_bytes=ws_bytes)


def test_form_boundaries():
    """The thresholds of bn_fused_shape and bn_fused_select, from both sides, in both directions."""
    for plan in (_fwd, _bwd):
        for c in (1, 127, 128, 300):
            for lo, hi, e0, e1 in ((4096, 4097, 4, 9), (9216, 9217, 9, 16)):
                assert (plan(c, lo).ept, plan(c, hi).ept) == (e0, e1)
            assert plan(c, 1).ept == 4 and plan(c, 16384).ept == 16
            assert plan(c, 16385).fused == int(c >= 128) and plan(c, 33792).fused == int(c >= 128)
            assert plan(c, 33793).fused == 0 and plan(c, 122881).fused == 0
        assert plan(128, 16385).ept == 33 and plan(128, 33792).ept == 33
        for p in (1, 4096, 9216, 16384, 33792):  # never fused: eval mode, or the form switched off
            assert plan(256, p, training=0).fused == 0 and plan(256, p, fused=0).fused == 0
        # the joint forms: a pair of at most 256 channels, up to 9 elements (the forward up to 16)
        for p, e in ((4096, 4), (9216, 9), (16384, 16)):
            top = int(e < 16 or plan is _fwd)
            assert plan(256, p, nimg=2).joint == top and plan(1, p, nimg=2).joint == top
            assert plan(257, p, nimg=2).joint == 0
            assert plan(256, p, nimg=1).joint == 0 and plan(256, p, nimg=3).joint == 0
        assert plan(256, 16385, nimg=2).joint == 0
    # no backward plan is joint at 16 elements (kBnJoint16Bwd): flipping the constant needs a case first
    for cs in bc.grid():
        pl = bc.plan_of(hip, cs)
        assert not (cs.dir == "bwd" and pl.joint and pl.ept == 16), cs


def test_plans_are_consistent_with_their_kernels(swept):
    shapes, _ = swept
    lib = hip.load(require_gpu=False)
    for (key, cls), cases in shapes.items():
        for cs in cases[:: max(1, len(cases) // 40)]:
            pl = bc.plan_of(hip, cs)
            c, n, p = cs.c, cs.nimg, cs.p
            assert pl.S == max(1, min(16, -(-p // 8192)))
            assert lib.msl_bn_workspace(c, p, n) == -(-(c * n * pl.S * 16) // 256) * 256
            assert pl.chunk % 4 == 0 and pl.chunk // p + 2 <= 256 and (pl.chunk == 4096 or 2 * pl.chunk // p + 2 > 256)
            if pl.fused:
                assert cs.training and cs.bn_fused and pl.launches == 1
                assert (pl.grid_x[0], pl.grid_y[0], pl.block[0]) == (c, 1, 1024)
                assert bc.PREV_BLOCKS[pl.ept] * 1024 < p <= pl.ept * 1024
                assert (pl.vec, pl.max_rows) == (0, 0)
                assert not pl.joint or (n == 2 and c <= 256)
                continue
            assert (pl.ept, pl.joint) == (0, 0) and pl.vec == cs.aligned
            blocks = -(-(c * n * p) // pl.chunk)
            two = cs.dir == "bwd" or cs.training  # the reduce / statistics launch
            assert pl.launches == 1 + int(two)
            if two:
                assert (pl.grid_x[0], pl.grid_y[0], pl.block[0]) == (c * n, pl.S, 256)
            assert (pl.grid_x[pl.launches - 1], pl.grid_y[pl.launches - 1], pl.block[pl.launches - 1]) == (blocks, 1, 256)
            assert 1 <= pl.max_rows <= 256  # the LDS coefficient arrays of the apply kernels hold 256 rows
            if blocks <= 3000:
                rows = max((min(c * n * p, (b + 1) * pl.chunk) - 1) // p - b * pl.chunk // p + 1 for b in range(blocks))
                assert pl.max_rows == rows, cs
    # eval mode zeroes the maxima in a launch of its own
    pl = bc.plan_of(hip, bc.F(300, 2, 63, training=0, absmax=1))
    assert pl.launches == 2 and (pl.grid_x[0], pl.grid_y[0], pl.block[0]) == (2, 1, 256)


def test_refusals():
    """What the calls refuse, through the plan's status."""
    ok, arg, wsp = bc.MSL_OK, bc.MSL_ERR_ARG, bc.MSL_ERR_WORKSPACE
    # the mask bits: fused kernels with relu only, in both directions
    assert _fwd(64, 4096, relu=1, mask=1).status == ok
    assert _fwd(64, 4096, relu=0, mask=1).status == arg
    assert _fwd(64, 4096, relu=1, mask=1, fused=0).status == arg
    assert _fwd(64, 4096, relu=1, mask=1, training=0).status == arg
    assert _fwd(64, 16385, relu=1, mask=1).status == arg and _fwd(128, 16385, relu=1, mask=1).status == ok
    assert _bwd(64, 4096, src="bits").status == ok and _bwd(128, 33792, src="bits").status == ok
    assert _bwd(64, 4096, src="bits", fused=0).status == arg and _bwd(64, 4096, src="bits", training=0).status == arg
    assert _bwd(64, 33793, src="bits").status == arg
    # y = NULL: the fused forms up to 16 elements alone ...
    assert _bwd(64, 16384, src="recompute").status == ok and _bwd(64, 1, src="recompute", nimg=3).status == ok
    assert _bwd(128, 16385, src="recompute").status == arg  # (fused, at 33 elements)
    assert _bwd(64, 4096, src="recompute", fused=0).status == arg
    assert _bwd(64, 4096, src="recompute", training=0).status == arg
    # ... and never through msl_bn_bwd / msl_bn_bwd_am
    lib = hip.load(require_gpu=False)
    out = hip.BnPlan()
    fm = hip.Forms(5, 1, 1, 1)

    def raw(backward, c, p, nimg, training, relu, aligned, entry, src, dx, am, mask, ws=None, o=out, f=fm):
        ws = lib.msl_bn_workspace(c, p, nimg) if ws is None else ws
        return lib.msl_bn_plan(backward, c, p, nimg, training, relu, aligned, entry, src, dx, am, mask, ws,
                               None if f is None else ctypes.addressof(f), None if o is None else ctypes.addressof(o))

    assert raw(1, 64, 4096, 1, 1, 1, 1, 0, 3, 1, 0, 0) == ok and out.status == arg   # msl_bn_bwd_am, y = NULL
    assert raw(1, 64, 4096, 1, 1, 1, 1, 1, 3, 1, 0, 0) == ok and out.status == ok    # msl_bn_bwd_am_beta
    assert raw(1, 64, 4096, 1, 1, 0, 1, 2, 2, 1, 0, 0) == ok and out.status == arg   # msl_bn_bwd_mask without relu
    # absmax_dx needs dx
    assert _bwd(64, 4096, dx=0, absmax=1, dres=1).status == arg and _bwd(64, 4096, dx=1, absmax=1).status == ok
    assert _bwd(64, 33793, dx=0, absmax=1, dres=1).status == arg
    # a workspace one byte short (the forward needs none in eval mode)
    for plan in (_fwd, _bwd):
        for c, p, n in ((64, 4096, 2), (3, 122881, 1), (64, 63, 3)):
            for fused in (0, 1):
                need = lib.msl_bn_workspace(c, p, n)
                assert need >= c * n * max(1, min(16, -(-p // 8192))) * 16
                assert plan(c, p, nimg=n, fused=fused, ws_bytes=need).status == ok
                assert plan(c, p, nimg=n, fused=fused, ws_bytes=need - 1).status == wsp
    assert _fwd(64, 4096, training=0, ws_bytes=0).status == ok and _bwd(64, 4096, training=0, ws_bytes=0).status == wsp
    # c * nimg from 2^31 on, and sizes below 1
    assert raw(0, 2 ** 30, 1, 2, 0, 0, 1, 0, 0, 0, 0, 0, ws=0) == ok and out.status == arg
    assert raw(1, 2 ** 30, 1, 2, 0, 0, 1, 0, 0, 1, 0, 0, ws=2 ** 40) == ok and out.status == arg
    assert raw(0, 2 ** 30 - 1, 1, 2, 0, 0, 1, 0, 0, 0, 0, 0, ws=0) == ok and out.status == ok
    for c, p, n in ((0, 5, 1), (5, 0, 1), (5, 5, 0)):
        assert raw(0, c, p, n, 1, 0, 1, 0, 0, 0, 0, 0, ws=2 ** 20) == ok and out.status == arg
        assert raw(1, c, p, n, 1, 0, 1, 0, 0, 1, 0, 0, ws=2 ** 20) == ok and out.status == arg
    # a forms record the library does not know
    assert raw(0, 64, 4096, 1, 1, 0, 1, 0, 0, 0, 0, 0, f=hip.Forms(5, 1, 1, 7)) == ok and out.status == arg
    assert raw(0, 64, 4096, 1, 1, 0, 1, 0, 0, 0, 0, 0, f=None) == ok and out.status == ok and out.fused == 1
    # arguments that describe no call: the query itself refuses, out untouched
    out.status = 77
    bad = [(0, 64, 4096, 1, 1, 0, 1, 0, 0, 0, 0, 0, None, None),      # no out
           (2, 64, 4096, 1, 1, 0, 1, 0, 0, 0, 0, 0), (0, 64, 4096, 1, 2, 0, 1, 0, 0, 0, 0, 0),
           (0, 64, 4096, 1, 1, 0, 1, 1, 0, 0, 0, 0), (0, 64, 4096, 1, 1, 1, 1, 0, 1, 0, 0, 0),  # forward with an entry / a source
           (0, 64, 4096, 1, 1, 0, 1, 0, 0, 1, 0, 0),                                         # forward with dx
           (1, 64, 4096, 1, 1, 1, 1, 0, 0, 1, 0, 0),                                         # relu without a source
           (1, 64, 4096, 1, 1, 1, 1, 0, 2, 1, 0, 0), (1, 64, 4096, 1, 1, 1, 1, 2, 1, 1, 0, 0),  # bits <=> msl_bn_bwd_mask
           (1, 64, 4096, 1, 1, 1, 1, 3, 1, 1, 0, 0), (1, 64, 4096, 1, 1, 1, 1, 0, 4, 1, 0, 0),
           (1, 64, 4096, 1, 1, 1, 1, 0, 1, 1, 0, 1)]                                          # backward with has_mask
    for a in bad:
        assert raw(*a) == arg, a
    assert out.status == 77


# ------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("c,nimg,p,training,relu,res,affine", [(3, 2, 37, 1, 1, 1, 1), (5, 3, 130, 1, 0, 0, 1),
                                                               (4, 2, 64, 0, 1, 0, 1), (3, 1, 50, 1, 1, 0, 0),
                                                               (2, 2, 9, 0, 0, 1, 0)])
def test_reference_agrees_with_torch(c, nimg, p, training, relu, res, affine):
    """bn_ref's explicit formulas against F.batch_norm and autograd in fp64, image by image (p > 1)."""
    d = bn_ref.make_inputs(c, nimg, p, 7, training, relu, res, affine, far=1)
    x, dy = d["x"], d["dy"]
    f = bn_ref.forward(x, d["gamma"], d["beta"], d["residual"], d["running_mean"], d["running_var"], 5, training, 1, relu)
    b = bn_ref.backward(dy, x, (f["y"] > 0) if relu else None, d["gamma"], f["mean"].float().double(),
                        f["invstd"].float().double(), training, d["dgamma0"], d["dbeta0"])
    rm, rv = d["running_mean"].double().clone(), d["running_var"].double().clone()
    gam = (torch.ones(c) if d["gamma"] is None else d["gamma"]).double().requires_grad_()
    bet = (torch.zeros(c) if d["beta"] is None else d["beta"]).double().requires_grad_()
    dgam, dbet = d["dgamma0"].double().clone(), d["dbeta0"].double().clone()
    for n in range(nimg):
        xi = x[:, n].double().reshape(1, c, p, 1).requires_grad_()
        y = F.batch_norm(xi, rm, rv, gam, bet, bool(training), bn_ref.MOMENTUM, bn_ref.EPS)
        if res:
            y = y + d["residual"][:, n].double().reshape(1, c, p, 1)
        if relu:
            y = torch.relu(y)
        gx, gg, gb = torch.autograd.grad(y, (xi, gam, bet), dy[:, n].double().reshape(1, c, p, 1))
        dgam, dbet = dgam + gg, dbet + gb
        assert torch.allclose(y.detach().reshape(c, p), f["y"][:, n], rtol=1e-12, atol=1e-12)
        # (the reference's backward reads the saved statistics as the library does: rounded to fp32)
        assert torch.allclose(gx.reshape(c, p), b["dx"][:, n], rtol=1e-5, atol=1e-6)
    assert torch.allclose(rm, f["running_mean"], rtol=1e-12, atol=1e-12)
    assert torch.allclose(rv, f["running_var"], rtol=1e-12, atol=1e-12)
    assert torch.allclose(dgam, b["dgamma"], rtol=1e-5, atol=1e-5) and torch.allclose(dbet, b["dbeta"], rtol=1e-9, atol=1e-9)
    assert f["nbt"] == (5 + nimg if training else 5)


@pytest.mark.parametrize("c,nimg,p", [(3, 1, 1), (3, 2, 37), (5, 2, 4097), (300, 2, 5), (2, 1, 122881)])
def test_inputs_keep_clear_of_the_relu_edge(c, nimg, p):
    """make_inputs leaves no pre-activation within MARGIN * max|z| of zero, which is far above what the fp32
    arithmetic of fma(x, alpha, bsh) + r can move it (2^-23 * (|x alpha| + |bsh| + |z|))."""
    for training in (0, 1):
        for far in (0, 1):
            d = bn_ref.make_inputs(c, nimg, p, c + p, training, 1, 1, 1, far)
            f = bn_ref.forward(d["x"], d["gamma"], d["beta"], d["residual"], d["running_mean"], d["running_var"], None,
                               training, 0, 1)
            z = f["z"]
            margin = z.abs().min().item()
            assert margin >= 0.9 * bn_ref.MARGIN * z.abs().max().item()
            alpha = (f["invstd"] * d["gamma"].double()[:, None])[..., None]
            fp32 = 2.0 ** -23 * ((d["x"].double() * alpha).abs().max().item() * 2 + z.abs().max().item())
            assert margin >= 10 * fp32, (margin, fp32)


def test_pack_bits_and_ulps():
    pos = torch.zeros(2, 130, dtype=torch.bool)
    pos[0, 0] = pos[0, 63] = pos[0, 64] = pos[1, 129] = True
    w = bn_ref.pack_bits(pos)
    assert w.shape == (2, 3) and w[0].tolist() == [1 - 2 ** 63, 1, 0] and w[1].tolist() == [0, 0, 2]
    one = torch.tensor([1.0, 1.0, -3.0])
    got = torch.tensor([1.0 + 2.0 ** -23, 1.0, -3.0 - 2.0 ** -21])
    assert bn_ref.ulp_distance(got, one).tolist() == [1.0, 0.0, 2.0]
