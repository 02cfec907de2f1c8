"""Every BN kernel form and option against fp64, straight through the C ABI (GPU only).

One test over tests/bn_form_cases.py TABLE.  A forward case is one msl_bn_fwd_mask call, a backward case one
msl_bn_bwd_am / msl_bn_bwd_am_beta / msl_bn_bwd_mask call on the reference's own saved statistics, output and mask
bits (rounded to fp32 once), so a backward kernel is held to the reference without a forward kernel in between.
The reference is tests/bn_ref.py: explicit fp64 formulas on the CPU, on inputs without a pre-activation near zero,
so the ReLU masks must agree everywhere.  Bars: y, dx, dgamma, dbeta and the running statistics within 1e-5 of
max|ref| (an all-zero reference exactly), the saved statistics within 1 fp32 ulp, everything
else exact.  Each call must also write its outputs wholly and nothing else (NaN pre-fill, guard words around every
output, a guard tail behind the queried workspace), leave its operands alone, give the same bytes whatever the
workspace held and through every ReLU source the case allows, and - for two and three images - the bytes of that
many one-image calls made in order, the invariant csrc/bn.hip documents.

The table found one defect when it first ran: the forward at p = 1 in train mode with x around 40 missed the y bar
(fwd:fused.4 3x3x1: 4.5e-4 off where the reference is exactly 0; fwd:joint.4 1x2x1: 6.8e-5).  A one-element row has
variance 0, so invstd = 1 / sqrt(eps) = 316, and y = fma(x, alpha, beta - mean alpha) cancelled x alpha = 12 650
against an fp32-rounded term of the same size, where the exact result is beta.  The kernels now give a constant row
(every element equal to the first) alpha = 0, and the backward's mask recompute does the same;
test_constant_rows holds that at one and many pixels, with beta at and next to zero.
"""
import ctypes

import pytest
import torch

import bn_form_cases as bc
import bn_ref

pytestmark = pytest.mark.gpu

from maxsquareloss_amd import hip  # noqa: E402

DEV = "cuda"
GUARD_WORD = 0x5A5A5A5B  # a finite float no kernel computes
GUARD = 1024             # elements before and behind every output
WS_GUARD = 4096
BAR = 1e-5
NBT0 = 5


def _sync():
    torch.cuda.synchronize()


class _Buf:
    """`n` elements between guard words, on the device; aligned = 0 starts them 4 bytes (one float) off 16-byte
    alignment, as a buffer sliced at [1:]."""

    def __init__(self, n, dtype=torch.float32, aligned=1, fill=None, src=None):
        off = GUARD + (0 if aligned else 1)
        self.whole = torch.empty(off + n + GUARD, dtype=dtype, device=DEV)
        self.whole.view(torch.int32).fill_(GUARD_WORD)
        self.t = self.whole[off:off + n]
        self.off, self.n = off, n
        assert self.t.data_ptr() % 16 == (0 if aligned else self.t.element_size() % 16)
        if src is not None:
            self.t.copy_(src.reshape(-1))
        elif fill is not None:
            self.t.fill_(fill)
        self.src = None if src is None else self.t.clone()

    @property
    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        g = self.whole.view(torch.int32)
        k = self.whole.element_size() // 4
        return bool((g[:self.off * k] == GUARD_WORD).all()) and bool((g[(self.off + self.n) * k:] == GUARD_WORD).all())

    def unchanged(self):
        return torch.equal(self.t.view(torch.int32), self.src.view(torch.int32))

    def cpu(self, *shape):
        return self.t.cpu().reshape(*shape)


def _ptr(b):
    return None if b is None else b.ptr


def _workspace(lib, c, p, nimg, ws_byte):
    wsb = lib.msl_bn_workspace(c, p, nimg)
    ws = torch.empty(wsb + WS_GUARD, dtype=torch.uint8, device=DEV)
    ws.fill_(ws_byte)
    ws[wsb:].fill_(0xA5)
    return ws, wsb


def _finish(name, ws, wsb, outputs, inputs):
    _sync()
    assert bool((ws[wsb:] == 0xA5).all()), "%s wrote behind its queried workspace" % name
    for tag, b in outputs.items():
        assert b is None or b.intact(), "%s wrote outside %s" % (name, tag)
    for tag, b in inputs.items():
        assert b is None or (b.intact() and b.unchanged()), "%s wrote to %s" % (name, tag)


def run_fwd(lib, case, x, res, gamma, beta, rm0, rv0, nbt0, ws_byte=0xA5):
    """One msl_bn_fwd_mask call on CPU operands x / res [c][nimg][p]; returns the outputs on the CPU."""
    c, nimg, p = x.shape
    al = case.aligned
    ins = dict(x=_Buf(c * nimg * p, aligned=al, src=x), residual=None if res is None else _Buf(c * nimg * p, aligned=al, src=res),
               gamma=None if gamma is None else _Buf(c, src=gamma), beta=None if beta is None else _Buf(c, src=beta))
    nan = float("nan")
    words = -(-p // 64)
    outs = dict(y=_Buf(c * nimg * p, aligned=al, fill=nan), save_mean=_Buf(c * nimg, fill=nan),
                save_invstd=_Buf(c * nimg, fill=nan), running_mean=_Buf(c, src=rm0), running_var=_Buf(c, src=rv0),
                nbt=_Buf(1, torch.int64, src=torch.tensor([nbt0])) if case.nbt else None,
                absmax=_Buf(c, fill=nan) if case.absmax else None,
                mask=_Buf(c * nimg * words, torch.int64, fill=-1) if case.mask else None)
    assert not case.mask or lib.msl_bn_relu_mask_bytes(c, p, nimg) == c * nimg * words * 8
    ws, wsb = _workspace(lib, c, p, nimg, ws_byte)
    fm = hip.Forms(5, 1, 1, case.bn_fused)
    rc = lib.msl_bn_fwd_mask(ins["x"].ptr, _ptr(ins["gamma"]), _ptr(ins["beta"]), _ptr(ins["residual"]), outs["y"].ptr,
                             outs["running_mean"].ptr, outs["running_var"].ptr, _ptr(outs["nbt"]), outs["save_mean"].ptr,
                             outs["save_invstd"].ptr, c, p, nimg, case.training, case.upd, bn_ref.MOMENTUM, bn_ref.EPS,
                             case.relu, ctypes.addressof(fm), ws.data_ptr(), wsb, hip.stream_ptr(), _ptr(outs["absmax"]),
                             _ptr(outs["mask"]))
    assert rc == 0, rc
    _finish("msl_bn_fwd_mask", ws, wsb, outs, ins)
    return dict(y=outs["y"].cpu(c, nimg, p), save_mean=outs["save_mean"].cpu(c, nimg),
                save_invstd=outs["save_invstd"].cpu(c, nimg), running_mean=outs["running_mean"].cpu(c),
                running_var=outs["running_var"].cpu(c), nbt=outs["nbt"].cpu(1) if case.nbt else None,
                absmax=outs["absmax"].cpu(c) if case.absmax else None,
                mask=outs["mask"].cpu(c * nimg, words) if case.mask else None)


def run_bwd(lib, case, src, acc, dy, x, y, bits, gamma, beta, sm, si, dgamma0, dbeta0, ws_byte=0xA5):
    """One backward call through the entry point of the ReLU source `src` on CPU operands [c][nimg][p]; dgamma0 /
    dbeta0: what the gradient buffers hold before the call (read only when acc)."""
    c, nimg, p = x.shape
    al = case.aligned
    n = c * nimg * p
    ins = dict(dy=_Buf(n, aligned=al, src=dy), x=_Buf(n, aligned=al, src=x),
               y=_Buf(n, aligned=al, src=y) if src == "y" else None,
               bits=_Buf(bits.numel(), torch.int64, src=bits) if src == "bits" else None,
               gamma=None if gamma is None else _Buf(c, src=gamma), beta=None if beta is None else _Buf(c, src=beta),
               save_mean=_Buf(c * nimg, src=sm), save_invstd=_Buf(c * nimg, src=si))
    nan = float("nan")
    outs = dict(dx=_Buf(n, aligned=al, fill=nan) if case.dx else None, dres=_Buf(n, aligned=al, fill=nan) if case.dres else None,
                dgamma=_Buf(c, src=dgamma0) if case.dparams else None, dbeta=_Buf(c, src=dbeta0) if case.dparams else None,
                absmax=_Buf(c, fill=nan) if case.absmax else None)
    ws, wsb = _workspace(lib, c, p, nimg, ws_byte)
    fm = hip.Forms(5, 1, 1, case.bn_fused)
    relu = int(src != "none")
    head = (ins["dy"].ptr, ins["x"].ptr)
    stats = (ins["save_mean"].ptr, ins["save_invstd"].ptr, _ptr(outs["dx"]), _ptr(outs["dres"]), _ptr(outs["dgamma"]),
             _ptr(outs["dbeta"]), c, p, nimg, case.training, relu, acc, ctypes.addressof(fm), ws.data_ptr(), wsb,
             hip.stream_ptr(), _ptr(outs["absmax"]))
    if src == "bits":
        name, rc = "msl_bn_bwd_mask", lib.msl_bn_bwd_mask(*head, ins["bits"].ptr, _ptr(ins["gamma"]), _ptr(ins["beta"]), *stats)
    elif src == "recompute":
        name, rc = "msl_bn_bwd_am_beta", lib.msl_bn_bwd_am_beta(*head, None, _ptr(ins["gamma"]), _ptr(ins["beta"]), *stats)
    else:
        name, rc = "msl_bn_bwd_am", lib.msl_bn_bwd_am(*head, _ptr(ins["y"]), _ptr(ins["gamma"]), *stats)
    assert rc == 0, (name, rc)
    _finish(name, ws, wsb, outs, ins)
    return dict(dx=outs["dx"].cpu(c, nimg, p) if case.dx else None, dres=outs["dres"].cpu(c, nimg, p) if case.dres else None,
                dgamma=outs["dgamma"].cpu(c) if case.dparams else None, dbeta=outs["dbeta"].cpu(c) if case.dparams else None,
                absmax=outs["absmax"].cpu(c) if case.absmax else None)


def _same_bytes(a, b, what):
    for k in a:
        assert (a[k] is None) == (b[k] is None), (what, k)
        if a[k] is not None:
            ia, ib = (t.view(torch.int32) if t.dtype == torch.float32 else t for t in (a[k], b[k]))
            assert torch.equal(ia, ib), "%s: %s differs" % (what, k)


def _rel(got, ref, tag, errs):
    """max|got - ref| / max|ref| into errs[tag]; an all-zero reference must be met exactly."""
    assert bool(torch.isfinite(got).all()), "%s not wholly written" % tag
    top = ref.abs().max().item()
    err = (got.double() - ref).abs().max().item()
    if top == 0.0:  # (inf fails every bar; the absolute figure is printed beside it)
        errs[tag] = 0.0 if err == 0.0 else float("inf")
        errs[tag + "_abs"] = err
    else:
        errs[tag] = err / top


def check_fwd(case, d, ref, out):
    """One forward call's outputs against the reference; returns the measured errors (asserted by the caller after
    printing)."""
    errs = {}
    c, nimg, p = d["x"].shape
    _rel(out["y"], ref["y"], "y", errs)
    for k in ("save_mean", "save_invstd"):
        assert bool(torch.isfinite(out[k]).all()), "%s not wholly written" % k
    errs["mean_ulp"] = bn_ref.ulp_distance(out["save_mean"], ref["mean"].float()).max().item()
    errs["invstd_ulp"] = bn_ref.ulp_distance(out["save_invstd"], ref["invstd"].float()).max().item()
    if case.training and case.upd:
        _rel(out["running_mean"], ref["running_mean"], "running_mean", errs)
        _rel(out["running_var"], ref["running_var"], "running_var", errs)
    else:  # untouched
        assert torch.equal(out["running_mean"], d["running_mean"]) and torch.equal(out["running_var"], d["running_var"])
    if case.nbt:
        assert out["nbt"].item() == NBT0 + (nimg if case.training and case.upd else 0)
    if case.absmax:  # max |y| of the call's own y over all images of the channel, exactly
        assert torch.equal(out["absmax"], out["y"].abs().reshape(c, -1).amax(1))
    if case.relu:
        assert torch.equal(out["y"] > 0, ref["y"] > 0), "a ReLU decision differs from the reference's"
    if case.mask:  # bit e % 64 of word [row][e / 64], the tail bits zero
        assert torch.equal(out["mask"], bn_ref.pack_bits((out["y"] > 0).reshape(c * nimg, p)))
    return errs


def assert_fwd(errs):
    assert errs["y"] <= BAR
    assert errs["mean_ulp"] <= 1.0 and errs["invstd_ulp"] <= 1.0
    assert errs.get("running_mean", 0.0) <= BAR and errs.get("running_var", 0.0) <= BAR


def check_bwd(case, d, positive, ref, out):
    errs = {}
    c, nimg, p = d["x"].shape
    if case.dres:  # where(y_ref > 0, dy, 0), bit for bit
        want = d["dy"] if positive is None else torch.where(positive, d["dy"], torch.zeros_like(d["dy"]))
        assert torch.equal(out["dres"].view(torch.int32), want.view(torch.int32)), "dres is not the masked dy"
    if case.dx:
        _rel(out["dx"], ref["dx"], "dx", errs)
    if case.dparams:
        _rel(out["dgamma"], ref["dgamma"], "dgamma", errs)
        _rel(out["dbeta"], ref["dbeta"], "dbeta", errs)
    if case.absmax:
        assert torch.equal(out["absmax"], out["dx"].abs().reshape(c, -1).amax(1))
    return errs


def assert_bwd(errs):
    for k in ("dx", "dgamma", "dbeta"):
        assert errs.get(k, 0.0) <= BAR, k


def _seed(case):
    return (case.c * 131 + case.p * 7 + case.nimg * 3 + (case.dir == "bwd") * 17 + case.training * 5 + case.relu) % (2 ** 31)


def forward_case(lib, case, name):
    c, nimg, p = case.c, case.nimg, case.p
    d = bn_ref.make_inputs(c, nimg, p, _seed(case), case.training, case.relu, case.residual, case.affine, case.far)
    x, res, gamma, beta, rm0, rv0 = (d[k] for k in ("x", "residual", "gamma", "beta", "running_mean", "running_var"))
    ref = bn_ref.forward(x, gamma, beta, res, rm0, rv0, NBT0, case.training, case.upd, case.relu)
    first = run_fwd(lib, case, x, res, gamma, beta, rm0, rv0, NBT0, 0xA5)
    errs = check_fwd(case, d, ref, first)
    print("bn %s: %s" % (name, " ".join("%s %.3e" % kv for kv in sorted(errs.items()))))
    assert_fwd(errs)
    for ws_byte in (0xFF, 0x00):  # bit-reproducible, whatever the workspace held
        _same_bytes(first, run_fwd(lib, case, x, res, gamma, beta, rm0, rv0, NBT0, ws_byte), "workspace %#x" % ws_byte)
    if nimg >= 2:  # the bytes of nimg one-image calls made in order
        rm, rv, nbt, am = rm0, rv0, NBT0, None
        for n in range(nimg):
            one = run_fwd(lib, case, x[:, n:n + 1].contiguous(), None if res is None else res[:, n:n + 1].contiguous(), gamma,
                          beta, rm, rv, nbt)
            rm, rv, nbt = one["running_mean"], one["running_var"], one["nbt"].item() if case.nbt else NBT0
            part = dict(y=first["y"][:, n:n + 1], save_mean=first["save_mean"][:, n:n + 1],
                        save_invstd=first["save_invstd"][:, n:n + 1],
                        mask=first["mask"].reshape(c, nimg, -1)[:, n].reshape(c, -1) if case.mask else None)
            _same_bytes({k: one[k] for k in part}, part, "image %d alone" % n)
            if case.absmax:
                am = one["absmax"] if am is None else torch.maximum(am, one["absmax"])
        last = dict(running_mean=rm, running_var=rv, absmax=am, nbt=torch.tensor([nbt]) if case.nbt else None)
        _same_bytes(last, {k: first[k] for k in last}, "after %d one-image calls" % nimg)
    return errs


def backward_case(lib, case, name):
    c, nimg, p = case.c, case.nimg, case.p
    d = bn_ref.make_inputs(c, nimg, p, _seed(case), case.training, case.relu, case.residual, case.affine, case.far)
    x, dy, gamma, beta = d["x"], d["dy"], d["gamma"], d["beta"]
    f = bn_ref.forward(x, gamma, beta, d["residual"], d["running_mean"], d["running_var"], None, case.training, 0, case.relu)
    sm, si, y = f["mean"].float(), f["invstd"].float(), f["y"].float()  # what a forward leaves, rounded once
    positive = (f["y"] > 0) if case.relu else None
    assert positive is None or torch.equal(y > 0, positive)
    bits = bn_ref.pack_bits(positive.reshape(c * nimg, p)) if case.relu else None
    ref = bn_ref.backward(dy, x, positive, gamma, sm, si, case.training, d["dgamma0"] if case.acc else None,
                          d["dbeta0"] if case.acc else None)
    # without accumulate the buffers start as NaN: every element must be written, not added to
    nan = torch.full((c,), float("nan"))
    g0, b0 = (d["dgamma0"], d["dbeta0"]) if case.acc else (nan, nan)

    def run(src, ws_byte=0xA5):
        return run_bwd(lib, case, src, case.acc, dy, x, y, bits, gamma, beta, sm, si, g0, b0, ws_byte)

    first = run(case.src)
    errs = check_bwd(case, d, positive, ref, first)
    print("bn %s: %s" % (name, " ".join("%s %.3e" % kv for kv in sorted(errs.items()))))
    assert_bwd(errs)
    for ws_byte in (0xFF, 0x00):
        _same_bytes(first, run(case.src, ws_byte), "workspace %#x" % ws_byte)
    if case.relu:  # every ReLU source the case allows: the same bytes
        for src in ("y", "bits", "recompute"):
            if src == case.src or (src == "recompute" and case.residual):
                continue
            if bc.plan_of(hip, case, src=src).status == bc.MSL_OK:
                _same_bytes(first, run(src), "ReLU source %s" % src)
    if nimg >= 2:  # the bytes of nimg one-image calls made in order, each accumulating onto the one before
        g, b, am, acc = g0, b0, None, case.acc
        for n in range(nimg):
            sl = slice(n, n + 1)
            one = run_bwd(lib, case, case.src, acc, dy[:, sl].contiguous(), x[:, sl].contiguous(), y[:, sl].contiguous(),
                          None if bits is None else bits.reshape(c, nimg, -1)[:, n].reshape(c, -1).contiguous(), gamma, beta,
                          sm[:, sl].contiguous(), si[:, sl].contiguous(), g, b)
            part = dict(dx=first["dx"][:, sl] if case.dx else None, dres=first["dres"][:, sl] if case.dres else None)
            _same_bytes({k: one[k] for k in part}, part, "image %d alone" % n)
            if case.dparams:
                g, b, acc = one["dgamma"], one["dbeta"], 1
            if case.absmax:
                am = one["absmax"] if am is None else torch.maximum(am, one["absmax"])
        last = dict(dgamma=g if case.dparams else None, dbeta=b if case.dparams else None, absmax=am)
        _same_bytes(last, {k: first[k] for k in last}, "after %d one-image calls" % nimg)
    return errs


@pytest.mark.parametrize("key,shape,image,case", bc.TABLE, ids=[bc.case_id(*row) for row in bc.TABLE])
def test_bn_form_against_fp64(key, shape, image, case):
    lib = hip.load()
    pl = bc.plan_of(hip, case)
    assert pl.status == bc.MSL_OK
    assert (bc.plan_key(case, pl), bc.shape_class(case, pl), bc.image_class(case, pl)) == (key, shape, image)
    name = bc.case_id(key, shape, image, case)
    (forward_case if case.dir == "fwd" else backward_case)(lib, case, name)


@pytest.mark.parametrize("c,nimg,p,fused", [(6, 3, 1, 1), (6, 1, 37, 1), (6, 2, 37, 1), (6, 2, 4097, 1), (6, 1, 9217, 1),
                                            (6, 3, 9217, 1), (6, 3, 1, 0), (6, 2, 37, 0), (6, 1, 8193, 0)])
def test_constant_rows(c, nimg, p, fused):
    """Rows constant at a large value (every row, at p = 1) beside ordinary ones, in train mode: the row normalises
    to exactly 0, so y = relu(beta + residual) as fp32 rounds that sum - beta at 0 and within 1e-6 of it included -
    and the backward gives the same bytes whether it reads y, the bits or recomputes the mask from x."""
    lib = hip.load()
    g = torch.Generator().manual_seed(c + nimg + p + fused)
    x = torch.randn(c, nimg, p, generator=g) * 3 + 40.0
    const = torch.arange(c) % 2 == 0 if p > 1 else torch.ones(c, dtype=torch.bool)
    x[const] = x[const][:, :, :1]  # every element of the row equals its first
    res = torch.randn(c, nimg, p, generator=g)
    gamma = torch.rand(c, generator=g) + 0.5
    beta = torch.tensor([0.0, 1.0, 1e-6, -1.0, -1e-6, 0.5])[:c].clone()
    rm, rv = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    dy = torch.randn(c, nimg, p, generator=g)
    for with_res in (0, 1):
        r = res if with_res else None
        case = bc.F(c, nimg, p, bn_fused=fused, relu=1, residual=with_res, absmax=1, mask=fused)
        pl = bc.plan_of(hip, case)
        assert pl.status == bc.MSL_OK and pl.fused == fused
        ref = bn_ref.forward(x, gamma, beta, r, rm, rv, NBT0, 1, 1, 1)
        out = run_fwd(lib, case, x, r, gamma, beta, rm, rv, NBT0)
        errs = {}
        _rel(out["y"], ref["y"], "y", errs)
        print("bn constant rows %dx%dx%d fused %d residual %d: y %.3e" % (c, nimg, p, fused, with_res, errs["y"]))
        assert errs["y"] <= BAR
        want = beta[:, None, None].expand(c, nimg, p) + (r if with_res else 0.0)  # one fp32 sum, as the kernel adds
        assert torch.equal(out["y"][const], torch.relu(want)[const]), "a constant row is not relu(beta + residual)"
        assert bn_ref.ulp_distance(out["save_mean"], ref["mean"].float()).max().item() <= 1.0
        assert bn_ref.ulp_distance(out["save_invstd"], ref["invstd"].float()).max().item() <= 1.0
        if case.mask:
            assert torch.equal(out["mask"], bn_ref.pack_bits((out["y"] > 0).reshape(c * nimg, p)))
        # the backward on what this forward left, through every ReLU source the shape allows
        bcase = bc.B(c, nimg, p, bn_fused=fused, src="y", residual=with_res, absmax=1, dres=1)
        outs = {}
        for src in ("y", "bits", "recompute"):
            if (src == "recompute" and with_res) or bc.plan_of(hip, bcase, src=src).status != bc.MSL_OK:
                continue
            outs[src] = run_bwd(lib, bcase, src, 0, dy, x, out["y"], out["mask"], gamma, beta, out["save_mean"],
                                out["save_invstd"], torch.zeros(c), torch.zeros(c))
        assert "y" in outs and (not fused or "bits" in outs) and (not fused or with_res or "recompute" in outs)
        for src, o in outs.items():
            _same_bytes(outs["y"], o, "ReLU source %s" % src)
        b = bn_ref.backward(dy, x, out["y"] > 0, gamma, out["save_mean"], out["save_invstd"], 1)
        errs = check_bwd(bcase, dict(x=x, dy=dy), out["y"] > 0, b, outs["y"])
        assert_bwd(errs)
