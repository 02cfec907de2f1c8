"""Every reachable weight-gradient conv kernel, reduce and schedule against fp64, straight through the C ABI (GPU only).

One test over tests/conv_wgrad_cases.py (TABLE and EDGES): workspace query, call.  The reference is fp64 on the
operands as the launched kernel's math rounds them - which math that is comes from the library's own plan
(msl_conv_wgrad_plan), not from the case: nine products of shifted views per branch, or one matrix product for pointwise.
Two bars, both the project's: max|dw - ref| / max|ref| < 1e-5 in every family, and for the
fp32-accurate maths (f32, bf16x6, f16x3) every element within 1e-6 of its own sum of |terms|
(test_f16x3_channel_spread_accuracy's bar).  Each call must also write its whole output and nothing else (NaN
pre-fill or dw0, guard words around dw and dbias, a guard tail behind the queried workspace), give the same bytes
whatever the workspace held, leave its operands alone, refuse a workspace one byte short - and, where the math
scales its operands, give the same bytes with the caller's per-row partials, hold under one tensor-wide partial
per operand (rowscale = 0) and on rows spread over eight decades.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import conv_wgrad_cases as cw

pytestmark = pytest.mark.gpu

from maxsquareloss_amd import hip  # noqa: E402

DEV = "cuda"
GUARD_WORD = 0x5A5A5A5B  # a finite float no kernel computes
GUARD = 1024  # floats before and behind dw and dbias
WS_GUARD = 4096
MSL_ERR_WORKSPACE = -2
BAR, ELEMENT_BAR = 1e-5, 1e-6


def _pow2(mx):
    """pow2_scale (csrc/dconv_kernels.h): the power of two that brings mx into [2^14, 2^15); 2^100 for zero."""
    e = torch.frexp(mx).exponent.double()
    return torch.where(mx > 0, torch.exp2((15 - e).clamp(-100, 100)), torch.full_like(e, 2.0 ** 100))


def _f16(t, per_row):
    """[rows][P] scaled by its power of two (per row or per tensor), rounded to fp16, unscaled; exact in fp64."""
    mx = t.abs().amax(1, keepdim=True) if per_row else t.abs().max().reshape(1, 1)
    sc = _pow2(mx)
    return (t.double() * sc).half().double() / sc


def _rounded(math, t, per_row):
    if math == "bf16":
        return t.bfloat16().double()
    if math == "h1p":
        return _f16(t, per_row)
    return t.double()  # f32, x6, h3p: fp32-accurate


def _dot(a, b):
    """a b^T over the pixel axis, [m][c] in fp64.  A long axis goes in 16384-pixel slabs, one batched product and a
    sum (the GPU's dgemm runs a skinny product over millions of pixels as one serial dot per tile)."""
    k, slab = a.size(1), 16384
    if k <= 4 * slab:
        return a @ b.t()
    s = k // slab  # whole slabs as views (no copies), then the tail
    a3 = a[:, :s * slab].reshape(a.size(0), s, slab).transpose(0, 1)
    b3 = b[:, :s * slab].reshape(b.size(0), s, slab).transpose(0, 1)
    return torch.bmm(a3, b3.transpose(1, 2)).sum(0) + a[:, s * slab:] @ b[:, s * slab:].t()


def _reference(case, math, per_row, x, dy, dw0):
    """(dw, sum of |terms|) in fp64 on the rounded operands, [nbranch][cout][cin][taps], on the operands' device."""
    n, h, w = case.nimg, case.h, case.w
    rx, rdy = _rounded(math, x, per_row), _rounded(math, dy, per_row)
    if case.taps == 1:
        ref, mag = _dot(rdy, rx).reshape(1, case.cout, case.cin, 1), _dot(rdy.abs(), rx.abs()).reshape(1, case.cout, case.cin, 1)
    else:
        ref = torch.zeros(case.nbranch, case.cout, case.cin, 9, dtype=torch.float64, device=x.device)
        mag = torch.zeros_like(ref)
        ady = rdy.abs()
        for b, d in zip(range(case.nbranch), (case.dil0, case.dil1)):
            xp = F.pad(rx.reshape(case.cin, n, h, w), (d, d, d, d))
            for t in range(9):
                oy, ox = (t // 3) * d, (t % 3) * d
                # x at (y + (ky - 1) d, x + (kx - 1) d), zero outside its image: einsum("mnhw,cnhw->mc") of the view
                view = xp[:, :, oy:oy + h, ox:ox + w].reshape(case.cin, -1)
                ref[b, :, :, t] = _dot(rdy, view)
                mag[b, :, :, t] = _dot(ady, view.abs())
    if dw0 is not None:
        ref, mag = ref + dw0.double().reshape(ref.shape), mag + dw0.double().abs().reshape(ref.shape)
    return ref, mag


def _fill(t, word):
    t.view(torch.int32).fill_(word if word < 2 ** 31 else word - 2 ** 32)


def _guarded(nelem):
    buf = torch.empty(GUARD + nelem + GUARD, device=DEV)
    return buf, buf[GUARD:GUARD + nelem]


def _guards_intact(buf, nelem):
    gw = buf.view(torch.int32)
    want = GUARD_WORD if GUARD_WORD < 2 ** 31 else GUARD_WORD - 2 ** 32
    return bool((gw[:GUARD] == want).all()) and bool((gw[GUARD + nelem:] == want).all())


@pytest.mark.parametrize("key,cls,case", cw.ALL_CASES, ids=[cw.case_id(*kc) for kc in cw.ALL_CASES])
def test_conv_wgrad_form_against_fp64(key, cls, case):
    lib = hip.load()
    pl = cw.plan_of(hip, case)
    assert pl.status == cw.MSL_OK
    assert (cw.plan_key(pl, case.taps), cw.schedule_class(pl)) == (key, cls)
    math = cw.MATHS[pl.math]
    scales = pl.gemm == 1 and math in ("h3p", "h1p")
    accurate = math in ("f32", "x6", "h3p")
    taps, nb, cin, cout, n, h, w, acc = case.taps, case.nbranch, case.cin, case.cout, case.nimg, case.h, case.w, case.accumulate
    p = n * h * w
    big = p >= cw.GPU_REFERENCE_PIXELS  # the reference in fp64 on the GPU
    rdev = DEV if big else "cpu"
    g = torch.Generator(device=rdev).manual_seed(cin * 131 + cout * 7 + p + taps + acc + case.dil0)
    ndw = nb * cout * cin * taps
    dw0 = torch.randn(ndw, generator=g, device=rdev) if acc else None
    db0 = torch.randn(nb * cout, generator=g, device=rdev) if acc and taps == 9 else None

    fm = hip.Forms(cw.F32_FORMS[case.f32_form], 1, 1, 1)
    fmp, st = ctypes.addressof(fm), hip.stream_ptr()
    wsb = lib.msl_dconv_wgrad_workspace(nb, cin, cout, h, w, n) if taps == 9 else lib.msl_pconv_wgrad_workspace(cin, cout, p)
    assert wsb > 0
    ws = torch.empty(wsb + WS_GUARD, dtype=torch.uint8, device=DEV)
    dwbuf, dw = _guarded(ndw)
    dbbuf, db = _guarded(nb * cout)
    sfx = {"fp32": "_sc", "fp16": "_f16", "bf16": "_bf16"}[case.family]
    dw0d = None if dw0 is None else dw0.to(DEV)
    db0d = None if db0 is None else db0.to(DEV)
    worst = {}

    def operands(spread):
        x, dy = torch.randn(cin, p, generator=g, device=rdev), torch.randn(cout, p, generator=g, device=rdev)
        if spread:  # per-row factors log-uniform over 1e-8..1
            x = x * torch.pow(10.0, -8 * torch.rand(cin, 1, generator=g, device=rdev))
            dy = dy * torch.pow(10.0, -8 * torch.rand(cout, 1, generator=g, device=rdev))
        return x, dy

    def run(xd, dyd, ws_byte, parts, ws_bytes=wsb):
        """One call; parts: None, or ((x_part, x_npart), (dy_part, dy_npart)).  Returns (status, dw, dbias)."""
        _fill(dwbuf, GUARD_WORD)
        _fill(dbbuf, GUARD_WORD)
        dw.copy_(dw0d) if acc else dw.fill_(float("nan"))
        if taps == 9:
            db.copy_(db0d) if acc else db.fill_(float("nan"))
        ws.fill_(ws_byte)
        ws[wsb:].fill_(0xA5)
        tail = ()
        if case.family != "bf16":
            (xp, xn), (dp, dn) = parts if parts else ((None, 0), (None, 0))
            tail = (hip.ptr(xp), xn, hip.ptr(dp), dn)
        if taps == 9:
            rc = getattr(lib, "msl_dconv_wgrad" + sfx)(xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), db.data_ptr(), nb, cin,
                                                       cout, h, w, n, case.dil0, case.dil1, acc, fmp, ws.data_ptr(),
                                                       ws_bytes, st, *tail)
        else:
            rc = getattr(lib, "msl_pconv_wgrad" + sfx)(xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), cin, cout, p, acc, fmp,
                                                       ws.data_ptr(), ws_bytes, st, *tail)
        torch.cuda.synchronize()
        assert _guards_intact(dwbuf, ndw), "wrote outside dw"
        assert _guards_intact(dbbuf, nb * cout), "wrote outside dbias"
        assert bool((ws[wsb:] == 0xA5).all()), "wrote behind its queried workspace"
        return rc, dw.clone(), db.clone()

    def held(tag, out, ref, mag):
        """Both bars of `out` against (ref, mag); records and prints the worst of each."""
        got = out.double().to(ref.device).reshape(ref.shape)
        assert bool(torch.isfinite(got).all()), "%s: dw not wholly written" % tag
        err = (got - ref).abs()
        rel = err.max().item() / ref.abs().max().item()
        elem = (err / mag.clamp_min(1e-300)).max().item()
        worst[tag] = (rel, elem)
        print("wgrad %s %s: max rel %.3e, per element %.3e" % (cw.case_id(key, cls, case), tag, rel, elem))
        assert rel < BAR, tag
        if accurate:
            assert elem < ELEMENT_BAR, tag

    # the one case over the MAC cap (the scalar mask cursor, 71 GMAC) runs the plain set with and without the per-row
    # partials only: the tensor-wide scale and the spread rows are k_split_rows' and the reduce's business, which the
    # other scaling cases cover, and each further set costs it another two seconds of fp64 reference
    over = case in cw.OVER_CAP
    for spread in ((False, True) if scales and not over else (False,)):
        x, dy = operands(spread)
        xd, dyd = x.to(DEV), dy.to(DEV)
        x_bytes, dy_bytes = xd.clone(), dyd.clone()
        tag = "spread" if spread else "plain"
        ref, mag = _reference(case, math, True, x, dy, dw0)
        rc, first, dbias = run(xd, dyd, 0xA5, None)
        assert rc == 0, rc
        held(tag, first, ref, mag)
        if taps == 9:  # dbias[b][m] (+)= sum of dy[m], an fp32 sum in every family
            dref = dy.double().sum(1).repeat(nb) + (0 if db0 is None else db0.double())
            derr = (dbias.double().to(dref.device) - dref).abs().max().item() / dref.abs().max().item()
            print("wgrad %s %s: dbias max rel %.3e" % (cw.case_id(key, cls, case), tag, derr))
            assert derr < BAR
            for b, d in zip(range(nb), (case.dil0, case.dil1)):  # taps wholly outside the image: exactly 0, or dw0
                t9 = torch.arange(9)
                out = ((d >= w) & (t9 % 3 != 1)) | ((d >= h) & (t9 // 3 != 1))
                got = first.view(nb, cout, cin, 9)[b][:, :, out.to(DEV)]
                want = dw0d.view(nb, cout, cin, 9)[b][:, :, out.to(DEV)] if acc else torch.zeros_like(got)
                assert torch.equal(got, want), "a tap outside the image is not exact"
        # bit-reproducible, whatever the workspace held (0xFF: NaNs - a piece or plane read before written shows)
        for ws_byte in (0xFF, 0x00):
            rc, again, dbias2 = run(xd, dyd, ws_byte, None)
            assert rc == 0 and torch.equal(again.view(torch.int32), first.view(torch.int32))
            assert taps == 1 or torch.equal(dbias2.view(torch.int32), dbias.view(torch.int32))
        if scales:
            rows = []
            for t, c in ((xd, cin), (dyd, cout)):
                part = torch.empty(c, device=DEV)
                assert lib.msl_absmax_partials(t.data_ptr(), c, p, part.data_ptr(), st) == 0
                rows.append((part, c))
            assert cw.plan_of(hip, case, cin, cout).rowscale == 1
            rc, again, _ = run(xd, dyd, 0xA5, rows)  # the caller's per-row partials: the scales the call reduces itself
            assert rc == 0 and torch.equal(again.view(torch.int32), first.view(torch.int32))
            if not spread and not over:  # one tensor-wide partial per operand: one scale per tensor
                assert cw.plan_of(hip, case, 1, 1).rowscale == 0
                one = [(t.abs().max().reshape(1).contiguous(), 1) for t in (xd, dyd)]
                rc, flat, _ = run(xd, dyd, 0xA5, one)
                assert rc == 0
                held("tensor-scale", flat, *_reference(case, math, False, x, dy, dw0))
        assert torch.equal(xd, x_bytes) and torch.equal(dyd, dy_bytes), "an operand was written"
        if not spread:  # a workspace one byte short: refused, nothing launched
            rc, untouched, _ = run(xd, dyd, 0xA5, None, ws_bytes=wsb - 1)
            assert rc == MSL_ERR_WORKSPACE
            assert torch.equal(untouched, dw0d) if acc else bool(torch.isnan(untouched).all())
