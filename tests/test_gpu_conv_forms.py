"""Every reachable forward-form conv kernel and schedule against fp64, straight through the C ABI (GPU only).

One test over tests/conv_form_cases.py: pack, workspace query, call.  The reference is an fp64 conv (or
matrix product) on the operands as the launched kernel's math sees them - which math that is comes from the
library's own plan (msl_conv_fwd_plan), not from the case - and the bar is the project's own:
max|out - ref| / max|ref| < 1e-5, in every family.  Each call must also write its whole output and nothing
else (NaN pre-fill, guard rows around the output, a guard tail behind the queried workspace), give the same
bytes three times over, and - where the kernel scales its image operand - the same bytes when handed the
operand's absmax partials.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import conv_form_cases as cf

pytestmark = pytest.mark.gpu

from maxsquareloss_amd import hip  # noqa: E402

DEV = "cuda"
GUARD_WORD = 0x5A5A5A5B  # a finite float no kernel computes
WS_GUARD = 4096


def _bf(t):
    """fp32 rounded to bf16 (RNE), exact in fp64."""
    return t.bfloat16().double()


def _f16(t):
    """Scaled by the tensor's power of two (absmax into [2^14, 2^15)), rounded to fp16, unscaled."""
    e = torch.frexp(t.abs().max()).exponent.item()
    sc = 2.0 ** (15 - e)
    return (t * sc).half().double() / sc


_ROUND = {"f32": lambda t: t.double(), "x6p": lambda t: t.double(), "h3p": lambda t: t.double(), "bf16": _bf,
          "h1p": _f16}


def _images(t, n, h, w):
    """[C][N][H][W] (the library's layout) -> (N, C, H, W)."""
    return t.reshape(-1, n, h, w).transpose(0, 1)


def _reference(case, math, img, wts, bias, dx0, res, bits):
    """The call in fp64 on the rounded operands; [rows][P]."""
    taps, dgrad, acc = cf.ENTRIES[case.entry]
    rnd = _ROUND[math]
    n, h, w = case.nimg, case.h, case.w
    ri = rnd(img)
    rw = rnd(wts)  # every branch of a pack shares one scale
    if taps == 1:
        wm = rw.reshape(case.cout, case.cin)
        out = (wm.t() if dgrad else wm) @ ri
    else:
        x = _images(ri, n, h, w)
        out = 0
        for b, d in zip(range(case.nbranch), (case.dil0, case.dil1)):
            wb = rw[b].transpose(0, 1).flip(2, 3) if dgrad else rw[b]
            out = out + F.conv2d(x, wb, padding=d, dilation=d)
        out = out.transpose(0, 1).reshape(out.size(1), -1)
        if bias is not None:
            out = out + bias.double().sum(0).view(-1, 1)
    if res is not None:
        hw = h * w
        words = bits.view(case.cin * n, (hw + 63) // 64)
        idx = torch.arange(hw)
        on = ((words[:, idx // 64] >> (idx % 64)) & 1).bool().reshape(case.cin, n * hw)
        out = out + torch.where(on, res.double(), torch.zeros((), dtype=torch.float64))
    elif acc:
        out = out + dx0.double()
    return out


def _fill(t, word):
    t.view(torch.int32).fill_(word if word < 2 ** 31 else word - 2 ** 32)


@pytest.mark.parametrize("key,cls,case", cf.TABLE, ids=["%s-%s-%s-%s-%s-%dx%d-%dx%dx%d" % (
    k, c, s.entry, s.family, s.f32_form, s.cin, s.cout, s.nimg, s.h, s.w) for k, c, s in cf.TABLE])
def test_conv_form_against_fp64(key, cls, case):
    lib = hip.load()
    pl = cf.plan_of(hip, case)
    assert pl.status == cf.MSL_OK
    assert ((cf.form_key(hip, pl.row) if pl.stream_k else "tile"), cf.schedule_class(pl)) == (key, cls)
    math = cf.MATHS[pl.math]
    taps, dgrad, acc = cf.ENTRIES[case.entry]
    n, h, w, cin, cout, nb = case.nimg, case.h, case.w, case.cin, case.cout, case.nbranch
    p = n * h * w
    cimg, m = (cout, cin) if dgrad else (cin, cout)
    resmask = case.entry == "pconv_dgrad_resmask"
    g = torch.Generator().manual_seed(cin * 131 + cout * 7 + p + taps + acc)
    img = torch.randn(cimg, p, generator=g)
    k = 3 if taps == 9 else 1
    wts = torch.randn(nb, cout, cin, k, k, generator=g) * 0.05
    bias = torch.randn(nb, cout, generator=g) if case.entry == "dconv_fwd" else None
    dx0 = torch.randn(m, p, generator=g) if acc and not resmask else None
    res = torch.randn(m, p, generator=g) if resmask else None
    hw = h * w
    bits = None
    if resmask:  # rows c * nimg + image of cdiv(h * w, 64) words: every bit random, the rows end inside a word
        assert hw % 64 != 0
        halves = torch.randint(0, 2 ** 32, (2, m * n * ((hw + 63) // 64)), generator=g, dtype=torch.int64)
        bits = (halves[0] << 32) | halves[1]
    ref = _reference(case, math, img, wts, bias, dx0, res, bits)

    fm = hip.Forms(cf.F32_FORMS[case.f32_form], case.sk_hybrid, 1, 1)
    fmp, st = ctypes.addressof(fm), hip.stream_ptr()
    wd = wts.to(DEV)
    if taps == 9:
        packed = torch.empty(lib.msl_dconv_packed_elems(nb, cin, cout, int(dgrad)), device=DEV)
        assert lib.msl_dconv_pack(wd.data_ptr(), cout * cin * 9, nb, cin, cout, int(dgrad), packed.data_ptr(), fmp,
                                  st) == 0
        query = lib.msl_dconv_dgrad_workspace if dgrad else lib.msl_dconv_fwd_workspace
        wsb = query(nb, cin, cout, h, w, n)
    else:
        packed = torch.empty(lib.msl_pconv_packed_elems(cin, cout, int(dgrad)), device=DEV)
        assert lib.msl_pconv_pack(wd.data_ptr(), cin, cout, int(dgrad), packed.data_ptr(), fmp, st) == 0
        query = lib.msl_pconv_dgrad_workspace if dgrad else lib.msl_pconv_fwd_workspace
        wsb = query(cin, cout, p)
    assert wsb > 0
    imgd = img.to(DEV)
    img_bytes = imgd.clone()
    biasd = None if bias is None else bias.to(DEV)
    resd = None if res is None else res.to(DEV)
    bitsd = None if bits is None else bits.to(DEV)
    guard = (2 * p + 63) // 64 * 64  # two rows before and behind the output, whole 256-byte lines
    buf = torch.empty(guard + m * p + guard, device=DEV)
    out = buf[guard:guard + m * p]
    ws = torch.empty(wsb + WS_GUARD, dtype=torch.uint8, device=DEV)
    scales = math in ("h3p", "h1p")
    part = None
    if scales:
        part = torch.empty(cimg, device=DEV)
        assert lib.msl_absmax_partials(imgd.data_ptr(), cimg, p, part.data_ptr(), st) == 0
    sfx = {"fp32": "_sc", "fp16": "_f16", "bf16": "_bf16"}[case.family]

    def call(ws_byte, with_part):
        _fill(buf, GUARD_WORD)
        if dx0 is not None:
            out.copy_(dx0.reshape(-1))
        else:
            out.fill_(float("nan"))
        ws.fill_(ws_byte)
        ws[wsb:].fill_(0xA5)
        tail = () if case.family == "bf16" else ((part.data_ptr(), cimg) if with_part else (None, 0))
        com = (fmp, ws.data_ptr(), wsb, st) + tail
        if case.entry == "dconv_fwd":
            rc = getattr(lib, "msl_dconv_fwd" + sfx)(imgd.data_ptr(), packed.data_ptr(), biasd.data_ptr(), out.data_ptr(),
                                                     nb, cin, cout, h, w, n, case.dil0, case.dil1, *com)
        elif case.entry == "dconv_dgrad":
            rc = getattr(lib, "msl_dconv_dgrad" + sfx)(imgd.data_ptr(), packed.data_ptr(), out.data_ptr(), nb, cin, cout,
                                                       h, w, n, case.dil0, case.dil1, *com)
        elif case.entry == "pconv_fwd":
            rc = getattr(lib, "msl_pconv_fwd" + sfx)(imgd.data_ptr(), packed.data_ptr(), out.data_ptr(), cin, cout, p,
                                                     *com)
        elif resmask:
            rc = getattr(lib, "msl_pconv_dgrad_resmask" + sfx)(imgd.data_ptr(), packed.data_ptr(), out.data_ptr(), cin,
                                                               cout, p, resd.data_ptr(), bitsd.data_ptr(), n, *com)
        elif case.family == "bf16":
            rc = lib.msl_pconv_dgrad_bf16(imgd.data_ptr(), packed.data_ptr(), out.data_ptr(), cin, cout, p, *com)
        else:
            name = "msl_pconv_dgrad_f16" if case.family == "fp16" else "msl_pconv_dgrad_acc_sc"
            rc = getattr(lib, name)(imgd.data_ptr(), packed.data_ptr(), out.data_ptr(), cin, cout, p, acc, *com)
        assert rc == 0, rc
        torch.cuda.synchronize()
        gw = buf.view(torch.int32)
        want = GUARD_WORD if GUARD_WORD < 2 ** 31 else GUARD_WORD - 2 ** 32
        assert bool((gw[:guard] == want).all()) and bool((gw[guard + m * p:] == want).all()), "wrote outside its output"
        assert bool((ws[wsb:] == 0xA5).all()), "wrote behind its queried workspace"
        return out.clone()

    first = call(0xA5, False)
    err = (first.double().cpu().view(m, p) - ref).abs().max().item() / ref.abs().max().item()
    print("%s %s %s: rel err %.3e" % (key, cls, tuple(case), err))
    assert err < 1e-5
    # bit-reproducible, whatever the workspace held (0xFF: NaNs)
    for ws_byte in (0xFF, 0x00):
        assert torch.equal(call(ws_byte, False).view(torch.int32), first.view(torch.int32))
    if scales:  # the caller's partials give the scale the call reduces itself
        assert torch.equal(call(0xA5, True).view(torch.int32), first.view(torch.int32))
    assert torch.equal(imgd, img_bytes)
