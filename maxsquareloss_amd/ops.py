"""torch.autograd wrappers over the HIP kernels of libmsl_hip.so.

Each Function is a thin shim: shape checks on the host, then one or two C-ABI
calls on torch's current HIP stream.  Tensors are bs=1 NCHW fp32 (the
reference only runs bs=1: IW_MaxSquareloss broadcasts (N,H,W) weights against
(N,C,H,W) probabilities, which only works for N=1 - SURVEY.md quirk Q3), or an
image PAIR (1, C, 2, H, W): the source and target images of one UDA iteration laid
out [C][2][H][W], each image convolved, pooled and batch-normalised on its own (its
own bs=1 statistics) while every conv GEMM runs once over both (pair_join /
pair_split; the trunk ops take either form, the losses one image).  The host sequences several
Functions share live once: next to _conv_call for the convs (_pconv_fwd, _pconv_dgrad, _wgrad_call,
_pconv_wgrad, _stack_bias / _branch_grads), in _LossUp and its _UP_LOSSES table for the fused losses.
"""
import ctypes
from contextlib import nullcontext as _nullctx

import torch
from torch.autograd import Function

from . import hip

_f32 = torch.float32

# Conv MFMA precision: "fp32" (fp32-accurate, in the library's fp32 form below), "fp16"
# (v_mfma_f32_32x32x16_f16 on operands scaled by a power of two and rounded to fp16, fp32 sums:
# BASELINE config 5's fp16 MFMA path; needs the f16x3 fp32 form's packs) or "bf16"
# (v_mfma_f32_32x32x16_bf16 on operands rounded to bf16, fp32 sums).  Activations, BN, losses
# and the optimizer stay fp32 in every case.
CONV_MATH = "fp32"


def set_conv_math(math):
    global CONV_MATH
    if math not in ("fp32", "fp16", "bf16"):
        raise ValueError(f"conv math must be 'fp32', 'fp16' or 'bf16', got {math!r}")
    CONV_MATH = math


# Matrix-core form of the fp32 conv math (hip.FORMS.f32_form, passed with every conv / pack call as
# msl_forms): "mfma_f32" = v_mfma_f32_32x32x2_f32, an exact fmaf chain; "bf16x6" =
# each operand split into three bf16 terms, six products per 16-deep K slice on
# v_mfma_f32_32x32x16_bf16 with fp32 sums (fp32-accurate; csrc/dconv_kernels.h Split3); "f16x3" =
# each operand tensor scaled by a power of two and split into two fp16 terms, three products per
# slice on v_mfma_f32_32x32x16_f16 with fp32 sums (fp32-accurate; dconv_kernels.h Split2h).
F32_FORMS = {"mfma_f32": 0, "bf16x6": 2, "f16x3": 5}


def _form_code():
    """The f32 form code the conv / pack calls pass (packs are form-specific: it keys the pack caches)."""
    return hip.FORMS.f32_form


def set_f32_form(form):
    """Select the fp32 conv form; returns the previous one."""
    if form not in F32_FORMS:
        raise ValueError(f"fp32 conv form must be one of {sorted(F32_FORMS)}, got {form!r}")
    prev = hip.set_form("f32_form", F32_FORMS[form])
    return {v: k for k, v in F32_FORMS.items()}[prev]


def set_bn_fused(fused):
    """Select the BN kernel form (msl_forms.bn_fused): True = one fused launch per train-mode BN
    call on maps of <= 16384 px (<= 33792 px with >= 128 channels); returns the previous setting."""
    return bool(hip.set_form("bn_fused", int(bool(fused))))


def f32_form():
    return {v: k for k, v in F32_FORMS.items()}[hip.FORMS.f32_form]


def _h3(math="fp32"):
    """Whether the conv GEMMs of this math scale their operands (and so read absmax partials)."""
    return math == "fp16" or (math == "fp32" and _form_code() == F32_FORMS["f16x3"])


def _tag_absmax(t, part):
    """Attach the per-channel absmax partials a BN kernel wrote for its output `t` (msl_bn_*_am)."""
    t._msl_absmax = (part, t._version)


def _parts(t, math="fp32", compute=True):
    """The per-channel absmax partials of an operand tensor for the f16x3 form, as (tensor, count =
    channels): the ones the BN kernel that produced `t` wrote (msl_bn_fwd_am / msl_bn_bwd_am, no
    pass of their own), else - when `compute` - msl_absmax_partials, so that a tensor two GEMMs read
    (x: forward and weight gradient; dy: data and weight gradient) is reduced once.  None in the other
    forms (the kernels ignore them), or when not worth a launch (the entry point then reduces the
    operand itself if its kernel needs it)."""
    if not _h3(math):
        return None
    rec = getattr(t, "_msl_absmax", None)
    if rec is not None and rec[1] == t._version:
        return rec[0], rec[0].numel()
    if not compute:
        return None
    lib = hip.load()
    rows = t.size(1)
    part = torch.empty(rows, dtype=_f32, device=t.device)
    hip.check(lib.msl_absmax_partials(t.data_ptr(), rows, t.numel() // rows, part.data_ptr(), hip.stream_ptr()),
              "msl_absmax_partials")
    return part, rows


def _pp(q):
    """(pointer, count) of _parts' result for the _sc entry points."""
    return (None, 0) if q is None else (q[0].data_ptr(), q[1])


def _conv_call(lib, name, math, args, parts):
    """fp32: the _sc entry point, given the operands' absmax partials (None = the call reduces them
    itself; ignored outside f16x3); bf16: the _bf16 entry point."""
    if math == "bf16":
        return getattr(lib, name + "_bf16")(*args)
    suffix = "_f16" if math == "fp16" else "_sc"
    return getattr(lib, name + suffix)(*args, *(v for q in parts for v in _pp(q)))


def _split_gemm(m, k_other):
    """Whether a forward-form GEMM with M output rows runs a split (f16x3) kernel that scales its
    image operand (128-row tiles: M > 64), or a weight gradient of these channel counts the pre-split
    kernel (both >= 128): a partials launch only pays off where one of them reads the tensor."""
    return m > 64 or min(m, k_other) >= 128


def _pconv_fwd(lib, math, x, packed, y, cin, cout, p, scale_from=None):
    """y = W x on the pointwise forward GEMM of this math.  Returns x's absmax partials (_parts), which
    the weight gradient reads again; `scale_from`: a tensor with x's absmax whose partials serve instead."""
    wsb = lib.msl_pconv_fwd_workspace(cin, cout, p)
    ws = hip.workspace(wsb, x.device)
    if scale_from is not None:
        xpart = _parts(scale_from, math)
    else:
        xpart = _parts(x, math, compute=_split_gemm(cout, cin))
    hip.check(_conv_call(lib, "msl_pconv_fwd", math,
                         (x.data_ptr(), packed.data_ptr(), y.data_ptr(), cin, cout, p,
                          hip.forms(), ws.data_ptr(), wsb, hip.stream_ptr()), (xpart,)), "msl_pconv_fwd")
    return xpart


def _pconv_dgrad(lib, math, gy, packed_d, dx, cin, cout, p, acc, fm, ws, wsb, gpart):
    """dx = W^T dy, or dx += W^T dy with `acc`, on the pointwise data-gradient GEMM of this math and of
    the forward's forms `fm`, in the caller's workspace (msl_pconv_dgrad_workspace).  The bf16 entry
    point has no accumulate epilogue: it ignores `acc`."""
    head = (gy.data_ptr(), packed_d.data_ptr(), dx.data_ptr(), cin, cout, p)
    tail = (ctypes.addressof(fm), ws.data_ptr(), wsb, hip.stream_ptr())
    if math == "bf16":
        st = lib.msl_pconv_dgrad_bf16(*head, *tail)
    else:
        fn = lib.msl_pconv_dgrad_f16 if math == "fp16" else lib.msl_pconv_dgrad_acc_sc
        st = fn(*head, acc, *tail, *_pp(gpart))
    hip.check(st, "msl_pconv_dgrad")


def _wgrad_call(lib, name, math, args, wsb, fm, operands, parts, sink=None):
    """The weight-gradient GEMM `name`(*args, fm, workspace, stream).  With a `sink` (grad_sink: the
    GEMM accumulates into the flat gradient buffer) it runs on the side stream under ASYNC_WGRAD, its
    workspace allocated there and its operands kept for that stream, and the flat buffer is notified."""
    dev = operands[0].device
    side = _wgrad_stream(operands[0]) if (ASYNC_WGRAD and sink is not None) else None
    with torch.cuda.stream(side) if side is not None else _nullctx():
        ws = hip.workspace(wsb, dev)
        hip.check(_conv_call(lib, name, math,
                             (*args, ctypes.addressof(fm), ws.data_ptr(), wsb, hip.stream_ptr()), parts), name)
    if side is not None:
        _keep(side, *operands, *(q[0] for q in parts if q is not None))
    if sink is not None:
        sink[1].notify(sink[2])


def _pconv_wgrad(lib, math, x, gy, xpart, gpart, cin, cout, p, weight, fm):
    """dW = dy x^T on the pointwise weight-gradient GEMM: accumulated into `weight`'s slice of the flat
    gradient buffer when it has a sink (returns None: autograd gets no gradient), else a new tensor."""
    sink = grad_sink(weight)
    dst = sink[0] if sink is not None else torch.empty_like(weight)
    _wgrad_call(lib, "msl_pconv_wgrad", math,
                (x.data_ptr(), gy.data_ptr(), dst.data_ptr(), cin, cout, p, int(sink is not None)),
                lib.msl_pconv_wgrad_workspace(cin, cout, p), fm, (x, gy), (xpart, gpart), sink)
    return None if sink is not None else dst


def _stack_bias(b0, b1, nb):
    """The biases of a one- or two-branch conv as one [nb][cout] tensor; None without biases."""
    if b0 is None:
        return None
    return torch.stack([b0] if nb == 1 else [b0, b1]).contiguous()


def _branch_grads(dw_all, db_all, nb):
    """(dw0, dw1, db0, db1) for autograd from the stacked [nb][...] gradients (None: not computed)."""
    def pair(t):
        return (None, None) if t is None else (t[0], t[1] if nb > 1 else None)
    return pair(dw_all) + pair(db_all)


def _check_act(x, name, images=False):
    """x contiguous; with `images`, (1,C,H,W) or an image batch (1,C,N,H,W) ([C][N][H][W])."""
    ok = x.is_cuda and x.dtype == _f32 and x.size(0) == 1 and (x.dim() == 4 or (images and x.dim() == 5))
    if not ok:
        shapes = "(1,C,H,W) or (1,C,N,H,W)" if images else "(1,C,H,W)"
        raise hip.MSLError(f"{name}: expected a CUDA fp32 tensor of shape {shapes}, got "
                           f"{tuple(x.shape)} {x.dtype} {x.device}")
    return x.contiguous()


def _nimg(x):
    """Images in an activation: 1 for (1,C,H,W), N for (1,C,N,H,W)."""
    return x.size(2) if x.dim() == 5 else 1


def _like(x, c, h, w, dtype=_f32):
    """An empty activation with x's image count and c channels of h x w."""
    shape = (1, c, x.size(2), h, w) if x.dim() == 5 else (1, c, h, w)
    return torch.empty(shape, dtype=dtype, device=x.device)


# --------------------------------------------------------------------------- gradient sinks
def grad_sink(p):
    """(grad view, FlatGrads, index) when `p`'s .grad is its slice of the optimizer's flat buffer.

    The backward of a HIP op then accumulates the weight gradient straight into that slice (the
    wgrad / BN kernels have an accumulate mode), notifies the flat buffer as AccumulateGrad's
    hook would (the data-parallel reducer listens there), and returns None for the parameter -
    saving autograd's separate `grad += new` kernel per parameter per backward.  Only for
    .backward()-driven training: torch.autograd.grad() on such a parameter would see None.
    """
    s = getattr(p, "_msl_flat", None)
    if s is None or p.grad is None or torch.is_grad_enabled():
        return None
    fg, i = s
    g = p.grad
    if g.data_ptr() != fg.flat.data_ptr() + 4 * int(fg.offsets[i]):
        return None
    return g, fg, i


# --------------------------------------------------------------------------- asynchronous weight gradients
# With ASYNC_WGRAD the weight gradients that accumulate in place into the flat gradient buffer (the
# training path: ops.grad_sink) run on a side stream per device, concurrently with the data-gradient
# chain of the backward (dgrad -> BN backward -> dgrad ...), which is latency-bound between its GEMMs.
# Everything that reads the flat buffer joins that stream first (wgrad_join: the SGD step, the data-
# parallel bucket launches, zero_grad).  Kernels, operands and per-buffer order are unchanged
# (results bit-identical).  Not in the reference, whose backward is one stream.  Off by default: the
# step measured slower with it (40.2 vs 39.5 ms same box: the concurrent GEMMs share the CUs and the
# caches; profiles/r03_async_wgrad_ab.txt).
ASYNC_WGRAD = False
_WG_STREAMS = {}


def _wgrad_stream(t):
    idx = t.device.index if t.device.index is not None else torch.cuda.current_device()
    ws = _WG_STREAMS.get(idx)
    if ws is None:
        ws = _WG_STREAMS[idx] = torch.cuda.Stream(device=t.device)
    ws.wait_stream(torch.cuda.current_stream(t.device))
    return ws


def _keep(ws, *tensors):
    """The side stream reads these: the caching allocator must not hand their memory to another
    stream's allocations before the side stream's work on them is done."""
    for t in tensors:
        if t is not None:
            t.record_stream(ws)


def wgrad_join(device=None):
    """Make the current stream wait for every weight gradient enqueued on the side stream."""
    if not _WG_STREAMS:
        return
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    ws = _WG_STREAMS.get(dev.index if dev.index is not None else torch.cuda.current_device())
    if ws is not None:
        torch.cuda.current_stream(dev).wait_stream(ws)


# --------------------------------------------------------------------------- packing cache
class PackCache:
    """Packed copies of a conv's weights, rebuilt when any weight changes.

    The forward GEMM wants W as [k = (tap, 16-channel block)][cout] and the
    data gradient wants the transposed, tap-flipped layout; both are derived
    from the parameters once per optimizer step (keyed on the tensors'
    in-place version counters), not once per call.
    """

    def __init__(self, pointwise=False):
        self.pointwise = pointwise
        self.key = {0: None, 1: None}
        self.buf = {0: None, 1: None}
        self.used = {0: False, 1: False}  # read by PackBatch: the directions a step consumes
        self.meta = {0: None, 1: None}    # (weights, cin, cout) of the last get()
        self._shift = None                # the ASPP shift form's packs (ops.aspp2)

    def shift_pack(self):
        if self._shift is None:
            self._shift = _ShiftPack()
        return self._shift

    @staticmethod
    def key_of(weights):
        return (_form_code(),) + tuple((w.data_ptr(), w._version) for w in weights)

    def get(self, weights, cin, cout, for_dgrad):
        key = self.key_of(weights)
        self.used[for_dgrad] = True
        self.meta[for_dgrad] = (list(weights), cin, cout)
        if self.key[for_dgrad] != key:
            lib = hip.load()
            nb = len(weights)
            if self.pointwise:
                total = lib.msl_pconv_packed_elems(cin, cout, for_dgrad)
            else:
                total = lib.msl_dconv_packed_elems(nb, cin, cout, for_dgrad)
            buf = self.buf[for_dgrad]
            if buf is None or buf.numel() != total or buf.device != weights[0].device:
                buf = torch.empty(total, dtype=_f32, device=weights[0].device)
            s = hip.stream_ptr()
            wc = [w.detach().contiguous() for w in weights]
            if self.pointwise:
                hip.check(lib.msl_pconv_pack(wc[0].data_ptr(), cin, cout, for_dgrad, buf.data_ptr(), hip.forms(), s),
                          "msl_pconv_pack")
            else:
                # one call packs every branch (and splits the bf16x6 planes behind them)
                stride = (wc[1].data_ptr() - wc[0].data_ptr()) // 4 if nb == 2 else 0
                if nb == 2 and (wc[1].data_ptr() - wc[0].data_ptr()) % 4:
                    raise hip.MSLError("dconv pack: misaligned branch weights")
                hip.check(lib.msl_dconv_pack(wc[0].data_ptr(), stride, nb, cin, cout, for_dgrad, buf.data_ptr(),
                                             hip.forms(), s),
                          "msl_dconv_pack")
            self.buf[for_dgrad] = buf
            self.key[for_dgrad] = key
        return self.buf[for_dgrad]


class PackBatch:
    """Every weight pack of a model in two launches (one per tap count) instead of one per conv
    and direction (~130 per training step): `run()` after the optimizer step packs each stale
    (PackCache, direction) that an earlier step consumed through msl_conv_pack_many
    (byte-identical to the per-conv calls) and marks it fresh.  The set of stale packs is the
    same every step (the parameters the loss reaches: with --multi False the layer3 ASPP head
    gets no gradient and keeps its packs), so the job tables are built once, outside graph
    capture (utils/graph.py captures iteration 1, after iteration 0 built them eagerly); a new
    set while capturing is left to PackCache.get's lazy path."""

    _JOB = None

    def __init__(self, module):
        self.caches = [m._pack for m in module.modules() if isinstance(getattr(m, "_pack", None), PackCache)]
        self.sig = None
        self.tables = {}
        self.launches = 0

    @classmethod
    def _dtype(cls):
        import numpy as np
        if cls._JOB is None:
            cls._JOB = np.dtype([("w", "<u8"), ("bs", "<i8"), ("packed", "<u8"), ("nb", "<i4"), ("cin", "<i4"),
                                 ("cout", "<i4"), ("fd", "<i4")])
            assert cls._JOB.itemsize == 40  # sizeof(msl_pack_job)
        return cls._JOB

    def _jobs(self):
        out = []
        for c in self.caches + [c._shift.pc for c in self.caches if c._shift is not None]:
            for d in (0, 1):
                if c.used[d] and c.buf[d] is not None and c.meta[d] is not None:
                    out.append((c, d))
        return out

    def _build(self, jobs, device):
        import numpy as np
        lib = hip.load()
        tables = {}
        for taps in (9, 1):
            sel = [(c, d) for c, d in jobs if (1 if c.pointwise else 9) == taps]
            if not sel:
                continue
            rec = np.zeros(len(sel), dtype=self._dtype())
            starts = np.zeros(len(sel) + 1, dtype=np.int64)
            for i, (c, d) in enumerate(sel):
                ws, cin, cout = c.meta[d]
                nb = len(ws)
                stride = 0
                if nb == 2:
                    diff = ws[1].data_ptr() - ws[0].data_ptr()
                    if diff % 4:
                        return None
                    stride = diff // 4
                if any(not w.is_contiguous() for w in ws):
                    return None
                rec[i] = (ws[0].data_ptr(), stride, c.buf[d].data_ptr(), nb, cin, cout, d)
                nblk = lib.msl_conv_pack_blocks(nb, taps, cin, cout, d)
                if nblk < 1:
                    return None
                starts[i + 1] = starts[i] + nblk
            jt = torch.from_numpy(rec.view(np.uint8).copy()).to(device)
            st = torch.from_numpy(starts).to(device)
            tables[taps] = (jt, st, len(sel), int(starts[-1]))
        return tables

    def run(self):
        for c in self.caches:  # the ASPP heads' shift-form layouts first (ops._ShiftPack): their packs follow
            if c._shift is not None and c._shift.meta is not None:
                c._shift.refresh()
        jobs, keys = [], []
        for c, d in self._jobs():
            k = c.key_of(c.meta[d][0])
            if c.key[d] != k:
                jobs.append((c, d))
                keys.append(k)
        if not jobs:
            return False
        sig = tuple((id(c), d, c.buf[d].data_ptr(), c.buf[d].numel(), tuple(w.data_ptr() for w in c.meta[d][0]),
                     c.meta[d][1], c.meta[d][2]) for c, d in jobs)
        if sig != self.sig:
            if torch.cuda.is_current_stream_capturing():
                return False
            tables = self._build(jobs, jobs[0][0].buf[jobs[0][1]].device)
            if tables is None:
                return False
            self.tables, self.sig = tables, sig
        lib = hip.load()
        s = hip.stream_ptr()
        for taps, (jt, st, n, total) in self.tables.items():
            hip.check(lib.msl_conv_pack_many(jt.data_ptr(), st.data_ptr(), n, taps, total, hip.forms(), s),
                      "msl_conv_pack_many")
        for (c, d), k in zip(jobs, keys):
            c.key[d] = k
        self.launches += 1
        return True


# --------------------------------------------------------------------------- dilated conv
# Live kernel timing for bench.py: PROBE[(nbranch, cin, cout, h, w, dil0)] = [] collects
# (start, end) HIP events recorded on the launching stream around each matching forward.
PROBE = {}


class _DConv3x3(Function):
    """sum_b conv3x3(x, W_b, dilation d_b) (+ sum_b bias_b); nbranch in {1, 2}."""

    @staticmethod
    def forward(ctx, x, w0, w1, b0, b1, dil0, dil1, cache):
        ctx.fm = hip.snapshot_forms()  # the backward runs the forms of its forward
        x = _check_act(x, "dconv3x3", images=True)
        n = _nimg(x)
        weights = [w0] if w1 is None else [w0, w1]
        nb = len(weights)
        cout, cin = w0.shape[0], w0.shape[1]
        if w0.shape[2:] != (3, 3) or x.size(1) != cin:
            raise hip.MSLError(f"dconv3x3: weight {tuple(w0.shape)} does not match input {tuple(x.shape)}")
        h, w = x.shape[-2], x.shape[-1]
        lib = hip.load()
        packed = cache.get(weights, cin, cout, 0)
        bias = _stack_bias(b0, b1, nb)
        y = _like(x, cout, h, w)
        wsb = lib.msl_dconv_fwd_workspace(nb, cin, cout, h, w, n)
        ws = hip.workspace(wsb, x.device)
        probe = PROBE.get((nb, cin, cout, h, w, dil0, n)) if PROBE else None
        if probe is not None:
            ev0 = torch.cuda.Event(enable_timing=True)
            ev0.record()
        math = CONV_MATH
        xpart = _parts(x, math, compute=_split_gemm(cout, cin))
        hip.check(_conv_call(lib, "msl_dconv_fwd", math,
                             (x.data_ptr(), packed.data_ptr(), hip.ptr(bias), y.data_ptr(), nb, cin, cout, h, w, n,
                              dil0, dil1 if nb > 1 else 0, hip.forms(), ws.data_ptr(), wsb,
                              hip.stream_ptr()), (xpart,)), "msl_dconv_fwd")
        if probe is not None:
            ev1 = torch.cuda.Event(enable_timing=True)
            ev1.record()
            probe.append((ev0, ev1))
        ctx.save_for_backward(x, *weights)
        ctx.meta = (nb, cin, cout, h, w, n, dil0, dil1, b0 is not None, cache, math)
        ctx.xpart = xpart
        return y

    @staticmethod
    def backward(ctx, gy):
        x, *weights = ctx.saved_tensors
        nb, cin, cout, h, w, n, dil0, dil1, has_bias, cache, math = ctx.meta
        gy = gy.contiguous()
        lib = hip.load()
        s = hip.stream_ptr()
        d1 = dil1 if nb > 1 else 0
        dx = None
        gpart = _parts(gy, math, compute=_split_gemm(cin, cout))
        xpart = ctx.xpart
        if ctx.needs_input_grad[0]:
            packed_d = cache.get(weights, cin, cout, 1)
            dx = torch.empty_like(x)
            wsb = lib.msl_dconv_dgrad_workspace(nb, cin, cout, h, w, n)
            ws = hip.workspace(wsb, x.device)
            hip.check(_conv_call(lib, "msl_dconv_dgrad", math,
                                 (gy.data_ptr(), packed_d.data_ptr(), dx.data_ptr(), nb, cin, cout, h, w, n, dil0, d1,
                                  ctypes.addressof(ctx.fm), ws.data_ptr(), wsb, s), (gpart,)),
                      "msl_dconv_dgrad")
        sink = grad_sink(weights[0]) if (nb == 1 and not has_bias and ctx.needs_input_grad[1]) else None
        wsb = lib.msl_dconv_wgrad_workspace(nb, cin, cout, h, w, n)
        if sink is not None:
            _wgrad_call(lib, "msl_dconv_wgrad", math,
                        (x.data_ptr(), gy.data_ptr(), sink[0].data_ptr(), None, 1, cin, cout, h, w, n, dil0, 0, 1),
                        wsb, ctx.fm, (x, gy), (xpart, gpart), sink)
            return dx, None, None, None, None, None, None, None
        # without a sink the workspace comes before the gradient tensors: not _wgrad_call's order
        ws = hip.workspace(wsb, x.device)
        dw_all = torch.empty((nb, cout, cin, 3, 3), dtype=_f32, device=x.device)
        db_all = torch.empty((nb, cout), dtype=_f32, device=x.device) if has_bias else None
        hip.check(_conv_call(lib, "msl_dconv_wgrad", math,
                             (x.data_ptr(), gy.data_ptr(), dw_all.data_ptr(), hip.ptr(db_all), nb, cin, cout, h, w,
                              n, dil0, d1, 0, ctypes.addressof(ctx.fm), ws.data_ptr(), wsb, s), (xpart, gpart)),
                  "msl_dconv_wgrad")
        return (dx, *_branch_grads(dw_all, db_all, nb), None, None, None)


def dconv3x3(x, weight, dilation, cache):
    """Stride-1, padding=dilation, bias-free 3x3 conv (Bottleneck.conv2, deeplab_multi.py:17-18)."""
    return _DConv3x3.apply(x, weight, None, None, None, int(dilation), 0, cache)


# --------------------------------------------------------------------------- ASPP heads: shift form
# ASPP_FORM = "shift" (default, r04): the head as one pointwise GEMM with 18*C rows and per-tap shifts
# (csrc/aspp.hip; x read once instead of once per tap), "direct": the two-branch implicit GEMM above.
ASPP_FORM = "shift"


class _ShiftPack:
    """W'[t*C + m][cin] = W_b[m][cin][k] (t = b*9 + k: the head's weights as one pointwise weight) and its
    pointwise packs, rebuilt when a branch weight changes (key: the weights' version counters)."""

    def __init__(self):
        self.key = None
        self.wp = None
        self.pc = PackCache(pointwise=True)
        self.meta = None  # (weights, cin, c) of the last get(): PackBatch refreshes the layout from them

    def get(self, weights, cin, c, for_dgrad):
        self.meta = (list(weights), cin, c)
        self.refresh()
        return self.pc.get([self.wp], cin, 9 * len(weights) * c, for_dgrad)

    def refresh(self):
        """Rebuild W' if a branch weight changed since (its version bump then makes the packs behind it
        stale: PackBatch.run packs them with the step's other packs)."""
        weights, cin, c = self.meta
        key = tuple((w.data_ptr(), w._version) for w in weights)
        nb = len(weights)
        if self.key != key:
            lib = hip.load()
            if self.wp is None or self.wp.shape != (9 * nb * c, cin) or self.wp.device != weights[0].device:
                self.wp = torch.empty((9 * nb * c, cin), dtype=_f32, device=weights[0].device)
            wc = [w.detach().contiguous() for w in weights]
            stride = (wc[1].data_ptr() - wc[0].data_ptr()) // 4 if nb == 2 else 0
            if nb == 2 and (wc[1].data_ptr() - wc[0].data_ptr()) % 4:
                raise hip.MSLError("aspp2: misaligned branch weights")
            hip.check(lib.msl_aspp_weight_layout(wc[0].data_ptr(), stride, nb, c, cin, self.wp.data_ptr(),
                                                 hip.stream_ptr()), "msl_aspp_weight_layout")
            torch.autograd.graph.increment_version(self.wp)  # the packs behind it key on it
            self.key = key


class _ASPPShift(Function):
    """sum_b conv3x3(x, W_b, d_b) + sum_b bias_b as Z = W' x (one pointwise GEMM, M = 18*C) and a
    masked shift-add of Z's rows (msl_aspp_shift_add); backward: G = the shifted, masked copies of dY
    (msl_aspp_shift_gather), dx = W'^T G, dW' = G x^T (the pointwise data / weight gradients)."""

    @staticmethod
    def forward(ctx, x, w0, w1, b0, b1, dil0, dil1, cache):
        ctx.fm = hip.snapshot_forms()  # the backward runs the forms of its forward
        x = _check_act(x, "aspp2", images=True)
        n = _nimg(x)
        weights = [w0] if w1 is None else [w0, w1]
        nb = len(weights)
        c, cin = w0.shape[0], w0.shape[1]
        if w0.shape[2:] != (3, 3) or x.size(1) != cin:
            raise hip.MSLError(f"aspp2: weight {tuple(w0.shape)} does not match input {tuple(x.shape)}")
        h, w = x.shape[-2], x.shape[-1]
        m, p = 9 * nb * c, h * w * n
        lib = hip.load()
        sp = cache.shift_pack()
        packed = sp.get(weights, cin, c, 0)
        z = torch.empty((1, m, p), dtype=_f32, device=x.device)
        math = CONV_MATH
        xpart = _pconv_fwd(lib, math, x, packed, z, cin, m, p)
        bias = _stack_bias(b0, b1, nb)
        y = _like(x, c, h, w)
        hip.check(lib.msl_aspp_shift_add(z.data_ptr(), hip.ptr(bias), y.data_ptr(), nb, c, h, w, n, dil0,
                                         dil1 if nb > 1 else 0, hip.stream_ptr()), "msl_aspp_shift_add")
        ctx.save_for_backward(x, *weights)
        ctx.meta = (nb, cin, c, h, w, n, dil0, dil1, b0 is not None, cache, math)
        ctx.xpart = xpart
        return y

    @staticmethod
    def backward(ctx, gy):
        x, *weights = ctx.saved_tensors
        nb, cin, c, h, w, n, dil0, dil1, has_bias, cache, math = ctx.meta
        gy = gy.contiguous()
        lib = hip.load()
        s = hip.stream_ptr()
        m, p = 9 * nb * c, h * w * n
        g = torch.empty((1, m, p), dtype=_f32, device=x.device)
        db_all = torch.empty((nb, c), dtype=_f32, device=x.device) if has_bias else None
        hip.check(lib.msl_aspp_shift_gather(gy.data_ptr(), g.data_ptr(), hip.ptr(db_all), nb, c, h, w, n, dil0,
                                            dil1 if nb > 1 else 0, s), "msl_aspp_shift_gather")
        gpart = _parts(g, math, compute=True)
        sp = cache.shift_pack()
        dx = None
        if ctx.needs_input_grad[0]:
            packed_d = sp.get(weights, cin, c, 1)
            dx = torch.empty_like(x)
            wsb = lib.msl_pconv_dgrad_workspace(cin, m, p)
            ws = hip.workspace(wsb, x.device)
            _pconv_dgrad(lib, math, g, packed_d, dx, cin, m, p, 0, ctx.fm, ws, wsb, gpart)
        dw_all = None
        if any(ctx.needs_input_grad[1:3]):
            dwp = torch.empty((m, cin), dtype=_f32, device=x.device)  # dW', never a parameter's: no sink
            _wgrad_call(lib, "msl_pconv_wgrad", math, (x.data_ptr(), g.data_ptr(), dwp.data_ptr(), cin, m, p, 0),
                        lib.msl_pconv_wgrad_workspace(cin, m, p), ctx.fm, (x, g), (ctx.xpart, gpart))
            dw_all = torch.empty((nb, c, cin, 3, 3), dtype=_f32, device=x.device)
            hip.check(lib.msl_aspp_weight_grad(dwp.data_ptr(), nb, c, cin, dw_all.data_ptr(), s),
                      "msl_aspp_weight_grad")
        return (dx, *_branch_grads(dw_all, db_all, nb), None, None, None)


def aspp2(x, w0, b0, w1, b1, dil0, dil1, cache):
    """conv_d6(x) + conv_d12(x) with biases: the live part of Classifier_Module (deeplab_multi.py:62-66)."""
    if ASPP_FORM == "shift":
        return _ASPPShift.apply(x, w0, w1, b0, b1, int(dil0), int(dil1), cache)
    return _DConv3x3.apply(x, w0, w1, b0, b1, int(dil0), int(dil1), cache)


# --------------------------------------------------------------------------- pointwise conv
class _PConv(Function):
    """y = W x for a 1x1, stride-1, bias-free conv (W: [cout][cin][1][1]) on the HIP pointwise GEMMs:
      y  = W x        msl_pconv_fwd (the conv math's form)
      dx = W^T dy     msl_pconv_dgrad; with a ResidualGrad `hold`, dx = (the identity residual's
                      gradient) + W^T dy, summed by the GEMM's accumulate epilogue (fp32 / fp16)
      dW += dy x^T    msl_pconv_wgrad, straight into the flat gradient buffer when the parameter
                      has a sink
    No library GEMM: every call is deterministic (fixed summation order)."""

    @staticmethod
    def forward(ctx, x, weight, cache, hold=None, grad_to=None):
        ctx.fm = hip.snapshot_forms()  # the backward runs the forms of its forward
        x = _check_act(x, "pconv", images=True)
        cout, cin = weight.shape[0], weight.shape[1]
        if weight.shape[2:] != (1, 1) or x.size(1) != cin:
            raise hip.MSLError(f"pconv: weight {tuple(weight.shape)} does not match input {tuple(x.shape)}")
        h, w = x.shape[-2], x.shape[-1]
        p = h * w * _nimg(x)  # every image: the pixel axis of a pointwise GEMM
        lib = hip.load()
        packed = cache.get([weight], cin, cout, 0)
        y = _like(x, cout, h, w)
        math = CONV_MATH
        # f16x3: x's absmax partials once for the forward and the weight gradient
        xpart = _pconv_fwd(lib, math, x, packed, y, cin, cout, p)
        ctx.save_for_backward(x, weight)
        ctx.meta = (cin, cout, p, cache, math)
        ctx.xpart = xpart
        ctx.hold = hold
        ctx.grad_to = grad_to
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        cin, cout, p, cache, math = ctx.meta
        gy = gy.contiguous()
        lib = hip.load()
        s = hip.stream_ptr()
        dx = None
        hold = ctx.hold
        # f16x3: dy's absmax partials once for the data and weight gradients
        gpart = _parts(gy, math, compute=_split_gemm(cin, cout))
        if ctx.needs_input_grad[0]:
            acc = 0
            if hold is not None:
                hold.consumed = True
            res = None
            if hold is not None and hold.g is not None:
                if isinstance(hold.g, MaskedResidual):
                    res, hold.g = hold.g, None
                    if math == "bf16":  # the bf16 form has no epilogue of either kind
                        dx, res, acc = res.materialize(), None, 1
                    else:
                        dx = torch.empty_like(x)
                else:
                    dx, hold.g = hold.g, None
                    acc = 1
            else:
                dx = torch.empty_like(x)
            packed_d = cache.get([weight], cin, cout, 1)
            wsb = lib.msl_pconv_dgrad_workspace(cin, cout, p)
            ws = hip.workspace(wsb, x.device)
            if res is not None:  # r06: dx = mask(dy of bn3) + W^T dy, the mask applied in the epilogue
                fn = lib.msl_pconv_dgrad_resmask_f16 if math == "fp16" else lib.msl_pconv_dgrad_resmask_sc
                hip.check(fn(gy.data_ptr(), packed_d.data_ptr(), dx.data_ptr(), cin, cout, p, res.dy.data_ptr(),
                             res.bits.data_ptr(), res.nimg, ctypes.addressof(ctx.fm), ws.data_ptr(), wsb, s,
                             *_pp(gpart)), "msl_pconv_dgrad_resmask")
            elif math == "bf16" and acc:  # the bf16 form has no accumulate epilogue
                tgt = torch.empty_like(x)
                _pconv_dgrad(lib, math, gy, packed_d, tgt, cin, cout, p, 0, ctx.fm, ws, wsb, gpart)
                dx.add_(tgt)
            else:
                _pconv_dgrad(lib, math, gy, packed_d, dx, cin, cout, p, acc, ctx.fm, ws, wsb, gpart)
        # a downsample conv (r05): its data gradient goes to the ResidualGrad that the block's conv1 sums
        # into its own (msl_pconv_dgrad_acc) - unless conv1's backward already ran, then autograd adds it
        to = ctx.grad_to
        if dx is not None and to is not None and not to.consumed:
            to.g, dx = dx, None
        if not ctx.needs_input_grad[1]:
            return dx, None, None, None, None
        dw = _pconv_wgrad(lib, math, x, gy, ctx.xpart, gpart, cin, cout, p, weight, ctx.fm)
        return dx, dw, None, None, None


def pconv(x, weight, cache, residual_grad=None, grad_to=None):
    """1x1, stride-1, bias-free conv (Bottleneck.conv1/conv3, downsample: deeplab_multi.py:13,20,96-99).
    `residual_grad` (a ResidualGrad also given to the block's bn_act or downsample conv): its gradient
    is added into this conv's input gradient by the data-gradient GEMM.  `grad_to` (the downsample
    conv of a block, r05): this conv's input gradient is handed to that ResidualGrad instead of to
    autograd, so the block's conv1 sums it (no separate accumulation kernel)."""
    return _PConv.apply(x, weight, cache, residual_grad, grad_to)


conv1x1 = pconv


# --------------------------------------------------------------------------- fused residual gradient
class ResidualGrad:
    """Carries the gradient of a bottleneck's identity residual from bn3's backward (which runs
    first) to conv1's backward, which adds it into the block input's gradient inside its data-
    gradient GEMM (msl_pconv_dgrad_acc) instead of autograd's separate accumulation kernel
    (deeplab_multi.py:31-48: x feeds conv1 and the residual)."""

    __slots__ = ("g", "consumed")

    def __init__(self):
        self.g = None
        self.consumed = False  # the summing conv's backward ran (a later producer hands to autograd)


class MaskedResidual:
    """r06: the identity residual's gradient left unmaterialised - relu'(y) * dy of the block's bn3, as
    bn3's output gradient `dy` and its forward's ReLU mask bits (msl_bn_fwd_mask).  conv1's data-gradient
    GEMM applies the mask in its epilogue (msl_pconv_dgrad_resmask), so bn3's backward skips writing the
    masked copy (one activation-sized write and read per identity block)."""

    __slots__ = ("dy", "bits", "nimg")

    def __init__(self, dy, bits, nimg):
        self.dy, self.bits, self.nimg = dy, bits, nimg

    def materialize(self):
        """The masked gradient as a tensor (the bf16 data-gradient form, which has no epilogue for it)."""
        c, hw = self.dy.size(1), self.dy.size(-2) * self.dy.size(-1)
        words = self.bits.view(c * self.nimg, (hw + 63) // 64)  # [channel][image][word] (msl_bn_relu_mask_bytes)
        idx = torch.arange(hw, device=self.dy.device)
        on = ((words[:, idx // 64] >> (idx % 64)) & 1).bool()  # [channel * image][pixel]
        g = self.dy.reshape(c * self.nimg, hw)  # (1,C[,N],H,W): channel-major, images inside
        return torch.where(on, g, torch.zeros((), dtype=g.dtype, device=g.device)).reshape(self.dy.shape)


# --------------------------------------------------------------------------- stem, maxpool, stride-2 glue
def pool_out(n, k, s, p, ceil):
    """torch's pooling_output_shape (dilation 1)."""
    num = n + 2 * p - (k - 1) - 1 + ((s - 1) if ceil else 0)
    o = num // s + 1
    if ceil and (o - 1) * s >= n + p:
        o -= 1
    return o


class _StemConv(Function):
    """conv2d(x, W, stride, padding) for a bias-free k x k conv as im2col + the pointwise GEMM
    (csrc/stem.hip): the [cout][cin][k][k] weight is a [cout][cin*k*k] pointwise weight as laid out."""

    @staticmethod
    def forward(ctx, x, weight, stride, pad, cache):
        ctx.fm = hip.snapshot_forms()  # the backward runs the forms of its forward
        x = _check_act(x, "stem_conv", images=True)
        cout, cin, kh, kw = weight.shape
        if x.size(1) != cin:
            raise hip.MSLError(f"stem_conv: weight {tuple(weight.shape)} does not match input {tuple(x.shape)}")
        h, w, n = x.shape[-2], x.shape[-1], _nimg(x)
        ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
        kk, p = cin * kh * kw, ho * wo * n
        lib = hip.load()
        s = hip.stream_ptr()
        col = _like(x, kk, ho, wo)
        hip.check(lib.msl_im2col(x.data_ptr(), cin, h, w, n, kh, kw, stride, pad, 1, ho, wo, col.data_ptr(), s),
                  "msl_im2col")
        wmat = weight.detach().contiguous()
        packed = cache.get([wmat], kk, cout, 0)
        y = _like(x, cout, ho, wo)
        # the bf16 / fp16 conv maths keep the stem (the raw image, values ~1e2; 2.5 GFLOP per image) in
        # the fp32 form: 8 significant bits there cost 3-4 % of the target loss after one update
        math = "fp32" if CONV_MATH in ("bf16", "fp16") else CONV_MATH
        # f16x3: the column matrix holds the image's values and padding zeros only, and with windows
        # that overlap (stride <= kernel) and reach both borders every pixel is in one: max |col| =
        # max |x|, so the GEMM's operand scale comes from the 3-channel image (r05: a 12-MB pass instead
        # of one over the 147 x P columns, 30-120 us).  The scale is a power of two of that maximum,
        # the same bits either way; the stem's weight gradient (64 x 147, exact-f32 tiles) reads none.
        cover = (stride <= min(kh, kw) and pad < min(kh, kw) and (ho - 1) * stride - pad + kh >= h and
                 (wo - 1) * stride - pad + kw >= w)
        cpart = _pconv_fwd(lib, math, col, packed, y, kk, cout, p, scale_from=x if cover else None)
        ctx.save_for_backward(col, weight)
        ctx.meta = (cin, h, w, n, kh, kw, stride, pad, ho, wo, cache, math)
        ctx.cpart = cpart
        return y

    @staticmethod
    def backward(ctx, gy):
        col, weight = ctx.saved_tensors
        cin, h, w, n, kh, kw, stride, pad, ho, wo, cache, math = ctx.meta
        cout, kk, p = weight.shape[0], col.size(1), ho * wo * n
        gy = gy.contiguous()
        lib = hip.load()
        s = hip.stream_ptr()
        dx = None
        gpart = _parts(gy, math, compute=_split_gemm(kk, cout))
        if ctx.needs_input_grad[0]:
            packed_d = cache.get([weight.detach().contiguous()], kk, cout, 1)
            dcol = torch.empty_like(col)
            wsb = lib.msl_pconv_dgrad_workspace(kk, cout, p)
            ws = hip.workspace(wsb, gy.device)
            _pconv_dgrad(lib, math, gy, packed_d, dcol, kk, cout, p, 0, ctx.fm, ws, wsb, gpart)
            dx = _like(col, cin, h, w)
            hip.check(lib.msl_col2im(dcol.data_ptr(), cin, h, w, n, kh, kw, stride, pad, 1, ho, wo, dx.data_ptr(), s),
                      "msl_col2im")
        if not ctx.needs_input_grad[1]:
            return dx, None, None, None, None
        dw = _pconv_wgrad(lib, math, col, gy, ctx.cpart, gpart, kk, cout, p, weight, ctx.fm)
        return dx, dw, None, None, None


def stem_conv(x, weight, stride, pad, cache):
    """nn.Conv2d(cin, cout, k, stride, pad, bias=False) (ResNetMulti.conv1, deeplab_multi.py:73-74)."""
    return _StemConv.apply(x, weight, int(stride), int(pad), cache)


class _MaxPool(Function):
    @staticmethod
    def forward(ctx, x, k, s, p, ceil):
        x = _check_act(x, "maxpool", images=True)
        h, w = x.shape[-2:]
        c = x.size(1) * _nimg(x)  # per plane: every (channel, image)
        ho, wo = pool_out(h, k, s, p, ceil), pool_out(w, k, s, p, ceil)
        y = _like(x, x.size(1), ho, wo)
        idx = _like(x, x.size(1), ho, wo, dtype=torch.int32)
        hip.check(hip.load().msl_maxpool_fwd(x.data_ptr(), c, h, w, k, s, p, ho, wo, y.data_ptr(), idx.data_ptr(),
                                             hip.stream_ptr()), "msl_maxpool_fwd")
        ctx.save_for_backward(idx)
        ctx.meta = (c, h, w, k, s, p, ho, wo)
        ctx.xshape = x.shape
        ctx.mark_non_differentiable(idx)
        return y, idx

    @staticmethod
    def backward(ctx, gy, _gi):
        (idx,) = ctx.saved_tensors
        c, h, w, k, s, p, ho, wo = ctx.meta
        gy = gy.contiguous()
        dx = torch.empty(ctx.xshape, dtype=_f32, device=gy.device)
        hip.check(hip.load().msl_maxpool_bwd(gy.data_ptr(), idx.data_ptr(), c, h, w, k, s, p, ho, wo, dx.data_ptr(),
                                             hip.stream_ptr()), "msl_maxpool_bwd")
        return dx, None, None, None, None


def maxpool2d(x, kernel_size, stride, padding, ceil_mode):
    """nn.MaxPool2d(k, s, p, ceil_mode) (deeplab_multi.py:77); returns the pooled tensor."""
    return _MaxPool.apply(x, int(kernel_size), int(stride), int(padding), bool(ceil_mode))[0]


class _Subsample(Function):
    @staticmethod
    def forward(ctx, x, s):
        x = _check_act(x, "subsample", images=True)
        h, w = x.shape[-2:]
        c = x.size(1) * _nimg(x)  # per plane
        ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
        y = _like(x, x.size(1), ho, wo)
        hip.check(hip.load().msl_subsample(x.data_ptr(), c, h, w, s, ho, wo, y.data_ptr(), hip.stream_ptr()),
                  "msl_subsample")
        ctx.meta = (c, h, w, s, ho, wo)
        ctx.xshape = x.shape
        return y

    @staticmethod
    def backward(ctx, gy):
        c, h, w, s, ho, wo = ctx.meta
        gy = gy.contiguous()
        dx = torch.empty(ctx.xshape, dtype=_f32, device=gy.device)
        hip.check(hip.load().msl_subsample_bwd(gy.data_ptr(), c, h, w, s, ho, wo, dx.data_ptr(), hip.stream_ptr()),
                  "msl_subsample_bwd")
        return dx, None


def subsample(x, stride):
    """x[:, :, ::stride, ::stride] (the input a stride-s 1x1 conv reads)."""
    return _Subsample.apply(x, int(stride))


# --------------------------------------------------------------------------- upsample
class _Upsample(Function):
    @staticmethod
    def forward(ctx, x, ho, wo):
        x = _check_act(x, "upsample")
        c, hi, wi = x.shape[1:]
        y = torch.empty((1, c, ho, wo), dtype=_f32, device=x.device)
        hip.check(hip.load().msl_upsample_fwd(x.data_ptr(), y.data_ptr(), c, hi, wi, ho, wo,
                                              hip.stream_ptr()), "msl_upsample_fwd")
        ctx.meta = (c, hi, wi, ho, wo)
        return y

    @staticmethod
    def backward(ctx, gy):
        c, hi, wi, ho, wo = ctx.meta
        gy = gy.contiguous()
        lib = hip.load()
        gx = torch.empty((1, c, hi, wi), dtype=_f32, device=gy.device)
        wsb = lib.msl_upsample_bwd_workspace(c, hi, wi, ho, wo)
        ws = hip.workspace(wsb, gy.device)
        hip.check(lib.msl_upsample_bwd(gy.data_ptr(), gx.data_ptr(), c, hi, wi, ho, wo, ws.data_ptr(),
                                       wsb, hip.stream_ptr()), "msl_upsample_bwd")
        return gx, None, None


def upsample_bilinear(x, size):
    """F.interpolate(x, size, mode='bilinear', align_corners=True) (deeplab_multi.py:124,128).

    The result carries `_msl_low` = x so the fused losses below can work from
    the low-resolution logits instead of re-reading the upsampled tensor.
    """
    y = _Upsample.apply(x, int(size[0]), int(size[1]))
    y._msl_low = (x, y._version, x._version)
    return y


def resize_bilinear(x, size):
    """F.interpolate(x, size, mode='bilinear', align_corners=True) of an image (1,C,H,W), C <= 4, up or
    down, with torch-CPU's rounding at every size (msl_resize_bilinear); no gradient."""
    x = _check_act(x.detach(), "resize_bilinear")
    c, hi, wi = x.shape[1:]
    ho, wo = int(size[0]), int(size[1])
    y = torch.empty((1, c, ho, wo), dtype=_f32, device=x.device)
    hip.check(hip.load().msl_resize_bilinear(x.data_ptr(), y.data_ptr(), c, hi, wi, ho, wo, hip.stream_ptr()),
              "msl_resize_bilinear")
    return y


# --------------------------------------------------------------------------- image pairs
def pair_join(x_s, x_t):
    """(1,C,H,W) x 2 -> the pair (1,C,2,H,W) ([C][2][H][W]) the trunk ops run as one batch."""
    return torch.stack([x_s, x_t], dim=2)


def pair_split(y):
    """(1,C,N,H,W) -> N contiguous (1,C,H,W) images (autograd stacks their gradients back)."""
    return tuple(t.contiguous() for t in y.unbind(2))


# --------------------------------------------------------------------------- fused losses
def _stats(device):
    return torch.empty(hip.load().msl_loss_stats_elems(), dtype=_f32, device=device)


def _geom(low, out_hw):
    c, hi, wi = low.shape[1:]
    return c, hi, wi, int(out_hw[0]), int(out_hw[1])


def _iw_outputs(c, device):
    """(hist int32[C], weights fp32[C]): the importance-weighted losses' extra outputs."""
    return torch.empty(c, dtype=torch.int32, device=device), torch.empty(c, dtype=_f32, device=device)


# The fused upsample-loss kinds: kind -> (second operand: None, "labels" or "low2"; the float argument
# after the geometry or None; whether the backward takes that float too; whether the forward also
# writes the IW histogram and class weights).  The entry points are msl_<kind>_up_fwd / _bwd:
#   fwd(low, [operand], c, hi, wi, ho, wo, [float], out, stats, [hist, weights], ws, wsb, stream)
#   bwd(low, [operand], c, hi, wi, ho, wo, [float], stats, g, d, ws, wsb, stream)
_UP_LOSSES = {
    "ce": ("labels", None, False, False),
    "maxsquare": (None, None, False, False),
    "iw_maxsquare": (None, "ratio", False, True),
    "multi_ce": ("low2", "thr", True, False),
    "entropy": (None, None, False, False),
    "iw_entropy": (None, "ratio", False, True),
    "hard_ce": (None, "thr", True, False),
}


class _LossUp(Function):
    """A loss of the upsampled logits computed from the low-resolution ones, by `kind` (_UP_LOSSES)."""

    @staticmethod
    def forward(ctx, kind, low, other, ho, wo, val):
        operand, fname, val_bwd, iw = _UP_LOSSES[kind]
        low = _check_act(low, kind + "_up")
        if operand == "low2":
            other = _check_act(other.detach(), kind + "_up")
        elif operand == "labels":
            other = other.contiguous()
        c, hi, wi, ho, wo = geo = _geom(low, (ho, wo))
        if operand == "labels" and (other.dtype != torch.int64 or other.numel() != ho * wo):
            raise hip.MSLError(f"{kind}_up: labels must be int64 with {ho*wo} elements")
        lib = hip.load()
        out = torch.empty((), dtype=_f32, device=low.device)
        st = _stats(low.device)
        extra = _iw_outputs(c, low.device) if iw else ()
        wsb = lib.msl_loss_workspace(*geo)
        ws = hip.workspace(wsb, low.device)
        head = (low.data_ptr(),) if operand is None else (low.data_ptr(), other.data_ptr())
        fval = () if fname is None else (float(val),)
        name = f"msl_{kind}_up_fwd"
        hip.check(getattr(lib, name)(*head, *geo, *fval, out.data_ptr(), st.data_ptr(),
                                     *(t.data_ptr() for t in extra), ws.data_ptr(), wsb, hip.stream_ptr()), name)
        ctx.save_for_backward(*((low, st) if operand is None else (low, other, st)))
        ctx.call = (kind, geo + (fval if val_bwd else ()))
        if not iw:
            return out
        ctx.mark_non_differentiable(*extra)
        return (out, *extra)

    @staticmethod
    def backward(ctx, g, *_unused):
        *head, st = ctx.saved_tensors
        kind, geo = ctx.call
        lib = hip.load()
        g = g.to(_f32).contiguous()
        d = torch.empty_like(head[0])
        wsb = lib.msl_loss_workspace(*geo[:5])
        ws = hip.workspace(wsb, d.device)
        name = f"msl_{kind}_up_bwd"
        hip.check(getattr(lib, name)(*(t.data_ptr() for t in head), *geo, st.data_ptr(), g.data_ptr(),
                                     d.data_ptr(), ws.data_ptr(), wsb, hip.stream_ptr()), name)
        return None, d, None, None, None, None


def low_of(pred):
    """The low-resolution logits behind an upsampled prediction, or None when there are none or
    when either tensor was modified in place since the upsample (then the loss must read `pred`
    itself: the fused path would silently ignore the edit)."""
    rec = getattr(pred, "_msl_low", None)
    if rec is None:
        return None
    low, v_pred, v_low = rec
    if pred._version != v_pred or low._version != v_low:
        return None
    return low


def loss_labels_up(low1, low2, out_hw, thr=0.95):
    """(argmax, label2) int32 [ho*wo]: the per-pixel decisions of the fused losses - first-max
    argmax of softmax(up(low1)) (IW histogram class) and, if low2 is given, the multi-level
    guidance label with low1 = x1 head, low2 = x2 head (solve_gta5.py:206-212)."""
    low1 = _check_act(low1.detach(), "loss_labels_up")
    c, hi, wi, ho, wo = _geom(low1, out_hw)
    arg = torch.empty(ho * wo, dtype=torch.int32, device=low1.device)
    lab = None
    if low2 is not None:
        low2 = _check_act(low2.detach(), "loss_labels_up")
        lab = torch.empty(ho * wo, dtype=torch.int32, device=low1.device)
    hip.check(hip.load().msl_loss_labels_up(low1.data_ptr(), hip.ptr(low2), c, hi, wi, ho, wo, float(thr),
                                            arg.data_ptr(), hip.ptr(lab), hip.stream_ptr()), "msl_loss_labels_up")
    return arg, lab


def ce_up(low, labels, out_hw):
    return _LossUp.apply("ce", low, labels, int(out_hw[0]), int(out_hw[1]), None)


def maxsquare_up(low, out_hw):
    return _LossUp.apply("maxsquare", low, None, int(out_hw[0]), int(out_hw[1]), None)


def iw_maxsquare_up(low, out_hw, ratio):
    """Returns (loss, hist int32[C], weights fp32[C])."""
    return _LossUp.apply("iw_maxsquare", low, None, int(out_hw[0]), int(out_hw[1]), float(ratio))


def multi_ce_up(low1, low2, out_hw, thr):
    return _LossUp.apply("multi_ce", low1, low2, int(out_hw[0]), int(out_hw[1]), float(thr))


def entropy_up(low, out_hw):
    """softCrossEntropy()(pred, softmax(pred)) of the upsampled logits (loss.py:17-35): the mean over
    C*H*W of -log_softmax * softmax, the gradient through both factors."""
    return _LossUp.apply("entropy", low, None, int(out_hw[0]), int(out_hw[1]), None)


def iw_entropy_up(low, out_hw, ratio):
    """IWsoftCrossEntropy(ratio)(pred, softmax(pred)) (loss.py:37-67).  Returns (loss, hist int32[C] of
    the logits' argmax, weights fp32[C])."""
    return _LossUp.apply("iw_entropy", low, None, int(out_hw[0]), int(out_hw[1]), float(ratio))


def hard_ce_up(low, out_hw, thr):
    """CE(pred, label) with the pseudo-label argmax p where max p > thr, else ignored
    (solve_gta5.py:185-199); nan with a zero gradient when no pixel passes."""
    return _LossUp.apply("hard_ce", low, None, int(out_hw[0]), int(out_hw[1]), float(thr))


def _pseudo(low, out_hw, thr, want_label, want_arg):
    low = _check_act(low.detach(), "pseudo_labels_up")
    c, hi, wi, ho, wo = _geom(low, out_hw)
    lab = torch.empty(ho * wo, dtype=torch.int32, device=low.device) if want_label else None
    arg = torch.empty(ho * wo, dtype=torch.int32, device=low.device) if want_arg else None
    hip.check(hip.load().msl_pseudo_labels_up(low.data_ptr(), c, hi, wi, ho, wo, float(thr), hip.ptr(lab),
                                              hip.ptr(arg), hip.stream_ptr()), "msl_pseudo_labels_up")
    return lab, arg


def pseudo_labels_up(low, out_hw, thr):
    """int32 [ho*wo]: the pseudo-label hard_ce_up trains on (-1 = ignored)."""
    return _pseudo(low, out_hw, thr, True, False)[0]


def logits_argmax_up(low, out_hw):
    """int32 [ho*wo]: the first-max argmax of the upsampled logits (iw_entropy_up's histogram class)."""
    return _pseudo(low, out_hw, 0.0, False, True)[1]


# --------------------------------------------------------------------------- evaluation
def _check_label(name, label, confusion, c, ho, wo):
    """The label / confusion pair of every predict_* wrapper: both or neither; returns the contiguous label."""
    if (label is None) != (confusion is None):
        raise hip.MSLError(f"{name}: label and confusion go together")
    if label is None:
        return None
    label = label.contiguous()
    if not label.is_cuda or label.dtype != torch.int64 or label.numel() != ho * wo:
        raise hip.MSLError(f"{name}: label must be a CUDA int64 tensor with {ho * wo} elements")
    if (not confusion.is_cuda or confusion.dtype != torch.int64 or confusion.numel() != c * c or
            not confusion.is_contiguous()):
        raise hip.MSLError(f"{name}: confusion must be a contiguous CUDA int64 tensor with {c * c} elements")
    return label


def predict_up(low, out_hw, low_flip=None, label=None, confusion=None, want_argmax=False):
    """The evaluator's per-pixel class (tools/evaluate.py:114-141) from the low-resolution logits
    `low` (1,C,hi,wi), fused with the confusion matrix (msl_predict_up): np.argmax of the upsampled
    logits, or - with `low_flip`, the low-res logits of the horizontally mirrored image - of
    (softmax(up(low)) + mirror(softmax(up(low_flip)))) / 2.  `label` (int64, ho*wo elements) and
    `confusion` (int64 [C*C] on the device, accumulated in place) go together; returns the int32
    [ho*wo] class map when `want_argmax`, else None."""
    low = _check_act(low.detach(), "predict_up")
    c, hi, wi, ho, wo = _geom(low, out_hw)
    if low_flip is not None:
        low_flip = _check_act(low_flip.detach(), "predict_up")
        if low_flip.shape != low.shape:
            raise hip.MSLError("predict_up: low_flip must have low's shape")
    label = _check_label("predict_up", label, confusion, c, ho, wo)
    if label is None and not want_argmax:
        raise hip.MSLError("predict_up: nothing to compute (no label / confusion and want_argmax=False)")
    arg = torch.empty(ho * wo, dtype=torch.int32, device=low.device) if want_argmax else None
    hip.check(hip.load().msl_predict_up(low.data_ptr(), hip.ptr(low_flip), c, hi, wi, ho, wo, hip.ptr(label),
                                        hip.ptr(confusion), hip.ptr(arg), hip.stream_ptr()), "msl_predict_up")
    return arg


def predict_rectify(low, crop0, crop1, out_hw, segy0, label=None, confusion=None, want_argmax=False):
    """predict_up without flip followed by the reference's Trainer.rectification with both crops, one launch
    (msl_predict_rectify): `crop0` / `crop1` are the low-resolution logits of the left and right half-size
    windows, magnified, stylised and forwarded; inside rows [segy0, segy0 + ho/2) a crop's class replaces the
    pixel's where its winning logit is strictly greater.  label / confusion / want_argmax as predict_up."""
    low = _check_act(low.detach(), "predict_rectify")
    c, hi, wi, ho, wo = _geom(low, out_hw)
    crops = []
    for t in (crop0, crop1):
        t = _check_act(t.detach(), "predict_rectify")
        if t.shape != low.shape:
            raise hip.MSLError("predict_rectify: the crops' logits must have low's shape")
        crops.append(t)
    label = _check_label("predict_rectify", label, confusion, c, ho, wo)
    if label is None and not want_argmax:
        raise hip.MSLError("predict_rectify: nothing to compute (no label / confusion and want_argmax=False)")
    arg = torch.empty(ho * wo, dtype=torch.int32, device=low.device) if want_argmax else None
    hip.check(hip.load().msl_predict_rectify(low.data_ptr(), crops[0].data_ptr(), crops[1].data_ptr(), c, hi, wi, ho, wo,
                                             int(segy0), hip.ptr(label), hip.ptr(confusion), hip.ptr(arg),
                                             hip.stream_ptr()), "msl_predict_rectify")
    return arg


# the maps of predict_images: name -> trailing shape after (ho, wo)
IMAGE_MAPS = {"class": (), "ids": (), "color": (3,), "confidence": (3,), "pseudo": ()}
_IMAGE_TABLES = {}  # (num_classes, device) -> (id_lut [C], palette [C*3], shade [4*C*3]) uint8 on the device


def image_tables(num_classes, device):
    """The three device tables of msl_predict_images (utils/palette.py), built once per class count."""
    key = (int(num_classes), torch.device(device))
    if key not in _IMAGE_TABLES:
        from .utils import palette
        try:
            host = (palette.id_table(key[0]), palette.palette_table(key[0]), palette.shade_table(key[0]))
        except ValueError as e:
            raise hip.MSLError(str(e)) from e
        _IMAGE_TABLES[key] = tuple(torch.from_numpy(t.reshape(-1).copy()).to(key[1]) for t in host)
    return _IMAGE_TABLES[key]


def image_buffers(out_hw, want, device):
    """Empty uint8 outputs of predict_images for the maps in `want` (static buffers of a captured graph)."""
    ho, wo = int(out_hw[0]), int(out_hw[1])
    bad = [k for k in want if k not in IMAGE_MAPS]
    if bad:
        raise hip.MSLError(f"predict_images: unknown maps {bad}; choose from {sorted(IMAGE_MAPS)}")
    return {k: torch.empty((ho, wo) + IMAGE_MAPS[k], dtype=torch.uint8, device=device) for k in want}


def _image_outputs(name, out, want, ho, wo, device, label):
    """The checked output maps of an image wrapper: `out`, or fresh buffers for `want`; with neither a map nor a
    label there is nothing to compute."""
    if out is None:
        out = image_buffers((ho, wo), want, device)
    for k, t in out.items():
        if (k not in IMAGE_MAPS or not t.is_cuda or t.dtype != torch.uint8 or not t.is_contiguous() or
                tuple(t.shape) != (ho, wo) + IMAGE_MAPS[k]):
            raise hip.MSLError(f"{name}: output {k!r} must be a contiguous CUDA uint8 tensor of shape "
                               f"{(ho, wo) + IMAGE_MAPS.get(k, ())}")
    if not out and label is None:
        raise hip.MSLError(f"{name}: nothing to compute (no map and no label / confusion)")
    return out


def predict_images(low, out_hw, low_flip=None, label=None, confusion=None, want=("color",), thr=0.95, out=None):
    """predict_up's decision as uint8 images, in the same single launch (msl_predict_images).  `want` names
    the maps (IMAGE_MAPS): "class" (ho,wo) the class index, "ids" (ho,wo) its Cityscapes labelId, "color"
    (ho,wo,3) its colour, "confidence" (ho,wo,3) the colour shaded by the winning probability (> 0.9 full,
    > 0.8, > 0.7, > 0.5, else black), "pseudo" (ho,wo) the class where that probability > `thr`, else 255.
    `label` / `confusion` as in predict_up.  `out`: a dict of buffers from image_buffers to write into
    (then `want` is its keys).  Returns the dict of maps."""
    low = _check_act(low.detach(), "predict_images")
    c, hi, wi, ho, wo = _geom(low, out_hw)
    if low_flip is not None:
        low_flip = _check_act(low_flip.detach(), "predict_images")
        if low_flip.shape != low.shape:
            raise hip.MSLError("predict_images: low_flip must have low's shape")
    label = _check_label("predict_images", label, confusion, c, ho, wo)
    out = _image_outputs("predict_images", out, want, ho, wo, low.device, label)
    id_lut, pal, shade = image_tables(c, low.device)
    hip.check(hip.load().msl_predict_images(
        low.data_ptr(), hip.ptr(low_flip), c, hi, wi, ho, wo, hip.ptr(label), hip.ptr(confusion), float(thr),
        id_lut.data_ptr(), pal.data_ptr(), shade.data_ptr(), hip.ptr(out.get("class")), hip.ptr(out.get("ids")),
        hip.ptr(out.get("color")), hip.ptr(out.get("confidence")), hip.ptr(out.get("pseudo")), hip.stream_ptr()),
        "msl_predict_images")
    return out


def _tta_table(entries, name):
    """(msl_tta_entry array, the checked tensors, C) of `entries`: (low (1,C,hi,wi), mirror) pairs, the
    low-resolution logits of the image at some input scale or - mirror - of that image's horizontal mirror."""
    entries = list(entries)
    cap = hip.load().msl_predict_tta_max_entries()
    if not 1 <= len(entries) <= cap:
        raise hip.MSLError(f"{name}: {len(entries)} entries; 1 to {cap} are fused in one launch")
    lows = [_check_act(low.detach(), name) for low, _ in entries]
    c = lows[0].shape[1]
    table = (hip.TtaEntry * len(lows))()
    for k, (low, (_, mirror)) in enumerate(zip(lows, entries)):
        if low.shape[1] != c or low.device != lows[0].device:
            raise hip.MSLError(f"{name}: entry {k} has {low.shape[1]} classes on {low.device}, entry 0 {c} on "
                               f"{lows[0].device}")
        if mirror not in (0, 1, False, True):
            raise hip.MSLError(f"{name}: entry {k}'s mirror is {mirror!r}, not 0 or 1")
        table[k] = hip.TtaEntry(low.data_ptr(), low.shape[2], low.shape[3], int(mirror))
    return table, lows, c


def predict_tta(entries, out_hw, label=None, confusion=None, want_argmax=False):
    """Multi-scale / mirror test-time augmentation in one launch (msl_predict_tta).  `entries`: (low, mirror)
    pairs, low (1,C,hi,wi) the low-resolution logits of the image at some input scale, mirror 1 when they are
    those of that image's horizontal mirror; each has its own hi, wi.  The class is np.argmax of the sum, in
    the entries' order, of softmax(up(low)) - mirrored back where mirror - at out_hw; [(low, 0), (low_flip, 1)]
    is predict_up's --flip class bit for bit.  label / confusion / want_argmax as predict_up."""
    table, lows, c = _tta_table(entries, "predict_tta")
    ho, wo = int(out_hw[0]), int(out_hw[1])
    label = _check_label("predict_tta", label, confusion, c, ho, wo)
    if label is None and not want_argmax:
        raise hip.MSLError("predict_tta: nothing to compute (no label / confusion and want_argmax=False)")
    arg = torch.empty(ho * wo, dtype=torch.int32, device=lows[0].device) if want_argmax else None
    hip.check(hip.load().msl_predict_tta(table, len(lows), c, ho, wo, hip.ptr(label), hip.ptr(confusion),
                                         hip.ptr(arg), hip.stream_ptr()), "msl_predict_tta")
    return arg


def predict_tta_images(entries, out_hw, label=None, confusion=None, want=("color",), thr=0.95, out=None):
    """predict_tta's class as predict_images' uint8 maps, in the same single launch
    (msl_predict_tta_images); the probability behind "confidence" and "pseudo" is the summed probability of
    the class divided by the number of entries.  `want`, `thr`, `out` and the result as predict_images."""
    table, lows, c = _tta_table(entries, "predict_tta_images")
    ho, wo = int(out_hw[0]), int(out_hw[1])
    label = _check_label("predict_tta_images", label, confusion, c, ho, wo)
    out = _image_outputs("predict_tta_images", out, want, ho, wo, lows[0].device, label)
    id_lut, pal, shade = image_tables(c, lows[0].device)
    hip.check(hip.load().msl_predict_tta_images(
        table, len(lows), c, ho, wo, hip.ptr(label), hip.ptr(confusion), float(thr), id_lut.data_ptr(),
        pal.data_ptr(), shade.data_ptr(), hip.ptr(out.get("class")), hip.ptr(out.get("ids")),
        hip.ptr(out.get("color")), hip.ptr(out.get("confidence")), hip.ptr(out.get("pseudo")), hip.stream_ptr()),
        "msl_predict_tta_images")
    return out


# --------------------------------------------------------------------------- class-balanced thresholds
def _source_of(name, low, low_flip, entries):
    """The source of a confidence / pseudo-label call: single scale (`low`, optional `low_flip`) or an entry
    table (`entries`, as predict_tta).  Returns (entry point suffix, leading arguments, C, device, the
    (hi, wi) of a single-scale call, the tensors to keep alive)."""
    if entries is not None:
        if low is not None or low_flip is not None:
            raise hip.MSLError(f"{name}: give low (and low_flip) or entries, not both")
        table, lows, c = _tta_table(entries, name)
        return "_tta", (table, len(lows)), c, lows[0].device, (), lows
    if low is None:
        raise hip.MSLError(f"{name}: give low (and low_flip) or entries")
    low = _check_act(low.detach(), name)
    if low_flip is not None:
        low_flip = _check_act(low_flip.detach(), name)
        if low_flip.shape != low.shape:
            raise hip.MSLError(f"{name}: low_flip must have low's shape")
    return "", (low.data_ptr(), hip.ptr(low_flip)), low.shape[1], low.device, tuple(low.shape[2:]), (low, low_flip)


def confidence_buffers(num_classes, bins, device):
    """(hist int64 [C, bins], thr fp32 [C], kept int64 [C]) on the device: the zeroed histogram of
    confidence_hist and the outputs of class_thresholds (the counts are uint64 in the library)."""
    return (torch.zeros((int(num_classes), int(bins)), dtype=torch.int64, device=device),
            torch.empty(int(num_classes), dtype=_f32, device=device),
            torch.zeros(int(num_classes), dtype=torch.int64, device=device))


def _check_hist(name, hist, c):
    if (not hist.is_cuda or hist.dtype != torch.int64 or hist.dim() != 2 or hist.shape[0] != c or
            not hist.is_contiguous()):
        raise hip.MSLError(f"{name}: hist must be a contiguous CUDA int64 tensor of shape ({c}, bins)")
    return int(hist.shape[1])


def confidence_hist(hist, out_hw, low=None, low_flip=None, entries=None):
    """hist[class][bin] += 1 for every pixel of out_hw (msl_confidence_hist[_tta]): the class is predict_up's
    (predict_tta's with `entries`), the bin min(bins - 1, int(top * bins)) of the probability behind
    predict_images' "pseudo" map.  `hist`: int64 [C, bins] on the device, accumulated in place; bins a power
    of two in [16, 1024] with C * bins <= 16384.  A NaN pixel is not counted."""
    sfx, head, c, device, hw, keep = _source_of("confidence_hist", low, low_flip, entries)
    bins = _check_hist("confidence_hist", hist, c)
    ho, wo = int(out_hw[0]), int(out_hw[1])
    name = "msl_confidence_hist" + sfx
    hip.check(getattr(hip.load(), name)(*head, c, *hw, ho, wo, bins, hist.data_ptr(), hip.stream_ptr()), name)
    return hist


def class_thresholds(hist, portion, thr_max, thr=None, kept=None):
    """One threshold per class from a confidence histogram (msl_class_thresholds): the largest bin edge that
    still keeps `portion` of the class's pixels at or above it, capped at `thr_max`; an empty class gets
    thr_max.  Writes `thr` (fp32 [C]) and `kept` (int64 [C]: the pixels at or above the threshold's bin), fresh
    tensors when not given; nothing is read by the host.  Returns (thr, kept)."""
    c = hist.shape[0] if hist.dim() == 2 else -1
    bins = _check_hist("class_thresholds", hist, c)
    if thr is None:
        thr = torch.empty(c, dtype=_f32, device=hist.device)
    if kept is None:
        kept = torch.empty(c, dtype=torch.int64, device=hist.device)
    for t, dt, what in ((thr, _f32, "thr"), (kept, torch.int64, "kept")):
        if not t.is_cuda or t.dtype != dt or t.numel() != c or not t.is_contiguous():
            raise hip.MSLError(f"class_thresholds: {what} must be a contiguous CUDA {dt} tensor with {c} elements")
    hip.check(hip.load().msl_class_thresholds(hist.data_ptr(), c, bins, float(portion), float(thr_max),
                                              thr.data_ptr(), kept.data_ptr(), hip.stream_ptr()),
              "msl_class_thresholds")
    return thr, kept


def pseudo_classwise(thr, out_hw, low=None, low_flip=None, entries=None, label=None, pseudo=None,
                     want=("label",)):
    """The pseudo-label under one threshold per class (msl_pseudo_classwise[_tta]): the class where the
    winning probability > thr[class], else ignored.  `thr`: fp32 [C] on the device, read by the kernel.
    Writes `label` (int64 [ho*wo], -1 = ignored) and / or `pseudo` (uint8 (ho, wo), 255 = ignored): the
    buffers given, or fresh ones for the names in `want`.  Returns (label, pseudo), None where not written."""
    sfx, head, c, device, hw, keep = _source_of("pseudo_classwise", low, low_flip, entries)
    ho, wo = int(out_hw[0]), int(out_hw[1])
    if not thr.is_cuda or thr.dtype != _f32 or thr.numel() != c or not thr.is_contiguous():
        raise hip.MSLError(f"pseudo_classwise: thr must be a contiguous CUDA float32 tensor with {c} elements")
    if label is None and pseudo is None:
        if "label" in want:
            label = torch.empty(ho * wo, dtype=torch.int64, device=device)
        if "pseudo" in want:
            pseudo = torch.empty((ho, wo), dtype=torch.uint8, device=device)
    for t, dt, what in ((label, torch.int64, "label"), (pseudo, torch.uint8, "pseudo")):
        if t is not None and (not t.is_cuda or t.dtype != dt or t.numel() != ho * wo or not t.is_contiguous()):
            raise hip.MSLError(f"pseudo_classwise: {what} must be a contiguous CUDA {dt} tensor with {ho * wo} "
                               "elements")
    if label is None and pseudo is None:
        raise hip.MSLError("pseudo_classwise: nothing to compute (no label and no pseudo map)")
    name = "msl_pseudo_classwise" + sfx
    hip.check(getattr(hip.load(), name)(*head, c, *hw, ho, wo, thr.data_ptr(), hip.ptr(label), hip.ptr(pseudo),
                                        hip.stream_ptr()), name)
    return label, pseudo


def colorize(mask, palette):
    """decode_labels on the device (msl_colorize): `mask` a CUDA int64 / int32 class map of any shape S,
    `palette` a CUDA uint8 [C, 3]; returns uint8 S + (3,), black where the value is outside [0, C)."""
    if not mask.is_cuda or mask.dtype not in (torch.int64, torch.int32):
        raise hip.MSLError(f"colorize: expected a CUDA int64 or int32 class map, got {mask.dtype} {mask.device}")
    if (not palette.is_cuda or palette.dtype != torch.uint8 or palette.dim() != 2 or palette.size(1) != 3 or
            palette.device != mask.device):
        raise hip.MSLError("colorize: palette must be a uint8 [C, 3] tensor on the mask's device")
    mask, palette = mask.contiguous(), palette.contiguous()
    out = torch.empty(tuple(mask.shape) + (3,), dtype=torch.uint8, device=mask.device)
    hip.check(hip.load().msl_colorize(mask.data_ptr(), int(mask.dtype == torch.int64), mask.numel(),
                                      palette.data_ptr(), palette.size(0), out.data_ptr(), hip.stream_ptr()),
              "msl_colorize")
    return out


# --------------------------------------------------------------------------- per-image analysis
METRICS_HEAD = ("PA", "MPA", "MIoU", "FWIoU", "MPA_13", "MIoU_13", "FWIoU_13", "pixels", "selected")
ANALYSIS_MAPS = ("label", "pred", "input", "error")  # msl_analysis_maps' outputs, in its argument order
_MEAN_TABLES = {}  # device -> IMG_MEAN as fp32 [3] on the device


def metrics_buffers(num_classes, capacity, device):
    """(rows fp64 [capacity, 9 + C], state int32 [3] = {cursor, selected, slot}) of image_metrics, zeroed."""
    return (torch.zeros((int(capacity), len(METRICS_HEAD) + int(num_classes)), dtype=torch.float64, device=device),
            torch.zeros(3, dtype=torch.int32, device=device))


def image_metrics(image_cm, total_cm, threshold, rows, state):
    """One image's scores on the device (msl_image_metrics): from `image_cm`, the int64 [C*C] matrix the
    image's prediction launch just filled, row state[0] % capacity of `rows` (metrics_buffers) becomes
    [PA, MPA, MIoU, FWIoU, MPA_13, MIoU_13, FWIoU_13, pixels, selected, iou[0..C-1]] by utils/eval.py:Eval's
    definitions, selected = val_info's MIoU < threshold (strict; NaN is not selected); then total_cm +=
    image_cm, image_cm = 0 and `state` = {cursor + 1, selected, slot}.  Nothing syncs."""
    cc = image_cm.numel()
    c = int(round(cc ** 0.5))
    for name, t in (("image_cm", image_cm), ("total_cm", total_cm)):
        if not t.is_cuda or t.dtype != torch.int64 or not t.is_contiguous() or t.numel() != cc or c * c != cc:
            raise hip.MSLError(f"image_metrics: {name} must be a contiguous CUDA int64 tensor with C*C elements")
    if (not rows.is_cuda or rows.dtype != torch.float64 or not rows.is_contiguous() or rows.dim() != 2 or
            rows.size(0) < 1 or rows.size(1) != len(METRICS_HEAD) + c):
        raise hip.MSLError(f"image_metrics: rows must be a contiguous CUDA float64 [capacity, {len(METRICS_HEAD) + c}]")
    if not state.is_cuda or state.dtype != torch.int32 or not state.is_contiguous() or state.numel() != 3:
        raise hip.MSLError("image_metrics: state must be a contiguous CUDA int32 tensor with 3 elements")
    hip.check(hip.load().msl_image_metrics(image_cm.data_ptr(), total_cm.data_ptr(), c, float(threshold),
                                           rows.data_ptr(), rows.size(0), state.data_ptr(), hip.stream_ptr()),
              "msl_image_metrics")


def analysis_buffers(hw, want, slots, device):
    """Empty uint8 [slots, h, w, 3] rings of analysis_maps for the maps in `want`."""
    bad = [k for k in want if k not in ANALYSIS_MAPS]
    if bad:
        raise hip.MSLError(f"analysis_maps: unknown maps {bad}; choose from {list(ANALYSIS_MAPS)}")
    return {k: torch.empty((int(slots), int(hw[0]), int(hw[1]), 3), dtype=torch.uint8, device=device) for k in want}


def analysis_maps(x, label, cls, num_classes, want=("label", "pred", "input"), state=None, out=None, palette=None):
    """The failure maps of one image (msl_analysis_maps), uint8 (h, w, 3) RGB each: "label" the label's
    colours (black outside [0, C)), "pred" those of `cls` - the uint8 (h, w) class map of predict_images -,
    "input" the image recovered from the network input `x` (1,3,h,w) (utils/images.py:recover_input's bytes),
    "error" black where unlabelled, the dimmed input where cls == label, the predicted colour where not.
    `state`: image_metrics' - the launch returns at once unless state[1], and writes slot state[2] of `out`.
    `out`: rings from analysis_buffers (then `want` is its keys; without `state` slot 0 is written); else fresh
    one-slot buffers.  `palette`: a CUDA uint8 [C, 3] instead of the class count's own.  Returns the dict."""
    c = int(num_classes)
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4 or x.size(0) != 1 or x.size(1) != 3:
        raise hip.MSLError("analysis_maps: x must be a CUDA fp32 (1, 3, h, w) network input")
    x = x.contiguous()
    h, w = int(x.shape[2]), int(x.shape[3])
    if out is None:
        out = analysis_buffers((h, w), want, 1, x.device)
    if not out:
        raise hip.MSLError("analysis_maps: nothing to compute (no map)")
    slots = {int(t.shape[0]) if t.dim() == 4 else -1 for t in out.values()}
    for k, t in out.items():
        if (k not in ANALYSIS_MAPS or not t.is_cuda or t.dtype != torch.uint8 or not t.is_contiguous() or
                t.dim() != 4 or tuple(t.shape[1:]) != (h, w, 3)):
            raise hip.MSLError(f"analysis_maps: output {k!r} must be a contiguous CUDA uint8 [slots, {h}, {w}, 3]")
    if len(slots) != 1:
        raise hip.MSLError("analysis_maps: the rings must have the same number of slots")
    if label is not None:
        label = label.contiguous()
        if not label.is_cuda or label.dtype != torch.int64 or label.numel() != h * w:
            raise hip.MSLError(f"analysis_maps: label must be a CUDA int64 tensor with {h * w} elements")
    if cls is not None and (not cls.is_cuda or cls.dtype != torch.uint8 or not cls.is_contiguous() or
                            cls.numel() != h * w):
        raise hip.MSLError(f"analysis_maps: cls must be a contiguous CUDA uint8 tensor with {h * w} elements")
    if state is not None and (not state.is_cuda or state.dtype != torch.int32 or not state.is_contiguous() or
                              state.numel() != 3):
        raise hip.MSLError("analysis_maps: state must be a contiguous CUDA int32 tensor with 3 elements")
    if palette is None:
        palette = image_tables(c, x.device)[1]
    elif (not palette.is_cuda or palette.dtype != torch.uint8 or not palette.is_contiguous() or
          palette.numel() != 3 * c):
        raise hip.MSLError(f"analysis_maps: palette must be a contiguous CUDA uint8 [{c}, 3]")
    if x.device not in _MEAN_TABLES:
        from .utils.synthetic import IMG_MEAN
        _MEAN_TABLES[x.device] = torch.tensor([float(v) for v in IMG_MEAN], dtype=torch.float32, device=x.device)
    hip.check(hip.load().msl_analysis_maps(
        x.data_ptr(), _MEAN_TABLES[x.device].data_ptr(), hip.ptr(label), hip.ptr(cls), palette.data_ptr(), c, h, w,
        hip.ptr(state), h * w * 3, *(hip.ptr(out.get(k)) for k in ANALYSIS_MAPS), hip.stream_ptr()),
        "msl_analysis_maps")
    return out


# --------------------------------------------------------------------------- soft cross-entropy, explicit target
class _SoftCE(Function):
    """softCrossEntropy (ratio None) / IWsoftCrossEntropy on (1,C,H,W) logits and an explicit target."""

    @staticmethod
    def forward(ctx, inputs, target, ignore, ratio):
        inputs = _check_act(inputs, "soft_ce")
        target = _check_act(target, "soft_ce")
        if inputs.shape != target.shape:
            raise hip.MSLError(f"soft_ce: inputs {tuple(inputs.shape)} and target {tuple(target.shape)} differ")
        c, hw = inputs.size(1), inputs.size(2) * inputs.size(3)
        lib = hip.load()
        out = torch.empty((), dtype=_f32, device=inputs.device)
        st = _stats(inputs.device)
        wsb = lib.msl_loss_workspace(c, 1, 1, 1, hw)
        ws = hip.workspace(wsb, inputs.device)
        ctx.save_for_backward(inputs, target, st)
        ctx.meta = (c, hw, float(ignore), ratio is not None)
        if ratio is None:
            hip.check(lib.msl_soft_ce_fwd(inputs.data_ptr(), target.data_ptr(), c, hw, float(ignore), out.data_ptr(),
                                          st.data_ptr(), ws.data_ptr(), wsb, hip.stream_ptr()), "msl_soft_ce_fwd")
            return out
        hist, weights = _iw_outputs(c, inputs.device)
        hip.check(lib.msl_iw_soft_ce_fwd(inputs.data_ptr(), target.data_ptr(), c, hw, float(ignore), float(ratio),
                                         out.data_ptr(), st.data_ptr(), hist.data_ptr(), weights.data_ptr(),
                                         ws.data_ptr(), wsb, hip.stream_ptr()), "msl_iw_soft_ce_fwd")
        ctx.mark_non_differentiable(hist, weights)
        return out, hist, weights

    @staticmethod
    def backward(ctx, g, *_unused):
        inputs, target, st = ctx.saved_tensors
        c, hw, ignore, iw = ctx.meta
        g = g.to(_f32).contiguous()
        di = torch.empty_like(inputs) if ctx.needs_input_grad[0] else None
        dt = torch.empty_like(target) if ctx.needs_input_grad[1] else None
        lib = hip.load()
        fn = lib.msl_iw_soft_ce_bwd if iw else lib.msl_soft_ce_bwd
        hip.check(fn(inputs.data_ptr(), target.data_ptr(), c, hw, ignore, st.data_ptr(), g.data_ptr(), hip.ptr(di),
                     hip.ptr(dt), hip.stream_ptr()), "msl_soft_ce_bwd")
        return di, dt, None, None


def soft_ce(inputs, target, ignore_index=-1):
    """softCrossEntropy(ignore_index)(inputs, target) (loss.py:17-35): the mean of -log_softmax(inputs) *
    target over the elements with target != ignore_index; gradients to both."""
    return _SoftCE.apply(inputs, target, float(ignore_index), None)


def iw_soft_ce(inputs, target, ratio, ignore_index=-1):
    """IWsoftCrossEntropy (loss.py:37-67) on explicit tensors.  Returns (loss, hist, weights)."""
    return _SoftCE.apply(inputs, target, float(ignore_index), float(ratio))


# --------------------------------------------------------------------------- prob-input losses
class _MaxSquareProb(Function):
    @staticmethod
    def forward(ctx, prob):
        prob = _check_act(prob, "maxsquare_prob")
        c, hw = prob.size(1), prob.size(2) * prob.size(3)
        lib = hip.load()
        out = torch.empty((), dtype=_f32, device=prob.device)
        wsb = lib.msl_loss_workspace(c, 1, 1, 1, hw)
        ws = hip.workspace(wsb, prob.device)
        hip.check(lib.msl_maxsquare_prob_fwd(prob.data_ptr(), c, hw, out.data_ptr(), ws.data_ptr(), wsb,
                                             hip.stream_ptr()), "msl_maxsquare_prob_fwd")
        ctx.save_for_backward(prob)
        return out

    @staticmethod
    def backward(ctx, g):
        (prob,) = ctx.saved_tensors
        c, hw = prob.size(1), prob.size(2) * prob.size(3)
        g = g.to(_f32).contiguous()
        d = torch.empty_like(prob)
        hip.check(hip.load().msl_maxsquare_prob_bwd(prob.data_ptr(), c, hw, g.data_ptr(), d.data_ptr(),
                                                    hip.stream_ptr()), "msl_maxsquare_prob_bwd")
        return d


class _IWMaxSquareProb(Function):
    @staticmethod
    def forward(ctx, prob, label, ratio):
        prob = _check_act(prob, "iw_maxsquare_prob")
        c, hw = prob.size(1), prob.size(2) * prob.size(3)
        if label is not None:
            label = label.contiguous()
            if label.dtype != torch.int64 or label.numel() != hw:
                raise hip.MSLError("iw_maxsquare_prob: label must be int64 (N,H,W) with N=1")
        lib = hip.load()
        out = torch.empty((), dtype=_f32, device=prob.device)
        hist, weights = _iw_outputs(c, prob.device)
        wsb = lib.msl_loss_workspace(c, 1, 1, 1, hw)
        ws = hip.workspace(wsb, prob.device)
        hip.check(lib.msl_iw_maxsquare_prob_fwd(prob.data_ptr(), hip.ptr(label), c, hw, float(ratio),
                                                out.data_ptr(), hist.data_ptr(), weights.data_ptr(),
                                                ws.data_ptr(), wsb, hip.stream_ptr()), "msl_iw_maxsquare_prob_fwd")
        ctx.save_for_backward(prob, weights)
        ctx.mark_non_differentiable(hist, weights)
        return out, hist, weights

    @staticmethod
    def backward(ctx, g, _gh, _gw):
        prob, weights = ctx.saved_tensors
        c, hw = prob.size(1), prob.size(2) * prob.size(3)
        g = g.to(_f32).contiguous()
        d = torch.empty_like(prob)
        hip.check(hip.load().msl_iw_maxsquare_prob_bwd(prob.data_ptr(), c, hw, weights.data_ptr(), g.data_ptr(),
                                                       d.data_ptr(), hip.stream_ptr()), "msl_iw_maxsquare_prob_bwd")
        return d, None, None


def maxsquare_prob(prob):
    return _MaxSquareProb.apply(prob)


def iw_maxsquare_prob(prob, label, ratio):
    return _IWMaxSquareProb.apply(prob, label, float(ratio))


# --------------------------------------------------------------------------- batch norm (+ReLU, +residual)
# r05: the residual BN + ReLU (each bottleneck's bn3, deeplab_multi.py:45-47) keeps its ReLU mask as bits
# for the backward (msl_bn_fwd_mask / msl_bn_bwd_mask) instead of re-reading the block output; the same
# mask bit for bit (tests/test_gpu_ops.py test_bn_relu_mask_bits).  False: the backward reads y.
BN_MASK_BITS = True
RESMASK_DGRAD = True  # r06: MaskedResidual instead of bn3 writing the residual gradient


class _BNAct(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, running_mean, running_var, num_batches, training, momentum,
                eps, relu, hold=None):
        ctx.fm = hip.snapshot_forms()  # the backward runs the forms of its forward
        x = _check_act(x, "bn_act", images=True)
        n = _nimg(x)
        c, p = x.size(1), x.size(-2) * x.size(-1)  # p: pixels of one image
        if residual is not None:
            residual = residual.contiguous()
            if residual.shape != x.shape:
                raise hip.MSLError("bn_act: residual shape mismatch")
        lib = hip.load()
        y = torch.empty_like(x)
        save_mean = torch.empty(c * n, dtype=_f32, device=x.device)
        save_invstd = torch.empty(c * n, dtype=_f32, device=x.device)
        wsb = lib.msl_bn_workspace(c, p, n)
        ws = hip.workspace(wsb, x.device)
        update = bool(training) and running_mean is not None
        # f16x3 / fp16: the per-channel absmax of y for the convs that read it (their operand scales):
        # from registers in the fused kernel, folded into the flat apply otherwise (r05: the big layer1
        # maps of configs 4 / 5 no longer pay a pass of their own)
        fused = bool(lib.msl_bn_uses_fused(c, p, int(bool(training)), hip.forms()))
        am = torch.empty(c, dtype=_f32, device=x.device) if _h3(CONV_MATH) else None
        # r05: a residual BN + ReLU under the fused kernels writes the ReLU mask as bits (msl_bn_fwd_mask),
        # so its backward reads 1 bit per pixel instead of y (msl_bn_bwd_mask)
        # (only for a backward: under torch.no_grad() - the evaluator - no input needs a gradient and
        # the bits would be written for nobody)
        bits = None
        if relu and residual is not None and fused and BN_MASK_BITS and any(ctx.needs_input_grad):
            bits = torch.empty(lib.msl_bn_relu_mask_bytes(c, p, n) // 8, dtype=torch.int64, device=x.device)
        hip.check(lib.msl_bn_fwd_mask(x.data_ptr(), hip.ptr(weight), hip.ptr(bias), hip.ptr(residual), y.data_ptr(),
                                      hip.ptr(running_mean), hip.ptr(running_var), hip.ptr(num_batches),
                                      save_mean.data_ptr(), save_invstd.data_ptr(), c, p, n, int(bool(training)),
                                      int(update), float(momentum), float(eps), int(bool(relu)), hip.forms(),
                                      ws.data_ptr(), wsb, hip.stream_ptr(), hip.ptr(am), hip.ptr(bits)), "msl_bn_fwd")
        if am is not None:
            _tag_absmax(y, am)
        # ReLU without a residual under the fused kernels (p <= 16384): the backward recomputes the
        # mask from x (msl_bn_bwd_am_beta, y = NULL) instead of reading y
        remask = (bool(relu) and residual is None and p <= 16384 and fused)
        ctx.bits = bits
        ctx.save_for_backward(x, weight, y if (relu and not remask and bits is None) else None, save_mean,
                              save_invstd)
        ctx.bias = bias
        ctx.meta = (c, p, n, bool(training), bool(relu))
        ctx.hold = hold
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, y, save_mean, save_invstd = ctx.saved_tensors
        c, p, n, training, relu = ctx.meta
        gy = gy.contiguous()
        lib = hip.load()
        nig = ctx.needs_input_grad
        dx = torch.empty_like(x) if nig[0] else None
        hold = ctx.hold
        # r06: an identity block's residual gradient stays unmaterialised (MaskedResidual) when conv1's
        # data-gradient form has the masked epilogue
        lazy = (hold is not None and not nig[3] and ctx.bits is not None and RESMASK_DGRAD and
                CONV_MATH != "bf16" and hasattr(lib, "msl_pconv_dgrad_resmask_sc"))
        dres = torch.empty_like(x) if (nig[3] or (hold is not None and not lazy)) else None
        sw = grad_sink(weight) if nig[1] else None
        sb = grad_sink(ctx.bias) if nig[2] else None
        direct = sw is not None and sb is not None
        if direct:
            dgamma, dbeta = sw[0], sb[0]
        else:
            dgamma = torch.empty(c, dtype=_f32, device=x.device) if nig[1] else None
            dbeta = torch.empty(c, dtype=_f32, device=x.device) if nig[2] else None
        wsb = lib.msl_bn_workspace(c, p, n)
        ws = hip.workspace(wsb, x.device)
        # f16x3 / fp16: the per-channel absmax of dx, the gradient the conv before this BN reads twice
        am = torch.empty(c, dtype=_f32, device=x.device) if (dx is not None and _h3(CONV_MATH)) else None
        if ctx.bits is not None:
            st = lib.msl_bn_bwd_mask(gy.data_ptr(), x.data_ptr(), ctx.bits.data_ptr(), hip.ptr(weight),
                                     hip.ptr(ctx.bias), save_mean.data_ptr(), save_invstd.data_ptr(), hip.ptr(dx),
                                     hip.ptr(dres), hip.ptr(dgamma), hip.ptr(dbeta), c, p, n, int(training), int(relu),
                                     int(direct), ctypes.addressof(ctx.fm), ws.data_ptr(), wsb, hip.stream_ptr(), hip.ptr(am))
        else:
            st = lib.msl_bn_bwd_am_beta(gy.data_ptr(), x.data_ptr(), hip.ptr(y), hip.ptr(weight),
                                        hip.ptr(ctx.bias), save_mean.data_ptr(), save_invstd.data_ptr(),
                                        hip.ptr(dx), hip.ptr(dres), hip.ptr(dgamma), hip.ptr(dbeta), c, p, n,
                                        int(training), int(relu), int(direct), ctypes.addressof(ctx.fm), ws.data_ptr(), wsb,
                                        hip.stream_ptr(), hip.ptr(am))
        hip.check(st, "msl_bn_bwd")
        if am is not None:
            _tag_absmax(dx, am)
        if direct:
            sw[1].notify(sw[2])
            sb[1].notify(sb[2])
            dgamma = dbeta = None
        if hold is not None:  # handed to the block's conv1 backward (ResidualGrad)
            hold.g = MaskedResidual(gy, ctx.bits, n) if lazy else dres
            dres = None
        return dx, dgamma, dbeta, dres, None, None, None, None, None, None, None, None


def bn_act(bn, x, residual=None, relu=False, residual_grad=None):
    """act(bn(x) [+ residual]) for an nn.BatchNorm2d `bn` (train mode: batch statistics, bs = 1).
    With `residual_grad` (ResidualGrad) the residual's gradient goes to that holder instead of
    autograd (pass the residual detached; the conv that shares its input adds it)."""
    training = bn.training or not bn.track_running_stats
    momentum = 0.1 if bn.momentum is None else bn.momentum
    return _BNAct.apply(x, bn.weight, bn.bias, residual, bn.running_mean, bn.running_var,
                        bn.num_batches_tracked if training else None, training, momentum, bn.eps, relu,
                        residual_grad)


# --------------------------------------------------------------------------- AdaIN style pass (csrc/style.hip)
# Forward only, no autograd: the style network runs under no_grad in the reference too
# (utils/style_transform.py).  A "grid" is a stage's input with its reflected border, (1, C, H+2, W+2);
# the kernels read a grid's interior or a plain (1, C, H, W) tensor (include/msl_hip.h).
STYLE_ACT = {"none": 0, "relu": 1, "relu_in": 2}
STYLE_RESAMPLE = {"none": 0, "pool": 1, "up": 2}


def _style_src(x, grid, name):
    """(contiguous x, C, H, W) of a plain (1,C,H,W) tensor or, with `grid`, of a grid's interior."""
    if not (x.is_cuda and x.dtype == _f32 and x.dim() == 4 and x.size(0) == 1):
        raise hip.MSLError(f"{name}: expected a CUDA fp32 tensor of shape (1,C,H,W), got {tuple(x.shape)} {x.dtype} "
                           f"{x.device}")
    pad = 2 if grid else 0
    return x.contiguous(), x.size(1), x.size(2) - pad, x.size(3) - pad


def style_out_hw(h, w, resample):
    """The interior size of style_pad's output grid."""
    if resample == "pool":
        return (h + 1) // 2, (w + 1) // 2
    return (2 * h, 2 * w) if resample == "up" else (h, w)


def style_pad(x, grid=False, act="none", resample="none", a=None, b=None, cpad=None):
    """reflect_pad1(resample(f(x))) as a grid (1, cpad, H'+2, W'+2): msl_style_pad, one launch.  act "relu"
    applies after the per-channel affine a, b (device tensors of C floats, or both None), "relu_in" before."""
    x, c, h, w = _style_src(x, grid, "style_pad")
    cpad = c if cpad is None else int(cpad)
    ho, wo = style_out_hw(h, w, resample)
    y = torch.empty((1, cpad, ho + 2, wo + 2), dtype=_f32, device=x.device)
    if a is not None:
        a, b = a.contiguous(), b.contiguous()
        if a.numel() != c or b.numel() != c or a.dtype != _f32 or b.dtype != _f32:
            raise hip.MSLError(f"style_pad: the affine needs two fp32 tensors of {c} elements")
    hip.check(hip.load().msl_style_pad(x.data_ptr(), int(bool(grid)), c, h, w, STYLE_ACT[act], STYLE_RESAMPLE[resample],
                                       hip.ptr(a), hip.ptr(b), y.data_ptr(), cpad, hip.stream_ptr()), "msl_style_pad")
    return y


def style_input(img, w1, b1, cpad=3):
    """The encoder's first grid (1, cpad, H+2, W+2) from a uint8 (H, W, 3) RGB image (divided by 255) or a
    float (1, 3, H, W) tensor in [0, 1], through the leading 1x1 conv (w1 (3,3,1,1), b1 (3,)): msl_style_input."""
    if img.dtype == torch.uint8:
        ok, h, w = img.dim() == 3 and img.size(2) == 3, img.size(0), img.size(1)
    else:
        ok, h, w = img.dtype == _f32 and img.dim() == 4 and tuple(img.shape[:2]) == (1, 3), img.size(-2), img.size(-1)
    if not (ok and img.is_cuda):
        raise hip.MSLError(f"style_input: expected a CUDA uint8 (H,W,3) or fp32 (1,3,H,W) image, got "
                           f"{tuple(img.shape)} {img.dtype} {img.device}")
    img, w1, b1 = img.contiguous(), w1.contiguous(), b1.contiguous()
    if w1.numel() != 9 or b1.numel() != 3 or w1.dtype != _f32 or b1.dtype != _f32:
        raise hip.MSLError("style_input: the 1x1 conv needs a (3,3,1,1) weight and a (3,) bias in fp32")
    y = torch.empty((1, cpad, h + 2, w + 2), dtype=_f32, device=img.device)
    u8 = img.dtype == torch.uint8
    hip.check(hip.load().msl_style_input(img.data_ptr() if u8 else None, None if u8 else img.data_ptr(), h, w,
                                         w1.data_ptr(), b1.data_ptr(), y.data_ptr(), cpad, hip.stream_ptr()),
              "msl_style_input")
    return y


def style_stats(x, grid=False, relu=True):
    """(2, C): the per-channel mean and unbiased variance of x (of relu(x) with `relu`): msl_style_stats."""
    x, c, h, w = _style_src(x, grid, "style_stats")
    lib = hip.load()
    stats = torch.empty((2, c), dtype=_f32, device=x.device)
    wsb = lib.msl_style_stats_workspace(c, h, w)
    ws = hip.workspace(wsb, x.device)
    hip.check(lib.msl_style_stats(x.data_ptr(), int(bool(grid)), c, h, w, int(bool(relu)), stats.data_ptr(),
                                  ws.data_ptr(), wsb, hip.stream_ptr()), "msl_style_stats")
    return stats


def style_adain_coef(content_stats, style_stats_, weights=(1.0,), alpha=1.0, eps=1e-5):
    """The AdaIN affine (a, b) of C floats each, from content statistics (2, C) and S style statistics
    (S, 2, C) weighted by `weights`: msl_style_adain_coef, no host sync."""
    c = content_stats.size(-1)
    s = len(weights)
    if tuple(content_stats.shape) != (2, c) or tuple(style_stats_.shape) != (s, 2, c):
        raise hip.MSLError(f"style_adain_coef: statistics {tuple(content_stats.shape)} / {tuple(style_stats_.shape)} "
                           f"do not match {s} weights")
    content_stats, style_stats_ = content_stats.contiguous(), style_stats_.contiguous()
    wt = (ctypes.c_float * s)(*[float(v) for v in weights])
    ab = torch.empty((2, c), dtype=_f32, device=content_stats.device)
    hip.check(hip.load().msl_style_adain_coef(content_stats.data_ptr(), style_stats_.data_ptr(),
                                              ctypes.addressof(wt), s, c, float(alpha), float(eps), ab[0].data_ptr(),
                                              ab[1].data_ptr(), hip.stream_ptr()), "msl_style_adain_coef")
    return ab[0], ab[1]


def style_output(x, grid=False, rgb=True, seg=False, mean=(0.0, 0.0, 0.0)):
    """(uint8 (H, W, 3) RGB or None, fp32 (1, 3, H, W) BGR - mean or None) of a 3-channel map in [0, 1]:
    msl_style_output; `mean` in B, G, R order."""
    x, c, h, w = _style_src(x, grid, "style_output")
    if c != 3 or not (rgb or seg):
        raise hip.MSLError(f"style_output: expected 3 channels and at least one output, got {c} channels")
    u8 = torch.empty((h, w, 3), dtype=torch.uint8, device=x.device) if rgb else None
    sg = torch.empty((1, 3, h, w), dtype=_f32, device=x.device) if seg else None
    hip.check(hip.load().msl_style_output(x.data_ptr(), int(bool(grid)), h, w, hip.ptr(u8), hip.ptr(sg), float(mean[0]),
                                          float(mean[1]), float(mean[2]), hip.stream_ptr()), "msl_style_output")
    return u8, sg


def style_input_window(img, window, size, w1, b1, cpad=3):
    """style_input of the window (x0, y0, cw, ch) of `img` magnified to size = (h, w) by torch's nearest rule
    (F.interpolate's default): msl_style_input_window, one launch, the magnified image never written."""
    if img.dtype == torch.uint8:
        ok, ih, iw = img.dim() == 3 and img.size(2) == 3, img.size(0), img.size(1)
    else:
        ok, ih, iw = img.dtype == _f32 and img.dim() == 4 and tuple(img.shape[:2]) == (1, 3), img.size(-2), img.size(-1)
    if not (ok and img.is_cuda):
        raise hip.MSLError(f"style_input_window: expected a CUDA uint8 (H,W,3) or fp32 (1,3,H,W) image, got "
                           f"{tuple(img.shape)} {img.dtype} {img.device}")
    img, w1, b1 = img.contiguous(), w1.contiguous(), b1.contiguous()
    if w1.numel() != 9 or b1.numel() != 3 or w1.dtype != _f32 or b1.dtype != _f32:
        raise hip.MSLError("style_input_window: the 1x1 conv needs a (3,3,1,1) weight and a (3,) bias in fp32")
    x0, y0, cw, ch = (int(v) for v in window)
    h, w = int(size[0]), int(size[1])
    if h < 1 or w < 1:
        raise hip.MSLError(f"style_input_window: size {size}")
    y = torch.empty((1, cpad, h + 2, w + 2), dtype=_f32, device=img.device)
    u8 = img.dtype == torch.uint8
    hip.check(hip.load().msl_style_input_window(img.data_ptr() if u8 else None, None if u8 else img.data_ptr(), ih, iw,
                                                x0, y0, cw, ch, h, w, w1.data_ptr(), b1.data_ptr(), y.data_ptr(), cpad,
                                                hip.stream_ptr()), "msl_style_input_window")
    return y


def style_output_resampled(x, out, window=None, grid=False, mid=None, full=None, off=(0, 0), mean=(0.0, 0.0, 0.0)):
    """style_output's seg tensor of the 3-channel map x, gathered by torch's nearest rule into the window
    (dx0, dy0, dw, dh) of `out` (1, 3, Hd, Wd), in place: msl_style_output_resampled.  One map (full None): the
    window is x resized to (dh, dw).  Two maps: x resized to mid = (mh, mw) sits at off = (oy, ox) of a
    stitched map of full = (fh, fw), which is resized to (Hd, Wd); only the cells of the window whose
    source is this image's part are written.  `window` defaults to the whole of `out`."""
    x, c, h, w = _style_src(x, grid, "style_output_resampled")
    if c != 3:
        raise hip.MSLError(f"style_output_resampled: expected 3 channels, got {c}")
    if not (out.is_cuda and out.dtype == _f32 and out.dim() == 4 and tuple(out.shape[:2]) == (1, 3) and
            out.is_contiguous() and out.device == x.device):
        raise hip.MSLError(f"style_output_resampled: out must be a contiguous CUDA fp32 (1,3,H,W) tensor, got "
                           f"{tuple(out.shape)} {out.dtype}")
    hd, wd = out.size(2), out.size(3)
    dx0, dy0, dw, dh = (0, 0, wd, hd) if window is None else (int(v) for v in window)
    if full is None:
        mh, mw, fh, fw = dh, dw, 0, 0
    else:
        (mh, mw), (fh, fw) = (int(v) for v in mid), (int(v) for v in full)
    hip.check(hip.load().msl_style_output_resampled(x.data_ptr(), int(bool(grid)), h, w, mh, mw, fh, fw, int(off[0]),
                                                    int(off[1]), out.data_ptr(), hd, wd, dx0, dy0, dw, dh,
                                                    float(mean[0]), float(mean[1]), float(mean[2]), hip.stream_ptr()),
              "msl_style_output_resampled")
    return out


def label_resize_nearest(label, size):
    """An int64 (H, W) label map resized to size = (ho, wo) by torch's nearest rule: msl_label_resize_nearest."""
    if not (label.is_cuda and label.dtype == torch.int64 and label.dim() == 2):
        raise hip.MSLError(f"label_resize_nearest: expected a CUDA int64 (H,W) map, got {tuple(label.shape)} "
                           f"{label.dtype} {label.device}")
    label = label.contiguous()
    ho, wo = int(size[0]), int(size[1])
    if ho < 1 or wo < 1:
        raise hip.MSLError(f"label_resize_nearest: size {size}")
    out = torch.empty((ho, wo), dtype=torch.int64, device=label.device)
    hip.check(hip.load().msl_label_resize_nearest(label.data_ptr(), label.size(0), label.size(1), out.data_ptr(), ho, wo,
                                                  hip.stream_ptr()), "msl_label_resize_nearest")
    return out


def conv3x3_reflect(x_grid, weight, bias, cache):
    """The reference's ReflectionPad2d(1) + Conv2d(cin, cout, 3) on a grid (1, cin, H+2, W+2) that already
    holds the reflected border: msl_dconv_fwd (one branch, dilation 1, zero padding) over the whole grid.
    Returns (1, cout, H+2, W+2), of which only the interior is the conv's output (the border cells also
    read the zero padding: finite, never to be read).  Forward only."""
    x, cin, h, w = _style_src(x_grid, False, "conv3x3_reflect")
    cout = weight.size(0)
    if tuple(weight.shape) != (cout, cin, 3, 3) or (bias is not None and bias.numel() != cout):
        raise hip.MSLError(f"conv3x3_reflect: weight {tuple(weight.shape)} does not match input {tuple(x.shape)}")
    lib = hip.load()
    packed = cache.get([weight], cin, cout, 0)
    y = torch.empty((1, cout, h, w), dtype=_f32, device=x.device)
    wsb = lib.msl_dconv_fwd_workspace(1, cin, cout, h, w, 1)
    ws = hip.workspace(wsb, x.device)
    math = CONV_MATH
    xpart = _parts(x, math, compute=_split_gemm(cout, cin))
    hip.check(_conv_call(lib, "msl_dconv_fwd", math,
                         (x.data_ptr(), packed.data_ptr(), hip.ptr(None if bias is None else bias.detach().contiguous()),
                          y.data_ptr(), 1, cin, cout, h, w, 1, 1, 0, hip.forms(), ws.data_ptr(), wsb, hip.stream_ptr()),
                         (xpart,)), "msl_dconv_fwd")
    return y
