"""SGD and Adam with the reference's optimizer semantics, one fused HIP step each.

The reference builds `torch.optim.SGD(params=model.optim_parameters(args),
lr, momentum, weight_decay)` (train_source.py:139-144) from two generator
groups, the first of which lists most backbone parameters 3 or 4 times
(deeplab_multi.py:139-154).  torch's single-tensor SGD
then applies k sequential updates to such a parameter, sharing its momentum
buffer, except that on its first step every occurrence starts a fresh buffer
(the last one is kept).  `SGD` reproduces exactly that, for all parameters of
the model, in a single `msl_sgd_step` launch.

Gradients live in one flat buffer (`FlatGrads`): `param.grad` is a view into
it, `zero_grad()` is one memset, and the data-parallel reducer all-reduces it
in buckets.  A parameter counts as having a gradient this step only if
autograd accumulated into it (post-accumulate-grad hook), so parameters the
reference would leave at `grad=None` (the dead ASPP branches, quirk Q1) are
still skipped, weight decay included.

`--optim Adam` (train_source.py:145-146) is `Adam`: torch's single-tensor
Adam over the same lists, where the k entries of a duplicated parameter share
exp_avg, exp_avg_sq and the step counter (which advances by k), as
`msl_adam_step`: a one-thread-per-parameter launch that reads and advances the
counters on the device, then one launch over every element.
"""
import numpy as np
import torch

from .. import hip

# msl_sgd_entry / msl_adam_entry of include/msl_hip.h
_ENTRY_SGD = np.dtype([("param", "<u8"), ("grad", "<u8"), ("momentum", "<u8"), ("numel", "<i8"),
                       ("mult", "<i4"), ("group", "<i4"), ("has_buf", "<i4"), ("pad", "<i4")])
assert _ENTRY_SGD.itemsize == 48
_ENTRY_ADAM = np.dtype([("param", "<u8"), ("grad", "<u8"), ("exp_avg", "<u8"), ("exp_avg_sq", "<u8"),
                        ("step", "<u8"), ("numel", "<i8"), ("mult", "<i4"), ("group", "<i4")])
assert _ENTRY_ADAM.itemsize == 56


def unique_with_multiplicity(params):
    """[(param, k)] in first-occurrence order; k = number of occurrences (identity)."""
    order, count = [], {}
    for p in params:
        if id(p) not in count:
            count[id(p)] = 0
            order.append(p)
        count[id(p)] += 1
    return [(p, count[id(p)]) for p in order]


class FlatGrads:
    """One flat fp32 gradient buffer; every trainable parameter's .grad is a view of it.

    Parameters are laid out in reverse registration order (the order the
    backward pass produces their gradients), so that contiguous slices of the
    buffer become complete early and can be all-reduced while the backward
    still runs (see utils/dist.py).
    """

    def __init__(self, params, device):
        self.params = list(params)[::-1]
        self.index = {id(p): i for i, p in enumerate(self.params)}
        sizes = [p.numel() for p in self.params]
        self.offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.numel = int(self.offsets[-1])
        self.flat = torch.zeros(self.numel, dtype=torch.float32, device=device)
        self.used = np.zeros(len(self.params), dtype=bool)
        self.listeners = []
        self.gen = 1                                      # backward-pass generation
        self.seen = np.zeros(len(self.params), dtype=np.int64)
        for i, p in enumerate(self.params):
            p.grad = self.flat[self.offsets[i]:self.offsets[i + 1]].view_as(p)
            p.register_post_accumulate_grad_hook(self._make_hook(i))
            # lets the HIP ops accumulate this parameter's gradient in place (ops.grad_sink)
            p._msl_flat = (self, i)

    def _make_hook(self, i):
        def hook(_p):
            self.notify(i)
        return hook

    def notify(self, i):
        """Parameter i's gradient for this backward is complete (AccumulateGrad's hook, or a
        HIP op that accumulated it directly into the flat buffer).  Listeners hear it once per
        backward pass: when an op has accumulated in place and returned None for the parameter,
        autograd still runs the AccumulateGrad node and fires its post-accumulate hook - a second
        report that would count a bucket down before its other parameters are final."""
        self.used[i] = True
        if self.seen[i] == self.gen:
            return
        self.seen[i] = self.gen
        for fn in self.listeners:
            fn(i)

    def new_backward(self):
        """The next reports belong to a new backward pass."""
        self.gen += 1

    def view(self, i):
        return self.flat[self.offsets[i]:self.offsets[i + 1]]

    def zero_(self):
        from .. import ops
        ops.wgrad_join(self.flat.device)  # weight gradients still being accumulated on the side stream
        self.flat.zero_()
        self.used[:] = False
        self.new_backward()

    def reattach(self):
        """Restore the .grad views (e.g. after someone set grads to None)."""
        for i, p in enumerate(self.params):
            if p.grad is None or p.grad.data_ptr() != self.flat.data_ptr() + 4 * int(self.offsets[i]):
                p.grad = self.flat[self.offsets[i]:self.offsets[i + 1]].view_as(p)


class _FlatOptimizer:
    """What SGD and Adam share: the reference's (at most two) parameter groups with their duplicated
    lists (Q2), the flat gradient buffer, and the device launch table - entries of the live
    parameters plus the block plan of msl_sgd_plan - rebuilt only when its key changes and never
    inside a hipGraph capture.  A subclass names its entry layout (`_ENTRY`) and lists the live
    rows (`_build_table`)."""

    _ENTRY = None

    def _init_groups(self, params, defaults):
        if isinstance(params, torch.Tensor):
            raise TypeError("params must be an iterable of tensors or dicts")
        groups = list(params)
        if groups and not isinstance(groups[0], dict):
            groups = [{"params": groups}]
        self.defaults = defaults
        self.param_groups = []
        for g in groups:
            plist = list(g["params"])
            pg = dict(self.defaults)
            pg.update({k: v for k, v in g.items() if k != "params"})
            pg["params"] = plist
            pg["_unique"] = unique_with_multiplicity(plist)
            self.param_groups.append(pg)
        if len(self.param_groups) > 2:
            raise NotImplementedError("at most two parameter groups (backbone, heads)")
        self.state = {}  # param -> its state tensors
        uniq, seen = [], set()
        for g in self.param_groups:
            for p, _ in g["_unique"]:
                if id(p) in seen:
                    raise NotImplementedError("a parameter in two groups")
                seen.add(id(p))
                if p.requires_grad:
                    uniq.append(p)
        self._uniq = uniq
        self.device = uniq[0].device if uniq else torch.device("cpu")
        self.grads = FlatGrads(uniq, self.device)
        self._table_key = None
        self._table = None
        self._last_used = None
        self.grad_scale = 1.0
        self.lr_dev = None  # device float32[2] learning rates (hipGraph replay), else by value

    # -- torch.optim.Optimizer surface ------------------------------------------------
    def zero_grad(self, set_to_none=True):
        """Gradients restart at zero (the flat buffer is cleared; views stay attached)."""
        self.grads.reattach()
        self.grads.zero_()

    def _live(self):
        """(group index, parameter, multiplicity) of every parameter that has a gradient this step;
        the others are `grad is None` in the reference: skipped entirely."""
        grads = self.grads
        for gi, g in enumerate(self.param_groups):
            for p, k in g["_unique"]:
                if p.requires_grad and grads.used[grads.index[id(p)]]:
                    yield gi, p, k

    def _with_used(self, used, fn):
        saved = self.grads.used.copy()
        self.grads.used[:] = used
        try:
            fn()
        finally:
            self.grads.used[:] = saved

    def _ensure_table(self):
        lib = hip.load()
        rows, key = self._build_table()
        if key != self._table_key:
            if torch.cuda.is_current_stream_capturing():
                raise hip.MSLError(f"{type(self).__name__}: the launch table changed inside a hipGraph capture; "
                                   "call optimizer.prepare() before capturing")
            ent = np.zeros(len(rows), dtype=self._ENTRY)
            for j, r in enumerate(rows):
                ent[j] = r
            numels = ent["numel"].astype(np.int64)
            be = lib.msl_sgd_block_elems()
            nblk_each = (numels + be - 1) // be
            block_entry = np.repeat(np.arange(len(rows), dtype=np.int32), nblk_each)
            starts = np.concatenate([[0], np.cumsum(nblk_each)[:-1]]).astype(np.int64)
            block_offset = (np.arange(int(nblk_each.sum()), dtype=np.int64) - np.repeat(starts, nblk_each)) * be
            blob = np.concatenate([ent.view(np.uint8), block_entry.view(np.uint8), block_offset.view(np.uint8)])
            dev = torch.from_numpy(blob).to(self.device)
            n_ent = ent.nbytes
            n_be = block_entry.nbytes
            self._table = (dev, dev.data_ptr(), dev.data_ptr() + n_ent, dev.data_ptr() + n_ent + n_be,
                           int(nblk_each.sum()))
            self._table_rows = len(rows)
            self._table_key = key

    def _before_step(self, what):
        if self.device.type != "cuda":
            raise hip.MSLError(f"{what} runs on the HIP path only (no CPU fallback)")
        from .. import ops
        ops.wgrad_join(self.device)  # the weight gradients accumulated on the side stream (ops.ASYNC_WGRAD)
        self._ensure_table()
        self._last_used = self.grads.used.copy()

    def _bump_versions(self):
        # the kernel wrote the parameters behind autograd's back: bump their version counters
        for _, p, _ in self._live():
            torch.autograd.graph.increment_version(p)

    def group_lrs(self):
        lr0 = float(self.param_groups[0]["lr"])
        return lr0, (float(self.param_groups[1]["lr"]) if len(self.param_groups) > 1 else lr0)

    def _packed_groups(self):
        """torch.optim.Optimizer.state_dict's numbering: list positions counted across the groups,
        every occurrence of a duplicated parameter (Q2) mapped to one position.  Returns
        ({id(param): position}, the groups with `params` as positions)."""
        first, start, groups = {}, 0, []
        for g in self.param_groups:
            # torch's pack_group: one dict comprehension per group, so inside a group the LAST
            # position of a duplicated tensor wins; a tensor seen in an earlier group keeps that one
            first.update({id(p): i for i, p in enumerate(g["params"], start) if id(p) not in first})
            pg = {k: v for k, v in g.items() if k not in ("params", "_unique")}
            pg["params"] = [first[id(p)] for p in g["params"]]
            start += len(g["params"])
            groups.append(pg)
        return first, groups


class SGD(_FlatOptimizer):
    """torch.optim.SGD(params, lr, momentum, weight_decay) for the reference's groups (no nesterov,
    no dampening) - drop-in for train_source.py:139-144."""

    _ENTRY = _ENTRY_SGD

    def __init__(self, params, lr, momentum=0.0, weight_decay=0.0, dampening=0.0, nesterov=False):
        if dampening != 0 or nesterov:
            raise NotImplementedError("the reference uses dampening=0, nesterov=False")
        self._init_groups(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay, dampening=0.0,
                                       nesterov=False))
        # state: param -> {"momentum_buffer": tensor}

    def _build_table(self):
        mom = self.defaults["momentum"]
        rows, key = [], []
        for gi, p, k in self._live():
            st = self.state.setdefault(p, {})
            has_buf = "momentum_buffer" in st
            if not has_buf:
                st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            buf = st["momentum_buffer"]
            rows.append((p.data_ptr(), p.grad.data_ptr(), buf.data_ptr(), p.numel(), k, gi,
                         int(has_buf and mom != 0), 0))
            key.append((rows[-1][0], rows[-1][1], rows[-1][2], rows[-1][6]))
        return rows, tuple(key)

    def prepare(self, used=None):
        """Build (and upload) the launch table for the given live-parameter mask now, creating the
        momentum buffers it needs - so a step captured into a hipGraph afterwards finds it ready
        (no host-to-device copy and no allocation may happen inside the capture).  `used`
        defaults to the parameters that received gradients in the last step."""
        if self._last_used is None:
            raise hip.MSLError("SGD.prepare(): run one step first (its first-step buffer rule, Q2, differs)")
        self._with_used(self._last_used if used is None else used, self._ensure_table)

    def step(self, closure=None):
        if closure is not None:
            raise NotImplementedError("closure")
        self._before_step("SGD.step")
        lib = hip.load()
        _dev, p_ent, p_be, p_bo, nblocks = self._table
        mom = float(self.defaults["momentum"])
        wd = float(self.defaults["weight_decay"])
        # momentum == 0: buffers are written but has_buf stays 0, i.e. buf = d, p -= lr*d
        if self.lr_dev is not None:
            # learning rates from device memory (set between hipGraph replays, utils/graph.py)
            hip.check(lib.msl_sgd_step_lr_dev(p_ent, p_be, p_bo, nblocks, self.lr_dev.data_ptr(), mom, wd,
                                              float(self.grad_scale), hip.stream_ptr()), "msl_sgd_step_lr_dev")
        else:
            lr0, lr1 = self.group_lrs()
            hip.check(lib.msl_sgd_step(p_ent, p_be, p_bo, nblocks, lr0, lr1, mom, wd, float(self.grad_scale),
                                       hip.stream_ptr()), "msl_sgd_step")
        self._bump_versions()
        return None

    # -- checkpoints (train_source.py:662-704 stores optimizer.state_dict()) -----------
    def state_dict(self):
        """torch.optim.Optimizer.state_dict's format: list positions numbered across the groups,
        every occurrence of a duplicated parameter (Q2) mapped to one position, and one
        momentum buffer per tensor under that index - what the reference's torch.optim.SGD writes
        into its checkpoints (train_source.py:672-674)."""
        first, groups = self._packed_groups()
        state = {}
        for g in self.param_groups:
            for p, _ in g["_unique"]:
                st = self.state.get(p)
                if st is not None and "momentum_buffer" in st:
                    state[first[id(p)]] = {"momentum_buffer": st["momentum_buffer"].detach().clone()}
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        """Accepts this class's and torch.optim.SGD's state dicts (same format)."""
        flat = [p for g in self.param_groups for p in g["params"]]
        for i, s in sd["state"].items():
            p = flat[int(i)]
            if "momentum_buffer" in s:
                self.state.setdefault(p, {})["momentum_buffer"] = s["momentum_buffer"].to(p.device).clone()
        for g, sg in zip(self.param_groups, sd["param_groups"]):
            for k, v in sg.items():
                if k in ("lr", "momentum", "weight_decay"):
                    g[k] = v
        self._table_key = None


class Adam(_FlatOptimizer):
    """torch.optim.Adam(params, lr, betas, eps, weight_decay) for the reference's groups
    (amsgrad=False, L2 weight decay) - drop-in for train_source.py:145-146.

    state[p] = {"step", "exp_avg", "exp_avg_sq"}, created as zeros the first time p has a gradient.
    `step` is a 0-dim fp32 view into one device array of the optimizer (`_steps`): the kernel
    advances it there - also under hipGraph replay, with no host write - and the host reads the
    same memory.  A parameter listed k times advances by k per step()."""

    _ENTRY = _ENTRY_ADAM
    _UNSUPPORTED = ("maximize", "foreach", "capturable", "fused", "decoupled_weight_decay", "differentiable")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, **kw):
        if amsgrad:
            raise NotImplementedError("amsgrad=True (the reference uses amsgrad=False)")
        for k, v in kw.items():
            if k not in self._UNSUPPORTED:
                raise TypeError(f"Adam: unexpected argument {k!r}")
            if v:
                raise NotImplementedError(f"{k}={v!r}: one implementation, the fused HIP step with L2 weight decay")
        # every key torch.optim.Adam of the installed torch keeps in a group (it also validates the values)
        defaults = dict(torch.optim.Adam([torch.zeros(1)], lr=lr, betas=tuple(betas), eps=eps,
                                         weight_decay=weight_decay, amsgrad=False).defaults)
        self._init_groups(params, defaults)
        kmax = hip.load(require_gpu=False).msl_adam_max_mult()  # rows of an entry's coefficient table
        for g in self.param_groups:
            if any(k > kmax for _, k in g["_unique"]):
                raise NotImplementedError(f"a parameter listed more than {kmax} times in a group")
        self._steps = torch.zeros(max(len(self._uniq), 1), dtype=torch.float32, device=self.device)
        self._step_of = {id(p): i for i, p in enumerate(self._uniq)}
        self._coef = None

    def init_state(self, p):
        """p's state, created as zeros with step 0 if it has none yet (torch creates it the first
        time p has a gradient)."""
        st = self.state.get(p)
        if st is None:
            i = self._step_of[id(p)]
            self._steps[i] = 0
            st = self.state[p] = {"step": self._steps[i],
                                  "exp_avg": torch.zeros_like(p, memory_format=torch.contiguous_format),
                                  "exp_avg_sq": torch.zeros_like(p, memory_format=torch.contiguous_format)}
        return st

    def _build_table(self):
        rows = []
        for gi, p, k in self._live():
            known = p in self.state
            if not known and torch.cuda.is_current_stream_capturing():
                raise hip.MSLError("Adam: a parameter without state inside a hipGraph capture; call "
                                   "optimizer.prepare() before capturing")
            st = self.init_state(p)
            rows.append((p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                         st["step"].data_ptr(), p.numel(), k, gi))
        return rows, tuple(r[:5] for r in rows)

    def _ensure_table(self):
        super()._ensure_table()
        nbytes = hip.load().msl_adam_coef_bytes(self._table_rows)
        if self._coef is None or self._coef.numel() * 4 < nbytes:
            self._coef = torch.zeros(max(nbytes // 4, 1), dtype=torch.float32, device=self.device)

    def prepare(self, used=None):
        """Build (and upload) the launch table for the given live-parameter mask now, creating every
        state tensor and the coefficient table it needs, so a step captured into a hipGraph
        afterwards finds them ready.  `used` defaults to the parameters that received gradients in
        the last step (before any step: in the backward passes since zero_grad).  Adam has no
        first-step rule, so this may be called before the first step."""
        if used is None:
            used = self._last_used if self._last_used is not None else self.grads.used.copy()
        self._with_used(used, self._ensure_table)

    def _hyper(self):
        g0 = self.param_groups[0] if self.param_groups else self.defaults
        for g in self.param_groups[1:]:
            if any(g[k] != g0[k] for k in ("betas", "eps", "weight_decay")):
                raise NotImplementedError("betas, eps and weight_decay must be the same in both groups")
        return float(g0["betas"][0]), float(g0["betas"][1]), float(g0["eps"]), float(g0["weight_decay"])

    def step(self, closure=None):
        if closure is not None:
            raise NotImplementedError("closure")
        b1, b2, eps, wd = self._hyper()
        self._before_step("Adam.step")
        lib = hip.load()
        _dev, p_ent, p_be, p_bo, nblocks = self._table
        n_ent, coef = self._table_rows, self._coef.data_ptr()
        if self.lr_dev is not None:
            # learning rates from device memory (set between hipGraph replays, utils/graph.py)
            hip.check(lib.msl_adam_step_lr_dev(p_ent, n_ent, p_be, p_bo, nblocks, self.lr_dev.data_ptr(), b1, b2,
                                               eps, wd, float(self.grad_scale), coef, hip.stream_ptr()),
                      "msl_adam_step_lr_dev")
        else:
            lr0, lr1 = self.group_lrs()
            hip.check(lib.msl_adam_step(p_ent, n_ent, p_be, p_bo, nblocks, lr0, lr1, b1, b2, eps, wd,
                                        float(self.grad_scale), coef, hip.stream_ptr()), "msl_adam_step")
        self._bump_versions()
        return None

    # -- checkpoints (train_source.py:662-704 stores optimizer.state_dict()) -----------
    def state_dict(self):
        """torch.optim.Adam.state_dict's format: SGD.state_dict's numbering of the duplicated lists,
        one {"step" (0-dim fp32), "exp_avg", "exp_avg_sq"} per tensor that has had a gradient, and
        groups carrying every key torch.optim.Adam of the installed torch writes."""
        first, groups = self._packed_groups()
        state = {}
        for g in self.param_groups:
            for p, _ in g["_unique"]:
                st = self.state.get(p)
                if st is not None:
                    state[first[id(p)]] = {k: st[k].detach().clone() for k in ("step", "exp_avg", "exp_avg_sq")}
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        """Accepts this class's and torch.optim.Adam's state dicts (same format).  State without
        the Adam moments (an SGD checkpoint) is an MSLError."""
        flat = [p for g in self.param_groups for p in g["params"]]
        for i, s in sd["state"].items():
            for k in ("exp_avg", "exp_avg_sq", "step"):
                if k not in s:
                    raise hip.MSLError(f"Adam.load_state_dict: state {i} has no {k!r} (keys {sorted(s)}): "
                                       "not an Adam optimizer state")
        for i, s in sd["state"].items():
            p = flat[int(i)]
            if not p.requires_grad:
                continue
            st = self.init_state(p)
            st["step"].copy_(torch.as_tensor(s["step"], dtype=torch.float32))
            for k in ("exp_avg", "exp_avg_sq"):
                st[k].copy_(s[k].to(p.device).reshape(p.shape))
        for g, sg in zip(self.param_groups, sd["param_groups"]):
            for k, v in sg.items():
                if k in ("lr", "betas", "eps", "weight_decay"):
                    g[k] = tuple(v) if k == "betas" else v
        self._table_key = None
