"""The fused Adam step (csrc/adam.hip, utils/optim.Adam) on the GPU.

The reference is live torch.optim.Adam(..., foreach=False) on the CPU - the class the reference
trainers build (tools/train_source.py:145-146) - in fp64, with torch's own fp32 run as the yardstick
for the error a correct fp32 evaluation may have.  The trainer tests hold --optim Adam to what the
SGD path is held to: eager and replayed steps, a resumed run and the RCCL exchange agree bit for bit.
"""
import gc
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

from maxsquareloss_amd.tools.solve_gta5 import UDATrainer, build_parser  # noqa: E402
from maxsquareloss_amd.tools.train_source import init_args  # noqa: E402
from maxsquareloss_amd.utils.optim import Adam  # noqa: E402
from maxsquareloss_amd.utils.synthetic import synthetic_image, synthetic_labels  # noqa: E402

DEV = "cuda"
SHAPES = [(64, 3, 7, 7), (4097,), (19, 64, 3, 3), (10,), (1,)]
MULT = [1, 3, 4, 1, 1]
LATE = 3          # the (10,) tensor has no gradient in steps 0 and 1
STEPS = 6
BETAS = (0.9, 0.99)
U = 2.0 ** -23


def _lr(it):
    return 2.5e-4 * (1 - it / 1000) ** 0.9


def _groups(ps, lr):
    g0 = [p for p, k in zip(ps[:3], MULT[:3]) for _ in range(k)]
    return [{"params": g0, "lr": lr}, {"params": list(ps[3:]), "lr": 10 * lr}]


def _data(seed=5):
    g = torch.Generator().manual_seed(seed)
    init = [torch.randn(s, generator=g) for s in SHAPES]
    grads = []
    for _ in range(STEPS):
        row = []
        for j, s in enumerate(SHAPES):
            mag = 10.0 ** (torch.rand(s, generator=g) * 15 - 12)  # log-uniform over 1e-12 .. 1e3
            gr = (torch.randn(s, generator=g) * mag).reshape(-1)
            if gr.numel() > 1:
                gr[::7] = 0.0
            row.append(gr.reshape(s))
        grads.append(row)
    return init, grads


def _has_grad(step, j):
    return not (j == LATE and step < 2)


def _torch_run(init, grads, dtype, wd, gs):
    ps = [t.clone().to(dtype).requires_grad_() for t in init]
    opt = torch.optim.Adam(_groups(ps, _lr(0)), betas=BETAS, weight_decay=wd, foreach=False)
    for step in range(STEPS):
        opt.param_groups[0]["lr"], opt.param_groups[1]["lr"] = _lr(step), 10 * _lr(step)
        for j, p in enumerate(ps):
            p.grad = (grads[step][j] * gs).to(dtype) if _has_grad(step, j) else None
        opt.step()
    return ps, opt


_CACHE = {}


def _reference(wd, gs):
    """(init, grads, fp64 run, fp32 run) of torch-CPU for one parameter set, computed once."""
    if "data" not in _CACHE:
        _CACHE["data"] = _data()
    init, grads = _CACHE["data"]
    if (wd, gs) not in _CACHE:
        _CACHE[(wd, gs)] = (_torch_run(init, grads, torch.float64, wd, gs), _torch_run(init, grads, torch.float32, wd, gs))
    return (init, grads) + _CACHE[(wd, gs)]


def _mine_step(opt, ps, grads_row, step):
    opt.zero_grad()
    for j, (p, gr) in enumerate(zip(ps, grads_row)):
        if _has_grad(step, j):
            (p * gr.to(DEV)).sum().backward()  # through autograd, so the used-parameter hooks fire
    opt.step()


@pytest.mark.parametrize("gs", [1.0, 0.5])
@pytest.mark.parametrize("wd", [0.0, 5e-4])
def test_adam_multiplicity_matches_torch_cpu(wd, gs):
    init, grads, (p64, o64), (p32, o32) = _reference(wd, gs)
    mine = [t.clone().to(DEV).requires_grad_() for t in init]
    opt = Adam(_groups(mine, _lr(0)), betas=BETAS, weight_decay=wd)
    opt.grad_scale = gs
    for step in range(STEPS):
        opt.param_groups[0]["lr"], opt.param_groups[1]["lr"] = _lr(step), 10 * _lr(step)
        _mine_step(opt, mine, grads[step], step)
        assert (mine[LATE] in opt.state) == (step >= 2), step
    torch.cuda.synchronize()
    for j, k in enumerate(MULT):
        want = 4.0 if j == LATE else float(STEPS * k)
        st = opt.state[mine[j]]
        assert st["step"].item() == want == o64.state[p64[j]]["step"].item(), (j, st["step"].item())
        assert st["step"].dtype == torch.float32 and st["step"].dim() == 0
        ref = p64[j].detach()
        moved = (ref - init[j].double()).abs().max().item()
        assert moved > 0
        e_mine = (mine[j].detach().cpu().double() - ref).abs().max().item() / moved
        e_t32 = (p32[j].detach().double() - ref).abs().max().item() / moved
        bar = max(3 * e_t32, 4 * U * ref.abs().max().item() / moved)
        print(f"wd {wd} gs {gs} tensor {j}: E(p) {e_mine:.3e} torch-fp32 {e_t32:.3e} bar {bar:.3e}")
        assert e_mine <= bar, (j, e_mine, e_t32, bar)
        for name in ("exp_avg", "exp_avg_sq"):
            x64 = o64.state[p64[j]][name]
            den = x64.abs().max().item()
            assert den > 0
            e_mine = (st[name].cpu().double() - x64).abs().max().item() / den
            e_t32 = (o32.state[p32[j]][name].double() - x64).abs().max().item() / den
            bar = max(3 * e_t32, 8 * U)
            print(f"wd {wd} gs {gs} tensor {j} {name}: {e_mine:.3e} torch-fp32 {e_t32:.3e} bar {bar:.3e}")
            assert e_mine <= bar, (j, name, e_mine, e_t32, bar)


def test_adam_lr_dev_equals_by_value():
    init, grads = _reference(5e-4, 1.0)[:2]
    runs = []
    for dev_rates in (False, True):
        ps = [t.clone().to(DEV).requires_grad_() for t in init]
        opt = Adam(_groups(ps, _lr(0)), betas=BETAS, weight_decay=5e-4)
        lr_dev = torch.zeros(2, dtype=torch.float32, device=DEV)
        for step in range(3):
            rates = np.array([_lr(step), 10 * _lr(step)], dtype=np.float32)  # the fp32-rounded rates
            if dev_rates:
                lr_dev.copy_(torch.from_numpy(rates))
                opt.lr_dev = lr_dev
                opt.param_groups[0]["lr"] = opt.param_groups[1]["lr"] = 123.0  # must not be read
            else:
                opt.param_groups[0]["lr"], opt.param_groups[1]["lr"] = float(rates[0]), float(rates[1])
            _mine_step(opt, ps, grads[step], step)
        torch.cuda.synchronize()
        runs.append((ps, opt))
    (pa, oa), (pb, ob) = runs
    assert LATE < len(pa) and pa[LATE] in oa.state
    for j, (a, b) in enumerate(zip(pa, pb)):
        assert torch.equal(a, b), j
        assert not torch.equal(a.detach().cpu(), init[j]), j
        for name in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(oa.state[a][name], ob.state[b][name]), (j, name)


# ---------------------------------------------------------------------------- the trainers
H, W = 256, 512


def _trainer(graph, save_dir="", extra=()):
    argv = ["--crop_size", f"{W},{H}", "--target_crop_size", f"{W},{H}", "--imagenet_pretrained", "False",
            "--save_dir", save_dir, "--target_mode", "IW_maxsquare", "--multi", "True", "--lambda_target", "0.09",
            "--iter_max", "1000", "--graph", str(graph), "--optim", "Adam"] + list(extra)
    args, _, _ = init_args(build_parser().parse_args(argv))
    tr = UDATrainer(args, cuda=True)
    assert isinstance(tr.optimizer, Adam) and tr.optimizer.param_groups[0]["betas"] == (0.9, 0.99)
    tr.optimizer.zero_grad()
    return tr


def _inputs(it):
    return (synthetic_image(H, W, 40 + it).cuda(), synthetic_labels(H, W, 19, 40 + it).cuda(),
            synthetic_image(H, W, 540 + it).cuda())


def _state(tr):
    """(names, tensors): every parameter, BN buffer and Adam state tensor of a trainer."""
    names, out = [], []
    for n, p in tr.model.named_parameters():
        names.append(n)
        out.append(p.detach().clone())
    for n, b in tr.model.named_buffers():
        names.append(n)
        out.append(b.detach().clone())
    by_id = {id(p): n for n, p in tr.model.named_parameters()}
    for p in tr.optimizer._uniq:
        if p in tr.optimizer.state:
            for key in ("exp_avg", "exp_avg_sq", "step"):
                names.append(f"{by_id[id(p)]}:{key}")
                out.append(tr.optimizer.state[p][key].detach().clone())
    return names, out


def _first_diff(a, b):
    (na, ta), (nb, tb) = a, b
    if na != nb:
        return ("names", len(na), len(nb))
    for n, x, y in zip(na, ta, tb):
        if not torch.equal(x, y):
            return n
    return None


def test_adam_uda_step_eager_vs_graph_bit_for_bit():
    eager, graphed = _trainer(False), _trainer(True)
    assert graphed.use_graph and not eager.use_graph
    mult = {id(p): k for tr in (eager, graphed) for g in tr.optimizer.param_groups for p, k in g["_unique"]}
    for it in range(4):
        xs, ys, xt = _inputs(it)
        for tr in (eager, graphed):
            tr.uda_step(xs, ys, xt)
        torch.cuda.synchronize()
        assert graphed._graphed is not None and graphed._graphed.replays == it
        for name in ("loss_val", "loss_target", "loss_target_2"):
            a, b = getattr(graphed, name).item(), getattr(eager, name).item()
            assert a == b, (it, name, a, b)
        assert torch.equal(graphed.target_loss.last_hist, eager.target_loss.last_hist), it
        d = _first_diff(_state(graphed), _state(eager))
        assert d is None, (it, d)
        # the counters advanced once per iteration, by the multiplicity, also under replay
        for tr in (eager, graphed):
            for p, st in tr.optimizer.state.items():
                assert st["step"].item() == (it + 1) * mult[id(p)], (it, tr.use_graph)
    assert len(graphed.optimizer.state) == len(eager.optimizer.state) > 300
    dead = dict(eager.model.named_parameters())["layer6.conv2d_list.3.weight"]
    assert dead not in eager.optimizer.state
    assert eager.optimizer.param_groups[0]["lr"] < 2.5e-4  # the poly rate moved (iter_max 1000)
    assert graphed.optimizer.param_groups[0]["lr"] == eager.optimizer.param_groups[0]["lr"]


def test_adam_resume_continues_bit_for_bit(tmp_path):
    whole = _trainer(False, save_dir=str(tmp_path))
    for it in range(2):
        whole.uda_step(*_inputs(it))
    whole.save_checkpoint("adam_it2.pth")
    path = os.path.join(str(tmp_path), "adam_it2.pth")
    assert os.path.exists(path)
    whole.uda_step(*_inputs(2))
    resumed = _trainer(False)
    resumed.load_checkpoint(path)
    assert resumed.current_iter == 2
    steps = {st["step"].item() for st in resumed.optimizer.state.values()}
    assert steps == {2.0, 6.0, 8.0}, steps
    resumed.optimizer.zero_grad()
    resumed.uda_step(*_inputs(2))
    torch.cuda.synchronize()
    for name in ("loss_val", "loss_target", "loss_target_2"):
        assert getattr(resumed, name).item() == getattr(whole, name).item(), name
    d = _first_diff(_state(resumed), _state(whole))
    assert d is None, d


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rccl_worker(port, q):
    """tests/test_gpu_dp.py's one-rank RCCL harness with --optim Adam: the captured, segmented DP step
    with the exchange forced on against the same run without a process group."""
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
        import torch.distributed as dist
        out = {}
        for dp in (False, True):
            print(f"[adam rccl worker] trainer dp={dp}", file=sys.stderr, flush=True)
            tr = _trainer(True, extra=["--dp_exchange", str(dp)])
            assert (tr.reducer is not None) == dp and dist.is_initialized() == dp
            if dp:
                assert dist.get_backend() == "nccl" and tr.reducer.always
            losses = []
            for it in range(3):
                tr.uda_step(*_inputs(it))
                torch.cuda.synchronize()
                print(f"[adam rccl worker] iteration {it} done", file=sys.stderr, flush=True)
                losses.append((tr.loss_val.item(), tr.loss_target.item(), tr.loss_target_2.item()))
            assert tr._graphed is not None and tr._graphed.replays == 2
            if dp:
                assert tr._graphed.graph_update is not None
            names, tensors = _state(tr)
            out[dp] = (losses, names, torch.cat([t.reshape(-1).float() for t in tensors]).cpu().numpy())
            del tr
            gc.collect()
        dist.destroy_process_group()
        q.put(("ok", out))
    except Exception as e:
        import traceback
        q.put(("error", traceback.format_exc() + repr(e)))
        raise


def test_adam_rccl_world1_exchange():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_worker, args=(_free_port(), q))
    p.start()
    try:
        import queue
        import time
        deadline = time.time() + 300
        while True:  # a worker that dies fails the test instead of hanging it
            try:
                status, got = q.get(timeout=5)
                break
            except queue.Empty:
                assert p.is_alive(), f"RCCL worker died, exit code {p.exitcode}"
                assert time.time() < deadline, "RCCL worker timed out"
        assert status == "ok", got
        p.join(timeout=60)
        assert p.exitcode == 0
    finally:
        if p.is_alive():
            p.kill()
            p.join(timeout=10)
    (l0, n0, s0), (l1, n1, s1) = got[False], got[True]
    assert l0 == l1, (l0, l1)
    assert n0 == n1 and any(n.endswith(":exp_avg_sq") for n in n0)
    assert np.array_equal(s0, s1), int((s0 != s1).sum())
