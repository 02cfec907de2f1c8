"""The fp64 reference of the BN entry points (csrc/bn.hip), in plain torch on the CPU: explicit formulas, not
F.batch_norm, shared by test_gpu_bn_forms.py and checked on the CPU by test_bn_forms.py.

Layout [c][nimg][p] as the library's: every (channel, image) row has its own batch statistics (bs = 1 per image).
"""
import torch

# momentum and eps as the calls receive them: C floats (the reference computes with exactly these values)
MOMENTUM, EPS = (float(torch.tensor(v, dtype=torch.float32)) for v in (0.1, 1e-5))
MARGIN = 1e-4  # no pre-activation within MARGIN * max|z| of zero (make_inputs)


def row_stats(x):
    """(mean, biased variance) of every row of x [c][nimg][p], fp64, two passes."""
    xd = x.double()
    mean = xd.mean(2)
    var = ((xd - mean[..., None]) ** 2).mean(2)
    return mean, var


def forward(x, gamma, beta, residual, running_mean, running_var, nbt, training, update_running, relu,
            momentum=MOMENTUM, eps=EPS):
    """y = act(bn(x) [+ residual]) and everything else msl_bn_fwd_mask leaves behind, in fp64 (nbt: int).

    Returns a dict: z (the pre-activation), y, mean / invstd [c][nimg] (what the call saves: the batch statistics
    in train mode, the running ones in eval mode), running_mean / running_var / nbt after the call.
    """
    c, nimg, p = x.shape
    xd = x.double()
    rm = None if running_mean is None else running_mean.double().clone()
    rv = None if running_var is None else running_var.double().clone()
    if training:
        mean, var = row_stats(x)
        if update_running:
            # torch refuses train mode at p = 1 (the unbiased variance divides by p - 1 = 0); the library defines
            # it: the unbiased variance is then the variance itself (0)
            unbiased = var * p / (p - 1) if p > 1 else var
            for n in range(nimg):  # image by image, image 0 first: nimg sequential bs = 1 calls
                rm = (1 - momentum) * rm + momentum * mean[:, n]
                rv = (1 - momentum) * rv + momentum * unbiased[:, n]
            if nbt is not None:
                nbt = nbt + nimg
        invstd = 1.0 / torch.sqrt(var + eps)
    else:
        mean = rm[:, None].expand(c, nimg).clone()
        invstd = (1.0 / torch.sqrt(rv + eps))[:, None].expand(c, nimg).clone()
    g = torch.ones(c, dtype=torch.float64) if gamma is None else gamma.double()
    b = torch.zeros(c, dtype=torch.float64) if beta is None else beta.double()
    z = (xd - mean[..., None]) * (invstd * g[:, None])[..., None] + b[:, None, None]
    if residual is not None:
        z = z + residual.double()
    y = torch.relu(z) if relu else z
    return dict(z=z, y=y, mean=mean, invstd=invstd, running_mean=rm, running_var=rv, nbt=nbt)


def backward(dy, x, positive, gamma, save_mean, save_invstd, training, dgamma0=None, dbeta0=None):
    """msl_bn_bwd* in fp64 from the operands the call reads: dy, x [c][nimg][p], the ReLU mask (`positive`: y > 0
    as a bool tensor, or None without ReLU), gamma (or None = 1) and the saved statistics [c][nimg] (fp32, as the
    forward left them).  dgamma0 / dbeta0: the previous contents when accumulating.

    Eval mode: the statistics are constants, so the two mean terms of dx are zero.
    Returns dict(dx, dres, dgamma, dbeta).
    """
    c, nimg, p = x.shape
    g = dy.double()
    if positive is not None:
        g = torch.where(positive, g, torch.zeros_like(g))
    mean, invstd = save_mean.double().reshape(c, nimg, 1), save_invstd.double().reshape(c, nimg, 1)
    xhat = (x.double() - mean) * invstd
    sg, sgx = g.sum(2), (g * xhat).sum(2)  # [c][nimg]
    w = invstd * (1.0 if gamma is None else gamma.double().reshape(c, 1, 1))
    if training:
        dx = (g - (sg / p)[..., None] - xhat * (sgx / p)[..., None]) * w
    else:
        dx = g * w
    dgamma, dbeta = sgx.sum(1), sg.sum(1)  # summed over the images
    if dgamma0 is not None:
        dgamma = dgamma + dgamma0.double()
    if dbeta0 is not None:
        dbeta = dbeta + dbeta0.double()
    return dict(dx=dx, dres=g, dgamma=dgamma, dbeta=dbeta)


def make_inputs(c, nimg, p, seed, training, relu, residual, affine, far):
    """The operands of one case, fp32 on the CPU.  x = 3 randn + 40 (`far`: the cancellation case of test_bn_act)
    or 3 randn + 1.  With relu, no pre-activation is left within MARGIN * max|z| of zero: such elements are moved
    away by nudging x (re-rounded to fp32, everything recomputed, at most 8 rounds), so the GPU's y > 0 must equal
    the reference's everywhere - no flip is excused.  (At p = 1 in train mode z does not depend on x; the
    assertion then holds or fails on beta and the residual alone.)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(c, nimg, p, generator=g) * 3 + (40.0 if far else 1.0)
    res = torch.randn(c, nimg, p, generator=g) if residual else None
    gamma = torch.rand(c, generator=g) + 0.5 if affine else None
    beta = torch.randn(c, generator=g) if affine else None
    rm, rv = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    dy = torch.randn(c, nimg, p, generator=g)
    dgamma0, dbeta0 = torch.randn(c, generator=g), torch.randn(c, generator=g)
    if relu:
        for _ in range(8):
            f = forward(x, gamma, beta, res, rm, rv, None, training, 0, 1)
            z = f["z"]
            thr = MARGIN * z.abs().max()
            near = z.abs() < thr
            if not bool(near.any()):
                break
            alpha = f["invstd"] * (1.0 if gamma is None else gamma.double()[:, None])
            step = torch.where(z >= 0, 1.0, -1.0) * (2 * thr - z.abs()) / alpha[..., None]
            x = torch.where(near, x.double() + step, x.double()).float()
        z = forward(x, gamma, beta, res, rm, rv, None, training, 0, 1)["z"]
        assert z.abs().max() > 0 and not bool((z.abs() < MARGIN * z.abs().max()).any()), "a pre-activation is still within the margin of 0"
    return dict(x=x, residual=res, gamma=gamma, beta=beta, running_mean=rm, running_var=rv, dy=dy, dgamma0=dgamma0,
                dbeta0=dbeta0)


def ulp_distance(got, want):
    """|got - want| in units of the fp32 spacing at `want` (both fp32), elementwise, as fp64."""
    want = want.float()
    spacing = (torch.nextafter(want.abs(), torch.full_like(want, float("inf"))) - want.abs()).double()
    return (got.double() - want.double()).abs() / spacing


def pack_bits(positive):
    """[rows][p] bool -> [rows][cdiv(p, 64)] int64 words, bit e % 64 of word e / 64 (msl_bn_fwd_mask's layout);
    the tail bits are zero."""
    rows, p = positive.shape
    words = -(-p // 64)
    pad = torch.zeros(rows, words * 64, dtype=torch.int64)
    pad[:, :p] = positive.to(torch.int64)
    lo = (pad.view(rows, words, 64)[:, :, :63] << torch.arange(63, dtype=torch.int64)).sum(2)
    top = pad.view(rows, words, 64)[:, :, 63]
    return lo + torch.where(top.bool(), torch.full_like(lo, -2 ** 63), torch.zeros_like(lo))
