"""What tests/test_gpu_mutual_information.py and tests/test_gpu_mi_dispatch.py share: the scenes, the torch
composition as the yardstick, the two gates and the host code's launch geometry restated for the printed lines.
The scheme is tests/warp_cases.py's and tests/jacobian_cases.py's.

The gates follow the project's rule: the torch composition of the reference's formula
(diffdrr_amd.metrics.mutual_information) in float64 on the device is the yardstick; the same composition in float32
(what the reference runs on a GPU) has an error of its own against it; the fused kernels may be off by at most twice
that, plus a floor of 2e-6 on a value and of 2e-5 of the largest gradient."""
import numpy as np
import torch

from conftest import rel_err
from diffdrr_amd.metrics import mutual_information

VALUE_FLOOR = 2e-6
GRAD_FLOOR = 2e-5


def _images(kind, B, H, W, g, bins=None):
    """(fixed (1, 1, H, W), moving (B, 1, H, W)) float32 on the CPU from the generator `g`."""
    if kind == "unit":
        return torch.rand(1, 1, H, W, generator=g), torch.rand(B, 1, H, W, generator=g)
    if kind == "outside":  # partly outside the bins' [0, 1]
        return torch.rand(1, 1, H, W, generator=g) * 1.6 - 0.3, torch.rand(B, 1, H, W, generator=g) * 1.4 - 0.2
    if kind == "constant":
        return torch.full((1, 1, H, W), 0.37), torch.rand(B, 1, H, W, generator=g)
    if kind == "background":  # a DRR's air: columns of exact zeros, of different widths in the two images
        fixed, moving = _images("unit", B, H, W, g)
        fixed[..., :5] = 0.0
        moving[..., :6] = 0.0
        return fixed, moving
    if kind == "on_bins":  # every moving pixel sits on a bin centre (u = 0 for one bin of each pixel)
        fixed = torch.rand(1, 1, H, W, generator=g)
        return fixed, bins.detach().cpu()[torch.randint(0, bins.numel(), (B, 1, H, W), generator=g)]
    raise ValueError(kind)


def _composition(crit, x1, x2, dtype):
    return mutual_information(x1.to(dtype), x2.to(dtype), crit.bins.to(dtype), crit.sigma.to(dtype),
                              crit.epsilon, crit.normalize)


def _value_gate(mine, f32, f64):
    """|kernel - f64| <= 2 |f32 - f64| + 2e-6 per pair (NaN exactly where the float64 composition is NaN).
    -> (largest kernel error, largest error of the float32 composition) over the pairs that are not NaN."""
    mine, f32, f64 = (np.asarray(v.detach().cpu(), dtype=np.float64) for v in (mine, f32, f64))
    nan = np.isnan(f64)
    assert np.array_equal(np.isnan(mine), nan), (mine, f64)
    ok = np.abs(mine - f64) <= 2 * np.abs(f32 - f64) + VALUE_FLOOR
    assert ok[~nan].all(), (mine, f32, f64)
    if nan.all():
        return 0.0, 0.0
    return float(np.abs(mine - f64)[~nan].max()), float(np.abs(f32 - f64)[~nan].max())


def _grad_gate(mine, r32, r64, what=None):
    """rel_err(kernel, f64) < 2 rel_err(f32, f64) + 2e-5 (conftest.rel_err: normalised by the largest gradient).
    -> (the kernel's error, the float32 composition's)."""
    e, e32 = rel_err(mine.cpu().numpy(), r64.cpu().numpy()), rel_err(r32.cpu().numpy(), r64.cpu().numpy())
    assert e < 2 * e32 + GRAD_FLOOR, (what, e, e32)
    return e, e32


def _run(fn, x1, x2, w, grad_of):
    """value and d (v w).sum() / d the images in `grad_of` ('moving', 'fixed', 'both').  The leaves are the float32
    images whatever `fn` computes in: a float64 composition's gradients arrive rounded to float32 (6e-8 of their
    size, far below the gate's floor)."""
    a = x1.clone().requires_grad_(grad_of in ("fixed", "both"))
    b = x2.clone().requires_grad_(grad_of in ("moving", "both"))
    v = fn(a.expand(x2.shape[0], -1, -1, -1), b)
    wanted = [t for t in (a, b) if t.requires_grad]
    grads = torch.autograd.grad((v * w).sum() if w is not None else v.sum(), wanted)
    return v.detach(), grads


def _references(crit, x1, x2, w):
    """(v32, (g32 fixed, g32 moving)), (v64, (g64 fixed, g64 moving)) of the composition; the float64 value has
    no NaN (so the NaN-matching branch of _value_gate excuses nothing)."""
    r32 = _run(lambda a, b: _composition(crit, a, b, torch.float32), x1, x2, w, "both")
    r64 = _run(lambda a, b: _composition(crit, a, b, torch.float64), x1, x2, w, "both")
    assert r64[0].dtype == torch.float64 and not bool(torch.isnan(r64[0]).any()), r64[0]
    return r32, r64


# ------------------------------------------------------------------------------------------------ geometry
def geometry(B, N, K):
    """csrc/mi.hip's launch geometry restated (geom(), ddrr_mi_backward), for the lines the tests print and for
    the cases that must take a stated path.  `workspace_floats` is what ddrr_mi_workspace_bytes returns / 4: the
    tests compare it with the library, which ties the forward's figures to the host code."""
    Kp = -(-K // 64) * 64
    nb = Kp // 64
    chunks = min(-(-1024 // (B * nb * nb)), -(-N // 256))
    cp = -(-(-(-N // chunks)) // 8) * 8
    chunks = -(-N // cp)
    ntiles = -(-N // 32)
    tpw = max(1, -(-ntiles * B // 256))
    ns = next(n for limit, n in ((2, 1), (8, 4), (32, 16), (64, 32), (128, 64), (256, 128)) if K <= limit)
    return dict(Kp=Kp, nb=nb, chunks=chunks, cp=cp, ntiles=ntiles, tpw=tpw, grad_chunks=-(-ntiles // tpw), NS=ns,
                waves=-(-K // 32), last_wave=K - 32 * (-(-K // 32) - 1),
                workspace_floats=B * chunks * (Kp * Kp + 2 * Kp) + 2 * B * (Kp * Kp + 2 * Kp))


def describe(B, N, K):
    g = geometry(B, N, K)
    return (f"B={B} N={N} K={K}: forward nb={g['nb']} chunks={g['chunks']} of {g['cp']} px "
            f"({g['cp'] // 4} per wave), backward NS={g['NS']} waves={g['waves']} (last holds {g['last_wave']}) "
            f"tpw={g['tpw']} of {g['ntiles']} tiles in {g['grad_chunks']} chunks")
