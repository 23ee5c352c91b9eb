"""What tests/test_prox.py (host emulation) and tests/test_gpu_prox.py (MI355X) share: the host build of
csrc/prox_core.h, the scenes, the float64 yardsticks and the checks themselves, written once for either device.
The scheme is tests/jacobian_cases.py's.

The gate follows the project's rule: the torch composition (``prox_total_variation_3d``) evaluated in float32 on
the CPU has an error of its own against the same in float64; the kernels may be off by at most twice that, plus a
floor of 1e-6 of the compared quantity's scale -- max |b| for x, 1 for the dual (|p| <= 1).

Shapes, against the kernels' tile (16 rows x 64 z voxels, four z voxels per lane) marched over 32 planes:
    (1, 1, 7)      every axis below a tile, two axes of size 1, Dz no multiple of 4
    (2, 3, 4)      one whole quad per row, nothing else
    (1, 40, 70)    one plane; rows: two tiles and half a third; z: one tile and 6 voxels (a quad and a half)
    (37, 1, 5)     planes: one chunk of 32 and 5 more; one row; z: a quad and one voxel
    (5, 70, 9)     rows: four tiles and 6 rows
    (9, 17, 67)    rows: one past the tile; z: three past the tile (a partial quad in the second tile)
    (33, 18, 130)  planes: one past the chunk; rows: two past the tile; z: two tiles and two voxels
"""
import functools
import itertools
import math
import os
import subprocess

import torch

from conftest import ROOT
from diffdrr_amd import (DRR, Reconstruction, TotalVariation3d, _lib, prox_total_variation_3d, total_variation_3d,
                         tv_divergence_adjoint)
from diffdrr_amd.data import make_subject, synthetic_subject

EMU_SRC = os.path.join(ROOT, "tests", "emu", "prox_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "_build", "libprox_emu.so")
FLOOR = 1e-6
MODES = ("isotropic", "anisotropic")
SHAPES = ((1, 1, 7), (2, 3, 4), (1, 40, 70), (37, 1, 5), (5, 70, 9), (9, 17, 67), (33, 18, 130))
SPACINGS = ((1.0, 1.0, 1.0), (0.8, 1.7, 2.5))
LAMBDAS = (0.0, 0.05, 0.5)
ITERATIONS = (0, 1, 10)
KINDS = ("step", "constant", "bounds")
BOUNDS = (1.0 / 3.0, 5.0 / 3.0)  # of a volume uniform over [0, 2): a sixth below, a sixth above
GAP_SHAPE = (9, 17, 23)
WORST = {}  # (device type, quantity) -> (error / allowance, case): printed by the tests that fill it


@functools.lru_cache(maxsize=None)
def emu_library():
    """The host build of the entries (tests/emu/prox_emu.cpp), bound through the product's own binding."""
    csrc = os.path.join(ROOT, "diffdrr_amd", "csrc")
    deps = [EMU_SRC, os.path.join(ROOT, "include", "diffdrr_prox_hip.h")] + [
        os.path.join(csrc, f) for f in ("prox_core.h", "ddrr_common.h")]
    if not (os.path.exists(EMU_SO) and all(os.path.getmtime(d) <= os.path.getmtime(EMU_SO) for d in deps)):
        os.makedirs(os.path.dirname(EMU_SO), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-mfma", "-ffp-contract=off",
                        "-Wno-unknown-pragmas", EMU_SRC, "-o", EMU_SO], check=True)
    return _lib.prox_library(EMU_SO)


def route_prox_to_emulation(monkeypatch, ops):
    """The launcher patch of the host tests: ops' prox launches go to the host build, CPU tensors count as the
    device's, and the TV value ``Fista.step`` takes through ``ops.tv3d`` is the composition's."""
    lib = emu_library()
    monkeypatch.setattr(ops, "on_device", lambda t: True)
    monkeypatch.setattr(ops, "_launch_prox", lambda name, device, *a: lib.call(name, *a, None))
    monkeypatch.setattr(ops, "_query_prox", lambda name, *a: lib.query(name, *a))
    monkeypatch.setattr(ops, "tv3d", lambda volume, spacing=(1.0, 1.0, 1.0), mode="isotropic", eps=1e-3, **kw:
                        total_variation_3d(volume, spacing, mode, eps))


# ------------------------------------------------------------------------------------------------ scenes
@functools.lru_cache(maxsize=None)
def volume(shape, kind):
    """float32 on the CPU, seeded; shared, never modified.  "step" / "bounds": uniform noise in [0, 1) with a step
    of +1 across the middle plane of the longest axis; "constant": 0.75 everywhere."""
    if kind == "constant":
        return torch.full(shape, 0.75)
    g = torch.Generator().manual_seed(4000 + 31 * shape[0] + 7 * shape[1] + shape[2])
    b = torch.rand(shape, generator=g)
    axis = max(range(3), key=lambda a: shape[a])
    index = [slice(None)] * 3
    index[axis] = slice(shape[axis] // 2, None)
    b[tuple(index)] += 1.0
    return b


@functools.lru_cache(maxsize=None)
def dual_start(shape, lam):
    """p_0: zeros, except for lambda = 0.5, which starts from a seeded field inside the unit ball (a warm start
    that is not a fixed point)."""
    if lam != 0.5:
        return torch.zeros(3, *shape)
    g = torch.Generator().manual_seed(5000 + sum(shape))
    return torch.rand(3, *shape, generator=g) - 0.5


def bounds_of(kind):
    return BOUNDS if kind == "bounds" else (None, None)


@functools.lru_cache(maxsize=None)
def yardstick(shape, kind, spacing, mode, lam, n):
    """(x64, p64, the float32 composition's own max error of x, of p) from the shared start."""
    b, p0 = volume(shape, kind), dual_start(shape, lam)
    lower, upper = bounds_of(kind)
    x64, p64 = prox_total_variation_3d(b.double(), lam, spacing, mode, n, lower, upper, p0.double().clone())
    x32, p32 = prox_total_variation_3d(b, lam, spacing, mode, n, lower, upper, p0.clone())
    return x64, p64, float((x32.double() - x64).abs().max()), float((p32.double() - p64).abs().max())


def gate(device, name, what, got, ref64, own, scale):
    err = float((got.double().cpu() - ref64).abs().max())
    allowed = 2 * own + FLOOR * scale
    key = (torch.device(device).type, what)
    if err / allowed > WORST.get(key, (-1.0, ""))[0]:
        WORST[key] = (err / allowed, f"{name}: error {err:.3e}, float32 composition's {own:.3e}, allowed {allowed:.3e}")
    assert err <= allowed, (name, what, err, own, scale)


def print_worst(device):
    for (kind, what), (ratio, text) in sorted(WORST.items()):
        if kind == torch.device(device).type:
            print(f"worst {what} on {kind}: {ratio:.2f} of the allowance ({text})")


def run_kernel(ops, device, b, lam, spacing, mode, n, lower, upper, p0, **kw):
    dual = p0.clone().to(device)
    x, y = ops.prox_tv3d(b.to(device), lam, spacing, mode, n, lower, upper, dual, **kw)
    return x, y, dual


def check_against_float64(shape, mode, device, ops):
    """Every (kind, spacing, lambda, iterations) of one shape and mode on `device` against the float64 definition
    (item 2), with the exact cases on the way: lambda = 0 is clamp(b) and leaves the dual, a zero dual and no
    iterations is clamp(b), a constant volume is a fixed point, the bounds hold."""
    for kind, spacing, lam, n in itertools.product(KINDS, SPACINGS, LAMBDAS, ITERATIONS):
        b, p0 = volume(shape, kind), dual_start(shape, lam)
        lower, upper = bounds_of(kind)
        x64, p64, own_x, own_p = yardstick(shape, kind, spacing, mode, lam, n)
        x, _, dual = run_kernel(ops, device, b, lam, spacing, mode, n, lower, upper, p0)
        name = f"{shape} {kind} {spacing} {mode} lambda {lam} n {n}"
        assert x.shape == b.shape and x.dtype == torch.float32 and x.device.type == torch.device(device).type
        gate(device, name, "x", x, x64, own_x, float(b.abs().max()))
        gate(device, name, "dual", dual, p64, own_p, 1.0)
        x, dual = x.cpu(), dual.cpu()
        clamped = b if lower is None else b.clamp(lower, upper)
        if lam == 0.0:
            assert torch.equal(x, clamped) and torch.equal(dual, p0), name
        if n == 0:
            assert torch.equal(dual, p0), name
            if not bool(p0.any()):
                assert torch.equal(x, clamped), name
        if kind == "constant" and not bool(p0.any()):
            assert torch.equal(x, b) and not bool(dual.any()), name
        if lower is not None:
            assert float(x.min()) >= lower and float(x.max()) <= upper, name


# ------------------------------------------------------------------------------------- definition, float64
def primal_objective(x, b, lam, spacing, mode):
    return float(0.5 * (x - b).pow(2).sum() + lam * total_variation_3d(x, spacing, mode, 0.0))


def duality_gap(x, p, b, lam, spacing, mode):
    """P(x) - [1/2 |b|^2 - 1/2 |b - lambda D^T p|^2]: the unconstrained problem's, relative to lambda TV(b)."""
    dual_value = float(0.5 * b.pow(2).sum() - 0.5 * (b - lam * tv_divergence_adjoint(p, spacing)).pow(2).sum())
    return (primal_objective(x, b, lam, spacing, mode) - dual_value) / (
        lam * float(total_variation_3d(b, spacing, mode, 0.0)))


# -------------------------------------------------------------------------------------------- warm start
def check_warm_start(mode, device, ops):
    """Item 3: five iterations from the dual of five iterations are closer to the solution (1000 iterations in
    float64) than five cold ones, and the dual that comes back is the tensor that went in."""
    b, spacing, lam = volume(GAP_SHAPE, "step"), (1.0, 1.0, 1.0), 0.05
    solution, _ = prox_total_variation_3d(b.double(), lam, spacing, mode, 1000)
    tv = TotalVariation3d(mode=mode, spacing=spacing)
    bd = b.to(device)
    dual = torch.zeros(3, *b.shape, device=device)
    cold, _, back = tv._prox(bd, lam, 5, None, None, dual)
    assert back is dual and bool(dual.any())
    warm = tv.prox(bd, lam, 5, dual=dual)
    e_cold, e_warm = (float((v.double().cpu() - solution).abs().max()) for v in (cold, warm))
    print(f"{mode}: max |x - x_1000|: cold 5 iterations {e_cold:.3e}, warm 5 more {e_warm:.3e}")
    assert e_warm < e_cold
    again, same = prox_total_variation_3d(b, lam, spacing, mode, 5, dual=(start := torch.zeros(3, *b.shape)))
    assert same is start and again.shape == b.shape


# -------------------------------------------------------------------------------------------- epilogue
def check_epilogue(shape, mode, device, ops):
    """Item 4: y = x + beta (x - x_prev) to 1 ulp of the result, x bitwise the same with and without it.  x_prev is
    within a factor of two of x (x >= 0 here), so the float subtraction x - x_prev is exact and what is left is the
    single rounding of the fused multiply-add and that of beta to float: under one ulp."""
    b, spacing, lam, n = volume(shape, "step"), (0.8, 1.7, 2.5), 0.05, 3
    p0 = dual_start(shape, lam)
    plain, none, dual_plain = run_kernel(ops, device, b, lam, spacing, mode, n, 0.0, None, p0)
    assert none is None
    g = torch.Generator().manual_seed(77)
    x_prev = (plain.cpu() * (0.75 + 0.5 * torch.rand(shape, generator=g))).to(device)
    for beta in (0.0, 0.7):
        x, y, dual = run_kernel(ops, device, b, lam, spacing, mode, n, 0.0, None, p0, x_prev=x_prev, beta=beta)
        assert torch.equal(x, plain) and torch.equal(dual, dual_plain)
        ref = x.double() + beta * (x.double() - x_prev.double())
        ulp = torch.ldexp(torch.ones_like(ref), torch.frexp(ref.abs().clamp(min=2.0 ** -126))[1] - 24)
        worst = float(((y.double() - ref).abs() / ulp).max())
        print(f"{shape} {mode} beta {beta}: max |y - reference| = {worst:.3f} ulp")
        assert worst <= 1.0
        if beta == 0.0:
            assert torch.equal(y, x)


# ------------------------------------------------------------------------------------- reproducibility
def check_reproducible(device, ops, streams=()):
    """Item 5: two calls return equal x and dual; so does a call on each of `streams`."""
    for shape, mode in itertools.product(((9, 17, 67), (33, 18, 130)), MODES):
        b, p0 = volume(shape, "step"), dual_start(shape, 0.5)
        run = lambda: run_kernel(ops, device, b, 0.5, (0.8, 1.7, 2.5), mode, 10, *BOUNDS, p0)  # noqa: E731
        x, _, dual = run()
        x2, _, dual2 = run()
        assert torch.equal(x, x2) and torch.equal(dual, dual2) and bool(torch.isfinite(x).all())
        for stream in streams:
            stream.wait_stream(torch.cuda.current_stream(device))
            with torch.cuda.stream(stream):
                x3, _, dual3 = run()
            torch.cuda.current_stream(device).wait_stream(stream)
            assert torch.equal(x, x3) and torch.equal(dual, dual3)


# ------------------------------------------------------------------------------------- module routes
def check_module_routes(device, ops, monkeypatch):
    """Item 6: float32 contiguous device volumes take the kernel (one ops.prox_tv3d call each), float64, strided
    and CPU volumes the composition; the two agree within item 2's rule."""
    calls = []
    real = ops.prox_tv3d
    monkeypatch.setattr(ops, "prox_tv3d", lambda *a, **k: (calls.append(a), real(*a, **k))[1])
    shape, spacing, lam, n = (9, 17, 67), (0.8, 1.7, 2.5), 0.05, 10
    b = volume(shape, "step")
    tv = TotalVariation3d(mode="isotropic", eps=0.123, spacing=spacing)
    x64, p64, own_x, own_p = yardstick(shape, "step", spacing, "isotropic", lam, n)
    dual = torch.zeros(3, *shape, device=device)
    x = tv.prox(b.to(device), lam, n, dual=dual)
    assert len(calls) == 1
    gate(device, "module", "x", x, x64, own_x, float(b.abs().max()))
    gate(device, "module", "dual", dual, p64, own_p, 1.0)
    assert tv.prox(b.to(device), lam, n).shape == b.shape and len(calls) == 2  # (zeros allocated for None)
    # float64 and strided inputs on the device, then a CPU one: the composition
    d64 = torch.zeros(3, *shape, dtype=torch.float64, device=device)
    assert float((tv.prox(b.double().to(device), lam, n, dual=d64).cpu() - x64).abs().max()) <= 1e-12
    assert float((d64.cpu() - p64).abs().max()) <= 1e-12
    strided = b.to(device).transpose(0, 1).contiguous().transpose(0, 1)
    assert not strided.is_contiguous()
    xs = tv.prox(strided, lam, n)
    gate(device, "module (strided)", "x", xs, x64, own_x, float(b.abs().max()))
    assert len(calls) == 2
    monkeypatch.undo()
    xc = tv.prox(b, lam, n)
    assert xc.device.type == "cpu" and float((xc.double() - x64).abs().max()) <= own_x + 1e-12


# ------------------------------------------------------------------------------------- projector scenes
def views(n, device):
    rot = torch.zeros(n, 3, device=device)
    rot[:, 0] = torch.arange(n, device=device) * (2 * math.pi / n)
    xyz = torch.tensor([[0.0, 150.0, 0.0]], device=device).repeat(n, 1)
    return rot, xyz


def rmse(a, b):
    return float((a.double() - b.double()).pow(2).mean().sqrt())


def projector_scene(device, size, height, delx, renderer="siddon"):
    """8 views of a phantom of size^3 on a detector of height^2 -> (truth, DRR of a blank subject, pose arguments,
    keywords, measured): the scene of tests/test_gpu_reconstruction.py's end_to_end for size = height = 32."""
    subject = synthetic_subject(size, kind="phantom", seed=0)
    truth = subject.density.data.squeeze().to(device, torch.float32)
    geo = dict(sdd=300.0, height=height, delx=delx, renderer=renderer)
    kw = dict(parameterization="euler_angles", convention="ZXY")
    if renderer == "trilinear":
        kw["n_points"] = 3 * size
    rot, xyz = views(8, device)
    with torch.no_grad():
        measured = DRR(subject, **geo).to(device)(rot, xyz, **kw)
    blank = make_subject(torch.zeros(size, size, size), (1.0, 1.0, 1.0))
    return truth, DRR(blank, **geo).to(device), (rot, xyz), kw, measured


def check_lipschitz(device, renderer):
    """Item 7: 8 views of 24^2 through a 16^3 phantom."""
    truth, drr, pose, kw, measured = projector_scene(device, 16, 24, 1.6, renderer)
    recon = Reconstruction(drr, init=0.5 * truth, lower=0.0).to(device)
    before = recon.density.detach().clone()
    L = recon.lipschitz(*pose, generator=torch.Generator().manual_seed(0), **kw)
    q = recon.lipschitz_history
    print(f"{renderer}: Rayleigh quotients {' '.join(f'{v:.6g}' for v in q)}; L = {L:.6g}")
    assert isinstance(L, float) and len(q) == 12 and L == 1.05 * q[-1] and q[-1] > 0
    assert torch.equal(recon.density.detach(), before) and recon.density.grad is None
    assert all(b >= a * (1 - 1e-4) for a, b in zip(q, q[1:]))
    assert abs(q[-1] - q[-2]) <= 0.02 * q[-1]
    # the descent lemma on the first FISTA step: f(x1) <= f(y0) + <g, x1 - y0> + L / 2 |x1 - y0|^2
    mse = torch.nn.functional.mse_loss
    f_y = mse(recon(*pose, **kw), measured)
    (g,) = torch.autograd.grad(f_y, [recon.density])
    y0 = before
    fista = recon.make_fista(L, TotalVariation3d.for_drr(drr), weight=1e-3, inner_iterations=10)
    loss, _ = fista.step(measured, *pose, **kw)
    f_y = f_y.detach()
    assert abs(float(loss) - float(f_y)) <= 1e-5 * float(f_y)  # (the data loss at y_0: the same render)
    with torch.no_grad():
        d = (recon.density - y0).double()
        f_x = float(mse(recon(*pose, **kw), measured))
    bound = float(f_y) + float((g.double() * d).sum()) + 0.5 * L * float(d.pow(2).sum())
    print(f"{renderer}: f(y0) {float(f_y):.6g}, f(x1) {f_x:.6g}, quadratic bound {bound:.6g}")
    assert bool(d.any()) and f_x <= bound + 1e-6 * float(f_y)


FISTA_WEIGHT = 2e-4
FISTA_INNER = 10


def fista_yardstick(drr, pose, kw, measured, L, steps, dtype, keep=()):
    """FISTA with the same renderer, ``prox_total_variation_3d`` in `dtype` and torch arithmetic around it (the
    iterates themselves stay float32: the renderer's type) -> (x, {step: x after it}, last data loss)."""
    drr.density.requires_grad_()
    with torch.no_grad():
        drr.density.zero_()
    x = drr.density.detach().clone()
    y, t, dual, kept = x.clone(), 1.0, None, {}
    for it in range(steps):
        with torch.no_grad():
            drr.density.copy_(y)
        data = torch.nn.functional.mse_loss(drr(*pose, **kw), measured)
        (g,) = torch.autograd.grad(data, [drr.density])
        with torch.no_grad():
            b = (y - g / L).to(dtype)
            x_new, dual = prox_total_variation_3d(b, FISTA_WEIGHT / L, (1.0, 1.0, 1.0), "isotropic", FISTA_INNER, 0.0,
                                                  None, dual)
            x_new = x_new.to(torch.float32)
            t_new = 0.5 * (1.0 + math.sqrt(1.0 + 4.0 * t * t))
            y = x_new + ((t - 1.0) / t_new) * (x_new - x)
            x, t = x_new, t_new
        if it + 1 in keep:
            kept[it + 1] = x.clone()
    drr.density.requires_grad_(False)
    return x, kept, float(data.detach())


def objective(drr_like, x, pose, kw, measured):
    """mse(A x, measured) + weight TV(x), rendered through ``drr_like`` (a Reconstruction)."""
    with torch.no_grad():
        saved = drr_like.density.data
        drr_like.density.data = x
        data = torch.nn.functional.mse_loss(drr_like(*pose, **kw), measured)
        drr_like.density.data = saved
    return float(data) + FISTA_WEIGHT * float(total_variation_3d(x.double(), (1.0, 1.0, 1.0), "isotropic", 0.0))


def fista_end_to_end(device, steps=40):
    """Item 8 -> the figures its tests assert on (run once per session)."""
    truth, drr, pose, kw, measured = projector_scene(device, 32, 32, 2.4)
    recon = Reconstruction(drr, lower=0.0).to(device)
    L = recon.lipschitz(*pose, generator=torch.Generator().manual_seed(0), **kw)
    y32, early32, _ = fista_yardstick(drr, pose, kw, measured, L, steps, torch.float32, keep=(3,))
    _, early64, _ = fista_yardstick(drr, pose, kw, measured, L, 3, torch.float64, keep=(3,))
    tv = TotalVariation3d.for_drr(drr, mode="isotropic")
    fista = recon.make_fista(L, tv, weight=FISTA_WEIGHT, inner_iterations=FISTA_INNER)
    initial = (fista.t, fista.y.clone(), fista.dual)
    early = None
    for it in range(steps):
        data, tv_value = fista.step(measured, *pose, **kw)
        assert data.dim() == tv_value.dim() == 0 and data.device == tv_value.device == recon.density.device
        if it == 2:
            early = recon.density.detach().clone()
    final = recon.density.detach().clone()
    out = dict(truth=truth, L=L, history=recon.lipschitz_history, early=early, early32=early32[3], early64=early64[3],
               final=final, final_y=y32, objective_f=objective(recon, final, pose, kw, measured),
               objective_y=objective(recon, y32, pose, kw, measured), tv_value=float(tv_value),
               tv_final=float(total_variation_3d(final.double(), (1.0, 1.0, 1.0), "isotropic", 0.0)))
    # restart(): back to the state of a new object at the current density
    fista.restart()
    out["restart"] = (fista.t == initial[0] == 1.0 and fista.dual is None and initial[2] is None
                      and torch.equal(fista.y, recon.density.detach()) and not bool(initial[1].any()))
    return out


def check_fista_end_to_end(r):
    """The assertions of item 8 on what :func:`fista_end_to_end` returned.  With weight 2e-4 and 10 inner
    iterations the yardstick's RMSE to the phantom after 40 steps is 0.0176 against the zero volume's 0.1013 (host
    emulation of the renderer; a weight of 1e-3 gives 0.0303)."""
    truth = r["truth"]
    rmse0, rmse_y, rmse_f = rmse(torch.zeros_like(truth), truth), rmse(r["final_y"], truth), rmse(r["final"], truth)
    print(f"L {r['L']:.6g}; RMSE: start {rmse0:.6g} yardstick {rmse_y:.6g} fused {rmse_f:.6g}; objective yardstick "
          f"{r['objective_y']:.6g} fused {r['objective_f']:.6g}")
    assert rmse_y <= 0.5 * rmse0                          # first the yardstick alone
    own = float((r["early32"] - r["early64"]).abs().max())
    diff = float((r["early"] - r["early64"]).abs().max())
    scale = float(r["early64"].abs().max())
    print(f"after 3 steps: max |fused - float64 yardstick| {diff:.3e}, float32 yardstick's {own:.3e}, max {scale:.4g}")
    assert diff <= 2 * own + 1e-5 * scale
    assert abs(r["objective_f"] - r["objective_y"]) <= 0.01 * r["objective_y"]
    assert rmse_f <= 0.5 * rmse0
    assert float(r["final"].min()) >= 0.0
    assert abs(r["tv_value"] - r["tv_final"]) <= 1e-4 * r["tv_final"]  # (the value step returned is TV(x), eps = 0)
    assert r["restart"]
