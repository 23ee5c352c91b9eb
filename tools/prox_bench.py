"""The TV proximal operator and FISTA on one MI355X: the fused kernels (include/diffdrr_prox_hip.h) against the
float32 torch composition of the same iterations (prox_total_variation_3d), measured in the same run.

  * the prox at 256^3 and 512^3, isotropic and anisotropic: time per inner iteration (the slope between 10 and 20
    iterations) and per 10-iteration prox; the bytes the scheme has to move (72 B per voxel and iteration, 20 B for
    the last pass) over the time, beside the 4.1 TB/s the TV kernel reaches for a stencil of the same shape; peak
    device memory of both routes above what they are given;
  * one FISTA outer step at 512^3 -> 256^2, 32 views, Siddon (render + volume gradient, gradient step, prox with 10
    warm-started inner iterations, TV value), beside the Adam step (Reconstruction.step) on the same scene;
  * the objective mse + weight TV (no smoothing) of both loops every 10 steps from the same start.
HIP events, median of --reps after warm-up.  Prints one JSON line per measurement; --out FILE also writes them
there."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffdrr_amd import (DRR, Reconstruction, TotalVariation3d, ops, prox_total_variation_3d,  # noqa: E402
                         total_variation_3d)
from diffdrr_amd.data import make_subject, synthetic_subject  # noqa: E402

TV_KERNEL_TBS = 4.1       # what tv3d_kernel reaches for a stencil of the same shape (tools/recon_bench.py)
BYTES_PER_ITERATION = 72  # primal 16 + 4, dual 28 + 24
BYTES_LAST_PASS = 20

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--sizes", type=int, nargs="*", default=[256, 512])
ap.add_argument("--no-iteration", action="store_true")
ap.add_argument("--volume", type=int, default=512)
ap.add_argument("--views", type=int, default=32)
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--out", default=None)
a = ap.parse_args()
assert torch.cuda.is_available(), "prox_bench.py measures on the GPU"
dev = torch.device("cuda:0")
lines = []


def emit(**kw):
    print(json.dumps(kw), flush=True)
    lines.append(kw)


def timed(fn, reps=a.reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def peak_above(fn):
    """Peak device memory of one call above what is allocated before it (bytes)."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


# ------------------------------------------------------------------------------------------------ the prox
SPACING, LAM = (0.7, 0.7, 2.5), 0.05
for size in a.sizes:
    shape = (size, size, size)
    b = torch.rand(shape, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    b[size // 2:] += 1.0
    dual = torch.zeros(3, *shape, device=dev)
    n = b.numel()
    for mode in ("isotropic", "anisotropic"):
        def fused(iterations=10):
            dual.zero_()
            return ops.prox_tv3d(b, LAM, SPACING, mode, iterations, 0.0, None, dual)[0]

        def composition(iterations=10):
            dual.zero_()
            return prox_total_variation_3d(b, LAM, SPACING, mode, iterations, 0.0, None, dual)[0]

        t_zero = timed(dual.zero_)
        t10, t20 = timed(fused) - t_zero, timed(lambda: fused(20)) - t_zero
        t_c = timed(composition, reps=max(3, a.reps // 3)) - t_zero
        per_iteration = (t20 - t10) / 10
        diff = float((fused() - composition()).abs().max())
        emit(kind="prox", shape=list(shape), mode=mode, voxels=n, prox10_ms=t10, per_iteration_ms=per_iteration,
             composition10_ms=t_c, speedup=t_c / t10, iteration_tb_s=BYTES_PER_ITERATION * n / per_iteration / 1e9,
             prox10_tb_s=(10 * BYTES_PER_ITERATION - 12 + BYTES_LAST_PASS) * n / t10 / 1e9,
             tv_kernel_tb_s=TV_KERNEL_TBS, volume_mib=4 * n / 2**20, fused_peak_extra_mib=peak_above(fused) / 2**20,
             composition_peak_extra_mib=peak_above(composition) / 2**20, max_abs_difference=diff)
    del b, dual
    torch.cuda.empty_cache()

# -------------------------------------------------------------------------------------- one outer step
if not a.no_iteration:
    D, B, WEIGHT = a.volume, a.views, 1e-3
    subject = synthetic_subject(D, kind="phantom", seed=0)
    geo = dict(sdd=1020.0, height=256, delx=2.4)
    kw = dict(parameterization="euler_angles", convention="ZXY")
    rot = torch.zeros(B, 3, device=dev)
    rot[:, 0] = torch.arange(B, device=dev) * (2 * math.pi / B)
    xyz = torch.tensor([[0.0, 850.0, 0.0]], device=dev).repeat(B, 1)
    truth = DRR(subject, **geo).to(dev)
    with torch.no_grad():
        measured = truth(rot, xyz, **kw)
    del truth, subject
    blank = make_subject(torch.zeros(D, D, D), (1.0, 1.0, 1.0))

    def objective(recon):
        """(mse, TV without smoothing) of recon.density: the objective is mse + WEIGHT TV"""
        with torch.no_grad():
            data = torch.nn.functional.mse_loss(recon(rot, xyz, **kw), measured)
            return torch.stack([data, ops.tv3d(recon.density.detach(), (1.0, 1.0, 1.0), "isotropic", 0.0)])

    def trace_of(step):
        out = []
        for it in range(a.steps):
            step()
            if (it + 1) % 10 == 0:
                out.append(objective(recon))
        return out

    def totals(trace):
        return [d + WEIGHT * v for d, v in torch.stack(trace).tolist()]

    recon = Reconstruction(DRR(blank, **geo), lower=0.0).to(dev)
    tv = TotalVariation3d.for_drr(recon.drr)
    t_power = timed(lambda: recon.lipschitz(rot, xyz, **kw), reps=3, warmup=1)
    L = recon.lipschitz(rot, xyz, generator=torch.Generator().manual_seed(0), **kw)
    fista = recon.make_fista(L, tv, weight=WEIGHT, inner_iterations=10)
    trace_f = trace_of(lambda: fista.step(measured, rot, xyz, **kw))
    t_step = timed(lambda: fista.step(measured, rot, xyz, **kw))
    t_grad = timed(lambda: recon._data_gradient(fista._leaf, measured, (rot, xyz), kw))
    g = torch.rand_like(recon.density.data)
    t_prox = timed(lambda: tv._prox(g, WEIGHT / L, 10, 0.0, None, fista.dual, x_prev=recon.density.data, beta=0.5))
    peak_f = peak_above(lambda: fista.step(measured, rot, xyz, **kw))
    del fista, g

    # the same loop with a more exact prox, and with a larger constant: what the 10-iteration trace is bounded by
    variants = {}
    for name, inner, scale, restart in (("inner_50", 50, 1.0, 0), ("inner_10_lipschitz_x2", 10, 2.0, 0),
                                        ("inner_10_restart_every_10", 10, 1.0, 10)):
        with torch.no_grad():
            recon.density.zero_()
        other = recon.make_fista(scale * L, tv, weight=WEIGHT, inner_iterations=inner)
        count = [0]

        def step():
            if restart and count[0] and count[0] % restart == 0:
                other.restart()
            count[0] += 1
            other.step(measured, rot, xyz, **kw)

        variants[name] = trace_of(step)
        del other

    with torch.no_grad():
        recon.density.zero_()
    opt = recon.make_optimizer(lr=0.02)
    trace_a = trace_of(lambda: recon.step(opt, measured, rot, xyz, regularizer=tv, weight=WEIGHT, **kw))
    t_adam = timed(lambda: recon.step(opt, measured, rot, xyz, regularizer=tv, weight=WEIGHT, **kw))
    reached = next((10 * (i + 1) for i, v in enumerate(totals(trace_f)) if v <= totals(trace_a)[-1]), None)
    emit(kind="fista", volume=D, detector=256, views=B, renderer="siddon", weight=WEIGHT, inner_iterations=10,
         lipschitz=L, rayleigh_quotients=recon.lipschitz_history, lipschitz_12_iterations_ms=t_power,
         fista_step_ms=t_step, render_and_volume_gradient_ms=t_grad, prox10_with_extrapolation_ms=t_prox,
         adam_step_ms=t_adam, fista_peak_extra_mib=peak_f / 2**20, steps=a.steps,
         objective_every_10_steps_fista=totals(trace_f), objective_every_10_steps_adam=totals(trace_a),
         mse_and_tv_every_10_steps_fista=torch.stack(trace_f).tolist(),
         mse_and_tv_every_10_steps_adam=torch.stack(trace_a).tolist(),
         objective_every_10_steps_fista_variants={k: totals(v) for k, v in variants.items()},
         fista_steps_to_adam_final_objective=reached)

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
