"""Reconstruction on one MI355X: the fused kernels (include/diffdrr_recon_hip.h) against the torch ops a
reconstruction loop is otherwise built from, measured in the same run.

  * total variation, value + `grad += weight dTV/dV`, at 256^3, 512 x 512 x 133 and 512^3: the fused kernel
    against the fp32 composition through autograd (+ the `add_` into the gradient); the bytes the
    accumulate form has to move (12 B per voxel: read V, read and write grad) over the time, as a share of
    the 6.3 TB/s streaming ceiling; peak device memory of both routes above what they are given;
  * VolumeAdam against torch.optim.Adam(fused=True) + clamp_ at 2^27 elements (28 B per element);
  * one iteration at 512^3 -> 256^2, 32 views, Siddon: render + data loss, volume gradient, TV, optimiser,
    the fused route (Reconstruction.step) against the loop built from torch ops.
HIP events, median of --reps after warm-up.  Prints one JSON line per measurement; --out FILE also writes
them there."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffdrr_amd import DRR, Reconstruction, TotalVariation3d, VolumeAdam, total_variation_3d  # noqa: E402
from diffdrr_amd.data import make_subject, synthetic_subject  # noqa: E402

STREAM_TBS = 6.3  # the streaming ceiling of the MI355X's HBM

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--no-iteration", action="store_true")
ap.add_argument("--volume", type=int, default=512)
ap.add_argument("--views", type=int, default=32)
ap.add_argument("--out", default=None)
a = ap.parse_args()
assert torch.cuda.is_available(), "recon_bench.py measures on the GPU"
dev = torch.device("cuda:0")
lines = []


def emit(**kw):
    print(json.dumps(kw), flush=True)
    lines.append(kw)


def timed(fn, reps=a.reps, warmup=3):
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


# ------------------------------------------------------------------------------------ total variation
SPACING, WEIGHT = (0.7, 0.7, 2.5), 1e-3
for shape in ((256, 256, 256), (512, 512, 133), (512, 512, 512)):
    V = torch.rand(shape, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    grad = torch.zeros_like(V)
    n = V.numel()
    for mode in ("isotropic", "anisotropic"):
        tv = TotalVariation3d(mode=mode, eps=1e-3, spacing=SPACING)

        def fused():
            return tv.add_gradient_(V, grad, WEIGHT)

        def fused_value():
            with torch.no_grad():
                return tv(V)

        def composition():
            v = V.detach().requires_grad_(True)
            value = total_variation_3d(v, SPACING, mode, 1e-3)
            (g,) = torch.autograd.grad(value, [v])
            grad.add_(g, alpha=WEIGHT)
            return value.detach()

        t_f, t_v, t_c = timed(fused), timed(fused_value), timed(composition, reps=max(3, a.reps // 4))
        emit(kind="tv", shape=list(shape), mode=mode, voxels=n, fused_accumulate_ms=t_f, fused_value_ms=t_v,
             composition_ms=t_c, speedup=t_c / t_f, fused_tb_s=12.0 * n / t_f / 1e9,
             fused_stream_frac=12.0 * n / t_f / 1e9 / STREAM_TBS, volume_mib=4 * n / 2**20,
             fits_infinity_cache=bool(2 * 4 * n <= 256 * 2**20),
             fused_peak_extra_mib=peak_above(fused) / 2**20, composition_peak_extra_mib=peak_above(composition) / 2**20)
    del V, grad
    torch.cuda.empty_cache()

# ----------------------------------------------------------------------------------------- VolumeAdam
n = 2**27
p = torch.nn.Parameter(torch.rand(n, device=dev))
p.grad = torch.randn(n, device=dev)
mine = VolumeAdam([p], lr=0.02, lower=0.0)
t_mine = timed(mine.step)
del mine
theirs = torch.optim.Adam([p], lr=0.02, fused=True)


def torch_step():
    theirs.step()
    with torch.no_grad():
        p.clamp_(min=0)


t_theirs = timed(torch_step)
emit(kind="adam", elements=n, volume_adam_ms=t_mine, torch_fused_adam_clamp_ms=t_theirs, speedup=t_theirs / t_mine,
     volume_adam_tb_s=28.0 * n / t_mine / 1e9, volume_adam_stream_frac=28.0 * n / t_mine / 1e9 / STREAM_TBS,
     torch_tb_s=36.0 * n / t_theirs / 1e9)
del theirs, p
torch.cuda.empty_cache()

# -------------------------------------------------------------------------------------- one iteration
if not a.no_iteration:
    D, B = a.volume, a.views
    subject = synthetic_subject(D, kind="phantom", seed=0)
    geo = dict(sdd=1020.0, height=256, delx=2.4)
    kw = dict(parameterization="euler_angles", convention="ZXY")
    rot = torch.zeros(B, 3, device=dev)
    rot[:, 0] = torch.arange(B, device=dev) * (2 * math.pi / B)
    xyz = torch.tensor([[0.0, 850.0, 0.0]], device=dev).repeat(B, 1)
    truth = DRR(subject, **geo).to(dev)
    with torch.no_grad():
        measured = truth(rot, xyz, **kw)
    del truth
    blank = make_subject(torch.zeros(D, D, D), (1.0, 1.0, 1.0))
    del subject

    # the fused route, and its parts
    recon = Reconstruction(DRR(blank, **geo), lower=0.0).to(dev)
    with torch.no_grad():
        recon.density.fill_(0.01)
    tv = TotalVariation3d.for_drr(recon.drr)
    opt = recon.make_optimizer(lr=0.02)

    def fused_step():
        return recon.step(opt, measured, rot, xyz, regularizer=tv, weight=WEIGHT, **kw)

    def render_loss():
        with torch.no_grad():
            return torch.nn.functional.mse_loss(recon(rot, xyz, **kw), measured)

    def render_backward():
        recon.density.grad = None
        torch.nn.functional.mse_loss(recon(rot, xyz, **kw), measured).backward()

    t_step = timed(fused_step)
    t_render = timed(render_loss)
    t_fb = timed(render_backward)
    t_tv = timed(lambda: tv.add_gradient_(recon.density, recon.density.grad, WEIGHT))
    t_opt = timed(opt.step)
    peak_f = peak_above(fused_step)
    del recon, opt
    torch.cuda.empty_cache()

    # the same iteration from torch ops: what a user could build without this module
    drr = DRR(blank, **geo).to(dev)
    with torch.no_grad():
        drr.density.fill_(0.01)
    drr.density.requires_grad_()
    adam = torch.optim.Adam([drr.density], lr=0.02, fused=True)

    def torch_iteration():
        adam.zero_grad(set_to_none=True)
        data = torch.nn.functional.mse_loss(drr(rot, xyz, **kw), measured)
        (data + WEIGHT * total_variation_3d(drr.density, (1.0, 1.0, 1.0), "isotropic", 1e-3)).backward()
        adam.step()
        with torch.no_grad():
            drr.density.clamp_(min=0)
        return data.detach()

    t_torch = timed(torch_iteration, reps=max(3, a.reps // 4))
    peak_t = peak_above(torch_iteration)
    emit(kind="iteration", volume=D, detector=256, views=B, renderer="siddon", fused_step_ms=t_step,
         fused_it_s=1e3 / t_step, render_and_loss_ms=t_render, render_and_volume_gradient_ms=t_fb,
         volume_gradient_ms=t_fb - t_render, tv_accumulate_ms=t_tv, volume_adam_ms=t_opt,
         torch_iteration_ms=t_torch, torch_it_s=1e3 / t_torch, speedup=t_torch / t_step,
         fused_peak_extra_mib=peak_f / 2**20, torch_peak_extra_mib=peak_t / 2**20)

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
