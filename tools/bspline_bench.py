"""Cubic B-spline free-form deformation on one MI355X: the three kernels of `warp_volume(..., basis="bspline")`
against the torch composition they replace (the separable `index_select` field of `dense_field`, a normalised
grid, `F.grid_sample`) and against the trilinear kernels (`basis="linear"`) on the same shapes:

  * forward, coefficient gradient and volume gradient at 256^3 and 512^3 with node spacings of 16 and 32 voxels: ms
    per kernel (HIP events, median of --reps after warm-up), and peak memory of forward + backward above the
    inputs, for the kernels and for the composition;
  * one deformable iteration at 512^3 -> 256^2 and 8 views: `FreeFormDeformation(basis="bspline")` forward, MSE,
    backward, Adam.
Prints one JSON line per measurement; --out FILE also writes them as text."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffdrr_amd import DRR, FreeFormDeformation, dense_field, ops, warp_volume  # noqa: E402
from diffdrr_amd.data import make_subject, phantom_volume  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--volumes", type=int, nargs="+", default=[256, 512])
ap.add_argument("--spacings", type=int, nargs="+", default=[16, 32])
ap.add_argument("--views", type=int, default=8)
ap.add_argument("--detector", type=int, default=256)
ap.add_argument("--out", default=os.path.join("profiles", "r07", "bspline_bench.txt"))
a = ap.parse_args()
assert torch.cuda.is_available(), "bspline_bench.py measures on the GPU"
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


def peak_above_inputs(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated(dev) - before) / 2**20


def torch_warp(V, U):
    D = V.shape
    u = dense_field(U, D, "bspline")
    coords = [torch.arange(d, device=V.device, dtype=V.dtype).reshape([-1 if k == i else 1 for k in range(3)]) + u[i]
              for i, d in enumerate(D)]
    grid = torch.stack([2 * coords[i] / (D[i] - 1) - 1 for i in (2, 1, 0)], dim=-1)[None]
    return F.grid_sample(V[None, None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0, 0]


for D in a.volumes:
    g = torch.Generator().manual_seed(0)
    V = torch.rand(D, D, D, generator=g).to(dev)
    gW = torch.rand(D, D, D, generator=g).to(dev)
    for spacing in a.spacings:
        G = (D - 1) // spacing + 1
        U = ((torch.rand(3, G, G, G, generator=g) * 2 - 1) * 2.5).to(dev)
        n = D ** 3
        t_fwd = timed(lambda: ops.bspline_forward(V, U))
        t_gu = timed(lambda: ops.bspline_backward_displacement(V, U, gW))
        t_gv = timed(lambda: ops.bspline_backward_volume(U, gW))
        l_fwd = timed(lambda: ops.warp_forward(V, U))
        l_gu = timed(lambda: ops.warp_backward_displacement(V, U, gW))
        l_gv = timed(lambda: ops.warp_backward_volume(U, gW))

        def ours():
            v, u = V.clone().requires_grad_(), U.clone().requires_grad_()
            warp_volume(v, u, basis="bspline").backward(gW)

        def theirs():
            v, u = V.clone().requires_grad_(), U.clone().requires_grad_()
            torch_warp(v, u).backward(gW)

        t_ours, t_theirs = timed(ours, reps=max(3, a.reps // 4)), timed(theirs, reps=max(3, a.reps // 4))
        t_theirs_fwd = timed(lambda: torch_warp(V, U), reps=max(3, a.reps // 4))
        emit(kind="kernels", volume=D, lattice=G, spacing=spacing, forward_ms=t_fwd, forward_gb_s=8 * n / t_fwd / 1e6,
             coefficient_gradient_ms=t_gu, volume_gradient_ms=t_gv, forward_backward_ms=t_ours,
             linear_forward_ms=l_fwd, linear_lattice_gradient_ms=l_gu, linear_volume_gradient_ms=l_gv,
             torch_forward_ms=t_theirs_fwd, torch_forward_backward_ms=t_theirs,
             workspace_mib=ops._query_bspline("ddrr_bspline_workspace_bytes", D, D, D, G, G, G) / 2**20,
             peak_mib=peak_above_inputs(ours), torch_peak_mib=peak_above_inputs(theirs),
             note="forward_backward includes cloning both inputs; peaks are forward + backward above the inputs")
    del V, gW

D, H = max(a.volumes), a.detector
drr = DRR(make_subject(phantom_volume(D, seed=0)), sdd=1020.0, height=H, delx=2.4 * 256 / H).to(dev)
ffd = FreeFormDeformation(drr, grid=((D - 1) // 32 + 1,) * 3, basis="bspline")
rot = torch.zeros(a.views, 3, device=dev)
rot[:, 0] = torch.arange(a.views, device=dev) * (torch.pi / a.views)
xyz = torch.tensor([[0.0, 850.0, 0.0]], device=dev).repeat(a.views, 1)
kw = dict(parameterization="euler_angles", convention="ZXY")
with torch.no_grad():
    ffd.displacement.uniform_(-1.5, 1.5)
    measured = ffd(rot, xyz, **kw)
    ffd.displacement.zero_()
opt = torch.optim.Adam([ffd.displacement], lr=0.1)


def iteration():
    opt.zero_grad(set_to_none=True)
    F.mse_loss(ffd(rot, xyz, **kw), measured).backward()
    opt.step()


emit(kind="deformable_iteration", volume=D, detector=H, views=a.views, lattice=ffd.displacement.shape[1],
     iteration_ms=timed(iteration), peak_mib=peak_above_inputs(iteration))

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
