"""FDK initialisation on one MI355X: the kernels of include/diffdrr_fbp_hip.h against the fp32 torch composition
of the same steps (diffdrr_amd/analytic.py), measured in the same run at 512^3 <- 32 views of 256^2.

  * the filter (cosine weight + ramp along the columns), the backprojection with the distance weight, and the
    whole `fdk` call (geometry on the host, both kernels);
  * for each kernel the bytes it has to move (filter: read and write the views; backprojection: write the
    volume, read the views once) over its time, and the voxel-view updates per second of the backprojection;
  * the fp32 composition of each step, and the largest difference of the kernels from it.
HIP events, median of --reps after warm-up.  Prints one JSON line per measurement; --out FILE also writes them
there.  --kernels-only N launches each kernel N times and nothing else (for a counter run of a profiler)."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffdrr_amd import DRR, analytic, fdk, ops  # noqa: E402
from diffdrr_amd.data import make_subject  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--volume", type=int, default=512)
ap.add_argument("--detector", type=int, default=256)
ap.add_argument("--views", type=int, default=32)
ap.add_argument("--kernels-only", type=int, default=0)
ap.add_argument("--out", default=None)
a = ap.parse_args()
assert torch.cuda.is_available(), "fbp_bench.py measures on the GPU"
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


D, N, B = a.volume, a.detector, a.views
kw = dict(parameterization="euler_angles", convention="ZXY")
drr = DRR(make_subject(torch.zeros(D, D, D), (1.0, 1.0, 1.0)), sdd=1020.0, height=N, delx=2.4 * 256 / N).to(dev)
rot = torch.zeros(B, 3)
rot[:, 0] = torch.arange(B) * (2 * math.pi / B)
xyz = torch.tensor([[0.0, 850.0, 0.0]]).repeat(B, 1)
images = torch.rand(B, N, N, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
geometry = analytic.view_geometry(drr, rot, xyz, **kw)
orbit = analytic.orbit_of(geometry)
taps = analytic.ramp_taps(N).float().to(dev)
geo = dict(u0=float(geometry.origin[0]), du=float(geometry.col_step[0]), v0=float(geometry.origin[1]),
           dv=float(geometry.row_step[1]), sdd=float(geometry.origin[2]), cosine_weight=True)
scale = 1.0 / float(geometry.col_step.norm())
views = torch.zeros(B, 16, dtype=torch.float64)
views[:, :12] = geometry.matrices.reshape(B, 12)
views[:, 12] = orbit.arc_weights * orbit.radius * geo["sdd"]
views = views.float().to(dev)
filtered = torch.empty_like(images)
volume = torch.empty(D, D, D, device=dev)


def run_filter():
    return ops.fbp_filter(images, orbit.axis, taps, scale, out=filtered, **geo)


def run_backproject():
    return ops.fbp_backproject(filtered, views, distance_weight=True, out=volume)


if a.kernels_only:
    for _ in range(a.kernels_only):
        run_filter()
        run_backproject()
    torch.cuda.synchronize()
    sys.exit(0)

t_filter = timed(run_filter)
t_bp = timed(run_backproject)
t_fdk = timed(lambda: fdk(drr, images, rot, xyz, **kw))
filter_bytes, bp_bytes = 2 * 4 * images.numel(), 4 * volume.numel() + 4 * images.numel()
emit(kind="filter", views=B, detector=N, axis=orbit.axis, kernel_ms=t_filter, bytes=filter_bytes,
     tb_s=filter_bytes / t_filter / 1e9, multiply_adds=B * N * N * N, gfma_s=B * N * N * N / t_filter / 1e6)
emit(kind="backproject", volume=D, views=B, detector=N, kernel_ms=t_bp, bytes=bp_bytes, tb_s=bp_bytes / t_bp / 1e9,
     voxel_views=D**3 * B, giga_voxel_views_s=D**3 * B / t_bp / 1e6)
emit(kind="fdk", volume=D, views=B, detector=N, call_ms=t_fdk, host_and_geometry_ms=t_fdk - t_filter - t_bp)

# the fp32 composition of the same steps on the same machine
reps = max(1, a.reps // 5)
t_cfilter = timed(lambda: analytic.filter_composition(images, orbit.axis, taps, scale, **geo), reps=max(3, reps))
cfiltered = analytic.filter_composition(images, orbit.axis, taps, scale, **geo)
t_cbp = timed(lambda: analytic.backproject_composition(cfiltered, views, (D, D, D), True), reps=reps, warmup=1)
cvolume = analytic.backproject_composition(cfiltered, views, (D, D, D), True)
emit(kind="composition", filter_ms=t_cfilter, backproject_ms=t_cbp, filter_speedup=t_cfilter / t_filter,
     backproject_speedup=t_cbp / t_bp,
     filter_max_abs_diff=float((run_filter() - cfiltered).abs().max()), filtered_max_abs=float(cfiltered.abs().max()),
     volume_max_abs_diff=float((run_backproject() - cvolume).abs().max()), volume_max_abs=float(cvolume.abs().max()))

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
