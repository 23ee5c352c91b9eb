"""Multi-view Levenberg-Marquardt registration on one MI355X at 512^3 -> 256^2, for V = 2 and 4 views and S = 1 and 8
starts, all in one run on one board, the variants alternating:

  * the normal-sums kernel alone on one record: ddrr_mvlm_normal_sums on the S * V poses of S starts seen from V views,
    and ddrr_lm_normal_sums (one view; lm.hip is what the parent commit has) on S * V independent poses -- HIP events
    around --burst back-to-back launches, per launch;
  * the whole eager `MultiViewLevenbergMarquardt.step()` (four launches) and `LevenbergMarquardt.step()` at S * V poses;
  * the first-order iteration it is an alternative to: eager `drr(view_poses(rot, xyz, views))` through the matrix
    route, the mean of `NormalizedCrossCorrelation2d` over the S * V images, backward, `torch.optim.Adam` (1e-1 / 5e0).

The views are orbit offsets about the isocentre, K_v = E_0^-1 E(angle_v), angles 0, pi/2, pi/4, 3 pi/4.  Medians of --reps
after warm-up.  Prints one JSON line per measurement; --out FILE also writes them."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffdrr_amd import (  # noqa: E402
    DRR, LevenbergMarquardt, MultiViewLevenbergMarquardt, NormalizedCrossCorrelation2d, Registration, convert, ops,
)
from diffdrr_amd.data import synthetic_subject  # noqa: E402
from diffdrr_amd.registration import relative_views, view_poses  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--burst", type=int, default=20)
ap.add_argument("--volume", type=int, default=512)
ap.add_argument("--detector", type=int, default=256)
ap.add_argument("--views", type=int, nargs="+", default=[2, 4])
ap.add_argument("--starts", type=int, nargs="+", default=[1, 8])
ap.add_argument("--out", default=None)
a = ap.parse_args()
assert torch.cuda.is_available(), "mvlm_bench.py measures on the GPU"
dev = torch.device("cuda:0")
lines = []
ANGLES = (0.0, math.pi / 2, math.pi / 4, 3 * math.pi / 4)


def emit(**kw):
    print(json.dumps(kw), flush=True)
    lines.append(kw)


def timed(variants, reps=a.reps, warmup=5):
    """name -> median ms of one call, the variants alternating inside every repetition"""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return {k: statistics.median(v) for k, v in ts.items()}, {k: min(v) for k, v in ts.items()}


D, H = a.volume, a.detector
N = H * H
drr = DRR(synthetic_subject(D, kind="phantom", seed=0), sdd=1020.0, height=H, delx=2.4 * 256 / H,
          stop_gradients_through_grid_sample=True).to(dev)
true_rot, true_xyz = torch.zeros(1, 3, device=dev), torch.tensor([[0.0, 850.0, 0.0]], device=dev)
with torch.no_grad():
    fixed_one = drr(true_rot, true_xyz, parameterization="euler_angles", convention="ZXY")
ncc = NormalizedCrossCorrelation2d()


def starts(B):
    g = torch.Generator().manual_seed(1)
    return (true_rot + ((torch.rand(B, 3, generator=g) - 0.5) * 0.4).to(dev),
            true_xyz + ((torch.rand(B, 3, generator=g) - 0.5) * 60.0).to(dev))


def registration(B):
    r0, x0 = starts(B)
    return Registration(drr, r0.clone(), x0.clone(), parameterization="euler_angles", convention="ZXY")


def burst(fn):
    def run():
        for _ in range(a.burst):
            fn()
    return run


for V in a.views:
    rot_v = torch.tensor([[t, 0.0, 0.0] for t in ANGLES[:V]], dtype=torch.float64)
    K = relative_views(convert(rot_v, true_xyz.double().cpu().expand(V, 3), parameterization="euler_angles",
                               convention="ZXY"))
    with torch.no_grad():
        fixed = drr(view_poses(true_rot, true_xyz, K, "ZXY")).reshape(V, 1, H, H).contiguous()
    for S in a.starts:
        B = S * V
        # ---- the two sums kernels, each on a record of B poses
        mv, lm = MultiViewLevenbergMarquardt(registration(S), fixed, K), LevenbergMarquardt(registration(B), fixed_one)
        mv_args, mv_kw = mv._render()
        lm_args, lm_kw = lm._render()
        mv_aux, lm_aux = mv_args.pop("aux"), lm_args.pop("aux")
        mv_ws, lm_ws = ops.mvlm_workspace(S, V, N, dev), ops.lm_workspace(B, N, dev)
        med, low = timed({
            "mvlm": burst(lambda: ops.mvlm_normal_sums(mv_aux, mv.fixed, **mv_args, **mv_kw, ws=mv_ws)),
            "lm": burst(lambda: ops.lm_normal_sums(lm_aux, lm.fixed, **lm_args, **lm_kw, ws=lm_ws)),
        })
        emit(kind="normal_sums_kernel_ms", starts=S, views=V, poses=B, volume=D, detector=H, reps=a.reps, burst=a.burst,
             mvlm_normal_sums_ms=med["mvlm"] / a.burst, lm_normal_sums_same_poses_ms=med["lm"] / a.burst,
             mvlm_normal_sums_min_ms=low["mvlm"] / a.burst, lm_normal_sums_same_poses_min_ms=low["lm"] / a.burst,
             bytes_per_ray=48, mvlm_tb_s=B * N * 48 / (med["mvlm"] / a.burst) / 1e9,
             note="HIP events around `burst` back-to-back launches on the default stream, per launch, median; bytes "
                  "per ray: 32 record + 4 fixed + 12 detector point")

        # ---- the whole step, and the first-order iteration through view_poses and the matrix route
        reg = registration(S)
        adam = torch.optim.Adam([{"params": [reg._rotation], "lr": 1e-1}, {"params": [reg._translation], "lr": 5e0}],
                                maximize=True)
        targets = fixed.repeat(S, 1, 1, 1)  # pose s V + v against image v

        def adam_iteration():
            adam.zero_grad()
            ncc(targets, drr(view_poses(reg._rotation, reg._translation, K, "ZXY"))).mean().backward()
            adam.step()

        med, low = timed({"mvlm_step": mv.step, "lm_step": lm.step, "adam_iteration": adam_iteration})
        emit(kind="eager_step_ms", starts=S, views=V, poses=B, volume=D, detector=H, reps=a.reps,
             mvlm_step_ms=med["mvlm_step"], lm_step_same_poses_ms=med["lm_step"],
             multiview_adam_iteration_ms=med["adam_iteration"], mvlm_step_min_ms=low["mvlm_step"],
             lm_step_same_poses_min_ms=low["lm_step"], multiview_adam_iteration_min_ms=low["adam_iteration"],
             note="HIP events around one eager call, median; the poses move while they are timed (LM: trial after "
                  "trial; Adam: step after step), as they do in use; Adam: drr(view_poses(...)), mean NCC, backward, "
                  "torch.optim.Adam")

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
