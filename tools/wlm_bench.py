"""Levenberg-Marquardt registration with a pixel weight on one MI355X at 512^3 -> 256^2, for 1 and for 32 poses, all
in one run on one board, the variants alternating:

  * the normal-sums kernel alone on one record: ddrr_lm_normal_sums (unweighted, what the parent commit has) and
    ddrr_wlm_normal_sums (weighted) -- HIP events around --burst back-to-back launches, per launch;
  * the whole eager `LevenbergMarquardt.step()` (four launches) without and with `weight=`;
  * the weighted first-order iteration it is an alternative to: eager `DRR.ncc(fixed, rot, xyz, weight=w)` forward +
    backward + `PoseAdam.step()` (1e-1 / 5e0).

The weight is tools/wncc_bench.py's collimator: an ellipse with semi-axes 0.45 H, 0.45 W, zero outside (36 % of the
pixels masked).  Medians of --reps after warm-up.  Prints one JSON line per measurement; --out FILE also writes them."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffdrr_amd import DRR, LevenbergMarquardt, PoseAdam, Registration, ops  # noqa: E402
from diffdrr_amd.data import synthetic_subject  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--burst", type=int, default=20)
ap.add_argument("--volume", type=int, default=512)
ap.add_argument("--detector", type=int, default=256)
ap.add_argument("--poses", type=int, nargs="+", default=[1, 32])
ap.add_argument("--out", default=None)
a = ap.parse_args()
assert torch.cuda.is_available(), "wlm_bench.py measures on the GPU"
dev = torch.device("cuda:0")
lines = []


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
    fixed = drr(true_rot, true_xyz, parameterization="euler_angles", convention="ZXY")
i, j = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(H, dtype=torch.float64), indexing="ij")
weight = ((((i - (H - 1) / 2) / (0.45 * H)) ** 2 + ((j - (H - 1) / 2) / (0.45 * H)) ** 2) <= 1.0).float()
weight = weight.reshape(1, 1, H, H).to(dev)
masked = float((weight == 0).float().mean())


def starts(B):
    g = torch.Generator().manual_seed(1)
    return (true_rot + ((torch.rand(B, 3, generator=g) - 0.5) * 0.4).to(dev),
            true_xyz + ((torch.rand(B, 3, generator=g) - 0.5) * 60.0).to(dev))


def registration(B):
    r0, x0 = starts(B)
    return Registration(drr, r0.clone(), x0.clone(), parameterization="euler_angles", convention="ZXY")


for B in a.poses:
    # ---- the two kernels on one record
    lm, wlm = LevenbergMarquardt(registration(B), fixed), LevenbergMarquardt(registration(B), fixed, weight=weight)
    args, kw = lm._render()
    aux = args.pop("aux")
    ws, wws = ops.lm_workspace(B, N, dev), ops.wlm_workspace(B, N, dev)

    def burst(fn):
        def run():
            for _ in range(a.burst):
                fn()
        return run

    med, low = timed({
        "lm_normal_sums": burst(lambda: ops.lm_normal_sums(aux, lm.fixed, **args, **kw, ws=ws)),
        "wlm_normal_sums": burst(lambda: ops.wlm_normal_sums(aux, wlm.fixed, wlm.weight, **args, **kw, ws=wws)),
    })
    t0, t1 = med["lm_normal_sums"] / a.burst, med["wlm_normal_sums"] / a.burst
    emit(kind="normal_sums_kernel_ms", poses=B, volume=D, detector=H, masked_fraction=masked, reps=a.reps,
         burst=a.burst, lm_normal_sums_ms=t0, wlm_normal_sums_ms=t1, weighted_over_unweighted=t1 / t0,
         lm_normal_sums_min_ms=low["lm_normal_sums"] / a.burst, wlm_normal_sums_min_ms=low["wlm_normal_sums"] / a.burst,
         lm_bytes_per_ray=48, wlm_bytes_per_ray=52, lm_tb_s=B * N * 48 / t0 / 1e9, wlm_tb_s=B * N * 52 / t1 / 1e9,
         note="HIP events around `burst` back-to-back launches on the default stream, per launch, median; bytes per "
              "ray: 32 record + 4 fixed + 12 detector point (+ 4 weight)")
    # with w == 1 the weighted sums are the unweighted ones (printed, not asserted: the compiler may contract the
    # two kernels' Jacobian rows differently)
    ones = torch.ones(1, N, device=dev)
    same = torch.equal(ops.wlm_normal_sums(aux, lm.fixed, ones, **args, **kw)[0][..., :44],
                       ops.lm_normal_sums(aux, lm.fixed, **args, **kw)[0])
    emit(kind="ones_weight_equals_unweighted_bit_for_bit", poses=B, equal=bool(same))

    # ---- the whole step, and the weighted first-order iteration
    reg = registration(B)
    adam = PoseAdam(reg.rotation, reg.translation, 1e-1, 5e0, maximize=True)

    def adam_iteration():
        adam.zero_grad()
        drr.ncc(fixed, reg.rotation, reg.translation, convention="ZXY", weight=weight).sum().backward()
        adam.step()

    med, low = timed({"lm_step": lm.step, "wlm_step": wlm.step, "weighted_adam_iteration": adam_iteration})
    emit(kind="eager_step_ms", poses=B, volume=D, detector=H, masked_fraction=masked, reps=a.reps,
         lm_step_ms=med["lm_step"], wlm_step_ms=med["wlm_step"],
         weighted_adam_iteration_ms=med["weighted_adam_iteration"],
         lm_step_min_ms=low["lm_step"], wlm_step_min_ms=low["wlm_step"],
         weighted_adam_iteration_min_ms=low["weighted_adam_iteration"],
         weighted_over_unweighted_step=med["wlm_step"] / med["lm_step"],
         note="HIP events around one eager call, median; the poses move while they are timed (LM: trial after trial; "
              "Adam: step after step), as they do in use")

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
