"""Weighted multi-view Levenberg-Marquardt registration on one MI355X at 512^3 -> 256^2, for V = 2 and 4 views and
S = 1 and 8 starts, all in one run on one board, the variants alternating:

  * the normal-sums kernel alone on one record: ddrr_wmvlm_normal_sums on the S * V poses of S starts seen from V views
    with one detector (P_stride 0) and with a detector per view (P_stride 3 N), beside what the parent commit has at
    the same number of poses: ddrr_mvlm_normal_sums (V views, no weight) and ddrr_wlm_normal_sums (one view, a weight,
    S * V independent poses) -- HIP events around --burst back-to-back launches, per launch;
  * the whole eager `WeightedMultiViewLevenbergMarquardt.step()` (four launches; a weight, a detector per view) beside
    `MultiViewLevenbergMarquardt.step()`.

The views are tools/mvlm_bench.py's orbit offsets about the isocentre (angles 0, pi/2, pi/4, 3 pi/4); the weight is
tools/wlm_bench.py's collimator (an ellipse with semi-axes 0.45 H, 0.45 W, zero outside: 36 % of the pixels masked),
shared by the views; the detectors of the odd views have another source-detector distance, pitch and principal point.
Medians of --reps after warm-up.  Prints one JSON line per measurement; --out FILE also writes them."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffdrr_amd import (  # noqa: E402
    DRR, Detector, LevenbergMarquardt, MultiViewLevenbergMarquardt, Registration, WeightedMultiViewLevenbergMarquardt,
    convert, ops,
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
assert torch.cuda.is_available(), "wmvlm_bench.py measures on the GPU"
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
i, j = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(H, dtype=torch.float64), indexing="ij")
weight = ((((i - (H - 1) / 2) / (0.45 * H)) ** 2 + ((j - (H - 1) / 2) / (0.45 * H)) ** 2) <= 1.0).float()
weight = weight.reshape(1, 1, H, H).to(dev)
masked = float((weight == 0).float().mean())
d0 = drr.detector
lateral = Detector(d0.sdd * 1.15, H, H, d0.delx * 0.9, d0.dely * 1.1, 3.0, -2.0, d0._reorient.detach().cpu().clone(),
                   reverse_x_axis=d0.reverse_x_axis).to(dev)


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
    dets = [lateral if v % 2 else None for v in range(V)]
    for S in a.starts:
        B = S * V
        # ---- the sums kernels, each on a record of B poses
        wmv1 = WeightedMultiViewLevenbergMarquardt(registration(S), fixed, K, weight=weight)
        wmv = WeightedMultiViewLevenbergMarquardt(registration(S), fixed, K, weight=weight, detectors=dets)
        mv = MultiViewLevenbergMarquardt(registration(S), fixed, K)
        wlm = LevenbergMarquardt(registration(B), fixed_one, weight=weight)
        held = {}
        for key, obj in (("wmv1", wmv1), ("wmv", wmv), ("mv", mv), ("wlm", wlm)):
            args, kw = obj._render()
            held[key] = (args.pop("aux"), args, kw)
        ws = {"wmv1": ops.wmvlm_workspace(S, V, N, dev), "wmv": ops.wmvlm_workspace(S, V, N, dev),
              "mv": ops.mvlm_workspace(S, V, N, dev), "wlm": ops.wlm_workspace(B, N, dev)}

        def sums(key):
            aux, args, kw = held[key]
            if key == "mv":
                return lambda: ops.mvlm_normal_sums(aux, mv.fixed, **args, **kw, ws=ws[key])
            if key == "wlm":
                return lambda: ops.wlm_normal_sums(aux, wlm.fixed, wlm.weight, **args, **kw, ws=ws[key])
            obj = wmv1 if key == "wmv1" else wmv
            return lambda: ops.wmvlm_normal_sums(aux, obj.fixed, obj.weight, **args, **kw, ws=ws[key])

        med, low = timed({key: burst(sums(key)) for key in ("wmv1", "wmv", "mv", "wlm")})
        per = {k: v / a.burst for k, v in med.items()}
        emit(kind="normal_sums_kernel_ms", starts=S, views=V, poses=B, volume=D, detector=H, masked_fraction=masked,
             reps=a.reps, burst=a.burst, wmvlm_normal_sums_one_detector_ms=per["wmv1"],
             wmvlm_normal_sums_detector_per_view_ms=per["wmv"], mvlm_normal_sums_ms=per["mv"],
             wlm_normal_sums_same_poses_ms=per["wlm"], wmvlm_over_mvlm=per["wmv"] / per["mv"],
             wmvlm_over_wlm=per["wmv"] / per["wlm"], detector_per_view_over_one=per["wmv"] / per["wmv1"],
             wmvlm_normal_sums_one_detector_min_ms=low["wmv1"] / a.burst,
             wmvlm_normal_sums_detector_per_view_min_ms=low["wmv"] / a.burst,
             mvlm_normal_sums_min_ms=low["mv"] / a.burst, wlm_normal_sums_same_poses_min_ms=low["wlm"] / a.burst,
             bytes_per_ray=52, wmvlm_tb_s=B * N * 52 / per["wmv"] / 1e9,
             note="HIP events around `burst` back-to-back launches on the default stream, per launch, median; bytes "
                  "per ray: 32 record + 4 fixed + 4 weight + 12 detector point")

        # ---- the whole step
        med, low = timed({"wmvlm_step": wmv.step, "wmvlm_step_one_detector": wmv1.step, "mvlm_step": mv.step})
        emit(kind="eager_step_ms", starts=S, views=V, poses=B, volume=D, detector=H, masked_fraction=masked,
             reps=a.reps, wmvlm_step_ms=med["wmvlm_step"], wmvlm_step_one_detector_ms=med["wmvlm_step_one_detector"],
             mvlm_step_ms=med["mvlm_step"], wmvlm_step_min_ms=low["wmvlm_step"],
             wmvlm_step_one_detector_min_ms=low["wmvlm_step_one_detector"], mvlm_step_min_ms=low["mvlm_step"],
             weighted_over_unweighted_step=med["wmvlm_step_one_detector"] / med["mvlm_step"],
             note="HIP events around one eager call, median; the parameters move while they are timed (trial after "
                  "trial), as they do in use; with a detector per view the odd views render another geometry, so "
                  "only the one-detector step renders what the unweighted step renders")

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
