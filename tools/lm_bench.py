"""Levenberg-Marquardt registration on one MI355X at 512^3 -> 256^2, at 1 and 8 poses, against the first-order
iteration (`GraphedIteration` + `PoseAdam`, 1e-1 / 5e0) measured in the same run:

  * ms per LM step (eager: four launches, no host synchronisation) and per kernel of it -- ddrr_pose_raygen_forward, the
    brick kernel with its record, ddrr_lm_normal_sums, ddrr_lm_step -- against ms per Adam iteration;
  * renders and wall time to NCC >= 0.9999 for both methods from the start of `bench.py --config 4` (truth
    rot = 0, xyz = (0, 850, 0); start off by up to 0.2 rad / 30 mm, seed 1; with 8 poses: 8 such starts, the
    count is that of the first start to get there, LM only).
HIP events, median of --reps after warm-up.  Prints one JSON line per measurement; --out FILE also writes them."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffdrr_amd import (DRR, GraphedIteration, LevenbergMarquardt, NormalizedCrossCorrelation2d, PoseAdam,  # noqa: E402
                         Registration, ops)
from diffdrr_amd.data import synthetic_subject  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--volume", type=int, default=512)
ap.add_argument("--detector", type=int, default=256)
ap.add_argument("--poses", type=int, nargs="+", default=[1, 8])
ap.add_argument("--cap", type=int, default=400, help="renders / iterations after which a method has not converged")
ap.add_argument("--out", default=None)
a = ap.parse_args()
assert torch.cuda.is_available(), "lm_bench.py measures on the GPU"
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


D, H = a.volume, a.detector
drr = DRR(synthetic_subject(D, kind="phantom", seed=0), sdd=1020.0, height=H, delx=2.4 * 256 / H,
          stop_gradients_through_grid_sample=True).to(dev)
true_rot, true_xyz = torch.zeros(1, 3, device=dev), torch.tensor([[0.0, 850.0, 0.0]], device=dev)
with torch.no_grad():
    fixed = drr(true_rot, true_xyz, parameterization="euler_angles", convention="ZXY")


def starts(B):
    g = torch.Generator().manual_seed(1)
    return (true_rot + ((torch.rand(B, 3, generator=g) - 0.5) * 0.4).to(dev),
            true_xyz + ((torch.rand(B, 3, generator=g) - 0.5) * 60.0).to(dev))


def registration(B):
    r0, x0 = starts(B)
    return Registration(drr, r0.clone(), x0.clone(), parameterization="euler_angles", convention="ZXY")


for B in a.poses:
    # ---- time per step
    lm_eager = LevenbergMarquardt(registration(B), fixed)
    reg = registration(B)
    adam = GraphedIteration(reg, NormalizedCrossCorrelation2d(), PoseAdam(reg.rotation, reg.translation, 1e-1, 5e0,
                                                                          maximize=True), fixed)
    t_eager, t_adam = timed(lm_eager.step), timed(adam)
    # ---- per kernel of the step, on the eager object's buffers
    args, kw = lm_eager._render()
    aux = args.pop("aux")
    source_target_img = ops.pose_raygen_forward(args["rot"], args["xyz"], args["axes"], args["reorient34"],
                                                args["Ainv"], args["P"])
    from diffdrr_amd.renderers import _brick_storage
    cfg = drr.renderer._cfg(False, det=(H, H))
    launch_ws = ops.launch_workspace(drr.density.shape, dev)
    t_raygen = timed(lambda: ops.pose_raygen_forward(args["rot"], args["xyz"], args["axes"], args["reorient34"],
                                                     args["Ainv"], args["P"], clear=aux, clear_launch_ws=launch_ws))
    _, source, target, img = source_target_img

    def bricks():
        aux.zero_()
        launch_ws.zero_()
        ops.siddon_forward_bricks(drr.density, source, target, img, cfg["det"], voxel_shift=cfg["voxel_shift"],
                                  eps=cfg["eps"], want_aux=True, storage=_brick_storage(drr.density, cfg, B),
                                  want_image=False, aux=aux, launch_ws=launch_ws, cleared=True)

    t_bricks_and_fills = timed(bricks)
    t_fills = timed(lambda: (aux.zero_(), launch_ws.zero_()))
    bricks()
    ws = ops.lm_workspace(B, H * H, dev)
    t_sums = timed(lambda: ops.lm_normal_sums(aux, lm_eager.fixed, **args, **kw, ws=ws))
    state, rot, xyz = ops.lm_state(B, 1.0, dev), args["rot"].clone(), args["xyz"].clone()
    t_step = timed(lambda: ops.lm_step(ws, state, rot, xyz, H * H))
    emit(kind="step_time", poses=B, volume=D, detector=H, lm_eager_ms=t_eager,
         adam_graph_ms=t_adam, raygen_ms=t_raygen, brick_kernel_ms=t_bricks_and_fills - t_fills,
         normal_sums_ms=t_sums, lm_step_ms=t_step, sums_bytes=B * H * H * 36,
         sums_tb_s=B * H * H * 36 / t_sums / 1e9)

    # ---- renders and wall time to NCC >= 0.9999
    def run(step, cap=a.cap):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        best, n = -1.0, cap
        for it in range(1, cap + 1):
            best = max(best, float(step().max()))
            if best >= 0.9999:
                n = it
                break
        torch.cuda.synchronize()
        return n, best, (time.perf_counter() - t0) * 1e3

    lm = LevenbergMarquardt(registration(B), fixed)
    n_lm, ncc_lm, ms_lm = run(lm.step)
    if B == 1:
        reg = registration(B)
        it = GraphedIteration(reg, NormalizedCrossCorrelation2d(), PoseAdam(reg.rotation, reg.translation, 1e-1, 5e0,
                                                                            maximize=True), fixed)
        n_adam, ncc_adam, ms_adam = run(lambda: it().reshape(1))
    else:  # (the captured first-order iteration hands back the SUM of the poses' values: no per-pose stopping test)
        n_adam = ncc_adam = ms_adam = None
    emit(kind="to_ncc_0.9999", poses=B, cap=a.cap, lm_renders=n_lm, lm_best_ncc=ncc_lm, lm_wall_ms=ms_lm,
         adam_iterations=n_adam, adam_best_ncc=ncc_adam, adam_wall_ms=ms_adam,
         note="wall time includes one host read of the NCC per step for the stopping test; several poses: the first "
              "start to get there")

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
