"""MutualInformation on one MI355X: the fused kernels (include/diffdrr_mi_hip.h) against the fp32 torch
composition (what the reference -- kornia's marginal_pdf / joint_pdf -- runs on a GPU).

  * forward and forward + backward (w.r.t. the moving image) at 256^2, num_bins in {64, 256},
    B in {1, 8, 32}, timed with HIP events (median of --reps, after warm-up);
  * the kernels' FLOP rate: 2 N K^2 per pair for J (forward) and as much again for the backward GEMM,
    against the 157.3 TF fp32 MFMA peak;
  * one registration iteration with MI as the criterion at 512^3 -> 256^2 (one pose), eager and as a
    GraphedIteration, in it/s.
Prints one JSON line per measurement; --out FILE also writes them there."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffdrr_amd import DRR, GraphedIteration, MutualInformation, Registration  # noqa: E402
from diffdrr_amd.data import synthetic_subject  # noqa: E402
from diffdrr_amd.metrics import mutual_information  # noqa: E402

PEAK_TF = 157.3

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--no-registration", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda:0")
lines = []


def emit(**kw):
    print(json.dumps(kw), flush=True)
    lines.append(kw)


def timed(fn, reps):
    for _ in range(3):
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


g = torch.Generator().manual_seed(0)
H = W = a.size
N = H * W
for K in (64, 256):
    crit = MutualInformation(num_bins=K).to(dev)
    for B in (1, 8, 32):
        fixed = torch.rand(1, 1, H, W, generator=g).to(dev).expand(B, -1, -1, -1)
        moving = torch.rand(B, 1, H, W, generator=g).to(dev)
        mv = moving.clone().requires_grad_(True)

        def fused_fwd():
            with torch.no_grad():
                crit(fixed, moving)

        def fused_fb():
            torch.autograd.grad(crit(fixed, mv).sum(), [mv])

        def comp_fwd():
            with torch.no_grad():
                mutual_information(fixed, moving, crit.bins, crit.sigma)

        def comp_fb():
            torch.autograd.grad(mutual_information(fixed, mv, crit.bins, crit.sigma).sum(), [mv])

        flop = 2.0 * N * K * K * B
        res = {}
        for name, fn in (("fused_fwd", fused_fwd), ("fused_fwd_bwd", fused_fb),
                         ("composition_fwd", comp_fwd), ("composition_fwd_bwd", comp_fb)):
            try:
                res[name] = timed(fn, a.reps)
            except torch.cuda.OutOfMemoryError:
                res[name] = None
            torch.cuda.empty_cache()
        # TF and share of the peak (None where the run did not fit in memory)
        tf_fwd = None if res["fused_fwd"] is None else flop / res["fused_fwd"] / 1e9
        tf_fb = None if res["fused_fwd_bwd"] is None else 2 * flop / res["fused_fwd_bwd"] / 1e9
        emit(kind="mi", H=H, W=W, num_bins=K, B=B,
             fused_fwd_ms=res["fused_fwd"], fused_fwd_bwd_ms=res["fused_fwd_bwd"],
             composition_fwd_ms=res["composition_fwd"], composition_fwd_bwd_ms=res["composition_fwd_bwd"],
             fused_fwd_tflops=tf_fwd, fused_fwd_bwd_tflops=tf_fb,
             fused_fwd_peak_frac=None if tf_fwd is None else tf_fwd / PEAK_TF,
             fused_fwd_bwd_peak_frac=None if tf_fb is None else tf_fb / PEAK_TF)

if not a.no_registration:
    drr = DRR(synthetic_subject(512, kind="phantom", seed=0), sdd=1020.0, height=256, delx=2.4,
              stop_gradients_through_grid_sample=True).to(dev)
    true_rot = torch.zeros(1, 3, device=dev)
    true_xyz = torch.tensor([[0.0, 850.0, 0.0]], device=dev)
    with torch.no_grad():
        gt = drr(true_rot, true_xyz, parameterization="euler_angles", convention="ZXY")
    scale = float(gt.max()) * 1.1

    class ScaledMI(torch.nn.Module):
        """MI of the two images brought into the bins' [0, 1] by a fixed scale."""

        def __init__(self):
            super().__init__()
            self.mi = MutualInformation()

        def forward(self, x1, x2):
            return self.mi(x1 / scale, x2 / scale)

    crit = ScaledMI().to(dev)
    rot = true_rot + torch.tensor([[0.1, -0.08, 0.05]], device=dev)
    xyz = true_xyz + torch.tensor([[10.0, -8.0, 6.0]], device=dev)

    def make():
        reg = Registration(drr, rot.clone(), xyz.clone(), parameterization="euler_angles", convention="ZXY")
        opt = torch.optim.SGD([{"params": [reg._rotation], "lr": 1e-3},
                               {"params": [reg._translation], "lr": 1e-1}], maximize=True)
        return reg, opt

    iters = 100
    reg, opt = make()

    def eager_step():
        opt.zero_grad()
        loss = crit(gt, reg()).sum()
        loss.backward()
        opt.step()
        return loss

    for _ in range(5):
        eager_step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        loss = eager_step()
    torch.cuda.synchronize()
    eager_its = iters / (time.perf_counter() - t0)
    reg, opt = make()
    step = GraphedIteration(reg, crit, opt, gt, warmup=3)
    for _ in range(5):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        loss = step()
    torch.cuda.synchronize()
    graphed_its = iters / (time.perf_counter() - t0)
    emit(kind="mi_registration", volume=512, detector=256, num_bins=256, eager_it_s=eager_its,
         graphed_it_s=graphed_its, last_mi=float(loss))

if a.out:
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
