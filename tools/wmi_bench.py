"""Weighted (masked) MutualInformation on one MI355X: the kernels of include/diffdrr_wmi_hip.h against the unweighted
kernels (include/diffdrr_mi_hip.h, what the parent commit has) and against the fp32 torch composition
(metrics.weighted_mutual_information, the only way to write the masked criterion without them).

  * forward and forward + backward (w.r.t. the moving image) at 256^2, num_bins in {64, 256}, B in {1, 8, 32}, with
    w = 1 everywhere and with a collimator (an ellipse with semi-axes 0.45 H, 0.45 W, zero outside: 36 % of the
    pixels masked, tools/wncc_bench.py's), the variants alternating inside every repetition; HIP events, median of
    --reps after warm-up.  The composition materialises (B, N, K) tensors: it is timed up to --composition-max-b poses;
  * one registration iteration with MI as the criterion at 512^3 -> 256^2 (one pose) as a GraphedIteration, with and
    without the weight, in it/s (a host clock around --replays replays that end in a device synchronise).
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
from diffdrr_amd.metrics import weighted_mutual_information  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--composition-max-b", type=int, default=8)
ap.add_argument("--replays", type=int, default=100)
ap.add_argument("--no-registration", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda:0")
lines = []


def emit(**kw):
    print(json.dumps(kw), flush=True)
    lines.append(kw)


def collimator(H, W):
    i, j = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    w = ((((i - (H - 1) / 2) / (0.45 * H)) ** 2 + ((j - (W - 1) / 2) / (0.45 * W)) ** 2) <= 1.0).float()
    return w.reshape(1, 1, H, W).to(dev)


def timed(variants, reps):
    """name -> median ms; the variants alternate inside every repetition"""
    ts = {k: [] for k in variants}
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return {k: statistics.median(v) for k, v in ts.items()}


g = torch.Generator().manual_seed(0)
H = W = a.size
mask, ones = collimator(H, W), torch.ones(1, 1, H, W, device=dev)
masked = float((mask == 0).float().mean())
for K in (64, 256):
    crit = MutualInformation(num_bins=K).to(dev)
    for B in (1, 8, 32):
        fixed = torch.rand(1, 1, H, W, generator=g).to(dev).expand(B, -1, -1, -1)
        moving = torch.rand(B, 1, H, W, generator=g).to(dev)
        mv = moving.clone().requires_grad_(True)

        def fwd(fn):
            def run():
                with torch.no_grad():
                    fn(moving)
            return run

        def fwd_bwd(fn):
            return lambda: torch.autograd.grad(fn(mv).sum(), [mv])

        calls = {"unweighted": lambda x: crit(fixed, x),
                 "weighted_ones": lambda x: crit(fixed, x, weight=ones),
                 "weighted_collimator": lambda x: crit(fixed, x, weight=mask)}
        if B <= a.composition_max_b:
            calls["composition_collimator"] = lambda x: weighted_mutual_information(fixed, x, mask, crit.bins, crit.sigma)
        res = {"fwd_ms": timed({k: fwd(fn) for k, fn in calls.items()}, a.reps),
               "fwd_bwd_ms": timed({k: fwd_bwd(fn) for k, fn in calls.items()}, a.reps)}
        torch.cuda.empty_cache()
        emit(kind="wmi", H=H, W=W, num_bins=K, B=B, masked_fraction=masked, reps=a.reps,
             **{f"{k}_{what}": v for what, d in res.items() for k, v in d.items()})

if not a.no_registration:
    drr = DRR(synthetic_subject(512, kind="phantom", seed=0), sdd=1020.0, height=256, delx=2.4,
              stop_gradients_through_grid_sample=True).to(dev)
    true_rot = torch.zeros(1, 3, device=dev)
    true_xyz = torch.tensor([[0.0, 850.0, 0.0]], device=dev)
    with torch.no_grad():
        gt = drr(true_rot, true_xyz, parameterization="euler_angles", convention="ZXY")
    top = float(gt.max()) * 1.1
    crit = MutualInformation(sigma=0.1 * top).to(dev)  # images in [0, top]: the bins and the kernel width scaled
    with torch.no_grad():
        crit.bins.mul_(top)
    rot = true_rot + torch.tensor([[0.1, -0.08, 0.05]], device=dev)
    xyz = true_xyz + torch.tensor([[10.0, -8.0, 6.0]], device=dev)
    mask = collimator(256, 256)
    its = {}
    for name, kw in (("unweighted", {}), ("weighted_collimator", {"weight": mask})):
        reg = Registration(drr, rot.clone(), xyz.clone(), parameterization="euler_angles", convention="ZXY")
        opt = torch.optim.SGD([{"params": [reg._rotation], "lr": 1e-3},
                               {"params": [reg._translation], "lr": 1e-1}], maximize=True)
        step = GraphedIteration(reg, crit, opt, gt, warmup=3, **kw)
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.replays):
            loss = step()
        torch.cuda.synchronize()
        its[name] = a.replays / (time.perf_counter() - t0)
        its[name + "_last_mi"] = float(loss)
    emit(kind="wmi_registration", volume=512, detector=256, num_bins=256, replays=a.replays,
         masked_fraction=float((mask == 0).float().mean()),
         **{(k if k.endswith("last_mi") else k + "_graphed_it_s"): v for k, v in its.items()})

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
