"""The weighted (masked) registration step on one MI355X at 512^3 -> 256^2, for 1 and for 32 poses, all in one run,
the variants alternating inside every repetition:

  (a) the unweighted fused step, `DRR.ncc(fixed, rot, xyz)` forward + backward (what the parent commit has);
  (b) the weighted fused step, `DRR.ncc(fixed, rot, xyz, weight=w)` forward + backward;
  (c) the same objective as (b) the only way it can be written without the weighted kernels: `drr(rot, xyz, ...)`
      (the differentiable render), the masked NCC from torch ops (`metrics.weighted_ncc`), backward;
  (d) at one pose: `GraphedIteration` iterations per second for (a), (b) and (c) (`PoseAdam`, 1e-1 / 5e0).
The weight is a collimator: an ellipse with semi-axes 0.45 H, 0.45 W, zero outside (36 % of the pixels masked).
(a)-(c): HIP events around one eager step, median of --reps after warm-up.  (d): a host clock around --replays
replays that end in a device synchronise, median of --rounds.  Prints one JSON line per measurement; --out FILE
also writes them."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffdrr_amd import DRR, GraphedIteration, NormalizedCrossCorrelation2d, PoseAdam, Registration  # noqa: E402
from diffdrr_amd.data import synthetic_subject  # noqa: E402
from diffdrr_amd.metrics import weighted_ncc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--replays", type=int, default=2000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--volume", type=int, default=512)
ap.add_argument("--detector", type=int, default=256)
ap.add_argument("--poses", type=int, nargs="+", default=[1, 32])
ap.add_argument("--out", default=None)
a = ap.parse_args()
assert torch.cuda.is_available(), "wncc_bench.py measures on the GPU"
dev = torch.device("cuda:0")
lines = []


def emit(**kw):
    print(json.dumps(kw), flush=True)
    lines.append(kw)


D, H = a.volume, a.detector
drr = DRR(synthetic_subject(D, kind="phantom", seed=0), sdd=1020.0, height=H, delx=2.4 * 256 / H,
          stop_gradients_through_grid_sample=True).to(dev)
true_rot, true_xyz = torch.zeros(1, 3, device=dev), torch.tensor([[0.0, 850.0, 0.0]], device=dev)
with torch.no_grad():
    fixed = drr(true_rot, true_xyz, parameterization="euler_angles", convention="ZXY")
i, j = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(H, dtype=torch.float64), indexing="ij")
weight = ((((i - (H - 1) / 2) / (0.45 * H)) ** 2 + ((j - (H - 1) / 2) / (0.45 * H)) ** 2) <= 1.0).float()
weight = weight.reshape(1, 1, H, H).to(dev)
masked = float((weight == 0).float().mean())


class TorchMaskedNCC(torch.nn.Module):
    """(c) as a criterion: the masked NCC from torch ops"""

    def forward(self, x1, x2):
        return weighted_ncc(x1.expand(x2.shape[0], -1, -1, -1), x2, weight, 1e-5)


def starts(B):
    g = torch.Generator().manual_seed(1)
    return (true_rot + ((torch.rand(B, 3, generator=g) - 0.5) * 0.4).to(dev),
            true_xyz + ((torch.rand(B, 3, generator=g) - 0.5) * 60.0).to(dev))


def eager_steps(B):
    r0, x0 = starts(B)
    r, x = r0.clone().requires_grad_(), x0.clone().requires_grad_()
    torch_ncc = TorchMaskedNCC()

    def run(value):
        r.grad = x.grad = None
        value().sum().backward()

    return {
        "a_unweighted_fused": lambda: run(lambda: drr.ncc(fixed, r, x, convention="ZXY")),
        "b_weighted_fused": lambda: run(lambda: drr.ncc(fixed, r, x, convention="ZXY", weight=weight)),
        "c_render_torch_masked_ncc": lambda: run(lambda: torch_ncc(
            fixed, drr(r, x, parameterization="euler_angles", convention="ZXY"))),
    }


for B in a.poses:
    steps = eager_steps(B)
    for fn in steps.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in steps}
    for _ in range(a.reps):
        for k, fn in steps.items():  # (alternating: the variants share whatever else the host is doing)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    emit(kind="eager_step_ms", poses=B, volume=D, detector=H, masked_fraction=masked, reps=a.reps,
         **{k: statistics.median(v) for k, v in ts.items()},
         **{k + "_min": min(v) for k, v in ts.items()},
         extra_bytes_per_ray_each_way=4, note="HIP events around forward + backward of one eager step, median")

# (d) captured iterations per second at one pose
graphs = {}
for name, crit, kw in (("a_unweighted_fused", NormalizedCrossCorrelation2d(), {}),
                       ("b_weighted_fused", NormalizedCrossCorrelation2d(), {"weight": weight}),
                       ("c_render_torch_masked_ncc", TorchMaskedNCC(), {})):
    r0, x0 = starts(1)
    reg = Registration(drr, r0.clone(), x0.clone(), parameterization="euler_angles", convention="ZXY")
    opt = PoseAdam(reg.rotation, reg.translation, 1e-1, 5e0, maximize=True)
    graphs[name] = GraphedIteration(reg, crit, opt, fixed, **kw)
    assert graphs[name].fused_similarity == (not name.startswith("c_"))
rates = {k: [] for k in graphs}
for _ in range(a.rounds):
    for k, g in graphs.items():
        for _ in range(20):
            g()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.replays):
            g()
        torch.cuda.synchronize()
        rates[k].append(a.replays / (time.perf_counter() - t0))
emit(kind="graphed_iterations_per_s", poses=1, volume=D, detector=H, replays=a.replays, rounds=a.rounds,
     **{k: statistics.median(v) for k, v in rates.items()},
     **{k + "_spread": [min(v), max(v)] for k, v in rates.items()},
     note="host clock around the replays, ended by a device synchronise; median of the rounds")

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
