"""What the Python side of the fused Euler-pose calls costs, without a GPU: ``ops._launch`` is a no-op and the size
queries go to the host build of the kernels (tests/emu), so the clock sees the module, autograd and ops layers alone --
the share of ``ms_per_step`` that bench.py reports as ``roofline.step_minus_kernel_ms``.  Two calls, 40^3 phantom ->
30 x 26, two poses, fp32 bricks:
  * the fused step: ``drr.ncc(fixed, rot, xyz, reduction="sum")`` + ``backward(gradient=one)``
  * the inference call: ``drr(rot, xyz, parameterization="euler_angles")`` under ``no_grad``
7 repetitions of 300 calls after 50 warm-up calls; every repetition is printed (us per call), then one JSON line.
(Development tool, CPU.  The numbers in the buffers are whatever ``torch.empty`` left: nothing here reads them.)"""
import gc
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import build_emu  # noqa: E402
from diffdrr_amd import DRR, ops  # noqa: E402
from diffdrr_amd._lib import DdrrLibrary  # noqa: E402
from diffdrr_amd.data import synthetic_subject  # noqa: E402

REPS, CALLS, WARMUP = 7, 300, 50
torch.set_num_threads(1)  # (tiny host tensors: a thread pool only adds jitter)

emu = DdrrLibrary(build_emu())
ops._require_gpu = lambda volume: None
ops.on_device = lambda t: True
ops._launch = lambda name, device, *a: None
ops._query = lambda name, *a: emu.query(name, *a)

drr = DRR(synthetic_subject(40, kind="phantom", seed=3), sdd=600.0, height=30, width=26, delx=3.0)
drr.renderer.brick_storage = "f32"
rot = torch.tensor([[0.1, -0.2, 0.05], [0.0, 0.15, -0.1]], requires_grad=True)
xyz = torch.tensor([[2.0, 400.0, -3.0], [0.0, 395.0, 1.0]], requires_grad=True)
fixed = torch.rand(1, 1, 30, 26)
one = torch.ones(())


def fused_step():
    rot.grad = xyz.grad = None
    drr.ncc(fixed, rot, xyz, reduction="sum").backward(gradient=one)


def inference_call():
    with torch.no_grad():
        drr(rot, xyz, parameterization="euler_angles", convention="ZXY")


def clock(call):
    for _ in range(WARMUP):
        call()
    reps = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            call()
        reps.append((time.perf_counter() - t0) / CALLS * 1e6)
    return reps


gc.collect()
gc.disable()
result = {}
for name, call in (("fused_step", fused_step), ("inference_call", inference_call)):
    reps = clock(call)
    result[name + "_us"] = [round(t, 1) for t in reps]
    print(f"{name}: " + " ".join(f"{t:.1f}" for t in reps) + f"  us per call (min {min(reps):.1f})", flush=True)
print(json.dumps(result))
