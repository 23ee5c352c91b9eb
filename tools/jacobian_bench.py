"""The Jacobian determinant kernels on one MI355X against the float32 torch composition they replace
(`volume_penalty_reference` with autograd: a dense (3, 3, Dx, Dy, Dz) derivative field, a determinant map, both kept
for backward), on the same device in the same run:

  * the determinant map, the fused penalty forward, and penalty forward + backward, at 256^3 and 512^3 with
    lattices of 16^3 and 32^3 nodes, both bases: ms (HIP events, median of --reps after warm-up) and peak memory
    above the inputs;
  * the composition's forward and forward + backward where it fits in memory (an out-of-memory error is recorded
    as such, not hidden).
Prints one JSON line per configuration; --out FILE also writes them as text."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffdrr_amd import ops, volume_penalty, volume_penalty_reference  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--volumes", type=int, nargs="+", default=[256, 512])
ap.add_argument("--lattices", type=int, nargs="+", default=[16, 32])
ap.add_argument("--bases", nargs="+", default=["linear", "bspline"])
ap.add_argument("--eps", type=float, default=0.1)
ap.add_argument("--out", default=os.path.join("profiles", "r07", "jacobian_bench.txt"))
a = ap.parse_args()
assert torch.cuda.is_available(), "jacobian_bench.py measures on the GPU"
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


def peak_above_inputs(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated(dev) - before) / 2**20


for D in a.volumes:
    shape = (D, D, D)
    for G in a.lattices:
        g = torch.Generator().manual_seed(0)
        U = ((torch.rand(3, G, G, G, generator=g) * 2 - 1) * 2.5).to(dev)
        for basis in a.bases:
            def ours():
                u = U.clone().requires_grad_()
                volume_penalty(u, shape, basis, a.eps).backward()
                return u.grad

            def theirs():
                u = U.clone().requires_grad_()
                volume_penalty_reference(u, shape, basis, a.eps).backward()
                return u.grad

            row = dict(kind="jacobian", volume=D, lattice=G, basis=basis, reps=a.reps,
                       map_ms=timed(lambda: ops.jacobian_determinant(U, shape, basis)),
                       penalty_forward_ms=timed(lambda: ops.jacobian_penalty(U, shape, basis, a.eps)),
                       penalty_forward_backward_ms=timed(ours),
                       workspace_mib=ops._query_jacobian("ddrr_jacobian_workspace_bytes", D, D, D, G, G, G,
                                                         ops._JACOBIAN_BASIS[basis]) / 2**20,
                       map_peak_mib=peak_above_inputs(lambda: ops.jacobian_determinant(U, shape, basis)),
                       penalty_forward_backward_peak_mib=peak_above_inputs(ours))
            row["map_gb_s"] = 4 * D ** 3 / row["map_ms"] / 1e6
            try:
                with torch.no_grad():
                    row["torch_forward_ms"] = timed(lambda: volume_penalty_reference(U, shape, basis, a.eps))
                row["torch_forward_backward_ms"] = timed(theirs)
                row["torch_forward_backward_peak_mib"] = peak_above_inputs(theirs)
                gu, gt = ours(), theirs()
                row["gradient_difference_over_max"] = float((gu - gt).abs().max() / gt.abs().max())
                row["speedup_forward_backward"] = row["torch_forward_backward_ms"] / row["penalty_forward_backward_ms"]
            except torch.OutOfMemoryError:
                row["torch"] = "out of memory"
                torch.cuda.empty_cache()
            emit(**row)

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
