"""Polyrigid deformation on one MI355X: `polyrigid_warp`'s three kernels against the torch composition of the same
warp (`polyrigid_reference`: a dense twist field, a dense displacement, an eight-corner gather) on the same device:

  * forward, twist gradient and volume gradient at 256^3 and 512^3 with lattice spacings of 16 and 32 voxels and
    K = 8 bodies: ms per kernel (HIP events, median of --reps after warm-up), GB/s of the compulsory traffic, and
    peak memory of forward + backward above the inputs, for both.  `fused_peak_volumes` is the fused route's peak
    in units of the volume's size: beside the inputs (V, gW) it may allocate W and gV and nothing else of that size;
  * one deformable iteration at 512^3 -> 256^2 and 8 views: `PolyRigidDeformation` forward, MSE, backward, Adam.
Prints one JSON line per measurement; --out FILE also writes them as text.  Exits non-zero if the fused route's peak
is more than W, gV, the workspace, eight tensors of the twist lattice's size and 1 MiB: a third tensor of the volume's
size would be 512 MiB at 512^3, where that allowance is 7 MiB with a 32^3 lattice."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffdrr_amd import DRR, PolyRigidDeformation, ops, polyrigid_reference, polyrigid_warp, twist_lattice  # noqa: E402
from diffdrr_amd.data import make_subject, phantom_volume  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--volumes", type=int, nargs="+", default=[256, 512])
ap.add_argument("--spacings", type=int, nargs="+", default=[16, 32])
ap.add_argument("--bodies", type=int, default=8)
ap.add_argument("--views", type=int, default=8)
ap.add_argument("--detector", type=int, default=256)
ap.add_argument("--out", default=os.path.join("profiles", "r07", "polyrigid_bench.txt"))
a = ap.parse_args()
assert torch.cuda.is_available(), "polyrigid_bench.py measures on the GPU"
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


def peak_above_inputs(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated(dev) - before) / 2**20


def bodies(K, G, g):
    """K twists of up to 0.1 rad and 3 mm and their weights on a G^3 lattice (rand^3 + 1e-3, normalised)."""
    theta = torch.cat(((torch.rand(K, 3, generator=g) * 2 - 1) * 0.1, (torch.rand(K, 3, generator=g) * 2 - 1) * 3.0), 1)
    w = torch.rand(K, G, G, G, generator=g) ** 3 + 1e-3
    return theta.to(dev), (w / w.sum(0, keepdim=True)).to(dev)


for D in a.volumes:
    g = torch.Generator().manual_seed(0)
    V = torch.rand(D, D, D, generator=g).to(dev)
    gW = torch.rand(D, D, D, generator=g).to(dev)
    for spacing in a.spacings:
        G = (D - 1) // spacing + 1
        theta, weights = bodies(a.bodies, G, g)
        Xi = twist_lattice(theta, weights)
        n = D ** 3
        t_fwd = timed(lambda: ops.polyrigid_forward(V, Xi))
        t_gx = timed(lambda: ops.polyrigid_backward_twists(V, Xi, gW))
        t_gv = timed(lambda: ops.polyrigid_backward_volume(Xi, gW))

        def ours():
            v, t = V.detach().requires_grad_(), theta.detach().requires_grad_()
            polyrigid_warp(v, t, weights).backward(gW)

        def theirs():
            v, t = V.detach().requires_grad_(), theta.detach().requires_grad_()
            polyrigid_reference(v, t, weights).backward(gW)

        few = max(3, a.reps // 4)
        t_ours, t_theirs = timed(ours, reps=few), timed(theirs, reps=few, warmup=1)
        t_theirs_fwd = timed(lambda: polyrigid_reference(V, theta, weights), reps=few, warmup=1)
        peak = peak_above_inputs(ours)
        ws_mib = ops._query_polyrigid("ddrr_polyrigid_workspace_bytes", D, D, D, G, G, G) / 2**20
        # what the route allocates by design beside W and gV: the workspace, and tensors of the twist lattice's size
        # (Xi, gXi and what torch's einsum and its adjoint hold: 8 of them are allowed for), plus 1 MiB
        small_mib = ws_mib + 8 * Xi.numel() * 4 / 2**20 + 1.0
        emit(kind="kernels", volume=D, lattice=G, spacing=spacing, bodies=a.bodies, forward_ms=t_fwd,
             forward_gb_s=8 * n / t_fwd / 1e6, twist_gradient_ms=t_gx, volume_gradient_ms=t_gv,
             volume_gradient_atomic_gb_s=32 * n / t_gv / 1e6, forward_backward_ms=t_ours,
             torch_forward_ms=t_theirs_fwd, torch_forward_backward_ms=t_theirs, peak_mib=peak,
             workspace_mib=ws_mib, fused_peak_volumes=peak / (4 * n / 2**20),
             lattice_mib=Xi.numel() * 4 / 2**20,
             fused_peak_is_W_and_gV=bool(peak <= 2 * 4 * n / 2**20 + small_mib),
             torch_peak_mib=peak_above_inputs(theirs),
             note="peaks are forward + backward above the inputs (V, gW, theta, weights); fused_peak_is_W_and_gV: the "
                  "fused route's peak is at most two volumes (W, gV), the twist gradient's workspace, eight tensors of "
                  "the twist lattice's size and 1 MiB")
    del V, gW

D, H = max(a.volumes), a.detector
drr = DRR(make_subject(phantom_volume(D, seed=0)), sdd=1020.0, height=H, delx=2.4 * 256 / H).to(dev)
theta, weights = bodies(a.bodies, (D - 1) // 32 + 1, torch.Generator().manual_seed(1))
module = PolyRigidDeformation(drr, weights)
rot = torch.zeros(a.views, 3, device=dev)
rot[:, 0] = torch.arange(a.views, device=dev) * (torch.pi / a.views)
xyz = torch.tensor([[0.0, 850.0, 0.0]], device=dev).repeat(a.views, 1)
kw = dict(parameterization="euler_angles", convention="ZXY")
with torch.no_grad():
    module.rotation.copy_(0.3 * theta[:, :3])
    module.translation.copy_(0.3 * theta[:, 3:])
    measured = module(rot, xyz, **kw)
    module.rotation.zero_()
    module.translation.zero_()
opt = torch.optim.Adam(module.parameters(), lr=0.01)


def iteration():
    opt.zero_grad(set_to_none=True)
    F.mse_loss(module(rot, xyz, **kw), measured).backward()
    opt.step()


emit(kind="deformable_iteration", volume=D, detector=H, views=a.views, lattice=weights.shape[1], bodies=a.bodies,
     iteration_ms=timed(iteration), peak_mib=peak_above_inputs(iteration))

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
# the structural claim: beside its inputs the fused route allocates W and gV and nothing else of the volume's size
broken = [(line["volume"], line["lattice"]) for line in lines if not line.get("fused_peak_is_W_and_gV", True)]
if broken:
    sys.exit(f"the fused route's peak memory exceeds W + gV + workspace + lattice tensors at (volume, lattice) {broken}")
