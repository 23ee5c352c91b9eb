"""What tests/test_warp.py (host emulation) and tests/test_gpu_warp.py (MI355X) share: the host build of
csrc/warp_core.h, the scenes, the float64 yardsticks and the checks themselves, written once for either device.

The gate follows the project's rule: the definition evaluated in float32 on the CPU has an error of its own
against ``warp_reference`` in float64; the kernels may be off by at most twice that, plus a floor of 1e-6 of the
compared tensor's scale (max |reference|).  The float32 side is ``sample_displaced(V, dense_field(U))``, the same
function with floor and fraction formed from u, as the kernels form them: ``warp_reference`` rounds p = x + u
itself, which costs 2^-8 voxel at x near 65535 -- in float32 a yardstick thousands of times the kernels' error."""
import copy
import functools
import os
import subprocess

import torch

from conftest import ROOT
from diffdrr_amd import DRR, FreeFormDeformation, _lib, warp_reference, warp_volume
from diffdrr_amd.data import make_subject, phantom_volume
from diffdrr_amd.deformation import dense_field, sample_coordinates, sample_displaced

EMU_SRC = os.path.join(ROOT, "tests", "emu", "warp_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "_build", "libwarp_emu.so")
FLOOR = 1e-6

# name -> (volume, lattice): every shape hits a seam
CASES = {
    "23x30x37": ((23, 30, 37), (4, 5, 3)),       # nothing is a multiple of 4
    "9x10x133": ((9, 10, 133), (2, 3, 17)),      # node spacing 8.25 voxels: cells of unequal extents
    "2x2x2": ((2, 2, 2), (2, 2, 2)),             # the smallest possible case
    "40x36x130": ((40, 36, 130), (3, 3, 5)),     # several workgroups per cell, with tails
    # rows of several 256-voxel z chunks (the B-spline kernels' unit), one node per voxel, the 65535 limit
    "5x6x600": ((5, 6, 600), (3, 4, 7)),         # three z chunks, chunk ends inside cells, nothing a multiple of 4
    "6x5x515": ((6, 5, 515), (2, 5, 515)),       # a node per voxel on y and z, a last chunk of 3 voxels
    "3x4x1024": ((3, 4, 1024), (3, 2, 33)),      # Dz a multiple of 4 and of 256: 16-byte stores, exact chunk ends
    "65535x2x3": ((65535, 2, 3), (9, 2, 2)),     # the limit on x: the longest chains of the lattice gradients
    "3x65535x2": ((3, 65535, 2), (2, 65535, 2)),  # the limit on y with a node per voxel
    "2x3x65535": ((2, 3, 65535), (2, 3, 700)),   # the limit on z: 256 chunks per row
}
KINDS = ("noise", "phantom")
PADDINGS = ("zeros", "border")
# (case, kind, padding, amplitude in voxels): the table above at +-2.5, one case per padding at +-12
VALUE_CASES = [(c, k, p, 2.5) for c in CASES for k in KINDS for p in PADDINGS] + \
    [("23x30x37", "noise", "zeros", 12.0), ("23x30x37", "noise", "border", 12.0)]


@functools.lru_cache(maxsize=None)
def emu_library():
    """The host build of the entries (tests/emu/warp_emu.cpp), bound through the product's own binding."""
    csrc = os.path.join(ROOT, "diffdrr_amd", "csrc")
    deps = [EMU_SRC, os.path.join(ROOT, "include", "diffdrr_warp_hip.h")] + [
        os.path.join(csrc, f) for f in ("warp_core.h", "ddrr_common.h")]
    if not (os.path.exists(EMU_SO) and all(os.path.getmtime(d) <= os.path.getmtime(EMU_SO) for d in deps)):
        os.makedirs(os.path.dirname(EMU_SO), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-mfma", "-ffp-contract=off",
                        "-Wno-unknown-pragmas", EMU_SRC, "-o", EMU_SO], check=True)
    return _lib.warp_library(EMU_SO)


def route_warp_to_emulation(monkeypatch, ops):
    """The launcher patch of the host tests: ops' warp launches go to the host build."""
    lib = emu_library()
    monkeypatch.setattr(ops, "_launch_warp", lambda name, device, *a: lib.call(name, *a, None))
    monkeypatch.setattr(ops, "_query_warp", lambda name, *a: lib.query(name, *a))


# ------------------------------------------------------------------------------------------------ scenes
@functools.lru_cache(maxsize=None)
def scene(case, kind, amplitude):
    """(V, U, gW) float32 on the CPU, seeded: the volume, a lattice uniform in +-amplitude voxels, a uniform
    upstream gradient.  Shared by every test of the case; never modified."""
    dims, grid = CASES[case]
    g = torch.Generator().manual_seed(1000 + 7 * len(case) + int(amplitude * 2) + (kind == "phantom"))
    V = torch.rand(*dims, generator=g) if kind == "noise" else phantom_volume(dims, seed=3).contiguous()
    U = (torch.rand(3, *grid, generator=g) * 2 - 1) * amplitude
    gW = torch.rand(*dims, generator=g)
    return V, U, gW


def near_face_fraction(U64, dims):
    """Share of the sample coordinates x + u (float64) within 1e-4 voxel of a voxel face (an integer), where
    the lattice gradient jumps."""
    u = dense_field(U64, dims)
    near = 0
    for a, D in enumerate(dims):
        x = torch.arange(D, dtype=torch.float64).reshape([-1 if d == a else 1 for d in range(3)])
        p = x + u[a]
        near += int(((p - p.round()).abs() < 1e-4).sum())
    return near / (3 * u[0].numel())


def reference(V, U, gW, padding, dtype):
    """(W, gV, gU) of the definition in `dtype` on the CPU, as float64 tensors: ``warp_reference`` in float64,
    ``sample_displaced(V, dense_field(U))`` in float32 (the module's docstring says why)."""
    V, U = V.to(dtype).requires_grad_(), U.to(dtype).requires_grad_()
    W = warp_reference(V, U, padding) if dtype == torch.float64 else \
        sample_displaced(V, dense_field(U, V.shape), padding)
    gV, gU = torch.autograd.grad(W, (V, U), gW.to(dtype))
    return W.detach().double(), gV.double(), gU.double()


@functools.lru_cache(maxsize=None)
def yardstick(case, kind, padding, amplitude):
    """The float64 definition of a case and the float32 reference's own error against it (computed once)."""
    V, U, gW = scene(case, kind, amplitude)
    r64 = reference(V, U, gW, padding, torch.float64)
    r32 = reference(V, U, gW, padding, torch.float32)
    own = tuple(float((a - b).abs().max()) for a, b in zip(r32, r64))
    return r64, own


def gate(name, what, got, ref64, own):
    err, scale = float((got.double().cpu() - ref64).abs().max()), float(ref64.abs().max())
    rel = scale if scale > 0 else 1.0
    print(f"{name}: {what}: kernel error / scale {err / rel:.2e}, float32 reference's {own / rel:.2e}")
    assert err <= 2 * own + FLOOR * scale, (name, what, err, own, scale)


def check_value_and_gradients(case, kind, padding, amplitude, device):
    """W, gV and gU of one case on `device` against the float64 definition, gated by the float32 reference's
    own error."""
    V, U, gW = scene(case, kind, amplitude)
    dims, _ = CASES[case]
    share = near_face_fraction(U.double(), dims)
    print(f"{case} {kind} +-{amplitude}: share of sample coordinates within 1e-4 voxel of a face {share:.1e}")
    assert share <= 1e-3
    (W64, gV64, gU64), own = yardstick(case, kind, padding, amplitude)
    Vd, Ud = V.to(device).requires_grad_(), U.to(device).requires_grad_()
    W = warp_volume(Vd, Ud, padding)
    assert W.shape == V.shape and W.dtype == torch.float32 and W.requires_grad
    gV, gU = torch.autograd.grad(W, (Vd, Ud), gW.to(device))
    name = f"{case} {kind} {padding} +-{amplitude}"
    gate(name, "W", W.detach(), W64, own[0])
    gate(name, "gV", gV, gV64, own[1])
    gate(name, "gU", gU, gU64, own[2])
    if amplitude > 10:  # the case is about samples that leave the volume: many must
        p = sample_coordinates(U.double(), dims)
        outside = sum((p[a] < 0) | (p[a] > dims[a] - 1) for a in range(3)) > 0
        print(f"{name}: share of samples with a corner outside the volume {float(outside.double().mean()):.2f}")
        assert float(outside.double().mean()) > 0.2


def forward_difference_gradient(V, gW, grid, padding):
    """gU at the identity lattice, from its definition in float64: sum_x hat_n(x) gW[x] (V[x + e_a] - V[x]),
    the voxel past the end being 0 (zeros) or the last voxel again (border)."""
    V, gW = V.double(), gW.double()
    U = torch.zeros(3, *grid, dtype=torch.float64, requires_grad=True)
    u = dense_field(U, V.shape)  # linear in U: its adjoint spreads a dense field over the nodes
    diffs = []
    for a in range(3):
        nxt = torch.roll(V, -1, dims=a)
        last = [slice(None)] * 3
        last[a] = -1
        nxt[tuple(last)] = 0.0 if padding == "zeros" else V[tuple(last)]
        diffs.append(gW * (nxt - V))
    return torch.autograd.grad((u * torch.stack(diffs)).sum(), U)[0]


def check_identity(case, kind, padding, device):
    """u = 0: W is V bit for bit; gU is the forward-difference convention's."""
    V, _, gW = scene(case, kind, 2.5)
    dims, grid = CASES[case]
    U = torch.zeros(3, *grid)
    Vd, Ud = V.to(device), U.to(device).requires_grad_()
    W = warp_volume(Vd, Ud, padding)
    assert torch.equal(W.detach(), Vd)
    gU, = torch.autograd.grad(W, Ud, gW.to(device))
    _, _, gU64 = reference(V, U, gW, padding, torch.float64)
    _, _, gU32 = reference(V, U, gW, padding, torch.float32)
    direct = forward_difference_gradient(V, gW, grid, padding)
    assert float((direct - gU64).abs().max()) <= 1e-12 * max(float(gU64.abs().max()), 1.0)
    gate(f"{case} {kind} {padding} identity", "gU", gU, gU64, float((gU32 - gU64).abs().max()))


def check_reproducible(device, ops):
    """Forward and the lattice gradient, each run twice, agree bit for bit (several workgroups per cell; rows of
    several z chunks, with and without 16-byte stores)."""
    for case in ("40x36x130", "23x30x37", "5x6x600", "3x4x1024"):
        V, U, gW = (t.to(device) for t in scene(case, "noise", 2.5))
        for padding in PADDINGS:
            assert torch.equal(ops.warp_forward(V, U, padding), ops.warp_forward(V, U, padding))
            a = ops.warp_backward_displacement(V, U, gW, padding)
            b = ops.warp_backward_displacement(V, U, gW, padding)
            assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ through the renderer
def render_with_density(drr, density, *pose, **kw):
    """``drr`` renders ``density`` instead of its own volume (as FreeFormDeformation.forward does)."""
    buffers = drr._buffers
    theirs = buffers["density"]
    buffers["density"] = density
    try:
        return drr(*pose, **kw)
    finally:
        buffers["density"] = theirs


@functools.lru_cache(maxsize=None)
def chain_scene():
    drr = DRR(make_subject(phantom_volume(40, seed=3)), sdd=600.0, height=30, width=26, delx=3.0)
    g = torch.Generator().manual_seed(77)
    rot = (torch.rand(2, 3, generator=g) - 0.5) * 0.6
    xyz = torch.tensor([0.0, 400.0, 0.0]) + (torch.rand(2, 3, generator=g) - 0.5) * 20
    U = (torch.rand(3, 4, 4, 4, generator=g) * 2 - 1) * 2.5
    weight = torch.rand(2, 1, 30, 26, generator=g)
    return drr, rot, xyz, U, weight


_chain_yardsticks = {}


def check_chain_through_siddon(device):
    """d/d lattice of (FreeFormDeformation(...)(rot, xyz) * fixed_random).sum() through the Siddon renderer
    against the float64 route (the float64 render of warp_reference), gated by the error of the float32 torch
    composition (warp_reference in float32) in front of the same float32 renderer."""
    drr_cpu, rot, xyz, U, weight = chain_scene()
    kw = dict(parameterization="euler_angles", convention="ZXY")
    drr = copy.deepcopy(drr_cpu).to(device)
    rot, xyz, weight = rot.to(device), xyz.to(device), weight.to(device)
    if str(device) not in _chain_yardsticks:  # (once per device, never modified)
        d64 = copy.deepcopy(drr).to(torch.float64)
        U64 = U.double().to(device).requires_grad_()
        img64 = render_with_density(d64, warp_reference(d64.density, U64), rot.double(), xyz.double(), **kw)
        g64, = torch.autograd.grad((img64 * weight.double()).sum(), U64)
        U32 = U.to(device).requires_grad_()
        img32 = render_with_density(drr, warp_reference(drr.density, U32), rot, xyz, **kw)
        g32, = torch.autograd.grad((img32 * weight).sum(), U32)
        _chain_yardsticks[str(device)] = (g64.cpu(), float((g32.double().cpu() - g64.cpu()).abs().max()),
                                          img64.detach().cpu())
    g64, own, img64 = _chain_yardsticks[str(device)]
    ffd = FreeFormDeformation(drr, grid=(4, 4, 4))
    with torch.no_grad():
        ffd.displacement.copy_(U.to(device))  # (1 mm voxels: millimetres are voxels)
    theirs = drr.density
    img = ffd(rot, xyz, **kw)
    assert drr.density is theirs and not theirs.requires_grad  # drr's own volume is put back, untouched
    assert img.shape == (2, 1, 30, 26)
    assert float((img.detach().double().cpu() - img64).abs().max()) <= 1e-4 * float(img64.abs().max())
    (img * weight).sum().backward()
    gate("chain 40^3 -> 30x26, 2 poses", "d loss / d lattice", ffd.displacement.grad, g64, own)


# ------------------------------------------------------------------------------------------------ recovery
def check_recovery_volume_to_volume(device):
    """A 24^3 phantom, a 4^3 lattice, truth uniform in +-1.5 voxels, start zero, Adam at lr 0.1 on the MSE
    between warped volumes: the loss falls to <= 1 % of its start within 100 steps."""
    g = torch.Generator().manual_seed(5)
    V = phantom_volume(24, seed=3).contiguous().to(device)
    truth = ((torch.rand(3, 4, 4, 4, generator=g) * 2 - 1) * 1.5).to(device)
    with torch.no_grad():
        target = warp_volume(V, truth)
    U = torch.zeros_like(truth).requires_grad_()
    opt = torch.optim.Adam([U], lr=0.1)
    first = last = None
    for step in range(1, 101):
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(warp_volume(V, U), target)
        loss.backward()
        opt.step()
        last = float(loss.detach())
        first = last if first is None else first
        if last <= 0.01 * first:
            break
    print(f"volume-to-volume recovery: loss {first:.3e} -> {last:.3e} ({last / first:.2%}) at step {step}")
    assert last <= 0.01 * first, (first, last)


RECOVERY_LR, RECOVERY_STEPS = 0.2, 60


def recovery_scene(device, dtype=torch.float32):
    """A 32^3 phantom (1 mm voxels), a 40 x 40 detector, 6 views over 180 degrees, truth +-1.5 mm on 4^3."""
    drr = DRR(make_subject(phantom_volume(32, seed=3)), sdd=600.0, height=40, width=40, delx=1.5).to(device)
    drr = drr.to(dtype)
    g = torch.Generator().manual_seed(9)
    truth = ((torch.rand(3, 4, 4, 4, generator=g) * 2 - 1) * 1.5).to(device=device, dtype=dtype)
    rot = torch.zeros(6, 3, device=device, dtype=dtype)
    rot[:, 0] = torch.arange(6, device=device, dtype=dtype) * (torch.pi / 6)
    xyz = torch.tensor([[0.0, 400.0, 0.0]], device=device, dtype=dtype).repeat(6, 1)
    return drr, truth, rot, xyz


def recovery_loop(loss_of, U, steps=RECOVERY_STEPS, lr=RECOVERY_LR):
    """Adam on ``loss_of(U)`` -> (first loss, last loss)."""
    opt = torch.optim.Adam([U], lr=lr)
    first = last = None
    for _ in range(steps):
        opt.zero_grad()
        loss = loss_of(U)
        loss.backward()
        opt.step()
        last = float(loss.detach())
        first = last if first is None else first
    return first, last


def recovery_float64_ratio(device):
    """The float64 route of the loop of check_recovery_through_drr: warp_reference in front of the float64
    renderer."""
    kw = dict(parameterization="euler_angles", convention="ZXY")
    drr, truth, rot, xyz = recovery_scene(device, torch.float64)
    with torch.no_grad():
        measured = render_with_density(drr, warp_reference(drr.density, truth), rot, xyz, **kw)
    U = torch.zeros_like(truth).requires_grad_()
    first, last = recovery_loop(lambda u: torch.nn.functional.mse_loss(
        render_with_density(drr, warp_reference(drr.density, u), rot, xyz, **kw), measured), U)
    return last / first


# final / first data loss of recovery_float64_ratio on the host emulation (tests/test_warp.py runs it again and
# compares); the kernels' loop may end at three times that
RECOVERY_FLOAT64_RATIO = 1.6773e-3
RECOVERY_GATE = 3 * RECOVERY_FLOAT64_RATIO


def check_recovery_through_drr(device):
    """A 32^3 phantom, a 40 x 40 detector, 6 views over 180 degrees, truth uniform in +-1.5 mm on a 4^3 lattice,
    start zero, Adam at lr 0.2 on the MSE of the views: after 60 steps the data loss is at most 5.03e-3 of
    its start -- three times the 1.6773e-3 the float64 route of the same loop (warp_reference in front of
    the float64 renderer) reaches on the host emulation."""
    drr, truth, rot, xyz = recovery_scene(device)
    kw = dict(parameterization="euler_angles", convention="ZXY")
    ffd = FreeFormDeformation(drr, grid=(4, 4, 4))
    with torch.no_grad():
        ffd.displacement.copy_(truth)
        measured = ffd(rot, xyz, **kw)
        ffd.displacement.zero_()
    first, last = recovery_loop(lambda u: torch.nn.functional.mse_loss(ffd(rot, xyz, **kw), measured),
                                ffd.displacement)
    print(f"recovery through the DRR: data loss {first:.3e} -> {last:.3e} (ratio {last / first:.3e}; float64 loop "
          f"{RECOVERY_FLOAT64_RATIO:.3e}, gate {RECOVERY_GATE:.3e})")
    assert last <= RECOVERY_GATE * first, (first, last)
