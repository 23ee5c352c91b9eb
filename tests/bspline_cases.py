"""What tests/test_bspline.py (host emulation) and tests/test_gpu_bspline.py (MI355X) share: the host build of
csrc/bspline_core.h, the scenes, the float64 yardsticks and the checks themselves, written once for either
device.  The scheme is tests/warp_cases.py's, with ``basis="bspline"``.

The gate follows the project's rule: ``warp_reference(..., basis="bspline")`` evaluated in float32 on the CPU has
an error of its own against the same in float64; the kernels may be off by at most twice that, plus a floor of
1e-6 of the compared tensor's scale.  For W and gV the scale is max |reference|.  For gU it is, per component a,
max_n sum_x |B_n(x) gW[x] d_a V(p(x))| in float64: the rounding of a sum is relative to the sum of the
magnitudes of its terms, not to what survives their cancellation (on noise, most does not)."""
import copy
import functools
import os
import subprocess

import torch

import warp_cases
from conftest import ROOT
from diffdrr_amd import FreeFormDeformation, _lib, warp_reference, warp_volume
from diffdrr_amd.data import phantom_volume
from diffdrr_amd.deformation import dense_field, sample_coordinates, sample_displaced
from warp_cases import KINDS, PADDINGS, recovery_loop, recovery_scene, render_with_density  # noqa: F401

EMU_SRC = os.path.join(ROOT, "tests", "emu", "bspline_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "_build", "libbspline_emu.so")
FLOOR = 1e-6
BASIS = "bspline"

# name -> (volume, lattice): warp_cases' table, and the only shape with cells whose four taps are all unclamped
# on every axis
CASES = dict(warp_cases.CASES)
CASES["37x41x45"] = ((37, 41, 45), (7, 6, 8))
# (case, kind, padding, amplitude of the coefficients in voxels): the table at +-2.5; two shapes at +-24 (the
# spline shrinks random coefficients: +-12 would leave most samples inside the volume)
VALUE_CASES = [(c, k, p, 2.5) for c in CASES for k in KINDS for p in PADDINGS] + \
    [(c, "noise", p, 24.0) for c in ("23x30x37", "37x41x45") for p in PADDINGS]


@functools.lru_cache(maxsize=None)
def emu_library():
    """The host build of the entries (tests/emu/bspline_emu.cpp), bound through the product's own binding."""
    csrc = os.path.join(ROOT, "diffdrr_amd", "csrc")
    deps = [EMU_SRC] + [os.path.join(ROOT, "include", f) for f in ("diffdrr_bspline_hip.h", "diffdrr_warp_hip.h")] + [
        os.path.join(csrc, f) for f in ("bspline_core.h", "warp_core.h", "ddrr_common.h")]
    if not (os.path.exists(EMU_SO) and all(os.path.getmtime(d) <= os.path.getmtime(EMU_SO) for d in deps)):
        os.makedirs(os.path.dirname(EMU_SO), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-mfma", "-ffp-contract=off",
                        "-Wno-unknown-pragmas", EMU_SRC, "-o", EMU_SO], check=True)
    return _lib.bspline_library(EMU_SO)


def route_bspline_to_emulation(monkeypatch, ops):
    """The launcher patch of the host tests: ops' B-spline launches go to the host build."""
    lib = emu_library()
    monkeypatch.setattr(ops, "_launch_bspline", lambda name, device, *a: lib.call(name, *a, None))
    monkeypatch.setattr(ops, "_query_bspline", lambda name, *a: lib.query(name, *a))


# ------------------------------------------------------------------------------------------------ scenes
@functools.lru_cache(maxsize=None)
def scene(case, kind, amplitude):
    """(V, U, gW) float32 on the CPU, seeded and drawn as warp_cases.scene does: the volume, coefficients
    uniform in +-amplitude voxels, a uniform upstream gradient.  Shared by every test of the case; never
    modified."""
    dims, grid = CASES[case]
    g = torch.Generator().manual_seed(1000 + 7 * len(case) + int(amplitude * 2) + (kind == "phantom"))
    V = torch.rand(*dims, generator=g) if kind == "noise" else phantom_volume(dims, seed=3).contiguous()
    U = (torch.rand(3, *grid, generator=g) * 2 - 1) * amplitude
    gW = torch.rand(*dims, generator=g)
    return V, U, gW


def leaf(t, device=None, dtype=None):
    """A copy of a shared scene tensor that takes a gradient (the scene's own tensors are never modified)."""
    return t.detach().to(device=device, dtype=dtype).clone().requires_grad_()


def near_face_fraction(U64, dims):
    """Share of the sample coordinates x + u (float64) within 1e-4 voxel of a voxel face (an integer), where
    the coefficient gradient jumps."""
    u = dense_field(U64, dims, BASIS)
    near = 0
    for a, D in enumerate(dims):
        x = torch.arange(D, dtype=torch.float64).reshape([-1 if d == a else 1 for d in range(3)])
        p = x + u[a]
        near += int(((p - p.round()).abs() < 1e-4).sum())
    return near / (3 * u[0].numel())


def reference(V, U, gW, padding, dtype):
    """(W, gV, gU) of ``warp_reference(..., basis="bspline")`` in `dtype` on the CPU, as float64 tensors."""
    V, U = leaf(V, dtype=dtype), leaf(U, dtype=dtype)
    W = warp_reference(V, U, padding, BASIS)
    gV, gU = torch.autograd.grad(W, (V, U), gW.to(dtype))
    return W.detach().double(), gV.double(), gU.double()


def coefficient_gradient_spread(V, U, gW, padding, box=None, part=None):
    """(3, Gx, Gy, Gz): sum_x |B_n(x) gW[x] d_a V(p(x))| in float64.  q = gW dV(p) is the gradient of the
    sampling in the dense field; B_n >= 0, so the adjoint of ``dense_field`` spreads |q| over the nodes.  With
    ``box`` and ``part`` (diffdrr_amd.deformation.sample_displaced) the sum runs over the box's voxels."""
    V, U, gW = V.double(), U.double(), gW.double()
    shape = V.shape if part is None else part[0]
    u = dense_field(U, shape, BASIS, box).requires_grad_()
    q, = torch.autograd.grad(sample_displaced(V, u, padding, box, part), u, gW)
    leaf = torch.zeros_like(U).requires_grad_()
    spread, = torch.autograd.grad((dense_field(leaf, shape, BASIS, box) * q.abs()).sum(), leaf)
    return spread


def coefficient_gradient_scale(V, U, gW, padding):
    """Per component a: the largest entry of :func:`coefficient_gradient_spread` over the nodes."""
    spread = coefficient_gradient_spread(V, U, gW, padding)
    return [float(spread[a].max()) for a in range(3)]


@functools.lru_cache(maxsize=None)
def yardstick(case, kind, padding, amplitude):
    """The float64 definition of a case, the float32 reference's own error against it (gU: per component) and
    the scales of gU (computed once)."""
    V, U, gW = scene(case, kind, amplitude)
    r64 = reference(V, U, gW, padding, torch.float64)
    r32 = reference(V, U, gW, padding, torch.float32)
    own = [float((a - b).abs().max()) for a, b in zip(r32[:2], r64[:2])]
    own_gU = [float((r32[2][a] - r64[2][a]).abs().max()) for a in range(3)]
    return r64, own, own_gU, coefficient_gradient_scale(V, U, gW, padding)


def gate(name, what, got, ref64, own, scale=None):
    err = float((got.double().cpu() - ref64).abs().max())
    scale = float(ref64.abs().max()) if scale is None else scale
    rel = scale if scale > 0 else 1.0
    print(f"{name}: {what}: kernel error / scale {err / rel:.2e}, float32 reference's {own / rel:.2e}, "
          f"scale {scale:.3e}")
    assert err <= 2 * own + FLOOR * scale, (name, what, err, own, scale)


def gate_gU(name, gU, gU64, own_gU, scales):
    for a in range(3):
        gate(name, f"gU[{a}]", gU[a], gU64[a], own_gU[a], scales[a])


def check_value_and_gradients(case, kind, padding, amplitude, device):
    """W, gV and gU of one case on `device` against the float64 definition, gated by the float32 reference's
    own error."""
    V, U, gW = scene(case, kind, amplitude)
    dims, _ = CASES[case]
    share = near_face_fraction(U.double(), dims)
    print(f"{case} {kind} +-{amplitude}: share of sample coordinates within 1e-4 voxel of a face {share:.1e}")
    assert share <= 1e-3
    (W64, gV64, gU64), own, own_gU, scales = yardstick(case, kind, padding, amplitude)
    Vd, Ud = leaf(V, device), leaf(U, device)
    W = warp_volume(Vd, Ud, padding, BASIS)
    assert W.shape == V.shape and W.dtype == torch.float32 and W.requires_grad
    gV, gU = torch.autograd.grad(W, (Vd, Ud), gW.to(device))
    name = f"{case} {kind} {padding} +-{amplitude}"
    gate(name, "W", W.detach(), W64, own[0])
    gate(name, "gV", gV, gV64, own[1])
    gate_gU(name, gU, gU64, own_gU, scales)
    if amplitude > 10:  # the case is about samples that leave the volume: many must
        p = sample_coordinates(U.double(), dims, BASIS)
        outside = sum((p[a] < 0) | (p[a] > dims[a] - 1) for a in range(3)) > 0
        print(f"{name}: share of samples with a corner outside the volume {float(outside.double().mean()):.2f}")
        assert float(outside.double().mean()) > 0.2


def check_identity(case, kind, padding, device):
    """Zero coefficients: W is V bit for bit; gU against the float64 reference."""
    V, _, gW = scene(case, kind, 2.5)
    _, grid = CASES[case]
    U = torch.zeros(3, *grid)
    Vd, Ud = V.to(device), leaf(U, device)
    W = warp_volume(Vd, Ud, padding, BASIS)
    assert torch.equal(W.detach(), Vd)
    gU, = torch.autograd.grad(W, Ud, gW.to(device))
    _, _, gU64 = reference(V, U, gW, padding, torch.float64)
    _, _, gU32 = reference(V, U, gW, padding, torch.float32)
    own_gU = [float((gU32[a] - gU64[a]).abs().max()) for a in range(3)]
    gate_gU(f"{case} {kind} {padding} identity", gU, gU64, own_gU, coefficient_gradient_scale(V, U, gW, padding))


def check_reproducible(device, ops):
    """Forward and the coefficient gradient, each run twice, agree bit for bit (rows of several chunks' worth
    of nodes, tails, interior cells; chains that continue from one z chunk to the next, with and without
    16-byte stores)."""
    for case in ("40x36x130", "37x41x45", "5x6x600", "3x4x1024"):
        V, U, gW = (t.to(device) for t in scene(case, "noise", 2.5))
        for padding in PADDINGS:
            a, b = ops.bspline_forward(V, U, padding), ops.bspline_forward(V, U, padding)
            assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
            a = ops.bspline_backward_displacement(V, U, gW, padding)
            b = ops.bspline_backward_displacement(V, U, gW, padding)
            assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ through the renderer
_chain_yardsticks = {}


def check_chain_through_siddon(device):
    """d/d coefficients of (FreeFormDeformation(..., basis="bspline")(rot, xyz) * fixed_random).sum() through
    the Siddon renderer against the float64 route (the float64 render of warp_reference), gated by the error of
    the float32 torch composition (warp_reference in float32) in front of the same float32 renderer."""
    drr_cpu, rot, xyz, U, weight = warp_cases.chain_scene()
    kw = dict(parameterization="euler_angles", convention="ZXY")
    drr = copy.deepcopy(drr_cpu).to(device)
    rot, xyz, weight = rot.to(device), xyz.to(device), weight.to(device)
    if str(device) not in _chain_yardsticks:  # (once per device, never modified)
        d64 = copy.deepcopy(drr).to(torch.float64)
        U64 = U.double().to(device).requires_grad_()
        img64 = render_with_density(d64, warp_reference(d64.density, U64, basis=BASIS), rot.double(), xyz.double(),
                                    **kw)
        g64, = torch.autograd.grad((img64 * weight.double()).sum(), U64)
        U32 = U.to(device).requires_grad_()
        img32 = render_with_density(drr, warp_reference(drr.density, U32, basis=BASIS), rot, xyz, **kw)
        g32, = torch.autograd.grad((img32 * weight).sum(), U32)
        _chain_yardsticks[str(device)] = (g64.cpu(), float((g32.double().cpu() - g64.cpu()).abs().max()),
                                          img64.detach().cpu())
    g64, own, img64 = _chain_yardsticks[str(device)]
    ffd = FreeFormDeformation(drr, grid=(4, 4, 4), basis=BASIS)
    with torch.no_grad():
        ffd.displacement.copy_(U.to(device))  # (1 mm voxels: millimetres are voxels)
    theirs = drr.density
    img = ffd(rot, xyz, **kw)
    assert drr.density is theirs and not theirs.requires_grad  # drr's own volume is put back, untouched
    assert img.shape == (2, 1, 30, 26)
    assert float((img.detach().double().cpu() - img64).abs().max()) <= 1e-4 * float(img64.abs().max())
    (img * weight).sum().backward()
    gate("chain 40^3 -> 30x26, 2 poses", "d loss / d coefficients", ffd.displacement.grad, g64, own)


# ------------------------------------------------------------------------------------------------ recovery
def recovery_float64_ratio(device):
    """The float64 route of the loop of check_recovery_through_drr: warp_reference(..., basis="bspline") in
    front of the float64 renderer."""
    kw = dict(parameterization="euler_angles", convention="ZXY")
    drr, truth, rot, xyz = recovery_scene(device, torch.float64)
    with torch.no_grad():
        measured = render_with_density(drr, warp_reference(drr.density, truth, basis=BASIS), rot, xyz, **kw)
    U = torch.zeros_like(truth).requires_grad_()
    first, last = recovery_loop(lambda u: torch.nn.functional.mse_loss(
        render_with_density(drr, warp_reference(drr.density, u, basis=BASIS), rot, xyz, **kw), measured), U)
    return last / first


# final / first data loss of recovery_float64_ratio on the host emulation (tests/test_bspline.py runs it again
# and compares); the kernels' loop may end at three times that
RECOVERY_FLOAT64_RATIO = 2.8385e-3
RECOVERY_GATE = 3 * RECOVERY_FLOAT64_RATIO


def check_recovery_through_drr(device):
    """warp_cases.recovery_scene (a 32^3 phantom, a 40 x 40 detector, 6 views over 180 degrees, truth uniform in
    +-1.5 mm on a 4^3 lattice) with the truth generated by the B-spline warp, start zero, Adam at lr 0.2 on the
    MSE of the views: after 60 steps the data loss is at most RECOVERY_GATE of its start -- three times what
    the float64 route of the same loop reaches on the host emulation."""
    drr, truth, rot, xyz = recovery_scene(device)
    kw = dict(parameterization="euler_angles", convention="ZXY")
    ffd = FreeFormDeformation(drr, grid=(4, 4, 4), basis=BASIS)
    with torch.no_grad():
        ffd.displacement.copy_(truth)
        measured = ffd(rot, xyz, **kw)
        ffd.displacement.zero_()
    first, last = recovery_loop(lambda u: torch.nn.functional.mse_loss(ffd(rot, xyz, **kw), measured),
                                ffd.displacement)
    print(f"recovery through the DRR: data loss {first:.3e} -> {last:.3e} (ratio {last / first:.3e}; float64 loop "
          f"{RECOVERY_FLOAT64_RATIO:.3e}, gate {RECOVERY_GATE:.3e})")
    assert last <= RECOVERY_GATE * first, (first, last)
