"""What tests/test_polyrigid.py (host emulation) and tests/test_gpu_polyrigid.py (MI355X) share: the host build of
csrc/polyrigid_core.h, the scenes, the float64 yardsticks and the checks themselves, written once for either
device.

The gate follows the project's rule (warp_cases.gate): ``polyrigid_reference`` evaluated in float32 on the CPU has
an error of its own against ``polyrigid_reference`` in float64; the kernels may be off by at most twice that, plus
a floor of 1e-6 of the compared tensor's scale (max |reference|)."""
import copy
import functools
import os
import subprocess

import torch

from conftest import ROOT
from diffdrr_amd import PolyRigidDeformation, _lib, polyrigid_reference, polyrigid_warp, twist_lattice
from diffdrr_amd.data import phantom_volume
from diffdrr_amd.deformation import dense_field
from diffdrr_amd.polyrigid import SERIES_BELOW, displacement_field
from warp_cases import CASES, KINDS, PADDINGS, chain_scene, gate, recovery_loop, recovery_scene, render_with_density

EMU_SRC = os.path.join(ROOT, "tests", "emu", "polyrigid_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "_build", "libpolyrigid_emu.so")
PITCH = (0.8, 1.0, 2.5)
# amplitude -> (bodies, |omega| <= . rad, |v| <= . mm).  "lever" bounds the rotation by LEVER_MM over the distance
# of the volume's corners from its centre: the corners move by a few voxels whatever the shape.  The fixed bounds
# move the ends of an axis of 65535 voxels by thousands of voxels, where one float32 ulp of the displacement
# (5e-4 voxel at 4096) is more than the 1e-4 voxel that near_face_fraction asks of a sample's distance to a voxel
# face: the float32 reference then guesses the side, and with border padding, where such samples still interpolate
# along the long axis, its own error -- the gate -- is 1e-3 .. 3e-1 of scale in the lattice gradients.  The kernels
# form the position in double, but from the float32 twist lattice, whose own rounding times such a lever is 1e-4
# voxel: they sit at up to 9e-3 and 1.4e-1 there.  "lever" is where the gate on the long shapes is tight.
AMPLITUDES = {"small": (1, 0.05, 1.5), "large": (3, 0.3, 6.0), "lever": (2, None, 1.5)}
LEVER_MM = 3.0
LONG = ("5x6x600", "6x5x515", "3x4x1024", "65535x2x3", "3x65535x2", "2x3x65535")  # the shapes "lever" runs on
# (case, kind, padding, amplitude): every shape at the small amplitude; at the large one every shape but 2x2x2
# (there every sample leaves the volume, W = 0 and there is no scale to gate against); the long shapes at "lever"
VALUE_CASES = [(c, k, p, a) for a in ("small", "large") for c in CASES for k in KINDS for p in PADDINGS
               if not (c == "2x2x2" and a == "large")] + \
    [(c, k, p, "lever") for c in LONG for k in KINDS for p in PADDINGS]
SEED = 2100  # (with it every large scene has more than 0.2 of its samples outside the volume)
KW = dict(parameterization="euler_angles", convention="ZXY")


@functools.lru_cache(maxsize=None)
def emu_library():
    """The host build of the entries (tests/emu/polyrigid_emu.cpp), bound through the product's own binding."""
    csrc = os.path.join(ROOT, "diffdrr_amd", "csrc")
    deps = [EMU_SRC] + [os.path.join(ROOT, "include", f) for f in ("diffdrr_polyrigid_hip.h", "diffdrr_warp_hip.h")] + [
        os.path.join(csrc, f) for f in ("polyrigid_core.h", "warp_core.h", "ddrr_common.h")]
    if not (os.path.exists(EMU_SO) and all(os.path.getmtime(d) <= os.path.getmtime(EMU_SO) for d in deps)):
        os.makedirs(os.path.dirname(EMU_SO), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-mfma", "-ffp-contract=off",
                        "-Wno-unknown-pragmas", EMU_SRC, "-o", EMU_SO], check=True)
    return _lib.polyrigid_library(EMU_SO)


def route_polyrigid_to_emulation(monkeypatch, ops):
    """The launcher patch of the host tests: ops' polyrigid launches go to the host build."""
    lib = emu_library()
    monkeypatch.setattr(ops, "_launch_polyrigid", lambda name, device, *a: lib.call(name, *a, None))
    monkeypatch.setattr(ops, "_query_polyrigid", lambda name, *a: lib.query(name, *a))


# ------------------------------------------------------------------------------------------------ scenes
def bounded(g, n, bound):
    """n seeded 3-vectors of norm in [0.9, 1] * bound."""
    d = torch.randn(n, 3, generator=g)
    return d / d.norm(dim=1, keepdim=True) * bound * (0.9 + 0.1 * torch.rand(n, 1, generator=g))


def random_weights(g, K, grid):
    """rand^3 + 1e-3, normalised over the bodies: most nodes belong mostly to one body."""
    w = torch.rand(K, *grid, generator=g) ** 3 + 1e-3
    return w / w.sum(0, keepdim=True)


@functools.lru_cache(maxsize=None)
def scene(case, kind, amplitude):
    """(V, theta, weights, gW) float32 on the CPU, seeded: the volume, the bodies' twists within the amplitude's
    bounds, their lattice weights, a uniform upstream gradient.  Shared by every test of the case; never modified."""
    dims, grid = CASES[case]
    K, rotation, translation = AMPLITUDES[amplitude]
    if rotation is None:
        rotation = LEVER_MM / (0.5 * sum((h * (D - 1)) ** 2 for h, D in zip(PITCH, dims)) ** 0.5)
    g = torch.Generator().manual_seed(SEED + 7 * len(case) + K + (kind == "phantom"))
    V = torch.rand(*dims, generator=g) if kind == "noise" else phantom_volume(dims, seed=3).contiguous()
    theta = torch.cat((bounded(g, K, rotation), bounded(g, K, translation)), dim=1)
    weights = random_weights(g, K, grid)
    gW = torch.rand(*dims, generator=g)
    return V, theta, weights, gW


@functools.lru_cache(maxsize=None)
def seam_scene():
    """23 x 30 x 37 noise, two bodies that turn about one axis by 1.5 rad -/+ 0.05 %: s = |omega|^2 of a voxel's
    blended twist falls below the seam of A, B, C (the series) or above it (the closed forms) with its weights."""
    dims, grid = CASES["23x30x37"]
    g = torch.Generator().manual_seed(31)
    V = torch.rand(*dims, generator=g)
    axis = torch.tensor([0.48, -0.6, 0.64])  # (a unit vector)
    phi = SERIES_BELOW ** 0.5
    theta = torch.zeros(2, 6)
    theta[0, :3], theta[1, :3] = axis * phi * (1 - 5e-4), axis * phi * (1 + 5e-4)
    theta[:, 3:] = bounded(g, 2, 1.5)
    return V, theta, random_weights(g, 2, grid), torch.rand(*dims, generator=g)


def sample_positions(theta, weights, dims, pitch=PITCH):
    """(u, p = x + u(x)), each (3, Dx, Dy, Dz), in float64."""
    u = displacement_field(twist_lattice(theta.double(), weights.double()), dims, pitch)
    return u, torch.stack([torch.arange(D, dtype=torch.float64).reshape([-1 if d == a else 1 for d in range(3)])
                           + u[a] for a, D in enumerate(dims)])


def near_face_fraction(p):
    """Share of the sample coordinates (float64) within 1e-4 voxel of a voxel face (an integer), where the twist
    gradient jumps."""
    return float(((p - p.round()).abs() < 1e-4).double().mean())


def outside_fraction(p, dims):
    """Share of the samples with a corner outside the volume."""
    return float((sum((p[a] < 0) | (p[a] > dims[a] - 1) for a in range(3)) > 0).double().mean())


def reference(V, theta, weights, gW, padding, dtype, pitch=PITCH):
    """(W, gV, g theta, g weights) of ``polyrigid_reference`` in `dtype` on the CPU, as float64 tensors."""
    V, theta, weights = (t.detach().to(dtype, copy=True).requires_grad_() for t in (V, theta, weights))
    W = polyrigid_reference(V, theta, weights, pitch, padding)
    grads = torch.autograd.grad(W, (V, theta, weights), gW.to(dtype))
    return (W.detach().double(), *(t.double() for t in grads))


def yardstick_of(tensors, padding, pitch=PITCH):
    """The float64 definition of a scene and the float32 reference's own error against it."""
    r64 = reference(*tensors, padding, torch.float64, pitch)
    r32 = reference(*tensors, padding, torch.float32, pitch)
    return r64, tuple(float((a - b).abs().max()) for a, b in zip(r32, r64))


@functools.lru_cache(maxsize=None)
def yardstick(case, kind, padding, amplitude):
    """(computed once per case, never modified)"""
    return yardstick_of(scene(case, kind, amplitude), padding)


@functools.lru_cache(maxsize=None)
def seam_yardstick(padding):
    return yardstick_of(seam_scene(), padding)


def kernels(tensors, padding, device, pitch=PITCH):
    """(W, gV, g theta, g weights) of ``polyrigid_warp`` on `device`."""
    V, theta, weights, gW = tensors
    Vd, td, wd = (t.detach().to(device, copy=True).requires_grad_() for t in (V, theta, weights))
    W = polyrigid_warp(Vd, td, wd, pitch, padding)
    assert W.shape == V.shape and W.dtype == torch.float32 and W.requires_grad
    return (W.detach(), *torch.autograd.grad(W, (Vd, td, wd), gW.to(device)))


WHAT = ("W", "gV", "g theta", "g weights")


def gate_all(name, got, r64, own, which=WHAT):
    for what, a, b, e in zip(WHAT, got, r64, own):
        if what in which:
            gate(name, what, a, b, e)


def check_value_and_gradients(case, kind, padding, amplitude, device):
    """W, gV, g theta and g weights of one case on `device` against the float64 definition, gated by the float32
    reference's own error."""
    tensors = scene(case, kind, amplitude)
    dims, _ = CASES[case]
    u, p = sample_positions(tensors[1], tensors[2], dims)
    share = near_face_fraction(p)
    name = f"{case} {kind} {padding} {amplitude}"
    print(f"{name}: largest displacement {float(u.abs().max()):.1f} voxels, share of sample coordinates within 1e-4 "
          f"voxel of a face {share:.1e}")
    assert share <= 1e-3
    if amplitude == "large":  # the case is about samples that leave the volume: many must
        outside = outside_fraction(p, dims)
        print(f"{name}: share of samples with a corner outside the volume {outside:.2f}")
        assert outside > 0.2
    r64, own = yardstick(case, kind, padding, amplitude)
    gate_all(name, kernels(tensors, padding, device), r64, own)


def check_identity(case, padding, device):
    """theta = 0: W is V bit for bit, and g theta (the series of A, B, C at s = 0: no 0 / 0) is finite and passes
    the gate."""
    for kind in KINDS:
        V, theta, weights, gW = scene(case, kind, "large" if case != "2x2x2" else "small")
        tensors = (V, torch.zeros_like(theta), weights, gW)
        got = kernels(tensors, padding, device)
        assert torch.equal(got[0], V.to(device))
        assert bool(torch.isfinite(got[2]).all())
        r64, own = yardstick_of(tensors, padding)
        gate_all(f"{case} {kind} {padding} identity", got, r64, own, which=("g theta", "g weights"))


def check_seam(padding, device):
    """Two bodies whose |omega|^2 is just below and just above the seam between the series and the closed forms of
    A, B, C: value and every gradient pass the gate."""
    tensors = seam_scene()
    dims, _ = CASES["23x30x37"]
    below = float((rotation_squared(tensors[1], tensors[2], dims) < SERIES_BELOW).double().mean())
    print(f"seam {padding}: share of voxels on the series side {below:.2f}")
    assert 0.1 < below < 0.9
    assert near_face_fraction(sample_positions(tensors[1], tensors[2], dims)[1]) <= 1e-3
    r64, own = seam_yardstick(padding)
    gate_all(f"seam {padding}", kernels(tensors, padding, device), r64, own)


def rotation_squared(theta, weights, dims):
    """s = |omega(x)|^2 at every voxel (float64)."""
    return dense_field(twist_lattice(theta.double(), weights.double()), dims)[:3].pow(2).sum(0)


def check_exact_translation(device):
    """K = 1, pitch 1, omega = 0, v = (2, -1, 3), zeros padding: W is V shifted by v, zeros shifted in, bit for
    bit (the interpolation of a constant lattice is exact)."""
    dims, grid = CASES["23x30x37"]
    V = scene("23x30x37", "noise", "small")[0]
    shift = (2, -1, 3)
    theta = torch.tensor([[0.0, 0.0, 0.0, *map(float, shift)]])
    weights = random_weights(torch.Generator().manual_seed(4), 1, grid)
    assert torch.equal(weights, torch.ones_like(weights))
    expect = torch.zeros_like(V)
    src, dst = [], []
    for d, D in zip(shift, dims):  # W[x] = V[x + v]
        dst.append(slice(max(0, -d), min(D, D - d)))
        src.append(slice(max(0, d), min(D, D + d)))
    expect[tuple(dst)] = V[tuple(src)]
    W = polyrigid_warp(V.to(device), theta.to(device), weights.to(device), (1.0, 1.0, 1.0), "zeros")
    assert torch.equal(W.cpu(), expect)


def check_reproducible(device, ops):
    """Forward and the twist gradient, each run twice, agree bit for bit (several pieces per cell, with tails)."""
    for case in ("40x36x130", "23x30x37", "5x6x600", "3x4x1024"):
        V, theta, weights, gW = (t.to(device) for t in scene(case, "noise", "large"))
        Xi = twist_lattice(theta, weights)
        for padding in PADDINGS:
            a, b = (ops.polyrigid_forward(V, Xi, PITCH, padding) for _ in range(2))
            assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
            a, b = (ops.polyrigid_backward_twists(V, Xi, gW, PITCH, padding) for _ in range(2))
            assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ through the renderer
@functools.lru_cache(maxsize=None)
def chain_bodies():
    """K = 3 on a 4^3 lattice at 0.3 of the large amplitude, for warp_cases.chain_scene."""
    g = torch.Generator().manual_seed(78)
    _, rotation, translation = AMPLITUDES["large"]
    theta = 0.3 * torch.cat((bounded(g, 3, rotation), bounded(g, 3, translation)), dim=1)
    return theta, random_weights(g, 3, (4, 4, 4))


_chain_yardsticks = {}


def check_chain_through_siddon(device):
    """d/d theta of (PolyRigidDeformation(...)(rot, xyz) * fixed_random).sum() through the Siddon renderer against
    the float64 route (the float64 render of polyrigid_reference), gated by the error of the float32 torch
    composition (polyrigid_reference in float32) in front of the same float32 renderer."""
    drr_cpu, rot, xyz, _, weight = chain_scene()
    theta, weights = chain_bodies()
    drr = copy.deepcopy(drr_cpu).to(device)
    rot, xyz, weight = rot.to(device), xyz.to(device), weight.to(device)
    module = PolyRigidDeformation(drr, weights)
    if str(device) not in _chain_yardsticks:  # (once per device, never modified)
        d64 = copy.deepcopy(drr).to(torch.float64)
        t64 = theta.double().to(device).requires_grad_()
        img64 = render_with_density(d64, polyrigid_reference(d64.density, t64, weights.double().to(device), module.pitch),
                                    rot.double(), xyz.double(), **KW)
        g64, = torch.autograd.grad((img64 * weight.double()).sum(), t64)
        t32 = theta.to(device).requires_grad_()
        img32 = render_with_density(drr, polyrigid_reference(drr.density, t32, weights.to(device), module.pitch), rot,
                                    xyz, **KW)
        g32, = torch.autograd.grad((img32 * weight).sum(), t32)
        _chain_yardsticks[str(device)] = (g64.cpu(), float((g32.double().cpu() - g64.cpu()).abs().max()),
                                          img64.detach().cpu())
    g64, own, img64 = _chain_yardsticks[str(device)]
    with torch.no_grad():
        module.rotation.copy_(theta[:, :3].to(device))
        module.translation.copy_(theta[:, 3:].to(device))
    theirs = drr.density
    img = module(rot, xyz, **KW)
    assert drr.density is theirs and not theirs.requires_grad  # drr's own volume is put back, untouched
    assert img.shape == (2, 1, 30, 26)
    assert float((img.detach().double().cpu() - img64).abs().max()) <= 1e-4 * float(img64.abs().max())
    (img * weight).sum().backward()
    got = torch.cat((module.rotation.grad, module.translation.grad), dim=1)
    gate("chain 40^3 -> 30x26, 2 poses", "d loss / d theta", got, g64, own)


# ------------------------------------------------------------------------------------------------ recovery
TRUTH = torch.tensor([[0.10, -0.05, 0.08, 1.5, -1.0, 0.5], [-0.08, 0.12, 0.03, -1.0, 0.8, 1.2], [0.0] * 6])
MOVING = torch.tensor([[1.0], [1.0], [0.0]])  # the background body is held at zero: a mask on the gradient


def three_bodies(grid=(6, 6, 6)):
    """Two Gaussian blobs of width 0.35 at (-0.4, 0, 0) and (0.45, 0.1, 0) in lattice coordinates of [-1, 1]^3 and
    a background of max(1 - their sum, 0.02), normalised over the bodies -> (3, Gx, Gy, Gz)."""
    axes = torch.meshgrid(*(torch.linspace(-1, 1, g) for g in grid), indexing="ij")
    blobs = [torch.exp(-sum((x - c) ** 2 for x, c in zip(axes, centre)) / (2 * 0.35 ** 2))
             for centre in ((-0.4, 0.0, 0.0), (0.45, 0.1, 0.0))]
    w = torch.stack(blobs + [(1 - sum(blobs)).clamp(min=0.02)])
    return w / w.sum(0, keepdim=True)


def check_recovery_volume_to_volume(device):
    """A 24^3 phantom, 1 mm pitch, a 6^3 lattice, three bodies (three_bodies), truth TRUTH with the background
    held at zero, start zero, Adam at lr 0.02 on the MSE between warped volumes: the loss falls to <= 1 % of its
    start within 150 steps."""
    V = phantom_volume(24, seed=3).contiguous().to(device)
    weights, mask = three_bodies().to(device), MOVING.to(device)
    with torch.no_grad():
        target = polyrigid_warp(V, TRUTH.to(device), weights)
    theta = torch.zeros(3, 6, device=device, requires_grad=True)
    theta.register_hook(lambda g: g * mask)
    opt = torch.optim.Adam([theta], lr=0.02)
    first = last = None
    for step in range(1, 151):
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(polyrigid_warp(V, theta, weights), target)
        loss.backward()
        opt.step()
        last = float(loss.detach())
        first = last if first is None else first
        if last <= 0.01 * first:
            break
    error = float((theta.detach() - TRUTH.to(device)).abs().max())
    print(f"volume-to-volume recovery: loss {first:.3e} -> {last:.3e} ({last / first:.2%}) at step {step}, "
          f"largest parameter error {error:.1e}")
    assert last <= 0.01 * first, (first, last)


RECOVERY_LR, RECOVERY_STEPS = 0.02, 60
# the truth through the DRR: TRUTH scaled to |omega| <= 0.06 rad and |v| <= 1.5 mm
DRR_TRUTH = torch.cat((TRUTH[:, :3] * (0.06 / float(TRUTH[:, :3].norm(dim=1).max())),
                       TRUTH[:, 3:] * (1.5 / float(TRUTH[:, 3:].norm(dim=1).max()))), dim=1)


def recovery_float64_ratio(device):
    """The float64 route of the loop of check_recovery_through_drr: polyrigid_reference in front of the float64
    renderer."""
    drr, _, rot, xyz = recovery_scene(device, torch.float64)
    weights, mask = three_bodies().double().to(device), MOVING.double().to(device)
    with torch.no_grad():
        measured = render_with_density(drr, polyrigid_reference(drr.density, DRR_TRUTH.double().to(device), weights),
                                       rot, xyz, **KW)
    theta = torch.zeros(3, 6, dtype=torch.float64, device=device, requires_grad=True)
    theta.register_hook(lambda g: g * mask)
    first, last = recovery_loop(lambda t: torch.nn.functional.mse_loss(
        render_with_density(drr, polyrigid_reference(drr.density, t, weights), rot, xyz, **KW), measured), theta,
        RECOVERY_STEPS, RECOVERY_LR)
    return last / first


# final / first data loss of recovery_float64_ratio on the host emulation (tests/test_polyrigid.py runs it again
# and compares); the kernels' loop may end at three times that
RECOVERY_FLOAT64_RATIO = 3.8451e-2
RECOVERY_GATE = 3 * RECOVERY_FLOAT64_RATIO


def check_recovery_through_drr(device):
    """A 32^3 phantom, a 40 x 40 detector, 6 views over 180 degrees, the three bodies of three_bodies on a 6^3
    lattice, truth DRR_TRUTH with the background held at zero, start zero, Adam at lr RECOVERY_LR on the MSE of
    the views: after RECOVERY_STEPS steps the data loss is at most three times what the float64 route of the same
    loop (polyrigid_reference in front of the float64 renderer) reaches on the host emulation."""
    drr, _, rot, xyz = recovery_scene(device)
    module = PolyRigidDeformation(drr, three_bodies())
    mask = MOVING.to(device)
    for p in (module.rotation, module.translation):
        p.register_hook(lambda g: g * mask)
    with torch.no_grad():
        module.rotation.copy_(DRR_TRUTH[:, :3].to(device))
        module.translation.copy_(DRR_TRUTH[:, 3:].to(device))
        measured = module(rot, xyz, **KW)
        module.rotation.zero_()
        module.translation.zero_()
    opt = torch.optim.Adam([module.rotation, module.translation], lr=RECOVERY_LR)
    first = last = None
    for _ in range(RECOVERY_STEPS):
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(module(rot, xyz, **KW), measured)
        loss.backward()
        opt.step()
        last = float(loss.detach())
        first = last if first is None else first
    print(f"recovery through the DRR: data loss {first:.3e} -> {last:.3e} (ratio {last / first:.3e}; float64 loop "
          f"{RECOVERY_FLOAT64_RATIO:.3e}, gate {RECOVERY_GATE:.3e})")
    assert last <= RECOVERY_GATE * first, (first, last)
