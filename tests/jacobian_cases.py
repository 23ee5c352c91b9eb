"""What tests/test_jacobian.py (host emulation) and tests/test_gpu_jacobian.py (MI355X) share: the host build of
csrc/jacobian_core.h, the scenes, the float64 yardsticks and the checks themselves, written once for either
device.  The scheme is tests/bspline_cases.py's.

The gate follows the project's rule: the torch definition evaluated in float32 on the CPU has an error of its own
against the same in float64; the kernels may be off by at most twice that, plus a floor of 1e-6 of the compared
quantity's scale.  For the determinant map the scale is the largest, over the voxels, sum of the magnitudes of the
six products of the expansion; for the penalty the value itself; for gU, per component a,
max_n sum_x sum_b |c_ab(x)| |d J_ab(x) / d U[a, n]| in float64 (the adjoint with absolute weights): the rounding of
a sum is relative to the sum of the magnitudes of its terms, not to what survives their cancellation."""
import functools
import itertools
import os
import subprocess

import torch

import warp_cases
from conftest import ROOT
from diffdrr_amd import (FreeFormDeformation, _lib, field_jacobian, jacobian_determinant, jacobian_reference,
                         jacobian_statistics, volume_penalty, volume_penalty_reference)
from diffdrr_amd.deformation import _cells, bspline_derivative_weights, bspline_weights, volume_penalty_of

EMU_SRC = os.path.join(ROOT, "tests", "emu", "jacobian_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "_build", "libjacobian_emu.so")
FLOOR = 1e-6
BASES = ("linear", "bspline")
AMPLITUDES = (2.5, 12.0)
EPS = 0.1

# name -> (volume, lattice): warp_cases' table without the y limit, and the only shape with B-spline cells whose
# four taps are unclamped on every axis
CASES = {k: warp_cases.CASES[k] for k in ("23x30x37", "9x10x133", "2x2x2", "40x36x130", "5x6x600", "6x5x515",
                                          "3x4x1024", "65535x2x3", "2x3x65535")}
CASES["37x41x45"] = ((37, 41, 45), (7, 6, 8))
SMALL = [c for c in CASES if "65535" not in c]  # the shapes the refined-field check of the yardstick covers
VALUE_CASES = list(itertools.product(CASES, BASES, AMPLITUDES))
REPRODUCIBLE = ("40x36x130", "37x41x45", "5x6x600", "3x4x1024")
# (case, basis, amplitude) that must have more than 20 % of the voxels folded in float64 / none at all
FOLDED_CASES = {("37x41x45", "linear", 12.0), ("6x5x515", "bspline", 12.0)}
UNFOLDED_CASES = {("40x36x130", "bspline", 12.0)}


@functools.lru_cache(maxsize=None)
def emu_library():
    """The host build of the entries (tests/emu/jacobian_emu.cpp), bound through the product's own binding."""
    csrc = os.path.join(ROOT, "diffdrr_amd", "csrc")
    deps = [EMU_SRC] + [os.path.join(ROOT, "include", f) for f in (
        "diffdrr_jacobian_hip.h", "diffdrr_bspline_hip.h", "diffdrr_warp_hip.h")] + [
        os.path.join(csrc, f) for f in ("jacobian_core.h", "bspline_core.h", "warp_core.h", "ddrr_common.h")]
    if not (os.path.exists(EMU_SO) and all(os.path.getmtime(d) <= os.path.getmtime(EMU_SO) for d in deps)):
        os.makedirs(os.path.dirname(EMU_SO), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-mfma", "-ffp-contract=off",
                        "-Wno-unknown-pragmas", EMU_SRC, "-o", EMU_SO], check=True)
    return _lib.jacobian_library(EMU_SO)


def route_jacobian_to_emulation(monkeypatch, ops):
    """The launcher patch of the host tests: ops' Jacobian launches go to the host build."""
    lib = emu_library()
    monkeypatch.setattr(ops, "_launch_jacobian", lambda name, device, *a: lib.call(name, *a, None))
    monkeypatch.setattr(ops, "_query_jacobian", lambda name, *a: lib.query(name, *a))


# ------------------------------------------------------------------------------------------------ scenes
@functools.lru_cache(maxsize=None)
def scene(case, amplitude):
    """(U, gD) float32 on the CPU, seeded: coefficients uniform in +-amplitude voxels, a uniform upstream gradient
    of the map.  Shared by every test of the case; never modified."""
    dims, grid = CASES[case]
    g = torch.Generator().manual_seed(2000 + 7 * len(case) + int(amplitude * 2) + sum(dims))
    U = (torch.rand(3, *grid, generator=g) * 2 - 1) * amplitude
    return U, torch.rand(*dims, generator=g)


def leaf(t, device=None, dtype=None):
    return t.detach().to(device=device, dtype=dtype).clone().requires_grad_()


def cofactors(J):
    """(3, 3, ...) cof_ab = d det / d J_ab."""
    rows = []
    for a in range(3):
        a1, a2 = (a + 1) % 3, (a + 2) % 3
        rows.append(torch.stack([J[a1, (b + 1) % 3] * J[a2, (b + 2) % 3] - J[a1, (b + 2) % 3] * J[a2, (b + 1) % 3]
                                 for b in range(3)]))
    return torch.stack(rows)


def expansion_scale(J):
    """The largest, over the voxels, sum of the magnitudes of the six products of det J."""
    total = 0
    for p in itertools.permutations(range(3)):
        total = total + (J[0, p[0]] * J[1, p[1]] * J[2, p[2]]).abs()
    return float(total.max())


def absolute_adjoint(c, grid, shape, basis):
    """(3, Gx, Gy, Gz): sum_x sum_b |c_ab(x)| |d J_ab(x) / d U[a, n]| in float64 -- the adjoint of field_jacobian
    with every weight replaced by its magnitude (a clamped tap adds to the border node)."""
    lattice = torch.zeros(3, *grid, dtype=torch.float64, requires_grad=True)
    total = 0
    for b in range(3):
        u = lattice
        for axis, D in enumerate(shape):
            G = grid[axis]
            cell, t = _cells(int(D), G, u.device, u.dtype)
            t = t.reshape([-1 if d == axis + 1 else 1 for d in range(4)])
            scale = (G - 1) / (int(D) - 1) if axis == b else 1.0
            if basis == "linear":
                lo, hi = u.index_select(axis + 1, cell), u.index_select(axis + 1, cell + 1)
                u = (hi + lo) * scale if axis == b else (1 - t) * lo + t * hi
            else:
                ws = bspline_derivative_weights(t) if axis == b else bspline_weights(t)
                u = sum(w.abs() * u.index_select(axis + 1, (cell - 1 + k).clamp(0, G - 1))
                        for k, w in enumerate(ws)) * scale
        total = total + (u * c[:, b].abs()).sum()
    spread, = torch.autograd.grad(total, lattice)
    return spread


def reference(U, gD, shape, basis, dtype):
    """(map, gU for gD, penalty, gU of the penalty) of the torch definition in `dtype` on the CPU, as float64."""
    u = leaf(U, dtype=dtype)
    d = jacobian_reference(u, shape, basis)
    gU, = torch.autograd.grad(d, u, gD.to(dtype), retain_graph=True)
    P = volume_penalty_of(d, EPS).mean()
    gP, = torch.autograd.grad(P, u)
    return d.detach().double(), gU.double(), float(P.detach().double()), gP.double()


@functools.lru_cache(maxsize=None)
def yardstick(case, basis, amplitude):
    """The float64 definition of a case, the float32 reference's own errors against it and the scales (once)."""
    dims, grid = CASES[case]
    U, gD = scene(case, amplitude)
    r64 = reference(U, gD, dims, basis, torch.float64)
    r32 = reference(U, gD, dims, basis, torch.float32)
    J = field_jacobian(U.double(), dims, basis) + torch.eye(3, dtype=torch.float64).reshape(3, 3, 1, 1, 1)
    cof = cofactors(J)
    d = r64[0]
    # psi'(d) / N in float64, from autograd of the definition
    dl = d.clone().requires_grad_()
    dpsi, = torch.autograd.grad(volume_penalty_of(dl, EPS).mean(), dl)
    scales = {
        "map": expansion_scale(J),
        "gU": [float(v.max()) for v in absolute_adjoint(cof * gD.double(), grid, dims, basis)],
        "gP": [float(v.max()) for v in absolute_adjoint(cof * dpsi, grid, dims, basis)],
    }
    own = {
        "map": float((r32[0] - r64[0]).abs().max()),
        "gU": [float((r32[1][a] - r64[1][a]).abs().max()) for a in range(3)],
        "P": abs(r32[2] - r64[2]),
        "gP": [float((r32[3][a] - r64[3][a]).abs().max()) for a in range(3)],
    }
    return r64, own, scales


def gate(name, what, got, ref64, own, scale):
    err = float((torch.as_tensor(got).double().cpu() - ref64).abs().max())
    rel = scale if scale > 0 else 1.0
    print(f"{name}: {what}: kernel error / scale {err / rel:.2e}, float32 reference's {own / rel:.2e}, "
          f"scale {scale:.3e}")
    assert err <= 2 * own + FLOOR * scale, (name, what, err, own, scale)


def check_against_float64(case, basis, amplitude, device):
    """Map, statistics, penalty and both gradients of one case on `device` against the float64 definition."""
    dims, _ = CASES[case]
    U, gD = scene(case, amplitude)
    (d64, gU64, P64, gP64), own, scales = yardstick(case, basis, amplitude)
    name = f"{case} {basis} +-{amplitude}"
    Ud = leaf(U, device)
    d = jacobian_determinant(Ud, dims, basis)
    assert d.shape == tuple(dims) and d.dtype == torch.float32 and d.requires_grad
    gU, = torch.autograd.grad(d, Ud, gD.to(device))
    gate(name, "det", d.detach(), d64, own["map"], scales["map"])
    for a in range(3):
        gate(name, f"gU[{a}]", gU[a], gU64[a], own["gU"][a], scales["gU"][a])
    Up = leaf(U, device)
    P = volume_penalty(Up, dims, basis, EPS)
    assert P.shape == () and P.dtype == torch.float32 and P.requires_grad
    gP, = torch.autograd.grad(P, Up)
    gate(name, "penalty", P.detach(), torch.tensor(P64, dtype=torch.float64), own["P"], abs(P64))
    for a in range(3):
        gate(name, f"gP[{a}]", gP[a], gP64[a], own["gP"][a], scales["gP"][a])
    # statistics, with the map's gate as the tolerance
    tau = 2 * own["map"] + FLOOR * scales["map"]
    stats = jacobian_statistics(U.to(device), dims, basis)
    assert stats.folded.dtype == torch.int64 and stats.folded.device.type == torch.device(device).type
    folded, lo, hi = int(stats.folded), float(stats.minimum), float(stats.maximum)
    share = float((d64 <= 0).double().mean())
    print(f"{name}: folded {folded} of {d64.numel()} ({share:.0%} in float64), d in [{lo:.4g}, {hi:.4g}] "
          f"(float64 [{float(d64.min()):.4g}, {float(d64.max()):.4g}]), tolerance {tau:.2e}")
    assert int((d64 < -tau).sum()) <= folded <= int((d64 <= tau).sum())
    assert abs(lo - float(d64.min())) <= tau and abs(hi - float(d64.max())) <= tau
    if (case, basis, amplitude) in FOLDED_CASES:
        assert share > 0.2, share
    if (case, basis, amplitude) in UNFOLDED_CASES:
        assert share == 0.0 and folded == 0


def check_identity(case, basis, device):
    """A zero lattice: the map is 1.0f everywhere, nothing folds, the penalty and its gradient are exactly 0."""
    dims, grid = CASES[case]
    U = torch.zeros(3, *grid, device=device).requires_grad_()
    d = jacobian_determinant(U, dims, basis)
    assert torch.equal(d.detach(), torch.ones(dims, device=device))
    stats = jacobian_statistics(U.detach(), dims, basis)
    assert int(stats.folded) == 0 and float(stats.minimum) == 1.0 and float(stats.maximum) == 1.0
    P = volume_penalty(U, dims, basis, EPS)
    assert float(P.detach()) == 0.0
    gP, = torch.autograd.grad(P, U)
    assert torch.equal(gP, torch.zeros_like(gP))


def check_reproducible(device, ops):
    """The map, the statistics, the penalty and both gradients, each run twice, agree bit for bit."""
    for case, basis in itertools.product(REPRODUCIBLE, BASES):
        dims, _ = CASES[case]
        U, gD = (t.to(device) for t in scene(case, 12.0))
        for run in (lambda: ops.jacobian_determinant(U, dims, basis), lambda: ops.jacobian_penalty(U, dims, basis, EPS),
                    lambda: (ops.jacobian_backward(U, dims, gD, basis),),
                    lambda: (ops.jacobian_backward(U, dims, None, basis, EPS),)):
            first, second = run(), run()
            for a, b in zip(first, second):
                assert torch.equal(a, b) and bool(torch.isfinite(a.double()).all())
            assert float(first[0].double().abs().max()) > 0


def check_map_and_fused_penalty_agree(case, basis, device, ops):
    """The fused penalty is psi of the kernel's own map, averaged in float64; the two forward modes' statistics
    are equal."""
    dims, _ = CASES[case]
    U = scene(case, 12.0)[0].to(device)
    d, folded, rng = ops.jacobian_determinant(U, dims, basis)
    P, folded2, rng2 = ops.jacobian_penalty(U, dims, basis, EPS)
    want = float(volume_penalty_of(d.double(), EPS).mean())
    print(f"{case} {basis}: fused penalty {float(P):.9g}, psi of the map {want:.9g}")
    assert abs(float(P) - want) <= 1e-6 * abs(want)
    assert torch.equal(folded, folded2) and torch.equal(rng, rng2)
    assert int(folded) == int((d <= 0).sum()) and float(rng[0]) == float(d.min()) and float(rng[1]) == float(d.max())


# ------------------------------------------------------------------------------------------------ unfolding
UNFOLD_CASE, UNFOLD_LR = "23x30x37", 0.2
UNFOLD_STEPS = {"bspline": 50, "linear": 100}


def unfolding_loop(penalty_of, stats_of, U, steps):
    """Adam on ``penalty_of(U)`` alone -> (first penalty, last penalty, folded at the start, folded at the end,
    min det at the end)."""
    opt = torch.optim.Adam([U], lr=UNFOLD_LR)
    start = stats_of(U.detach())
    first = None
    for _ in range(steps):
        opt.zero_grad()
        loss = penalty_of(U)
        first = float(loss.detach()) if first is None else first
        loss.backward()
        opt.step()
    end = stats_of(U.detach())
    return first, float(penalty_of(U).detach()), int(start[0]), int(end[0]), float(end[1])


def unfolding_float64(basis):
    """The float64 torch route of check_unfolding."""
    dims, _ = CASES[UNFOLD_CASE]
    U = leaf(scene(UNFOLD_CASE, 12.0)[0], dtype=torch.float64)

    def stats(u):
        d = jacobian_reference(u, dims, basis)
        return int((d <= 0).sum()), float(d.min())

    return unfolding_loop(lambda u: volume_penalty_reference(u, dims, basis, EPS), stats, U, UNFOLD_STEPS[basis])


# final / first penalty of unfolding_float64 (tests/test_jacobian.py runs it again and compares); the kernels'
# loop may end at three times that
UNFOLD_FLOAT64_RATIO = {"bspline": 1.9238e-2, "linear": 3.1540e-3}


def check_unfolding(basis, device):
    """Adam at lr 0.2 on volume_penalty alone from coefficients uniform in +-12 voxels on 23x30x37 / (4, 5, 3): the
    penalty ratio is at most three times the float64 route's; the B-spline ends unfolded with min det > eps, the
    linear lattice with no more folded voxels than at the start."""
    dims, _ = CASES[UNFOLD_CASE]
    U = leaf(scene(UNFOLD_CASE, 12.0)[0], device)

    def stats(u):
        s = jacobian_statistics(u, dims, basis)
        return int(s.folded), float(s.minimum)

    first, last, before, after, lowest = unfolding_loop(lambda u: volume_penalty(u, dims, basis, EPS), stats, U,
                                                        UNFOLD_STEPS[basis])
    print(f"unfolding {basis}: penalty {first:.4e} -> {last:.4e} (ratio {last / first:.3e}; float64 loop "
          f"{UNFOLD_FLOAT64_RATIO[basis]:.3e}), folded {before} -> {after}, min det {lowest:.3f}")
    assert last <= 3 * UNFOLD_FLOAT64_RATIO[basis] * first, (first, last)
    if basis == "bspline":
        assert after == 0 and lowest > EPS
    else:
        assert after <= before


# ------------------------------------------------------------------------------------------------ the module
def check_module(device):
    """FreeFormDeformation on an anisotropic volume (spacing 0.5 / 2.0 / 1.25): the determinant is that of
    displacement / pitch; folding() and volume_penalty() reach ``displacement`` in millimetres."""
    from diffdrr_amd import DRR
    from diffdrr_amd.data import make_subject, phantom_volume

    vol = phantom_volume((12, 10, 14), seed=3)
    drr = DRR(make_subject(vol, spacing=(0.5, 2.0, 1.25)), sdd=600.0, height=8, width=8, delx=4.0).to(device)
    dims, grid = (12, 10, 14), (3, 4, 5)
    eye = torch.eye(3, dtype=torch.float64).reshape(3, 3, 1, 1, 1)
    for basis in BASES:
        ffd = FreeFormDeformation(drr, grid=grid, padding="border", basis=basis)
        assert torch.equal(ffd.jacobian_determinant().detach(), torch.ones(dims, device=device))
        g = torch.Generator().manual_seed(11)
        with torch.no_grad():
            ffd.displacement.copy_(((torch.rand(3, *grid, generator=g) * 2 - 1) * 3.0).to(device))
        pitch = ffd.pitch.cpu()
        mm = ffd.displacement.detach().cpu()
        # the definition on displacement / pitch, in float64 and (for the gate) in float32
        ref = {}
        for dtype in (torch.float64, torch.float32):
            u = leaf(mm, dtype=dtype)
            d = jacobian_reference(u / pitch.to(dtype), dims, basis)
            P = volume_penalty_of(d, EPS).mean()
            gP, = torch.autograd.grad(P, u)
            ref[dtype] = (d.detach().double(), float(P.detach().double()), gP.double())
        (d64, P64, g64), (d32, P32, g32) = ref[torch.float64], ref[torch.float32]
        J = field_jacobian(mm.double() / pitch.double(), dims, basis) + eye
        name = f"module {basis}"
        d = ffd.jacobian_determinant()
        gate(name, "det", d.detach(), d64, float((d32 - d64).abs().max()), expansion_scale(J))
        stats, dd = ffd.folding(), d.detach()
        assert int(stats.folded) == int((dd <= 0).sum()) and float(stats.minimum) == float(dd.min())
        assert float(stats.maximum) == float(dd.max())
        P = ffd.volume_penalty()
        gate(name, "penalty", P.detach(), torch.tensor(P64, dtype=torch.float64), abs(P32 - P64), abs(P64))
        P.backward()
        dl = d64.clone().requires_grad_()
        dpsi, = torch.autograd.grad(volume_penalty_of(dl, EPS).mean(), dl)
        spread = absolute_adjoint(cofactors(J) * dpsi, grid, dims, basis) / pitch.double()
        for a in range(3):  # d / d millimetres = d / d voxels / pitch
            gate(name, f"d penalty / d displacement[{a}]", ffd.displacement.grad[a], g64[a],
                 float((g32[a] - g64[a]).abs().max()), float(spread[a].max()))
        ffd.displacement.grad = None
        (d * d).sum().backward()
        assert bool(torch.isfinite(ffd.displacement.grad).all()) and float(ffd.displacement.grad.abs().max()) > 0
