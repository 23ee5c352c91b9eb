"""The Jacobian determinant of a lattice deformation without a GPU: the definition in float64 torch, checked on its
own against the refined field, and the host build of csrc/jacobian_core.h (tests/emu/jacobian_emu.cpp) behind the
product's own Python layers -- map, statistics, penalty and both gradients against the float64 definition, the
identity lattice, reproducibility, the two forward modes, the unfolding, the module, the errors."""
import pytest
import torch

import diffdrr_amd
import jacobian_cases
from diffdrr_amd import (_lib, dense_field, field_jacobian, jacobian_determinant, jacobian_reference,
                         jacobian_statistics, volume_penalty, volume_penalty_reference)
from diffdrr_amd.deformation import _cells, volume_penalty_of

CPU = torch.device("cpu")
BASES = jacobian_cases.BASES


@pytest.fixture()
def jacobian_ops(emulated_ops, monkeypatch):
    jacobian_cases.route_jacobian_to_emulation(monkeypatch, emulated_ops)
    return emulated_ops


def test_exported_from_the_package():
    for name in ("field_jacobian", "jacobian_reference", "volume_penalty_reference", "jacobian_determinant",
                 "jacobian_statistics", "volume_penalty", "bspline_derivative_weights", "JacobianStatistics"):
        assert callable(getattr(diffdrr_amd, name)), name
    assert _lib.JACOBIAN_ABI_VERSION == 1
    for name in ("jacobian_determinant", "jacobian_penalty", "jacobian_backward", "_check_jacobian",
                 "_launch_jacobian", "_query_jacobian"):
        assert callable(getattr(diffdrr_amd.ops, name)), name
    for name in ("jacobian_determinant", "folding", "volume_penalty"):
        assert callable(getattr(diffdrr_amd.FreeFormDeformation, name)), name


# ------------------------------------------------------------------------------------------------ the definition
def test_derivative_weights_are_the_derivatives_of_the_weights():
    t = torch.linspace(0, 1, 41, dtype=torch.float64, requires_grad=True)
    for B, dB in zip(diffdrr_amd.bspline_weights(t), diffdrr_amd.bspline_derivative_weights(t)):
        g, = torch.autograd.grad(B.sum(), t)
        assert float((g - dB).detach().abs().max()) < 1e-15
    assert float(sum(diffdrr_amd.bspline_derivative_weights(t)).detach().abs().max()) < 1e-15


@pytest.mark.parametrize("basis", BASES)
@pytest.mark.parametrize("case", jacobian_cases.SMALL)
def test_field_jacobian_is_the_derivative_of_the_refined_field(case, basis):
    """Per axis b the field on the shape refined 8 x along b (voxel x is voxel 8 x, in the same cell) under the
    four-point one-sided stencil (-11 f0 + 18 f1 - 9 f2 + 2 f3) / (6 h), h = 1 / 8 -- forward, or backward where
    the forward points would leave the voxel's cell.  The stencil is exact for cubics, hence for both bases
    inside a cell."""
    dims, grid = jacobian_cases.CASES[case]
    U = jacobian_cases.scene(case, 12.0)[0].double()
    J = field_jacobian(U, dims, basis)
    assert J.shape == (3, 3, *dims)
    worst = 0.0
    for b in range(3):
        D, G = dims[b], grid[b]
        fine = list(dims)
        fine[b] = 8 * (D - 1) + 1
        f = dense_field(U, fine, basis)
        cells, _ = _cells(fine[b], G, CPU, torch.float64)
        at = 8 * torch.arange(D)
        forward = (at + 3 <= fine[b] - 1) & (cells[(at + 3).clamp(max=fine[b] - 1)] == cells[at])
        sign = torch.where(forward, 1, -1)
        assert bool((cells[at + 3 * sign] == cells[at]).all())
        taps = [f.index_select(b + 1, at + k * sign) for k in range(4)]
        shape = [-1 if d == b + 1 else 1 for d in range(4)]
        stencil = (-11 * taps[0] + 18 * taps[1] - 9 * taps[2] + 2 * taps[3]) / (6 / 8) * sign.reshape(shape)
        worst = max(worst, float((stencil - J[:, b]).abs().max()))
    print(f"{case} {basis}: field_jacobian against the stencil on the refined field: {worst:.1e}")
    assert worst <= 1e-10


@pytest.mark.parametrize("basis", BASES)
def test_an_affine_lattice_has_the_determinant_of_its_matrix(basis):
    """u_a at node i = sum_b M_ab i_b: det(I + M diag(s)) at every voxel for the linear basis, and at the voxels
    of the cells 1 <= c <= G - 3 for the B-spline (a clamped tap breaks linear reproduction in the border cells)."""
    dims, grid = jacobian_cases.CASES["37x41x45"]
    M = torch.tensor([[0.3, -0.2, 0.1], [0.15, -0.25, 0.05], [-0.1, 0.2, 0.35]], dtype=torch.float64)
    idx = torch.meshgrid(*[torch.arange(g, dtype=torch.float64) for g in grid], indexing="ij")
    U = torch.stack([sum(M[a, b] * idx[b] for b in range(3)) for a in range(3)])
    s = torch.tensor([(g - 1) / (d - 1) for g, d in zip(grid, dims)], dtype=torch.float64)
    want = float(torch.linalg.det(torch.eye(3, dtype=torch.float64) + M * s))
    dev = (jacobian_reference(U, dims, basis) - want).abs()
    inner = torch.ones(dims, dtype=torch.bool)
    if basis == "bspline":
        for a, (D, G) in enumerate(zip(dims, grid)):
            c, _ = _cells(D, G, CPU, torch.float64)
            inner = inner & ((c >= 1) & (c <= G - 3)).reshape([-1 if d == a else 1 for d in range(3)])
        assert bool(inner.any()) and float(dev[~inner].max()) > 1e-3
    print(f"{basis}: det(I + A) = {want:.6f}, deviation {float(dev[inner].max()):.1e}")
    assert float(dev[inner].max()) <= 1e-12


def test_the_penalty_is_twice_differentiable_at_eps_and_finite_below_zero():
    eps = 0.1
    # 1e-9 either side of eps: a jump would be of the order of psi' (46), psi'' (660); continuity leaves the
    # next derivative times 2e-9
    d = torch.tensor([eps - 1e-9, eps + 1e-9], dtype=torch.float64, requires_grad=True)
    psi = volume_penalty_of(d, eps)
    g, = torch.autograd.grad(psi.sum(), d, create_graph=True)
    h, = torch.autograd.grad(g.sum(), d)
    psi, g = psi.detach(), g.detach()
    assert abs(float(psi[0] - psi[1])) < 1e-6 and abs(float(g[0] - g[1])) < 1e-5 and abs(float(h[0] - h[1])) < 1e-3
    below = volume_penalty_of(torch.tensor([-3.0, 0.0], dtype=torch.float64), eps)
    assert bool(torch.isfinite(below).all()) and float(below[0]) > float(below[1]) > 0
    assert float(volume_penalty_of(torch.ones(1), eps)) == 0.0


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("case,basis,amplitude", jacobian_cases.VALUE_CASES)
def test_map_statistics_penalty_and_gradients_against_float64(jacobian_ops, case, basis, amplitude):
    jacobian_cases.check_against_float64(case, basis, amplitude, CPU)


@pytest.mark.parametrize("basis", BASES)
@pytest.mark.parametrize("case", sorted(jacobian_cases.CASES))
def test_identity_lattice_is_exact(jacobian_ops, case, basis):
    jacobian_cases.check_identity(case, basis, CPU)


def test_everything_is_reproducible(jacobian_ops):
    jacobian_cases.check_reproducible(CPU, jacobian_ops)


@pytest.mark.parametrize("basis", BASES)
@pytest.mark.parametrize("case", jacobian_cases.REPRODUCIBLE)
def test_map_and_fused_penalty_agree(jacobian_ops, case, basis):
    jacobian_cases.check_map_and_fused_penalty_agree(case, basis, CPU, jacobian_ops)


@pytest.mark.parametrize("basis", BASES)
def test_unfolding(jacobian_ops, basis):
    jacobian_cases.check_unfolding(basis, CPU)


@pytest.mark.parametrize("basis", BASES)
def test_unfolding_gate_is_three_times_the_float64_loop(basis):
    """The gate of the unfolding is derived, not chosen: three times the final ratio of the float64 torch route
    of the same loop, run here."""
    first, last, before, after, lowest = jacobian_cases.unfolding_float64(basis)
    print(f"float64 loop, {basis}: penalty ratio {last / first:.4e}, folded {before} -> {after}, min det {lowest:.3f}")
    want = jacobian_cases.UNFOLD_FLOAT64_RATIO[basis]
    assert abs(last / first - want) <= 0.05 * want
    assert after < before and (basis == "linear" or (after == 0 and lowest > jacobian_cases.EPS))


def test_module(jacobian_ops):
    jacobian_cases.check_module(CPU)


# ------------------------------------------------------------------------------------------------ errors
def test_domain_errors_name_the_condition(jacobian_ops, monkeypatch):
    U = torch.zeros(3, 2, 3, 4)
    shape = (6, 7, 8)
    jacobian_determinant(U, shape)
    for fn in (jacobian_determinant, jacobian_statistics, volume_penalty):
        with pytest.raises(ValueError, match="basis.*'cubic'"):
            fn(U, shape, "cubic")
        with pytest.raises(ValueError, match="float32"):
            fn(U.double(), shape)
        with pytest.raises(ValueError, match=r"\(Dx, Dy, Dz\)"):
            fn(U, shape[:2])
        with pytest.raises(ValueError, match=r"\(3, Gx, Gy, Gz\)"):
            fn(U[:2], shape)
        with pytest.raises(ValueError, match="G_a <= D_a"):
            fn(torch.zeros(3, 7, 3, 4), shape)
        with pytest.raises(ValueError, match="65535"):
            fn(torch.zeros(3, 2, 2, 2), (2, 2, 65536))
        with pytest.raises(ValueError, match="contiguous"):
            fn(torch.zeros(3, 3, 2, 4).transpose(1, 2), shape)
    for eps in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"eps must be in \(0, 1\]"):
            volume_penalty(U, shape, eps=eps)
        with pytest.raises(ValueError, match=r"eps must be in \(0, 1\]"):
            volume_penalty_reference(U, shape, eps=eps)
    with pytest.raises(ValueError, match="basis.*'cubic'"):
        field_jacobian(U, shape, "cubic")
    with pytest.raises(ValueError, match=r"2\^31 voxels"):
        diffdrr_amd.ops._check_jacobian("jacobian_determinant", (2048, 2048, 513), torch.zeros(3, 2, 2, 2), "linear")
    with pytest.raises(ValueError, match="grad_out has shape"):
        diffdrr_amd.ops.jacobian_backward(U, shape, torch.zeros(6, 7, 7))
    # the module: eps = 0, and a CPU tensor -- there is no CPU fallback
    from diffdrr_amd import DRR, FreeFormDeformation
    from diffdrr_amd.data import make_subject

    ffd = FreeFormDeformation(DRR(make_subject(torch.rand(*shape)), sdd=600.0, height=8, delx=4.0), grid=(2, 3, 4))
    with pytest.raises(ValueError, match=r"eps must be in \(0, 1\]"):
        ffd.volume_penalty(eps=0)
    monkeypatch.setattr(diffdrr_amd.ops, "on_device", lambda t: t.is_cuda)
    for call in (ffd.jacobian_determinant, ffd.folding, ffd.volume_penalty, lambda: jacobian_determinant(U, shape)):
        with pytest.raises(ValueError, match="GPU only"):
            call()
