"""Cubic B-spline free-form deformation without a GPU: the definition in float64 torch, and the host build of
csrc/bspline_core.h (tests/emu/bspline_emu.cpp) behind the product's own Python layers -- value and both
gradients against the float64 definition, the identity lattice, reproducibility, the chain through the Siddon
renderer, the recovery, the module, the errors."""
import pytest
import torch

import bspline_cases
import diffdrr_amd
from diffdrr_amd import DRR, FreeFormDeformation, _lib, warp_reference, warp_volume
from diffdrr_amd.data import make_subject, phantom_volume
from diffdrr_amd.deformation import _cells, dense_field

CPU = torch.device("cpu")
BASIS = bspline_cases.BASIS


@pytest.fixture()
def bspline_ops(emulated_ops, monkeypatch):
    bspline_cases.route_bspline_to_emulation(monkeypatch, emulated_ops)
    return emulated_ops


def test_exported_from_the_package():
    assert diffdrr_amd.dense_field is dense_field and callable(diffdrr_amd.bspline_weights)
    assert _lib.BSPLINE_ABI_VERSION == 1 and callable(diffdrr_amd.ops.bspline_forward)
    assert callable(diffdrr_amd.ops.bspline_backward_displacement) and callable(diffdrr_amd.ops.bspline_backward_volume)


# ------------------------------------------------------------------------------------------------ the definition
def test_weights_are_a_partition_of_unity_and_the_uniform_cubic_b_spline():
    t = torch.linspace(0, 1, 101, dtype=torch.float64)
    B = diffdrr_amd.bspline_weights(t)
    assert float((sum(B) - 1).abs().max()) < 1e-15 and all(float(b.min()) >= 0 for b in B)
    # C^2 across a node: value, first and second derivative of piece k at t = 1 are piece k + 1's at t = 0
    t0 = torch.zeros(1, dtype=torch.float64, requires_grad=True)
    t1 = torch.ones(1, dtype=torch.float64, requires_grad=True)
    for k in range(3):
        a, b = diffdrr_amd.bspline_weights(t1)[k + 1], diffdrr_amd.bspline_weights(t0)[k]
        for _ in range(3):
            assert abs(float(a.detach()) - float(b.detach())) < 1e-15
            a, = torch.autograd.grad(a, t1, create_graph=True)
            b, = torch.autograd.grad(b, t0, create_graph=True)


def test_a_constant_lattice_gives_the_constant_everywhere():
    """Partition of unity, the clamped border taps included (64 products in float64: well below 1e-13)."""
    for dims, grid in bspline_cases.CASES.values():
        u = dense_field(torch.full((3, *grid), 0.7, dtype=torch.float64), dims, BASIS)
        print(f"{dims}: deviation from the constant {float((u - 0.7).abs().max()):.1e}")
        assert float((u - 0.7).abs().max()) <= 1e-13


def test_linear_coefficients_give_the_linear_function_inside_and_not_in_the_border_cells():
    """Coefficients 0.3 (a + 1) i in the node index i of axis a: component a of the field is
    0.3 (a + 1) x (G - 1) / (D - 1) wherever the voxel's cell on that axis has four unclamped taps
    (1 <= c <= G - 3); in the two border cells a tap is clamped and it is not -- which pins the edge rule."""
    dims, grid = bspline_cases.CASES["37x41x45"]
    U = torch.zeros(3, *grid, dtype=torch.float64)
    for a, G in enumerate(grid):
        U[a] = (0.3 * (a + 1) * torch.arange(G, dtype=torch.float64)).reshape([-1 if d == a else 1 for d in range(3)])
    u = dense_field(U, dims, BASIS)
    for a, (D, G) in enumerate(zip(dims, grid)):
        shape = [-1 if d == a else 1 for d in range(3)]
        x = torch.arange(D, dtype=torch.float64)
        dev = (u[a] - (0.3 * (a + 1) * x * (G - 1) / (D - 1)).reshape(shape)).abs()
        c, _ = _cells(D, G, CPU, torch.float64)
        inner = ((c >= 1) & (c <= G - 3)).reshape(shape).expand(dims)
        assert bool(inner.any()) and bool((~inner).any())
        print(f"axis {a}: deviation inside {float(dev[inner].max()):.1e}, in the border cells "
              f"{float(dev[~inner].max()):.1e}")
        assert float(dev[inner].max()) <= 1e-12
        for border in (c == 0, c == G - 2):
            assert float(dev[border.reshape(shape).expand(dims)].max()) > 1e-3


def test_the_field_at_a_node_is_not_its_coefficient():
    """The spline approximates: (c[n - 1] + 4 c[n] + c[n + 1]) / 6 per axis at an inner node."""
    U = torch.zeros(3, 5, 5, 5, dtype=torch.float64)
    U[:, 2, 2, 2] = 1.0
    u = dense_field(U, (9, 9, 9), BASIS)  # node 2 is voxel 4
    assert abs(float(u[0, 4, 4, 4]) - (4 / 6) ** 3) < 1e-15
    assert abs(float(u[0, 2, 4, 4]) - (1 / 6) * (4 / 6) ** 2) < 1e-15


def test_linear_basis_is_bit_for_bit_what_it_was():
    """``basis="linear"`` is the default and the same arithmetic as a call without the keyword."""
    V, U, gW = bspline_cases.scene("23x30x37", "noise", 2.5)
    for padding in bspline_cases.PADDINGS:
        assert torch.equal(warp_reference(V, U, padding), warp_reference(V, U, padding, basis="linear"))
    assert torch.equal(dense_field(U, V.shape), dense_field(U, V.shape, "linear"))
    assert not torch.equal(dense_field(U, V.shape), dense_field(U, V.shape, BASIS))


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("case,kind,padding,amplitude", bspline_cases.VALUE_CASES)
def test_value_and_gradients_against_float64(bspline_ops, case, kind, padding, amplitude):
    bspline_cases.check_value_and_gradients(case, kind, padding, amplitude, CPU)


@pytest.mark.parametrize("padding", bspline_cases.PADDINGS)
@pytest.mark.parametrize("case", sorted(bspline_cases.CASES))
def test_identity_lattice_is_exact(bspline_ops, case, padding):
    for kind in bspline_cases.KINDS:
        bspline_cases.check_identity(case, kind, padding, CPU)


def test_forward_and_coefficient_gradient_are_reproducible(bspline_ops):
    bspline_cases.check_reproducible(CPU, bspline_ops)


def test_coefficient_gradient_through_the_siddon_renderer(bspline_ops):
    bspline_cases.check_chain_through_siddon(CPU)


def test_recovery_through_the_drr(bspline_ops):
    bspline_cases.check_recovery_through_drr(CPU)


def test_recovery_gate_is_three_times_the_float64_loop(bspline_ops):
    """The gate of the recovery through the DRR is derived, not chosen: three times the final ratio of the
    float64 route of the same loop (warp_reference(..., basis="bspline") in front of the float64 renderer), run
    here."""
    ratio = bspline_cases.recovery_float64_ratio(CPU)
    print(f"float64 loop: final / first data loss {ratio:.4e}")
    assert abs(ratio - bspline_cases.RECOVERY_FLOAT64_RATIO) <= 0.05 * bspline_cases.RECOVERY_FLOAT64_RATIO
    assert bspline_cases.RECOVERY_GATE == 3 * bspline_cases.RECOVERY_FLOAT64_RATIO


# ------------------------------------------------------------------------------------------------ the module
def _anisotropic(padding="border", **kw):
    vol = phantom_volume((12, 10, 14), seed=3)
    drr = DRR(make_subject(vol, spacing=(0.5, 2.0, 1.25)), sdd=600.0, height=8, width=8, delx=4.0)
    return drr, FreeFormDeformation(drr, grid=(3, 4, 5), padding=padding, **kw)


def test_module_with_the_bspline_basis(bspline_ops):
    drr, ffd = _anisotropic(basis=BASIS)
    assert ffd.basis == BASIS and list(ffd.parameters()) == [ffd.displacement]
    assert [n for n, _ in ffd.named_buffers(recurse=False)] == ["pitch"]
    assert torch.equal(ffd.warped().detach(), drr.density) and float(ffd.bending_energy().detach()) == 0.0
    with torch.no_grad():
        ffd.displacement[0] = 1.0   # 1 mm along x = 2 voxels of 0.5 mm
        ffd.displacement[1] = 4.0   # 4 mm along y = 2 voxels of 2 mm
    shift = torch.tensor([2.0, 2.0, 0.0]).reshape(3, 1, 1, 1).expand(3, 3, 4, 5)
    # constants survive the spline: the same uniform shift as with the trilinear field
    assert torch.allclose(ffd.warped().detach(), warp_reference(drr.density, shift, "border", BASIS), atol=1e-6)
    assert torch.allclose(ffd.warped().detach(), warp_reference(drr.density, shift, "border"), atol=1e-6)
    theirs = drr.density
    img = ffd(torch.zeros(1, 3), torch.tensor([[0.0, 400.0, 0.0]]), parameterization="euler_angles", convention="ZXY")
    assert img.requires_grad and drr.density is theirs
    img.sum().backward()
    assert ffd.displacement.grad is not None and bool(torch.isfinite(ffd.displacement.grad).all())


def test_bending_energy():
    _, ffd = _anisotropic()
    assert float(ffd.bending_energy().detach()) == 0.0
    i, j, k = torch.meshgrid(torch.arange(3.0), torch.arange(4.0), torch.arange(5.0), indexing="ij")
    with torch.no_grad():  # affine in the node index: no second difference of either kind
        for a in range(3):
            ffd.displacement[a] = 0.5 * a + 0.25 * i - 0.75 * j + (a + 1) * k
    assert abs(float(ffd.bending_energy().detach())) < 1e-10
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        ffd.displacement.copy_(torch.rand(3, 3, 4, 5, generator=g))
    d = ffd.displacement.detach().double()
    total, count = 0.0, 0
    for a in (1, 2, 3):  # written out: d[i - 1] - 2 d[i] + d[i + 1] along each axis ...
        n = d.shape[a]
        x = d.narrow(a, 0, n - 2) - 2 * d.narrow(a, 1, n - 2) + d.narrow(a, 2, n - 2)
        total, count = total + float((x ** 2).sum()), count + x.numel()
    for a, b in ((1, 2), (1, 3), (2, 3)):  # ... and d[i+1, j+1] - d[i+1, j] - d[i, j+1] + d[i, j], twice
        na, nb = d.shape[a], d.shape[b]
        hi, lo = d.narrow(a, 1, na - 1), d.narrow(a, 0, na - 1)
        x = hi.narrow(b, 1, nb - 1) - hi.narrow(b, 0, nb - 1) - lo.narrow(b, 1, nb - 1) + lo.narrow(b, 0, nb - 1)
        total, count = total + 2 * float((x ** 2).sum()), count + x.numel()
    want = total / count
    assert want > 0 and abs(float(ffd.bending_energy().detach()) - want) < 1e-6 * want
    ffd.bending_energy().backward()
    assert ffd.displacement.grad is not None and float(ffd.displacement.grad.abs().max()) > 0
    # an axis of two nodes has no second difference: only the mixed terms remain
    drr = DRR(make_subject(phantom_volume((12, 10, 14), seed=3)), sdd=600.0, height=8, width=8, delx=4.0)
    two = FreeFormDeformation(drr, grid=(2, 2, 2), basis=BASIS)
    with torch.no_grad():
        two.displacement[0, 1, 1, 1] = 6.0
    # (component 0: each of the 3 pairs of axes has 2 mixed differences, one of them 6; 3 components)
    assert abs(float(two.bending_energy().detach()) - 2 * 3 * 36.0 / 18) < 1e-5


def test_linear_module_is_unchanged(emulated_ops, monkeypatch):
    import warp_cases

    warp_cases.route_warp_to_emulation(monkeypatch, emulated_ops)
    drr, ffd = _anisotropic()
    _, named = _anisotropic(basis="linear")
    assert ffd.basis == "linear" and list(ffd.parameters()) == [ffd.displacement]
    g = torch.Generator().manual_seed(4)
    U = torch.rand(3, 3, 4, 5, generator=g) * 2 - 1
    with torch.no_grad():
        ffd.displacement.copy_(U)
        named.displacement.copy_(U)
    assert torch.equal(ffd.warped(), named.warped())
    V = drr.density
    assert torch.equal(warp_volume(V, U.contiguous()), warp_volume(V, U.contiguous(), basis="linear"))
    assert torch.equal(warp_volume(V, U.contiguous(), "border"), warp_volume(V, U.contiguous(), "border", "linear"))


# ------------------------------------------------------------------------------------------------ errors
def test_domain_errors_name_the_condition(bspline_ops, monkeypatch):
    V, U = torch.rand(6, 7, 8), torch.zeros(3, 2, 3, 4)
    warp_volume(V, U, basis=BASIS)
    with pytest.raises(ValueError, match="basis.*'cubic'"):
        warp_volume(V, U, basis="cubic")
    with pytest.raises(ValueError, match="basis.*'cubic'"):
        warp_reference(V, U, basis="cubic")
    with pytest.raises(ValueError, match="basis.*'cubic'"):
        dense_field(U, V.shape, "cubic")
    with pytest.raises(ValueError, match="padding"):
        warp_volume(V, U, padding="reflection", basis=BASIS)
    with pytest.raises(ValueError, match="float32"):
        warp_volume(V.double(), U, basis=BASIS)
    with pytest.raises(ValueError, match="float32"):
        warp_volume(V, U.double(), basis=BASIS)
    with pytest.raises(ValueError, match="contiguous"):
        warp_volume(V.transpose(0, 1), U, basis=BASIS)
    with pytest.raises(ValueError, match=r"\(Dx, Dy, Dz\)"):
        warp_volume(V[0], U, basis=BASIS)
    with pytest.raises(ValueError, match=r"\(3, Gx, Gy, Gz\)"):
        warp_volume(V, U[:2], basis=BASIS)
    with pytest.raises(ValueError, match="G_a <= D_a"):
        warp_volume(V, torch.zeros(3, 7, 3, 4), basis=BASIS)
    with pytest.raises(ValueError, match="2 <= G_a"):
        warp_volume(V, torch.zeros(3, 1, 3, 4), basis=BASIS)
    with pytest.raises(ValueError, match="65535"):
        warp_volume(torch.zeros(2, 2, 65536), torch.zeros(3, 2, 2, 2), basis=BASIS)
    with pytest.raises(ValueError, match=r"2\^31 voxels"):
        diffdrr_amd.ops._check_bspline("warp_volume", (2048, 2048, 513), torch.zeros(3, 2, 2, 2), "zeros")
    gW = torch.rand(6, 7, 8)
    with pytest.raises(ValueError, match="grad_out has shape"):
        diffdrr_amd.ops.bspline_backward_displacement(V, U, gW[:5], "zeros")
    with pytest.raises(ValueError, match="float32"):
        diffdrr_amd.ops.bspline_backward_volume(U, gW.double(), "zeros")
    drr = DRR(make_subject(V), sdd=600.0, height=8, delx=4.0)
    with pytest.raises(ValueError, match="basis.*'cubic'"):
        FreeFormDeformation(drr, grid=(2, 3, 4), basis="cubic")
    with pytest.raises(ValueError, match="grid"):
        FreeFormDeformation(drr, grid=(2, 3, 9), basis=BASIS)
    # a CPU tensor: there is no CPU fallback
    monkeypatch.setattr(diffdrr_amd.ops, "on_device", lambda t: t.is_cuda)
    with pytest.raises(ValueError, match="GPU only"):
        warp_volume(V, U, basis=BASIS)
    with pytest.raises(ValueError, match="GPU only"):
        diffdrr_amd.ops.bspline_forward(V, U)
