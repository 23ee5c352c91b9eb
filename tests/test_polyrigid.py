"""Polyrigid deformation without a GPU: the host build of csrc/polyrigid_core.h (tests/emu/polyrigid_emu.cpp)
behind the product's own Python layers -- value and every gradient against the float64 definition, the definition
against matrix exponentials, the identity, the seam of the series, an exact translation, reproducibility, the
chain through the Siddon renderer, both recoveries, the module, the helper, the errors."""
import pytest
import torch

import diffdrr_amd
import polyrigid_cases as cases
from diffdrr_amd import (DRR, PolyRigidDeformation, _lib, polyrigid_reference, polyrigid_warp, twist_lattice,
                         weights_from_labels)
from diffdrr_amd.data import make_subject, phantom_volume
from diffdrr_amd.deformation import dense_field, sample_displaced
from diffdrr_amd.polyrigid import centred_coordinates, exponential_coefficients

CPU = torch.device("cpu")


@pytest.fixture()
def polyrigid_ops(emulated_ops, monkeypatch):
    cases.route_polyrigid_to_emulation(monkeypatch, emulated_ops)
    return emulated_ops


def test_exported_from_the_package():
    assert diffdrr_amd.polyrigid_warp is polyrigid_warp and diffdrr_amd.PolyRigidDeformation is PolyRigidDeformation
    assert diffdrr_amd.polyrigid_reference is polyrigid_reference and diffdrr_amd.twist_lattice is twist_lattice
    assert diffdrr_amd.weights_from_labels is weights_from_labels
    assert _lib.POLYRIGID_ABI_VERSION == 1 and callable(diffdrr_amd.ops.polyrigid_forward)


# the largest |W - W'| of test_reference_is_the_matrix_exponential_in_float64, as measured (zeros padding; border 3.9e-14)
DEFINITION_DIFFERENCE = 5.5e-14


def test_reference_is_the_matrix_exponential_in_float64():
    """The definition against an independent composition: per voxel the matrix exponential of the 4 x 4 twist
    matrix applied to y, then ``sample_displaced``.  On the 23 x 30 x 37 large scene (noise, zeros padding) the
    two W differ by 5.5e-14 (measured: DEFINITION_DIFFERENCE; the displacements by 7e-14 voxel); the gate is 100
    times that."""
    V, theta, weights, _ = (t.double() for t in cases.scene("23x30x37", "noise", "large"))
    dims = V.shape
    xi = dense_field(twist_lattice(theta, weights), dims).reshape(6, -1).T
    M = torch.zeros(xi.shape[0], 4, 4, dtype=torch.float64)
    M[:, 0, 1], M[:, 0, 2], M[:, 1, 2] = -xi[:, 2], xi[:, 1], -xi[:, 0]
    M[:, 1, 0], M[:, 2, 0], M[:, 2, 1] = xi[:, 2], -xi[:, 1], xi[:, 0]
    M[:, :3, 3] = xi[:, 3:]
    E = torch.linalg.matrix_exp(M)
    y = centred_coordinates(dims, cases.PITCH, CPU, torch.float64).reshape(3, -1).T
    moved = (E[:, :3, :3] @ y[:, :, None])[:, :, 0] + E[:, :3, 3]
    u = ((moved - y) / torch.tensor(cases.PITCH, dtype=torch.float64)).T.reshape(3, *dims)
    for padding in cases.PADDINGS:
        W = polyrigid_reference(V, theta, weights, cases.PITCH, padding)
        difference = float((W - sample_displaced(V, u, padding)).abs().max())
        print(f"{padding}: definition against matrix exponentials: {difference:.2e}")
        assert difference <= 100 * DEFINITION_DIFFERENCE


def test_series_and_closed_forms_agree_at_the_seam():
    """A, B, C on either side of the seam, in float32 against float64: to a few float32 roundings."""
    s = torch.tensor([cases.SERIES_BELOW * (1 - 1e-6), cases.SERIES_BELOW], dtype=torch.float64)
    for c32, c64 in zip(exponential_coefficients(s.float()), exponential_coefficients(s)):
        assert float((c32.double() - c64).abs().max()) <= 4 * 2.0 ** -24 * float(c64.abs().max())
    for c64 in exponential_coefficients(s):
        assert abs(float(c64[1] - c64[0])) <= 1e-6  # (continuous: the slope times the step)


@pytest.mark.parametrize("case,kind,padding,amplitude", cases.VALUE_CASES)
def test_value_and_gradients_against_float64(polyrigid_ops, case, kind, padding, amplitude):
    """While the kernels formed the sample position in float, two of these cases missed the gate on the host build:
    ``65535x2x3-phantom-border-large`` (``g theta`` 7.18e-3 of its scale, float32 reference 1.31e-6: 5 of the
    394980 coordinates that still interpolate lay within one float32 ulp of u, 2.4e-4 voxel at 2505 voxels, of a
    voxel face) and ``2x3x65535-phantom-zeros-large`` (``W`` 3.54e-6, reference 6.43e-7: a voxel 507 mm from the
    centre whose u of about one voxel is a difference of terms of 150 mm).  With the position in double they are at
    2.55e-7 and 5.18e-7."""
    cases.check_value_and_gradients(case, kind, padding, amplitude, CPU)


@pytest.mark.parametrize("padding", cases.PADDINGS)
@pytest.mark.parametrize("case", sorted(cases.CASES))
def test_zero_twists_are_the_identity(polyrigid_ops, case, padding):
    cases.check_identity(case, padding, CPU)


@pytest.mark.parametrize("padding", cases.PADDINGS)
def test_seam_between_series_and_closed_forms(polyrigid_ops, padding):
    cases.check_seam(padding, CPU)


def test_integer_translation_is_exact(polyrigid_ops):
    cases.check_exact_translation(CPU)


def test_forward_and_twist_gradient_are_reproducible(polyrigid_ops):
    cases.check_reproducible(CPU, polyrigid_ops)


def test_twist_gradient_through_the_siddon_renderer(polyrigid_ops):
    cases.check_chain_through_siddon(CPU)


def test_recovery_volume_to_volume(polyrigid_ops):
    cases.check_recovery_volume_to_volume(CPU)


def test_recovery_through_the_drr(polyrigid_ops):
    cases.check_recovery_through_drr(CPU)


def test_recovery_gate_is_three_times_the_float64_loop(polyrigid_ops):
    """The gate of the recovery through the DRR is derived, not chosen: three times the final ratio of the float64
    route of the same loop (polyrigid_reference in front of the float64 renderer), run here; that ratio is itself
    below 0.05, so the test is about recovery."""
    ratio = cases.recovery_float64_ratio(CPU)
    print(f"float64 loop: final / first data loss {ratio:.4e}")
    assert abs(ratio - cases.RECOVERY_FLOAT64_RATIO) <= 0.05 * cases.RECOVERY_FLOAT64_RATIO
    assert cases.RECOVERY_GATE == 3 * cases.RECOVERY_FLOAT64_RATIO and cases.RECOVERY_FLOAT64_RATIO < 0.05


def _drr(shape=(12, 10, 14), spacing=(0.5, 2.0, 1.25)):
    return DRR(make_subject(phantom_volume(shape, seed=3), spacing=spacing), sdd=600.0, height=8, width=8, delx=4.0)


def test_module_parameters_weights_and_state(polyrigid_ops):
    drr = _drr()
    raw = torch.rand(3, 3, 4, 5, generator=torch.Generator().manual_seed(1)) + 0.1
    module = PolyRigidDeformation(drr, raw, padding="border")
    assert module.rotation.shape == module.translation.shape == (3, 3)
    assert float(module.rotation.detach().abs().max()) == 0.0 == float(module.translation.detach().abs().max())
    assert {n for n, _ in module.named_parameters()} == {"rotation", "translation"}
    assert module.pitch == pytest.approx((0.5, 2.0, 1.25))
    assert float((module.weights.sum(0) - 1).abs().max()) <= 2e-7 and not module.weights.requires_grad
    assert torch.allclose(module.weights, raw / raw.sum(0, keepdim=True))
    assert torch.equal(module.warped().detach(), drr.density)
    with torch.no_grad():
        module.translation[:] = torch.tensor([1.0, 4.0, 0.0])  # every body alike: 2 voxels along x, 2 along y
    shifted = polyrigid_reference(drr.density, module.twists().detach(), module.weights, module.pitch, "border")
    assert torch.allclose(module.warped().detach(), shifted, atol=1e-6)
    assert torch.allclose(shifted[:-2, :-2], drr.density[2:, 2:], atol=1e-5)
    other = PolyRigidDeformation(_drr(), torch.ones(3, 3, 4, 5), padding="border")
    other.load_state_dict(module.state_dict())
    assert torch.equal(other.weights, module.weights) and torch.equal(other.translation, module.translation)
    # the render goes through drr with its own volume put back
    theirs = drr.density
    img = module(torch.zeros(1, 3), torch.tensor([[0.0, 400.0, 0.0]]), **cases.KW)
    assert img.requires_grad and drr.density is theirs
    img.sum().backward()
    assert module.rotation.grad is not None and bool(torch.isfinite(module.rotation.grad).all())


def test_module_refuses_bad_weights():
    drr = _drr()
    good = torch.ones(2, 3, 4, 5)
    with pytest.raises(ValueError, match=r"\(K, Gx, Gy, Gz\)"):
        PolyRigidDeformation(drr, good[0])
    with pytest.raises(ValueError, match="non-negative"):
        PolyRigidDeformation(drr, good - 1.5)
    for bad in (float("nan"), float("inf")):
        w = good.clone()
        w[0, 1, 1, 1] = bad
        with pytest.raises(ValueError, match="finite"):
            PolyRigidDeformation(drr, w)
    w = good.clone()
    w[:, 2, 3, 4] = 0.0
    with pytest.raises(ValueError, match="positive sum"):
        PolyRigidDeformation(drr, w)
    with pytest.raises(ValueError, match="2 <= G_a <= D_a"):
        PolyRigidDeformation(drr, torch.ones(2, 13, 4, 5))
    with pytest.raises(ValueError, match="2 <= G_a <= D_a"):
        PolyRigidDeformation(drr, torch.ones(2, 3, 1, 5))
    with pytest.raises(ValueError, match="padding"):
        PolyRigidDeformation(drr, good, padding="wrap")


def test_weights_from_labels_on_blocks():
    labels = torch.zeros(24, 24, 24, dtype=torch.int64)
    labels[4:12, 8:16, 8:16] = 1
    labels[12:20, 4:12, 12:20] = 7
    w = weights_from_labels(labels, [[1], [7]], (6, 6, 6), sigma=0.5)
    assert w.shape == (3, 6, 6, 6) and w.dtype == torch.float32 and float(w.min()) >= 0
    assert float((w.sum(0) - 1).abs().max()) <= 2e-7
    body = w.argmax(0)
    for k, ids in enumerate((1, 7)):
        pooled = torch.nn.functional.adaptive_avg_pool3d((labels == ids).float()[None, None], (6, 6, 6))[0, 0]
        assert int((pooled == 1).sum()) == 8 and bool((body[pooled == 1] == k).all())
    assert bool((body[0] == 2).all())  # far from both blocks: the background
    assert weights_from_labels(labels, [1, 7], (6, 6, 6), sigma=0.5).equal(w)  # an id is a group of one
    with pytest.raises(ValueError, match="claimed by no group"):
        weights_from_labels(labels, [[1], [7]], (6, 6, 6), sigma=0.0, background=False)
    with pytest.raises(ValueError, match="integer label map"):
        weights_from_labels(labels.float(), [[1]], (6, 6, 6))
    with pytest.raises(ValueError, match="grid"):
        weights_from_labels(labels, [[1]], (6, 25, 6))


def test_domain_errors_name_the_condition(polyrigid_ops, monkeypatch):
    V, theta, weights = torch.rand(6, 7, 8), torch.zeros(2, 6), torch.full((2, 2, 3, 4), 0.5)
    polyrigid_warp(V, theta, weights)
    with pytest.raises(ValueError, match="padding"):
        polyrigid_warp(V, theta, weights, padding="reflection")
    with pytest.raises(ValueError, match="float32"):
        polyrigid_warp(V.double(), theta, weights)
    with pytest.raises(ValueError, match="float32"):
        polyrigid_warp(V, theta.double(), weights)
    with pytest.raises(ValueError, match="contiguous"):
        polyrigid_warp(V.transpose(0, 1), theta, weights)
    with pytest.raises(ValueError, match=r"\(Dx, Dy, Dz\)"):
        polyrigid_warp(V[0], theta, weights)
    with pytest.raises(ValueError, match=r"\(K, 6\)"):
        polyrigid_warp(V, theta[:, :5], weights)
    with pytest.raises(ValueError, match=r"\(K, 6\)"):
        polyrigid_warp(V, theta, weights[:1])
    with pytest.raises(ValueError, match="G_a <= D_a"):
        polyrigid_warp(V, theta, torch.ones(2, 7, 3, 4))
    with pytest.raises(ValueError, match="2 <= G_a"):
        polyrigid_warp(V, theta, torch.ones(2, 1, 3, 4))
    for pitch in ((1.0, 0.0, 1.0), (1.0, -2.0, 1.0), (1.0, float("inf"), 1.0), (1.0, float("nan"), 1.0), (1.0, 1.0)):
        with pytest.raises(ValueError, match="pitch"):
            polyrigid_warp(V, theta, weights, pitch)
    with pytest.raises(ValueError, match="65535"):
        polyrigid_warp(torch.zeros(2, 2, 65536), theta, torch.ones(2, 2, 2, 2))
    with pytest.raises(ValueError, match=r"2\^31 voxels"):
        diffdrr_amd.ops._check_polyrigid("polyrigid_warp", (2048, 2048, 513), torch.zeros(6, 2, 2, 2), (1, 1, 1), "zeros")
    with pytest.raises(ValueError, match=r"\(6, Gx, Gy, Gz\)"):
        diffdrr_amd.ops.polyrigid_forward(V, torch.zeros(3, 2, 3, 4))
    # a CPU tensor: there is no CPU fallback
    monkeypatch.setattr(diffdrr_amd.ops, "on_device", lambda t: t.is_cuda)
    with pytest.raises(ValueError, match="GPU only"):
        polyrigid_warp(V, theta, weights)
