"""Free-form deformation without a GPU: the host build of csrc/warp_core.h (tests/emu/warp_emu.cpp) behind the
product's own Python layers -- value and both gradients against the float64 definition, the identity lattice,
reproducibility, the chain through the Siddon renderer, both recoveries, the errors."""
import pytest
import torch

import diffdrr_amd
import warp_cases
from diffdrr_amd import DRR, FreeFormDeformation, _lib, warp_reference, warp_volume
from diffdrr_amd.data import make_subject, phantom_volume
from diffdrr_amd.deformation import dense_field

CPU = torch.device("cpu")


@pytest.fixture()
def warp_ops(emulated_ops, monkeypatch):
    warp_cases.route_warp_to_emulation(monkeypatch, emulated_ops)
    return emulated_ops


def test_exported_from_the_package():
    assert diffdrr_amd.warp_volume is warp_volume and diffdrr_amd.FreeFormDeformation is FreeFormDeformation
    assert diffdrr_amd.warp_reference is warp_reference
    assert _lib.WARP_ABI_VERSION == 1 and callable(diffdrr_amd.ops.warp_forward)


def test_reference_is_interpolate_plus_grid_sample_in_float64():
    """The definition against the torch composition it replaces (align_corners=True throughout), value and
    both gradients, both paddings."""
    import torch.nn.functional as F

    V, U, gW = (t.double() for t in warp_cases.scene("23x30x37", "noise", 2.5))
    dims = V.shape
    for padding in warp_cases.PADDINGS:
        a, b = V.clone().requires_grad_(), U.clone().requires_grad_()
        u = F.interpolate(b[None], size=dims, mode="trilinear", align_corners=True)[0]
        assert float((u - dense_field(b, dims)).detach().abs().max()) < 1e-13
        coords = [torch.arange(d, dtype=torch.float64).reshape([-1 if k == i else 1 for k in range(3)]) + u[i]
                  for i, d in enumerate(dims)]
        grid = torch.stack([2 * coords[i] / (dims[i] - 1) - 1 for i in (2, 1, 0)], dim=-1)[None]  # (x: fastest axis)
        W = F.grid_sample(a[None, None], grid, mode="bilinear", padding_mode=padding, align_corners=True)[0, 0]
        gV, gU = torch.autograd.grad(W, (a, b), gW)
        W64, gV64, gU64 = warp_cases.reference(V, U, gW, padding, torch.float64)
        assert float((W.detach() - W64).abs().max()) < 1e-13
        assert float((gV - gV64).abs().max()) < 1e-12 and float((gU - gU64).abs().max()) < 1e-11 * float(gU64.abs().max())


@pytest.mark.parametrize("case,kind,padding,amplitude", warp_cases.VALUE_CASES)
def test_value_and_gradients_against_float64(warp_ops, case, kind, padding, amplitude):
    warp_cases.check_value_and_gradients(case, kind, padding, amplitude, CPU)


@pytest.mark.parametrize("padding", warp_cases.PADDINGS)
@pytest.mark.parametrize("case", sorted(warp_cases.CASES))
def test_identity_lattice_is_exact(warp_ops, case, padding):
    for kind in warp_cases.KINDS:
        warp_cases.check_identity(case, kind, padding, CPU)


def test_forward_and_lattice_gradient_are_reproducible(warp_ops):
    warp_cases.check_reproducible(CPU, warp_ops)


def test_lattice_gradient_through_the_siddon_renderer(warp_ops):
    warp_cases.check_chain_through_siddon(CPU)


def test_recovery_volume_to_volume(warp_ops):
    warp_cases.check_recovery_volume_to_volume(CPU)


def test_recovery_through_the_drr(warp_ops):
    warp_cases.check_recovery_through_drr(CPU)


def test_recovery_gate_is_three_times_the_float64_loop(warp_ops):
    """The gate of the recovery through the DRR is derived, not chosen: three times the final ratio of the
    float64 route of the same loop (warp_reference in front of the float64 renderer), run here."""
    ratio = warp_cases.recovery_float64_ratio(CPU)
    print(f"float64 loop: final / first data loss {ratio:.4e}")
    assert abs(ratio - warp_cases.RECOVERY_FLOAT64_RATIO) <= 0.05 * warp_cases.RECOVERY_FLOAT64_RATIO
    assert warp_cases.RECOVERY_GATE == 3 * warp_cases.RECOVERY_FLOAT64_RATIO


def test_module_parameter_pitch_and_smoothness(warp_ops):
    vol = phantom_volume((12, 10, 14), seed=3)
    drr = DRR(make_subject(vol, spacing=(0.5, 2.0, 1.25)), sdd=600.0, height=8, width=8, delx=4.0)
    ffd = FreeFormDeformation(drr, grid=(3, 4, 5), padding="border")
    assert isinstance(ffd.displacement, torch.nn.Parameter) and ffd.displacement.shape == (3, 3, 4, 5)
    assert float(ffd.displacement.detach().abs().max()) == 0.0 and list(ffd.parameters()) == [ffd.displacement]
    assert torch.allclose(ffd.pitch.flatten(), torch.tensor([0.5, 2.0, 1.25]))
    assert torch.equal(ffd.warped().detach(), drr.density) and float(ffd.smoothness().detach()) == 0.0
    with torch.no_grad():
        ffd.displacement[0] = 1.0   # 1 mm along x = 2 voxels of 0.5 mm
        ffd.displacement[1] = 4.0   # 4 mm along y = 2 voxels of 2 mm
    expect = warp_reference(drr.density, torch.tensor([2.0, 2.0, 0.0]).reshape(3, 1, 1, 1).expand(3, 3, 4, 5), "border")
    assert torch.allclose(ffd.warped().detach(), expect, atol=1e-6)
    assert float(ffd.smoothness().detach()) == 0.0  # a constant field is smooth
    with torch.no_grad():
        ffd.displacement[2, :, :, 1] = 3.0
    d = ffd.displacement.detach()
    diffs = [d.diff(dim=a + 1) for a in range(3)]
    want = sum(float(x.pow(2).sum()) for x in diffs) / sum(x.numel() for x in diffs)
    assert abs(float(ffd.smoothness().detach()) - want) < 1e-6 and want > 0
    ffd.smoothness().backward()
    assert ffd.displacement.grad is not None
    # the render goes through drr with its own volume put back
    theirs = drr.density
    img = ffd(torch.zeros(1, 3), torch.tensor([[0.0, 400.0, 0.0]]), parameterization="euler_angles", convention="ZXY")
    assert img.requires_grad and drr.density is theirs


def test_domain_errors_name_the_condition(warp_ops, monkeypatch):
    V, U = torch.rand(6, 7, 8), torch.zeros(3, 2, 3, 4)
    warp_volume(V, U)
    with pytest.raises(ValueError, match="padding"):
        warp_volume(V, U, padding="reflection")
    with pytest.raises(ValueError, match="float32"):
        warp_volume(V.double(), U)
    with pytest.raises(ValueError, match="float32"):
        warp_volume(V, U.double())
    with pytest.raises(ValueError, match="contiguous"):
        warp_volume(V.transpose(0, 1), U)
    with pytest.raises(ValueError, match=r"\(Dx, Dy, Dz\)"):
        warp_volume(V[0], U)
    with pytest.raises(ValueError, match=r"\(3, Gx, Gy, Gz\)"):
        warp_volume(V, U[:2])
    with pytest.raises(ValueError, match="G_a <= D_a"):
        warp_volume(V, torch.zeros(3, 7, 3, 4))
    with pytest.raises(ValueError, match="2 <= G_a"):
        warp_volume(V, torch.zeros(3, 1, 3, 4))
    with pytest.raises(ValueError, match="65535"):
        warp_volume(torch.zeros(2, 2, 65536), torch.zeros(3, 2, 2, 2))
    with pytest.raises(ValueError, match=r"2\^31 voxels"):
        diffdrr_amd.ops._check_warp("warp_volume", (2048, 2048, 513), torch.zeros(3, 2, 2, 2), "zeros")
    # a CPU tensor: there is no CPU fallback
    monkeypatch.setattr(diffdrr_amd.ops, "on_device", lambda t: t.is_cuda)
    with pytest.raises(ValueError, match="GPU only"):
        warp_volume(V, U)
    with pytest.raises(ValueError, match="grid"):
        FreeFormDeformation(DRR(make_subject(V), sdd=600.0, height=8, delx=4.0), grid=(2, 3, 9))
    with pytest.raises(ValueError, match="padding"):
        FreeFormDeformation(DRR(make_subject(V), sdd=600.0, height=8, delx=4.0), grid=(2, 3, 4), padding="wrap")
