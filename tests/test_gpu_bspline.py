"""Cubic B-spline free-form deformation on the MI355X: the checks of tests/test_bspline.py through the gfx950
kernels (libdiffdrr_bspline_hip.so)."""
import pytest
import torch

import bspline_cases
import large_deformation as large
from diffdrr_amd import DRR, FreeFormDeformation, ops, warp_reference, warp_volume
from diffdrr_amd.data import make_subject, phantom_volume
from diffdrr_amd.deformation import dense_field

pytestmark = pytest.mark.gpu
BASIS = bspline_cases.BASIS


@pytest.mark.parametrize("case,kind,padding,amplitude", bspline_cases.VALUE_CASES)
def test_value_and_gradients_against_float64(gpu, case, kind, padding, amplitude):
    bspline_cases.check_value_and_gradients(case, kind, padding, amplitude, gpu)


@pytest.mark.parametrize("padding", bspline_cases.PADDINGS)
@pytest.mark.parametrize("case", sorted(bspline_cases.CASES))
def test_identity_lattice_is_exact(gpu, case, padding):
    for kind in bspline_cases.KINDS:
        bspline_cases.check_identity(case, kind, padding, gpu)


def test_forward_and_coefficient_gradient_are_reproducible(gpu):
    bspline_cases.check_reproducible(gpu, ops)


def test_volume_gradient_is_a_scatter_of_the_same_weights(gpu):
    """<gW, warp(V)> = <gV, V> for any V (the warp is linear in the volume): the atomic scatter against the
    forward kernel on the device itself, in float64 sums."""
    V, U, gW = (t.to(gpu) for t in bspline_cases.scene("40x36x130", "noise", 2.5))
    for padding in bspline_cases.PADDINGS:
        lhs = float((gW.double() * ops.bspline_forward(V, U, padding).double()).sum())
        rhs = float((ops.bspline_backward_volume(U, gW, padding).double() * V.double()).sum())
        assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (padding, lhs, rhs)


def test_coefficient_gradient_through_the_siddon_renderer(gpu):
    bspline_cases.check_chain_through_siddon(gpu)


def test_recovery_through_the_drr(gpu):
    bspline_cases.check_recovery_through_drr(gpu)


def test_module_with_the_bspline_basis(gpu):
    vol = phantom_volume((12, 10, 14), seed=3)
    drr = DRR(make_subject(vol, spacing=(0.5, 2.0, 1.25)), sdd=600.0, height=8, width=8, delx=4.0).to(gpu)
    ffd = FreeFormDeformation(drr, grid=(3, 4, 5), padding="border", basis=BASIS)
    assert list(ffd.parameters()) == [ffd.displacement] and ffd.displacement.device.type == "cuda"
    assert torch.equal(ffd.warped().detach(), drr.density)
    with torch.no_grad():
        ffd.displacement[0] = 1.0   # 1 mm along x = 2 voxels of 0.5 mm
        ffd.displacement[1] = 4.0   # 4 mm along y = 2 voxels of 2 mm
    shift = torch.tensor([2.0, 2.0, 0.0], device=gpu).reshape(3, 1, 1, 1).expand(3, 3, 4, 5)
    assert torch.allclose(ffd.warped().detach(), warp_reference(drr.density, shift, "border", BASIS), atol=1e-6)
    # the linear basis is the call without the keyword
    U = (torch.rand(3, 3, 4, 5, generator=torch.Generator().manual_seed(4)) * 2 - 1).to(gpu)
    assert torch.equal(warp_volume(drr.density, U, "border"), warp_volume(drr.density, U, "border", "linear"))


def test_cpu_tensors_are_rejected(gpu):
    V, U, _ = bspline_cases.scene("2x2x2", "noise", 2.5)
    with pytest.raises(ValueError, match="GPU only"):
        ops.bspline_forward(V, U)
    with pytest.raises(ValueError, match="displacement is on cpu.*GPU only"):
        ops.bspline_forward(V.to(gpu), U)
    with pytest.raises(ValueError, match="volume is on cpu.*GPU only"):
        ops.bspline_forward(V, U.to(gpu))
    with pytest.raises(ValueError, match="GPU only"):
        warp_volume(V, U, basis=BASIS)


LARGE_SEED = 1  # (the first seed from 1 that keeps large_deformation.FACE_MARGIN)


@pytest.mark.parametrize("padding", bspline_cases.PADDINGS)
def test_volume_past_2_to_the_30_voxels(gpu, padding):
    """W, gV and gU of a (1040, 1024, 1024) volume on four windows (tests/large_deformation.py): byte offsets
    past 2 GiB and 4 GiB.  gU is gated per component on bspline_cases' scale, summed over the windows."""
    U = large.lattice(LARGE_SEED, 5.0)

    def gate_gU(name, names, got, ref64, ref32, held):
        spread = sum(bspline_cases.coefficient_gradient_spread(part, U, gW, padding, box, (large.SHAPE, reach))
                     for box, reach, part, gW in held)
        own = [float((ref32[0][a].double() - ref64[0][a]).abs().max()) for a in range(3)]
        bspline_cases.gate_gU(name, got[0], ref64[0], own, [float(spread[a].max()) for a in range(3)])

    large.check(f"bspline {padding}", gpu, LARGE_SEED, (U,), ("gU",),
                kernel=lambda V, U: warp_volume(V, U, padding, BASIS),
                definition=lambda V, U, box, part: warp_reference(V, U, padding, BASIS, box=box, part=part),
                field=lambda box: dense_field(U.double(), large.SHAPE, BASIS, box=box), lattice_gate=gate_gU)


def test_sizes_outside_the_domain_are_refused_before_any_launch(gpu, monkeypatch):
    U = torch.zeros(3, 2, 2, 2, device=gpu)
    large.check_domain_errors(monkeypatch, ops, "_launch_bspline", lambda V: ops.bspline_forward(V, U),
                              lambda shape: ops._check_bspline("bspline_forward", shape, U, "zeros"), U)
