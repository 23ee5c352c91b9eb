"""Free-form deformation on the MI355X: the checks of tests/test_warp.py through the gfx950 kernels
(libdiffdrr_warp_hip.so)."""
import pytest
import torch

import large_deformation as large
import warp_cases
from diffdrr_amd import ops, warp_reference, warp_volume
from diffdrr_amd.deformation import dense_field, sample_displaced

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case,kind,padding,amplitude", warp_cases.VALUE_CASES)
def test_value_and_gradients_against_float64(gpu, case, kind, padding, amplitude):
    warp_cases.check_value_and_gradients(case, kind, padding, amplitude, gpu)


@pytest.mark.parametrize("padding", warp_cases.PADDINGS)
@pytest.mark.parametrize("case", sorted(warp_cases.CASES))
def test_identity_lattice_is_exact(gpu, case, padding):
    for kind in warp_cases.KINDS:
        warp_cases.check_identity(case, kind, padding, gpu)


def test_forward_and_lattice_gradient_are_reproducible(gpu):
    warp_cases.check_reproducible(gpu, ops)


def test_volume_gradient_is_a_scatter_of_the_same_weights(gpu):
    """<gW, warp(V)> = <gV, V> for any V (the warp is linear in the volume): the atomic scatter against the
    forward kernel on the device itself, in float64 sums."""
    V, U, gW = (t.to(gpu) for t in warp_cases.scene("40x36x130", "noise", 2.5))
    for padding in warp_cases.PADDINGS:
        lhs = float((gW.double() * ops.warp_forward(V, U, padding).double()).sum())
        rhs = float((ops.warp_backward_volume(U, gW, padding).double() * V.double()).sum())
        assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (padding, lhs, rhs)


def test_lattice_gradient_through_the_siddon_renderer(gpu):
    warp_cases.check_chain_through_siddon(gpu)


def test_recovery_volume_to_volume(gpu):
    warp_cases.check_recovery_volume_to_volume(gpu)


def test_recovery_through_the_drr(gpu):
    warp_cases.check_recovery_through_drr(gpu)


def test_cpu_tensors_are_rejected(gpu):
    V, U, _ = warp_cases.scene("2x2x2", "noise", 2.5)
    with pytest.raises(ValueError, match="GPU only"):
        ops.warp_forward(V, U)
    with pytest.raises(ValueError, match="displacement is on cpu.*GPU only"):
        ops.warp_forward(V.to(gpu), U)
    with pytest.raises(ValueError, match="volume is on cpu.*GPU only"):
        ops.warp_forward(V, U.to(gpu))


LARGE_SEED = 1  # (the first seed from 1 that keeps large_deformation.FACE_MARGIN)


@pytest.mark.parametrize("padding", warp_cases.PADDINGS)
def test_volume_past_2_to_the_30_voxels(gpu, padding):
    """W, gV and gU of a (1040, 1024, 1024) volume on four windows (tests/large_deformation.py): byte offsets
    past 2 GiB and 4 GiB.  The float32 yardstick is warp_cases.reference's."""
    U = large.lattice(LARGE_SEED, 3.0)
    large.check(f"warp {padding}", gpu, LARGE_SEED, (U,), ("gU",),
                kernel=lambda V, U: warp_volume(V, U, padding),
                definition=lambda V, U, box, part: warp_reference(V, U, padding, box=box, part=part),
                float32_definition=lambda V, U, box, part: sample_displaced(
                    V, dense_field(U, large.SHAPE, box=box), padding, box, part),
                field=lambda box: dense_field(U.double(), large.SHAPE, box=box))


def test_sizes_outside_the_domain_are_refused_before_any_launch(gpu, monkeypatch):
    U = torch.zeros(3, 2, 2, 2, device=gpu)
    large.check_domain_errors(monkeypatch, ops, "_launch_warp", lambda V: ops.warp_forward(V, U),
                              lambda shape: ops._check_warp("warp_forward", shape, U, "zeros"), U)
