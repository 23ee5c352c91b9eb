"""Polyrigid deformation on the MI355X: the checks of tests/test_polyrigid.py through the gfx950 kernels
(libdiffdrr_polyrigid_hip.so)."""
import pytest

import polyrigid_cases as cases
from diffdrr_amd import ops, twist_lattice

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case,kind,padding,amplitude", cases.VALUE_CASES)
def test_value_and_gradients_against_float64(gpu, case, kind, padding, amplitude):
    cases.check_value_and_gradients(case, kind, padding, amplitude, gpu)


@pytest.mark.parametrize("padding", cases.PADDINGS)
@pytest.mark.parametrize("case", sorted(cases.CASES))
def test_zero_twists_are_the_identity(gpu, case, padding):
    cases.check_identity(case, padding, gpu)


@pytest.mark.parametrize("padding", cases.PADDINGS)
def test_seam_between_series_and_closed_forms(gpu, padding):
    cases.check_seam(padding, gpu)


def test_integer_translation_is_exact(gpu):
    cases.check_exact_translation(gpu)


def test_forward_and_twist_gradient_are_reproducible(gpu):
    cases.check_reproducible(gpu, ops)


def test_volume_gradient_is_a_scatter_of_the_same_weights(gpu):
    """<gW, warp(V)> = <gV, V> for any V (the warp is linear in the volume): the atomic scatter against the
    forward kernel on the device itself, in float64 sums."""
    V, theta, weights, gW = (t.to(gpu) for t in cases.scene("40x36x130", "noise", "large"))
    Xi = twist_lattice(theta, weights)
    for padding in cases.PADDINGS:
        lhs = float((gW.double() * ops.polyrigid_forward(V, Xi, cases.PITCH, padding).double()).sum())
        rhs = float((ops.polyrigid_backward_volume(Xi, gW, cases.PITCH, padding).double() * V.double()).sum())
        assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (padding, lhs, rhs)


def test_twist_gradient_through_the_siddon_renderer(gpu):
    cases.check_chain_through_siddon(gpu)


def test_recovery_volume_to_volume(gpu):
    cases.check_recovery_volume_to_volume(gpu)


def test_recovery_through_the_drr(gpu):
    cases.check_recovery_through_drr(gpu)


def test_cpu_tensors_are_rejected(gpu):
    V, theta, weights, _ = cases.scene("2x2x2", "noise", "small")
    Xi = twist_lattice(theta, weights)
    with pytest.raises(ValueError, match="GPU only"):
        ops.polyrigid_forward(V, Xi)
    with pytest.raises(ValueError, match="twists is on cpu.*GPU only"):
        ops.polyrigid_forward(V.to(gpu), Xi)
    with pytest.raises(ValueError, match="volume is on cpu.*GPU only"):
        ops.polyrigid_forward(V, Xi.to(gpu))
