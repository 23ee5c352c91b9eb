"""Polyrigid deformation on the MI355X: the checks of tests/test_polyrigid.py through the gfx950 kernels
(libdiffdrr_polyrigid_hip.so)."""
import pytest
import torch

import large_deformation as large
import polyrigid_cases as cases
from diffdrr_amd import ops, polyrigid_reference, polyrigid_warp, twist_lattice
from diffdrr_amd.polyrigid import displacement_field

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


LARGE_SEED = 4  # (the first seed from 1 that keeps large_deformation.FACE_MARGIN)


def large_bodies(seed):
    """Two bodies on large.GRID, |omega| <= 0.003 rad and |v| <= 2 mm: with cases.PITCH the corners of the
    (1040, 1024, 1024) volume lie 1440 mm from its centre and move by at most 4.3 + 2 mm = 7.9 voxels of 0.8 mm."""
    g = torch.Generator().manual_seed(seed)
    theta = torch.cat((cases.bounded(g, 2, 0.003), cases.bounded(g, 2, 2.0)), dim=1)
    return theta, cases.random_weights(g, 2, large.GRID)


@pytest.mark.parametrize("padding", cases.PADDINGS)
def test_volume_past_2_to_the_30_voxels(gpu, padding):
    """W, gV, g theta and g weights of a (1040, 1024, 1024) volume on four windows (tests/large_deformation.py):
    byte offsets past 2 GiB and 4 GiB."""
    theta, weights = large_bodies(LARGE_SEED)
    Xi = twist_lattice(theta.double(), weights.double())
    large.check(f"polyrigid {padding}", gpu, LARGE_SEED, (theta, weights), ("g theta", "g weights"),
                kernel=lambda V, t, w: polyrigid_warp(V, t, w, cases.PITCH, padding),
                definition=lambda V, t, w, box, part: polyrigid_reference(V, t, w, cases.PITCH, padding, box, part),
                field=lambda box: displacement_field(Xi, large.SHAPE, cases.PITCH, box))


def test_sizes_outside_the_domain_are_refused_before_any_launch(gpu, monkeypatch):
    Xi = torch.zeros(6, 2, 2, 2, device=gpu)
    large.check_domain_errors(
        monkeypatch, ops, "_launch_polyrigid", lambda V: ops.polyrigid_forward(V, Xi),
        lambda shape: ops._check_polyrigid("polyrigid_forward", shape, Xi, (1.0, 1.0, 1.0), "zeros"), Xi)
