"""The Jacobian determinant of a lattice deformation on the MI355X: the checks of tests/test_jacobian.py through
the gfx950 kernels (libdiffdrr_jacobian_hip.so)."""
import pytest
import torch

import jacobian_cases
from diffdrr_amd import jacobian_determinant, ops, volume_penalty

pytestmark = pytest.mark.gpu
BASES = jacobian_cases.BASES


@pytest.mark.parametrize("case,basis,amplitude", jacobian_cases.VALUE_CASES)
def test_map_statistics_penalty_and_gradients_against_float64(gpu, case, basis, amplitude):
    jacobian_cases.check_against_float64(case, basis, amplitude, gpu)


@pytest.mark.parametrize("basis", BASES)
@pytest.mark.parametrize("case", sorted(jacobian_cases.CASES))
def test_identity_lattice_is_exact(gpu, case, basis):
    jacobian_cases.check_identity(case, basis, gpu)


def test_everything_is_reproducible(gpu):
    jacobian_cases.check_reproducible(gpu, ops)


@pytest.mark.parametrize("basis", BASES)
@pytest.mark.parametrize("case", jacobian_cases.REPRODUCIBLE)
def test_map_and_fused_penalty_agree(gpu, case, basis):
    jacobian_cases.check_map_and_fused_penalty_agree(case, basis, gpu, ops)


@pytest.mark.parametrize("basis", BASES)
def test_unfolding(gpu, basis):
    jacobian_cases.check_unfolding(basis, gpu)


def test_module(gpu):
    jacobian_cases.check_module(gpu)


def test_cpu_tensors_and_bad_eps_are_rejected(gpu):
    U = jacobian_cases.scene("2x2x2", 2.5)[0]
    with pytest.raises(ValueError, match="displacement is on cpu.*GPU only"):
        jacobian_determinant(U, (2, 2, 2))
    with pytest.raises(ValueError, match="GPU only"):
        ops.jacobian_backward(U.to(gpu), (2, 2, 2), torch.zeros(2, 2, 2))
    with pytest.raises(ValueError, match=r"eps must be in \(0, 1\]"):
        volume_penalty(U.to(gpu), (2, 2, 2), eps=0.0)
    with pytest.raises(ValueError, match="float32"):
        volume_penalty(U.double().to(gpu), (2, 2, 2))
