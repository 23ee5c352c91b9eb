"""Multi-view (biplane) Levenberg-Marquardt registration on the MI355X: the checks of tests/test_mvlm.py through the
gfx950 kernels (libdiffdrr_mvlm_hip.so)."""
import pytest
import torch

import mvlm_cases
from diffdrr_amd import ops
from mvlm_cases import NAMES, SV, SV_IDS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("S,V", SV, ids=SV_IDS)
@pytest.mark.parametrize("name", NAMES)
def test_rays_equal_the_one_view_entry_bit_for_bit_and_the_clears(gpu, name, S, V):
    mvlm_cases.check_raygen(name, S, V, gpu, ops)


@pytest.mark.parametrize("S,V", SV, ids=SV_IDS)
@pytest.mark.parametrize("name", NAMES)
def test_sums_and_jacobian_equal_the_one_view_entry_bit_for_bit(gpu, name, S, V):
    mvlm_cases.check_sums_bit_for_bit(name, S, V, gpu, ops)


@pytest.mark.parametrize("S,V", SV, ids=SV_IDS)
@pytest.mark.parametrize("name", NAMES)
def test_sums_and_jacobian_against_float64(gpu, name, S, V):
    mvlm_cases.check_sums_against_float64(name, S, V, gpu, ops)


def test_step_with_one_view_is_the_one_view_step_bit_for_bit(gpu):
    mvlm_cases.check_step_one_view_is_lm_step(gpu, ops)


@pytest.mark.parametrize("V", (2, 3))
def test_step_sequences_against_the_definition(gpu, V):
    mvlm_cases.check_step_sequences(V, gpu, ops)


def test_a_second_view_conditions_the_depth_translation(gpu):
    mvlm_cases.check_conditioning(gpu)


def test_registration_from_two_views(gpu):
    mvlm_cases.check_registration(gpu, ops)


def test_multi_starts_jacobian_and_independence(gpu):
    mvlm_cases.check_multi_starts(gpu, ops)


def test_errors_name_the_condition(gpu):
    mvlm_cases.check_errors(gpu, torch.device("cpu"))
