"""Weighted multi-view Levenberg-Marquardt registration with a detector per view on the MI355X: the checks of
tests/test_wmvlm.py through the gfx950 kernels (libdiffdrr_wmvlm_hip.so)."""
import pytest
import torch

import wmvlm_cases
from diffdrr_amd import ops
from wmvlm_cases import NAMES, SMALL, SV, SV_IDS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("S,V", SV, ids=SV_IDS)
@pytest.mark.parametrize("name", NAMES)
def test_rays_equal_the_one_view_entry_with_each_views_detector_and_the_clears(gpu, name, S, V):
    wmvlm_cases.check_raygen(name, S, V, gpu, ops)


@pytest.mark.parametrize("S,V", SV, ids=SV_IDS)
@pytest.mark.parametrize("name", NAMES)
def test_sums_and_jacobian_equal_the_weighted_one_view_entry_bit_for_bit(gpu, name, S, V):
    wmvlm_cases.check_sums_bit_for_bit(name, S, V, gpu, ops)


@pytest.mark.parametrize("S,V", SV[1:], ids=SV_IDS[1:])
@pytest.mark.parametrize("name", NAMES)
def test_masked_pixels_are_not_read(gpu, name, S, V):
    wmvlm_cases.check_masked_pixels_are_not_read(name, S, V, gpu, ops)


@pytest.mark.parametrize("S,V", SV, ids=SV_IDS)
@pytest.mark.parametrize("name", SMALL)
def test_sums_and_jacobian_against_float64(gpu, name, S, V):
    wmvlm_cases.check_sums_against_float64(name, S, V, gpu, ops)


def test_step_with_one_view_is_the_weighted_one_view_step_bit_for_bit(gpu):
    wmvlm_cases.check_step_one_view_is_wlm_step(gpu, ops)


@pytest.mark.parametrize("V", (2, 3))
def test_step_with_unit_weights_is_the_unweighted_multi_view_step(gpu, V):
    wmvlm_cases.check_step_with_unit_weights_is_mvlm_step(V, gpu, ops)


@pytest.mark.parametrize("V", (2, 3))
def test_step_sequences_against_the_definition(gpu, V):
    wmvlm_cases.check_step_sequences(V, gpu, ops)


def test_step_skips_a_view_without_weights(gpu):
    wmvlm_cases.check_step_skips_empty_views(gpu, ops)


@pytest.mark.parametrize("V", (2, 3))
def test_step_under_scaled_weights(gpu, V):
    wmvlm_cases.check_step_scaling(V, gpu, ops)


def test_step_of_a_start_does_not_depend_on_its_neighbours(gpu):
    wmvlm_cases.check_step_neighbours(gpu, ops)


def test_registration_of_an_occluded_biplane_pair(gpu):
    wmvlm_cases.check_occluded_biplane(gpu, ops)


def test_registration_with_a_detector_per_view(gpu):
    wmvlm_cases.check_calibrated_biplane(gpu, ops)


def test_multi_starts_jacobian_and_bookkeeping(gpu):
    wmvlm_cases.check_multi_starts(gpu, ops)


def test_errors_name_the_condition(gpu):
    wmvlm_cases.check_errors(gpu, torch.device("cpu"))
