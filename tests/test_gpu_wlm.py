"""Levenberg-Marquardt registration with a pixel weight on the MI355X: the checks of tests/test_wlm.py through the
gfx950 kernels (libdiffdrr_wlm_hip.so), and the device's partial sums against the same order on the host."""
import pytest
import torch

import wlm_cases
from diffdrr_amd import ops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", wlm_cases.SUM_NAMES)
def test_sums_and_jacobian_against_float64(gpu, name):
    wlm_cases.check_sums_and_jacobian(name, gpu, ops)


@pytest.mark.parametrize("name", wlm_cases.SUM_NAMES)
def test_bit_for_bit_properties(gpu, name):
    wlm_cases.check_bit_for_bit_properties(name, gpu, ops)


@pytest.mark.parametrize("name", ("780_rays_zyx_stop", "4087_rays_four_workgroups", "1025_rays"))
def test_device_sums_equal_the_host_order_bit_for_bit_given_the_same_rows(gpu, name):
    wlm_cases.check_device_sums_from_the_devices_own_rows(name, gpu, ops)


@pytest.mark.parametrize("name", wlm_cases.SUM_NAMES)
def test_masked_pixels_are_not_read(gpu, name):
    wlm_cases.check_masked_pixels_are_not_read(name, gpu, ops)


@pytest.mark.parametrize("name", ("780_rays_zxy", "4087_rays_four_workgroups", "1025_rays"))
def test_power_of_four_scaling_of_the_weight(gpu, name):
    wlm_cases.check_power_of_four_scaling(name, gpu, ops)


def test_step_sequences_against_the_definition(gpu):
    wlm_cases.check_step_sequences(gpu, ops)


def test_registration_of_the_occluded_image(gpu):
    wlm_cases.check_registration(gpu, ops)


def test_python_surface_multi_starts_and_the_empty_pose(gpu):
    wlm_cases.check_python_surface(gpu, ops)


def test_weight_errors_name_the_condition(gpu):
    wlm_cases.check_weight_errors(gpu, torch.device("cpu"))
