"""The weighted (masked) NCC on the MI355X: the checks of tests/wncc_cases.py (shared with the host emulation,
tests/test_wncc.py) on the gfx950 kernels of csrc/wncc.hip, with 256 poses of 4355 rays next to the small cases,
and one captured registration iteration with a weight."""
import pytest
import torch

import wncc_cases
from diffdrr_amd import _lib, ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(gpu):
    _lib.get_wncc_lib()  # fail loudly if the library was not built
    return gpu


@pytest.mark.parametrize("name", wncc_cases.GPU_CASES)
def test_weights_are_a_sharp_check_in_float64(dev, name):
    wncc_cases.check_sharpness(name, dev, ops)


@pytest.mark.parametrize("name", wncc_cases.GPU_CASES)
def test_fused_forward_against_float64(dev, name):
    wncc_cases.check_forward(name, dev, ops)


@pytest.mark.parametrize("name", wncc_cases.GPU_CASES)
def test_fused_backward_against_float64(dev, name):
    wncc_cases.check_backward(name, dev, ops)


@pytest.mark.parametrize("name", wncc_cases.GPU_CASES)
def test_masked_pixels_are_not_read(dev, name):
    wncc_cases.check_masked_pixels_are_not_read(name, dev, ops)


@pytest.mark.parametrize("name", wncc_cases.GPU_CASES)
def test_scaled_weights_and_repeated_calls_give_the_same_bits(dev, name):
    wncc_cases.check_scale_and_repeat(name, dev, ops)


@pytest.mark.parametrize("shape,setting", wncc_cases.IMAGE_CASES,
                         ids=[f"{'x'.join(map(str, s))}-{t}" for s, t in wncc_cases.IMAGE_CASES])
def test_image_entries_against_float64(dev, shape, setting):
    wncc_cases.check_image_entries(shape, setting, dev, ops)


def test_criteria_with_a_weight_and_their_routes(dev):
    wncc_cases.check_criteria_and_routes(dev, ops)


def test_module_route_and_fallbacks(dev):
    wncc_cases.check_module_route(dev, ops)


def test_registration_with_a_mask_converges_and_does_not_read_the_bar(dev):
    wncc_cases.check_registration(dev, ops)


def test_the_registration_scene_needs_the_mask(dev):
    wncc_cases.check_scene_needs_the_mask(dev, ops)


def test_graphed_iteration_with_a_weight_replays_the_eager_steps(dev):
    wncc_cases.check_graphed_iteration(dev, ops)


def test_ops_refuse_other_records_and_shapes_without_a_launch(dev):
    wncc_cases.check_layout_errors(ops)
