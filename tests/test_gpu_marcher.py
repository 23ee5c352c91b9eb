"""On the MI355X: the marcher's brick entries (ddrr_trilinear_forward_bricks with and without its record,
ddrr_trilinear_backward_rays, the two channel variants, ddrr_trilinear_backward_volume_bricks on the owner-box
scenes) and the per-ray entries they are compared with, per pixel against float64: the checks of
tests/marcher_cases.py, which tests/test_marcher.py runs on the host emulation."""
import pytest

import marcher_cases as mc
from diffdrr_amd import ops

pytestmark = pytest.mark.gpu
ids = mc.case_id


@pytest.mark.parametrize("case", mc.CASES, ids=ids)
def test_forward_per_pixel(gpu, case):
    mc.check_forward(case, gpu, ops)


@pytest.mark.parametrize("case", mc.CASES, ids=ids)
def test_ray_gradients_per_pixel(gpu, case):
    mc.check_ray_gradients(case, gpu, ops)


@pytest.mark.parametrize("case", mc.CHANNEL_CASES, ids=ids)
def test_channels_per_pixel(gpu, case):
    mc.check_channels(case, gpu, ops)


@pytest.mark.parametrize("case", mc.ORDERING_CASES, ids=ids)
def test_a_pose_alone_equals_the_pose_in_a_batch(gpu, case):
    mc.check_ordering(case, gpu, ops)


@pytest.mark.parametrize("case", mc.OWNER_BOX_CASES, ids=ids)
def test_owner_box_volume_gradient_per_voxel(gpu, case):
    mc.check_owner_box(case, gpu, ops)
