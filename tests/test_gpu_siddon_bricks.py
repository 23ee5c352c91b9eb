"""On the MI355X: the Siddon brick entries (ddrr_siddon_forward_bricks on every storage, with and without its record,
masked, with the packed record; the planes of the blocked record; ddrr_siddon_backward_rays on either record;
ddrr_siddon_forward_channels_bricks) per pixel against float64: the checks of tests/siddon_brick_cases.py, which
tests/test_siddon_bricks.py runs on the host emulation."""
import pytest

import siddon_brick_cases as sb
from diffdrr_amd import ops

pytestmark = pytest.mark.gpu

CASE_STORAGE = [(n, s) for n in sb.CASES for s in (sb.STORAGES_DEVICE if n in sb.GENERIC else ("f32", "q16", "q16py"))]


@pytest.mark.parametrize("name,storage", CASE_STORAGE, ids=lambda v: v)
def test_forward_and_record_per_pixel(gpu, name, storage):
    sb.check_forward_and_record(name, storage, gpu, ops)


@pytest.mark.parametrize("storage", ("f32", "q16p", "q16y"))
@pytest.mark.parametrize("name", sb.PACKED_CASES)
def test_packed_record_per_ray(gpu, name, storage):
    sb.check_packed_record(name, storage, gpu, ops)


@pytest.mark.parametrize("kind", sb.MASKS)
@pytest.mark.parametrize("name,storage", [("generic_21x19", "f32"), ("generic_24x20", "q16p"), ("sparse", "q16"),
                                          ("generic_21x19", "q16py")], ids=lambda v: v)
def test_masked_entry_per_pixel(gpu, name, storage, kind):
    sb.check_masked(name, kind, storage, gpu, ops)


@pytest.mark.parametrize("name", ["generic_21x19", "poses33_8x6"])
def test_record_into_buffers_cleared_by_the_ray_generation(gpu, name):
    sb.check_cleared(name, gpu, ops)


@pytest.mark.parametrize("name", sb.CHANNEL_CASES)
def test_channels_per_pixel(gpu, name):
    sb.check_channels(name, gpu, ops)
