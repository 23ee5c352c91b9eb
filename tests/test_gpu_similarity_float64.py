"""The similarity kernels on the MI355X against the float64 composition on radiograph-like images: what the host
twin (tests/test_similarity_float64.py) cannot reach -- the forward's tile walk, the LDS staging at every
instantiated window size, the backward's large-LDS launch, the scalar and misaligned loops of ncc_fwd_kernel.
Cases, reference and yardstick: tests/similarity_cases.py."""
import pytest

import similarity_cases as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,setting", S.PATCH_CASES)
def test_patch_ncc_against_float64(gpu, name, setting):
    S.check_patch_ncc(gpu, name, setting)


def test_patch_ncc_tile_walk_against_float64(gpu):
    S.check_patch_ncc_tile_walk(gpu)


@pytest.mark.parametrize("name,setting", S.NCC_CASES)
def test_whole_image_ncc_against_float64(gpu, name, setting):
    S.check_whole_image_ncc(gpu, name, setting)


@pytest.mark.parametrize("name,setting", S.SOBEL_CASES)
def test_sobel_against_float64(gpu, name, setting):
    S.check_sobel(gpu, name, setting)


@pytest.mark.parametrize("name,setting", S.CRITERION_CASES)
def test_criteria_against_float64(gpu, name, setting):
    S.check_end_to_end(gpu, name, setting)
