"""The similarity kernels' arithmetic against the float64 composition on radiograph-like images, through the
host build of the kernel cores (tests/emu compiles the same ncc_patch_core.h, blur_core.h, sobel_core.h; the
launch code -- tiles, LDS staging, the vector loads -- is the device twin's: tests/test_gpu_similarity_float64.py).
Cases, reference and yardstick: tests/similarity_cases.py."""
import pytest
import torch

import similarity_cases as S

CPU = torch.device("cpu")


@pytest.mark.parametrize("name,setting", S.PATCH_CASES)
def test_patch_ncc_against_float64(emulated_ops, name, setting):
    S.check_patch_ncc(CPU, name, setting)


def test_patch_ncc_tile_walk_against_float64(emulated_ops):
    S.check_patch_ncc_tile_walk(CPU)


@pytest.mark.parametrize("name,setting", S.NCC_CASES)
def test_whole_image_ncc_against_float64(emulated_ops, name, setting):
    S.check_whole_image_ncc(CPU, name, setting)


@pytest.mark.parametrize("name,setting", S.SOBEL_CASES)
def test_sobel_against_float64(emulated_ops, name, setting):
    S.check_sobel(CPU, name, setting)


@pytest.mark.parametrize("name,setting", S.CRITERION_CASES)
def test_criteria_against_float64(emulated_ops, name, setting):
    S.check_end_to_end(CPU, name, setting)
