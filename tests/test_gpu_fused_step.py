"""The fused registration step on the MI355X: the checks of tests/test_fused_step.py through the gfx950 kernels, at
every launch-size variant of the two epilogues (csrc/pose_ncc.hip: forward <1> / <4>, backward <1024> / <2048>, either
side of the 512-workgroup threshold), on the 16-byte and the scalar load path, with ragged last workgroups.

Measured on an MI355X, largest err / own per case in units of 2^-24 fine (explicit backward dense | edge-hot | NCC
route): 1x2x3 0.46/0.46 | 1.2/0.8 | 0.03/0.12; 3x30x26 0.06/0.25 | 0.6/0.9 | 0.01/0.03; 2x67x61 0.04/0.10 | 0.36/0.21
| 0.003/0.02; 2x64x65 0.05/0.09 | 0.30/0.30 | 0.004/0.02; 511x30x26 12.3/12.5 | 10.6/10.6 | 1.5/1.6; 512x30x26
17.5/17.1 | 2.8/2.8 | 74.8/74.8; 256x68x63 4.8/4.8 | 3.1/3.2 | 0.43/0.44; 256x67x65 3.2/3.2 | 2.6/2.2 | 0.38/0.38.
Where a figure exceeds the floor of 8, one ray of the pose crosses a voxel plane at a grazing angle: 1 / (tv_a - sv_a)
is ill-conditioned there in any float32 evaluation, the torch composition is as far off, and the gate holds on 2 own.
Forward statistics: at most 5.7/5.8 (the six-ray case), 2.4/3.1 elsewhere."""
import pytest

import fused_step_cases as cases
from diffdrr_amd import ops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(cases.CASES))
def test_forward_against_float64(gpu, name):
    cases.check_forward(name, gpu, ops)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_ncc_backward_against_float64(gpu, name):
    cases.check_ncc_backward(name, gpu, ops)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_explicit_backward_dense_and_edge_hot_against_float64(gpu, name):
    cases.check_explicit_backward(name, gpu, ops)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_workspace_left_zero_and_second_call(gpu, name):
    cases.check_workspace_and_repeat(name, gpu, ops)


def test_pose_euler_every_convention_against_float64(gpu):
    cases.check_pose_euler(gpu, ops)


def test_pose_raygen_clears_exactly_what_it_is_given(gpu):
    cases.check_clears(gpu, ops)


def test_pose_adam_against_float64_adam(gpu):
    cases.check_pose_adam(gpu, ops)


def test_unfused_backward_on_both_float_records(gpu):
    cases.check_unfused_entry(gpu, ops)
