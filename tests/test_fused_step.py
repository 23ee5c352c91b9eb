"""The fused registration step without a GPU: the host emulation of csrc/pose_ncc.hip's entries (tests/emu/ddrr_emu.cpp,
the same cores compiled for the CPU) against the float64 definition of tests/fused_step_cases.py, at the cases
small enough for it; the definition itself against autograd; the wrappers' errors."""
import pytest
import torch

import fused_step_cases as cases

CPU = torch.device("cpu")


def test_cases_land_on_the_dispatch_they_were_chosen_for():
    """Both sides of either threshold, one and several workgroups per pose, ragged last workgroups, both load paths."""
    for name, (B, H, W, _) in cases.CASES.items():
        N, vector, fwd, bwd = cases.DISPATCH[name]
        assert N == H * W and vector == (N % 4 == 0)
        assert cases.forward_variant(B, N) == fwd and cases.backward_variant(B, N) == bwd, name
    seen = {(cases.DISPATCH[n][1], cases.DISPATCH[n][2][0], cases.DISPATCH[n][3][0]) for n in cases.CASES}
    assert seen == {(v, q, r) for v in (False, True) for q, r in ((1, 1024), (4, 2048))}
    assert cases.forward_variant(511, 780)[0] == 1 and cases.forward_variant(512, 780)[0] == 4
    assert cases.backward_variant(511, 780)[0] == 1024 and cases.backward_variant(512, 780)[0] == 2048
    assert cases.edge_set(6) == [0, 1, 2, 3, 4, 5]
    assert {255, 256, 1023, 1024, 2047, 2048, 4082, 4083, 4086} <= set(cases.edge_set(4087))


def test_written_out_chain_is_the_gradient_of_its_model(emulated_ops):
    cases.check_chain_against_autograd(CPU, emulated_ops)


@pytest.mark.parametrize("name", cases.HOST_CASES)
def test_forward_against_float64(emulated_ops, name):
    cases.check_forward(name, CPU, emulated_ops)


@pytest.mark.parametrize("name", cases.HOST_CASES)
def test_ncc_backward_against_float64(emulated_ops, name):
    cases.check_ncc_backward(name, CPU, emulated_ops)


@pytest.mark.parametrize("name", cases.HOST_CASES)
def test_explicit_backward_dense_and_edge_hot_against_float64(emulated_ops, name):
    cases.check_explicit_backward(name, CPU, emulated_ops)


@pytest.mark.parametrize("name", cases.HOST_CASES)
def test_workspace_left_zero_and_second_call(emulated_ops, name):
    cases.check_workspace_and_repeat(name, CPU, emulated_ops)


def test_pose_euler_every_convention_against_float64(emulated_ops):
    cases.check_pose_euler(CPU, emulated_ops)


def test_pose_raygen_clears_exactly_what_it_is_given(emulated_ops):
    cases.check_clears(CPU, emulated_ops)


def test_pose_adam_against_float64_adam(emulated_ops):
    cases.check_pose_adam(CPU, emulated_ops)


def test_unfused_backward_on_both_float_records(emulated_ops):
    cases.check_unfused_entry(CPU, emulated_ops)


def test_fused_entries_refuse_other_records_and_other_fixed_images(emulated_ops):
    cases.check_layout_errors(emulated_ops)
