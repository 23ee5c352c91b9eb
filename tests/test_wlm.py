"""Levenberg-Marquardt registration with a pixel weight, without a GPU: the host build of csrc/wlm_core.h
(tests/emu/wlm_emu.cpp) behind the product's own Python layers -- the 45 weighted sums and the per-ray Jacobian
against the float64 render route, the bit-for-bit properties of include/diffdrr_wlm_hip.h, the step against its
definition in float64, the registration of an occluded image, the Python surface and its errors."""
import pytest
import torch

import diffdrr_amd
import lm_cases
import wlm_cases
import wncc_cases
from diffdrr_amd import _lib

CPU = torch.device("cpu")


@pytest.fixture()
def wlm_ops(emulated_ops, monkeypatch):
    lm_cases.route_lm_to_emulation(monkeypatch, emulated_ops)
    wlm_cases.route_wlm_to_emulation(monkeypatch, emulated_ops)
    return emulated_ops


def test_surface_of_the_package():
    assert _lib.WLM_ABI_VERSION == 1 and _lib.WLM_SUMS == 45 == _lib.LM_SUMS + 1
    assert _lib.WLM_GROUP_RAYS == _lib.LM_GROUP_RAYS and _lib.WLM_STATE_DOUBLES == _lib.LM_STATE_DOUBLES
    for name in ("wlm_workspace", "wlm_normal_sums", "wlm_step", "_launch_wlm", "_query_wlm"):
        assert callable(getattr(diffdrr_amd.ops, name))
    assert not hasattr(diffdrr_amd, "weighted_normal_equations_reference")  # (nothing new exported)
    pq = wlm_cases.pair_table()
    assert pq.shape == (45, 2) and (pq[:44] == lm_cases.pair_table()).all() and tuple(pq[44]) == (8, 8)


def test_weighted_reference_is_the_gauss_newton_model_of_the_weighted_residual():
    wlm_cases.check_reference()


@pytest.mark.parametrize("name", wlm_cases.SUM_NAMES)
def test_sums_and_jacobian_against_float64(wlm_ops, name):
    wlm_cases.check_sums_and_jacobian(name, CPU, wlm_ops)


@pytest.mark.parametrize("name", wlm_cases.SUM_NAMES)
def test_bit_for_bit_properties(wlm_ops, name):
    wlm_cases.check_bit_for_bit_properties(name, CPU, wlm_ops)


def test_host_sums_from_the_kernels_own_rows(wlm_ops):
    wlm_cases.check_device_sums_from_the_devices_own_rows("4087_rays_four_workgroups", CPU, wlm_ops)


@pytest.mark.parametrize("name", wlm_cases.SUM_NAMES)
def test_masked_pixels_are_not_read(wlm_ops, name):
    wlm_cases.check_masked_pixels_are_not_read(name, CPU, wlm_ops)


@pytest.mark.parametrize("name", ("780_rays_zxy", "4087_rays_four_workgroups", "1025_rays"))
def test_power_of_four_scaling_of_the_weight(wlm_ops, name):
    wlm_cases.check_power_of_four_scaling(name, CPU, wlm_ops)


def test_step_sequences_against_the_definition(wlm_ops):
    wlm_cases.check_step_sequences(CPU, wlm_ops)


def test_registration_of_the_occluded_image(wlm_ops, monkeypatch):
    wncc_cases.route_wncc_to_emulation(monkeypatch, wlm_ops)  # (the Adam loop printed beside it)
    wlm_cases.check_registration(CPU, wlm_ops)


def test_python_surface_multi_starts_and_the_empty_pose(wlm_ops):
    wlm_cases.check_python_surface(CPU, wlm_ops)


def test_weight_errors_name_the_condition(wlm_ops):
    wlm_cases.check_weight_errors(CPU, torch.device("meta"))


def test_ops_reject_what_the_entries_would_misread(wlm_ops):
    wlm_cases.check_ops_errors(wlm_ops)
