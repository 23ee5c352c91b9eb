"""Weighted multi-view Levenberg-Marquardt registration with a detector per view, without a GPU: the host build of
csrc/wmvlm_core.h (tests/emu/wmvlm_emu.cpp) behind the product's own Python layers -- the rays of S starts x V views
against the one-view entry with every view's detector points, the weighted sums and the per-ray Jacobian bit for bit
against ddrr_wlm_normal_sums per view and against the float64 render route, masked pixels, the step against
ddrr_wlm_step (one view), ddrr_mvlm_step (unit weights) and its definition in float64, the occluded and the
calibrated biplane registration, the Python surface and its errors."""
import pytest
import torch

import diffdrr_amd
import lm_cases
import mvlm_cases
import wlm_cases
import wmvlm_cases
from diffdrr_amd import _lib
from wmvlm_cases import NAMES, SMALL, SV, SV_IDS

CPU = torch.device("cpu")


@pytest.fixture()
def wmv_ops(emulated_ops, monkeypatch):
    lm_cases.route_lm_to_emulation(monkeypatch, emulated_ops)
    wlm_cases.route_wlm_to_emulation(monkeypatch, emulated_ops)
    mvlm_cases.route_mvlm_to_emulation(monkeypatch, emulated_ops)
    wmvlm_cases.route_wmvlm_to_emulation(monkeypatch, emulated_ops)
    return emulated_ops


def test_surface_of_the_package():
    cls = diffdrr_amd.WeightedMultiViewLevenbergMarquardt
    assert cls is diffdrr_amd.registration.WeightedMultiViewLevenbergMarquardt
    assert issubclass(cls, diffdrr_amd.MultiViewLevenbergMarquardt)
    assert _lib.WMVLM_ABI_VERSION == 1 and _lib.WMVLM_SUMS == 45 == _lib.WLM_SUMS
    assert _lib.WMVLM_GROUP_RAYS == _lib.LM_GROUP_RAYS and _lib.WMVLM_STATE_DOUBLES == _lib.LM_STATE_DOUBLES == 40
    assert _lib.WMVLM_MAX_POSES == 65535
    for name in ("wmvlm_workspace", "wmvlm_raygen", "wmvlm_normal_sums", "wmvlm_step", "_launch_wmvlm",
                 "_query_wmvlm"):
        assert callable(getattr(diffdrr_amd.ops, name))
    assert callable(diffdrr_amd.registration.weighted_multiview_normal_equations_reference)
    assert all(word in cls.__doc__ for word in ("per start", "graph", "DRR.ncc", "detectors", "weight"))
    # the three "Not built" sentences point at the new class
    assert "WeightedMultiViewLevenbergMarquardt" in diffdrr_amd.MultiViewLevenbergMarquardt.__doc__
    import inspect

    parent = inspect.signature(diffdrr_amd.MultiViewLevenbergMarquardt.__init__).parameters
    assert "weight" not in parent and "detectors" not in parent
    mine = list(inspect.signature(cls.__init__).parameters)
    assert mine[:6] == ["self", "reg", "fixed", "views", "weight", "detectors"]
    assert mine[6:] == ["damping", "up", "down", "damping_min", "damping_max", "eps"]


def test_reference_is_the_gauss_newton_model_of_the_stacked_weighted_residual():
    wmvlm_cases.check_reference()


@pytest.mark.parametrize("S,V", SV, ids=SV_IDS)
@pytest.mark.parametrize("name", NAMES)
def test_rays_equal_the_one_view_entry_with_each_views_detector_and_the_clears(wmv_ops, name, S, V):
    wmvlm_cases.check_raygen(name, S, V, CPU, wmv_ops)


@pytest.mark.parametrize("S,V", SV, ids=SV_IDS)
@pytest.mark.parametrize("name", NAMES)
def test_sums_and_jacobian_equal_the_weighted_one_view_entry_bit_for_bit(wmv_ops, name, S, V):
    wmvlm_cases.check_sums_bit_for_bit(name, S, V, CPU, wmv_ops)


@pytest.mark.parametrize("S,V", SV[1:], ids=SV_IDS[1:])
@pytest.mark.parametrize("name", NAMES)
def test_masked_pixels_are_not_read(wmv_ops, name, S, V):
    wmvlm_cases.check_masked_pixels_are_not_read(name, S, V, CPU, wmv_ops)


@pytest.mark.parametrize("S,V", SV, ids=SV_IDS)
@pytest.mark.parametrize("name", SMALL)
def test_sums_and_jacobian_against_float64(wmv_ops, name, S, V):
    wmvlm_cases.check_sums_against_float64(name, S, V, CPU, wmv_ops)


def test_step_with_one_view_is_the_weighted_one_view_step_bit_for_bit(wmv_ops):
    wmvlm_cases.check_step_one_view_is_wlm_step(CPU, wmv_ops)


@pytest.mark.parametrize("V", (2, 3))
def test_step_with_unit_weights_is_the_unweighted_multi_view_step(wmv_ops, V):
    wmvlm_cases.check_step_with_unit_weights_is_mvlm_step(V, CPU, wmv_ops)


@pytest.mark.parametrize("V", (2, 3))
def test_step_sequences_against_the_definition(wmv_ops, V):
    wmvlm_cases.check_step_sequences(V, CPU, wmv_ops)


def test_step_skips_a_view_without_weights(wmv_ops):
    wmvlm_cases.check_step_skips_empty_views(CPU, wmv_ops)


@pytest.mark.parametrize("V", (2, 3))
def test_step_under_scaled_weights(wmv_ops, V):
    wmvlm_cases.check_step_scaling(V, CPU, wmv_ops)


def test_step_of_a_start_does_not_depend_on_its_neighbours(wmv_ops):
    wmvlm_cases.check_step_neighbours(CPU, wmv_ops)


def test_registration_of_an_occluded_biplane_pair(wmv_ops):
    wmvlm_cases.check_occluded_biplane(CPU, wmv_ops)


def test_registration_with_a_detector_per_view(wmv_ops):
    wmvlm_cases.check_calibrated_biplane(CPU, wmv_ops)


def test_multi_starts_run_as_alone_jacobian_and_bookkeeping(wmv_ops):
    wmvlm_cases.check_multi_starts(CPU, wmv_ops)


def test_errors_name_the_condition(wmv_ops):
    wmvlm_cases.check_errors(CPU, torch.device("meta"))


def test_ops_reject_what_the_entries_would_misread(wmv_ops):
    wmvlm_cases.check_ops_errors(wmv_ops)


def test_entries_reject_strides_and_counts_before_anything_runs():
    wmvlm_cases.check_entries_refuse_bad_arguments()
