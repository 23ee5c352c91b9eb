"""Multi-view (biplane) Levenberg-Marquardt registration without a GPU: the host build of csrc/mvlm_core.h
(tests/emu/mvlm_emu.cpp) behind the product's own Python layers -- the rays of S starts x V views against the
one-view entry, the sums and the per-ray Jacobian bit for bit against ddrr_lm_normal_sums per view and against the
float64 render route at view_poses(...), the step against ddrr_lm_step (one view) and against its definition in
float64 (several), the conditioning a second view buys, the registration, the Python surface and its errors."""
import pytest
import torch

import diffdrr_amd
import lm_cases
import mvlm_cases
from diffdrr_amd import _lib
from mvlm_cases import NAMES, SV, SV_IDS

CPU = torch.device("cpu")


@pytest.fixture()
def mv_ops(emulated_ops, monkeypatch):
    lm_cases.route_lm_to_emulation(monkeypatch, emulated_ops)
    mvlm_cases.route_mvlm_to_emulation(monkeypatch, emulated_ops)
    return emulated_ops


def test_surface_of_the_package():
    assert diffdrr_amd.MultiViewLevenbergMarquardt is diffdrr_amd.registration.MultiViewLevenbergMarquardt
    assert _lib.MVLM_ABI_VERSION == 1 and _lib.MVLM_SUMS == 44 == _lib.LM_SUMS
    assert _lib.MVLM_GROUP_RAYS == _lib.LM_GROUP_RAYS and _lib.MVLM_STATE_DOUBLES == _lib.LM_STATE_DOUBLES == 40
    assert _lib.MVLM_MAX_POSES == 65535
    for name in ("mvlm_workspace", "mvlm_raygen", "mvlm_normal_sums", "mvlm_step", "_launch_mvlm", "_query_mvlm"):
        assert callable(getattr(diffdrr_amd.ops, name))
    for name in ("relative_views", "view_poses", "multiview_normal_equations_reference"):
        assert callable(getattr(diffdrr_amd.registration, name))
    doc = diffdrr_amd.MultiViewLevenbergMarquardt.__doc__
    assert all(word in doc for word in ("pixel weights", "detector per view", "graph", "DRR.ncc"))


def test_reference_is_the_gauss_newton_model_of_the_stacked_residual():
    mvlm_cases.check_reference()


def test_view_poses_and_relative_views():
    mvlm_cases.check_view_poses()


@pytest.mark.parametrize("S,V", SV, ids=SV_IDS)
@pytest.mark.parametrize("name", NAMES)
def test_rays_equal_the_one_view_entry_bit_for_bit_and_the_clears(mv_ops, name, S, V):
    mvlm_cases.check_raygen(name, S, V, CPU, mv_ops)


@pytest.mark.parametrize("S,V", SV, ids=SV_IDS)
@pytest.mark.parametrize("name", NAMES)
def test_sums_and_jacobian_equal_the_one_view_entry_bit_for_bit(mv_ops, name, S, V):
    mvlm_cases.check_sums_bit_for_bit(name, S, V, CPU, mv_ops)


@pytest.mark.parametrize("S,V", SV, ids=SV_IDS)
@pytest.mark.parametrize("name", NAMES)
def test_sums_and_jacobian_against_float64(mv_ops, name, S, V):
    mvlm_cases.check_sums_against_float64(name, S, V, CPU, mv_ops)


def test_step_with_one_view_is_the_one_view_step_bit_for_bit(mv_ops):
    mvlm_cases.check_step_one_view_is_lm_step(CPU, mv_ops)


@pytest.mark.parametrize("V", (2, 3))
def test_step_sequences_against_the_definition(mv_ops, V):
    mvlm_cases.check_step_sequences(V, CPU, mv_ops)


def test_a_second_view_conditions_the_depth_translation(mv_ops):
    mvlm_cases.check_conditioning(CPU)


def test_registration_from_two_views(mv_ops):
    mvlm_cases.check_registration(CPU, mv_ops)


def test_multi_starts_run_as_alone_jacobian_and_independence(mv_ops):
    mvlm_cases.check_multi_starts(CPU, mv_ops)


def test_errors_name_the_condition(mv_ops):
    mvlm_cases.check_errors(CPU, torch.device("meta"))


def test_ops_reject_what_the_entries_would_misread(mv_ops):
    mvlm_cases.check_ops_errors(mv_ops)
