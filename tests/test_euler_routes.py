"""The fused Euler-pose routes without a GPU: the checks of tests/euler_route_cases.py on the host emulation --
which entries each route launches, where each route ends, and that every route computes the composition's numbers."""
import pytest
import torch

import euler_route_cases as E
import lm_cases
import wncc_cases

CPU = torch.device("cpu")


@pytest.fixture()
def ops(emulated_ops, monkeypatch):
    lm_cases.route_lm_to_emulation(monkeypatch, emulated_ops)
    wncc_cases.route_wncc_to_emulation(monkeypatch, emulated_ops)
    return emulated_ops


@pytest.mark.parametrize("B", (1, 3))
def test_every_route_launches_its_entries_in_order(ops, B):
    E.check_sequences(CPU, ops, B)


@pytest.mark.parametrize("flip", list(E.RENDER_BOUNDARIES[False]), ids=str)
@pytest.mark.parametrize("grad", (False, True), ids=("inference", "image"))
def test_render_route_boundaries(ops, grad, flip):
    E.check_render_boundary(CPU, ops, grad, flip)


@pytest.mark.parametrize("flip", list(E.NCC_BOUNDARIES), ids=str)
@pytest.mark.parametrize("weighted", (False, True), ids=("ncc", "wncc"))
def test_ncc_route_boundaries(ops, weighted, flip):
    E.check_ncc_boundary(CPU, ops, flip, weighted)


@pytest.mark.parametrize("weighted", (False, True), ids=("ncc", "wncc"))
def test_ncc_with_nothing_to_differentiate_composes(ops, weighted):
    E.check_ncc_without_a_gradient(CPU, ops, weighted)


def test_p_subsample_boundaries(ops):
    E.check_subsample_boundaries(CPU, ops)


def test_fixed_and_weight_boundaries(ops):
    E.check_fixed_and_weight_boundaries(CPU, ops)


def test_levenberg_marquardt_refuses_outside_its_domain(ops):
    E.check_lm_boundaries(CPU, ops)
