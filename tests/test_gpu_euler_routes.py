"""The fused Euler-pose routes on the MI355X: the checks of tests/euler_route_cases.py (shared with the host
emulation, tests/test_euler_routes.py) on the gfx950 kernels, at the same shapes."""
import pytest

import euler_route_cases as E
from diffdrr_amd import _lib, ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(gpu):
    _lib.get_lm_lib(), _lib.get_wncc_lib()  # fail loudly if a library was not built
    return gpu


@pytest.mark.parametrize("B", (1, 3))
def test_every_route_launches_its_entries_in_order(dev, B):
    E.check_sequences(dev, ops, B)


@pytest.mark.parametrize("flip", list(E.RENDER_BOUNDARIES[False]), ids=str)
@pytest.mark.parametrize("grad", (False, True), ids=("inference", "image"))
def test_render_route_boundaries(dev, grad, flip):
    E.check_render_boundary(dev, ops, grad, flip)


@pytest.mark.parametrize("flip", list(E.NCC_BOUNDARIES), ids=str)
@pytest.mark.parametrize("weighted", (False, True), ids=("ncc", "wncc"))
def test_ncc_route_boundaries(dev, weighted, flip):
    E.check_ncc_boundary(dev, ops, flip, weighted)


@pytest.mark.parametrize("weighted", (False, True), ids=("ncc", "wncc"))
def test_ncc_with_nothing_to_differentiate_composes(dev, weighted):
    E.check_ncc_without_a_gradient(dev, ops, weighted)


def test_p_subsample_boundaries(dev):
    E.check_subsample_boundaries(dev, ops)


def test_fixed_and_weight_boundaries(dev):
    E.check_fixed_and_weight_boundaries(dev, ops)


def test_levenberg_marquardt_refuses_outside_its_domain(dev):
    E.check_lm_boundaries(dev, ops)
