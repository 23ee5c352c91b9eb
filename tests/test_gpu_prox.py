"""The TV proximal operator and FISTA reconstruction on the MI355X: the checks of tests/test_prox.py through the
gfx950 kernels (libdiffdrr_prox_hip.so)."""
import pytest
import torch

import prox_cases
from diffdrr_amd import TotalVariation3d, ops
from prox_cases import MODES, SHAPES

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_against_float64(gpu, shape, mode):
    prox_cases.check_against_float64(shape, mode, gpu, ops)


def test_worst_case_against_float64(gpu):
    for mode in MODES:
        prox_cases.check_against_float64(SHAPES[-1], mode, gpu, ops)
    prox_cases.print_worst(gpu)


@pytest.mark.parametrize("mode", MODES)
def test_warm_start(gpu, mode):
    prox_cases.check_warm_start(mode, gpu, ops)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(5, 70, 9), (33, 18, 130)])
def test_extrapolation_epilogue(gpu, shape, mode):
    prox_cases.check_epilogue(shape, mode, gpu, ops)


def test_reproducible_also_on_a_second_stream(gpu):
    prox_cases.check_reproducible(gpu, ops, streams=(torch.cuda.Stream(gpu),))


def test_module_routes(gpu, monkeypatch):
    prox_cases.check_module_routes(gpu, ops, monkeypatch)


def test_cpu_tensors_and_bad_arguments_are_rejected(gpu):
    b = prox_cases.volume((2, 3, 4), "step")
    with pytest.raises(ValueError, match="GPU"):
        ops.prox_tv3d(b, 0.1, dual=torch.zeros(3, 2, 3, 4))
    with pytest.raises(ValueError, match="dual"):
        ops.prox_tv3d(b.to(gpu), 0.1, dual=torch.zeros(3, 2, 3, 4))
    with pytest.raises(ValueError, match="float32"):
        ops.prox_tv3d(b.double().to(gpu), 0.1, dual=torch.zeros(3, 2, 3, 4, device=gpu))
    # an empty volume is a no-op
    x, y = ops.prox_tv3d(torch.zeros(0, 3, 4, device=gpu), 0.1, dual=torch.zeros(3, 0, 3, 4, device=gpu))
    assert x.shape == (0, 3, 4) and y is None
    assert TotalVariation3d().prox(torch.zeros(0, 3, 4, device=gpu), 0.1).shape == (0, 3, 4)


@pytest.mark.parametrize("renderer", ["siddon", "trilinear"])
def test_lipschitz_and_the_descent_lemma(gpu, renderer):
    prox_cases.check_lipschitz(gpu, renderer)


def test_fista_step_does_not_synchronise(gpu):
    """torch raises on any host synchronisation while two steps run (after the first render has built what the
    renderer caches per scene)."""
    truth, drr, pose, kw, measured = prox_cases.projector_scene(gpu, 16, 24, 1.6)
    from diffdrr_amd import Reconstruction

    recon = Reconstruction(drr, lower=0.0).to(gpu)
    recon.lipschitz(*pose, iterations=2, **kw)  # (first use: builds and caches what the renderer caches)
    fista = recon.make_fista(1.0, TotalVariation3d.for_drr(drr), weight=1e-3, inner_iterations=2)
    fista.step(measured, *pose, **kw)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(2):
            fista.step(measured, *pose, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")


@pytest.fixture(scope="module")
def end_to_end(gpu):
    return prox_cases.fista_end_to_end(gpu)


def test_fista_end_to_end_against_the_torch_loop(end_to_end):
    """8 views of the 32^3 phantom, from zeros, density >= 0, isotropic TV with weight 2e-4, 10 warm-started inner
    iterations, 40 steps: the yardstick loop -- the same renderer, ``prox_total_variation_3d`` and torch arithmetic
    -- recovers the phantom (RMSE 0.0176 against the zero volume's 0.1013 on the host emulation), and the fused
    route agrees with it voxel-wise after three steps and in objective and RMSE after 40."""
    prox_cases.check_fista_end_to_end(end_to_end)
