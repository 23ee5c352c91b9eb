"""The TV proximal operator and FISTA without a GPU: the float64 definition (``prox_total_variation_3d``) against
the properties a prox has, and the host build of the kernels' per-voxel arithmetic (tests/emu/prox_emu.cpp)
against the definition.  The same checks run through the gfx950 kernels in tests/test_gpu_prox.py."""
import itertools

import pytest
import torch

import diffdrr_amd
import prox_cases
from diffdrr_amd import (Fista, Reconstruction, TotalVariation3d, ops, prox_total_variation_3d, reconstruction,
                         total_variation_3d, tv_divergence_adjoint, tv_gradient_operator)
from prox_cases import MODES, SHAPES, SPACINGS

CPU = torch.device("cpu")


def test_public_names():
    for name in ("Fista", "prox_total_variation_3d", "tv_gradient_operator", "tv_divergence_adjoint"):
        assert getattr(diffdrr_amd, name) is getattr(reconstruction, name)
    assert hasattr(TotalVariation3d, "prox") and hasattr(Reconstruction, "lipschitz")
    assert hasattr(Reconstruction, "make_fista")


# ---------------------------------------------------------------------------- 1. the definition, float64
@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("shape", SHAPES)
def test_divergence_is_the_adjoint_of_the_difference_operator(shape, spacing):
    g = torch.Generator().manual_seed(1)
    x = torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 0.5
    p = torch.rand(3, *shape, generator=g, dtype=torch.float64) * 2 - 1  # (the last planes too: they must not count)
    lhs, rhs = (tv_gradient_operator(x, spacing) * p).sum(), (x * tv_divergence_adjoint(p, spacing)).sum()
    assert abs(float(lhs - rhs)) <= 1e-12 * float(x.norm() * p.norm())
    D = tv_gradient_operator(x, spacing)
    assert float(D.pow(2).sum(0).sqrt().sum()) == pytest.approx(float(total_variation_3d(x, spacing, "isotropic", 0.0)),
                                                               rel=1e-14)
    assert float(D.abs().sum()) == pytest.approx(float(total_variation_3d(x, spacing, "anisotropic", 0.0)), rel=1e-14)
    assert not bool(D[0, -1].any()) and not bool(D[1, :, -1].any()) and not bool(D[2, :, :, -1].any())


@pytest.mark.parametrize("mode", MODES)
def test_duality_gap_closes(mode):
    """The unconstrained gap, relative to lambda TV(b): never negative, non-increasing over 10 -> 50 -> 200
    iterations, at most 1e-5 at 200 for lambda = 0.05 (measured: 3.1e-9 isotropic, 3.4e-7 anisotropic); and the
    iterate is no worse than b itself or its mean."""
    shape, spacing, lam = prox_cases.GAP_SHAPE, (1.0, 1.0, 1.0), 0.05
    b = prox_cases.volume(shape, "step").double()
    gaps = []
    for n in (10, 50, 200):
        x, p = prox_total_variation_3d(b, lam, spacing, mode, n)
        assert float(p.pow(2).sum(0).max() if mode == "isotropic" else p.abs().max()) <= 1.0 + 1e-12
        gaps.append(prox_cases.duality_gap(x, p, b, lam, spacing, mode))
    print(f"{mode}: relative duality gaps at 10, 50, 200 iterations: {gaps}")
    assert all(g >= -1e-12 for g in gaps) and gaps[0] >= gaps[1] >= gaps[2] and gaps[2] <= 1e-5
    P = lambda v: prox_cases.primal_objective(v, b, lam, spacing, mode)  # noqa: E731
    assert P(x) <= P(b) and P(x) <= P(torch.full_like(b, float(b.mean())))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_exact_cases_of_the_definition(shape, mode):
    b = prox_cases.volume(shape, "step").double()
    lo, hi = prox_cases.BOUNDS
    for spacing in SPACINGS:
        warm = prox_cases.dual_start(shape, 0.5).double()
        x, p = prox_total_variation_3d(b, 0.0, spacing, mode, 10, lo, hi, warm.clone())
        assert torch.equal(x, b.clamp(lo, hi)) and torch.equal(p, warm)            # lambda = 0
        x, p = prox_total_variation_3d(b, 0.5, spacing, mode, 0, lo, hi)
        assert torch.equal(x, b.clamp(lo, hi)) and not bool(p.any())                 # no iterations, zero dual
        c = prox_cases.volume(shape, "constant").double()
        x, p = prox_total_variation_3d(c, 0.5, spacing, mode, 10)
        assert torch.equal(x, c) and not bool(p.any())                               # a constant is a fixed point
        x, _ = prox_total_variation_3d(b, 0.5, spacing, mode, 10, lo, hi)
        assert float(x.min()) >= lo and float(x.max()) <= hi
        clipped = float(((b < lo) | (b > hi)).double().mean())
        assert b.numel() < 100 or 0.25 <= clipped <= 0.42, clipped                   # "about a third"


def test_definition_rejects_bad_arguments():
    b = torch.zeros(3, 4, 5)
    for kw, what in ((dict(weight=-1.0), "weight"), (dict(weight=float("nan")), "weight"),
                     (dict(weight=0.1, iterations=-1), "iterations"), (dict(weight=0.1, mode="tv"), "mode"),
                     (dict(weight=0.1, spacing=(1.0, 0.0, 1.0)), "spacing"),
                     (dict(weight=0.1, lower=1.0, upper=0.0), "lower"),
                     (dict(weight=0.1, dual=torch.zeros(3, 4, 5, 5)), "dual"),
                     (dict(weight=0.1, dual=torch.zeros(3, 3, 4, 5, dtype=torch.float64)), "dual")):
        with pytest.raises(ValueError, match=what):
            prox_total_variation_3d(b, **kw)
    with pytest.raises(ValueError, match="volume"):
        prox_total_variation_3d(torch.zeros(4, 5), 0.1)
    x = torch.zeros(3, 4, 5, requires_grad=True)
    assert not prox_total_variation_3d(x, 0.1)[0].requires_grad


# ------------------------------------------------------------- 2. - 6. the host build of the kernels' arithmetic
@pytest.fixture()
def emulated_prox(monkeypatch):
    prox_cases.route_prox_to_emulation(monkeypatch, ops)
    return ops


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_emulation_against_float64(emulated_prox, shape, mode):
    prox_cases.check_against_float64(shape, mode, CPU, emulated_prox)


def test_emulation_worst_case(emulated_prox):
    for shape, mode in itertools.product(SHAPES[-2:], MODES):
        prox_cases.check_against_float64(shape, mode, CPU, emulated_prox)
    prox_cases.print_worst(CPU)


@pytest.mark.parametrize("mode", MODES)
def test_warm_start(emulated_prox, mode):
    prox_cases.check_warm_start(mode, CPU, emulated_prox)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(5, 70, 9), (33, 18, 130)])
def test_extrapolation_epilogue(emulated_prox, shape, mode):
    prox_cases.check_epilogue(shape, mode, CPU, emulated_prox)


def test_reproducible(emulated_prox):
    prox_cases.check_reproducible(CPU, emulated_prox)


def test_module_routes(monkeypatch):
    prox_cases.route_prox_to_emulation(monkeypatch, ops)
    # (on the host every tensor counts as the device's: what is left of the rule is dtype and strides)
    prox_cases.check_module_routes(CPU, ops, monkeypatch)


def test_module_on_the_host_is_the_composition():
    b = prox_cases.volume((5, 70, 9), "step")
    tv = TotalVariation3d(mode="anisotropic", spacing=(0.8, 1.7, 2.5))
    dual = torch.zeros(3, *b.shape)
    x = tv.prox(b, 0.05, 7, lower=0.2, dual=dual)
    ref, p = prox_total_variation_3d(b, 0.05, tv.spacing, tv.mode, 7, 0.2)
    assert torch.equal(x, ref) and torch.equal(dual, p)
    assert "eps" in TotalVariation3d.prox.__doc__


# ------------------------------------------------------------------------------------- 7., 8. the outer loop
@pytest.fixture()
def emulated_everything(emulated_ops, monkeypatch):
    prox_cases.route_prox_to_emulation(monkeypatch, emulated_ops)
    return emulated_ops


@pytest.mark.parametrize("renderer", ["siddon", "trilinear"])
def test_lipschitz_and_the_descent_lemma(emulated_everything, renderer):
    prox_cases.check_lipschitz(CPU, renderer)


def test_fista_state_and_errors(emulated_everything):
    truth, drr, pose, kw, measured = prox_cases.projector_scene(CPU, 8, 8, 2.4)
    recon = Reconstruction(drr, lower=0.0)
    for args, what in (((0.0,), "lipschitz"), ((float("inf"),), "lipschitz"), ((1.0, None, -1.0), "weight"),
                       ((1.0, None, 0.0, -1), "inner_iterations"), ((1.0, object(), 1.0), "regularizer")):
        with pytest.raises(ValueError, match=what):
            Fista(recon, *args)
    with pytest.raises(ValueError, match="iterations"):
        recon.lipschitz(*pose, iterations=0, **kw)
    L = recon.lipschitz(*pose, iterations=4, **kw)
    assert len(recon.lipschitz_history) == 4
    tv = TotalVariation3d.for_drr(drr)
    fista = recon.make_fista(L, tv, weight=1e-3, inner_iterations=3)
    assert isinstance(fista, Fista) and fista.t == 1.0 and fista.dual is None and torch.equal(fista.y, recon.density)
    losses = []
    for _ in range(3):
        data, value = fista.step(measured, *pose, **kw)
        assert data.dim() == value.dim() == 0 and float(recon.density.detach().min()) >= 0.0
        losses.append(float(data))
    assert fista.t > 1.0 and fista.dual.shape == (3, 8, 8, 8) and not torch.equal(fista.y, recon.density)
    assert losses[2] < losses[0] and float(value) == pytest.approx(
        float(total_variation_3d(recon.density.detach(), tv.spacing, tv.mode, 0.0)))
    fista.restart()
    assert fista.t == 1.0 and fista.dual is None and torch.equal(fista.y, recon.density)
    with pytest.raises(ValueError, match="measured"):
        fista.step(measured[:1], *pose, **kw)
    # without a regulariser: projected FISTA, the same state
    plain = Reconstruction(drr, lower=0.0).make_fista(L)
    data, value = plain.step(measured, *pose, **kw)
    assert float(value) == 0.0 and plain.dual is None and float(plain.recon.density.detach().min()) >= 0.0
    assert float(data) == pytest.approx(losses[0], rel=1e-6)  # (the first step's data loss: at zeros either way)


def test_fista_end_to_end_on_the_host(emulated_everything):
    """Item 8 with the renderer's and the prox's host builds (the device runs tests/test_gpu_prox.py's)."""
    prox_cases.check_fista_end_to_end(prox_cases.fista_end_to_end(CPU))
