"""MutualInformation on the MI355X: the fused kernels of include/diffdrr_mi_hip.h against the torch
composition of the reference's formula (diffdrr_amd.metrics.mutual_information).

Yardstick: the composition in float64 on the device.  The reference's own error is the same
composition in float32 (what the reference runs on a GPU); the fused route must stay within twice it.
"""
import numpy as np
import pytest
import torch

from diffdrr_amd import MutualInformation, ops
from diffdrr_amd.metrics import mutual_information
from mi_cases import _composition, _grad_gate, _images, _run, _value_gate

pytestmark = pytest.mark.gpu


CASES = [  # B, H, W, num_bins, sigma, normalize, images
    (1, 256, 256, 256, 0.1, True, "unit"),
    (3, 37, 53, 64, 0.1, False, "unit"),
    (8, 37, 53, 100, 0.02, True, "outside"),
    (3, 256, 256, 2, 0.5, True, "unit"),
    (3, 1, 1, 64, 0.1, True, "unit"),
    (3, 37, 53, 256, 0.5, False, "constant"),
    (8, 64, 64, 256, 0.1, True, "outside"),
]


@pytest.mark.parametrize("case", CASES, ids=[f"B{c[0]}_{c[1]}x{c[2]}_K{c[3]}_s{c[4]}_n{int(c[5])}_{c[6]}"
                                             for c in CASES])
def test_fused_mi_values_and_gradients_within_twice_the_fp32_error(gpu, case, monkeypatch):
    B, H, W, K, sigma, normalize, kind = case
    g = torch.Generator().manual_seed(B * 1000 + H + K)
    fixed, moving = (t.to(gpu) for t in _images(kind, B, H, W, g))
    w = (torch.rand(B, generator=g) + 0.5).to(gpu)
    crit = MutualInformation(sigma=sigma, num_bins=K, normalize=normalize).to(gpu)
    calls = []
    fwd, bwd = ops.mi_forward, ops.mi_backward
    monkeypatch.setattr(ops, "mi_forward", lambda *a, **k: (calls.append("f"), fwd(*a, **k))[1])
    monkeypatch.setattr(ops, "mi_backward", lambda *a, **k: (calls.append("b"), bwd(*a, **k))[1])
    for grad_of in ("moving", "fixed", "both"):
        for weights in (w, None):
            calls.clear()
            v, gm = _run(crit, fixed, moving, weights, grad_of)
            assert calls.count("f") == 1 and calls.count("b") == (2 if grad_of == "both" else 1), calls
            v32, g32 = _run(lambda a, b: _composition(crit, a, b, torch.float32), fixed, moving, weights, grad_of)
            v64, g64 = _run(lambda a, b: _composition(crit, a, b, torch.float64), fixed, moving, weights, grad_of)
            _value_gate(v, v32, v64)
            for mine, r32, r64 in zip(gm, g32, g64):
                assert mine.dtype == torch.float32 and mine.shape == r64.shape
                _grad_gate(mine, r32, r64, grad_of)


@pytest.mark.parametrize("K,normalize", [(1, False), (2, True), (256, True)])
def test_fused_mi_values_only(gpu, K, normalize):
    g = torch.Generator().manual_seed(K)
    crit = MutualInformation(num_bins=K, normalize=normalize).to(gpu)
    fixed, moving = (t.to(gpu) for t in _images("unit", 3, 37, 53, g))
    x1 = fixed.expand(3, -1, -1, -1)
    with torch.no_grad():
        _value_gate(crit(x1, moving), _composition(crit, x1, moving, torch.float32),
                    _composition(crit, x1, moving, torch.float64))


def test_nan_where_the_composition_is_nan(gpu):
    """Both images far outside the bins: every kernel value underflows, the entropies are 0 and the
    normalised value is 0 / 0 -- in the composition and in the kernels."""
    crit = MutualInformation().to(gpu)
    x1 = torch.full((2, 1, 16, 16), 40.0, device=gpu)
    x2 = torch.full((2, 1, 16, 16), -30.0, device=gpu)
    with torch.no_grad():
        ref = _composition(crit, x1, x2, torch.float64)
        assert torch.isnan(ref).all()
        assert torch.isnan(crit(x1, x2)).all()
    crit.normalize = False
    with torch.no_grad():
        assert torch.equal(crit(x1, x2).cpu(), _composition(crit, x1, x2, torch.float32).cpu())


def test_expanded_fixed_image_equals_materialised(gpu):
    g = torch.Generator().manual_seed(7)
    fixed, moving = (t.to(gpu) for t in _images("unit", 4, 48, 40, g))
    crit = MutualInformation(num_bins=128).to(gpu)
    res = []
    for x1 in (fixed.expand(4, -1, -1, -1), fixed.expand(4, -1, -1, -1).contiguous()):
        m = moving.clone().requires_grad_(True)
        v = crit(x1, m)
        (gm,) = torch.autograd.grad(v.sum(), [m])
        res.append((v.detach(), gm))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    # ... and an expanded MOVING image (both sides are read in place)
    with torch.no_grad():
        a = crit(moving, fixed.expand(4, -1, -1, -1))
        b = crit(moving, fixed.expand(4, -1, -1, -1).contiguous())
    assert torch.equal(a, b)


def test_both_images_expanded_equal_materialised(gpu):
    """Both sides expand()ed: read in place, and still B values and per-pose gradients."""
    g = torch.Generator().manual_seed(9)
    fixed, moving = (t.to(gpu) for t in _images("unit", 1, 40, 36, g))
    crit = MutualInformation(num_bins=64).to(gpu)
    res = []
    for expand in (True, False):
        a = fixed.clone().requires_grad_(True)
        b = moving.clone().requires_grad_(True)
        x1, x2 = a.expand(5, -1, -1, -1), b.expand(5, -1, -1, -1)
        if not expand:
            x1, x2 = x1.contiguous(), x2.contiguous()
        v = crit(x1, x2)
        assert v.shape == (5,)
        w = torch.arange(1.0, 6.0, device=gpu)
        res.append((v.detach(), *torch.autograd.grad((v * w).sum(), [a, b])))
    assert torch.equal(res[0][0], res[1][0])
    # (the gradients: the same per-pose gradients, summed over the batch by two different torch reductions)
    for x, y in zip(res[0][1:], res[1][1:]):
        assert torch.allclose(x, y, rtol=1e-5, atol=1e-7 * float(y.abs().max()))


def test_sigma_that_requires_grad_is_differentiated(gpu):
    g = torch.Generator().manual_seed(4)
    fixed, moving = (t.to(gpu) for t in _images("unit", 2, 20, 24, g))
    crit = MutualInformation(num_bins=32).to(gpu)
    crit.sigma.requires_grad_(True)
    v = crit(fixed.expand(2, -1, -1, -1), moving)
    (gs,) = torch.autograd.grad(v.sum(), [crit.sigma])
    s64 = crit.sigma.detach().double().requires_grad_(True)
    v64 = mutual_information(fixed.double().expand(2, -1, -1, -1), moving.double(), crit.bins.double(), s64)
    (g64,) = torch.autograd.grad(v64.sum(), [s64])
    assert torch.allclose(gs.double(), g64, rtol=1e-3, atol=1e-6)


def test_more_bins_than_the_kernels_take_the_composition(gpu, monkeypatch):
    calls = []
    monkeypatch.setattr(ops, "mi_forward", lambda *a, **k: calls.append(1))
    g = torch.Generator().manual_seed(3)
    fixed, moving = (t.to(gpu) for t in _images("unit", 2, 20, 24, g))
    crit = MutualInformation(num_bins=300).to(gpu)
    w = torch.tensor([1.0, 0.5], device=gpu)
    v, gm = _run(crit, fixed, moving, w, "both")
    v32, g32 = _run(lambda a, b: _composition(crit, a, b, torch.float32), fixed, moving, w, "both")
    v64, g64 = _run(lambda a, b: _composition(crit, a, b, torch.float64), fixed, moving, w, "both")
    assert not calls
    _value_gate(v, v32, v64)
    for mine, r32, r64 in zip(gm, g32, g64):
        _grad_gate(mine, r32, r64)


def test_forward_backward_is_bitwise_reproducible(gpu):
    g = torch.Generator().manual_seed(11)
    fixed, moving = (t.to(gpu) for t in _images("outside", 3, 256, 256, g))
    crit = MutualInformation().to(gpu)
    res = []
    for _ in range(2):
        a = fixed.clone().requires_grad_(True)
        b = moving.clone().requires_grad_(True)
        v = crit(a.expand(3, -1, -1, -1), b)
        res.append((v.detach(), *torch.autograd.grad(v.sum(), [a, b])))
    for x, y in zip(*res):
        assert torch.equal(x, y)


def test_edited_buffers_take_effect(gpu):
    """sigma and bins are read on the device at every call (no host copy is cached)."""
    g = torch.Generator().manual_seed(5)
    fixed, moving = (t.to(gpu) for t in _images("unit", 2, 30, 30, g))
    crit = MutualInformation(num_bins=64).to(gpu)
    with torch.no_grad():
        before = crit(fixed.expand(2, -1, -1, -1), moving)
        crit.sigma.fill_(0.05)
        crit.bins.mul_(0.5)
        after = crit(fixed.expand(2, -1, -1, -1), moving)
        ref = _composition(crit, fixed.expand(2, -1, -1, -1), moving, torch.float64)
    assert not torch.equal(before, after)
    assert torch.allclose(after.double(), ref, atol=1e-5)


def test_fused_forward_backward_memory_stays_small(gpu):
    """B = 8, 256^2, 256 bins: one (B, N, K) fp32 kernel-value tensor of the composition is 512 MiB."""
    g = torch.Generator().manual_seed(2)
    fixed, moving = (t.to(gpu) for t in _images("unit", 8, 256, 256, g))
    x1 = fixed.expand(8, -1, -1, -1)
    m = moving.clone().requires_grad_(True)
    crit = MutualInformation().to(gpu)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(gpu)
    base = torch.cuda.memory_allocated(gpu)
    v = crit(x1, m)
    (gm,) = torch.autograd.grad(v.sum(), [m])
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(gpu) - base
    assert torch.isfinite(gm).all()
    assert peak < 64 * 2**20, peak


def test_graphed_registration_iteration_with_mutual_information(gpu):
    """GraphedIteration captures and replays `criterion(target, reg())` with MI as the criterion: the
    losses of 6 replays equal those of the eager loop (the render's own atomics keep this from being
    bitwise), and the similarity rises."""
    from diffdrr_amd import DRR, GraphedIteration, Registration
    from diffdrr_amd.data import synthetic_subject

    drr = DRR(synthetic_subject(64, kind="phantom", seed=0), sdd=1020.0, height=64, delx=4.0,
              stop_gradients_through_grid_sample=True).to(gpu)
    true_rot = torch.zeros(1, 3, device=gpu)
    true_xyz = torch.tensor([[0.0, 850.0, 0.0]], device=gpu)
    with torch.no_grad():
        gt = drr(true_rot, true_xyz, parameterization="euler_angles", convention="ZXY")
    scale = float(gt.max()) * 1.1

    class ScaledMI(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.mi = MutualInformation(num_bins=64, sigma=0.05)

        def forward(self, x1, x2):
            return self.mi(x1 / scale, x2 / scale)

    crit = ScaledMI().to(gpu)
    r0 = true_rot + torch.tensor([[0.08, -0.05, 0.06]], device=gpu)
    x0 = true_xyz + torch.tensor([[8.0, -5.0, 6.0]], device=gpu)

    # learning rates that move the pose by ~0.005 rad / ~0.5 mm in the first step
    probe = Registration(drr, r0.clone(), x0.clone(), parameterization="euler_angles", convention="ZXY")
    crit(gt, probe()).sum().backward()
    lr_rot = 0.005 / float(probe._rotation.grad.abs().max())
    lr_xyz = 0.5 / float(probe._translation.grad.abs().max())

    def make():
        reg = Registration(drr, r0.clone(), x0.clone(), parameterization="euler_angles", convention="ZXY")
        opt = torch.optim.SGD([{"params": [reg._rotation], "lr": lr_rot},
                               {"params": [reg._translation], "lr": lr_xyz}], maximize=True)
        return reg, opt

    reg_e, opt_e = make()
    eager = []
    for _ in range(6):
        opt_e.zero_grad()
        loss = crit(gt, reg_e()).sum()
        loss.backward()
        opt_e.step()
        eager.append(loss.item())
    reg_g, opt_g = make()
    step = GraphedIteration(reg_g, crit, opt_g, gt, warmup=3)
    assert not step.fused_similarity
    graphed = [step().item() for _ in range(6)]
    assert np.allclose(graphed, eager, atol=2e-4), (graphed, eager)
    assert graphed[-1] > graphed[0], graphed
