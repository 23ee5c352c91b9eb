"""MutualInformation (reference diffdrr/metrics.py:110-139) on the host: the module's interface and the
torch composition route (CPU, float64), against an independent numpy float64 restatement of the formula.
No GPU needed."""
import numpy as np
import pytest
import torch

import diffdrr_amd
from diffdrr_amd import metrics


def numpy_mi(x1, x2, module):
    """kornia's marginal_pdf / joint_pdf and the reference's entropies, per pair, in float64, with the
    module's bins and sigma (float32 buffers, as in the reference: their values are float32-rounded)."""
    bins = module.bins.double().numpy()
    sigma, epsilon, normalize = float(module.sigma), module.epsilon, module.normalize
    out = []
    for a, b in zip(np.asarray(x1, np.float64).reshape(len(x1), -1), np.asarray(x2, np.float64).reshape(len(x2), -1)):
        k1 = np.exp(-0.5 * ((a[:, None] - bins[None, :]) / sigma) ** 2)
        k2 = np.exp(-0.5 * ((b[:, None] - bins[None, :]) / sigma) ** 2)
        p1, p2 = k1.mean(0), k2.mean(0)
        p1, p2 = p1 / (p1.sum() + epsilon), p2 / (p2.sum() + epsilon)
        joint = k1.T @ k2
        pj = joint / (joint.sum() + 1e-10)
        h1 = -(p1 * np.log2(p1 + epsilon)).sum()
        h2 = -(p2 * np.log2(p2 + epsilon)).sum()
        h12 = -(pj * np.log2(pj + epsilon)).sum()
        mi = h1 + h2 - h12
        out.append(2 * mi / (h1 + h2) if normalize else mi)
    return np.array(out)


def test_importable_with_the_reference_interface():
    assert diffdrr_amd.MutualInformation is metrics.MutualInformation
    m = metrics.MutualInformation()
    assert m.epsilon == 1e-10 and m.normalize is True
    assert m.sigma.dim() == 0 and float(m.sigma) == pytest.approx(0.1)
    assert m.sigma.dtype == m.bins.dtype == torch.float32
    assert torch.equal(m.bins, torch.linspace(0.0, 1.0, 256))
    assert list(m.state_dict()) == ["sigma", "bins"]
    assert [n for n, _ in m.named_buffers()] == ["sigma", "bins"]
    m2 = metrics.MutualInformation(sigma=0.3, num_bins=17, epsilon=1e-6, normalize=False)
    assert m2.bins.numel() == 17 and float(m2.sigma) == pytest.approx(0.3)
    assert m2.epsilon == 1e-6 and m2.normalize is False


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
# (one bin, normalised: 0 / 0 up to rounding -- not a comparable value)
@pytest.mark.parametrize("sigma,num_bins,normalize", [(s, k, n) for s, k in ((0.1, 256), (0.02, 64), (0.5, 9), (0.1, 1))
                                                      for n in (True, False) if not (k == 1 and n)])
def test_composition_matches_numpy_restatement(dtype, sigma, num_bins, normalize):
    g = torch.Generator().manual_seed(num_bins)
    x1 = torch.rand(3, 1, 13, 11, generator=g, dtype=torch.float64) * 1.4 - 0.2
    x2 = torch.rand(3, 1, 13, 11, generator=g, dtype=torch.float64)
    m = metrics.MutualInformation(sigma=sigma, num_bins=num_bins, normalize=normalize).to(dtype)
    got = m(x1.to(dtype), x2.to(dtype))
    assert got.dtype == dtype and got.shape == (3,)
    ref = numpy_mi(x1.numpy(), x2.numpy(), metrics.MutualInformation(sigma, num_bins, normalize=normalize))
    tol = 1e-10 if dtype == torch.float64 else 2e-5
    np.testing.assert_allclose(got.numpy(), ref, rtol=tol, atol=tol)


def test_expanded_fixed_image_on_the_host():
    g = torch.Generator().manual_seed(1)
    fixed = torch.rand(1, 1, 9, 8, generator=g, dtype=torch.float64)
    moving = torch.rand(4, 1, 9, 8, generator=g, dtype=torch.float64)
    m = metrics.MutualInformation(num_bins=32).double()
    a = m(fixed.expand(4, -1, -1, -1), moving)
    np.testing.assert_allclose(a.numpy(), numpy_mi(np.repeat(fixed.numpy(), 4, 0), moving.numpy(), m),
                               rtol=1e-10)


@pytest.mark.parametrize("normalize", [True, False])
def test_gradcheck_float64(normalize):
    g = torch.Generator().manual_seed(2)
    x1 = torch.rand(2, 1, 5, 7, generator=g, dtype=torch.float64, requires_grad=True)
    x2 = torch.rand(2, 1, 5, 7, generator=g, dtype=torch.float64, requires_grad=True)
    m = metrics.MutualInformation(sigma=0.2, num_bins=8, normalize=normalize).double()
    assert torch.autograd.gradcheck(lambda a, b: m(a, b), (x1, x2))


def test_bad_shapes_raise():
    m = metrics.MutualInformation(num_bins=8)
    with pytest.raises(ValueError, match="single|1, H, W"):
        m(torch.rand(2, 3, 5, 5), torch.rand(2, 3, 5, 5))
    with pytest.raises(ValueError, match="same size"):
        m(torch.rand(2, 1, 5, 5), torch.rand(2, 1, 5, 6))
    with pytest.raises(ValueError, match="same size"):
        m(torch.rand(1, 1, 5, 5), torch.rand(2, 1, 5, 5))


def test_fused_route_is_given_the_batch_size_when_both_images_are_expanded(monkeypatch):
    """Both images expand()ed: the kernels read one image per side in place, and the batch size is still
    B (the launch is stubbed here: what is checked is what the module hands to it)."""
    from diffdrr_amd import ops

    seen = []

    def fake_forward(x1, x2, bins, sigma, epsilon, normalize, B, want_state=True):
        seen.append((tuple(x1.shape), tuple(x2.shape), B))
        return torch.zeros(B), None

    monkeypatch.setattr(ops, "on_device", lambda t: True)
    monkeypatch.setattr(ops, "mi_forward", fake_forward)
    m = metrics.MutualInformation(num_bins=8)
    a, b = torch.rand(1, 1, 6, 5), torch.rand(1, 1, 6, 5)
    with torch.no_grad():
        out = m(a.expand(4, -1, -1, -1), b.expand(4, -1, -1, -1))
    assert out.shape == (4,)
    assert seen == [((1, 6, 5), (1, 6, 5), 4)]


def test_buffers_that_require_grad_take_the_composition(monkeypatch):
    """The kernels differentiate the images only: a module whose sigma / bins require grad is served by
    the composition, which differentiates through them."""
    from diffdrr_amd import ops

    monkeypatch.setattr(ops, "on_device", lambda t: True)
    monkeypatch.setattr(ops, "mi_forward", lambda *a, **k: pytest.fail("fused route taken"))
    m = metrics.MutualInformation(num_bins=8)
    m.sigma.requires_grad_(True)
    v = m(torch.rand(2, 1, 6, 5), torch.rand(2, 1, 6, 5))
    (gs,) = torch.autograd.grad(v.sum(), [m.sigma])
    assert torch.isfinite(gs) and gs != 0
