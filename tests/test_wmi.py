"""The definition of the weighted (masked) mutual information: diffdrr_amd.metrics.weighted_mutual_information, the
yardstick of the kernels of include/diffdrr_wmi_hip.h and the route every call takes that they do not serve.  No GPU.

B = 3, 19 x 23 images partly outside the bins' [0, 1], K in {2, 8, 33, 256}, sigma in {0.1, 0.03}, normalised and
plain, in float64 and float32."""
import pytest
import torch

from diffdrr_amd import MutualInformation
from diffdrr_amd.metrics import mutual_information, weighted_mutual_information
from mi_cases import _images
from wmi_cases import F32, F64

B, H, W = 3, 19, 23
CASES = [(K, sigma, normalize) for K in (2, 8, 33, 256) for sigma in (0.1, 0.03) for normalize in (True, False)]
IDS = ["K%d-sigma%g-%s" % (K, s, "normalised" if n else "plain") for K, s, n in CASES]


def _scene(K, sigma, dtype, seed=0):
    g = torch.Generator().manual_seed(7 * K + int(1000 * sigma) + seed)
    fixed, moving = _images("outside", B, H, W, g)
    g_out = (torch.rand(B, generator=g) + 0.5).to(dtype)
    return (fixed.expand(B, -1, -1, -1).to(dtype).contiguous(), moving.to(dtype), g_out,
            torch.linspace(0.0, 1.0, K, dtype=dtype), torch.tensor(sigma, dtype=dtype))


def _value_and_grads(fn, x1, x2, g_out, *more):
    leaves = [t.clone().requires_grad_() for t in (x1, x2, *more)]
    v = fn(*leaves)
    return v.detach(), torch.autograd.grad((v * g_out).sum(), leaves)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["float64", "float32"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_unit_weight_is_mutual_information_exactly(case, dtype):
    K, sigma, normalize = case
    x1, x2, g_out, bins, sg = _scene(K, sigma, dtype)
    want = _value_and_grads(lambda a, b: mutual_information(a, b, bins, sg, 1e-10, normalize), x1, x2, g_out)
    for w in (torch.ones(1, 1, H, W, dtype=dtype), torch.ones(B, 1, H, W, dtype=dtype)):
        got = _value_and_grads(lambda a, b: weighted_mutual_information(a, b, w, bins, sg, 1e-10, normalize), x1, x2,
                               g_out)
        assert torch.equal(got[0], want[0])
        assert torch.equal(got[1][0], want[1][0]) and torch.equal(got[1][1], want[1][1])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_collimator_is_the_cropped_call(case):
    """A 0/1 mask that keeps columns 4..18 against mutual_information of the cropped images, in float64: value and
    gradients within 1e-12, and the gradient exactly 0 outside the mask."""
    K, sigma, normalize = case
    x1, x2, g_out, bins, sg = _scene(K, sigma, F64)
    w = torch.zeros(1, 1, H, W, dtype=F64)
    w[..., 4:19] = 1.0
    got = _value_and_grads(lambda a, b: weighted_mutual_information(a, b, w, bins, sg, 1e-10, normalize), x1, x2, g_out)
    want = _value_and_grads(lambda a, b: mutual_information(a, b, bins, sg, 1e-10, normalize),
                            x1[..., 4:19].contiguous(), x2[..., 4:19].contiguous(), g_out)
    assert float((got[0] - want[0]).abs().max()) <= 1e-12
    for mine, theirs in zip(got[1], want[1]):
        assert float((mine[..., 4:19] - theirs).abs().max()) <= 1e-12 * max(1.0, float(theirs.abs().max()))
        assert float(theirs.abs().max()) > 0
        assert bool((mine[..., :4] == 0).all()) and bool((mine[..., 19:] == 0).all())


@pytest.mark.parametrize("dtype", [F64, F32], ids=["float64", "float32"])
@pytest.mark.parametrize("normalize", [True, False], ids=["normalised", "plain"])
def test_nan_under_weight_zero_and_an_emptied_pair(normalize, dtype):
    """NaN and Inf where the weight is 0 change nothing and get the gradient exactly 0; a pair whose weights are all
    0 has the value 0 and a zero, finite gradient in everything, and the other pairs are what they are without it."""
    K, sigma = 33, 0.1
    x1, x2, g_out, bins, sg = _scene(K, sigma, dtype)
    g = torch.Generator().manual_seed(3)
    w = (torch.rand(B, 1, H, W, generator=g) < 0.6).to(dtype) * (0.5 + torch.rand(B, 1, H, W, generator=g).to(dtype))
    w[1] = 0.0
    off = w == 0
    fn = lambda a, b, ww: weighted_mutual_information(a, b, ww, bins, sg, 1e-10, normalize)  # noqa: E731
    clean = _value_and_grads(fn, x1, x2, g_out, w)
    bad = torch.tensor([float("nan"), float("inf"), -float("inf")], dtype=dtype)[torch.arange(W) % 3].expand_as(x1)
    dirty = _value_and_grads(fn, torch.where(off, bad, x1), torch.where(off, bad, x2), g_out, w)
    assert torch.equal(clean[0], dirty[0]) and bool(torch.isfinite(dirty[0]).all())
    for a, b in zip(clean[1], dirty[1]):
        assert torch.equal(a, b) and bool(torch.isfinite(b).all())
    assert bool((dirty[1][0][off] == 0).all()) and bool((dirty[1][1][off] == 0).all())
    assert float(dirty[0][1]) == 0.0
    assert all(bool((t[1] == 0).all()) for t in dirty[1])  # (images and weight of the emptied pair)
    keep = torch.tensor([0, 2])
    alone = _value_and_grads(fn, x1[keep], x2[keep], g_out[keep], w[keep])
    assert torch.equal(alone[0], dirty[0][keep])
    for a, b in zip(alone[1], dirty[1]):
        assert torch.equal(a, b[keep]) and float(a.abs().max()) > 0


def test_scaling_the_weight_is_not_an_identity_but_close():
    """4 w against w: the two epsilons and the joint normaliser's 1e-10 do not scale; <= 1e-9 in float64."""
    x1, x2, g_out, bins, sg = _scene(33, 0.1, F64)
    w = 0.25 + 1.5 * torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(4), dtype=F64)
    a, b = (weighted_mutual_information(x1, x2, s * w, bins, sg) for s in (1.0, 4.0))
    assert float((a - b).abs().max()) <= 1e-9


def test_module_on_the_cpu_returns_the_composition_and_refuses_bad_shapes():
    x1, x2, _, _, _ = _scene(32, 0.1, F32)
    crit = MutualInformation(num_bins=32)
    g = torch.Generator().manual_seed(5)
    for w in (torch.rand(1, 1, H, W, generator=g), torch.rand(B, 1, H, W, generator=g),
              torch.rand(1, 1, H, W, generator=g).expand(B, -1, -1, -1)):
        want = weighted_mutual_information(x1, x2, w, crit.bins, crit.sigma, crit.epsilon, crit.normalize)
        assert torch.equal(crit(x1, x2, weight=w), want)
    assert torch.equal(crit(x1, x2, weight=None), crit(x1, x2))
    for bad in (torch.ones(H, W), torch.ones(1, H, W), torch.ones(2, 1, H, W), torch.ones(1, 1, H, W + 1),
                torch.ones(B, 2, H, W)):
        with pytest.raises(ValueError, match=r"weight has shape .* expected"):
            crit(x1, x2, weight=bad)
    d64 = MutualInformation(num_bins=8).double()
    v = d64(x1.double(), x2.double(), weight=torch.ones(1, 1, H, W, dtype=F64))
    assert v.dtype == F64 and torch.equal(v, d64(x1.double(), x2.double()))


@pytest.mark.parametrize("normalize", [True, False], ids=["normalised", "plain"])
def test_gradcheck_images_and_weight(normalize):
    g = torch.Generator().manual_seed(6)
    x1 = torch.rand(2, 1, 5, 6, generator=g, dtype=F64).requires_grad_()
    x2 = torch.rand(2, 1, 5, 6, generator=g, dtype=F64).requires_grad_()
    w = (0.25 + torch.rand(2, 1, 5, 6, generator=g, dtype=F64)).requires_grad_()
    bins, sg = torch.linspace(0.0, 1.0, 4, dtype=F64), torch.tensor(0.2, dtype=F64)
    assert torch.autograd.gradcheck(lambda a, b, ww: weighted_mutual_information(a, b, ww, bins, sg, 1e-10, normalize),
                                    (x1, x2, w), eps=1e-6, atol=1e-7, rtol=1e-5)
