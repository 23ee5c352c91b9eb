"""Reconstruction on the host: the total-variation composition against an independent numpy float64
restatement of its definition, the closed-form gradient the kernel computes against float64 autograd, and
the interfaces of TotalVariation3d, VolumeAdam and Reconstruction.  No GPU needed."""
import numpy as np
import pytest
import torch

import diffdrr_amd
from diffdrr_amd import DRR, reconstruction
from diffdrr_amd.data import synthetic_subject
from diffdrr_amd.reconstruction import Reconstruction, TotalVariation3d, VolumeAdam, total_variation_3d

SPACING = (0.7, 0.7, 2.5)
SHAPES = [(1, 1, 1), (2, 1, 1), (1, 1, 5), (1, 4, 3), (7, 5, 9)]
MODES = ["isotropic", "anisotropic"]


def numpy_differences(V, spacing):
    """Forward differences, zero past the last plane, by loops over the voxels."""
    Dx, Dy, Dz = V.shape
    d = np.zeros((3,) + V.shape)
    for i in range(Dx):
        for j in range(Dy):
            for k in range(Dz):
                if i + 1 < Dx:
                    d[0, i, j, k] = (V[i + 1, j, k] - V[i, j, k]) / spacing[0]
                if j + 1 < Dy:
                    d[1, i, j, k] = (V[i, j + 1, k] - V[i, j, k]) / spacing[1]
                if k + 1 < Dz:
                    d[2, i, j, k] = (V[i, j, k + 1] - V[i, j, k]) / spacing[2]
    return d


def numpy_tv(V, spacing, mode, eps):
    d = numpy_differences(np.asarray(V, np.float64), spacing)
    if mode == "isotropic":
        return np.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2 + eps ** 2).sum()
    return np.abs(d).sum()


def numpy_tv_gradient(V, spacing, mode, eps):
    """The closed form the kernel evaluates: dTV/dV = -(px + py + pz) + px[i-1] + py[j-1] + pz[k-1]."""
    d = numpy_differences(np.asarray(V, np.float64), spacing)
    s = np.asarray(spacing, np.float64).reshape(3, 1, 1, 1)
    if mode == "isotropic":
        p = d / (np.sqrt((d ** 2).sum(0) + eps ** 2) * s)
    else:
        p = np.sign(d) / s
    g = -p.sum(0)
    g[1:] += p[0, :-1]
    g[:, 1:] += p[1, :, :-1]
    g[:, :, 1:] += p[2, :, :, :-1]
    return g


def volume(shape, seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * 2.0 - 0.5).to(dtype)


def test_public_names():
    for name in ("Reconstruction", "TotalVariation3d", "VolumeAdam", "total_variation_3d"):
        assert getattr(diffdrr_amd, name) is getattr(reconstruction, name)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_composition_matches_numpy_restatement(shape, mode, dtype):
    V = volume(shape, seed=sum(shape), dtype=dtype)
    got = total_variation_3d(V, SPACING, mode, eps=1e-3)
    assert got.dtype == dtype and got.dim() == 0
    ref = numpy_tv(V.double().numpy(), SPACING, mode, 1e-3)
    tol = 1e-12 if dtype == torch.float64 else 1e-5
    np.testing.assert_allclose(float(got), ref, rtol=tol, atol=tol)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES + [(33, 17, 70)])
def test_closed_form_gradient_equals_float64_autograd(shape, mode):
    V = volume(shape, seed=1 + sum(shape)).requires_grad_(True)
    (g,) = torch.autograd.grad(total_variation_3d(V, SPACING, mode, eps=1e-3), [V])
    ref = numpy_tv_gradient(V.detach().numpy(), SPACING, mode, 1e-3)
    np.testing.assert_allclose(g.numpy(), ref, rtol=0, atol=1e-13)


@pytest.mark.parametrize("mode", MODES)
def test_gradcheck_float64(mode):
    # (anisotropic: |d| has a kink at d = 0 -- distinct random values have no equal neighbours)
    V = volume((4, 3, 5), seed=3).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda v: total_variation_3d(v, SPACING, mode, eps=1e-3), (V,))
    tv = TotalVariation3d(mode=mode, eps=1e-3, spacing=SPACING)
    assert torch.autograd.gradcheck(tv, (V,))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_gradient_of_a_zero_volume_is_exactly_zero(mode, dtype):
    V = torch.zeros(3, 4, 5, dtype=dtype, requires_grad=True)
    (g,) = torch.autograd.grad(total_variation_3d(V, SPACING, mode), [V])
    assert torch.equal(g, torch.zeros_like(g))
    assert np.all(numpy_tv_gradient(np.zeros((3, 4, 5)), SPACING, mode, 1e-3) == 0)


def test_module_defaults_and_errors():
    tv = TotalVariation3d()
    assert (tv.mode, tv.eps, tv.spacing) == ("isotropic", 1e-3, (1.0, 1.0, 1.0))
    assert list(tv.state_dict()) == []
    np.testing.assert_allclose(float(tv(volume((3, 4, 5), dtype=torch.float32))),
                               numpy_tv(volume((3, 4, 5)).numpy(), (1, 1, 1), "isotropic", 1e-3), rtol=1e-5)
    with pytest.raises(ValueError, match="mode"):
        TotalVariation3d(mode="huber")
    with pytest.raises(ValueError, match="spacing"):
        TotalVariation3d(spacing=(1.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="spacing"):
        TotalVariation3d(spacing=(1.0, 1.0))
    with pytest.raises(ValueError, match="eps"):
        TotalVariation3d(eps=-1.0)
    with pytest.raises(ValueError, match="Dx, Dy, Dz"):
        tv(torch.rand(2, 3, 4, 5))
    with pytest.raises(ValueError, match="Dx, Dy, Dz"):
        total_variation_3d(torch.rand(5, 5))
    with pytest.raises(ValueError, match="mode"):
        total_variation_3d(torch.rand(2, 3, 4), mode="l2")
    with pytest.raises(ValueError, match="shape"):
        tv.add_gradient_(torch.rand(2, 3, 4), torch.zeros(2, 3, 5))


def test_add_gradient_on_the_host_is_the_composition():
    V = volume((5, 4, 6), seed=5)
    tv = TotalVariation3d(mode="isotropic", eps=1e-2, spacing=SPACING)
    grad0 = volume((5, 4, 6), seed=6)
    grad = grad0.clone()
    value = tv.add_gradient_(V, grad, weight=0.25)
    assert not value.requires_grad
    np.testing.assert_allclose(float(value), numpy_tv(V.numpy(), SPACING, "isotropic", 1e-2), rtol=1e-12)
    np.testing.assert_allclose(grad.numpy(), grad0.numpy() + 0.25 * numpy_tv_gradient(V.numpy(), SPACING, "isotropic", 1e-2),
                               rtol=0, atol=1e-13)


def _stub_device(monkeypatch, seen):
    from diffdrr_amd import ops

    def fake_tv3d(volume, spacing=(1.0, 1.0, 1.0), mode="isotropic", eps=1e-3, grad=None, accumulate=False,
                  weight=1.0, scale=None):
        seen.append(dict(shape=tuple(volume.shape), spacing=spacing, mode=mode, eps=eps, grad=grad is not None,
                         accumulate=accumulate, weight=weight, scale=scale))
        if grad is not None and not accumulate:
            grad.fill_(2.0)
            if scale is not None:
                grad.mul_(scale)
        return torch.tensor(5.0)

    monkeypatch.setattr(ops, "on_device", lambda t: True)
    monkeypatch.setattr(ops, "tv3d", fake_tv3d)


def test_dispatch_float32_contiguous_device_volumes_take_the_kernel(monkeypatch):
    """The launch is stubbed: what is checked is which route the module takes and what it hands over."""
    seen = []
    _stub_device(monkeypatch, seen)
    tv = TotalVariation3d(mode="anisotropic", eps=1e-2, spacing=SPACING)
    V = torch.rand(3, 4, 5, requires_grad=True)
    out = tv(V)
    assert float(out.detach()) == 5.0 and len(seen) == 1
    assert seen[0] == dict(shape=(3, 4, 5), spacing=SPACING, mode="anisotropic", eps=1e-2, grad=False,
                           accumulate=False, weight=1.0, scale=None)
    # backward: one call that writes the gradient, the upstream gradient handed over as `scale`
    (3.0 * out).backward()
    assert len(seen) == 2 and seen[1]["grad"] and not seen[1]["accumulate"]
    assert seen[1]["scale"].shape == (1,) and float(seen[1]["scale"]) == 3.0
    assert torch.equal(V.grad, torch.full((3, 4, 5), 6.0))
    # the accumulate form
    grad = torch.zeros(3, 4, 5)
    tv.add_gradient_(V, grad, weight=0.5)
    assert seen[2]["accumulate"] and seen[2]["weight"] == 0.5 and seen[2]["grad"]


def test_dispatch_everything_else_takes_the_composition(monkeypatch):
    from diffdrr_amd import ops

    monkeypatch.setattr(ops, "on_device", lambda t: True)
    monkeypatch.setattr(ops, "tv3d", lambda *a, **k: pytest.fail("fused route taken"))
    tv = TotalVariation3d(spacing=SPACING)
    V64 = volume((4, 5, 6))
    strided = volume((4, 5, 12), dtype=torch.float32)[:, :, ::2]
    for V in (V64, strided):
        np.testing.assert_allclose(float(tv(V)), numpy_tv(V.double().numpy(), SPACING, "isotropic", 1e-3), rtol=1e-5)
        tv.add_gradient_(V, torch.zeros(V.shape, dtype=V.dtype))
    # a float32 volume with a strided gradient buffer: the composition as well
    tv.add_gradient_(volume((4, 5, 6), dtype=torch.float32), torch.zeros(4, 5, 12)[:, :, ::2])
    monkeypatch.setattr(ops, "on_device", lambda t: False)
    tv(volume((4, 5, 6), dtype=torch.float32))  # a host tensor


def test_ops_reject_bad_arguments_before_any_launch():
    from diffdrr_amd import ops

    V = torch.rand(3, 4, 5)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.tv3d(V)
    with pytest.raises(ValueError, match="Dx, Dy, Dz"):
        ops.tv3d(torch.rand(3, 4))
    with pytest.raises(ValueError, match="float32"):
        ops.tv3d(V.double())
    with pytest.raises(ValueError, match="contiguous"):
        ops.tv3d(torch.rand(3, 4, 10)[:, :, ::2])
    with pytest.raises(ValueError, match="float32"):
        ops.volume_adam_step(V.double(), V, V, V, torch.zeros(()), lr=0.1)


def test_volume_adam_state_layout_and_errors(monkeypatch):
    from diffdrr_amd import ops

    p = torch.nn.Parameter(torch.rand(3, 4, 5))
    with pytest.raises(ValueError, match="GPU"):
        VolumeAdam([p], lr=0.1)
    monkeypatch.setattr(ops, "on_device", lambda t: True)
    opt = VolumeAdam([p], lr=0.1, lower=0.0)
    assert isinstance(opt, torch.optim.Optimizer)
    assert list(opt.state[p]) == ["step", "exp_avg", "exp_avg_sq"]  # torch.optim.Adam's layout
    st = opt.state[p]
    assert st["step"].dim() == 0 and st["step"].dtype == torch.float32 and float(st["step"]) == 0.0
    assert st["exp_avg"].shape == st["exp_avg_sq"].shape == p.shape
    assert not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    g = opt.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["lower"], g["upper"], g["maximize"]) == \
        (0.1, (0.9, 0.999), 1e-8, 0.0, None, False)
    # the state round-trips through torch's own state_dict machinery, and into torch.optim.Adam's
    opt2 = VolumeAdam([p], lr=0.1)
    opt2.load_state_dict(opt.state_dict())
    assert list(opt2.state[p]) == ["step", "exp_avg", "exp_avg_sq"]
    # what step() hands to the launch (stubbed)
    seen = []
    monkeypatch.setattr(ops, "volume_adam_step", lambda *a, **k: seen.append((a, k)))
    opt.step()
    assert seen == []  # no gradient: nothing to do
    p.grad = torch.ones_like(p)
    opt.step()
    (a, k), = seen
    assert a[0] is p and a[2] is st["exp_avg"] and a[3] is st["exp_avg_sq"] and a[4] is st["step"]
    assert k == dict(lr=0.1, betas=(0.9, 0.999), eps=1e-8, lower=0.0, upper=None, maximize=False)
    with pytest.raises(ValueError, match="float32"):
        VolumeAdam([torch.nn.Parameter(torch.rand(3, dtype=torch.float64))], lr=0.1)
    with pytest.raises(ValueError, match="contiguous"):
        VolumeAdam([torch.nn.Parameter(torch.rand(3, 8)[:, ::2])], lr=0.1)
    with pytest.raises(ValueError, match="learning rate"):
        VolumeAdam([p], lr=-1.0)
    with pytest.raises(ValueError, match="betas"):
        VolumeAdam([p], lr=0.1, betas=(1.0, 0.999))
    with pytest.raises(ValueError, match="lower"):
        VolumeAdam([p], lr=0.1, lower=1.0, upper=0.0)


def _drr(size=8):
    return DRR(synthetic_subject(size, kind="phantom", seed=0), sdd=300.0, height=6, delx=2.4)


def test_reconstruction_parameter_init_and_state_dict():
    drr = _drr()
    theirs = drr.density
    recon = Reconstruction(drr)
    assert isinstance(recon.density, torch.nn.Parameter) and recon.density.requires_grad
    assert recon.density.shape == drr.density.shape and recon.density.dtype == torch.float32
    assert not recon.density.any()
    assert [n for n, _ in recon.named_parameters()] == ["density"]
    assert (recon.lower, recon.upper) == (0.0, None)
    assert "density" in recon.state_dict() and "drr.density" in recon.state_dict()
    init = torch.rand(drr.density.shape, dtype=torch.float64)
    recon2 = Reconstruction(drr, init=init, lower=None, upper=2.0)
    assert recon2.density.dtype == torch.float32 and torch.equal(recon2.density.detach(), init.float())
    assert recon2.density.data_ptr() != init.data_ptr()
    recon.load_state_dict(recon2.state_dict())
    assert torch.equal(recon.density.detach(), recon2.density.detach())
    with pytest.raises(ValueError, match="shape"):
        Reconstruction(drr, init=torch.zeros(2, 2, 2))
    with pytest.raises(ValueError, match="lower"):
        Reconstruction(drr, lower=1.0, upper=0.0)
    # the swap that makes `drr` render the parameter is undone, also when the render raises
    with recon._own_density():
        assert drr.density is recon.density
    assert drr.density is theirs
    with pytest.raises(RuntimeError):
        recon(torch.zeros(1, 3), torch.zeros(1, 3), parameterization="euler_angles", convention="ZXY")
    assert drr.density is theirs and [n for n, _ in drr.named_buffers() if n == "density"] == ["density"]
