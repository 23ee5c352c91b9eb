"""Reconstruction on the MI355X: the kernels of include/diffdrr_recon_hip.h against the torch compositions
they replace, and the module on top of them against the same iteration built from torch ops.

Yardsticks: the composition in float64 on the device, evaluated on the SAME float32 values (float64
originals rounded to float32 flip the signs of near-zero differences: an error of the input, not of the
code).  How far is acceptable: the float32 composition's own distance from that float64 result, doubled,
plus a floor from the number format (stated at each gate).
"""
import math

import pytest
import torch

from diffdrr_amd import DRR, Reconstruction, TotalVariation3d, VolumeAdam, ops, total_variation_3d
from diffdrr_amd.data import make_subject, phantom_volume, synthetic_subject
from diffdrr_amd.pose import convert

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 1, 1), (1, 1, 5), (33, 17, 70), (257, 130, 67), (512, 512, 133), (256, 256, 256),
          (512, 512, 512)]
KINDS = ["noise", "phantom", "zeros", "constant", "negative"]
SPACINGS = [(1.0, 1.0, 1.0), (0.7, 0.7, 2.5)]
MODES = ["isotropic", "anisotropic"]
EPS = 1e-3
_phantoms = {}


def make_volume(kind, shape, device):
    g = torch.Generator(device=device).manual_seed(sum(shape) + len(kind))
    if kind == "noise":
        return torch.rand(shape, generator=g, device=device)
    if kind == "negative":
        return torch.rand(shape, generator=g, device=device) * 3.0 - 2.0
    if kind == "zeros":
        return torch.zeros(shape, device=device)
    if kind == "constant":
        return torch.full(shape, 0.37, device=device)
    if shape not in _phantoms:  # (built on the host, the last shape kept)
        _phantoms.clear()
        _phantoms[shape] = phantom_volume(shape, seed=0).contiguous()
    return _phantoms[shape].to(device)


def composition(volume, spacing, mode, dtype):
    """-> (value, gradient) of the torch composition in `dtype`, as float64 tensors."""
    v = volume.to(dtype).requires_grad_(True)
    value = total_variation_3d(v, spacing, mode, EPS)
    (g,) = torch.autograd.grad(value, [v])
    return value.detach().double(), g.double()


def ulp(x):
    """The spacing of float32 at |x|."""
    a = x.abs()
    return (torch.nextafter(a, torch.full_like(a, math.inf)) - a).double()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tv_value_and_gradient_within_twice_the_fp32_composition(gpu, shape, kind):
    V = make_volume(kind, shape, gpu)
    for spacing in SPACINGS:
        # |dTV/dV| <= G: at most six terms, each of magnitude <= 1 / s; each is allowed a few ulp (a
        # reciprocal square root, a multiplication by 1 / s instead of a division): 8 * 2^-24 * G
        G = 2.0 * sum(1.0 / s for s in spacing)
        for mode in MODES:
            v64, g64 = composition(V, spacing, mode, torch.float64)
            v32, g32 = composition(V, spacing, mode, torch.float32)
            what = (shape, kind, spacing, mode)
            # the three call forms
            value_only = ops.tv3d(V, spacing, mode, EPS)
            written = torch.full_like(V, float("nan"))
            value_w = ops.tv3d(V, spacing, mode, EPS, grad=written)
            g0 = torch.randn(shape, device=gpu, generator=torch.Generator(device=gpu).manual_seed(1))
            acc = g0.clone()
            weight, scale = 0.37, torch.tensor([1.7], device=gpu)
            value_a = ops.tv3d(V, spacing, mode, EPS, grad=acc, accumulate=True, weight=weight, scale=scale)
            assert torch.equal(value_only, value_w) and torch.equal(value_only, value_a), what
            # value: within twice the float32 composition's error plus a relative 1e-6
            err, ref = abs(float(value_only) - float(v64)), abs(float(v32) - float(v64))
            print(f"{what}: value {float(value_only):.9g} f64 {float(v64):.12g} err {err:.3g} fp32 composition {ref:.3g}")
            assert math.isfinite(float(value_only)) and err <= 2 * ref + 1e-6 * abs(float(v64)), what
            # gradient, max abs per voxel
            gerr, gref = float((written.double() - g64).abs().max()), float((g32 - g64).abs().max())
            print(f"{what}: gradient err {gerr:.3g} fp32 composition {gref:.3g} floor {8 * 2.0 ** -24 * G:.3g}")
            assert gerr <= max(2 * gref, 8 * 2.0 ** -24 * G), what
            if kind in ("zeros", "constant"):
                assert not written.any(), what  # sign(0) = 0 and 0 / eps = 0: exactly zero
            # accumulate = grad0 + (weight * scale) * written, one fused multiply-add: within 2 ulp of it
            w = (torch.tensor(weight, dtype=torch.float32, device=gpu) * scale).double()
            expect = g0.double() + w * written.double()
            assert bool(((acc.double() - expect).abs() <= 2 * ulp(acc)).all()), what


@pytest.mark.parametrize("mode", MODES)
def test_tv_is_bitwise_reproducible(gpu, mode):
    V = make_volume("noise", (257, 130, 67), gpu)
    outs = []
    for _ in range(2):
        g = torch.zeros_like(V)
        outs.append((ops.tv3d(V, (0.7, 0.7, 2.5), mode, EPS, grad=g), g))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_tv_module_routes_through_the_kernel_and_autograd(gpu, monkeypatch):
    calls = []
    real = ops.tv3d
    monkeypatch.setattr(ops, "tv3d", lambda *a, **k: (calls.append(k), real(*a, **k))[1])
    V = make_volume("phantom", (33, 17, 70), gpu).requires_grad_(True)
    tv = TotalVariation3d(mode="isotropic", eps=EPS, spacing=(0.7, 0.7, 2.5))
    (2.5 * tv(V)).backward()
    assert len(calls) == 2 and calls[1]["scale"] is not None  # one launch each way, upstream as `scale`
    _, g64 = composition(V.detach(), tv.spacing, tv.mode, torch.float64)
    assert float((V.grad.double() - 2.5 * g64).abs().max()) <= 2.5 * 8 * 2.0 ** -24 * 2.0 * (2 / 0.7 + 1 / 2.5)
    # the accumulate form returns the value and adds in place
    grad = torch.ones_like(V)
    value = tv.add_gradient_(V, grad, weight=0.5)
    assert torch.equal(value, tv(V).detach())
    assert float((grad.double() - 1.0 - 0.5 * g64).abs().max()) <= 2e-6
    # a for_drr module takes the affine's spacing
    drr = DRR(make_subject(torch.rand(8, 9, 10), (0.7, 0.8, 2.5)), sdd=300.0, height=8, delx=2.0).to(gpu)
    assert TotalVariation3d.for_drr(drr).spacing == pytest.approx((0.7, 0.8, 2.5), rel=1e-6)


def test_tv_above_2_to_the_31_voxels(gpu):
    shape = (1290, 1290, 1291)
    n = shape[0] * shape[1] * shape[2]
    assert n > 2**31
    free, _ = torch.cuda.mem_get_info(gpu)
    need = 2 * 4 * n + (4 << 30)  # volume, gradient, and room for the slabs' float64 composition
    if free < need:
        pytest.skip(f"{free / 2**30:.0f} GiB of device memory free, the tensors need {need / 2**30:.0f} GiB")
    spacing, mode = (0.7, 0.7, 2.5), "isotropic"
    V = torch.rand(shape, device=gpu, generator=torch.Generator(device=gpu).manual_seed(3))
    grad = torch.empty_like(V)
    value = ops.tv3d(V, spacing, mode, EPS, grad=grad)
    assert math.isfinite(float(value)) and float(value) > 0
    G = 2.0 * sum(1.0 / s for s in spacing)
    # slabs of four planes with the planes whose stencil the slab holds whole: the first planes, the
    # planes around 2^31 voxels, the last ones (every slab has the last rows and columns of y and z)
    mid = 2**31 // (shape[1] * shape[2])
    for a, b, lo, hi in ((0, 4, 0, 3), (mid - 2, mid + 2, mid - 1, mid + 1), (shape[0] - 4, shape[0], shape[0] - 3,
                                                                             shape[0])):
        _, g64 = composition(V[a:b], spacing, mode, torch.float64)
        _, g32 = composition(V[a:b], spacing, mode, torch.float32)
        sel = slice(lo - a, hi - a)
        gerr = float((grad[lo:hi].double() - g64[sel]).abs().max())
        gref = float((g32[sel] - g64[sel]).abs().max())
        print(f"planes {lo}..{hi - 1}: gradient err {gerr:.3g} fp32 composition {gref:.3g}")
        assert gerr <= max(2 * gref, 8 * 2.0 ** -24 * G), (a, b)
    # the value against per-slab float64 sums would cost minutes; its order of magnitude is the mean norm
    # of three uniform differences times the voxel count
    assert 0.3 * n < float(value) < 3.0 * n


# ------------------------------------------------------------------------------------------ VolumeAdam
BOUNDS = [(None, None), (0.0, None), (None, 0.25), (-0.1, 0.2)]


@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("bounds", BOUNDS, ids=lambda b: f"{b[0]}_{b[1]}")
@pytest.mark.parametrize("steps", [1, 10])
@pytest.mark.parametrize("n", [1, 63, 2**20 + 3])
def test_volume_adam_against_torch_adam_and_clamp(gpu, n, steps, bounds, maximize):
    lr = 0.02
    lower, upper = bounds
    gen = torch.Generator(device=gpu).manual_seed(n + steps)
    p0 = torch.randn(n, device=gpu, generator=gen)
    grads = [torch.randn(n, device=gpu, generator=gen) for _ in range(steps)]

    def torch_loop(dtype):
        p = p0.to(dtype).clone().requires_grad_(True)
        opt = torch.optim.Adam([p], lr=lr, maximize=maximize, foreach=False)
        for g in grads:
            p.grad = g.to(dtype)
            opt.step()
            if lower is not None or upper is not None:
                with torch.no_grad():
                    p.clamp_(min=lower, max=upper)
        st = opt.state[p]
        return p.detach().double(), st["exp_avg"].double(), st["exp_avg_sq"].double(), float(st["step"])

    p64, m64, v64, k64 = torch_loop(torch.float64)
    p32, m32, v32, _ = torch_loop(torch.float32)
    p = torch.nn.Parameter(p0.clone())
    opt = VolumeAdam([p], lr=lr, lower=lower, upper=upper, maximize=maximize)
    for g in grads:
        p.grad = g.clone()
        opt.step()
    st = opt.state[p]
    assert float(st["step"]) == k64 == steps
    # the parameter: twice torch's own float32 distance from float64, plus lr 2^-22.  The moments: the
    # same, with the floor their own format gives: two roundings per step, each at most half an ulp
    # (<= 2^-24 of the largest moment)
    for name, mine, f32, f64, floor in (
            ("param", p.detach().double(), p32, p64, lr * 2.0 ** -22),
            ("exp_avg", st["exp_avg"].double(), m32, m64, steps * 2.0 ** -23 * float(m64.abs().max())),
            ("exp_avg_sq", st["exp_avg_sq"].double(), v32, v64, steps * 2.0 ** -23 * float(v64.abs().max()))):
        err, ref = float((mine - f64).abs().max()), float((f32 - f64).abs().max())
        print(f"n={n} steps={steps} bounds={bounds} maximize={maximize} {name}: err {err:.3g} torch fp32 {ref:.3g}")
        assert err <= 2 * ref + floor, name
    # (the bounds as float32 holds them: -0.1 rounds to just below -0.1)
    if lower is not None:
        assert float(p.detach().min()) >= float(torch.tensor(lower, dtype=torch.float32))
    if upper is not None:
        assert float(p.detach().max()) <= float(torch.tensor(upper, dtype=torch.float32))


def test_volume_adam_unaligned_and_multidimensional_parameters(gpu):
    """A parameter that is a view at an odd offset (no 16-byte accesses) and a 3-D one take the same
    update."""
    base = torch.randn(4 * 5 * 7 + 1, device=gpu)
    g = torch.randn(4 * 5 * 7, device=gpu)
    outs = []
    for p in (torch.nn.Parameter(base[1:]), torch.nn.Parameter(base[1:].clone().reshape(4, 5, 7))):
        opt = VolumeAdam([p], lr=0.02, lower=0.0)
        for _ in range(3):
            p.grad = g.reshape(p.shape).clone()
            opt.step()
        outs.append(p.detach().flatten().clone())
    assert torch.equal(outs[0], outs[1])
    with pytest.raises(ValueError, match="float32"):
        VolumeAdam([torch.nn.Parameter(torch.zeros(3, device=gpu, dtype=torch.float64))], lr=0.1)
    with pytest.raises(ValueError, match="GPU"):
        VolumeAdam([torch.nn.Parameter(torch.zeros(3))], lr=0.1)


# -------------------------------------------------------------------------------------- Reconstruction
def _views(n, device):
    rot = torch.zeros(n, 3, device=device)
    rot[:, 0] = torch.arange(n, device=device) * (2 * math.pi / n)
    xyz = torch.tensor([[0.0, 150.0, 0.0]], device=device).repeat(n, 1)
    return rot, xyz


@pytest.mark.parametrize("pose", ["euler", "rigid"])
@pytest.mark.parametrize("renderer", ["siddon", "trilinear"])
def test_forward_is_the_render_of_a_drr_whose_density_requires_grad(gpu, renderer, pose):
    subject = synthetic_subject(24, kind="phantom", seed=1)
    values = phantom_volume(24, seed=2).to(gpu)
    kw = {"n_points": 64} if renderer == "trilinear" else {}
    drr = DRR(make_subject(values.cpu(), (1.0, 1.0, 1.0)), sdd=300.0, height=24, delx=2.4, renderer=renderer).to(gpu)
    drr.density.requires_grad_()
    recon = Reconstruction(DRR(subject, sdd=300.0, height=24, delx=2.4, renderer=renderer), init=values).to(gpu)
    rot, xyz = _views(2, gpu)
    if pose == "euler":
        args, pkw = (rot, xyz), dict(parameterization="euler_angles", convention="ZXY")
    else:
        args, pkw = (convert(rot, xyz, parameterization="euler_angles", convention="ZXY"),), {}
    theirs = drr(*args, **pkw, **kw)
    theirs.sum().backward()
    mine = recon(*args, **pkw, **kw)
    mine.sum().backward()
    assert mine.shape == theirs.shape and float(theirs.detach().abs().max()) > 0
    assert torch.equal(mine, theirs)
    assert torch.equal(recon.density.grad, drr.density.grad) and bool(recon.density.grad.any())
    # the rays' route (the tutorial's drr.render(density, source, target))
    with torch.no_grad():
        p = convert(rot, xyz, parameterization="euler_angles", convention="ZXY")
        source, target = recon.drr.detector(p, None)
        assert torch.allclose(recon.forward_rays(source, target, **kw).reshape(mine.shape), mine, rtol=1e-4, atol=1e-4)


def _rmse(a, b):
    return float((a.double() - b.double()).pow(2).mean().sqrt())


def _scene(gpu, renderer="siddon"):
    subject = synthetic_subject(32, kind="phantom", seed=0)
    truth = subject.density.data.squeeze().to(gpu, torch.float32)
    geo = dict(sdd=300.0, height=32, delx=2.4, renderer=renderer)
    kw = dict(parameterization="euler_angles", convention="ZXY")
    if renderer == "trilinear":
        kw["n_points"] = 96
    rot, xyz = _views(8, gpu)
    with torch.no_grad():
        measured = DRR(subject, **geo).to(gpu)(rot, xyz, **kw)
    blank = make_subject(torch.zeros(32, 32, 32), (1.0, 1.0, 1.0))
    return truth, geo, kw, rot, xyz, measured, blank


@pytest.fixture(scope="module")
def end_to_end(gpu):
    """8 views of the 32^3 phantom, all views every step, from zeros, Adam lr 0.02, 81 steps, isotropic TV
    (eps 1e-3) with weight 1e-3 on the sum, density >= 0: the yardstick loop -- the same iteration from
    torch ops only, what a user could build before -- and the fused route."""
    truth, geo, kw, rot, xyz, measured, blank = _scene(gpu)
    lr, steps, weight = 0.02, 81, 1e-3
    drr = DRR(blank, **geo).to(gpu)
    drr.density.requires_grad_()
    opt = torch.optim.Adam([drr.density], lr=lr)
    for it in range(steps):
        opt.zero_grad(set_to_none=True)
        data = torch.nn.functional.mse_loss(drr(rot, xyz, **kw), measured)
        (data + weight * total_variation_3d(drr.density, (1.0, 1.0, 1.0), "isotropic", EPS)).backward()
        opt.step()
        with torch.no_grad():
            drr.density.clamp_(min=0)
        if it == 2:
            early_y = drr.density.detach().clone()
    final_y, data_y = drr.density.detach(), float(data)
    recon = Reconstruction(DRR(blank, **geo), lower=0.0).to(gpu)
    tv = TotalVariation3d.for_drr(recon.drr, mode="isotropic", eps=EPS)
    assert tv.spacing == pytest.approx((1.0, 1.0, 1.0))
    optimizer = recon.make_optimizer(lr=lr)
    for it in range(steps):
        data, tv_value = recon.step(optimizer, measured, rot, xyz, regularizer=tv, weight=weight, **kw)
        assert data.device == tv_value.device == recon.density.device and data.dim() == tv_value.dim() == 0
        if it == 2:
            early_f = recon.density.detach().clone()
    final_f, data_f = recon.density.detach(), float(data)
    return dict(truth=truth, early_y=early_y, early_f=early_f, final_y=final_y, final_f=final_f, data_y=data_y,
                data_f=data_f)


def test_reconstruction_end_to_end_against_the_torch_loop(end_to_end):
    """The yardstick loop recovers the phantom (RMSE at most half the zero start's), and the fused route
    lands where it lands: within 2 % of its final RMSE and final data loss.  (Not voxel-wise at the end:
    Adam divides by the root of the second moment, so rounding-level differences in near-zero gradients
    move single voxels by whole steps, while the aggregate does not move.)"""
    r = end_to_end
    truth = r["truth"]
    rmse0, rmse_y, rmse_f = _rmse(torch.zeros_like(truth), truth), _rmse(r["final_y"], truth), _rmse(r["final_f"], truth)
    print(f"RMSE: start {rmse0:.6g} yardstick {rmse_y:.6g} fused {rmse_f:.6g}; data loss yardstick {r['data_y']:.6g} "
          f"fused {r['data_f']:.6g}; final max |diff| {float((r['final_f'] - r['final_y']).abs().max()):.3g}")
    assert rmse_y <= 0.5 * rmse0
    assert abs(rmse_f - rmse_y) <= 0.02 * rmse_y
    assert abs(r["data_f"] - r["data_y"]) <= 0.02 * r["data_y"]
    assert float(r["final_f"].min()) >= 0.0


def test_reconstruction_first_three_steps_agree_voxelwise(end_to_end):
    """After the first three steps the two volumes must agree voxel-wise to 1e-5 (three steps of at most
    lr each, differing by rounding).

    What makes this hold on the device is that VolumeAdam's arithmetic is bit for bit that of the
    yardstick's ``torch.optim.Adam`` (the multi-tensor flavour torch takes by default there): Adam's first
    steps have size lr whatever the gradient's size, and last-bit differences of the parameter after step 1
    come back through projection, back-projection and Adam's normalisation ~700x larger per step.  torch's
    own single-tensor flavour (which multiplies by the float reciprocal of sqrt(bias_correction2) where the
    multi-tensor one divides) is 3.2e-5 away from the yardstick after three steps, and so was VolumeAdam
    (6.7e-5 ... 7.8e-5) while it did the same."""
    diff = float((end_to_end["early_f"] - end_to_end["early_y"]).abs().max())
    print(f"after 3 steps max |fused - yardstick| = {diff:.3g}")
    assert diff <= 1e-5


def test_volume_gradient_of_the_scene_is_bitwise_reproducible(gpu):
    """What the three-step comparison above rests on: the two routes get the same volume gradient from the same
    volume.  The brick kernels accumulate it in fixed point (integer sums: any order), with a scale formed from a
    bound summed over the poses -- in whole numbers, so that this sum does not depend on the order in which the
    poses' workgroups arrive either (csrc/bricks.hip volgrad_prepare_kernel).  One brick: every ray's forward
    value is a single contribution."""
    truth, geo, kw, rot, xyz, measured, blank = _scene(gpu)
    recon = Reconstruction(DRR(blank, **geo), init=truth * 0.5).to(gpu)
    grads = []
    for _ in range(6):
        recon.density.grad = None
        torch.nn.functional.mse_loss(recon(rot, xyz, **kw), measured).backward()
        grads.append(recon.density.grad.clone())
    assert float(grads[0].abs().max()) > 0
    for g in grads[1:]:
        assert torch.equal(g, grads[0])


def test_reconstruction_with_the_trilinear_renderer_reduces_the_loss(gpu):
    truth, geo, kw, rot, xyz, measured, blank = _scene(gpu, renderer="trilinear")
    recon = Reconstruction(DRR(blank, **geo), lower=0.0).to(gpu)
    tv = TotalVariation3d.for_drr(recon.drr)
    optimizer = recon.make_optimizer(lr=0.02)
    losses = [float(recon.step(optimizer, measured, rot, xyz, regularizer=tv, weight=1e-3, **kw)[0]) for _ in range(20)]
    print("trilinear data loss:", losses[0], "->", losses[-1])
    assert losses[-1] < losses[0]
