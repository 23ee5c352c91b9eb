"""The FDK kernels on the device (include/diffdrr_fbp_hip.h) against the float64 torch composition of the same
definitions, evaluated from the same float32 inputs.

The rule for both kernels: the largest absolute difference from the float64 composition must be at most
max(2 x the float32 composition's own difference, floor), the floor being 8 * 2^-24 of the largest magnitude
the definition allows (given with each test).  Every comparison prints the kernel's error, the float32
composition's and the floor."""
import math

import pytest
import torch

import diffdrr_amd
from diffdrr_amd import Reconstruction, TotalVariation3d, analytic, ops
from fbp_cases import (BACKPROJECTION_CASES, EPS, GPU_ONLY_CASES, KW, backprojection_case, fdk_scene, quality)

pytestmark = pytest.mark.gpu


def held(tag, kernel, comp64, comp32, floor):
    """Assert the rule; -> error / allowance."""
    err = float((kernel.double() - comp64).abs().max())
    err32 = float((comp32.double() - comp64).abs().max())
    allowed = max(2 * err32, floor)
    print(f"{tag}: kernel error {err:.3e}, float32 composition error {err32:.3e}, floor {floor:.3e}, "
          f"error / allowance {err / allowed if allowed else 0.0:.3f}")
    assert err <= allowed, (tag, err, err32, floor)
    return err / allowed if allowed else 0.0


# ------------------------------------------------------------------------------------------------ filter
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (40, 56), (47, 63), (256, 256)])
def test_filter_against_float64(gpu, shape, B):
    H, W = shape
    g = torch.Generator().manual_seed(1000 * H + W + B)
    noise = torch.randn(B, H, W, generator=g).to(gpu)
    constant = torch.full((B, H, W), 0.731, device=gpu)
    geo = dict(u0=-0.5 * W + 3.25, du=1.0, v0=0.35 * H, dv=-0.7, sdd=1020.0)
    scale = 1.0 / 0.7
    worst = 0.0
    for axis in (0, 1):
        L = W if axis == 0 else H
        for window in ("ram-lak", "hann"):
            taps = analytic.ramp_taps(L, window).float().to(gpu)
            for kind, images in (("noise", noise), ("constant", constant)):
                for cw in (False, True):
                    out = ops.fbp_filter(images, axis, taps, scale, cosine_weight=cw, **geo,
                                         out=torch.full_like(images, float("nan")))
                    assert torch.isfinite(out).all()
                    comp64 = analytic.filter_composition(images.double(), axis, taps.double(), scale,
                                                         cosine_weight=cw, **geo)
                    comp32 = analytic.filter_composition(images, axis, taps, scale, cosine_weight=cw, **geo)
                    floor = 8 * EPS * scale * float(taps.double().abs().sum()) * float(images.abs().max())
                    worst = max(worst, held(f"filter {B}x{H}x{W} axis {axis} {window} {kind} cw={int(cw)}", out,
                                            comp64, comp32, floor))
                    assert out is not images and torch.equal(analytic.fbp_filter(images, axis, taps, scale,
                                                                                 cosine_weight=cw, **geo), out)
    print(f"filter {B}x{H}x{W}: worst error / allowance {worst:.3f}")


# ---------------------------------------------------------------------------------------- backprojection
def contributions(case, device):
    """-> (the smallest depth U of any (voxel, view) pair whose sample touches the image, the voxels no view
    reaches by a margin of 1e-3 pixels), from the float32 views in float64."""
    views = case["views"].double().to(device)
    shape = case["shape"]
    H, W = case["images"].shape[1:]
    idx = torch.stack(torch.meshgrid(*[torch.arange(d, dtype=torch.float64, device=device) for d in shape],
                                     indexing="ij"), -1)
    u_min, untouched = math.inf, torch.ones(shape, dtype=torch.bool, device=device)
    for m in views:
        a, b, U = (idx @ m[4 * r:4 * r + 3] + m[4 * r + 3] for r in range(3))
        ok = U > 0
        col, row = a / torch.where(ok, U, torch.ones_like(U)), b / torch.where(ok, U, torch.ones_like(U))
        touches = ok & (col > -1) & (col < W) & (row > -1) & (row < H)
        if bool(touches.any()):
            u_min = min(u_min, float(U[touches].min()))
        untouched &= ~(ok & (col > -1 - 1e-3) & (col < W + 1e-3) & (row > -1 - 1e-3) & (row < H + 1e-3))
    return u_min, untouched


@pytest.mark.parametrize("name", sorted(BACKPROJECTION_CASES) + sorted(GPU_ONLY_CASES))
def test_backprojection_against_float64(gpu, name):
    case = backprojection_case(name)
    images, views = case["images"].to(gpu), case["views"].to(gpu)
    shape, dw = case["shape"], case["distance_weight"]
    out = ops.fbp_backproject(images, views, distance_weight=dw, out=torch.full(shape, float("nan"), device=gpu))
    assert torch.isfinite(out).all()  # every voxel is written
    comp64 = analytic.backproject_composition(images.double(), views.double(), shape, dw)
    comp32 = analytic.backproject_composition(images, views, shape, dw)
    u_min, untouched = contributions(case, gpu)
    peak = images.double().abs().amax(dim=(1, 2))
    floor = 0.0 if u_min == math.inf else \
        8 * EPS * float((views[:, 12].double().abs() * peak).sum()) / (u_min ** 2 if dw else 1.0)
    held(f"backproject {name}", out, comp64, comp32, floor)
    assert bool((out[untouched] == 0).all())  # no view reaches them: exactly zero
    print(f"backproject {name}: {float(untouched.double().mean()):.2f} of the voxels out of every view")
    # accumulate: what was there plus the overwrite result, to 2 ulp
    prior = case["prior"].to(gpu)
    acc = ops.fbp_backproject(images, views, distance_weight=dw, out=prior.clone(), accumulate=True)
    want = prior + out
    ulp = torch.maximum(want.abs(), torch.full_like(want, 2.0 ** -126)) * 2.0 ** -23
    assert bool(((acc - want).abs() <= 2 * ulp).all())
    # the public entry takes the same route
    pub = diffdrr_amd.backproject(case["drr"], images[:, None], case["rot"], case["xyz"],
                                  view_weights=case["views"][:, 12], distance_weight=dw, **KW)
    assert torch.equal(pub, out)


def test_fdk_is_reproducible(gpu):
    drr, images, rot, xyz, _ = fdk_scene("anisotropic")
    images = images.float().to(gpu)
    first = diffdrr_amd.fdk(drr, images, rot, xyz, **KW)
    assert first.is_cuda and first.dtype == torch.float32
    assert torch.equal(diffdrr_amd.fdk(drr, images, rot, xyz, **KW), first)


def sampled_definition(images, view, idx, distance_weight):
    """The backprojection of ONE view at the voxels `idx` (n, 3), in the dtype of `images` (1, H, W)."""
    H, W = images.shape[1:]
    idx = idx.to(images.dtype)
    a, b, U = (((view[4 * r + 3] + view[4 * r] * idx[:, 0]) + view[4 * r + 1] * idx[:, 1]) + view[4 * r + 2] * idx[:, 2]
               for r in range(3))
    col, row = a / U, b / U
    c0, r0 = torch.floor(col), torch.floor(row)
    fc, fr = col - c0, row - r0
    c0, r0 = c0.long(), r0.long()

    def pixel(r, c):
        inside = (r >= 0) & (r < H) & (c >= 0) & (c < W)
        return torch.where(inside, images[0][r.clamp(0, H - 1), c.clamp(0, W - 1)], torch.zeros_like(fc))

    value = (pixel(r0, c0) * (1 - fc) + pixel(r0, c0 + 1) * fc) * (1 - fr) \
        + (pixel(r0 + 1, c0) * (1 - fc) + pixel(r0 + 1, c0 + 1) * fc) * fr
    return torch.where(U > 0, view[12] / (U * U) * value if distance_weight else view[12] * value,
                       torch.zeros_like(value))


def test_backprojection_above_2_31_voxels(gpu):
    shape = (2048, 1024, 1025)  # 2^31 + 2^21 voxels: the last ones lie past a 32-bit offset
    voxels = shape[0] * shape[1] * shape[2]
    free, _ = torch.cuda.mem_get_info(gpu)
    if free < 4 * voxels + (2 << 30):
        pytest.skip(f"needs {4 * voxels / 2**30:.1f} GiB of device memory, {free / 2**30:.1f} free")
    g = torch.Generator().manual_seed(31)
    images = torch.randn(1, 64, 64, generator=g).to(gpu)
    # x = 0.01 (i - 1024), y = 0.02 (j - 512), U = 100 + 0.01 k;  col = 32 + 150 x / U, row = 31 + 150 y / U
    view = torch.zeros(1, 16, dtype=torch.float64)
    depth = torch.tensor([0.0, 0.0, 0.01, 100.0], dtype=torch.float64)
    view[0, 0:4] = 150 * torch.tensor([0.01, 0.0, 0.0, -10.24], dtype=torch.float64) + 32 * depth
    view[0, 4:8] = 150 * torch.tensor([0.0, 0.02, 0.0, -10.24], dtype=torch.float64) + 31 * depth
    view[0, 8:12] = depth
    view[0, 12] = 1.7e4
    view = view.float().to(gpu)
    out = torch.empty(shape, dtype=torch.float32, device=gpu)
    out[-1, -1, -8:] = float("nan")
    ops.fbp_backproject(images, view, distance_weight=True, out=out)
    idx = torch.stack([torch.randint(0, d, (4096,), generator=g) for d in shape], -1)
    idx = torch.cat([idx, torch.tensor([[d - 1 for d in shape], [shape[0] - 1, shape[1] - 1, 0], [0, 0, 0]])]).to(gpu)
    assert int((idx[:, 0] * shape[1] + idx[:, 1]) .max()) * shape[2] > 2**31
    got = out[idx[:, 0], idx[:, 1], idx[:, 2]]
    comp64 = sampled_definition(images.double(), view[0].double(), idx, True)
    comp32 = sampled_definition(images, view[0], idx, True)
    assert float(comp64.abs().min()) > 0  # every sampled voxel is in view
    floor = 8 * EPS * float(view[0, 12]) * float(images.abs().max()) / 100.0 ** 2
    held("backproject 2048x1024x1025", got, comp64, comp32, floor)


# ------------------------------------------------------------------------------------------- end to end
def test_fdk_end_to_end_and_as_a_start(gpu):
    cpu_drr, _, rot, xyz, truth = fdk_scene("cube_32")
    drr = diffdrr_amd.DRR(cpu_drr.subject, sdd=1020.0, height=48, width=64, delx=1.0).to(gpu)
    rot, xyz = rot.to(gpu), xyz.to(gpu)
    with torch.no_grad():
        measured = drr(rot, xyz, **KW).contiguous()  # the package's own Siddon
    assert measured.shape == (60, 1, 48, 64) and measured.dtype == torch.float32
    volume = diffdrr_amd.fdk(drr, measured, rot, xyz, **KW)
    comp64 = diffdrr_amd.fdk(drr, measured.double(), rot, xyz, **KW)
    comp32 = analytic._backproject(  # the float32 composition of both steps
        *_composition_steps(drr, measured, rot, xyz), tuple(truth.shape), True)
    # floor: the backprojection's, of the filtered views, plus the filter's own floor carried through it
    geometry = analytic.view_geometry(drr, rot, xyz, **KW)
    orb = analytic.orbit_of(geometry)
    taps = analytic.ramp_taps(64)
    filtered = analytic.filter_composition(measured[:, 0].double(), 0, taps, 1.0, cosine_weight=False)
    peak = filtered.abs().amax(dim=(1, 2)).cpu()
    filter_floor = 8 * EPS * float(taps.abs().sum()) * measured.double().abs().amax(dim=(1, 2, 3)).cpu()
    weights = (orb.arc_weights * orb.radius * 1020.0).abs()
    corners = torch.tensor([[i, j, k, 1.0] for i in (0, 31) for j in (0, 31) for k in (0, 31)], dtype=torch.float64)
    u_min = float((geometry.matrices[:, 2] @ corners.T).min())
    floor = float((weights * (8 * EPS * peak + filter_floor)).sum()) / u_min ** 2
    held("fdk cube_32", volume, comp64, comp32, floor)
    rmse, scale = quality(volume, truth)
    rmse64, _ = quality(comp64, truth)
    print(f"fdk cube_32 on the device: rmse / rmse(0) = {rmse:.4f} (float64 composition {rmse64:.4f}), scale {scale:.3f}")
    assert rmse <= 1.05 * rmse64

    # as the start of an iterative reconstruction, against a start from zeros: the same five steps
    tv = TotalVariation3d.for_drr(drr)
    losses = {}
    for start in ("fdk", "zeros"):
        recon = Reconstruction.from_fdk(drr, measured, rot, xyz, **KW) if start == "fdk" else Reconstruction(drr)
        opt = recon.make_optimizer(lr=0.02)
        steps = [recon.step(opt, measured, rot, xyz, regularizer=tv, weight=1e-3, **KW)[0] for _ in range(5)]
        with torch.no_grad():
            after = torch.nn.functional.mse_loss(recon(rot, xyz, **KW), measured)
        losses[start] = (float(steps[0]), float(after))
    print(f"data loss at step 0 / after step 5: FDK start {losses['fdk']}, zeros {losses['zeros']}")
    assert losses["fdk"][0] < losses["zeros"][0]
    assert losses["fdk"][1] < losses["zeros"][1]


def _composition_steps(drr, measured, rot, xyz):
    """fdk's two steps with the float32 composition in place of the kernels: -> (filtered, geometry, weights)"""
    geometry = analytic.view_geometry(drr, rot, xyz, **KW)
    orb = analytic.orbit_of(geometry)
    assert orb.axis == 0
    filtered = analytic.filter_composition(
        measured[:, 0], 0, analytic.ramp_taps(64), 1.0 / float(geometry.col_step.norm()),
        u0=float(geometry.origin[0]), du=float(geometry.col_step[0]), v0=float(geometry.origin[1]),
        dv=float(geometry.row_step[1]), sdd=float(geometry.origin[2]), cosine_weight=True)
    # (strided on purpose: _backproject sends what is not contiguous float32 to the composition)
    filtered = filtered.transpose(1, 2).contiguous().transpose(1, 2)
    return filtered, geometry, orb.arc_weights * orb.radius * float(geometry.origin[2])
