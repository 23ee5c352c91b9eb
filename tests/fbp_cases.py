"""Scenes shared by tests/test_fbp.py (host) and tests/test_gpu_fbp.py (device): backprojection cases, an
evaluation of the backprojection's definition in float64 that does not use the package's matrices, and
cone-beam scenes with ground truth for ``fdk``."""
import copy
import math
from functools import lru_cache

import numpy as np
import torch

from diffdrr_amd import DRR, RigidTransform, analytic, convert
from diffdrr_amd.data import synthetic_subject

EPS = 2.0 ** -24  # half an fp32 ulp, relative
KW = dict(parameterization="euler_angles", convention="ZXY")

# name -> (volume shape, spacing, (H, W), pixel pitch, B, a view from inside the volume, reverse_x_axis + offsets,
#          distance_weight, accumulate)
BACKPROJECTION_CASES = {
    "one_voxel": ((1, 1, 1), 1.0, (40, 56), 1.0, 1, False, False, True, False),
    "tiny_accumulate": ((2, 3, 5), 1.0, (47, 63), 1.0, 3, False, True, False, True),
    "tiny_small_detector": ((2, 3, 5), 1.0, (8, 8), 0.5, 1, False, False, True, False),
    "anisotropic_33_views": ((33, 17, 40), (0.7, 1.3, 0.8), (40, 56), 1.0, 33, True, True, True, False),
    "anisotropic_mostly_outside": ((33, 17, 40), (0.7, 1.3, 0.8), (8, 8), 1.0, 3, False, True, True, True),
    "anisotropic_odd_detector": ((33, 17, 40), (0.7, 1.3, 0.8), (47, 63), 1.0, 3, True, False, False, False),
}
GPU_ONLY_CASES = {
    "several_blocks": ((257, 130, 67), 1.0, (40, 56), 4.0, 33, False, True, True, False),
}


@lru_cache(maxsize=None)
def backprojection_case(name):
    """-> dict: drr, rot, xyz (float32 poses), images (B, H, W) float32 noise, views (B, 16) float32 as the
    package builds them, prior (the volume's contents before an accumulating call), flags."""
    shape, spacing, (H, W), pitch, B, inside, reverse, dw, acc = {**BACKPROJECTION_CASES, **GPU_ONLY_CASES}[name]
    det = dict(reverse_x_axis=True, x0=3.0, y0=-2.0) if reverse else dict(reverse_x_axis=False)
    drr = DRR(synthetic_subject(shape, "phantom", spacing=spacing), sdd=1020.0, height=H, width=W, delx=pitch, **det)
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    rot = torch.zeros(B, 3)
    rot[:, 0] = torch.arange(B) * (2 * math.pi / B) + 0.3
    rot[:, 1:] = (torch.rand(B, 2, generator=g) - 0.5) * 0.2
    xyz = torch.tensor([0.0, 850.0, 0.0]) + (torch.rand(B, 3, generator=g) - 0.5) * 10
    if inside:
        xyz[B // 2] = torch.tensor([1.0, 2.0, -1.0])  # the source sits inside the volume: U <= 0 behind it
    images = torch.randn(B, H, W, generator=g)
    weights = 0.5 + torch.rand(B, generator=g, dtype=torch.float64)
    geometry = analytic.view_geometry(drr, rot, xyz, **KW)
    views = torch.zeros(B, 16, dtype=torch.float64)
    views[:, :12] = geometry.matrices.reshape(B, 12)
    views[:, 12] = weights
    prior = torch.randn(shape, generator=g)
    return dict(drr=drr, rot=rot, xyz=xyz, images=images, views=views.float(), prior=prior, shape=shape,
                distance_weight=dw, accumulate=acc)


def definition_float64(case):
    """The backprojection of `case` by its definition, in float64 numpy, from the world-space source and pixel
    positions the detector module gives for the poses (NOT from the package's matrices): the line source ->
    voxel is intersected with the detector plane and the hit solved for (row, col).
    -> (volume, bound): `bound` is, per voxel, what rounding the 12 matrix entries to fp32 can move the
    result by -- 2^-24 of the sum of the magnitudes of each homogeneous coordinate's four terms, carried
    through col = a / U to a shift in pixels, times the steepest a bilinear sample can be (2 max|image| per
    pixel) -- plus 16 * 2^-24 of sum |w| max|image| / U^2 for the arithmetic."""
    drr, shape = case["drr"], case["shape"]
    H, W = drr.detector.height, drr.detector.width
    det64 = copy.deepcopy(drr.detector).double()
    # (the poses are the float32 matrices the renderer is given; everything after them is float64)
    pose = RigidTransform(convert(case["rot"], case["xyz"], **KW).matrix.double())
    source, target = det64(pose, None)
    source, target = source[:, 0].numpy(), target.numpy()
    A = drr._affine.reshape(-1, 4, 4)[0].double().numpy()
    idx = np.stack(np.meshgrid(*[np.arange(d, dtype=np.float64) for d in shape], indexing="ij"), -1).reshape(-1, 3)
    absidx = np.concatenate([idx, np.ones((len(idx), 1))], 1)
    world = idx @ A[:3, :3].T + A[:3, 3]
    images = case["images"].double().numpy()
    w = case["views"][:, 12].double().numpy()
    out, bound = np.zeros(len(idx)), np.zeros(len(idx))
    for b in range(len(w)):
        p00, ec, er = target[b, 0], target[b, 1] - target[b, 0], target[b, W] - target[b, 0]
        n = np.cross(ec, er)
        n /= np.linalg.norm(n)
        if n @ (p00 - source[b]) < 0:
            n = -n
        D = n @ (p00 - source[b])
        d = world - source[b]
        U = d @ n
        ok = U > 0
        Us = np.where(ok, U, 1.0)
        hit = source[b] + (D / Us)[:, None] * d - p00
        # (col, row) with hit = col ec + row er: the float32 pose is orthonormal to 1e-7 only, so ec.er is not 0
        gram = np.array([[ec @ ec, ec @ er], [ec @ er, er @ er]])
        col, row = np.linalg.solve(gram, np.stack([hit @ ec, hit @ er]))
        c0, r0 = np.floor(col), np.floor(row)
        fc, fr = col - c0, row - r0

        def pixel(r, c):
            inside = (r >= 0) & (r < H) & (c >= 0) & (c < W) & ok
            return np.where(inside, images[b][np.clip(r, 0, H - 1).astype(int), np.clip(c, 0, W - 1).astype(int)], 0.0)

        value = (pixel(r0, c0) * (1 - fc) + pixel(r0, c0 + 1) * fc) * (1 - fr) \
            + (pixel(r0 + 1, c0) * (1 - fc) + pixel(r0 + 1, c0 + 1) * fc) * fr
        weight = w[b] / (Us * Us) if case["distance_weight"] else np.full_like(Us, w[b])
        out += np.where(ok, weight * value, 0.0)
        # the same map as homogeneous rows: col U = ((s - p00).ec U + D (x - s).ec) / |ec|^2, x = A (i, j, k, 1)
        lin = np.concatenate([A[:3, :3], (A[:3, 3] - source[b])[:, None]], 1)  # (i, j, k, 1) -> x - s
        u_row = n @ lin
        sizes = []
        for e in (ec, er):
            h_row = (((source[b] - p00) @ e) * u_row + D * (e @ lin)) / (e @ e)
            sizes.append(absidx @ np.abs(h_row))
        size_u = absidx @ np.abs(u_row)
        shift = EPS * ((sizes[0] + np.abs(col) * size_u) + (sizes[1] + np.abs(row) * size_u)) / Us
        reach = ok & (col > -1.5) & (col < W + 0.5) & (row > -1.5) & (row < H + 0.5)
        peak = np.abs(images[b]).max()
        bound += np.where(reach, np.abs(weight) * peak * (2.0 * shift + 16 * EPS), 0.0)
    return out.reshape(shape), bound.reshape(shape)


# ------------------------------------------------------------------------------------------------ fdk scenes
# name -> (volume shape, spacing, (H, W), views, the Euler angle swept, detector keywords)
FDK_SCENES = {
    "cube_32": ((32, 32, 32), 1.0, (48, 64), 60, 0, {}),
    "row_tangent_orbit": ((32, 32, 32), 1.0, (64, 48), 60, 1, {}),
    "anisotropic": ((33, 17, 40), (0.7, 1.3, 0.8), (40, 56), 48, 0, dict(reverse_x_axis=True, x0=3.0, y0=-2.0)),
}


def orbit(n, sweep=0, start=0.0, stop=2 * math.pi):
    rot = torch.zeros(n, 3)
    rot[:, sweep] = start + torch.arange(n) * ((stop - start) / n)
    return rot, torch.tensor([[0.0, 850.0, 0.0]]).repeat(n, 1)


@lru_cache(maxsize=None)
def fdk_scene(name):
    """-> (drr, images (B, 1, H, W) float64 from the float64 oracle, rot, xyz, the true volume float64)"""
    import oracle

    shape, spacing, (H, W), n, sweep, det = FDK_SCENES[name]
    drr = DRR(synthetic_subject(shape, "phantom", spacing=spacing), sdd=1020.0, height=H, width=W, delx=1.0, **det)
    rot, xyz = orbit(n, sweep)
    with torch.no_grad():
        source, target = drr.detector(convert(rot, xyz, **KW), None)
        length = (target - source).norm(dim=-1)
        s, t = drr.affine_inverse(source), drr.affine_inverse(target)
    f64 = lambda x: x.double().numpy()  # noqa: E731
    img = oracle.siddon(f64(drr.density), f64(s), f64(t), f64(length))["out"]
    return drr, torch.from_numpy(np.asarray(img, dtype=np.float64)).reshape(n, 1, H, W), rot, xyz, drr.density.double()


def quality(volume, truth):
    """-> (rmse(volume, truth) / rmse(0, truth), the least-squares scale <volume, truth> / <truth, truth>)"""
    volume, truth = volume.double().cpu(), truth.double().cpu()
    return (float((volume - truth).pow(2).mean().sqrt() / truth.pow(2).mean().sqrt()),
            float((volume * truth).sum() / (truth * truth).sum()))
