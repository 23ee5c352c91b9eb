"""Analytic (filtered-backprojection) reconstruction from cone-beam views: the start an iterative
``Reconstruction`` refines.

``fdk`` is Feldkamp-Davis-Kress for a circular orbit of the C-arm ``drr`` describes: the projections
are cosine weighted and ramp filtered along the detector axis tangent to the orbit (``fbp_filter``),
then backprojected voxel by voxel with the 1 / U^2 distance weight (``backproject``).  Both passes are
gfx950 kernels (``include/diffdrr_fbp_hip.h``) for float32 contiguous tensors on the device; everything
else (CPU, float64) takes a torch composition of the same definitions -- the definition the kernels are
held to.

The geometry is read from what the renderer casts -- ``reorient.compose(pose)``, the calibrated pixel
grid, the volume's affine -- so projector and backprojector cannot disagree about ``reverse_x_axis``,
principal-point offsets, pixel pitches or the volume's orientation.

    volume = fdk(drr, measured, rot, xyz, parameterization="euler_angles", convention="ZXY")
    recon = Reconstruction.from_fdk(drr, measured, rot, xyz, parameterization="euler_angles", convention="ZXY")
"""
from __future__ import annotations

import math
from typing import NamedTuple

import torch

from . import ops
from .pose import RigidTransform, convert

_WINDOWS = ("ram-lak", "hann")
_MAX_TILT_DEGREES = 8.0


def ramp_taps(length: int, window: str = "ram-lak") -> torch.Tensor:
    """The band-limited ramp filter for unit pixel pitch as ``2 length - 1`` float64 taps, lag 0 at index
    ``length - 1``: ``h[0] = 1/4``, ``h[n] = 0`` for even ``n != 0``, ``h[n] = -1 / (pi n)^2`` for odd ``n``
    (Ram-Lak).  ``window="hann"``: that sequence convolved with ``[1/4, 1/2, 1/4]`` -- exactly the ramp's
    spectrum times ``1/2 + 1/2 cos(pi f / f_Nyquist)``."""
    length = int(length)
    if length < 1:
        raise ValueError(f"ramp_taps: length must be >= 1, not {length}")
    if window not in _WINDOWS:
        raise ValueError(f"ramp_taps: window must be one of {_WINDOWS}, not {window!r}")

    def ram_lak(n):
        n = n.abs()
        odd = -1.0 / (math.pi * n.clamp_min(1)) ** 2
        return torch.where(n == 0, torch.full_like(odd, 0.25), torch.where(n % 2 == 1, odd, torch.zeros_like(odd)))

    n = torch.arange(-(length - 1), length, dtype=torch.float64)
    if window == "ram-lak":
        return ram_lak(n)
    return 0.25 * ram_lak(n - 1) + 0.5 * ram_lak(n) + 0.25 * ram_lak(n + 1)


def _fused(t) -> bool:
    """The kernels' domain (the dispatch rule of ``TotalVariation3d``)."""
    return ops.on_device(t) and t.dtype == torch.float32 and t.is_contiguous()


# ------------------------------------------------------------------------------------------ filter
def filter_composition(images, axis, taps, scale=1.0, *, u0=0.0, du=1.0, v0=0.0, dv=1.0, sdd=1.0,
                       cosine_weight=False):
    """``ddrr_fbp_filter`` as a torch composition, in the dtype of ``images`` (B, H, W):
    ``out[b, ., n] = scale sum_k taps[(n - k) + L - 1] images[b, ., k] cw[., k]`` along the columns
    (``axis`` 0) or the rows (``axis`` 1), ``cw(r, c) = sdd / sqrt(sdd^2 + (u0 + c du)^2 + (v0 + r dv)^2)``."""
    B, H, W = images.shape
    L = W if axis == 0 else H
    kw = dict(dtype=images.dtype, device=images.device)
    x = images
    if cosine_weight:
        u = u0 + torch.arange(W, **kw) * du
        v = v0 + torch.arange(H, **kw) * dv
        x = images * (sdd / torch.sqrt(sdd * sdd + u[None, :] ** 2 + v[:, None] ** 2))
    idx = torch.arange(L, device=images.device)
    T = taps.to(**kw)[(idx[:, None] - idx[None, :]) + (L - 1)]  # T[n, k] = the tap of lag n - k
    return scale * (x @ T.T if axis == 0 else T @ x)


def fbp_filter(images, axis, taps, scale=1.0, *, u0=0.0, du=1.0, v0=0.0, dv=1.0, sdd=1.0, cosine_weight=False):
    """Cosine weighting and 1-D convolution of (B, H, W) images along one detector axis: the kernel for
    float32 contiguous device tensors, :func:`filter_composition` otherwise."""
    if images.dim() != 3:
        raise ValueError(f"fbp_filter: (B, H, W) images expected, got {tuple(images.shape)}")
    if axis not in (0, 1):
        raise ValueError(f"fbp_filter: axis must be 0 or 1, not {axis!r}")
    L = images.shape[2] if axis == 0 else images.shape[1]
    if tuple(taps.shape) != (2 * L - 1,):
        raise ValueError(f"fbp_filter: {2 * L - 1} taps expected for a filtered axis of {L}, got {tuple(taps.shape)}")
    geometry = dict(u0=float(u0), du=float(du), v0=float(v0), dv=float(dv), sdd=float(sdd),
                    cosine_weight=bool(cosine_weight))
    if _fused(images):
        return ops.fbp_filter(images, axis, taps.to(device=images.device, dtype=torch.float32).contiguous(),
                              float(scale), **geometry)
    return filter_composition(images, axis, taps, float(scale), **geometry)


# ---------------------------------------------------------------------------------- backprojection
def backproject_composition(images, views, volume_shape, distance_weight=False):
    """``ddrr_fbp_backproject`` as a torch composition, in the dtype of ``images`` (B, H, W): per view
    ``(a, b, U) = M (i, j, k, 1)``, ``col, row = a / U, b / U``, the bilinear sample of the four neighbours
    of ``(floor(row), floor(col))`` with zeros outside the image, times ``w`` (``/ U^2`` with
    ``distance_weight``), summed over the views in ascending order.  ``views``: (B, 16), the row-major 3 x 4
    ``M`` and ``w`` per view.  -> (Dx, Dy, Dz)"""
    B, H, W = images.shape
    Dx, Dy, Dz = (int(d) for d in volume_shape)
    kw = dict(dtype=images.dtype, device=images.device)
    volume = torch.zeros(Dx, Dy, Dz, **kw)
    if B == 0 or H == 0 or W == 0 or volume.numel() == 0:
        return volume
    views = views.to(**kw)
    jj, kk = torch.arange(Dy, **kw), torch.arange(Dz, **kw)
    planes = max(1, 2**22 // (Dy * Dz))  # (the temporaries are a few dozen times this many voxels)
    for x0 in range(0, Dx, planes):
        ii = torch.arange(x0, min(x0 + planes, Dx), **kw)
        acc = volume[x0:x0 + planes]
        for b in range(B):
            m, flat = views[b], images[b].reshape(-1)

            def component(r):
                return ((m[4 * r + 3] + m[4 * r] * ii)[:, None, None] + (m[4 * r + 1] * jj)[None, :, None]) \
                    + (m[4 * r + 2] * kk)[None, None, :]

            U = component(2)
            valid = (U > 0) & torch.isfinite(U)
            Us = torch.where(valid, U, torch.ones_like(U))
            col, row = component(0) / Us, component(1) / Us
            valid &= torch.isfinite(col) & torch.isfinite(row)
            c0 = torch.floor(col).clamp(-2, W).nan_to_num(-2.0)
            r0 = torch.floor(row).clamp(-2, H).nan_to_num(-2.0)
            fc, fr = col - c0, row - r0
            c0, r0 = c0.long(), r0.long()

            def pixel(r, c):
                inside = (r >= 0) & (r < H) & (c >= 0) & (c < W)
                return torch.where(inside, flat[r.clamp(0, H - 1) * W + c.clamp(0, W - 1)], torch.zeros_like(fc))

            top = pixel(r0, c0) * (1 - fc) + pixel(r0, c0 + 1) * fc
            bottom = pixel(r0 + 1, c0) * (1 - fc) + pixel(r0 + 1, c0 + 1) * fc
            value = top * (1 - fr) + bottom * fr
            weight = m[12] / (Us * Us) if distance_weight else m[12]
            # (a voxel whose four neighbours are all outside gets an exact zero, whatever fc and fr are)
            valid &= (c0 >= -1) & (c0 < W) & (r0 >= -1) & (r0 < H)
            acc += torch.where(valid, weight * value, torch.zeros_like(value))
    return volume


class Geometry(NamedTuple):
    """What ``drr`` and a batch of poses say about the views, in float64 on the host."""
    matrices: torch.Tensor   # (B, 3, 4): voxel index (i, j, k, 1) -> (col U, row U, U), U the depth in world units
    sources: torch.Tensor    # (B, 3) world
    e_col: torch.Tensor      # (B, 3) world unit vector of increasing column index
    e_row: torch.Tensor      # (B, 3) ... of increasing row index
    e_w: torch.Tensor        # (B, 3) the optical axis, source -> detector
    origin: torch.Tensor     # (3,) camera-frame position of pixel (0, 0), on the plane z = sdd
    col_step: torch.Tensor   # (3,) camera-frame step to the next column
    row_step: torch.Tensor   # (3,) ... to the next row
    height: int
    width: int


def _pose_of(pose_args, pose_kwargs):
    kwargs = dict(pose_kwargs)
    parameterization = kwargs.pop("parameterization", None)
    convention = kwargs.pop("convention", None)
    degrees = kwargs.pop("degrees", False)
    if kwargs:
        raise TypeError(f"unexpected keyword arguments {sorted(kwargs)} (a pose is a RigidTransform, or rot, xyz "
                        "with parameterization=, convention=, degrees=)")
    if parameterization is None:
        if len(pose_args) != 1 or not isinstance(pose_args[0], RigidTransform):
            raise ValueError("a pose is a RigidTransform, or rot, xyz with parameterization= (and convention=)")
        return pose_args[0]
    return convert(*pose_args, parameterization=parameterization, convention=convention, degrees=degrees)


def view_geometry(drr, *pose_args, **pose_kwargs) -> Geometry:
    """The views ``drr(*pose_args, **pose_kwargs)`` renders, from what the renderer casts: the world pose
    ``reorient.compose(pose)``, the calibrated pixel grid ``drr._calibrated_points()`` -- its first point,
    that point's column neighbour and its row neighbour give origin and steps on the plane z = sdd -- and
    the volume's affine.  Built in float64 (one host synchronisation)."""
    det = drr.detector
    if det.n_subsample is not None or drr.patch_size is not None:
        raise ValueError("analytic reconstruction takes whole detector grids: a DRR with p_subsample or patch_size "
                         "renders only part of one")
    H, W = int(det.height), int(det.width)
    pose = _pose_of(pose_args, pose_kwargs)
    f64 = lambda t: t.detach().to(device="cpu", dtype=torch.float64)  # noqa: E731
    world = f64(pose.matrix) @ f64(det._reorient)  # reorient.compose(pose): camera -> world
    P = f64(drr._calibrated_points())
    cal = f64(det._calibration)
    origin = P[0]
    col_step = P[1] - P[0] if W > 1 else torch.stack([cal[0, 0] * (-1.0 if det.reverse_x_axis else 1.0),
                                                      cal[0, 0] * 0, cal[0, 0] * 0])
    row_step = P[W] - P[0] if H > 1 else torch.stack([cal[1, 1] * 0, -cal[1, 1], cal[1, 1] * 0])
    sdd = float(origin[2])
    affine = f64(drr._affine).reshape(-1, 4, 4)[0]
    camera = (torch.linalg.inv(world) @ affine)[:, :3, :]  # voxel index -> camera frame, (B, 3, 4)
    G = torch.linalg.inv(torch.stack([col_step[:2], row_step[:2]], dim=1))  # plane offset -> (col, row)
    K = torch.zeros(3, 3, dtype=torch.float64)
    K[:2, :2] = G * sdd
    K[:2, 2] = -(G @ origin[:2])
    K[2, 2] = 1.0
    R = world[:, :3, :3]
    unit = lambda v: v / v.norm()  # noqa: E731
    return Geometry(K @ camera, world[:, :3, 3].clone(), R @ unit(col_step), R @ unit(row_step), R[:, :, 2].clone(),
                    origin, col_step, row_step, H, W)


def _volume_shape(drr):
    """(Dx, Dy, Dz) of ``drr``'s volume grid (``drr.density`` is squeezed: a dimension of one voxel is not in it)"""
    return tuple(int(d) for d in drr.subject.density.data.shape[-3:])


def _as_stack(images, H, W):
    """(B, 1, H, W), (B, 1, H W) or (B, H, W) -> (B, H, W)"""
    shape = tuple(images.shape) if torch.is_tensor(images) else None
    if shape is not None and len(shape) == 4 and shape[1:] == (1, H, W):
        return images[:, 0]
    if shape is not None and len(shape) == 3 and shape[1:] == (1, H * W):
        return images.reshape(shape[0], H, W)
    if shape is not None and len(shape) == 3 and shape[1:] == (H, W):
        return images
    raise ValueError(f"images must be (B, 1, {H}, {W}), (B, 1, {H * W}) or (B, {H}, {W}), got {shape}")


def _backproject(images, geometry, weights, shape, distance_weight, out=None, accumulate=False):
    B = images.shape[0]
    if geometry.matrices.shape[0] != B:
        raise ValueError(f"{B} images for {geometry.matrices.shape[0]} poses")
    views = torch.zeros(B, 16, dtype=torch.float64)
    views[:, :12] = geometry.matrices.reshape(B, 12)
    views[:, 12] = weights
    if out is not None and (tuple(out.shape) != tuple(shape) or out.device != images.device):
        raise ValueError(f"out must be a {tuple(shape)} volume on {images.device}, got {tuple(out.shape)} on {out.device}")
    if accumulate and out is None:
        raise ValueError("accumulate needs an out tensor")
    if _fused(images) and (out is None or _fused(out)):
        views = views.to(device=images.device, dtype=torch.float32).contiguous()
        return ops.fbp_backproject(images, views, shape, distance_weight=distance_weight, out=out,
                                   accumulate=accumulate)
    volume = backproject_composition(images, views.to(images.device), shape, distance_weight)
    if out is None:
        return volume
    with torch.no_grad():
        return out.add_(volume.to(out.dtype)) if accumulate else out.copy_(volume)


def _view_weights(view_weights, B):
    if view_weights is None:
        return torch.ones(B, dtype=torch.float64)
    w = torch.as_tensor(view_weights).detach().to(device="cpu", dtype=torch.float64).reshape(-1)
    if w.numel() != B:
        raise ValueError(f"view_weights: {B} weights expected, got {w.numel()}")
    return w


@torch.no_grad()
def backproject(drr, images, *pose_args, view_weights=None, distance_weight=False, out=None, accumulate=False,
                **pose_kwargs):
    """Voxel-driven backprojection of ``images`` -- (B, 1, H, W), (B, 1, H W) or (B, H, W), as ``drr``
    renders the poses -- into ``drr``'s volume grid: every voxel gets the sum over the views of
    ``view_weights[b]`` (default 1) times the bilinear sample of view ``b`` where the voxel projects,
    divided by its squared depth along the optical axis (world units) with ``distance_weight``.  The pose
    arguments are those of ``DRR.forward``.  ``out``: a volume to write, or with ``accumulate`` to add to.
    -> (Dx, Dy, Dz)"""
    geometry = view_geometry(drr, *pose_args, **pose_kwargs)
    stack = _as_stack(images, geometry.height, geometry.width)
    return _backproject(stack, geometry, _view_weights(view_weights, stack.shape[0]), _volume_shape(drr),
                        bool(distance_weight), out, bool(accumulate))


class Orbit(NamedTuple):
    """What :func:`fdk` reads off the source positions and camera axes."""
    normal: torch.Tensor    # (3,) unit normal of the orbit plane
    axis: int               # the filtered detector axis: 0 along columns, 1 along rows
    tilt: float             # degrees the filtered axis leaves the orbit plane by (largest over the views)
    radius: torch.Tensor    # (B,) R_b = e_w . (iso - s_b)
    angles: torch.Tensor    # (B,) beta_b
    arc_weights: torch.Tensor  # (B,) delta beta_b / 2
    largest_gap: float      # radians


def orbit_of(geometry: Geometry, isocenter=None) -> Orbit:
    s = geometry.sources
    B = s.shape[0]
    if B < 3:
        raise ValueError(f"fdk needs at least 3 views to find the orbit's plane, got {B}")
    iso = torch.zeros(3, dtype=torch.float64) if isocenter is None else \
        torch.as_tensor(isocenter).detach().to(device="cpu", dtype=torch.float64).reshape(3)
    normal = torch.linalg.svd(s - s.mean(0)).Vh[-1]
    out_of_plane = [(e @ normal).abs() for e in (geometry.e_col, geometry.e_row)]
    axis = 0 if float(out_of_plane[0].mean()) <= float(out_of_plane[1].mean()) else 1
    tilt = math.degrees(math.asin(min(1.0, float(out_of_plane[axis].max()))))
    d = s - iso
    d = d - (d @ normal)[:, None] * normal
    e1 = d[0] / d[0].norm()
    e2 = torch.linalg.cross(normal, e1)
    angles = torch.atan2(d @ e2, d @ e1)
    order = torch.argsort(angles)
    ordered = angles[order]
    gaps = torch.cat([ordered[1:] - ordered[:-1], (ordered[0] + 2 * math.pi - ordered[-1]).reshape(1)])  # to the next
    arc = torch.empty(B, dtype=torch.float64)
    arc[order] = 0.25 * (gaps + torch.roll(gaps, 1))  # half of (half the sum of the two neighbouring gaps)
    radius = (geometry.e_w * (iso - s)).sum(-1)
    return Orbit(normal, axis, tilt, radius, angles, arc, float(gaps.max()))


@torch.no_grad()
def fdk(drr, images, *pose_args, window="ram-lak", view_weights=None, isocenter=None, **pose_kwargs):
    """Feldkamp-Davis-Kress reconstruction of ``drr``'s volume grid from the views ``images`` of a full
    circular orbit (``images`` and the pose arguments as for :func:`backproject`):

        volume = sum_b  w_b R_b D / U^2 * bilinear(p~_b, row, col),     p~ = (ramp * (p cw)) / pitch

    with ``D`` the source-detector distance, ``R_b`` the source's distance from the isocentre along the
    optical axis, ``U`` the voxel's depth, ``cw`` the cosine weight, the ramp (``window``: "ram-lak", "hann"
    or a tensor of ``2 L - 1`` taps for unit pitch) applied along the detector axis that lies in the
    orbit's plane, and ``w_b`` half the angle view ``b`` stands for on the circle.  DRRs are line integrals
    in world length, so a density comes back as that density.

    ``view_weights`` replaces ``w_b`` (needed for anything but a full orbit: an angular gap of pi or more
    raises, short-scan weights are the caller's).  ``isocenter``: the orbit's centre in world coordinates
    (default the origin, where a centred affine puts the volume's centre).  -> (Dx, Dy, Dz)"""
    geometry = view_geometry(drr, *pose_args, **pose_kwargs)
    stack = _as_stack(images, geometry.height, geometry.width)
    if stack.shape[0] != geometry.sources.shape[0]:
        raise ValueError(f"{stack.shape[0]} images for {geometry.sources.shape[0]} poses")
    orbit = orbit_of(geometry, isocenter)
    if orbit.tilt > _MAX_TILT_DEGREES:
        raise ValueError(f"the detector axis nearest the orbit's plane is {orbit.tilt:.1f} degrees out of it "
                         f"(more than {_MAX_TILT_DEGREES:g}): the ramp filter has no axis to run along")
    if view_weights is None:
        if orbit.largest_gap >= math.pi:
            raise ValueError(f"the views leave an angular gap of {math.degrees(orbit.largest_gap):.0f} degrees: not a "
                             "full orbit (pass view_weights for a short scan)")
        weights = orbit.arc_weights
    else:
        weights = _view_weights(view_weights, stack.shape[0])
    step = geometry.col_step if orbit.axis == 0 else geometry.row_step
    if abs(float(geometry.col_step[1])) > 1e-9 * float(geometry.col_step.norm()) \
            or abs(float(geometry.row_step[0])) > 1e-9 * float(geometry.row_step.norm()):
        raise ValueError("the pixel grid's columns and rows do not run along the camera's x and y axes")
    L = geometry.width if orbit.axis == 0 else geometry.height
    taps = window if torch.is_tensor(window) else ramp_taps(L, window)
    sdd = float(geometry.origin[2])
    filtered = fbp_filter(stack, orbit.axis, taps, 1.0 / float(step.norm()), u0=float(geometry.origin[0]),
                          du=float(geometry.col_step[0]), v0=float(geometry.origin[1]),
                          dv=float(geometry.row_step[1]), sdd=sdd, cosine_weight=True)
    return _backproject(filtered, geometry, weights * orbit.radius * sdd, _volume_shape(drr), True)
