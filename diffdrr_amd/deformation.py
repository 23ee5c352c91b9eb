"""Free-form deformation of the volume in front of the renderers: ``W = V o (id + u)`` with ``u`` the
trilinear interpolation of a control lattice, differentiable in the volume and in the lattice
(``csrc/warp.hip``, ``include/diffdrr_warp_hip.h``: one fused forward kernel, an atomic-free lattice gradient,
an atomic scatter for the volume gradient).  The torch composition it replaces -- ``F.interpolate`` of the
lattice, a normalised grid, ``grid_sample`` -- materialises a (Dx, Dy, Dz, 3) grid and keeps it for backward.

``basis="bspline"`` makes ``u`` the tensor-product cubic B-spline of the same lattice (Rueckert et al.: a C^2
field from 4 x 4 x 4 coefficients per voxel, border coefficients edge-replicated; ``csrc/bspline.hip``,
``include/diffdrr_bspline_hip.h``).  That spline approximates, it does not interpolate: the field at a node is
not that node's coefficient.  ``basis="linear"``, the default, is the trilinear field.

:func:`warp_reference` is the definition in pure torch, for any dtype: the float64 yardstick of the tests.

Whether the map ``x -> x + u(x)`` is still a deformation is read off its Jacobian determinant
(``csrc/jacobian.hip``, ``include/diffdrr_jacobian_hip.h``): :func:`jacobian_determinant` (the map, differentiable),
:func:`jacobian_statistics` (folded voxels, extremes) and :func:`volume_penalty` (the fused regulariser on
``ln det``), with :func:`field_jacobian`, :func:`jacobian_reference` and :func:`volume_penalty_reference` as their
definitions in torch.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import torch
from torch import nn

from . import ops

_PADDING = ("zeros", "border")
_BASES = ("linear", "bspline")


def _check_basis(basis):
    if basis not in _BASES:
        raise ValueError(f"basis must be 'linear' or 'bspline', not {basis!r}")


# ------------------------------------------------------------------------------------------------ definition
def _span(D, box, axis):
    """The voxels of an axis a definition is evaluated at: all of them, or ``box[axis] = (start, stop)``."""
    if box is None:
        return 0, int(D)
    start, stop = (int(v) for v in box[axis])
    if not 0 <= start < stop <= int(D):
        raise ValueError(f"box must be three (start, stop) ranges inside the volume, got {tuple(box[axis])} on axis "
                         f"{axis} of {int(D)} voxels")
    return start, stop


def _cells(D: int, G: int, device, dtype, span=None):
    """Cell and fraction of every voxel of an axis (include/diffdrr_warp_hip.h): integers, then one division."""
    num = torch.arange(*(span or (0, D)), device=device) * (G - 1)
    c = torch.div(num, D - 1, rounding_mode="floor").clamp(max=G - 2)
    return c, (num - c * (D - 1)).to(dtype) / (D - 1)


def bspline_weights(t: torch.Tensor):
    """The four cubic B-spline weights of a fraction ``t`` in [0, 1] (include/diffdrr_bspline_hip.h)."""
    return ((1 - t) ** 3 / 6, (3 * t ** 3 - 6 * t ** 2 + 4) / 6, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6, t ** 3 / 6)


def bspline_derivative_weights(t: torch.Tensor):
    """The derivatives in ``t`` of the four :func:`bspline_weights` (include/diffdrr_jacobian_hip.h)."""
    return (-(1 - t) ** 2 / 2, (3 * t ** 2 - 4 * t) / 2, (-3 * t ** 2 + 2 * t + 1) / 2, t ** 2 / 2)


def dense_field(displacement: torch.Tensor, shape, basis: str = "linear", box=None) -> torch.Tensor:
    """u (3, Dx, Dy, Dz): the lattice ``displacement`` (3, Gx, Gy, Gz) evaluated at every voxel, node i of axis a
    at voxel coordinate i (D_a - 1) / (G_a - 1): interpolated trilinearly (``basis="linear"``), or the cubic
    B-spline with these coefficients (``basis="bspline"``: per axis the four weights of the voxel's fraction on
    the coefficients c - 1 .. c + 2 of its cell c, indices clamped to the lattice; an approximating spline --
    the field at a node is not the node's coefficient).  ``box``, three (start, stop) voxel ranges: the field on
    those voxels only, (3, x1 - x0, y1 - y0, z1 - z0) -- what the whole field holds there."""
    _check_basis(basis)
    u = displacement
    for axis, D in enumerate(shape):
        G = u.shape[axis + 1]
        c, t = _cells(int(D), G, u.device, u.dtype, _span(D, box, axis))
        t = t.reshape([-1 if d == axis + 1 else 1 for d in range(4)])
        if basis == "linear":
            u = (1 - t) * u.index_select(axis + 1, c) + t * u.index_select(axis + 1, c + 1)
        else:
            u = sum(w * u.index_select(axis + 1, (c - 1 + k).clamp(0, G - 1)) for k, w in enumerate(bspline_weights(t)))
    return u


def field_jacobian(displacement: torch.Tensor, shape, basis: str = "linear", box=None) -> torch.Tensor:
    """du_a / dx_b, (3, 3, Dx, Dy, Dz), of :func:`dense_field` at every voxel: the analytic derivative of the
    basis in the cell the voxel is assigned to (include/diffdrr_jacobian_hip.h) -- axis b takes derivative weights
    times (G_b - 1) / (D_b - 1), the other two axes the field's own weights.  For ``basis="linear"`` it is
    piecewise constant along b and one-sided at node planes (a voxel on a node gets its own cell's slope); for
    ``basis="bspline"`` it is continuous.  Any dtype: in float64, the yardstick of the kernels."""
    _check_basis(basis)
    columns = []
    for b in range(3):
        u = displacement
        for axis, D in enumerate(shape):
            G = u.shape[axis + 1]
            c, t = _cells(int(D), G, u.device, u.dtype, _span(D, box, axis))
            t = t.reshape([-1 if d == axis + 1 else 1 for d in range(4)])
            scale = (G - 1) / (int(D) - 1) if axis == b else 1.0
            if basis == "linear":
                lo, hi = u.index_select(axis + 1, c), u.index_select(axis + 1, c + 1)
                u = (hi - lo) * scale if axis == b else (1 - t) * lo + t * hi
            else:
                ws = bspline_derivative_weights(t) if axis == b else bspline_weights(t)
                u = sum(w * u.index_select(axis + 1, (c - 1 + k).clamp(0, G - 1)) for k, w in enumerate(ws)) * scale
        columns.append(u)
    return torch.stack(columns, dim=1)


def _determinant(J: torch.Tensor) -> torch.Tensor:
    """det of (3, 3, ...) by cofactor expansion along the first row."""
    return (J[0, 0] * (J[1, 1] * J[2, 2] - J[1, 2] * J[2, 1]) + J[0, 1] * (J[1, 2] * J[2, 0] - J[1, 0] * J[2, 2])
            + J[0, 2] * (J[1, 0] * J[2, 1] - J[1, 1] * J[2, 0]))


def jacobian_reference(displacement: torch.Tensor, shape, basis: str = "linear") -> torch.Tensor:
    """The definition of :func:`jacobian_determinant` in torch: det(I + du/dx) of :func:`field_jacobian`,
    (Dx, Dy, Dz), in the dtype of the lattice; autograd gives the lattice gradient."""
    J = field_jacobian(displacement, shape, basis)
    eye = torch.eye(3, dtype=J.dtype, device=J.device).reshape(3, 3, 1, 1, 1)
    return _determinant(J + eye)


def _check_eps(eps):
    if not 0.0 < float(eps) <= 1.0:
        raise ValueError(f"eps must be in (0, 1], got {eps!r}")


def volume_penalty_of(det: torch.Tensor, eps: float = 0.1) -> torch.Tensor:
    """psi of a determinant map, elementwise: ln^2 d for d >= eps, its C^2 quadratic continuation below
    (include/diffdrr_jacobian_hip.h)."""
    _check_eps(eps)
    le = math.log(eps)
    x = det - eps
    below = le * le + (2 * le / eps) * x + ((1 - le) / eps ** 2) * x * x
    return torch.where(det >= eps, det.clamp(min=eps).log() ** 2, below)


def volume_penalty_reference(displacement: torch.Tensor, shape, basis: str = "linear", eps: float = 0.1):
    """The definition of :func:`volume_penalty` in torch: the mean of psi(det) over the voxels (Rohlfing et al.
    2003, with a quadratic continuation below ``eps`` so that a folded start has a finite gradient)."""
    return volume_penalty_of(jacobian_reference(displacement, shape, basis), eps).mean()


def sample_coordinates(displacement: torch.Tensor, shape, basis: str = "linear", box=None) -> torch.Tensor:
    """p (3, Dx, Dy, Dz) = x + u(x), clamped to [-2, D_a + 1] (which changes no sample); with ``box`` on its voxels
    only (see :func:`dense_field`)."""
    u = dense_field(displacement, shape, basis, box)
    p = []
    for a, D in enumerate(shape):
        x = torch.arange(*_span(D, box, a), device=u.device, dtype=u.dtype).reshape(
            [-1 if d == a else 1 for d in range(3)])
        p.append((x + u[a]).clamp(-2.0, float(D) + 1.0))
    return torch.stack(p)


def _trilinear(volume, pairs, padding, part=None):
    """sum over the 8 corners of w_c V[i0 + c] from the per-axis (floor, fraction) ``pairs``.  The voxels are
    gathered from ``volume`` as it is and cast to the weights' dtype after the gather.  ``part`` = (shape, three
    (start, stop) ranges): ``volume`` holds only those ranges of a volume of ``shape``, and every voxel the
    samples reach must lie in them."""
    shape, held = (volume.shape, None) if part is None else part
    axes = []
    for a, (D, (i, f)) in enumerate(zip(shape, pairs)):
        pair = []
        for idx, w in ((i, 1 - f), (i + 1, f)):
            if padding == "zeros":
                w = w * ((idx >= 0) & (idx < D)).to(w.dtype)
            idx = idx.clamp(0, int(D) - 1)
            if held is not None:
                start, stop = (int(v) for v in held[a])
                if stop - start != volume.shape[a] or int(idx.min()) < start or int(idx.max()) >= stop:
                    raise ValueError(f"axis {a}: the samples reach voxels {int(idx.min())} .. {int(idx.max())}, the "
                                     f"part of the volume given is {start} .. {stop - 1} ({volume.shape[a]} voxels)")
                idx = idx - start
            pair.append((idx, w))
        axes.append(pair)
    out = 0
    for ix, wx in axes[0]:
        for iy, wy in axes[1]:
            for iz, wz in axes[2]:
                out = out + wx * wy * wz * volume[ix, iy, iz].to(wz.dtype)
    return out


def sample_displaced(volume: torch.Tensor, u: torch.Tensor, padding: str = "zeros", box=None,
                     part=None) -> torch.Tensor:
    """``V(x + u(x))`` for a dense field ``u`` (3, Dx, Dy, Dz) in voxels, trilinear.  floor(p) = x + floor(u) and
    f = u - floor(u) are formed from u, as the kernels form them: they carry the precision of u (a few voxels),
    not that of p = x + u (up to D).  u_a is clamped to [-(D_a + 2), D_a + 2] first (which changes no sample).

    ``box``, three (start, stop) voxel ranges: ``u`` is the field on those voxels only and so is the result.
    ``part`` = (shape, three (start, stop) ranges): ``volume`` is only that part of a volume of ``shape`` (for a
    box of a volume too large to copy or to take a gradient of); it must hold every voxel the samples reach."""
    shape = volume.shape if part is None else part[0]
    pairs = []
    for a, D in enumerate(shape):
        ua = u[a].clamp(-(float(D) + 2.0), float(D) + 2.0)
        fl = ua.detach().floor()
        x = torch.arange(*_span(D, box, a), device=u.device).reshape([-1 if d == a else 1 for d in range(3)])
        pairs.append((x + fl.long(), ua - fl))
    return _trilinear(volume, pairs, padding, part)


def warp_reference(volume: torch.Tensor, displacement: torch.Tensor, padding: str = "zeros",
                   basis: str = "linear", box=None, part=None) -> torch.Tensor:
    """The definition of :func:`warp_volume` by torch indexing, in the dtype of the lattice and on the
    arguments' device; autograd gives both gradients (``floor`` has none: at f = 0 the derivative is the forward
    difference).  ``basis``: see :func:`dense_field`; ``box`` and ``part``: see :func:`sample_displaced`."""
    if padding not in _PADDING:
        raise ValueError(f"padding must be 'zeros' or 'border', not {padding!r}")
    _check_basis(basis)
    shape = volume.shape if part is None else part[0]
    if volume.dim() != 3 or len(shape) != 3 or displacement.dim() != 4 or displacement.shape[0] != 3:
        raise ValueError("a (Dx, Dy, Dz) volume and a (3, Gx, Gy, Gz) lattice expected")
    if any(g < 2 or g > d for g, d in zip(displacement.shape[1:], shape)):
        raise ValueError("the lattice needs 2 <= G_a <= D_a nodes per axis")
    if basis == "bspline":  # (the linear basis rounds p itself, as it always has)
        return sample_displaced(volume, dense_field(displacement, shape, basis, box), padding, box, part)
    p = sample_coordinates(displacement, shape, box=box)
    pairs = []
    for a in range(3):
        fl = p[a].detach().floor()
        pairs.append((fl.long(), p[a] - fl))
    return _trilinear(volume, pairs, padding, part)


# ------------------------------------------------------------------------------------------------ kernels
class _WarpFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, volume, displacement, padding):
        ctx.padding = padding
        ctx.save_for_backward(volume, displacement)
        return ops.warp_forward(volume, displacement, padding)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        volume, displacement = ctx.saved_tensors
        grad_out = grad_out.contiguous()
        g_volume = ops.warp_backward_volume(displacement, grad_out, ctx.padding) if ctx.needs_input_grad[0] else None
        g_disp = ops.warp_backward_displacement(volume, displacement, grad_out, ctx.padding) \
            if ctx.needs_input_grad[1] else None
        return g_volume, g_disp, None


class _BsplineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, volume, displacement, padding):
        ctx.padding = padding
        ctx.save_for_backward(volume, displacement)
        return ops.bspline_forward(volume, displacement, padding)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        volume, displacement = ctx.saved_tensors
        grad_out = grad_out.contiguous()
        g_volume = ops.bspline_backward_volume(displacement, grad_out, ctx.padding) \
            if ctx.needs_input_grad[0] else None
        g_disp = ops.bspline_backward_displacement(volume, displacement, grad_out, ctx.padding) \
            if ctx.needs_input_grad[1] else None
        return g_volume, g_disp, None


class _JacobianFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, displacement, shape, basis):
        ctx.shape, ctx.basis = shape, basis
        ctx.save_for_backward(displacement)
        return ops.jacobian_determinant(displacement, shape, basis)[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        displacement, = ctx.saved_tensors
        return ops.jacobian_backward(displacement, ctx.shape, grad_out.contiguous(), ctx.basis), None, None


class _VolumePenaltyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, displacement, shape, basis, eps):
        ctx.shape, ctx.basis, ctx.eps = shape, basis, eps
        ctx.save_for_backward(displacement)
        return ops.jacobian_penalty(displacement, shape, basis, eps)[0].to(torch.float32).reshape(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        displacement, = ctx.saved_tensors
        return grad_out * ops.jacobian_backward(displacement, ctx.shape, None, ctx.basis, ctx.eps), None, None, None


class JacobianStatistics(NamedTuple):
    """Where the map x -> x + u(x) folds: device tensors, no host synchronisation."""
    folded: torch.Tensor    # int64 scalar: the number of voxels with det <= 0
    minimum: torch.Tensor   # float32 scalar: min det
    maximum: torch.Tensor   # float32 scalar: max det


def jacobian_determinant(displacement: torch.Tensor, shape, basis: str = "linear") -> torch.Tensor:
    """det(I + du/dx) at every voxel of a volume of ``shape`` (Dx, Dy, Dz), for the lattice ``displacement``
    (3, Gx, Gy, Gz) in voxels of each axis, float32, contiguous and on the GPU, 2 <= G_a <= D_a: the local volume
    change of the map x -> x + u(x); <= 0 where it folds.  ``u`` as in :func:`warp_volume`; the derivative is the
    analytic one of the voxel's cell (:func:`field_jacobian`), so for ``basis="linear"`` it is piecewise and
    one-sided at node planes.  Differentiable in ``displacement`` (no atomics: bitwise reproducible).  The
    determinant does not depend on the voxel pitch.  Anything outside the domain raises ValueError naming the
    condition."""
    dims, _, _ = ops._check_jacobian("jacobian_determinant", shape, displacement, basis)
    return _JacobianFn.apply(displacement, dims, basis)


def jacobian_statistics(displacement: torch.Tensor, shape, basis: str = "linear") -> JacobianStatistics:
    """(folded, minimum, maximum) of :func:`jacobian_determinant` without the map in memory and without a host
    synchronisation: the number of voxels with det <= 0 and the extremes, as device scalars."""
    _, folded, rng = ops.jacobian_penalty(displacement.detach(), shape, basis, 1.0)
    return JacobianStatistics(folded[0], rng[0], rng[1])


def volume_penalty(displacement: torch.Tensor, shape, basis: str = "linear", eps: float = 0.1) -> torch.Tensor:
    """The volume-preservation penalty (1 / N) sum_x psi(det J(x)), psi = ln^2 above ``eps`` and its C^2 quadratic
    continuation below (finite, with a finite gradient, for folded voxels), 0 < eps <= 1: a differentiable
    float32 scalar, fused -- neither the derivative field nor the determinant map is in memory, forward or
    backward.  The arguments are those of :func:`jacobian_determinant`."""
    dims, _, _ = ops._check_jacobian("volume_penalty", shape, displacement, basis, eps)
    return _VolumePenaltyFn.apply(displacement, dims, basis, float(eps))


def warp_volume(volume: torch.Tensor, displacement: torch.Tensor, padding: str = "zeros",
                basis: str = "linear") -> torch.Tensor:
    """``W[x] = V(x + u(x))``: ``volume`` (Dx, Dy, Dz) and the lattice ``displacement`` (3, Gx, Gy, Gz), in
    voxels of each axis, 2 <= G_a <= D_a, both float32, contiguous and on the GPU; trilinear sampling with
    ``padding`` "zeros" or "border".  ``u`` is the trilinear interpolation of the lattice (``basis="linear"``)
    or its cubic B-spline (``basis="bspline"``, which approximates: the field at a node is not the node's
    coefficient).  Differentiable in both arguments.  Anything outside that domain -- a CPU tensor included:
    there is no CPU fallback -- raises ValueError naming the condition."""
    _check_basis(basis)
    if basis == "bspline":
        ops._check_bspline("warp_volume", getattr(volume, "shape", ()), displacement, padding, volume=volume)
        return _BsplineFn.apply(volume, displacement, padding)
    ops._check_warp("warp_volume", getattr(volume, "shape", ()), displacement, padding, volume=volume)
    return _WarpFn.apply(volume, displacement, padding)


class FreeFormDeformation(nn.Module):
    """A learnable smooth deformation of ``drr``'s volume in front of its renderer (between ``Registration``,
    which moves six pose numbers, and ``Reconstruction``, which moves every voxel): ``displacement`` is an
    ``nn.Parameter`` of zeros, (3, Gx, Gy, Gz), in MILLIMETRES along the volume's index axes; it is divided by
    the voxel pitch (the column norms of ``drr``'s affine) and handed to :func:`warp_volume`.

    ``forward`` renders the deformed volume through ``drr`` with the arguments and on the routes of a ``DRR``
    whose own ``density`` requires a gradient; ``drr``'s own volume is read, never written.

    ``basis="bspline"`` reads the same parameter as the coefficients of a cubic B-spline: a C^2 field, with
    :meth:`bending_energy` as its regulariser.  The spline approximates -- the displacement at a node is a
    weighted mean of the coefficients around it, not the node's own."""

    def __init__(self, drr, grid=(8, 8, 8), padding: str = "zeros", basis: str = "linear"):
        super().__init__()
        if padding not in _PADDING:
            raise ValueError(f"padding must be 'zeros' or 'border', not {padding!r}")
        _check_basis(basis)
        grid = tuple(int(g) for g in grid)
        shape = tuple(drr.density.shape)
        if len(grid) != 3 or any(g < 2 or g > d for g, d in zip(grid, shape)):
            raise ValueError(f"grid must be (Gx, Gy, Gz) with 2 <= G_a <= D_a, got {grid} for a volume of {shape}")
        if drr.density.dtype != torch.float32:
            raise ValueError(f"a float32 volume expected, got {drr.density.dtype}")
        self.drr = drr
        self.padding = padding
        self.basis = basis
        dev = drr.density.device
        affine = drr._affine.reshape(-1, 4, 4)[0, :3, :3]
        self.register_buffer("pitch", affine.norm(dim=0).reshape(3, 1, 1, 1).to(dev, torch.float32).contiguous(),
                             persistent=False)
        self.displacement = nn.Parameter(torch.zeros(3, *grid, dtype=torch.float32, device=dev))

    def warped(self) -> torch.Tensor:
        """The deformed volume (the shape of ``drr``'s)."""
        return warp_volume(self.drr.density, self._voxel_lattice(), self.padding, self.basis)

    def forward(self, *pose_args, **kwargs):
        buffers = self.drr._buffers
        theirs = buffers["density"]
        buffers["density"] = self.warped()
        try:
            return self.drr(*pose_args, **kwargs)
        finally:
            buffers["density"] = theirs

    def _voxel_lattice(self) -> torch.Tensor:
        return (self.displacement / self.pitch).contiguous()

    def jacobian_determinant(self) -> torch.Tensor:
        """det(I + du/dx) at every voxel of the volume (:func:`jacobian_determinant` of ``displacement / pitch``,
        as :meth:`warped` reads it), differentiable in ``displacement``.  The determinant is independent of the
        pitch: in millimetres J is S J S^-1.  For ``basis="linear"`` it is piecewise constant along each axis and
        one-sided at node planes."""
        return jacobian_determinant(self._voxel_lattice(), tuple(self.drr.density.shape), self.basis)

    def folding(self) -> JacobianStatistics:
        """(folded, minimum, maximum): the number of voxels where the deformation folds (det <= 0) and the
        extremes of the determinant, as device scalars without a host synchronisation and without the map in
        memory.  Independent of the pitch; for ``basis="linear"`` piecewise and one-sided at node planes."""
        return jacobian_statistics(self._voxel_lattice(), tuple(self.drr.density.shape), self.basis)

    def volume_penalty(self, eps: float = 0.1) -> torch.Tensor:
        """The volume-preservation regulariser (:func:`volume_penalty`): the mean over the voxels of ln^2 det,
        continued quadratically below ``eps`` so that a folded lattice is pushed back.  Differentiable in
        ``displacement`` (millimetres); independent of the pitch; for ``basis="linear"`` the determinant is
        piecewise and one-sided at node planes."""
        return volume_penalty(self._voxel_lattice(), tuple(self.drr.density.shape), self.basis, eps)

    def smoothness(self) -> torch.Tensor:
        """Mean squared first difference of the lattice (mm^2), over the three lattice axes."""
        d = self.displacement
        diffs = [d.diff(dim=a + 1) for a in range(3)]
        return sum(x.pow(2).sum() for x in diffs) / sum(x.numel() for x in diffs)

    def bending_energy(self) -> torch.Tensor:
        """The discrete bending energy of the lattice (mm^2): the squared second differences along each lattice
        axis plus twice the squared mixed second differences of each pair of axes, summed and divided by the
        number of differences.  An axis of fewer than 3 nodes has no second difference and adds nothing; a
        lattice that is affine in the node index has none of either kind: 0."""
        d = self.displacement
        pure = [d.diff(n=2, dim=a + 1) for a in range(3)]
        mixed = [d.diff(dim=a + 1).diff(dim=b + 1) for a in range(3) for b in range(a + 1, 3)]
        total = sum(x.pow(2).sum() for x in pure) + 2 * sum(x.pow(2).sum() for x in mixed)
        return total / sum(x.numel() for x in pure + mixed)
