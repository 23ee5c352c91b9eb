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
"""
from __future__ import annotations

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
        return warp_volume(self.drr.density, (self.displacement / self.pitch).contiguous(), self.padding, self.basis)

    def forward(self, *pose_args, **kwargs):
        buffers = self.drr._buffers
        theirs = buffers["density"]
        buffers["density"] = self.warped()
        try:
            return self.drr(*pose_args, **kwargs)
        finally:
            buffers["density"] = theirs

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
