"""Volume reconstruction from projections (reference ``notebooks/tutorials/reconstruction.ipynb:116-122,
183-217``): a learnable volume in front of a ``DRR``, the 3-D total-variation regulariser sparse-view
reconstruction needs, and the volume's Adam step with the non-negativity projection folded in.

The renderers differentiate with respect to the volume already (``ddrr_*_backward_volume_bricks``); what
is here owns the rest of the iteration, each as one pass over the volume
(``include/diffdrr_recon_hip.h``): ``TotalVariation3d`` (value and gradient, no volume-sized temporary)
and ``VolumeAdam`` (update + clamp).  ``Reconstruction`` is the counterpart of ``Registration``.

    recon = Reconstruction(drr).to("cuda")
    tv = TotalVariation3d.for_drr(drr)
    opt = recon.make_optimizer(lr=0.02)
    for it in range(n):
        data_loss, tv_value = recon.step(opt, measured, rot, xyz, parameterization="euler_angles",
                                         convention="ZXY", regularizer=tv, weight=1e-3)
"""
from __future__ import annotations

from contextlib import contextmanager

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import ops

_MODES = ("isotropic", "anisotropic")


def _check_tv_arguments(volume, spacing, mode):
    if not torch.is_tensor(volume) or volume.dim() != 3:
        raise ValueError(f"total variation takes a (Dx, Dy, Dz) volume, got shape "
                         f"{tuple(volume.shape) if torch.is_tensor(volume) else type(volume).__name__}")
    if mode not in _MODES:
        raise ValueError(f"mode must be 'isotropic' or 'anisotropic', not {mode!r}")
    spacing = tuple(float(s) for s in spacing)
    if len(spacing) != 3 or not all(0.0 < s < float("inf") for s in spacing):
        raise ValueError(f"spacing must be three positive numbers, not {spacing}")
    return spacing


def total_variation_3d(volume, spacing=(1.0, 1.0, 1.0), mode="isotropic", eps=1e-3):
    """Total variation of a (Dx, Dy, Dz) volume as a torch composition -- the definition the kernel is
    held to, and the route of everything the kernel does not take (CPU, float64, strided volumes):
    forward differences ``d_a = (V[.. + 1 ..] - V) / spacing_a`` that are zero past the last plane;
    isotropic ``sum sqrt(dx^2 + dy^2 + dz^2 + eps^2)``, anisotropic ``sum |dx| + |dy| + |dz|``.
    Differentiable by autograd (``abs`` differentiates to ``sign`` with ``sign(0) = 0``: the gradient at
    a volume of zeros is exactly zero in both modes)."""
    sx, sy, sz = _check_tv_arguments(volume, spacing, mode)
    pad = torch.nn.functional.pad
    dx = pad((volume[1:] - volume[:-1]) / sx, (0, 0, 0, 0, 0, 1))
    dy = pad((volume[:, 1:] - volume[:, :-1]) / sy, (0, 0, 0, 1))
    dz = pad((volume[:, :, 1:] - volume[:, :, :-1]) / sz, (0, 1))
    if mode == "isotropic":
        return torch.sqrt(dx * dx + dy * dy + dz * dz + eps * eps).sum()
    return dx.abs().sum() + dy.abs().sum() + dz.abs().sum()


class _TV3dFn(torch.autograd.Function):
    """The fused route of ``TotalVariation3d.forward``: the value in one pass that reads the volume, the
    gradient in one more that reads it and writes the gradient, scaled by the upstream gradient on the
    device (``ops.tv3d``)."""

    @staticmethod
    def forward(ctx, volume, spacing, mode, eps):
        ctx.save_for_backward(volume)
        ctx.cfg = (spacing, mode, eps)
        return ops.tv3d(volume, spacing, mode, eps)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (volume,) = ctx.saved_tensors
        spacing, mode, eps = ctx.cfg
        grad = torch.empty_like(volume)
        ops.tv3d(volume, spacing, mode, eps, grad=grad, scale=g.to(torch.float32).reshape(1).contiguous())
        return grad, None, None, None


def _fused_volume(volume) -> bool:
    """The kernels' domain: float32, contiguous, on the device (the dispatch rule of
    ``MutualInformation.forward``)."""
    return (ops.on_device(volume) and volume.dtype == torch.float32 and volume.is_contiguous()
            and volume.numel() > 0)


class TotalVariation3d(nn.Module):
    """3-D total variation of a volume -- :func:`total_variation_3d` -- as a module.  float32 contiguous
    volumes on the device take the fused kernel (value and gradient each one pass over the volume, bitwise
    reproducible); everything else the composition."""

    def __init__(self, mode="isotropic", eps=1e-3, spacing=(1.0, 1.0, 1.0)):
        super().__init__()
        if mode not in _MODES:
            raise ValueError(f"mode must be 'isotropic' or 'anisotropic', not {mode!r}")
        if not 0.0 <= float(eps) < float("inf"):
            raise ValueError(f"eps must be >= 0, not {eps}")
        self.mode = mode
        self.eps = float(eps)
        self.spacing = tuple(float(s) for s in spacing)
        if len(self.spacing) != 3 or not all(0.0 < s < float("inf") for s in self.spacing):
            raise ValueError(f"spacing must be three positive numbers, not {spacing}")

    @classmethod
    def for_drr(cls, drr, mode="isotropic", eps=1e-3):
        """The regulariser of ``drr``'s volume: the voxel spacing is the norm of the affine's columns."""
        affine = drr._affine.reshape(-1, 4, 4)[0, :3, :3]
        return cls(mode=mode, eps=eps, spacing=affine.norm(dim=0).tolist())

    def forward(self, volume):
        _check_tv_arguments(volume, self.spacing, self.mode)
        if _fused_volume(volume):
            return _TV3dFn.apply(volume, self.spacing, self.mode, self.eps)
        return total_variation_3d(volume, self.spacing, self.mode, self.eps)

    @torch.no_grad()
    def add_gradient_(self, volume, grad, weight=1.0):
        """``grad += weight * dTV/dV(volume)`` in place -> the (unweighted) value, detached.  On the fused
        route one launch that reads the volume and reads and writes ``grad``: no second volume-sized
        gradient for autograd to allocate and add."""
        _check_tv_arguments(volume, self.spacing, self.mode)
        if grad.shape != volume.shape:
            raise ValueError(f"grad {tuple(grad.shape)} does not have the volume's shape {tuple(volume.shape)}")
        if _fused_volume(volume) and _fused_volume(grad) and grad.device == volume.device:
            return ops.tv3d(volume.detach(), self.spacing, self.mode, self.eps, grad=grad, accumulate=True,
                            weight=float(weight))
        with torch.enable_grad():
            v = volume.detach().requires_grad_(True)
            value = total_variation_3d(v, self.spacing, self.mode, self.eps)
            (g,) = torch.autograd.grad(value, [v])
        grad.add_(g.to(grad.dtype), alpha=float(weight))
        return value.detach()

    def extra_repr(self):
        return f"mode={self.mode!r}, eps={self.eps}, spacing={self.spacing}"


class VolumeAdam(torch.optim.Optimizer):
    """``torch.optim.Adam(params, lr, betas, eps, maximize=maximize)`` followed by
    ``p.clamp_(lower, upper)`` -- the optimiser of the reference's reconstruction loop and the projection
    a density needs -- as ONE pass over each parameter (``ddrr_recon_adam_step``: 16 B read and 12 B
    written per element).  Same update rule (no weight decay, no amsgrad) with the operations in the order
    of torch's single-tensor implementation, same state layout (``state[p] = {"step", "exp_avg",
    "exp_avg_sq"}``).  The step counters live on the device and the state exists from the start, as
    ``PoseAdam``'s and for the same reasons: nothing synchronises, and a first step inside a graph capture
    would not bake zero-fills into the graph.  Parameters: float32, contiguous, on the GPU."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, lower=None, upper=None, maximize=False):
        if not lr >= 0.0:
            raise ValueError(f"VolumeAdam: invalid learning rate {lr}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or not eps >= 0.0:
            raise ValueError("VolumeAdam: invalid betas / eps")
        if lower is not None and upper is not None and not lower <= upper:
            raise ValueError(f"VolumeAdam: lower {lower} must be <= upper {upper}")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, lower=lower, upper=upper,
                                      maximize=maximize))
        for group in self.param_groups:
            for p in group["params"]:
                if p.dtype != torch.float32:
                    raise ValueError(f"VolumeAdam: float32 parameters only, got {p.dtype}")
                if not p.is_contiguous():
                    raise ValueError("VolumeAdam: contiguous parameters only")
                if not ops.on_device(p):
                    raise ValueError("VolumeAdam: parameters on the GPU only (torch.optim.Adam serves the host)")
                self._state(p)

    def _state(self, p):
        st = self.state[p]
        if not st:
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return st

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("VolumeAdam does not support sparse gradients")
                st = self._state(p)
                ops.volume_adam_step(p, p.grad.contiguous(), st["exp_avg"], st["exp_avg_sq"], st["step"],
                                     lr=group["lr"], betas=group["betas"], eps=group["eps"],
                                     lower=group["lower"], upper=group["upper"], maximize=group["maximize"])
        return loss


class Reconstruction(nn.Module):
    """A learnable volume in front of a ``DRR`` (the counterpart of ``Registration``; reference
    ``notebooks/tutorials/reconstruction.ipynb:116-122``): ``density`` is an ``nn.Parameter`` of the shape
    of ``drr``'s volume -- zeros, or ``init`` -- and ``forward`` renders IT through ``drr``, with the
    arguments and on the routes of a ``DRR`` whose own ``density`` requires a gradient.  ``drr`` supplies
    the geometry (affine, detector, renderer); its own volume is not read.

    ``lower`` / ``upper``: the bounds a volume of this kind lives in (a density is non-negative), handed to
    ``VolumeAdam`` by :meth:`make_optimizer`."""

    def __init__(self, drr, init: torch.Tensor | None = None, lower: float | None = 0.0,
                 upper: float | None = None):
        super().__init__()
        self.drr = drr
        shape = drr.density.shape
        if init is None:
            init = torch.zeros(shape, dtype=torch.float32, device=drr.density.device)
        else:
            if tuple(init.shape) != tuple(shape):
                raise ValueError(f"init has shape {tuple(init.shape)}, the volume {tuple(shape)}")
            init = init.detach().to(device=drr.density.device, dtype=torch.float32).clone(
                memory_format=torch.contiguous_format)
        if lower is not None and upper is not None and not lower <= upper:
            raise ValueError(f"lower {lower} must be <= upper {upper}")
        self.density = nn.Parameter(init)
        self.lower, self.upper = lower, upper

    @classmethod
    def from_fdk(cls, drr, measured, *pose_args, window="ram-lak", lower: float | None = 0.0,
                 upper: float | None = None, **kw):
        """A ``Reconstruction`` that starts from the filtered backprojection of the views ``measured`` of a
        full circular orbit (``analytic.fdk``: the pose arguments of ``DRR.forward``; ``view_weights=``,
        ``isocenter=``), clamped to ``[lower, upper]``, instead of from zeros."""
        from .analytic import fdk

        start = fdk(drr, measured, *pose_args, window=window, **kw)
        if lower is not None or upper is not None:
            start = start.clamp(min=lower, max=upper)
        return cls(drr, init=start.reshape(drr.density.shape), lower=lower, upper=upper)

    @contextmanager
    def _own_density(self):
        """``drr`` renders ``self.density`` for the length of the block: every route of ``DRR.forward``
        reads the volume as ``drr.density``, so that is what is swapped (and put back)."""
        buffers = self.drr._buffers
        theirs = buffers["density"]
        buffers["density"] = self.density
        try:
            yield
        finally:
            buffers["density"] = theirs

    def forward(self, *pose_args, **kwargs):
        with self._own_density():
            return self.drr(*pose_args, **kwargs)

    def forward_rays(self, source, target, **kwargs):
        """The tutorial's ``drr.render(self.density, source, target)``: world-space rays -> (B, C, N)."""
        return self.drr.render(self.density, source, target, **kwargs)

    def make_optimizer(self, lr, betas=(0.9, 0.999), eps=1e-8):
        return VolumeAdam([self.density], lr, betas=betas, eps=eps, lower=self.lower, upper=self.upper)

    def step(self, optimizer, measured, *pose_args, regularizer=None, weight=0.0, **kwargs):
        """One iteration: render the views of ``pose_args``, mean squared error against ``measured`` (the
        shape ``forward`` returns), backward, ``grad += weight * d regularizer / d density``
        (``TotalVariation3d.add_gradient_``), ``optimizer.step()``.  -> (data loss, regulariser value), both
        0-dim device tensors (the regulariser's unweighted; zero without one).  Nothing synchronises with
        the host."""
        optimizer.zero_grad(set_to_none=True)
        img = self(*pose_args, **kwargs)
        if img.shape != measured.shape:
            raise ValueError(f"measured has shape {tuple(measured.shape)}, the render {tuple(img.shape)}")
        loss = torch.nn.functional.mse_loss(img, measured)
        loss.backward()
        if regularizer is not None:
            value = regularizer.add_gradient_(self.density, self.density.grad, weight)
        else:
            value = torch.zeros((), dtype=loss.dtype, device=loss.device)
        optimizer.step()
        return loss.detach(), value
