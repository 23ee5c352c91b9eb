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

The proximal route to the same problem, without a learning rate and without smoothing the TV (FISTA with a fast
gradient projection inner solver, Beck & Teboulle 2009; ``include/diffdrr_prox_hip.h``):

    L = recon.lipschitz(rot, xyz, parameterization="euler_angles", convention="ZXY")
    fista = recon.make_fista(L, regularizer=tv, weight=1e-3, inner_iterations=10)
    for it in range(n):
        data_loss, tv_value = fista.step(measured, rot, xyz, parameterization="euler_angles", convention="ZXY")

With a fixed number of inner iterations the prox is inexact, and acceleration accumulates that error when
``weight / L`` is large against the volume's values: raise ``inner_iterations`` or call ``fista.restart()`` every few
steps there (DESIGN.md section 3.14 has the numbers).
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


def tv_gradient_operator(volume, spacing=(1.0, 1.0, 1.0)):
    """``D`` of :func:`total_variation_3d`: the forward differences of a (Dx, Dy, Dz) volume, zero past the last
    plane, stacked -> (3, Dx, Dy, Dz)."""
    sx, sy, sz = _check_tv_arguments(volume, spacing, "isotropic")
    out = volume.new_zeros((3, *volume.shape))
    out[0, :-1] = (volume[1:] - volume[:-1]) / sx
    out[1, :, :-1] = (volume[:, 1:] - volume[:, :-1]) / sy
    out[2, :, :, :-1] = (volume[:, :, 1:] - volume[:, :, :-1]) / sz
    return out


def tv_divergence_adjoint(dual, spacing=(1.0, 1.0, 1.0)):
    """``D^T``, the exact adjoint of :func:`tv_gradient_operator` (``<D x, p> = <x, D^T p>``): a (3, Dx, Dy, Dz)
    dual field -> (Dx, Dy, Dz).  What the field holds on the last plane of a component's own axis never
    contributes."""
    if not torch.is_tensor(dual) or dual.dim() != 4 or dual.shape[0] != 3:
        raise ValueError("a (3, Dx, Dy, Dz) dual field expected")
    sx, sy, sz = _check_tv_arguments(dual[0], spacing, "isotropic")
    out = torch.zeros_like(dual[0])
    ux, uy, uz = dual[0, :-1] / sx, dual[1, :, :-1] / sy, dual[2, :, :, :-1] / sz
    out[:-1] -= ux
    out[1:] += ux
    out[:, :-1] -= uy
    out[:, 1:] += uy
    out[:, :, :-1] -= uz
    out[:, :, 1:] += uz
    return out


def _check_prox_arguments(volume, weight, spacing, mode, iterations, lower, upper, dual):
    spacing = _check_tv_arguments(volume, spacing, mode)
    if not 0.0 <= float(weight) < float("inf"):
        raise ValueError(f"weight must be >= 0 and finite, not {weight}")
    if int(iterations) != iterations or iterations < 0:
        raise ValueError(f"iterations must be an integer >= 0, not {iterations}")
    if lower is not None and upper is not None and not lower <= upper:
        raise ValueError(f"lower {lower} must be <= upper {upper}")
    if dual is not None and (not torch.is_tensor(dual) or tuple(dual.shape) != (3, *volume.shape)
                             or dual.dtype != volume.dtype or dual.device != volume.device):
        raise ValueError(f"dual must be a {volume.dtype} tensor of shape {(3, *volume.shape)} on {volume.device}")
    return spacing


def _box(v, lower, upper):
    return v if lower is None and upper is None else v.clamp(min=lower, max=upper)


@torch.no_grad()
def prox_total_variation_3d(volume, weight, spacing=(1.0, 1.0, 1.0), mode="isotropic", iterations=20, lower=None,
                            upper=None, dual=None):
    """``argmin_{lower <= x <= upper} 1/2 |x - volume|^2 + weight TV(x)`` for the non-smooth TV (no ``eps``) by
    ``iterations`` steps of the fast gradient projection of Beck & Teboulle (2009) on the dual, as a torch
    composition -- the definition the kernel is held to (include/diffdrr_prox_hip.h), and the route of everything
    the kernel does not take (CPU, float64, strided volumes).  ``dual``: the (3, Dx, Dy, Dz) start p_0, updated in
    place to p_n (zeros are allocated for None) -> (x, dual).  Not differentiable.

        Lip = 4 (1/sx^2 + 1/sy^2 + 1/sz^2);  t_0 = 1;  r_0 = p_0
        x = P_C(volume - weight D^T r_k);  p_{k+1} = Pi(r_k + D x / (Lip weight))
        t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2;  r_{k+1} = p_{k+1} + ((t_k - 1) / t_{k+1}) (p_{k+1} - p_k)
        x = P_C(volume - weight D^T p_n)

    ``weight == 0`` returns ``P_C(volume)`` and leaves the dual as given."""
    spacing = _check_prox_arguments(volume, weight, spacing, mode, iterations, lower, upper, dual)
    if dual is None:
        dual = volume.new_zeros((3, *volume.shape))
    weight = float(weight)
    if weight == 0.0:
        return _box(volume.clone(), lower, upper), dual
    lip = 4.0 * sum(1.0 / (s * s) for s in spacing)
    p, r, t = dual.clone(), dual.clone(), 1.0
    for _ in range(int(iterations)):
        x = _box(volume - weight * tv_divergence_adjoint(r, spacing), lower, upper)
        q = r + tv_gradient_operator(x, spacing) / (lip * weight)
        if mode == "isotropic":
            q = q / q.pow(2).sum(0, keepdim=True).sqrt().clamp(min=1.0)
        else:
            q = q.clamp(-1.0, 1.0)
        t_next = 0.5 * (1.0 + (1.0 + 4.0 * t * t) ** 0.5)
        r = q + ((t - 1.0) / t_next) * (q - p)
        p, t = q, t_next
    dual.copy_(p)
    return _box(volume - weight * tv_divergence_adjoint(p, spacing), lower, upper), dual


def _next_t(t):
    return 0.5 * (1.0 + (1.0 + 4.0 * t * t) ** 0.5)


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

    @torch.no_grad()
    def prox(self, volume, weight, iterations=20, lower=None, upper=None, dual=None):
        """``argmin_{lower <= x <= upper} 1/2 |x - volume|^2 + weight TV(x)`` -- :func:`prox_total_variation_3d`
        with the module's mode and spacing -> x.  The prox is of the non-smooth TV: the module's ``eps`` is not
        used.  ``dual``: a (3, Dx, Dy, Dz) tensor, the warm start in and p_n out (updated in place); zeros are
        allocated for None.  float32 contiguous volumes on the device take the fused kernels (``ops.prox_tv3d``:
        two passes per iteration, bitwise reproducible), everything else the composition."""
        return self._prox(volume, weight, iterations, lower, upper, dual)[0]

    def _prox(self, volume, weight, iterations, lower, upper, dual, x_prev=None, beta=0.0):
        """:meth:`prox` -> (x, y, dual), with ``y = x + beta (x - x_prev)`` (None without ``x_prev``): on the
        fused route the extrapolation comes out of the launch that writes x."""
        _check_prox_arguments(volume, weight, self.spacing, self.mode, iterations, lower, upper, dual)
        if dual is None:
            dual = volume.new_zeros((3, *volume.shape))
        if (_fused_volume(volume) and dual.is_contiguous()
                and (x_prev is None or (_fused_volume(x_prev) and x_prev.device == volume.device))):
            x, y = ops.prox_tv3d(volume.detach(), float(weight), self.spacing, self.mode, int(iterations), lower,
                                 upper, dual, x_prev=x_prev, beta=float(beta))
            return x, y, dual
        x, _ = prox_total_variation_3d(volume.detach(), weight, self.spacing, self.mode, iterations, lower, upper,
                                       dual)
        return x, (None if x_prev is None else torch.add(x, x - x_prev, alpha=float(beta))), dual

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
    def _own_density(self, volume=None):
        """``drr`` renders ``self.density`` -- or ``volume``, a tensor of its shape -- for the length of the
        block: every route of ``DRR.forward`` reads the volume as ``drr.density``, so that is what is swapped
        (and put back)."""
        buffers = self.drr._buffers
        theirs = buffers["density"]
        buffers["density"] = self.density if volume is None else volume
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

    def _leaf_like_density(self):
        """A tensor that requires a gradient, to hand volumes other than ``density`` to :meth:`_data_gradient`
        as ``leaf.data = volume``: one tensor for many volumes, so that what the renderers cache per volume
        tensor (``ops.brick_workspace``) is rebuilt in place instead of allocated per volume."""
        return torch.empty_like(self.density.data).requires_grad_(True)

    def _data_gradient(self, v, measured, pose_args, kwargs):
        """mse(A v, measured) -- against zeros for ``measured`` None -- and its gradient in ``v`` (a tensor that
        requires a gradient), rendered on the routes of :meth:`forward` -> (loss, gradient), both detached."""
        if v is not self.density:
            ops.invalidate_brick_workspace(v)  # (`v.data = volume` moves no version counter: rebuild, never guess)
        with torch.enable_grad():
            with self._own_density(v):
                img = self.drr(*pose_args, **kwargs)
            if measured is None:
                loss = img.square().mean()
            else:
                if img.shape != measured.shape:
                    raise ValueError(f"measured has shape {tuple(measured.shape)}, the render {tuple(img.shape)}")
                loss = torch.nn.functional.mse_loss(img, measured)
            (g,) = torch.autograd.grad(loss, [v])
        return loss.detach(), g

    @torch.no_grad()
    def lipschitz(self, *pose_args, iterations=12, safety=1.05, generator=None, **kwargs):
        """``safety`` times the largest eigenvalue of ``(2 / M) A^T A`` -- the Lipschitz constant of the gradient
        of ``mse(A V, measured)``, M the number of measured pixels, A the render of the views ``pose_args`` -- by
        ``iterations`` steps of power iteration from a normal random volume (``generator``).  A is linear, so
        ``(2 / M) A^T A v`` is the gradient of ``mse(A v, 0)`` through the routes :meth:`forward` takes.
        -> a Python float: the one host synchronisation, at the end.  ``density`` is not touched.  The Rayleigh
        quotients of the iterations (non-decreasing towards the eigenvalue) are kept on
        ``self.lipschitz_history``."""
        if int(iterations) != iterations or iterations < 1:
            raise ValueError(f"iterations must be an integer >= 1, not {iterations}")
        if not float(safety) >= 1.0:
            raise ValueError(f"safety must be >= 1, not {safety}")
        ref = self.density
        v = torch.randn(ref.shape, dtype=torch.float32, generator=generator,
                        device=ref.device if generator is None else generator.device).to(ref.device)
        v /= v.norm()
        quotients, leaf = [], self._leaf_like_density()
        for _ in range(int(iterations)):
            leaf.data = v
            _, w = self._data_gradient(leaf, None, pose_args, kwargs)
            quotients.append((v * w).sum())
            v = w / w.norm()
        self.lipschitz_history = [float(q) for q in torch.stack(quotients).tolist()]
        return float(safety) * self.lipschitz_history[-1]

    def make_fista(self, lipschitz, regularizer=None, weight=0.0, inner_iterations=10, warm_start=True):
        return Fista(self, lipschitz, regularizer=regularizer, weight=weight, inner_iterations=inner_iterations,
                     warm_start=warm_start)

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


class Fista:
    """FISTA (Beck & Teboulle 2009) on ``mse(A V, measured) + weight TV(V)``, ``lower <= V <= upper``: the
    proximal counterpart of ``Reconstruction.step`` with ``VolumeAdam`` -- no learning rate and no smoothing of
    the TV.  ``lipschitz``: the constant L of the data term's gradient (``Reconstruction.lipschitz``).  One step:

        g = grad f(y_k);   x_{k+1} = prox_{(weight / L) TV, C}(y_k - g / L)
        t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2;   y_{k+1} = x_{k+1} + ((t_k - 1) / t_{k+1}) (x_{k+1} - x_k)

    with ``inner_iterations`` fast-gradient-projection steps of the prox (``TotalVariation3d.prox``), its dual
    carried from step to step (``warm_start``) or started from zeros every time.  ``recon.density`` holds x_k
    after every step; ``y``, the dual and ``t`` are this object's state.  Without a regulariser (or with
    ``weight == 0``) the prox is the projection onto the box: projected FISTA.  The bounds are ``recon``'s."""

    def __init__(self, recon, lipschitz, regularizer=None, weight=0.0, inner_iterations=10, warm_start=True):
        if not 0.0 < float(lipschitz) < float("inf"):
            raise ValueError(f"lipschitz must be > 0 and finite, not {lipschitz}")
        if not 0.0 <= float(weight) < float("inf"):
            raise ValueError(f"weight must be >= 0 and finite, not {weight}")
        if int(inner_iterations) != inner_iterations or inner_iterations < 0:
            raise ValueError(f"inner_iterations must be an integer >= 0, not {inner_iterations}")
        if regularizer is not None and not isinstance(regularizer, TotalVariation3d):
            raise ValueError("regularizer must be a TotalVariation3d (or None)")
        self.recon = recon
        self.lipschitz = float(lipschitz)
        self.regularizer = regularizer if float(weight) > 0.0 else None
        self.weight = float(weight)
        self.inner_iterations = int(inner_iterations)
        self.warm_start = bool(warm_start)
        self.restart()

    @torch.no_grad()
    def restart(self):
        """Back to the state of a new object at the current ``recon.density``: t = 1, y = x, a zero dual."""
        self.t = 1.0
        self.y = self.recon.density.detach().clone()
        self.dual = None
        self._leaf = self.recon._leaf_like_density()

    @torch.no_grad()
    def step(self, measured, *pose_args, **kwargs):
        """One outer step -> (data loss at y_k, TV(x_{k+1})), 0-dim device tensors (the TV unweighted and
        without smoothing; zero without a regulariser).  Nothing synchronises with the host."""
        recon, tv = self.recon, self.regularizer
        self._leaf.data = self.y
        loss, g = recon._data_gradient(self._leaf, measured, pose_args, kwargs)
        g = g.contiguous()
        torch.add(self.y, g, alpha=-1.0 / self.lipschitz, out=g)  # b = y - g / L, in the gradient's buffer
        t_next = _next_t(self.t)
        beta = (self.t - 1.0) / t_next
        x_prev = recon.density.data
        if tv is None:
            x = _box(g, recon.lower, recon.upper)
            y = torch.add(x, x - x_prev, alpha=beta)
            value = torch.zeros((), dtype=loss.dtype, device=loss.device)
        else:
            if self.dual is None:
                self.dual = g.new_zeros((3, *g.shape))
            elif not self.warm_start:
                self.dual.zero_()
            x, y, _ = tv._prox(g, self.weight / self.lipschitz, self.inner_iterations, recon.lower, recon.upper,
                               self.dual, x_prev=x_prev, beta=beta)
            if _fused_volume(x):
                value = ops.tv3d(x, tv.spacing, tv.mode, 0.0)
            else:
                value = total_variation_3d(x, tv.spacing, tv.mode, 0.0)
        recon.density.data = x
        self.y, self.t = y, t_next
        return loss, value
