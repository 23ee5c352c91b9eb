"""2D/3D registration module (reference ``diffdrr/registration.py:14-50``):
learnable pose parameters in front of a ``DRR``.  ``PoseRegressor`` (a CNN) is
out of scope."""
from __future__ import annotations

import torch
import torch.nn as nn

from .pose import convert
from .renderers import _euler_siddon_render


class Registration(nn.Module):
    def __init__(self, drr, rotation: torch.Tensor, translation: torch.Tensor,
                 parameterization: str, convention: str | None = None):
        super().__init__()
        self.drr = drr
        self._rotation = nn.Parameter(rotation)
        self._translation = nn.Parameter(translation)
        self.parameterization = parameterization
        self.convention = convention

    def forward(self, **kwargs):
        # (same result as the reference's `self.drr(self.pose, **kwargs)`; handing the raw
        # parameters over lets DRR take its fused pose -> rays path for Euler angles)
        return self.drr(self._rotation, self._translation,
                        parameterization=self.parameterization, convention=self.convention,
                        **kwargs)

    @property
    def pose(self):
        return convert(self._rotation, self._translation,
                       parameterization=self.parameterization, convention=self.convention)

    @property
    def rotation(self):
        return self._rotation

    @property
    def translation(self):
        return self._translation


class PoseAdam(torch.optim.Optimizer):
    """``torch.optim.Adam([{"params": [rotation], "lr": lr_rotation}, {"params": [translation],
    "lr": lr_translation}], betas=betas, eps=eps, maximize=maximize)`` -- the optimizer of the
    reference's registration loop (``notebooks/tutorials/registration.ipynb:240-316``) -- with the
    step of both groups in ONE launch (``ddrr_pose_adam_step``): torch's fused / capturable Adam
    takes four (a step-counter and an update launch per group), ~19 us of a 0.19 ms iteration at
    512^3 -> 256^2.  Same update rule (no weight decay, no amsgrad), same state layout
    (``state[p] = {"step", "exp_avg", "exp_avg_sq"}``, the counters on the device: safe to capture
    in a HIP graph), same param groups (learning rates may be changed between EAGER steps through
    ``param_groups``; they are host numbers handed to the kernel as arguments, so a captured step
    keeps the values it was captured with -- ``GraphedIteration`` raises rather than replay a stale
    learning rate).  Parameters: float32 ``(B, 3)`` on the GPU."""

    def __init__(self, rotation, translation, lr_rotation, lr_translation, betas=(0.9, 0.999), eps=1e-8,
                 maximize=False):
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or eps < 0.0:
            raise ValueError("PoseAdam: invalid betas / eps")
        if lr_rotation < 0.0 or lr_translation < 0.0:
            raise ValueError("PoseAdam: negative learning rate")
        super().__init__([{"params": [rotation], "lr": lr_rotation}, {"params": [translation], "lr": lr_translation}],
                         dict(lr=lr_rotation, betas=betas, eps=eps, maximize=maximize))
        # (the state exists from the start, not from the first step: a first step inside a graph
        # capture would otherwise bake the zero-fills of its state into every replay)
        for p in (rotation, translation):
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
        from . import ops

        g_rot, g_xyz = self.param_groups
        rot, xyz = g_rot["params"][0], g_xyz["params"][0]
        if rot.grad is None or xyz.grad is None:
            raise RuntimeError("PoseAdam.step(): both pose parameters need a gradient")
        if (g_rot["betas"], g_rot["eps"], g_rot["maximize"]) != (g_xyz["betas"], g_xyz["eps"], g_xyz["maximize"]):
            raise ValueError("PoseAdam: betas, eps and maximize are shared by the two groups")
        s_rot, s_xyz = self._state(rot), self._state(xyz)
        ops.pose_adam_step(rot, xyz, rot.grad.contiguous(), xyz.grad.contiguous(), s_rot["exp_avg"],
                           s_rot["exp_avg_sq"], s_xyz["exp_avg"], s_xyz["exp_avg_sq"], s_rot["step"],
                           s_xyz["step"], lr_rot=g_rot["lr"], lr_xyz=g_xyz["lr"], betas=g_rot["betas"],
                           eps=g_rot["eps"], maximize=g_rot["maximize"])
        return loss


class GraphedIteration:
    """One registration iteration -- render, similarity, backward, optimizer step -- captured
    once as a HIP graph and replayed: the loop of reference
    ``notebooks/tutorials/registration.ipynb:240-316`` without the ~0.5 ms of Python / autograd
    / launch overhead per iteration that dwarfs its ~0.25 ms of GPU work at 512^3 -> 256^2
    (``profiles/r01/config4_registration_v2.txt``).

        step = GraphedIteration(reg, criterion, optimizer, target)
        for it in range(n):
            loss = step()          # replays the graph; `loss` is a device tensor (no sync)

    The optimizer must not synchronise in ``step()`` (``torch.optim.SGD``; Adam with
    ``capturable=True``).  Everything the iteration touches keeps its address: the parameters
    of ``reg`` and the optimizer state are updated in place, ``target`` is read in place.
    ``maximize`` / learning rates are whatever the optimizer was built with -- and FROZEN at
    capture: hyper-parameters that are Python numbers (``PoseAdam``'s and torch's ``lr``, ``betas``,
    ``eps``) are baked into the captured kernel arguments, so an ``lr_scheduler`` or a manual
    ``param_groups`` edit between replays would be ignored silently.  ``__call__`` therefore raises
    if a group's host-side hyper-parameters differ from the captured ones (build a new
    ``GraphedIteration`` after changing them; a tensor ``lr`` is read by the kernels and may change).

    Construction has no side effects on the optimisation: the ``warmup`` eager iterations and
    the capture itself (which runs the iteration once more) are undone -- parameters and
    optimizer state are restored to what they were -- so that ``step()`` number k is iteration
    k of the loop, as in the reference's.  ``iterations_done`` counts the replays.
    Limits of that undo: optimizer state created by the warm-up is ZEROED, which equals a fresh
    start for Adam and for SGD with momentum and ``dampening == 0``; with ``dampening != 0`` a
    fresh first step sets ``buf = grad`` while a zeroed buffer yields ``(1 - dampening) grad``
    (rejected below), and state that is not a tensor (Python-int step counts of non-capturable
    optimizers) is not restored.

    ``static_volume`` (default True): the CT volume is not edited in place between replays --
    the graph then renders from the volume's cached 16-bit bricks (``Siddon.brick_storage``),
    whose address and "already built" state are baked into the graph.  Pass False if the volume
    changes under the graph: the captured render then reads the live fp32 volume.

    ``fused_similarity`` (default True): with ``NormalizedCrossCorrelation2d()`` as the criterion
    and Euler pose parameters the iteration goes through ``DRR.ncc`` -- three fused launches around
    the brick kernel instead of nine -- where that applies (``self.fused_similarity`` says whether
    it was asked for; the value and the gradients are those of the criterion on the rendered
    image, up to the order of the sums).

    ``weight`` ((1 | B), 1, H, W), >= 0: the criterion's per-pixel weight (a mask of the collimator, of dead
    pixels, of instruments the CT does not hold), read in place like ``target``.  The fused route passes it to
    ``DRR.ncc``, the unfused one calls ``criterion(target, reg(), weight=weight)`` -- ``MutualInformation``
    included, which then runs its weighted kernels (include/diffdrr_wmi_hip.h) inside the captured graph."""

    def __init__(self, reg: Registration, criterion, optimizer, target: torch.Tensor,
                 warmup: int = 3, static_volume: bool = True, fused_similarity: bool = True,
                 weight: torch.Tensor = None, **render_kwargs):
        self.reg, self.criterion, self.optimizer, self.target = reg, criterion, optimizer, target
        self.weight = weight
        self.render_kwargs = render_kwargs
        self.iterations_done = 0
        for g in optimizer.param_groups:
            if g.get("momentum", 0) and g.get("dampening", 0):
                raise ValueError("GraphedIteration: SGD with momentum and dampening != 0 cannot "
                                 "be restored to a fresh first step after warm-up and capture")
        renderer = getattr(reg.drr, "renderer", None)
        had_static = getattr(renderer, "static_volume", None)
        if had_static is not None:
            renderer.static_volume = bool(static_volume)
        params = [p for g in optimizer.param_groups for p in g["params"]]
        saved_params = [p.detach().clone() for p in params]
        saved_state = {p: {k: v.detach().clone() for k, v in optimizer.state.get(p, {}).items()
                           if torch.is_tensor(v)} for p in params}

        # NCC of Euler poses: the step around the renderer as three fused launches (DRR.ncc; it
        # composes the same value from `reg()` and the criterion itself where they do not apply)
        from .metrics import NormalizedCrossCorrelation2d
        fused = (type(criterion) is NormalizedCrossCorrelation2d and criterion.patch_size is None
                 and reg.parameterization == "euler_angles" and not render_kwargs
                 and hasattr(reg.drr, "ncc") and fused_similarity)
        self.fused_similarity = bool(fused)

        # (two launches an iteration does not need: the sum of ONE value, and the ones autograd
        # fills in as the gradient of a scalar loss -- handed over ready-made)
        one = torch.ones((), dtype=reg._rotation.dtype, device=reg._rotation.device)

        def iteration():
            optimizer.zero_grad(set_to_none=True)
            if fused:
                values = reg.drr.ncc(target, reg._rotation, reg._translation, convention=reg.convention,
                                     eps=criterion.eps, weight=weight)
            elif weight is not None:
                values = criterion(target, reg(**render_kwargs), weight=weight)
            else:
                values = criterion(target, reg(**render_kwargs))
            loss = values.reshape(()) if values.numel() == 1 else values.sum()
            loss.backward(gradient=one)
            optimizer.step()
            return loss.detach()

        try:
            # warm up on a side stream (first-call costs and lazy initialisations must not be
            # captured)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(warmup):
                    iteration()
            torch.cuda.current_stream().wait_stream(side)
            self.graph = torch.cuda.CUDAGraph()
            # (the capture stream is ours, so that the fused step's zeroed workspace -- one per
            # stream -- exists before the capture: inside it, its zero-fill would become a node)
            cap = torch.cuda.Stream()
            cap.wait_stream(torch.cuda.current_stream())
            if fused or weight is not None:
                from . import ops
                from .metrics import GradientNormalizedCrossCorrelation2d
                poses, pixels = reg._rotation.shape[0], target.shape[-2] * target.shape[-1]
                with torch.cuda.stream(cap):
                    if fused:
                        ops.siddon_ncc_workspace(poses, reg._rotation.device)
                    if weight is not None:
                        # (the weighted kernels' partials, for the pairs either route launches: a pose's image, or
                        # its two Sobel channels -- inside the capture the buffer would come from the graph's pool)
                        channels = 2 if isinstance(criterion, GradientNormalizedCrossCorrelation2d) else 1
                        ops.wncc_workspace(poses * channels, pixels, reg._rotation.device)
                cap.synchronize()
            with torch.cuda.graph(self.graph, stream=cap):
                self.loss = iteration()
        finally:
            # (whatever the warm-up or the capture raised: the caller's module gets its own
            # promise back)
            if had_static is not None:
                renderer.static_volume = had_static
        # undo warm-up and capture: same parameter values, same optimizer state, IN PLACE (the
        # graph holds the addresses of both).  State the warm-up created is zeroed, which is what
        # a first step starts from (Adam's moments and step count, SGD's momentum buffer).
        with torch.no_grad():
            for p, v in zip(params, saved_params):
                p.copy_(v)
                p.grad = None
                for name, val in optimizer.state.get(p, {}).items():
                    if torch.is_tensor(val):
                        old = saved_state[p].get(name)
                        val.copy_(old) if old is not None else val.zero_()

        self._captured_hyper = self._host_hyper()

    def _host_hyper(self):
        """The param groups' hyper-parameters that live on the host (baked into the graph)."""
        return [tuple(sorted((k, v) for k, v in g.items()
                             if k != "params" and isinstance(v, (bool, int, float, tuple, type(None)))))
                for g in self.optimizer.param_groups]

    def __call__(self) -> torch.Tensor:
        if self._host_hyper() != self._captured_hyper:
            raise RuntimeError(
                "GraphedIteration: the optimizer's hyper-parameters changed after capture "
                f"({self._captured_hyper} -> {self._host_hyper()}); they are baked into the graph -- "
                "build a new GraphedIteration (or use tensor-valued learning rates)")
        self.graph.replay()
        self.iterations_done += 1
        return self.loss


def normal_equations_reference(J: torch.Tensor, x: torch.Tensor, f: torch.Tensor, eps: float = 1e-5):
    """The definition of what a Levenberg-Marquardt step solves, in float64 torch: with the residual
    ``r = z(x) - z(f)``, ``z(v) = (v - mean v) / sqrt(var v + eps)`` (biased variance, as
    ``NormalizedCrossCorrelation2d``) and ``J = dx / dtheta`` ((..., N, 6); ``x``, ``f`` (..., N))
    -> ``(ncc, A, g)`` = (mean z(x) z(f), J_r^T J_r with the exact J_r = dz(x) / dtheta, J_r^T r), shapes
    (...), (..., 6, 6), (..., 6).  ``1/2 |r|^2 = N (1 - ncc)`` up to ``eps``.  ``ddrr_lm_step`` forms the
    same three from 44 sums (include/diffdrr_lm_hip.h); this function is the yardstick of its tests."""
    J, x, f = J.double(), x.double(), f.double()
    N = x.shape[-1]
    mx, mf = x.mean(-1, keepdim=True), f.mean(-1, keepdim=True)
    vx, vf = ((x - mx) ** 2).mean(-1, keepdim=True), ((f - mf) ** 2).mean(-1, keepdim=True)
    sx, sf = (vx + eps).sqrt(), (vf + eps).sqrt()
    zx, zf = (x - mx) / sx, (f - mf) / sf
    # dz_n / dtheta = (J_n - mean J) / s_x - z_n (z^T J) / (N s_x)
    Jc = J - J.mean(-2, keepdim=True)
    zJ = (zx.unsqueeze(-1) * J).sum(-2, keepdim=True)
    Jr = Jc / sx.unsqueeze(-1) - zx.unsqueeze(-1) * zJ / (N * sx.unsqueeze(-1))
    r = zx - zf
    return (zx * zf).mean(-1), Jr.transpose(-1, -2) @ Jr, (Jr * r.unsqueeze(-1)).sum(-2)


def weighted_normal_equations_reference(J: torch.Tensor, x: torch.Tensor, f: torch.Tensor, w: torch.Tensor,
                                        eps: float = 1e-5):
    """:func:`normal_equations_reference` under per-pixel weights ``w`` ((..., N), >= 0), in float64 torch: with
    ``Sw = sum w``, the weighted mean and the weighted biased variance in ``z_w(v) = (v - mean_w v) /
    sqrt(var_w v + eps)``, and the residual ``r = sqrt(w) (z_w(x) - z_w(f))`` -> ``(ncc, A, g, Sw)`` = (sum w z_w(x)
    z_w(f) / Sw, J_r^T J_r with the exact J_r = dr / dtheta, J_r^T r, sum w).  ``1/2 |r|^2 = Sw (1 - ncc)`` up to
    ``eps``.  Pixels of weight 0 are selected out (``torch.where``), not multiplied: ``x`` and ``f`` may hold NaN
    or Inf there.  With ``w = 1`` it returns what the unweighted reference returns; a pose with ``Sw = 0`` gets
    ncc 0, A 0, g 0.  ``ddrr_wlm_step`` forms the same from 45 sums (include/diffdrr_wlm_hip.h); this function is
    the yardstick of its tests."""
    J, x, f, w = J.double(), x.double(), f.double(), w.double()
    on = w != 0
    zero = torch.zeros_like(x)
    x, f = torch.where(on, x, zero), torch.where(on, f, zero)
    J = torch.where(on.unsqueeze(-1), J, torch.zeros_like(J))
    Sw = w.sum(-1, keepdim=True)
    some = Sw > 0
    n = torch.where(some, Sw, torch.ones_like(Sw))
    mx, mf = (w * x).sum(-1, keepdim=True) / n, (w * f).sum(-1, keepdim=True) / n
    vx, vf = (w * (x - mx) ** 2).sum(-1, keepdim=True) / n, (w * (f - mf) ** 2).sum(-1, keepdim=True) / n
    sx, sf = (vx + eps).sqrt(), (vf + eps).sqrt()
    zx, zf = torch.where(on, (x - mx) / sx, zero), torch.where(on, (f - mf) / sf, zero)
    # dz_n / dtheta = (J_n - mean_w J) / s_x - z_n (sum w z J) / (Sw s_x); a row of r carries sqrt(w_n)
    wJ = w.unsqueeze(-1) * J
    Jc = J - wJ.sum(-2, keepdim=True) / n.unsqueeze(-1)
    zJ = (zx.unsqueeze(-1) * wJ).sum(-2, keepdim=True)
    Jz = Jc / sx.unsqueeze(-1) - zx.unsqueeze(-1) * zJ / (n * sx).unsqueeze(-1)
    Jz = torch.where(on.unsqueeze(-1), Jz, torch.zeros_like(Jz))
    r = zx - zf
    A = (w.unsqueeze(-1) * Jz).transpose(-1, -2) @ Jz
    g = (w.unsqueeze(-1) * Jz * r.unsqueeze(-1)).sum(-2)
    ncc = (w * zx * zf).sum(-1) / n.squeeze(-1)
    keep = some.squeeze(-1)
    return (torch.where(keep, ncc, torch.zeros_like(ncc)), torch.where(keep[..., None, None], A, torch.zeros_like(A)),
            torch.where(keep[..., None], g, torch.zeros_like(g)), Sw.squeeze(-1))


class LevenbergMarquardt:
    """Levenberg-Marquardt on the least-squares form of the global NCC, ``1/2 |z(drr) - z(fixed)|^2``,
    for the Euler pose parameters of ``reg`` -- the second-order counterpart of the reference's
    first-order loop (``notebooks/tutorials/registration.ipynb:240-316``): no learning rates, tens of
    renders instead of hundreds.

        lm = LevenbergMarquardt(reg, fixed)
        for _ in range(30):
            ncc = lm.step()        # (B,) best NCC so far per pose, a device tensor (no sync)
        lm.commit()                # the best poses -> reg's parameters

    ``step()`` is four launches and no host synchronisation: ``ddrr_pose_raygen_forward`` with the
    clears, the brick kernel with its record and no image, ``ddrr_lm_normal_sums`` (the 6 x 6 normal
    equations from the record, include/diffdrr_lm_hip.h) and ``ddrr_lm_step`` (accept / reject against the
    best pose so far, damped solve, next trial).  Every render is a trial: BETWEEN steps ``reg``'s
    parameters hold the next trial pose, not the best one -- ``commit()`` writes the best.  Several poses
    are independent multi-starts, each with its own damping (``damping``, a read-only (B,) view).

    Domain: that of ``DRR._render_euler_differentiable`` in radians -- Euler angles, a dense Siddon render
    on the bricks of a volume that takes no gradient, float32 (B, 3) parameters on the volume's device, at
    most ``DRR.FUSED_NCC_MAX_POSES`` poses; ``fixed`` ((1 | B), 1, H, W) float32.  Anything else raises
    ``ValueError`` naming the condition.

    ``weight`` ((1 | B), 1, H, W) float32 on the parameters' device, finite and >= 0 (checked once, here; then
    read in place at every step, as ``fixed`` is): the weighted (masked) problem of include/diffdrr_wlm_hip.h
    -- the residual ``sqrt(w) (z_w(drr) - z_w(fixed))`` with the weighted mean and variance, the objective of
    ``DRR.ncc(..., weight=)``.  Pixels of weight 0 (collimator, dead pixels, instruments) are selected out of every
    sum: ``fixed`` may hold anything there.  ``step()`` is the same four launches with ``ddrr_wlm_normal_sums``
    and ``ddrr_wlm_step`` in place of the two ``ddrr_lm_*`` entries, and returns the best weighted NCC;
    ``weight_sum`` is the sum of the weights of the last render per pose.  A pose whose weights are all 0 never
    moves and reports NCC 0.  Editing the weight between steps makes "best so far" compare different objectives:
    build a new object instead.  Without ``weight`` nothing changes: the unweighted kernels run.

    ``graph=True`` (the step captured as one HIP graph, as ``GraphedIteration`` captures its iteration) is
    not built: it raises ``NotImplementedError``.  Nothing in a step stands in its way -- no launch depends
    on data, nothing is read back -- but the render's record is summed with float atomics, so a captured
    step cannot be pinned bit for bit to the eager one, and it has not been run on a device."""

    def __init__(self, reg: Registration, fixed: torch.Tensor, damping: float = 1.0, up: float = 4.0,
                 down: float = 1.0 / 3.0, damping_min: float = 1e-7, damping_max: float = 1e6, eps: float = 1e-5,
                 graph: bool = False, weight: torch.Tensor | None = None):
        from . import ops
        from .pose import _check_convention
        from .renderers import Siddon

        if graph:
            raise NotImplementedError("LevenbergMarquardt: graph=True (the step as one captured HIP graph) is not "
                                      "built; run the eager step, which does not synchronise with the host either")
        self.reg = reg
        self.up, self.down, self.damping_min, self.damping_max, self.eps = (
            float(up), float(down), float(damping_min), float(damping_max), float(eps))
        if not (self.up > 1.0 and 0.0 < self.down < 1.0 and 0.0 < self.damping_min <= self.damping_max < float("inf")
                and self.damping_min <= float(damping) <= self.damping_max and self.eps >= 0.0):
            raise ValueError("LevenbergMarquardt: up > 1, 0 < down < 1, 0 < damping_min <= damping <= damping_max "
                             "< inf and eps >= 0 expected")
        drr = reg.drr
        r, det = getattr(drr, "renderer", None), getattr(drr, "detector", None)
        rot, xyz = reg._rotation, reg._translation

        def refuse(what):
            raise ValueError(f"LevenbergMarquardt: {what}")

        if reg.parameterization != "euler_angles":
            refuse(f"parameterization must be 'euler_angles', not {reg.parameterization!r}")
        _check_convention(reg.convention)
        if not isinstance(r, Siddon):
            refuse("the renderer must be Siddon")
        if r.grid_path != "bricks":
            refuse("the Siddon renderer must take the brick kernel (grid_path == 'bricks')")
        if r.packed_record:
            refuse("the packed backward record (packed_record=True) is not read; use the float record")
        if drr.density.requires_grad:
            refuse("the volume must not require a gradient")
        if drr.patch_size is not None:
            refuse("patch_size must be None")
        if det.n_subsample is not None:
            refuse("p_subsample must be None (a dense detector)")
        if not drr.fuse_ray_generation:
            refuse("fuse_ray_generation must be on")
        for name, t in (("rotation", rot), ("translation", xyz)):
            if t.dim() != 2 or t.shape[1] != 3 or t.dtype != torch.float32 or not t.is_contiguous():
                refuse(f"{name} must be a contiguous float32 (B, 3) parameter, got {tuple(t.shape)} {t.dtype}")
            if t.device != drr.density.device or not ops.on_device(t):
                refuse(f"{name} must live on the volume's device ({drr.density.device}), got {t.device}")
        B = rot.shape[0]
        if rot.shape != xyz.shape:
            refuse(f"rotation {tuple(rot.shape)} and translation {tuple(xyz.shape)} must have one shape")
        if not 0 < B <= drr.FUSED_NCC_MAX_POSES:
            refuse(f"1 ... {drr.FUSED_NCC_MAX_POSES} poses expected, got {B}")
        H, W = det.height, det.width
        if not (torch.is_tensor(fixed) and fixed.dim() == 4 and fixed.shape[0] in (1, B)
                and tuple(fixed.shape[1:]) == (1, H, W) and fixed.dtype == torch.float32):
            refuse(f"fixed must be a float32 ((1 | {B}), 1, {H}, {W}) tensor")
        if fixed.device != rot.device:
            refuse(f"fixed must live on the parameters' device ({rot.device}), got {fixed.device}")
        if weight is not None:
            if not torch.is_tensor(weight) or weight.dtype != torch.float32:
                refuse(f"weight must be a float32 tensor, got {getattr(weight, 'dtype', type(weight).__name__)}")
            if weight.dim() != 4 or weight.shape[0] not in (1, B) or tuple(weight.shape[1:]) != (1, H, W):
                refuse(f"weight must have the shape ((1 | {B}), 1, {H}, {W}), got {tuple(weight.shape)}")
            if weight.device != rot.device:
                refuse(f"weight must live on the parameters' device ({rot.device}), got {weight.device}")
            if not bool(torch.isfinite(weight).all()):
                refuse("weight must be finite (it holds NaN or Inf)")
            if bool((weight < 0).any()):
                refuse("weight must not be negative")
        self.B, self.N = B, H * W
        self.fixed = fixed.detach().reshape(fixed.shape[0], H * W).contiguous()
        # (a view where the caller's tensor is contiguous: read in place, as the fixed image is)
        self.weight = None if weight is None else weight.detach().reshape(weight.shape[0], H * W).contiguous()
        dev = rot.device
        self._state = ops.lm_state(B, damping, dev)
        self._ws = ops.lm_workspace(B, self.N, dev) if weight is None else ops.wlm_workspace(B, self.N, dev)
        self._aux = ops.brick_record_buffer(B, self.N, dev)
        self._ncc = torch.zeros(B, dtype=torch.float32, device=dev)
        self.steps_done = 0

    # -- one render of the current parameters with its record: the first two launches of a step
    def _render(self):
        drr = self.reg.drr
        rot, xyz = self.reg._rotation.detach(), self.reg._translation.detach()
        rot, reorient34, P, Ainv, axes, cfg = drr._euler_args(rot, self.reg.convention, False)
        Mw, source, _, _, aux, _ = _euler_siddon_render(rot, xyz, drr.density, reorient34, P, Ainv, axes, cfg,
                                                        aux=self._aux)
        return dict(aux=aux, source=source, Mw=Mw, Ainv=Ainv, P=P, rot=rot, xyz=xyz, axes=axes,
                    reorient34=reorient34), dict(eps=cfg["eps"], with_img_path=not cfg["stop_gradients"])

    @torch.no_grad()
    def _step(self, out):
        from . import ops

        args, kw = self._render()
        hyper = dict(ncc_eps=self.eps, up=self.up, down=self.down, damping_min=self.damping_min,
                     damping_max=self.damping_max)
        if self.weight is not None:
            ops.wlm_normal_sums(args.pop("aux"), self.fixed, self.weight, **args, **kw, ws=self._ws)
            return ops.wlm_step(self._ws, self._state, args["rot"], args["xyz"], self.N, **hyper, out=out)
        ops.lm_normal_sums(args.pop("aux"), self.fixed, **args, **kw, ws=self._ws)
        return ops.lm_step(self._ws, self._state, args["rot"], args["xyz"], self.N, ncc_eps=self.eps, up=self.up,
                           down=self.down, damping_min=self.damping_min, damping_max=self.damping_max, out=out)

    def step(self) -> torch.Tensor:
        """Render the current parameters, accept or reject them, write the next trial into them
        -> the best NCC per pose so far, (B,), detached."""
        out = self._step(None)
        self.steps_done += 1
        return out

    @torch.no_grad()
    def commit(self):
        """Copy the best pose of every start into ``reg``'s parameters (a start that has not rendered yet
        keeps its parameters)."""
        valid = self._state[:, 35:36] != 0
        best = self._state[:, :6].to(torch.float32)
        self.reg._rotation.copy_(torch.where(valid, best[:, :3], self.reg._rotation))
        self.reg._translation.copy_(torch.where(valid, best[:, 3:], self.reg._translation))

    @torch.no_grad()
    def jacobian(self) -> torch.Tensor:
        """d image / d (rot, xyz) at the current parameters, (B, N, 6) float32: one render and
        ``ddrr_lm_normal_sums`` with its per-ray output.  The optimiser's state is not touched."""
        from . import ops

        args, kw = self._render()
        return ops.lm_normal_sums(args.pop("aux"), self.fixed, **args, **kw, want_jacobian=True)[1]

    @property
    def damping(self) -> torch.Tensor:
        view = self._state[:, 34].detach()
        return view

    @property
    def best_parameters(self):
        """(rotation, translation) of the best pose of every start so far, (B, 3) float32 each (copies)."""
        best = self._state[:, :6].to(torch.float32)
        return best[:, :3], best[:, 3:]

    @property
    def best_ncc(self) -> torch.Tensor:
        return self._state[:, 6].detach()

    @property
    def weight_sum(self) -> torch.Tensor:
        """(B,) float64: the sum of the weights of the last render judged, per pose (0 before the first step,
        and always without ``weight``)."""
        return self._state[:, 37].detach()

    @property
    def accepted(self) -> torch.Tensor:
        """(B,) bool: whether the last step's render became the best pose."""
        return self._state[:, 36] != 0


# ------------------------------------------------------------------------------------------------ several views
def relative_views(poses) -> torch.Tensor:
    """The calibrated extrinsics ``E_v`` of V C-arm shots of ONE patient position (a ``RigidTransform`` of V poses,
    or a (V, 4, 4) tensor) -> ``K_v = E_0^-1 E_v``, (V, 4, 4) float64: what ``MultiViewLevenbergMarquardt`` takes as
    ``views``.  The parameters it optimises then describe view 0 (``K_0`` is the identity, exactly)."""
    E = (poses.matrix if hasattr(poses, "matrix") else poses).detach().double()
    if E.dim() != 3 or E.shape[0] < 1 or tuple(E.shape[1:]) != (4, 4):
        raise ValueError(f"relative_views: (V, 4, 4) poses with V >= 1 expected, got {tuple(E.shape)}")
    K = torch.linalg.solve(E[0], E)
    K[0] = torch.eye(4, dtype=torch.float64, device=E.device)
    return K


def view_poses(rot: torch.Tensor, xyz: torch.Tensor, views: torch.Tensor, convention: str = "ZXY"):
    """The S * V poses a multi-view registration renders, as a ``RigidTransform``: pose ``s * V + v`` is
    ``M(rot[s], xyz[s]) @ views[v]`` with ``M`` the Euler pose of ``convert(..., parameterization="euler_angles")``
    (radians), in the parameters' dtype and differentiable in torch.  ``drr(view_poses(...))`` is what a first-order
    multi-view loop renders through the matrix route, and the yardstick of the multi-view kernels' tests."""
    from .pose import RigidTransform

    M = convert(rot, xyz, parameterization="euler_angles", convention=convention).matrix  # (S, 4, 4)
    K = views.to(dtype=M.dtype, device=M.device)
    return RigidTransform(torch.einsum("sij,vjk->svik", M, K).reshape(-1, 4, 4))


def multiview_normal_equations_reference(J: torch.Tensor, x: torch.Tensor, f: torch.Tensor, eps: float = 1e-5):
    """The definition of what a multi-view Levenberg-Marquardt step solves, in float64 torch: the residual of a
    start is the stack over its views of ``z(x_v) - z(f_v)``, every view normalised on its own
    (:func:`normal_equations_reference` per view), with ``J`` (S, V, N, 6) the derivative of ``x`` (S, V, N) with
    respect to the start's six parameters and ``f`` (V, N) one fixed image per view
    -> ``(ncc, A, g, ncc_views)`` = (mean_v ncc_v (S,), sum_v A_v (S, 6, 6), sum_v g_v (S, 6), ncc_v (S, V)).
    ``ddrr_mvlm_step`` forms the same (include/diffdrr_mvlm_hip.h); this function is the yardstick of its tests."""
    ncc, A, g = normal_equations_reference(J, x, f.double().expand(x.shape), eps)
    return ncc.mean(-1), A.sum(-3), g.sum(-2), ncc


class MultiViewLevenbergMarquardt:
    """Levenberg-Marquardt for ONE set of six Euler pose parameters per start seen from several calibrated views
    (a biplane pair, a few C-arm shots of one patient position): the objective of a start is
    ``sum_v 1/2 |z(drr_v) - z(fixed_v)|^2``, every view normalised on its own, and the normal equations of the
    views are added before the step is judged and solved.  One view cannot determine the translation along its
    own viewing direction; a second one can.

        K = relative_views(extrinsics)                    # (V, 4, 4): E_0^-1 E_v, view 0 is the parameters' view
        lm = MultiViewLevenbergMarquardt(reg, fixed, K)   # fixed (V, 1, H, W), reg: S starts
        for _ in range(30):
            ncc = lm.step()                               # (S,) best mean NCC over the views so far
        lm.commit()

    View ``v`` renders the pose ``M(theta_s) @ views[v]`` (:func:`view_poses`): the existing Euler pose with
    ``(views[v] @ reorient)[:3]``, formed in float64 and rounded once, in place of the detector's reorient.
    ``step()`` is four launches and no host synchronisation -- ``ddrr_mvlm_raygen`` with the clears, the brick
    kernel with its record and no image (S * V poses), ``ddrr_mvlm_normal_sums`` and ``ddrr_mvlm_step``
    (include/diffdrr_mvlm_hip.h) -- and returns the best mean NCC per start; ``view_ncc`` (S, V) holds the NCC of
    every view of the render last judged.  ``commit``, ``damping``, ``best_parameters``, ``best_ncc`` and
    ``accepted`` are ``LevenbergMarquardt``'s, per start; ``jacobian()`` is (S, V, N, 6).

    Domain: that of ``LevenbergMarquardt``, with ``S * V <= DRR.FUSED_NCC_MAX_POSES``; ``views`` finite float
    (V, 4, 4) with the bottom row (0, 0, 0, 1) and an orthonormal rotation block; ``fixed`` float32 (V, 1, H, W) on
    the parameters' device, shared by the starts.  Anything else raises ``ValueError`` naming the condition.

    Not here: pixel weights and a detector per view -- ``WeightedMultiViewLevenbergMarquardt`` has both (this class
    takes no ``weight`` and all its views share the module's ``Detector``).  Not built: the step as a captured HIP
    graph, and a fused multi-view ``DRR.ncc`` for a first-order loop (which renders ``view_poses(...)`` through the
    matrix route)."""

    def __init__(self, reg: Registration, fixed: torch.Tensor, views: torch.Tensor, damping: float = 1.0,
                 up: float = 4.0, down: float = 1.0 / 3.0, damping_min: float = 1e-7, damping_max: float = 1e6,
                 eps: float = 1e-5):
        from . import ops
        from .pose import _check_convention
        from .renderers import Siddon

        self.reg = reg
        self.up, self.down, self.damping_min, self.damping_max, self.eps = (
            float(up), float(down), float(damping_min), float(damping_max), float(eps))
        if not (self.up > 1.0 and 0.0 < self.down < 1.0 and 0.0 < self.damping_min <= self.damping_max < float("inf")
                and self.damping_min <= float(damping) <= self.damping_max and self.eps >= 0.0):
            raise ValueError(f"{type(self).__name__}: up > 1, 0 < down < 1, 0 < damping_min <= damping <= "
                             "damping_max < inf and eps >= 0 expected")
        drr = reg.drr
        r, det = getattr(drr, "renderer", None), getattr(drr, "detector", None)
        rot, xyz = reg._rotation, reg._translation

        def refuse(what):
            raise ValueError(f"{type(self).__name__}: {what}")

        if reg.parameterization != "euler_angles":
            refuse(f"parameterization must be 'euler_angles', not {reg.parameterization!r}")
        _check_convention(reg.convention)
        if not isinstance(r, Siddon):
            refuse("the renderer must be Siddon")
        if r.grid_path != "bricks":
            refuse("the Siddon renderer must take the brick kernel (grid_path == 'bricks')")
        if r.packed_record:
            refuse("the packed backward record (packed_record=True) is not read; use the float record")
        if drr.density.requires_grad:
            refuse("the volume must not require a gradient")
        if drr.patch_size is not None:
            refuse("patch_size must be None")
        if det.n_subsample is not None:
            refuse("p_subsample must be None (a dense detector)")
        if not drr.fuse_ray_generation:
            refuse("fuse_ray_generation must be on")
        for name, t in (("rotation", rot), ("translation", xyz)):
            if t.dim() != 2 or t.shape[1] != 3 or t.dtype != torch.float32 or not t.is_contiguous():
                refuse(f"{name} must be a contiguous float32 (S, 3) parameter, got {tuple(t.shape)} {t.dtype}")
            if t.device != drr.density.device or not ops.on_device(t):
                refuse(f"{name} must live on the volume's device ({drr.density.device}), got {t.device}")
        if rot.shape != xyz.shape:
            refuse(f"rotation {tuple(rot.shape)} and translation {tuple(xyz.shape)} must have one shape")
        S = rot.shape[0]
        if not (torch.is_tensor(views) and views.is_floating_point() and views.dim() == 3 and views.shape[0] >= 1
                and tuple(views.shape[1:]) == (4, 4)):
            refuse(f"views must be a float (V, 4, 4) tensor with V >= 1, got "
                   f"{tuple(views.shape) if torch.is_tensor(views) else type(views).__name__} "
                   f"{getattr(views, 'dtype', '')}")
        K = views.detach().to(device=rot.device, dtype=torch.float64)
        if not bool(torch.isfinite(K).all()):
            refuse("views must be finite (they hold NaN or Inf)")
        if not bool((K[:, 3] == torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64, device=K.device)).all()):
            refuse("views must be rigid: the bottom row of every matrix must be (0, 0, 0, 1)")
        R = K[:, :3, :3]
        tol = 1e-5 if views.dtype == torch.float32 else 1e-9
        if float((R @ R.mT - torch.eye(3, dtype=torch.float64, device=K.device)).abs().max()) > tol \
                or bool((torch.linalg.det(R) < 0).any()):
            refuse(f"views must be rigid: the rotation block of every matrix must be orthonormal (to {tol:g}) with "
                   "determinant +1")
        V = K.shape[0]
        if not 0 < S * V <= drr.FUSED_NCC_MAX_POSES:
            refuse(f"1 ... {drr.FUSED_NCC_MAX_POSES} rendered poses (starts x views) expected, got {S} x {V}")
        H, W = det.height, det.width
        if not (torch.is_tensor(fixed) and fixed.dim() == 4 and tuple(fixed.shape) == (V, 1, H, W)
                and fixed.dtype == torch.float32):
            refuse(f"fixed must be a float32 ({V}, 1, {H}, {W}) tensor, one image per view")
        if fixed.device != rot.device:
            refuse(f"fixed must live on the parameters' device ({rot.device}), got {fixed.device}")
        self.S, self.V, self.N = S, V, H * W
        self.views = K
        # Ro_v = (K_v @ reorient)[:3], in float64, rounded once
        self._reorient_v = (K @ det._reorient.detach().to(K))[:, :3, :].to(torch.float32).contiguous()
        self.fixed = fixed.detach().reshape(V, H * W).contiguous()
        dev = rot.device
        self._state = ops.lm_state(S, damping, dev)
        self._ws = self._workspace(dev)
        self._aux = ops.brick_record_buffer(S * V, self.N, dev)
        self._view_ncc = torch.zeros(S, V, dtype=torch.float32, device=dev)
        self.steps_done = 0

    def _workspace(self, device):
        """the per-workgroup partial sums of a step (WeightedMultiViewLevenbergMarquardt has its own)"""
        from . import ops

        return ops.mvlm_workspace(self.S, self.V, self.N, device)

    # -- one render of the current parameters from every view with its record: the first two launches of a step
    def _render(self):
        from . import ops
        from .renderers import _brick_axis, _brick_storage

        drr = self.reg.drr
        rot, xyz = self.reg._rotation.detach(), self.reg._translation.detach()
        rot, _, P, Ainv, axes, cfg = drr._euler_args(rot, self.reg.convention, False)
        B, volume = self.S * self.V, drr.density
        launch_ws = ops.launch_workspace(volume.shape, volume.device)
        Mw, source, target, img = ops.mvlm_raygen(rot, xyz, axes, self._reorient_v, Ainv, P, clear=self._aux,
                                                  clear_launch_ws=launch_ws)
        ops.siddon_forward_bricks(
            volume, source, target, img, cfg["det"], voxel_shift=cfg["voxel_shift"], eps=cfg["eps"], want_aux=True,
            storage=_brick_storage(volume, cfg, B), axis=_brick_axis(volume, cfg, B), want_image=False, aux=self._aux,
            launch_ws=launch_ws, cleared=True)
        return dict(aux=self._aux, source=source, Mw=Mw, Ainv=Ainv, P=P, rot=rot, xyz=xyz, axes=axes,
                    reorient_v=self._reorient_v), dict(eps=cfg["eps"], with_img_path=not cfg["stop_gradients"])

    @torch.no_grad()
    def step(self) -> torch.Tensor:
        """Render the current parameters from every view, accept or reject them, write the next trial into them
        -> the best mean NCC per start so far, (S,), detached."""
        from . import ops

        args, kw = self._render()
        ops.mvlm_normal_sums(args.pop("aux"), self.fixed, **args, **kw, ws=self._ws)
        out = ops.mvlm_step(self._ws, self._state, args["rot"], args["xyz"], self.V, self.N, ncc_eps=self.eps,
                            up=self.up, down=self.down, damping_min=self.damping_min, damping_max=self.damping_max,
                            ncc_views=self._view_ncc)
        self.steps_done += 1
        return out

    @torch.no_grad()
    def commit(self):
        """Copy the best parameters of every start into ``reg``'s (a start that has not rendered yet keeps its
        parameters)."""
        valid = self._state[:, 35:36] != 0
        best = self._state[:, :6].to(torch.float32)
        self.reg._rotation.copy_(torch.where(valid, best[:, :3], self.reg._rotation))
        self.reg._translation.copy_(torch.where(valid, best[:, 3:], self.reg._translation))

    @torch.no_grad()
    def jacobian(self) -> torch.Tensor:
        """d image_v / d (rot, xyz) at the current parameters, (S, V, N, 6) float32: one render and
        ``ddrr_mvlm_normal_sums`` with its per-ray output.  The optimiser's state is not touched."""
        from . import ops

        args, kw = self._render()
        jac = ops.mvlm_normal_sums(args.pop("aux"), self.fixed, **args, **kw, want_jacobian=True)[1]
        return jac.view(self.S, self.V, self.N, 6)

    @property
    def damping(self) -> torch.Tensor:
        return self._state[:, 34].detach()

    @property
    def best_parameters(self):
        """(rotation, translation) of the best parameters of every start so far, (S, 3) float32 each (copies)."""
        best = self._state[:, :6].to(torch.float32)
        return best[:, :3], best[:, 3:]

    @property
    def best_ncc(self) -> torch.Tensor:
        """(S,) float64: the best mean NCC over the views of every start so far."""
        return self._state[:, 6].detach()

    @property
    def accepted(self) -> torch.Tensor:
        """(S,) bool: whether the last step's render became the best of its start."""
        return self._state[:, 36] != 0

    @property
    def view_ncc(self) -> torch.Tensor:
        """(S, V) float32: the NCC of every view of the render last judged, accepted or not (0 before the first
        step)."""
        return self._view_ncc.detach()


# ------------------------------------------------------------------------- several views, weights, detectors
def weighted_multiview_normal_equations_reference(J: torch.Tensor, x: torch.Tensor, f: torch.Tensor,
                                                  w: torch.Tensor, eps: float = 1e-5):
    """The definition of what a weighted multi-view Levenberg-Marquardt step solves, in float64 torch: the residual
    of a start is the stack over its views of ``sqrt(w_v) (z_w(x_v) - z_w(f_v))``, every view the weighted problem of
    :func:`weighted_normal_equations_reference` on its own, with ``J`` (S, V, N, 6) the derivative of ``x``
    (S, V, N) with respect to the start's six parameters, ``f`` (V, N) one fixed image per view and ``w``
    ((1 | V), N) one weight shared by the views or one per view
    -> ``(ncc, A, g, ncc_views, sw_views)`` = ((S,), sum_v A_v (S, 6, 6), sum_v g_v (S, 6), ncc_v (S, V),
    Sw_v (S, V)).  A view with ``Sw_v = 0`` is skipped (ncc_v 0, adds nothing).  The judged ``ncc`` is the mean of the
    non-empty views' ncc_v weighted by Sw_v -- ``sum_v Sw_v (1 - ncc_v)`` is the objective, ``1/2 |r|^2`` up to
    ``eps`` -- taken as ``sum_v (Sw_v ncc_v) / sum_v Sw_v`` over the non-empty views in ascending v; with exactly one
    non-empty view it is that view's ncc_v itself, with none 0.  Scaling one view's weight by c makes that view count
    c times; scaling every view's by c scales A and g by c and changes neither ncc nor the step.
    ``ddrr_wmvlm_step`` forms the same (include/diffdrr_wmvlm_hip.h); this function is the yardstick of its tests."""
    x = x.double()
    ncc_v, A_v, g_v, sw_v = weighted_normal_equations_reference(J, x, f.double().expand(x.shape),
                                                                w.double().expand(x.shape), eps)
    S, V = ncc_v.shape
    ncc = torch.zeros(S, dtype=torch.float64, device=x.device)
    A = torch.zeros(S, 6, 6, dtype=torch.float64, device=x.device)
    g = torch.zeros(S, 6, dtype=torch.float64, device=x.device)
    for s in range(S):  # (in the order of the kernel: the first non-empty view initialises)
        some = [v for v in range(V) if float(sw_v[s, v]) > 0]
        if not some:
            continue
        C, Sw = sw_v[s, some[0]] * ncc_v[s, some[0]], sw_v[s, some[0]]
        A[s], g[s] = A_v[s, some[0]], g_v[s, some[0]]
        for v in some[1:]:
            C, Sw = C + sw_v[s, v] * ncc_v[s, v], Sw + sw_v[s, v]
            A[s], g[s] = A[s] + A_v[s, v], g[s] + g_v[s, v]
        ncc[s] = ncc_v[s, some[0]] if len(some) == 1 else C / Sw
    return ncc, A, g, ncc_v, sw_v


class WeightedMultiViewLevenbergMarquardt(MultiViewLevenbergMarquardt):
    """``MultiViewLevenbergMarquardt`` with a pixel weight and a detector per view: what a real biplane acquisition
    needs at once -- every plane has its own collimator border and its own instruments in view, and frontal and
    lateral planes rarely share source-detector distance, pixel pitch or principal point.

        lm = WeightedMultiViewLevenbergMarquardt(reg, fixed, K, weight=w, detectors=(None, lateral))
        for _ in range(30):
            ncc = lm.step()          # (S,) best weighted NCC over the views so far
        lm.commit()

    The objective of a start is ``sum_v 1/2 sum_n w_vn (z_w(drr_v)_n - z_w(fixed_v)_n)^2 = sum_v Sw_v (1 - ncc_v)``
    up to ``eps``: per view the weighted problem of ``LevenbergMarquardt(weight=)``, the residuals stacked.  A pixel
    of weight 1 counts the same in every view; scaling ONE view's weight by c makes that view count c times (a
    per-view confidence); scaling all views' by c changes nothing.  The NCC that is judged, returned and kept as
    ``best_ncc`` is the mean of the views' NCC weighted by their sums of weights, the objective the step minimises
    (not the plain mean).  A view whose weights are all 0 is skipped; a start all of whose views are empty never
    moves and reports 0.

    ``weight``: float32 ((1 | V), 1, H, W) on the parameters' device, finite and >= 0 (checked once, here; then read
    in place at every step, as ``fixed`` is); one image shared by the views, or one per view; ``None``: ones, shared.
    Pixels of weight 0 are selected out of every sum: ``fixed`` may hold anything there.  Editing the weight between
    steps makes "best so far" compare different objectives: build a new object instead.

    ``detectors``: ``None``, or a sequence of V entries, each a ``Detector`` or ``None`` (the module's own).  Every
    detector must have the module's ``height x width`` and no ``n_subsample``; view v then renders the calibrated
    points ``det_v.calibration(det_v.full_target())[0]`` with ``(views[v] @ det_v._reorient)[:3]``.  ``None`` for
    all views keeps one set of points for all of them.

    ``step()`` is four launches and no host synchronisation: ``ddrr_wmvlm_raygen`` with the clears, the brick kernel
    with its record and no image (S * V poses), ``ddrr_wmvlm_normal_sums`` and ``ddrr_wmvlm_step``
    (include/diffdrr_wmvlm_hip.h).  ``view_ncc`` (S, V) and ``view_weight_sum`` (S, V) float64 hold the NCC and the
    sum of weights of every view of the render last judged, ``weight_sum`` (S,) their sum over the views;
    ``commit``, ``damping``, ``best_parameters``, ``best_ncc``, ``accepted`` and ``jacobian()`` ((S, V, N, 6)) are
    the parent's.  Domain and refusals: the parent's.

    Not built: weights per start (one weight image per view serves all starts), the step as a captured HIP graph,
    and a fused multi-view ``DRR.ncc`` for a first-order loop."""

    def __init__(self, reg: Registration, fixed: torch.Tensor, views: torch.Tensor,
                 weight: torch.Tensor | None = None, detectors=None, damping: float = 1.0, up: float = 4.0,
                 down: float = 1.0 / 3.0, damping_min: float = 1e-7, damping_max: float = 1e6, eps: float = 1e-5):
        from .detector import Detector

        super().__init__(reg, fixed, views, damping=damping, up=up, down=down, damping_min=damping_min,
                         damping_max=damping_max, eps=eps)
        V, N = self.V, self.N
        det = reg.drr.detector
        H, W = det.height, det.width
        dev = reg._rotation.device

        def refuse(what):
            raise ValueError(f"WeightedMultiViewLevenbergMarquardt: {what}")

        if weight is None:
            weight = torch.ones(1, 1, H, W, dtype=torch.float32, device=dev)
        if not torch.is_tensor(weight) or weight.dtype != torch.float32:
            refuse(f"weight must be a float32 tensor, got {getattr(weight, 'dtype', type(weight).__name__)}")
        if weight.dim() != 4 or weight.shape[0] not in (1, V) or tuple(weight.shape[1:]) != (1, H, W):
            refuse(f"weight must have the shape ((1 | {V}), 1, {H}, {W}), got {tuple(weight.shape)}")
        if weight.device != dev:
            refuse(f"weight must live on the parameters' device ({dev}), got {weight.device}")
        if not bool(torch.isfinite(weight).all()):
            refuse("weight must be finite (it holds NaN or Inf)")
        if bool((weight < 0).any()):
            refuse("weight must not be negative")
        # (a view where the caller's tensor is contiguous: read in place, as the fixed image is)
        self.weight = weight.detach().reshape(weight.shape[0], N).contiguous()
        self._P = None  # (None: the module's own calibrated points, one set for all views)
        if detectors is not None:
            if isinstance(detectors, (Detector, torch.Tensor, str)) or not hasattr(detectors, "__len__") \
                    or len(detectors) != V:
                refuse(f"detectors must be a sequence of {V} entries (one per view), each a Detector or None")
            dets = [det if d is None else d for d in detectors]
            for v, d in enumerate(dets):
                if not isinstance(d, Detector):
                    refuse(f"detectors[{v}] must be a Detector or None, got {type(d).__name__}")
                if (d.height, d.width) != (H, W):
                    refuse(f"detectors[{v}] must have the module's height x width ({H} x {W}), got "
                           f"{d.height} x {d.width}")
                if d.n_subsample is not None:
                    refuse(f"detectors[{v}] must be dense (n_subsample must be None)")
            if any(d is not det for d in dets):
                with torch.no_grad():
                    self._P = torch.stack([d.calibration(d.full_target())[0].detach().to(dev, torch.float32)
                                           for d in dets]).contiguous()
                    Ro = torch.stack([self.views[v] @ d._reorient.detach().to(self.views) for v, d in enumerate(dets)])
                    self._reorient_v = Ro[:, :3, :].to(torch.float32).contiguous()
        self._view_sw = torch.zeros(self.S, V, dtype=torch.float64, device=dev)

    def _workspace(self, device):
        from . import ops

        return ops.wmvlm_workspace(self.S, self.V, self.N, device)

    def _render(self):
        from . import ops
        from .renderers import _brick_axis, _brick_storage

        drr = self.reg.drr
        rot, xyz = self.reg._rotation.detach(), self.reg._translation.detach()
        rot, _, P, Ainv, axes, cfg = drr._euler_args(rot, self.reg.convention, False)
        if self._P is not None:
            P = self._P
        B, volume = self.S * self.V, drr.density
        launch_ws = ops.launch_workspace(volume.shape, volume.device)
        Mw, source, target, img = ops.wmvlm_raygen(rot, xyz, axes, self._reorient_v, Ainv, P, clear=self._aux,
                                                   clear_launch_ws=launch_ws)
        ops.siddon_forward_bricks(
            volume, source, target, img, cfg["det"], voxel_shift=cfg["voxel_shift"], eps=cfg["eps"], want_aux=True,
            storage=_brick_storage(volume, cfg, B), axis=_brick_axis(volume, cfg, B), want_image=False, aux=self._aux,
            launch_ws=launch_ws, cleared=True)
        return dict(aux=self._aux, source=source, Mw=Mw, Ainv=Ainv, P=P, rot=rot, xyz=xyz, axes=axes,
                    reorient_v=self._reorient_v), dict(eps=cfg["eps"], with_img_path=not cfg["stop_gradients"])

    @torch.no_grad()
    def step(self) -> torch.Tensor:
        """Render the current parameters from every view, accept or reject them, write the next trial into them
        -> the best NCC (the views' weighted by their sums of weights) per start so far, (S,), detached."""
        from . import ops

        args, kw = self._render()
        ops.wmvlm_normal_sums(args.pop("aux"), self.fixed, self.weight, **args, **kw, ws=self._ws)
        out = ops.wmvlm_step(self._ws, self._state, args["rot"], args["xyz"], self.V, self.N, ncc_eps=self.eps,
                             up=self.up, down=self.down, damping_min=self.damping_min, damping_max=self.damping_max,
                             ncc_views=self._view_ncc, sw_views=self._view_sw)
        self.steps_done += 1
        return out

    @torch.no_grad()
    def jacobian(self) -> torch.Tensor:
        """d image_v / d (rot, xyz) at the current parameters, (S, V, N, 6) float32, for every pixel whatever its
        weight: one render and ``ddrr_wmvlm_normal_sums`` with its per-ray output.  The optimiser's state is not
        touched."""
        from . import ops

        args, kw = self._render()
        jac = ops.wmvlm_normal_sums(args.pop("aux"), self.fixed, self.weight, **args, **kw, want_jacobian=True)[1]
        return jac.view(self.S, self.V, self.N, 6)

    @property
    def view_weight_sum(self) -> torch.Tensor:
        """(S, V) float64: the sum of the weights of every view of the render last judged (0 before the first
        step)."""
        return self._view_sw.detach()

    @property
    def weight_sum(self) -> torch.Tensor:
        """(S,) float64: the sum of the weights over the views of the render last judged (0 before the first
        step)."""
        return self._state[:, 37].detach()
