"""What tests/test_euler_routes.py (host emulation) and tests/test_gpu_euler_routes.py (MI355X) share: the fused
Euler-pose routes of ``DRR`` and ``LevenbergMarquardt`` -- which C entries each launches, in order, where each route
ends (one case per condition of its domain, that condition alone flipped) and that whatever route a call takes, it
computes what the composition computes.

The routes, by what they launch:
    inference   drr(rot, xyz, parameterization="euler_angles"), nothing to differentiate   DRR._render_euler_inference
    image       the same call with pose parameters that take a gradient                 DRR._render_euler_differentiable
    ncc / wncc  DRR.ncc(fixed, rot, xyz[, weight=]) with pose parameters that take a gradient
    lm          LevenbergMarquardt.step()
    composed    none of them: euler_world_pose + render_poses (or Detector + render), the criterion on the image

The composition of a case is the case's own module with ``FUSED_NCC_MAX_POSES = 0`` and a gradient wanted (the switch
tests/conftest.py uses), the criterion applied to its image.  Tolerances are conftest's for these routes: 2e-6 of the
image's scale, 2e-6 for an NCC value, 2e-4 relative for pose gradients.

24^3 phantom, detector 15 x 13 (N = 195: no multiple of 16 or 4), 16 x 13 where a case needs ``p_subsample`` (the
subsample's bit mask needs N % 32 == 0 to be built); fp32 bricks, so that no workspace launch depends on what ran
before."""
import contextlib
import copy
import functools

import pytest
import torch

from diffdrr_amd import DRR, LevenbergMarquardt, NormalizedCrossCorrelation2d, Registration
from diffdrr_amd.data import synthetic_subject

PAIR = ("ddrr_pose_raygen_forward", "ddrr_siddon_forward_bricks")
SEQUENCES = {
    "inference": PAIR,
    "inference_subsample": ("ddrr_pose_raygen_forward", "ddrr_siddon_forward_bricks_masked"),
    "image": PAIR + ("ddrr_siddon_backward_pose_euler",),
    "ncc": PAIR + ("ddrr_siddon_ncc_forward", "ddrr_siddon_ncc_backward_pose"),
    "ncc_sum": PAIR + ("ddrr_siddon_ncc_forward", "ddrr_siddon_ncc_backward_pose"),
    "wncc": PAIR + ("ddrr_wncc_siddon_forward", "ddrr_wncc_siddon_backward_pose"),
    "lm": PAIR + ("ddrr_lm_normal_sums", "ddrr_lm_step"),
}
KW = dict(parameterization="euler_angles", convention="ZXY")
EPS = 1e-5


@contextlib.contextmanager
def launches(ops):
    """the names of the C-ABI entries of the three libraries these routes use, as launched inside the block"""
    names, real = [], {k: getattr(ops, k) for k in ("_launch", "_launch_wncc", "_launch_lm")}
    for k, fn in real.items():
        setattr(ops, k, lambda name, device, *a, _fn=fn: (names.append(name), _fn(name, device, *a))[1])
    try:
        yield names
    finally:
        for k, fn in real.items():
            setattr(ops, k, fn)


def made_by(t):
    """The names of the autograd nodes a tensor came out of (a render's node sits behind the views that shape it)."""
    seen, todo = [], [t.grad_fn]
    while todo:
        node = todo.pop()
        if node is not None and node not in seen:
            seen.append(node)
            todo.extend(n for n, _ in node.next_functions)
    return " ".join(type(n).__name__ for n in seen)


def route_of(names):
    """Which route the launches of a call belong to (see the module's docstring)."""
    for entry, route in (("ddrr_siddon_ncc_forward", "ncc"), ("ddrr_wncc_siddon_forward", "wncc"),
                         ("ddrr_lm_normal_sums", "lm"), ("ddrr_siddon_backward_pose_euler", "image"),
                         ("ddrr_pose_raygen_forward", "inference")):
        if entry in names:
            return route
    return "composed"


# ------------------------------------------------------------------------------------------------ scenes
@functools.lru_cache(maxsize=None)
def _scene(B, det, subsample):
    """The CPU side of a scene, made once: module, poses, a fixed image shared by the batch and one per pose, a
    weight (a collimator's disc, slightly graded) -- never changed by a test (modules are copied before a flip)."""
    torch.manual_seed(5)  # (p_subsample draws its pixels from torch's global generator)
    drr = DRR(synthetic_subject(24, kind="phantom", seed=3), sdd=600.0, height=det[0], width=det[1], delx=4.0,
              p_subsample=0.5 if subsample else None)
    drr.renderer.brick_storage = "f32"
    g = torch.Generator().manual_seed(7 + B)
    rot = (torch.rand(B, 3, generator=g) - 0.5) * 0.5
    xyz = torch.tensor([0.0, 400.0, 0.0]) + (torch.rand(B, 3, generator=g) - 0.5) * 6
    return drr, rot, xyz


class Scene:
    def __init__(self, device, ops, B=3, det=(15, 13), subsample=False):
        drr, rot, xyz = _scene(B, det, subsample)
        self.ops, self.device, self.B, (self.H, self.W) = ops, device, B, det
        self.drr = copy.deepcopy(drr).to(device)
        self.rot, self.xyz = rot.to(device), xyz.to(device)
        with torch.no_grad():
            self.fixed_shared = self.drr(self.rot[:1] * 0.5, self.xyz[:1] + 1.0, **KW)
            self.fixed_per_pose = self.drr(self.rot + 0.03, self.xyz - 1.0, **KW)
        i, j = torch.meshgrid(torch.arange(self.H), torch.arange(self.W), indexing="ij")
        disc = (((i - 7.0) / 7.0) ** 2 + ((j - 6.0) / 6.0) ** 2 <= 1.0).float() * (1.0 + 0.02 * j)
        self.weight = disc.reshape(1, 1, self.H, self.W).to(device)
        self.pose_weights = torch.linspace(0.7, 1.9, B).to(device)

    def module(self, flip=None):
        """A copy of the scene's module with one condition flipped."""
        drr = copy.deepcopy(self.drr)
        if flip is not None:
            FLIPS[flip](drr, self.B)
        return drr


FLIPS = {
    "density_requires_grad": lambda drr, B: drr.density.requires_grad_(True),
    "packed_record": lambda drr, B: setattr(drr.renderer, "packed_record", True),
    "grid_path": lambda drr, B: setattr(drr.renderer, "grid_path", "generic"),
    "over_the_cap": lambda drr, B: setattr(drr, "FUSED_NCC_MAX_POSES", B - 1),
    "patch_size": lambda drr, B: setattr(drr, "patch_size", 4),
    "fuse_ray_generation": lambda drr, B: setattr(drr, "fuse_ray_generation", False),
}


# ------------------------------------------------------------------------------------------------ the calls
def pixel_weights(img):
    return torch.linspace(-1.0, 2.0, img.numel(), device=img.device).reshape(img.shape)


def leaves(sc, grad):
    if not grad:
        return sc.rot, sc.xyz
    return sc.rot.clone().requires_grad_(), sc.xyz.clone().requires_grad_()


def render(sc, drr, grad):
    """drr(rot, xyz, ...) and, where the image takes a gradient, the backward of a fixed per-pixel weighting
    -> dict(names, route, fn, img, g_rot, g_xyz)"""
    r, x = leaves(sc, grad)
    with launches(sc.ops) as names:
        img = drr(r, x, **KW)
        if img.requires_grad:
            (img * pixel_weights(img)).sum().backward()
    return dict(names=tuple(names), route=route_of(names), fn=made_by(img), img=img.detach(),
                g_rot=r.grad, g_xyz=x.grad)


def ncc(sc, drr, fixed, grad=True, reduction="none", weight=None):
    """drr.ncc(...) and its backward: a weighted sum of the per-pose values, or for ``reduction="sum"`` one
    ready-made value -> dict(names, route, fn, values (B,), total, g_rot, g_xyz)"""
    r, x = leaves(sc, grad)
    with launches(sc.ops) as names:
        val = drr.ncc(fixed, r, x, eps=EPS, reduction=reduction, weight=weight)
        if val.requires_grad and reduction == "sum":
            val.backward(gradient=torch.tensor(1.7, device=val.device, dtype=val.dtype))
        elif val.requires_grad:
            (val * sc.pose_weights).sum().backward()
    values = drr.ncc_per_pose if reduction == "sum" else val.detach()
    return dict(names=tuple(names), route=route_of(names), fn=made_by(val), values=values,
                total=val.detach() if reduction == "sum" else None, g_rot=r.grad, g_xyz=x.grad)


def lm_steps(sc, drr, fixed, steps=3):
    """``steps`` Levenberg-Marquardt steps from the scene's poses -> dict(names of the FIRST step, route, first (B,)
    = the NCC of the start poses, state, rot, xyz after the last step)"""
    reg = Registration(drr, sc.rot.clone(), sc.xyz.clone(), **KW)
    lm = LevenbergMarquardt(reg, fixed, eps=EPS)
    with launches(sc.ops) as names:
        first = lm.step().clone()
    for _ in range(steps - 1):
        lm.step()
    return dict(names=tuple(names), route=route_of(names), first=first, state=lm._state.clone(),
                rot=reg._rotation.detach().clone(), xyz=reg._translation.detach().clone())


# ------------------------------------------------------------------------------------------------ the composition
def composed_render(sc, drr):
    ref = copy.deepcopy(drr)
    ref.FUSED_NCC_MAX_POSES = 0
    out = render(sc, ref, grad=True)
    assert out["route"] == "composed", out["names"]
    return out


def composed_ncc(sc, drr, fixed, reduction="none", weight=None):
    """The criterion on the composition's image (``fixed`` / ``weight`` as the call got them), the same backward."""
    ref = copy.deepcopy(drr)
    ref.FUSED_NCC_MAX_POSES = 0
    r, x = leaves(sc, True)
    with launches(sc.ops) as names:
        img = ref(r, x, **KW)
        val = NormalizedCrossCorrelation2d(eps=EPS)(fixed.expand(sc.B, -1, -1, -1), img, weight=weight)
        ((val * sc.pose_weights).sum() if reduction == "none" else 1.7 * val.sum()).backward()
    assert route_of(names) == "composed", names
    return dict(values=val.detach(), g_rot=r.grad, g_xyz=x.grad)


def close_image(got, want, what):
    scale = float(want.abs().max())
    assert got.shape == want.shape and scale > 0, (what, got.shape, want.shape)
    assert float((got - want).abs().max()) <= 2e-6 * scale, what


def close_values(got, want, what):
    assert got.shape == want.shape and float((got.double() - want.double()).abs().max()) <= 2e-6, (what, got, want)


def close_gradients(got, want, what):
    for k in ("g_rot", "g_xyz"):
        a, b = got[k], want[k]
        assert a is not None and float(b.abs().max()) > 0, (what, k)
        assert float((a - b).abs().max()) <= 2e-4 * float(b.abs().max()), (what, k, a, b)


# ------------------------------------------------------------------------------------------------ 1 entry sequences
def check_sequences(device, ops, B):
    """Every route launches exactly its entries, in order, and computes the composition's numbers -- B poses, a fixed
    image shared by the batch and one per pose."""
    sc = Scene(device, ops, B)
    drr = sc.module()
    want_img = composed_render(sc, drr)

    got = render(sc, drr, grad=False)
    assert got["names"] == SEQUENCES["inference"] and not got["img"].requires_grad, got["names"]
    close_image(got["img"], want_img["img"], "inference")

    got = render(sc, drr, grad=True)
    assert got["names"] == SEQUENCES["image"] and ("_EulerSiddonImageFn" in got["fn"]), (got["names"], got["fn"])
    close_image(got["img"], want_img["img"], "image")
    close_gradients(got, want_img, "image")

    sub = Scene(device, ops, B, det=(16, 13), subsample=True)
    got = render(sub, sub.module(), grad=False)
    assert got["names"] == SEQUENCES["inference_subsample"], got["names"]
    close_image(got["img"], composed_render(sub, sub.module())["img"], "inference with p_subsample")

    for which, fixed in (("shared", sc.fixed_shared), ("per pose", sc.fixed_per_pose)):
        for reduction, name in (("none", "ncc"), ("sum", "ncc_sum")):
            want = composed_ncc(sc, drr, fixed, reduction)
            got = ncc(sc, drr, fixed, reduction=reduction)
            assert got["names"] == SEQUENCES[name] and ("_EulerSiddonNccFn" in got["fn"]), (got["names"], got["fn"])
            close_values(got["values"], want["values"], (name, which))
            close_gradients(got, want, (name, which))
            if reduction == "sum":
                assert got["total"].dim() == 0 and abs(float(got["total"]) - float(want["values"].sum())) <= 2e-6 * B
                assert not got["values"].requires_grad
            want = composed_ncc(sc, drr, fixed, reduction, weight=sc.weight)
            got = ncc(sc, drr, fixed, reduction=reduction, weight=sc.weight)
            assert got["names"] == SEQUENCES["wncc"] and ("_EulerSiddonWnccFn" in got["fn"]), (got["names"], got["fn"])
            close_values(got["values"], want["values"], ("wncc", which, reduction))
            close_gradients(got, want, ("wncc", which, reduction))
        got = lm_steps(sc, drr, fixed, steps=1)
        assert got["names"] == SEQUENCES["lm"], got["names"]
        close_values(got["first"], composed_ncc(sc, drr, fixed)["values"], ("lm", which))


# ------------------------------------------------------------------------------------------------ 2 route boundaries
# flip -> the route the call takes with that condition alone flipped (None: the scene as it is)
RENDER_BOUNDARIES = {
    # nothing to differentiate: drr(rot, xyz, ...)
    False: {None: "inference", "density_requires_grad": "composed", "packed_record": "composed",
            "grid_path": "composed", "over_the_cap": "inference", "patch_size": "inference",
            "fuse_ray_generation": "composed"},
    # pose parameters that take a gradient
    True: {None: "image", "density_requires_grad": "composed", "packed_record": "composed", "grid_path": "composed",
           "over_the_cap": "composed", "patch_size": "composed", "fuse_ray_generation": "composed"},
}
# (the render of a composed DRR.ncc goes through drr(...) and takes whatever route applies THERE: "image" below is
# DRR.ncc composing the criterion on the image route's render)
NCC_BOUNDARIES = {None: "ncc", "density_requires_grad": "composed", "packed_record": "composed",
                  "grid_path": "composed", "over_the_cap": "composed", "patch_size": "ncc",
                  "fuse_ray_generation": "composed"}


def check_render_boundary(device, ops, grad, flip):
    sc = Scene(device, ops)
    drr = sc.module(flip)
    got = render(sc, drr, grad=grad)
    assert got["route"] == RENDER_BOUNDARIES[grad][flip], (flip, got["names"])
    assert ("_EulerSiddonImageFn" in got["fn"]) == (got["route"] == "image"), got["fn"]
    if got["route"] != "composed":
        assert got["names"] == SEQUENCES[got["route"]], got["names"]
    want = composed_render(sc, drr)
    close_image(got["img"], want["img"], flip)
    if grad:
        close_gradients(got, want, flip)


def check_ncc_boundary(device, ops, flip, weighted):
    sc = Scene(device, ops)
    drr = sc.module(flip)
    weight = sc.weight if weighted else None
    want_route = NCC_BOUNDARIES[flip]
    if weighted and want_route == "ncc":
        want_route = "wncc"
    got = ncc(sc, drr, sc.fixed_shared, weight=weight)
    assert got["route"] == want_route, (flip, got["names"])
    assert ("_EulerSiddonNccFn" in got["fn"]) == (want_route == "ncc"), got["fn"]
    assert ("_EulerSiddonWnccFn" in got["fn"]) == (want_route == "wncc"), got["fn"]
    if want_route in ("ncc", "wncc"):
        assert got["names"] == SEQUENCES[want_route], got["names"]
    else:
        assert not any(n.startswith(("ddrr_siddon_ncc", "ddrr_wncc_siddon")) for n in got["names"]), got["names"]
    want = composed_ncc(sc, drr, sc.fixed_shared, weight=weight)
    close_values(got["values"], want["values"], flip)
    close_gradients(got, want, flip)


def check_ncc_without_a_gradient(device, ops, weighted):
    """Nothing to differentiate: the forward-only render (the inference route) and the criterion's own kernel."""
    sc = Scene(device, ops)
    drr = sc.module()
    weight = sc.weight if weighted else None
    for no_grad in (False, True):  # (poses that take no gradient; and grad mode switched off around poses that do)
        with torch.no_grad() if no_grad else contextlib.nullcontext():
            got = ncc(sc, drr, sc.fixed_shared, grad=no_grad, weight=weight)
        assert got["route"] == "inference" and got["names"][:2] == PAIR and got["fn"] == "", (got["names"], got["fn"])
        assert ("ddrr_wncc_forward" if weighted else "ddrr_ncc_forward") in got["names"], got["names"]
        close_values(got["values"], composed_ncc(sc, drr, sc.fixed_shared, weight=weight)["values"], "no gradient")


def check_subsample_boundaries(device, ops):
    """``p_subsample`` (16 x 13): inference keeps its route on the masked kernel; the image route and DRR.ncc do not
    take a subsample, with or without a weight."""
    sc = Scene(device, ops, det=(16, 13), subsample=True)
    drr = sc.module()
    want = composed_render(sc, drr)
    got = render(sc, drr, grad=False)
    assert got["names"] == SEQUENCES["inference_subsample"], got["names"]
    close_image(got["img"], want["img"], "inference")
    got = render(sc, drr, grad=True)
    assert got["route"] == "composed" and "_EulerSiddon" not in got["fn"], (got["names"], got["fn"])
    close_image(got["img"], want["img"], "image")
    close_gradients(got, want, "image")
    for weight in (None, sc.weight):
        got = ncc(sc, drr, sc.fixed_shared, weight=weight)
        assert got["route"] == "composed" and "_EulerSiddon" not in got["fn"], (got["names"], got["fn"])
        ref = composed_ncc(sc, drr, sc.fixed_shared, weight=weight)
        close_values(got["values"], ref["values"], "ncc")
        close_gradients(got, ref, "ncc")


def check_fixed_and_weight_boundaries(device, ops):
    """A float64 or mis-shaped ``fixed`` / ``weight`` and a weight that takes a gradient leave the fused step: DRR.ncc
    composes the criterion on the image route's render -- or raises what the criterion raises, nothing fused
    launched."""
    sc = Scene(device, ops)
    drr = sc.module()
    fixed, weight = sc.fixed_shared, sc.weight
    fused = ("ddrr_siddon_ncc", "ddrr_wncc_siddon")

    def composes(tag, fixed, weight):
        got = ncc(sc, drr, fixed, weight=weight)
        assert got["route"] == "image" and "NccFn" not in got["fn"], (tag, got["names"], got["fn"])
        assert not any(n.startswith(fused) for n in got["names"]), (tag, got["names"])
        want = composed_ncc(sc, drr, fixed, weight=weight)
        close_values(got["values"], want["values"], tag)
        close_gradients(got, want, tag)

    def raises(tag, fixed, weight):
        with launches(ops) as names, pytest.raises((RuntimeError, ValueError, AssertionError)):
            drr.ncc(fixed, *leaves(sc, True), weight=weight)
        assert not any(n.startswith(fused) for n in names), (tag, names)

    composes("float64 fixed", fixed.double(), None)
    composes("float64 fixed, weight", fixed.double(), weight)
    composes("float64 weight", fixed, weight.double())
    composes("weight that takes a gradient", fixed, weight.clone().requires_grad_())
    composes("fixed (1, H, W)", fixed[0], None)
    raises("fixed one column short", fixed[..., :-1], None)
    raises("weight one column short", fixed, weight[..., :-1])
    raises("two fixed images for three poses", sc.fixed_per_pose[:2], None)


def check_lm_boundaries(device, ops):
    """LevenbergMarquardt refuses what its render does not take, naming the condition (the rest of its domain:
    tests/test_lm.py::test_domain_errors_name_the_condition)."""
    sc = Scene(device, ops)
    for flip, word in (("patch_size", "patch_size"), ("fuse_ray_generation", "fuse_ray_generation"),
                       ("grid_path", "grid_path"), ("over_the_cap", "poses"), ("packed_record", "packed"),
                       ("density_requires_grad", "gradient")):
        reg = Registration(sc.module(flip), sc.rot.clone(), sc.xyz.clone(), **KW)
        with launches(ops) as names, pytest.raises(ValueError, match=word):
            LevenbergMarquardt(reg, sc.fixed_shared)
        assert not names
    sub = Scene(device, ops, det=(16, 13), subsample=True)
    with pytest.raises(ValueError, match="p_subsample"):
        LevenbergMarquardt(Registration(sub.module(), sub.rot.clone(), sub.xyz.clone(), **KW), sub.fixed_shared)
