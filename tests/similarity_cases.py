"""The image-similarity kernels (csrc/pose_ncc.hip, ncc_patch_core.h, blur_core.h, sobel_core.h) against the
torch composition they replace evaluated in FLOAT64, on images that look like the radiographs a registration
feeds them: a mean of hundreds to thousands, a smooth variation of a sixth of it across the image -- a fraction
of a percent across a 13 x 13 window -- and a little noise.  The cases of tests/test_similarity_float64.py (host
build of the kernel cores, tests/emu) and tests/test_gpu_similarity_float64.py (the device).

Images (:func:`drr_like`), per image with c = rand(4) - 0.5 from a seeded generator, x, y in [-1, 1]:
    mean + amp exp(-((x - c0)^2 + (y - c1)^2) / 0.3) + amp / 2 sin(3 x + 5 c2) cos(2 y + c3) + noise randn
formed in float64 and rounded once to float32; those float32 values, cast back, are the reference's input.
``SETTINGS``: (mean, amp, noise) = (350, 60, 0.5), (350, 60, 0.05), (3000, 500, 2).

Reference: the modules of diffdrr_amd.metrics with their kernels switched off (``_no_patch_kernel``,
``_no_blur_kernel``, ``ops.on_device`` -> False: `to_patches` + `norm`, reflect pad + conv2d, the whole-image
formula written out), float64 input, differentiated by autograd under per-pose weights rand(B) + 0.5.
Yardstick: what the same composition loses in float32, as in conftest.check_metrics_against_reference:
    values      max |kernel - f64|  <=  2 max |fp32 composition - f64| + 2e-6
    gradients   rel_err(kernel, f64)  <=  2 rel_err(fp32 composition, f64) + 2e-5,
    rel_err = the largest absolute difference over the largest |f64| entry;
every pair and every pixel compared.  (The Sobel responses are images, not scores: they and their adjoint take
the gradients' yardstick.)  Every case records the C-ABI entries it launched: the kernel evaluation must have
taken its entries, the two compositions none.

Measured: the largest and the smallest kernel error of each group of cases, gradients (d/d moving, d/d fixed,
`.sum()`) unless it says values; in brackets what the fp32 composition itself lost on the same cases.

    cases                                     host emulation                         MI355X
    patch p 5 ... 13, (3, 1, 64, 80)          6.0e-7 ... 9.0e-6 (6.5e-7 ... 2.2e-5)  not measured
    patch p 8, 32, 50, 64 (run-time loop)     2.4e-7 ... 1.2e-6 (1.2e-7 ... 1.7e-6)  not measured
    patch p 7, two channels                   5.5e-7 ... 9.1e-7 (1.4e-6 ... 1.8e-6)  not measured
    patch p 5, 64 pairs (tile walk)           2.6e-6 ... 4.0e-6 (5.4e-6 ... 7.7e-6)  not measured
    whole image                               1.4e-7 ... 4.9e-7 (1.1e-7 ... 4.8e-7)  not measured
    Sobel / blur + Sobel, output and adjoint  8.5e-8 ... 4.0e-7 (8.7e-8 ... 1.5e-6)  not measured
    criteria end to end                       4.6e-7 ... 2.3e-4 (5.8e-7 ... 3.0e-4)  not measured
    values, every case                        4.6e-9 ... 5.0e-7 (5.9e-9 ... 7.2e-7)  not measured

(The largest figures of the first row are p = 5 on the quiet images, those of `end to end` the patch-wise gradient
NCC: windows of Sobel responses with next to no variation, where the composition loses as much.)  Before the
window means were taken relative to a pivot and the backward's terms centred per window (ncc_patch_core.h) --
plain fp32 sums of p^2 pixels, the backward as a S1 - sum(mu_a c1) - b S3 + sum(c3 mu_b) -- the host emulation's
patch gradients missed the yardstick at every p <= 13: 7.1e-5 ... 1.3e-4 at p = 7 (allowed 2.5e-5 ... 3.5e-5),
4.0e-5 ... 8.3e-5 at p = 13 (allowed 2.1e-5 ... 2.2e-5); p >= 32 passed.
"""
from __future__ import annotations

import contextlib
import copy

import numpy as np
import torch

from conftest import rel_err
from diffdrr_amd import metrics as M
from diffdrr_amd import ops

SETTINGS = {"mean350": (350.0, 60.0, 0.5), "mean350_quiet": (350.0, 60.0, 0.05), "mean3000": (3000.0, 500.0, 2.0)}
FIXED_SEED, MOVING_SEED, WEIGHT_SEED = 1, 2, 3


def drr_like(n, H, W, seed, setting):
    """(n, H, W) float32 images of the module docstring's formula."""
    mean, amp, noise = SETTINGS[setting]
    g = torch.Generator().manual_seed(seed)
    f64 = torch.float64
    y, x = torch.meshgrid(torch.linspace(-1, 1, H, dtype=f64), torch.linspace(-1, 1, W, dtype=f64), indexing="ij")
    out = []
    for _ in range(n):
        c = torch.rand(4, generator=g, dtype=f64) - 0.5
        img = mean + amp * torch.exp(-((x - c[0]) ** 2 + (y - c[1]) ** 2) / 0.3)
        img = img + 0.5 * amp * torch.sin(3 * x + 5 * c[2]) * torch.cos(2 * y + c[3])
        out.append(img + noise * torch.randn(H, W, generator=g, dtype=f64))
    return torch.stack(out).float()


def pair(B, C, H, W, setting, device):
    """fixed (1, C, H, W), moving (B, C, H, W), weights (B): different seeds for the two images"""
    fixed = drr_like(C, H, W, FIXED_SEED, setting).reshape(1, C, H, W).to(device)
    moving = drr_like(B * C, H, W, MOVING_SEED, setting).reshape(B, C, H, W).to(device)
    w = (torch.rand(B, generator=torch.Generator().manual_seed(WEIGHT_SEED)) + 0.5).to(device)
    return fixed, moving, w


@contextlib.contextmanager
def launches():
    """the names of the C-ABI entries launched inside the block"""
    names, real = [], ops._launch
    ops._launch = lambda name, device, *a: (names.append(name), real(name, device, *a))[1]
    try:
        yield names
    finally:
        ops._launch = real


@contextlib.contextmanager
def composition():
    """nothing is `on the device` inside the block: every module takes its torch composition"""
    real = ops.on_device
    ops.on_device = lambda t: False
    try:
        with launches() as names:
            yield
    finally:
        ops.on_device = real
    assert not names, f"the reference launched {names}"


def unfused(crit):
    """the same module with its kernels switched off"""
    c = copy.deepcopy(crit)
    for m in [c] + list(getattr(c, "nccs", [])):
        m._no_patch_kernel = True
    for m in c.modules():
        if isinstance(m, M.Sobel):
            m._no_blur_kernel = True
    return c


def off_by_one(t):
    """the same values, contiguous, in storage that starts one float past an aligned address"""
    buf = t.new_empty(t.numel() + 1)
    buf[1:].copy_(t.reshape(-1))
    out = buf[1:].view(t.shape)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def as_numpy(*tensors):
    return tuple(t.detach().double().cpu().numpy() for t in tensors)


class Figures:
    """prints every figure of a case, then fails on those that missed the yardstick"""

    def __init__(self, case):
        self.case, self.missed = case, []

    def _note(self, what, err, own, allowed):
        print(f"[{self.case}] {what}: kernel {err:.2e}  fp32 composition {own:.2e}  allowed {allowed:.2e}")
        if not err <= allowed:
            self.missed.append(f"{what}: {err:.3e} > {allowed:.3e} (fp32 composition {own:.3e})")

    def value(self, what, k, c32, f64):
        err, own = float(np.abs(k - f64).max()), float(np.abs(c32 - f64).max())
        self._note(what, err, own, 2 * own + 2e-6)

    def grad(self, what, k, c32, f64):
        assert k.shape == f64.shape == c32.shape, (what, k.shape, c32.shape, f64.shape)
        err, own = rel_err(k, f64), rel_err(c32, f64)
        self._note(what, err, own, 2 * own + 2e-5)

    def done(self):
        assert not self.missed, (self.case, self.missed)


def evaluate(crit, fixed, moving, w, place_fixed=torch.clone, place_moving=torch.clone, grad_fixed=True):
    """(value (B), d / d moving, d / d fixed) of sum_b w_b crit(fixed expanded over the batch, moving)_b;
    w = None: `.sum()`, whose gradient arrives as an expanded scalar."""
    a = place_fixed(fixed).detach().requires_grad_(grad_fixed)
    x = place_moving(moving).detach().requires_grad_()
    v = crit(a.expand(moving.shape[0], -1, -1, -1), x)
    (v.sum() if w is None else (v * w).sum()).backward()
    return as_numpy(v, x.grad, a.grad if grad_fixed else x.grad)


def kernel_and_references(crit, fixed, moving, w, entries, **place):
    """:func:`evaluate` by the kernels (which must launch `entries`), by the float32 and by the float64 composition"""
    with launches() as names:
        k = evaluate(crit, fixed, moving, w, **place)
    assert set(entries) <= set(names), (entries, names)
    ref = unfused(crit)
    with composition():
        c32 = evaluate(ref, fixed, moving, w)
        f64 = evaluate(ref, fixed.double(), moving.double(), None if w is None else w.double())
    return k, c32, f64


def check_criterion(case, crit, fixed, moving, w, entries, **place):
    """value, d / d moving, d / d fixed under per-pose weights, and d / d moving of `.sum()`"""
    fig = Figures(case)
    k, c32, f64 = kernel_and_references(crit, fixed, moving, w, entries, **place)
    fig.value("value", k[0], c32[0], f64[0])
    fig.grad("d/d moving", k[1], c32[1], f64[1])
    fig.grad("d/d fixed", k[2], c32[2], f64[2])
    k, c32, f64 = kernel_and_references(crit, fixed, moving, None, entries, grad_fixed=False, **place)
    fig.grad("d/d moving of .sum()", k[1], c32[1], f64[1])
    fig.done()


# ------------------------------------------------------------------------------------------ patch NCC
PATCH_ENTRIES = ("ddrr_ncc_patch_forward", "ddrr_ncc_patch_backward")
# the instantiated window sizes on a window grid that is no multiple of the 16 x 16 tile either way; the
# run-time loop: even, large, and the first / last size whose backward asks for more than 64 KB of LDS
# (p = 50: 65 rows of 80 float4; hipFuncSetAttribute); two channels
PATCH_SHAPES = {
    **{f"p{p}": ((3, 1, 64, 80), p) for p in (5, 7, 9, 11, 13)},
    "p8": ((2, 1, 40, 33), 8), "p32": ((2, 1, 48, 48), 32), "p50": ((1, 1, 70, 66), 50), "p64": ((1, 1, 70, 66), 64),
    "p7_two_channels": ((2, 2, 40, 33), 7),
}
PATCH_CASES = [(name, setting) for name in PATCH_SHAPES for setting in SETTINGS]


def check_patch_ncc(device, name, setting):
    (B, C, H, W), p = PATCH_SHAPES[name]
    fixed, moving, w = pair(B, C, H, W, setting, device)
    check_criterion(f"patch {name} {setting}", M.NormalizedCrossCorrelation2d(patch_size=p), fixed, moving, w,
                    PATCH_ENTRIES)


def check_patch_ncc_tile_walk(device, setting="mean350"):
    """64 pairs of 96 x 120 windows: 48 tiles a pair for 32 workgroups a pair (pose_ncc.hip
    kPatchWorkgroupsWanted / B), so half of the forward's workgroups take two tiles.  Four distinct moving images
    (pair b: image b mod 4) under 64 weights: the float64 reference is four pairs, tiled; all 64 are compared."""
    B, n, H, W, p = 64, 4, 100, 124, 5
    fixed, base, _ = pair(n, 1, H, W, setting, device)
    which = torch.arange(B, device=device) % n
    w = (torch.rand(B, generator=torch.Generator().manual_seed(WEIGHT_SEED)) + 0.5).to(device)
    crit = M.NormalizedCrossCorrelation2d(patch_size=p)
    with launches() as names:
        k = evaluate(crit, fixed, base[which], w)
    assert set(PATCH_ENTRIES) <= set(names), names

    def four_pairs(dtype):
        a, x, wt = fixed.to(dtype).clone().requires_grad_(), base.to(dtype).clone().requires_grad_(), w.to(dtype)
        v = unfused(crit)(a.expand(n, -1, -1, -1), x)
        # the pairs are independent: d v_j / d x_j from `.sum()`, pair b's share is w_b times image (b mod 4)'s;
        # the fixed image collects every pair's
        gx, = torch.autograd.grad(v.sum(), x, retain_graph=True)
        ga, = torch.autograd.grad((v * torch.zeros(n, dtype=dtype, device=device).index_add_(0, which, wt)).sum(), a)
        return as_numpy(v[which], gx[which] * wt[:, None, None, None], ga)

    with composition():
        c32, f64 = four_pairs(torch.float32), four_pairs(torch.float64)
    fig = Figures(f"patch p5 tile walk {setting}")
    fig.value("value", k[0], c32[0], f64[0])
    fig.grad("d/d moving", k[1], c32[1], f64[1])
    fig.grad("d/d fixed", k[2], c32[2], f64[2])
    fig.done()


# ------------------------------------------------------------------------------------- whole-image NCC
NCC_ENTRIES = ("ddrr_ncc_forward", "ddrr_ncc_backward")
# N = 1665: no multiple of 4, the scalar loop; N = 480: 120 of the 1024 threads hold a float4; N = 9600: several
# strides of the vector loop -- and the same N from storage that starts one float past an aligned address, the
# moving batch or the shared fixed image: the misaligned fallback
NCC_SHAPES = {"45x37": (45, 37, {}), "24x20": (24, 20, {}), "96x100": (96, 100, {}),
              "96x100_moving_off_by_one": (96, 100, {"place_moving": off_by_one}),
              "96x100_fixed_off_by_one": (96, 100, {"place_fixed": off_by_one})}
NCC_CASES = [(name, setting) for name in NCC_SHAPES for setting in ("mean350", "mean3000")]


def check_whole_image_ncc(device, name, setting):
    H, W, place = NCC_SHAPES[name]
    fixed, moving, w = pair(3, 1, H, W, setting, device)
    check_criterion(f"ncc {name} {setting}", M.NormalizedCrossCorrelation2d(), fixed, moving, w, NCC_ENTRIES, **place)


# ---------------------------------------------------------------------------- Sobel, blur + Sobel
# sizes that are no multiple of the 32 x 32 tile, 3 ... 31 taps, an image barely larger than the padding (every
# pixel folded by the reflection), and sigma = 0: the plain Sobel pair
SOBEL_SHAPES = {"45x70_sigma1": ((2, 45, 70), 1.0), "32x64_sigma0.4": ((3, 32, 64), 0.4),
                "16x33_sigma5": ((2, 16, 33), 5.0), "4x5_sigma1": ((1, 4, 5), 1.0), "45x70_sigma0": ((2, 45, 70), 0.0)}
SOBEL_CASES = [(name, setting) for name in SOBEL_SHAPES for setting in ("mean350", "mean3000")]


def check_sobel(device, name, setting):
    (B, H, W), sigma = SOBEL_SHAPES[name]
    img = drr_like(B, H, W, MOVING_SEED, setting)[:, None].to(device)
    g = torch.Generator().manual_seed(WEIGHT_SEED)
    w = torch.randn(B, 2, H, W, generator=g).to(device)
    w3 = torch.randn(3, 2, H, W, generator=g).to(device)
    sob = M.Sobel(sigma)
    entries = ("ddrr_blur_sobel_forward", "ddrr_blur_sobel_backward") if sigma > 0 else \
        ("ddrr_sobel_forward", "ddrr_sobel_backward")

    def run(m, dtype):
        x = img.to(dtype).clone().requires_grad_()
        out = m(x)
        (out * w.to(dtype)).sum().backward()
        one = img[:1].to(dtype).clone().requires_grad_()  # one image for the whole batch, `expand`ed
        out3 = m(one.expand(3, -1, -1, -1))
        (out3 * w3.to(dtype)).sum().backward()
        return as_numpy(out, x.grad, out3, one.grad)

    with launches() as names:
        k = run(sob, torch.float32)
    assert set(entries) <= set(names), (entries, names)
    with composition():
        c32, f64 = run(unfused(sob), torch.float32), run(unfused(sob), torch.float64)
    fig = Figures(f"sobel {name} {setting}")
    for i, what in enumerate(("output", "adjoint", "output, expanded image", "adjoint, expanded image")):
        fig.grad(what, k[i], c32[i], f64[i])
    fig.done()


# ------------------------------------------------------------------------------------ the criteria
CRITERIA = {
    "gncc_sigma1": (lambda: M.GradientNormalizedCrossCorrelation2d(sigma=1.0),
                    ("ddrr_blur_sobel_forward", "ddrr_blur_sobel_backward") + NCC_ENTRIES),
    "gncc_patch9_sigma1": (lambda: M.GradientNormalizedCrossCorrelation2d(patch_size=9, sigma=1.0),
                           ("ddrr_blur_sobel_forward", "ddrr_blur_sobel_backward") + PATCH_ENTRIES),
    "multiscale_none_13": (lambda: M.MultiscaleNormalizedCrossCorrelation2d([None, 13], [0.5, 0.5]),
                           NCC_ENTRIES + PATCH_ENTRIES),
}
CRITERION_CASES = [(name, setting) for name in CRITERIA for setting in ("mean350", "mean3000")]


def check_end_to_end(device, name, setting):
    make, entries = CRITERIA[name]
    fixed, moving, w = pair(3, 1, 64, 80, setting, device)
    check_criterion(f"{name} {setting}", make(), fixed, moving, w, entries)
