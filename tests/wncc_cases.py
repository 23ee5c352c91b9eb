"""What tests/test_wncc.py (host emulation) and tests/test_gpu_wncc.py (MI355X) share: the host build of
csrc/wncc_core.h (tests/emu/wncc_emu.cpp), the weight patterns, the float64 definition of the weighted (masked)
NCC of include/diffdrr_wncc_hip.h and the checks, written once as ``check_*(device, ops)``.

The fused entries run on the scenes of tests/fused_step_cases.py (``F``): the real blocked record of a render,
the chain of that module written out in float64 (``F.pose_gradient``), its bound ``fine`` and its gate
    err <= max(2 x the float32 torch composition's error, 8 * 2^-24 x the absolute-value bound).
The weight enters the chain in one place, the per-pixel gradient of the similarity (:func:`wncc_of`):
    V = {w != 0};  Sw = sum_V w;  mu = sum_V w x / Sw;  s = sqrt(sum_V w (x - mu)^2 / Sw + eps);  z = (x - mu) / s
    ncc = sum_V w z1 z2 / Sw;      d ncc / d x2[n] = (w_n / Sw) (z1 - ncc z2) / s2
and its bound is F.ncc_of's with 1 / N replaced by w_n / Sw.  A pixel outside V is selected out of every sum.

The image entries (``NormalizedCrossCorrelation2d(...)(x1, x2, weight=)``) run on the images and under the
yardstick of tests/similarity_cases.py (``S``): values <= 2 x fp32 composition + 2e-6, gradients rel_err <= 2 x fp32
composition + 2e-5; the composition is ``metrics.weighted_ncc``."""
import contextlib
import copy
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import fused_step_cases as F
import lm_cases
import similarity_cases as S
from conftest import ROOT
from diffdrr_amd import Registration, _lib
from diffdrr_amd import metrics as M

EMU_SRC = os.path.join(ROOT, "tests", "emu", "wncc_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "_build", "libwncc_emu.so")
F64, F32 = torch.float64, torch.float32
NCC_EPS = F.NCC_EPS
HOST_CASES = F.HOST_CASES
GPU_CASES = HOST_CASES + ("256x67x65",)  # (one launch shape whatever the batch: no large-launch variant to hit)
WNCC_ENTRIES = ("ddrr_wncc_forward", "ddrr_wncc_backward")
SIDDON_ENTRIES = ("ddrr_wncc_siddon_forward", "ddrr_wncc_siddon_backward_pose")


@functools.lru_cache(maxsize=None)
def emu_library():
    """The host build of the entries (tests/emu/wncc_emu.cpp), bound through the product's own binding."""
    csrc = os.path.join(ROOT, "diffdrr_amd", "csrc")
    deps = [EMU_SRC, os.path.join(ROOT, "include", "diffdrr_wncc_hip.h")] + [
        os.path.join(csrc, f) for f in ("wncc_core.h", "siddon_core.h", "raygen_core.h", "record_layout.h",
                                        "ddrr_common.h")]
    if not (os.path.exists(EMU_SO) and all(os.path.getmtime(d) <= os.path.getmtime(EMU_SO) for d in deps)):
        os.makedirs(os.path.dirname(EMU_SO), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-mfma", "-ffp-contract=off",
                        "-Wno-unknown-pragmas", EMU_SRC, "-o", EMU_SO], check=True)
    return _lib.wncc_library(EMU_SO)


def route_wncc_to_emulation(monkeypatch, ops):
    """The launcher patch of the host tests: ops' weighted NCC launches go to the host build."""
    lib = emu_library()
    monkeypatch.setattr(ops, "_launch_wncc", lambda name, device, *a: lib.call(name, *a, None))
    monkeypatch.setattr(ops, "_query_wncc", lambda name, *a: lib.query(name, *a))


@contextlib.contextmanager
def launches(ops):
    """the names of the C-ABI entries of every library launched inside the block"""
    names, real, real_w = [], ops._launch, ops._launch_wncc
    ops._launch = lambda name, device, *a: (names.append(name), real(name, device, *a))[1]
    ops._launch_wncc = lambda name, device, *a: (names.append(name), real_w(name, device, *a))[1]
    try:
        yield names
    finally:
        ops._launch, ops._launch_wncc = real, real_w


# ------------------------------------------------------------------------------------------------ weights
PATTERNS = ("ones", "disc", "smooth", "half", "edge-hot", "one pose empty")


def _half(rows, N, gen):
    """Bernoulli(0.5) zeros, no row left empty (a row of six pixels can come out all zero: pixel 0 is kept)."""
    w = (torch.rand(rows, N, generator=gen) < 0.5).float()
    w[:, 0] = torch.where(w.sum(1) == 0, torch.ones(rows), w[:, 0])
    return w


def weights(pattern, B, H, W, per_pose, device, seed=0):
    """(B | 1, N) float32 weights of the issue's patterns; None where the pattern does not apply (one pose empty
    needs per-pose weights and more than one pose)."""
    N, rows = H * W, (B if per_pose else 1)
    gen = torch.Generator().manual_seed(1000 * seed + 41 + 7 * N + rows + 100 * PATTERNS.index(pattern))
    if pattern == "ones":
        w = torch.ones(rows, N)
    elif pattern == "disc":  # an ellipse with semi-axes 0.45 H, 0.45 W: a collimator; per pose: moved by b % 4 pixels
        i, j = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
        w = torch.stack([((((i - (H - 1) / 2 - 0.5 * (b % 4)) / (0.45 * H)) ** 2
                           + ((j - (W - 1) / 2 + 0.5 * (b % 4)) / (0.45 * W)) ** 2) <= 1.0).float().reshape(N)
                         for b in range(rows)])
    elif pattern == "smooth":
        w = 0.25 + 1.5 * torch.rand(rows, N, generator=gen)
    elif pattern == "half":
        w = _half(rows, N, gen)
    elif pattern == "edge-hot":
        cols = torch.tensor(F.edge_set(N))
        w = torch.zeros(rows, N)
        w[:, cols] = 0.5 + torch.rand(rows, len(cols), generator=gen)
    else:
        if not per_pose or B == 1:
            return None
        w = _half(rows, N, gen)
        w[-1] = 0.0
    return w.to(device).contiguous()


def all_weights(B, H, W, device, patterns=PATTERNS, edge_seeds=(0, 0)):
    """[(label, weight)]: every pattern as one weight for the batch and as per-pose weights; edge_seeds: the seeds
    of the shared and of the per-pose edge-hot magnitudes (:func:`edge_hot_seeds`)"""
    out = []
    for pattern in patterns:
        for per_pose in (False, True):
            w = weights(pattern, B, H, W, per_pose, device, seed=edge_seeds[per_pose] if pattern == "edge-hot" else 0)
            if w is not None:
                out.append((f"{pattern} {'per pose' if per_pose else 'shared'}", w))
    return out


def placements(w):
    return (("aligned", w), ("odd offset", F.unaligned(w)))


# ------------------------------------------------------------------------------------------------ the definition
def x2_of(sc, dtype):
    """The moving image x2 = L I of the scene in `dtype` (F.ncc_of's), computed once."""
    key = ("x2", dtype)
    if key not in sc.cache:
        q = F.inputs(sc, dtype)
        ry = F.rays_of(F.pose_of(q.rot, q.xyz, sc.axes, q.Ro), q.Ainv, q.P)
        sc.cache[key] = ry.L * q.planes[0]
    return sc.cache[key]


def wncc(x1, x2, w, eps, g_out=None):
    """The definition on (B, n) tensors in their dtype: stats (B, 6) = (mu1, s1, mu2, s2, ncc, Sw); with g_out the
    per-pixel gradient of sum_b g_out_b ncc_b w.r.t. x2 and its absolute-value bound."""
    on = w != 0
    zero = torch.zeros_like(x2)
    a, c = torch.where(on, x1, zero), torch.where(on, x2, zero)
    Sw = w.sum(-1, keepdim=True)
    some = Sw > 0
    inv = torch.where(some, 1.0 / torch.where(some, Sw, torch.ones_like(Sw)), torch.zeros_like(Sw))
    mu1, mu2 = (w * a).sum(-1, keepdim=True) * inv, (w * c).sum(-1, keepdim=True) * inv
    d1, d2 = torch.where(on, a - mu1, zero), torch.where(on, c - mu2, zero)
    s1 = ((w * d1 * d1).sum(-1, keepdim=True) * inv + eps).sqrt()
    s2 = ((w * d2 * d2).sum(-1, keepdim=True) * inv + eps).sqrt()
    z1, z2 = d1 / s1, d2 / s2
    ncc = (w * z1 * z2).sum(-1, keepdim=True) * inv
    stats = torch.cat([mu1, s1, mu2, s2, ncc, torch.where(some, Sw, torch.zeros_like(Sw))], -1)
    if g_out is None:
        return stats
    go = g_out.to(x2.dtype).reshape(-1, 1).expand(x2.shape[0], 1)
    g = go * w * inv * (z1 - z2 * ncc) / s2
    g_abs = go.abs() * w * inv * ((a.abs() + mu1.abs()) / s1 + (c.abs() + mu2.abs()) / s2 * ncc.abs()) / s2
    return stats, g, g_abs


def wncc_of(sc, x1, w, g_out=None, dtype=F64, cols=None):
    """:func:`wncc` of the scene's moving image with the fixed image(s) x1 ((1 | B), N) under w ((1 | B), N);
    cols: on those pixels alone (every other pixel has weight 0)."""
    x2 = x2_of(sc, dtype)
    x1, w = x1.to(dtype).expand(sc.B, -1), w.to(dtype).expand(sc.B, -1)
    if cols is not None:
        x1, x2, w = x1[:, cols], x2[:, cols], w[:, cols]
    return wncc(x1, x2, w, NCC_EPS, g_out)


def stats_mag(want):
    return torch.stack([want[:, 0].abs(), want[:, 1], want[:, 2].abs(), want[:, 3], torch.ones_like(want[:, 4]),
                        want[:, 5]], -1)


def gradient_reference(sc, x1, w, g_out, path, cols=None):
    """(want, own, fine) of the pose gradient: the definition in float64, the same chain in float32, the bound"""
    _, g, g_abs = wncc_of(sc, x1, w, g_out, cols=cols)
    want, fine = F.pose_gradient(sc, g, g_abs, with_img_path=path, cols=cols)
    _, g32, _ = wncc_of(sc, x1, w, g_out, dtype=F32, cols=cols)
    own, _ = F.pose_gradient(sc, g32, with_img_path=path, dtype=F32, cols=cols)
    return want, own, fine


def fixed_images(sc):
    return (("shared", sc.x1_shared), ("per pose", sc.x1_per_pose))


# ------------------------------------------------------------------------------------------------ 1 sharpness
def edge_hot_least_move(sc, w):
    """In float64: the least, over both fixed images, every pose and every weighted ray, of what removing that ray
    alone moves the value or a gradient output by, in allowances."""
    one = torch.ones((), device=sc.device)
    cols = torch.tensor(F.edge_set(sc.N), device=sc.device)
    least = float("inf")
    for _, x1 in fixed_images(sc):
        v = wncc_of(sc, x1, w, cols=cols)[:, 4]
        want, own, fine = gradient_reference(sc, x1, w, one, True, cols=cols)
        allow = F.allowance(want, own, fine)
        for e in range(len(cols)):
            w_e = w.clone()
            w_e[:, cols[e]] = 0.0
            v_e = wncc_of(sc, x1, w_e, cols=cols)[:, 4]
            g_e, _, _ = gradient_reference(sc, x1, w_e, one, True, cols=cols)
            move = torch.maximum((v_e - v).abs() / F.FLOOR, ((g_e - want).abs() / allow).amax(1))
            least = min(least, float(move.min()))
    return least


def edge_hot_seeds(name, device, ops):
    """The seeds of the case's edge-hot magnitudes (shared, per pose): the first of 0 ... 7 whose every weighted ray
    is visible by more than 4 allowances, decided in float64 alone (another draw, never a looser gate); the last
    one tried otherwise, and check_sharpness fails."""
    sc = F.scene(name, device, ops)
    if "edge seeds" not in sc.cache:
        seeds = []
        for per_pose in (False, True):
            for seed in range(8):
                least = edge_hot_least_move(sc, weights("edge-hot", sc.B, sc.H, sc.W, per_pose, device, seed=seed))
                print(f"{name} edge-hot {'per pose' if per_pose else 'shared'} seed {seed}: the least visible weighted "
                      f"ray moves an output by {least:.3g} allowances")
                if least > 4:
                    break
            seeds.append(seed)
        sc.cache["edge seeds"] = tuple(seeds)
    return sc.cache["edge seeds"]


SHARP_SEEDS = 4000  # draws tried before a pattern is given up as not sharp (the check then fails)


def _value_is_sharp(sc, w):
    """(B,) bool, in float64: under w the value differs from the unweighted one by more than 100 value allowances, with
    the shared and with the per-pose fixed image."""
    ones = torch.ones(1, sc.N, device=sc.device)
    ok = torch.ones(sc.B, dtype=torch.bool, device=sc.device)
    for x_label, x1 in fixed_images(sc):
        key = ("plain value", x_label)
        if key not in sc.cache:
            sc.cache[key] = wncc_of(sc, x1, ones)[:, 4]
        ok &= (wncc_of(sc, x1, w)[:, 4] - sc.cache[key]).abs() > 100 * F.FLOOR
    return ok


def sharp_weights(name, device, ops, pattern, per_pose):
    """The case's smooth / half weights: the issue's draw (0.25 + 1.5 rand; Bernoulli(0.5) zeros) under the first seed
    for which the weighted value is a sharp check at EVERY pose with either fixed image, decided in float64 alone --
    another seed, never a looser gate.  One weight for the batch: the first seed at which every pose passes (the
    value's difference changes sign from pose to pose, so at 256 poses most draws leave one to four of them short:
    hundreds of seeds are tried, each two evaluations of the definition).  Per-pose weights: every pose keeps the row
    of the first seed at which it passes.  The small cases pass at seed 0."""
    sc = F.scene(name, device, ops)
    key = ("sharp weights", pattern, per_pose)
    if key not in sc.cache:
        chosen, todo = None, torch.ones(sc.B, dtype=torch.bool, device=device)
        for seed in range(SHARP_SEEDS):
            w = weights(pattern, sc.B, sc.H, sc.W, per_pose, device, seed=seed)
            ok = _value_is_sharp(sc, w)
            if not per_pose:
                chosen = w
                if bool(ok.all()):
                    break
            else:
                chosen = w.clone() if chosen is None else chosen
                take = todo & ok
                chosen[take] = w[take]
                todo &= ~ok
                if not bool(todo.any()):
                    break
        print(f"{name} {pattern} {'per pose' if per_pose else 'shared'}: sharp at every pose after {seed + 1} draw(s)")
        sc.cache[key] = chosen.contiguous()
    return sc.cache[key]


def scene_weights(sc, ops, patterns=PATTERNS):
    """[(label, weight)] of the scene: every pattern shared and per pose, smooth and half by :func:`sharp_weights`,
    edge-hot by :func:`edge_hot_seeds`"""
    seeds = edge_hot_seeds(sc.name, sc.device, ops) if "edge-hot" in patterns else (0, 0)
    out = []
    for label, w in all_weights(sc.B, sc.H, sc.W, sc.device, patterns, seeds):
        pattern = label.rsplit(" ", 2 if label.endswith("per pose") else 1)[0]
        if pattern in ("smooth", "half"):
            w = sharp_weights(sc.name, sc.device, ops, pattern, label.endswith("per pose"))
        out.append((label, w))
    return out


def check_sharpness(name, device, ops):
    """In float64 alone, before any kernel is looked at: the weights matter.  smooth, half, disc: at every pose
    the weighted value differs from the unweighted one by more than 100 value allowances and one of the six
    gradient outputs by more than 10 of its allowances.  edge-hot: without any one weighted ray the value or one
    gradient output moves by more than 4 allowances."""
    sc = F.scene(name, device, ops)
    one = torch.ones((), device=device)
    ones = torch.ones(1, sc.N, device=device)
    for x_label, x1 in fixed_images(sc):
        plain_v = wncc_of(sc, x1, ones)[:, 4]
        plain_g, _, _ = gradient_reference(sc, x1, ones, one, True)
        for label, w in scene_weights(sc, ops, ("smooth", "half", "disc")):
            if label.startswith("disc") and name == "1x2x3":
                assert bool((w == 1).all())  # (the ellipse covers all six pixels)
                continue
            v = wncc_of(sc, x1, w)[:, 4]
            want, own, fine = gradient_reference(sc, x1, w, one, True)
            dv = (v - plain_v).abs() / F.FLOOR
            dg = ((want - plain_g).abs() / F.allowance(want, own, fine)).amax(1)
            print(f"{name} x1 {x_label} {label}: value differs by {float(dv.min()):.3g} allowances, a gradient by "
                  f"{float(dg.min()):.3g}")
            assert bool((dv > 100).all()) and bool((dg > 10).all()), (name, x_label, label, float(dv.min()), float(dg.min()))
    seeds = edge_hot_seeds(name, device, ops)
    for per_pose in (False, True):
        least = edge_hot_least_move(sc, weights("edge-hot", sc.B, sc.H, sc.W, per_pose, device, seed=seeds[per_pose]))
        print(f"{name} edge-hot {'per pose' if per_pose else 'shared'} (seed {seeds[per_pose]}): the least visible "
              f"weighted ray moves an output by {least:.3g} allowances")
        assert least > 4, (name, per_pose, least)


# ------------------------------------------------------------------------------------------------ 1 forward
def check_forward(name, device, ops):
    """ddrr_wncc_siddon_forward in every call form against the definition; with ones, ddrr_siddon_ncc_forward's
    values to 1 float32 ulp."""
    sc = F.scene(name, device, ops)
    image = sc.img * sc.planes[0]
    for x_label, x1 in fixed_images(sc):
        for label, w in scene_weights(sc, ops):
            want, own = wncc_of(sc, x1, w), wncc_of(sc, x1, w, dtype=F32)
            mag = stats_mag(want)
            for form, wt in placements(w):
                for want_image in (False, True):
                    for want_sum in (False, True):
                        res = ops.siddon_wncc_forward(sc.aux, sc.img, x1, wt, NCC_EPS, want_image=want_image,
                                                      want_sum=want_sum)
                        ncc, stats, out = res[:3]
                        tag = f"{name} forward, x1 {x_label}, w {label} {form}, image {want_image}, sum {want_sum}"
                        F.hold(tag + ": stats", stats, want, own, mag)
                        assert torch.equal(ncc, stats[:, 4])
                        assert (out is None) if not want_image else torch.equal(out, image), tag
                        if want_sum:
                            total = float(res[3]) - float(ncc.double().sum())
                            print(f"{tag}: sum - float64 sum of the values = {total:.3g}")
                            assert abs(total) <= F.FLOOR * sc.B, tag
            if label.startswith("ones"):
                ncc0, stats0, _ = ops.siddon_ncc_forward(sc.aux, sc.img, x1, NCC_EPS)
                ncc, stats, _ = ops.siddon_wncc_forward(sc.aux, sc.img, x1, w, NCC_EPS)
                assert (F.ulps32(ncc, ncc0) <= 1).all() and (F.ulps32(stats[:, :5], stats0) <= 1).all()
                assert torch.equal(stats[:, 5], torch.full((sc.B,), float(sc.N), device=device))
        # an odd offset of the fixed image too (no 16-byte loads from it)
        w = weights("smooth", sc.B, sc.H, sc.W, True, device)
        _, stats_b, _ = ops.siddon_wncc_forward(sc.aux, sc.img, F.unaligned(x1), w, NCC_EPS)
        F.hold(f"{name} forward, x1 {x_label} odd offset", stats_b, wncc_of(sc, x1, w), wncc_of(sc, x1, w, dtype=F32),
               stats_mag(wncc_of(sc, x1, w)))


# ------------------------------------------------------------------------------------------------ 1 backward
def check_backward(name, device, ops):
    """ddrr_wncc_siddon_backward_pose against the written-out chain: two conventions, both length paths, g_out per
    pose and shared, a shared and a per-pose fixed image, every weight pattern from both placements."""
    for conv in ("ZXY", "ZYX"):
        sc = F.scene(name, device, ops, conv)
        per_pose = (torch.randn(sc.B, generator=torch.Generator().manual_seed(31)) + 0.25).to(device)
        for x_label, x1 in fixed_images(sc):
            for label, w in scene_weights(sc, ops):
                _, stats, _ = ops.siddon_wncc_forward(sc.aux, sc.img, x1, w, NCC_EPS)
                for g_label, g_out in (("per pose", per_pose), ("shared", torch.tensor(1.7, device=device))):
                    for path in (True, False):
                        want, own, fine = gradient_reference(sc, x1, w, g_out, path)
                        for form, wt in placements(w):
                            g_rot, g_xyz = ops.siddon_wncc_backward_pose(sc.aux, x1, wt, stats, g_out, **sc.entry,
                                                                         eps=sc.eps, with_img_path=path)
                            F.hold(f"{name} {conv} backward, x1 {x_label}, w {label} {form}, g_out {g_label}, length "
                                   f"path {path}", torch.cat([g_rot, g_xyz], 1), want, own, fine)


# ------------------------------------------------------------------------------------------------ 2 masked pixels
def poison(t, w):
    """`t` with NaN, Inf and 1e30 (in turn) wherever w == 0"""
    bad = torch.tensor([float("nan"), float("inf"), 1e30], device=t.device)[torch.arange(t.shape[-1], device=t.device) % 3]
    return torch.where(w.expand_as(t) == 0, bad.expand_as(t), t).contiguous()


def check_masked_pixels_are_not_read(name, device, ops):
    """NaN, Inf and 1e30 under w == 0 change no output bit: fused entries (fixed image) and image entries (both
    images; their gradients are exactly 0 there).  The empty pose: value 0, gradients 0, finite statistics."""
    sc = F.scene(name, device, ops)
    image = (sc.img * sc.planes[0]).contiguous()
    g_out = torch.linspace(0.5, 1.5, sc.B).to(device)
    for label, w in scene_weights(sc, ops, ("disc", "half", "one pose empty")):
        if not bool((w == 0).any()):
            continue
        # (a per-pose fixed image takes per-pose poison; the shared one only where the shared weight is 0)
        x1 = sc.x1_per_pose
        runs = []
        for fixed, moving in ((x1, image), (poison(x1, w), poison(image, w))):
            ncc, stats, out, total = ops.siddon_wncc_forward(sc.aux, sc.img, fixed, w, NCC_EPS, want_image=True,
                                                             want_sum=True)
            g = ops.siddon_wncc_backward_pose(sc.aux, fixed, w, stats, g_out, **sc.entry, eps=sc.eps)
            v, st = ops.wncc_forward(fixed, moving, w, NCC_EPS)
            g1, g2 = ops.wncc_backward(fixed, moving, w, st, g_out, True, True)
            runs.append((ncc, stats, out, total, *g, v, st, g1, g2))
        for k, (clean, dirty) in enumerate(zip(*runs)):
            assert torch.equal(clean, dirty), (name, label, k)
        assert torch.isfinite(torch.stack([t.abs().max() for t in runs[1]])).all()
        off = w.expand(sc.B, -1) == 0
        assert bool((runs[1][8][off] == 0).all()) and bool((runs[1][9][off] == 0).all()), (name, label)
        if w.shape[0] == 1 and sc.B > 1:
            shared = ops.siddon_wncc_forward(sc.aux, sc.img, poison(sc.x1_shared, w), w, NCC_EPS)
            clean = ops.siddon_wncc_forward(sc.aux, sc.img, sc.x1_shared, w, NCC_EPS)
            assert torch.equal(shared[0], clean[0]) and torch.equal(shared[1], clean[1])
        if label.startswith("one pose empty"):
            ncc, stats, g_rot, g_xyz, v, st = (runs[1][k] for k in (0, 1, 4, 5, 6, 7))
            for s in (stats, st):
                assert float(s[-1, 4]) == 0 and float(s[-1, 5]) == 0 and float(s[-1, 0]) == 0 == float(s[-1, 2])
                assert abs(float(s[-1, 1]) - NCC_EPS ** 0.5) <= 1e-9 and float(s[-1, 1]) == float(s[-1, 3])
            assert float(ncc[-1]) == 0 == float(v[-1])
            assert bool((g_rot[-1] == 0).all()) and bool((g_xyz[-1] == 0).all())
            assert bool((runs[1][8][-1] == 0).all()) and bool((runs[1][9][-1] == 0).all())


# ------------------------------------------------------------------------------------------------ 3 scale, repeat
def _every_entry(sc, ops, x1, w, g_out):
    image = (sc.img * sc.planes[0]).contiguous()
    ncc, stats, out, total = ops.siddon_wncc_forward(sc.aux, sc.img, x1, w, NCC_EPS, want_image=True, want_sum=True)
    g = ops.siddon_wncc_backward_pose(sc.aux, x1, w, stats, g_out, **sc.entry, eps=sc.eps)
    v, st = ops.wncc_forward(x1, image, w, NCC_EPS)
    g1, g2 = ops.wncc_backward(x1.expand(sc.B, -1).contiguous(), image, w, st, g_out, True, True)
    return dict(ncc=ncc, stats=stats, out=out, total=total, g_rot=g[0], g_xyz=g[1], v=v, st=st, g1=g1, g2=g2)


def check_scale_and_repeat(name, device, ops):
    """4 w gives the bits w gives (a power of two scales every sum exactly; Sw is 4 times as large), and every
    entry called twice gives the same bits: no atomics, nothing left over in the workspace."""
    sc = F.scene(name, device, ops)
    g_out = torch.linspace(0.5, 1.5, sc.B).to(device)
    for x_label, x1 in fixed_images(sc):
        for label, w in scene_weights(sc, ops):
            first, again, scaled = (_every_entry(sc, ops, x1, t, g_out) for t in (w, w, 4 * w))
            for key in first:
                assert torch.equal(first[key], again[key]), (name, x_label, label, key, "repeat")
                if key in ("stats", "st"):
                    assert torch.equal(first[key][:, :5], scaled[key][:, :5]), (name, x_label, label, key)
                    assert torch.equal(4 * first[key][:, 5], scaled[key][:, 5]), (name, x_label, label, key)
                else:
                    assert torch.equal(first[key], scaled[key]), (name, x_label, label, key, "4 w")


# ------------------------------------------------------------------------------------------------ 4 image entries
IMAGE_SHAPES = ((3, 1, 64, 80), (2, 1, 67, 61), (1, 1, 2, 3), (33, 1, 30, 26))
IMAGE_CASES = [(shape, setting) for shape in IMAGE_SHAPES for setting in ("mean350", "mean3000")]


def _evaluate(crit, fixed, moving, weight, wts, place=torch.clone):
    """(value (B), d / d moving, d / d fixed) of sum_b wts_b crit(fixed, moving, weight=weight)_b; a (1, ...) fixed
    image is `expand`ed over the batch"""
    a = place(fixed).detach().requires_grad_()
    x = place(moving).detach().requires_grad_()
    v = crit(a.expand(moving.shape[0], -1, -1, -1) if a.shape[0] == 1 else a, x, weight=place(weight))
    (v * wts).sum().backward()
    return S.as_numpy(v, x.grad, a.grad)


def _image_case(case, crit, ops, fixed, moving, weight, wts, entries, fig=None):
    with launches(ops) as names:
        k = _evaluate(crit, fixed, moving, weight, wts)
        k1 = _evaluate(crit, fixed, moving, weight, wts, place=S.off_by_one)
    assert set(entries) <= set(names), (case, entries, names)
    ref = S.unfused(crit)
    with S.composition(), launches(ops) as none:
        c32 = _evaluate(ref, fixed, moving, weight, wts)
        f64 = _evaluate(ref, fixed.double(), moving.double(), weight.double(), wts.double())
    assert not none, (case, none)
    own = fig is None
    fig = S.Figures(case) if own else fig
    for form, got in (("", k), (" off by one", k1)):
        fig.value(f"{case} value{form}", got[0], c32[0], f64[0])
        fig.grad(f"{case} d/d moving{form}", got[1], c32[1], f64[1])
        fig.grad(f"{case} d/d fixed{form}", got[2], c32[2], f64[2])
    if own:
        fig.done()


def check_image_entries(shape, setting, device, ops):
    """NormalizedCrossCorrelation2d()(x1, x2, weight=) on DRR-like images: every weight pattern, the fixed image
    expanded and per pose, aligned and off by one, against the composition in float64."""
    B, C, H, W = shape
    fixed, moving, wts = S.pair(B, C, H, W, setting, device)
    fixed_b = S.drr_like(B * C, H, W, S.FIXED_SEED + 10, setting).reshape(B, C, H, W).to(device)
    crit = M.NormalizedCrossCorrelation2d()
    fig = S.Figures(f"wncc {shape} {setting}")
    for label, w in all_weights(B, H, W, device):
        for x_label, x1 in (("expanded", fixed), ("per pose", fixed_b)):
            _image_case(f"{label}, x1 {x_label}", crit, ops, x1, moving, w.reshape(-1, 1, H, W), wts, WNCC_ENTRIES, fig)
    fig.done()


def check_composition_is_the_definition(device):
    """metrics.weighted_ncc, the reference of the image-entry and module-route checks, against this module's own
    :func:`wncc` in float64: values and, by autograd of both, the gradients to either image -- NaN under the mask
    included."""
    B, H, W = 3, 30, 26
    fixed, moving, wts = S.pair(B, 1, H, W, "mean350", device)
    x1 = fixed.double().expand(B, -1, -1, -1).clone()
    for label, w in all_weights(B, H, W, device):
        w4 = w.double().reshape(-1, 1, H, W)
        res = []
        for fn in (lambda a, x: M.weighted_ncc(a, x, w4, NCC_EPS),
                   lambda a, x: wncc(a.reshape(B, -1), x.reshape(B, -1), w4.reshape(-1, H * W).expand(B, -1), NCC_EPS)[:, 4]):
            a, x = poison(x1, w4).requires_grad_(), poison(moving.double(), w4).requires_grad_()
            v = fn(a, x)
            (v * wts.double()).sum().backward()
            res.append((v.detach(), a.grad, x.grad))
        for k, (mine, theirs) in enumerate(zip(*res)):
            assert bool(torch.isfinite(mine).all()), (label, k)
            assert float((mine - theirs).abs().max()) <= 1e-12 * max(1.0, float(theirs.abs().max())), (label, k)
        off = (w4 == 0).expand(B, 1, H, W)
        assert bool((res[0][1][off] == 0).all()) and bool((res[0][2][off] == 0).all()), label


def check_criteria_and_routes(device, ops):
    """The gradient and the multiscale criterion with a weight end to end; weight + patch_size raises; weight=None
    launches what the call without the keyword launches."""
    B, C, H, W = 3, 1, 64, 80
    for setting in ("mean350", "mean3000"):
        fixed, moving, wts = S.pair(B, C, H, W, setting, device)
        for pattern, per_pose in (("disc", False), ("smooth", True)):
            w = weights(pattern, B, H, W, per_pose, device).reshape(-1, 1, H, W)
            _image_case(f"gncc {setting} {pattern}", M.GradientNormalizedCrossCorrelation2d(sigma=1.0), ops, fixed,
                        moving, w, wts, ("ddrr_blur_sobel_forward", "ddrr_blur_sobel_backward") + WNCC_ENTRIES)
            _image_case(f"multiscale [None] {setting} {pattern}", M.MultiscaleNormalizedCrossCorrelation2d([None], [1.0]),
                        ops, fixed, moving, w, wts, WNCC_ENTRIES)
    w = torch.ones(1, 1, H, W, device=device)
    a = fixed.expand(B, -1, -1, -1)
    for crit in (M.NormalizedCrossCorrelation2d(patch_size=7), M.GradientNormalizedCrossCorrelation2d(patch_size=7),
                 M.MultiscaleNormalizedCrossCorrelation2d([None, 7], [0.5, 0.5])):
        with launches(ops) as names, pytest.raises(ValueError, match="weight"):
            crit(a, moving, weight=w)
        assert not [n for n in names if "ncc" in n], names
    with pytest.raises(ValueError, match="weight"):
        M.NormalizedCrossCorrelation2d()(a, moving, weight=torch.ones(1, H, W, device=device))
    for crit in (M.NormalizedCrossCorrelation2d(), M.GradientNormalizedCrossCorrelation2d(sigma=1.0),
                 M.MultiscaleNormalizedCrossCorrelation2d([None, 7], [0.5, 0.5])):
        with launches(ops) as without:
            v0 = crit(a, moving)
        with launches(ops) as with_none:
            v1 = crit(a, moving, weight=None)
        assert without == with_none and without and not any("wncc" in n for n in without), (without, with_none)
        # (the same kernels on the same inputs: the same bits, but for the patch kernel, whose workgroups add their
        # windows' sums to the pair's value with a float atomic each, in whatever order they finish)
        if "ddrr_ncc_patch_forward" in without:
            assert float((v0 - v1).abs().max()) <= 2e-6
        else:
            assert torch.equal(v0, v1)


# ------------------------------------------------------------------------------------------------ 5 module route
def check_module_route(device, ops):
    """DRR.ncc(..., weight=) with gradients wanted takes the ddrr_wncc_siddon_* entries; value and pose gradients
    within the fused entries' gate of the float64 composition (the float64 module's render, metrics.weighted_ncc,
    autograd), `own` being the float32 composition of the same; the fallbacks compose the same number."""
    sc = F.scene("3x30x26", device, ops)
    B, H, W = sc.B, sc.H, sc.W
    drr = copy.deepcopy(sc.drr)
    drr.renderer.brick_storage = "f32"
    d64 = copy.deepcopy(drr).to(F64)
    fixed = sc.x1_shared.reshape(1, 1, H, W)
    wts = torch.linspace(0.5, 1.5, B).to(device)
    kw = dict(parameterization="euler_angles", convention="ZXY")

    def leaves(dtype=F32):
        return sc.rot.to(dtype).clone().requires_grad_(), sc.xyz.to(dtype).clone().requires_grad_()

    def composed(module, dtype, w4, g_out):
        r, x = leaves(dtype)
        v = M.weighted_ncc(fixed.to(dtype).expand(B, -1, -1, -1), module(r, x, **kw), w4.to(dtype), NCC_EPS)
        (v * g_out.to(dtype)).sum().backward()
        return v.detach(), torch.cat([r.grad, x.grad], 1)

    for pattern, per_pose in (("smooth", False), ("disc", True), ("half", True)):
        w = weights(pattern, B, H, W, per_pose, device)
        w4 = w.reshape(-1, 1, H, W)
        for reduction in ("none", "sum"):
            g_out = wts if reduction == "none" else torch.ones(B, device=device)
            want_v, want_g = composed(d64, F64, w4, g_out)
            own_v, own_g = composed(drr, F32, w4, g_out)
            _, g, g_abs = wncc_of(sc, sc.x1_shared, w, g_out)
            _, fine = F.pose_gradient(sc, g, g_abs)
            r, x = leaves()
            with launches(ops) as names:
                val = drr.ncc(fixed, r, x, weight=w4, reduction=reduction)
                (val * wts).sum().backward() if reduction == "none" else val.backward()
            assert set(SIDDON_ENTRIES) <= set(names) and not any(n.startswith("ddrr_siddon_ncc") for n in names), names
            assert type(val.grad_fn).__name__.startswith("_EulerSiddonWnccFn")
            tag = f"DRR.ncc weight {pattern} {'per pose' if per_pose else 'shared'}, reduction {reduction}"
            values = val.detach() if reduction == "none" else drr.ncc_per_pose
            F.hold(tag + ": values", values, want_v, own_v, torch.ones_like(want_v))
            if reduction == "sum":
                assert abs(float(val.detach()) - float(want_v.sum())) <= max(2 * abs(float(own_v.double().sum() - want_v.sum())),
                                                                             F.FLOOR * B)
            F.hold(tag + ": gradients", torch.cat([r.grad, x.grad], 1), want_g, own_g, fine)
            # the fallbacks: nothing to differentiate; a weight that takes a gradient
            with torch.no_grad(), launches(ops) as names:
                v0 = drr.ncc(fixed, sc.rot, sc.xyz, weight=w4)
            assert not any(n in SIDDON_ENTRIES for n in names) and "ddrr_wncc_forward" in names, names
            with torch.no_grad():  # (the forward-only render walks differently: its own float32 composition)
                own_v0 = M.weighted_ncc(fixed.expand(B, -1, -1, -1), drr(sc.rot, sc.xyz, **kw), w4, NCC_EPS)
            F.hold(tag + ": no gradient wanted", v0, want_v, own_v0, torch.ones_like(want_v))
            r, x = leaves()
            wg = w4.clone().requires_grad_()
            with launches(ops) as names:
                v1 = drr.ncc(fixed, r, x, weight=wg)
                (v1 * g_out).sum().backward()
            assert not any("wncc" in n for n in names), names
            assert wg.grad is not None and bool(torch.isfinite(wg.grad).all())
            F.hold(tag + ": weight with a gradient, values", v1.detach(), want_v, own_v, torch.ones_like(want_v))
            F.hold(tag + ": weight with a gradient", torch.cat([r.grad, x.grad], 1), want_g, own_g, fine)
    if device.type == "cpu":  # a float64 module on the host composes the definition itself
        r, x = leaves(F64)
        v = d64.ncc(fixed.double(), r, x, weight=w4.double())
        assert v.dtype == F64 and float((v.detach() - want_v).abs().max()) <= 1e-12


# ------------------------------------------------------------------------------------------------ 6 registration
def _q(rot, xyz):
    """the pose error in tolerances: 0.01 rad / 0.5 mm"""
    return max(float((rot.detach().cpu() - lm_cases.TRUTH[0]).abs().max()) / 0.01,
               float((xyz.detach().cpu() - lm_cases.TRUTH[1]).abs().max()) / 0.5)


def occluded_scene(device):
    """lm_cases.convergence_scene with a bright bar over rows 10-17 of the fixed image and the weight that masks it"""
    drr, fixed = lm_cases.convergence_scene(device)
    occluded = fixed.clone()
    occluded[:, :, 10:18, :] = 2 * fixed.max()
    weight = torch.ones_like(fixed)
    weight[:, :, 10:18, :] = 0.0
    return drr, fixed, occluded, weight


def adam_loop(drr, objective, device, cap=250, dtype=F32, stop_at=None):
    """The Adam loop of lm_cases.check_convergence (1e-1 / 5e0, maximize) on `objective(rot, xyz)` -> (the
    trajectory [(rot, xyz) before every step], the smallest q and its iteration); stops once q <= stop_at."""
    start = [(lm_cases.TRUTH[k] + lm_cases.OFFSET[k]).to(device=device, dtype=dtype) for k in (0, 1)]
    reg = Registration(drr, start[0].clone(), start[1].clone(), parameterization="euler_angles", convention="ZXY")
    opt = torch.optim.Adam([{"params": [reg._rotation], "lr": 1e-1}, {"params": [reg._translation], "lr": 5e0}],
                           maximize=True)
    track, best = [], (float("inf"), 0)
    for it in range(1, cap + 1):
        track.append((reg._rotation.detach().clone(), reg._translation.detach().clone()))
        q = _q(reg.rotation, reg.translation)
        best = min(best, (q, it))
        if stop_at is not None and q <= stop_at:
            break
        opt.zero_grad()
        objective(reg._rotation, reg._translation).sum().backward()
        opt.step()
    return track, best


def check_registration(device, ops):
    """The masked run through DRR.ncc(weight=) on the occluded image reaches q <= 1 within 250 iterations, and the bar
    is not read: at poses recorded along that run, from ONE record per pose, the fused entries give the clean and
    the occluded fixed image the same value, statistics and pose gradient bit for bit -- so from the same render
    Adam takes the same step whichever image it is shown.  On the host build, where a render is reproducible, the
    whole trajectory of the masked run on the clean image is that of the occluded image bit for bit.  On the device
    the brick kernel sums a ray's record with float atomics: where more than two bricks add to one ray the last
    bits depend on their order, two runs on the SAME image end 0.03 rad / 1 mm apart (Adam's normalised steps carry
    the last bits on), and no comparison of two runs' trajectories says anything about the bar; there the clean
    run has to reach q <= 1 as well."""
    drr, fixed, occluded, weight = occluded_scene(device)
    run = lambda image, **kw: adam_loop(drr, lambda r, x: drr.ncc(image, r, x, convention="ZXY", weight=weight),  # noqa: E731
                                        device, **kw)
    with launches(ops) as names:
        track, (q, it) = run(occluded, stop_at=1.0)
    print(f"masked run on the occluded image: q = {q:.3g} at iteration {it}")
    assert set(SIDDON_ENTRIES) <= set(names)
    assert q <= 1.0, (q, it)
    # one record per recorded pose (every eighth and the last), both fixed images through the same entries
    picks = track[::8] + [track[-1]]
    rot, xyz = (torch.cat([p[k] for p in picks]).contiguous() for k in (0, 1))
    aux, args, kw, _ = lm_cases.render_record(drr, rot, xyz, "ZXY", ops)
    img = ops.pose_raygen_forward(rot, xyz, args["axes"], args["reorient34"], args["Ainv"], args["P"])[3]
    g_out, w = torch.linspace(0.5, 1.5, len(picks)).to(device), weight.reshape(1, -1)
    outs = []
    for image in (occluded, fixed):
        x1 = image.reshape(1, -1).contiguous()
        ncc, stats, _ = ops.siddon_wncc_forward(aux, img, x1, w, 1e-5)
        outs.append((ncc, stats, *ops.siddon_wncc_backward_pose(aux, x1, w, stats, g_out, **args, **kw)))
    for k, (a, b) in enumerate(zip(*outs)):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all()), k
    assert float(outs[0][2].abs().min(0).values.max()) > 0 and float(outs[0][0].min()) > 0.5
    if device.type == "cpu":
        clean, _ = run(fixed, cap=len(track))
        assert len(clean) == len(track)
        assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(track, clean))
    else:
        _, (q_clean, it_clean) = run(fixed, stop_at=1.0)
        print(f"masked run on the clean image: q = {q_clean:.3g} at iteration {it_clean}")
        assert q_clean <= 1.0, (q_clean, it_clean)


def check_scene_needs_the_mask(device, ops):
    """The unmasked float64 composition on the occluded image never gets below q = 5: the scene needs the mask."""
    drr, _, occluded, _ = occluded_scene(device)
    d64 = copy.deepcopy(drr).to(F64)
    crit = M.NormalizedCrossCorrelation2d()
    target = occluded.double()
    _, (q, it) = adam_loop(d64, lambda r, x: crit(target, d64(r, x, parameterization="euler_angles", convention="ZXY")),
                           device, dtype=F64)
    print(f"unmasked float64 run on the occluded image: closest approach q = {q:.3g} at iteration {it}")
    assert q >= 5.0, (q, it)


def check_graphed_iteration(device, ops):
    """GraphedIteration(..., weight=w): ten replays against ten eager iterations from the same start, under plain
    gradient ascent (torch.optim.SGD, maximize), whose step is lr times the gradient: the parameters after ten
    steps differ by lr times the sum of the ten gradients' differences.  Both routes run the same kernels on the
    same inputs; only the record's float atomics are summed in another order, which leaves each gradient within its
    gate of float64 -- `allowance`: max(2 x the float32 composition's error, 8 * 2^-24 fine) -- so two of them are
    at most two gates apart, and ten steps 10 * 2 * lr * allowance.  (Not Adam: its normalised step turns the sign of
    a gradient component near zero into +-lr, whatever the size of the difference.)  The gate is taken at the start
    pose in float64; the learning rates keep ten steps within 1e-3 rad / 0.1 mm of it."""
    from diffdrr_amd import GraphedIteration

    sc = F.scene("3x30x26", device, ops)
    drr = copy.deepcopy(sc.drr)
    drr.renderer.brick_storage = "f32"  # (eager and captured renders from the same bricks)
    H, W = sc.H, sc.W
    fixed = sc.x1_shared.reshape(1, 1, H, W).contiguous()
    weight = weights("disc", sc.B, H, W, False, device).reshape(1, 1, H, W)
    one = torch.ones((), device=device)
    want, own, fine = gradient_reference(sc, sc.x1_shared, weight.reshape(1, -1), one, True)
    allow = F.allowance(want, own, fine)
    crit = M.NormalizedCrossCorrelation2d()
    # lr: ten steps move a parameter by 10 lr |gradient|, at most 1e-3 rad / 0.1 mm
    lrs = (1e-4 / float(want[:, :3].abs().max()), 1e-2 / float(want[:, 3:].abs().max()))

    def fresh():
        reg = Registration(drr, sc.rot.clone(), sc.xyz.clone(), parameterization="euler_angles", convention="ZXY")
        return reg, torch.optim.SGD([{"params": [reg._rotation], "lr": lrs[0]},
                                     {"params": [reg._translation], "lr": lrs[1]}], maximize=True)

    reg, opt = fresh()
    for _ in range(10):
        opt.zero_grad()
        drr.ncc(fixed, reg._rotation, reg._translation, convention="ZXY", weight=weight).sum().backward()
        opt.step()
    eager = (reg.rotation.detach().clone(), reg.translation.detach().clone())
    reg, opt = fresh()
    step = GraphedIteration(reg, crit, opt, fixed, weight=weight)
    assert step.fused_similarity is True
    assert torch.equal(reg.rotation.detach(), sc.rot) and torch.equal(reg.translation.detach(), sc.xyz)
    for _ in range(10):
        loss = step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all()) and step.iterations_done == 10
    for label, a, b, start, lr, gate, g in (
            ("rotation", reg.rotation.detach(), eager[0], sc.rot, lrs[0], allow[:, :3], want[:, :3]),
            ("translation", reg.translation.detach(), eager[1], sc.xyz, lrs[1], allow[:, 3:], want[:, 3:])):
        err, tol, moved = (a - b).abs().double(), 10 * 2 * lr * gate, (a - start).abs().double()
        print(f"graphed against eager after ten steps, {label}: largest difference {float(err.max()):.3g}, largest "
              f"difference / allowed {float((err / tol).max()):.3g}; allowed / moved {float((tol / moved).max()):.3g}")
        assert bool((err <= tol).all()), (label, err, tol)
        # (the steps moved the parameters: the one with the largest gradient by about ten times lr times that gradient)
        assert 5 * lr * float(g.abs().max()) < float(moved.max()) < 20 * lr * float(g.abs().max()), (label, moved)


# ------------------------------------------------------------------------------------------------ layouts
def check_layout_errors(ops):
    """The ops refuse anything but the blocked record, and every other x1 / weight shape, without a launch."""
    B, N = 2, 24
    blocked = torch.zeros(ops.record_blocks(B, N), 80)
    img, x1, w = torch.ones(B, N), torch.ones(1, N), torch.ones(1, N)
    stats = torch.zeros(B, 6)
    pose = dict(source=torch.zeros(B, 1, 3), Mw=torch.zeros(B, 3, 4), Ainv=torch.zeros(3, 4), P=torch.zeros(N, 3),
                rot=torch.zeros(B, 3), xyz=torch.zeros(B, 3), axes=(2, 0, 1), reorient34=torch.zeros(3, 4))
    with launches(ops) as launched:
        for bad in (torch.zeros(B, N, 8), torch.zeros(7, B, N), torch.zeros(ops.record_blocks(B, N) + 1, 80),
                    torch.zeros(B * N * 5)):
            with pytest.raises(ValueError, match="aux"):
                ops.siddon_wncc_forward(bad, img, x1, w, NCC_EPS)
            with pytest.raises(ValueError, match="aux"):
                ops.siddon_wncc_backward_pose(bad, x1, w, stats, torch.ones(B), **pose)
        for bad in (torch.ones(N), torch.ones(1, N + 1), torch.ones(3, N), torch.ones(1, 1, N), torch.ones(B, 4, 6)):
            for fixed, weight, what in ((bad, w, "x1"), (x1, bad, "weight")):
                with pytest.raises(ValueError, match=what):
                    ops.siddon_wncc_forward(blocked, img, fixed, weight, NCC_EPS)
                with pytest.raises(ValueError, match=what):
                    ops.siddon_wncc_backward_pose(blocked, fixed, weight, stats, torch.ones(B), **pose)
                with pytest.raises(ValueError, match=what):
                    ops.wncc_forward(fixed, img, weight, NCC_EPS)
                with pytest.raises(ValueError, match=what):
                    ops.wncc_backward(fixed, img, weight, stats, torch.ones(B), True, True)
        with pytest.raises(ValueError, match="weight"):
            ops.wncc_forward(x1, img, w.double(), NCC_EPS)
    assert not launched
