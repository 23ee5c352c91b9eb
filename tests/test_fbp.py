"""FDK initialisation without a GPU: the taps, the host build of csrc/fbp_core.h against the definitions in
float64, the torch composition of ``fdk`` against ground truth, the errors, the dispatch rule and
``Reconstruction.from_fdk``."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import diffdrr_amd
from conftest import ROOT
from diffdrr_amd import DRR, Reconstruction, analytic, ops
from diffdrr_amd.data import synthetic_subject
from fbp_cases import (BACKPROJECTION_CASES, EPS, FDK_SCENES, KW, backprojection_case, definition_float64,
                       fdk_scene, orbit, quality)

EMU_SRC = os.path.join(ROOT, "tests", "emu", "fbp_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "_build", "libfbp_emu.so")


# ------------------------------------------------------------------------------------------------ ramp_taps
def test_ramp_taps_match_the_closed_form():
    for L in (1, 2, 7, 64):
        h = analytic.ramp_taps(L)
        assert h.dtype == torch.float64 and tuple(h.shape) == (2 * L - 1,)
        for n in range(-(L - 1), L):
            want = 0.25 if n == 0 else (0.0 if n % 2 == 0 else -1.0 / (math.pi * n) ** 2)
            assert float(h[n + L - 1]) == pytest.approx(want, rel=1e-15, abs=0.0), (L, n)
    with pytest.raises(ValueError):
        analytic.ramp_taps(0)
    with pytest.raises(ValueError):
        analytic.ramp_taps(8, window="shepp")


def test_ramp_taps_sum_to_zero_as_the_length_grows():
    # the ramp has no DC gain: 1/4 - (2 / pi^2) sum_{odd n < L} 1 / n^2 -> 0 like 1 / (pi^2 L)
    sums = [float(analytic.ramp_taps(L).sum()) for L in (16, 256, 4096)]
    assert sums[0] > sums[1] > sums[2] > 0
    for L, s in zip((16, 256, 4096), sums):
        assert s < 2.0 / (math.pi ** 2 * L), (L, s)
    assert abs(float(analytic.ramp_taps(4096, "hann").sum())) < 2.0 / (math.pi ** 2 * 4096)


def test_hann_taps_are_the_ram_lak_taps_convolved_with_a_quarter_half_quarter():
    L = 33
    wide = analytic.ramp_taps(L + 1).numpy()  # lags -L .. L
    want = np.convolve(wide, [0.25, 0.5, 0.25], mode="valid")  # lags -(L - 1) .. L - 1
    got = analytic.ramp_taps(L, "hann").numpy()
    assert got.shape == want.shape and np.abs(got - want).max() < 1e-16
    # ... which is the ramp's spectrum times 1/2 + 1/2 cos(pi f / f_Nyquist): check on the periodic sequence
    n = np.arange(-64, 64)
    ram = np.where(n == 0, 0.25, np.where(n % 2 == 0, 0.0, -1.0 / (np.pi * np.where(n == 0, 1, n)) ** 2))
    hann = 0.25 * np.roll(ram, 1) + 0.5 * ram + 0.25 * np.roll(ram, -1)
    f = np.fft.fftfreq(128)
    assert np.abs(np.fft.fft(np.fft.ifftshift(hann)) - np.fft.fft(np.fft.ifftshift(ram))
                  * (0.5 + 0.5 * np.cos(2 * np.pi * f))).max() < 1e-12


# ------------------------------------------------------------------------------------- host build of the core
@pytest.fixture(scope="module")
def emu():
    deps = [EMU_SRC, os.path.join(ROOT, "diffdrr_amd", "csrc", "fbp_core.h")]
    if not (os.path.exists(EMU_SO) and all(os.path.getmtime(d) <= os.path.getmtime(EMU_SO) for d in deps)):
        os.makedirs(os.path.dirname(EMU_SO), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-mfma", "-ffp-contract=off", EMU_SRC,
                        "-o", EMU_SO], check=True)
    lib = ctypes.CDLL(EMU_SO)
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.fbp_emu_filter.argtypes = [P, I, I, I, I, P, F, F, F, F, F, F, I, P]
    lib.fbp_emu_backproject.argtypes = [P, I, I, I, P, I, P, I, I, I, I]
    lib.fbp_emu_filter.restype = lib.fbp_emu_backproject.restype = None
    return lib


@pytest.mark.parametrize("name", sorted(BACKPROJECTION_CASES))
def test_core_backprojection_against_the_definition_in_float64(emu, name):
    case = backprojection_case(name)
    images, views = case["images"].contiguous(), case["views"].contiguous()
    B, H, W = images.shape
    out = case["prior"].clone() if case["accumulate"] else torch.full(case["shape"], float("nan"))
    emu.fbp_emu_backproject(images.data_ptr(), B, H, W, views.data_ptr(), int(case["distance_weight"]),
                            out.data_ptr(), *case["shape"], int(case["accumulate"]))
    want, bound = definition_float64(case)
    got = out.double().numpy() - (case["prior"].double().numpy() if case["accumulate"] else 0.0)
    assert np.isfinite(got).all()  # every voxel written
    err = np.abs(got - want)
    slack = EPS * np.abs(case["prior"].numpy()) * 2 if case["accumulate"] else 0.0  # (the add's own rounding)
    print(f"{name}: max error {err.max():.3e}, bound there {bound.flat[err.argmax()]:.3e}, "
          f"largest |value| {np.abs(want).max():.3e}, non-zero voxels {(want != 0).mean():.2f}")
    assert (err <= bound + slack).all(), float((err - bound - slack).max())
    assert (got[want == 0] == 0).all()  # nothing reaches a voxel that projects outside every view


def test_core_backprojection_cases_cover_what_they_are_meant_to():
    inside = definition_float64(backprojection_case("anisotropic_33_views"))[0]
    outside = definition_float64(backprojection_case("anisotropic_mostly_outside"))[0]
    assert (inside != 0).mean() > 0.9 and 0 < (outside != 0).mean() < 0.5
    case = backprojection_case("anisotropic_33_views")  # the view from inside the volume has voxels behind it
    depth = case["views"][33 // 2, 8:12].double()
    corners = [float(depth @ torch.tensor([i, j, k, 1.0], dtype=torch.float64))
               for i in (0, 32) for j in (0, 16) for k in (0, 39)]
    assert min(corners) < 0 < max(corners)


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 3, 5), (2, 40, 56), (1, 47, 63)])
def test_core_filter_against_the_definition_in_float64(emu, shape):
    B, H, W = shape
    g = torch.Generator().manual_seed(H * W)
    for axis in (0, 1):
        L = W if axis == 0 else H
        for window in ("ram-lak", "hann"):
            for cw in (0, 1):
                images = torch.randn(B, H, W, generator=g)
                taps = analytic.ramp_taps(L, window).float().contiguous()
                scale, geo = 1.0 / 0.7, (-27.3, 1.0, 19.0, -0.7, 1020.0)
                out = torch.full((B, H, W), float("nan"))
                emu.fbp_emu_filter(images.data_ptr(), B, H, W, axis, taps.data_ptr(), scale, *geo, cw, out.data_ptr())
                x = images.double().numpy()
                if cw:
                    u = geo[0] + np.arange(W) * geo[1]
                    v = geo[2] + np.arange(H) * geo[3]
                    x = x * (geo[4] / np.sqrt(geo[4] ** 2 + u[None, :] ** 2 + v[:, None] ** 2))
                want = np.zeros_like(x)
                t64 = taps.double().numpy()
                for b in range(B):
                    for line in range(H if axis == 0 else W):
                        sel = (b, line, slice(None)) if axis == 0 else (b, slice(None), line)
                        want[sel] = np.float32(scale) * np.convolve(x[sel], t64)[L - 1:2 * L - 1]
                floor = 8 * EPS * scale * np.abs(t64).sum() * np.abs(x).max()
                err = np.abs(out.double().numpy() - want).max()
                assert err <= floor, (axis, window, cw, err, floor)
                # the composition is the same definition
                comp = analytic.filter_composition(images.double(), axis, taps.double(), float(np.float32(scale)),
                                                   u0=geo[0], du=geo[1], v0=geo[2], dv=geo[3], sdd=geo[4],
                                                   cosine_weight=bool(cw))
                assert np.abs(comp.numpy() - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("name", ["one_voxel", "tiny_accumulate", "anisotropic_33_views", "anisotropic_mostly_outside"])
def test_backprojection_composition_is_the_definition(name):
    case = backprojection_case(name)
    want, bound = definition_float64(case)
    got = analytic.backproject_composition(case["images"].double(), case["views"].double(), case["shape"],
                                           case["distance_weight"]).numpy()
    assert (np.abs(got - want) <= bound).all()
    # ... and through the public entry, from the poses (float64 matrices, not rounded to fp32; what is left is
    # the float32 pose's 1e-7 of non-orthonormality in what "depth along the optical axis" means)
    pub = diffdrr_amd.backproject(case["drr"], case["images"].double(), case["rot"], case["xyz"],
                                  view_weights=case["views"][:, 12].double(),
                                  distance_weight=case["distance_weight"], **KW).numpy()
    assert np.abs(pub - want).max() <= 1e-6 * np.abs(want).max()
    prior = case["prior"].double()
    acc = diffdrr_amd.backproject(case["drr"], case["images"].double()[:, None], case["rot"], case["xyz"],
                                  view_weights=case["views"][:, 12].double(), distance_weight=case["distance_weight"],
                                  out=prior.clone(), accumulate=True, **KW)
    assert torch.allclose(acc, prior + torch.from_numpy(pub), rtol=0, atol=1e-12)


# --------------------------------------------------------------------------------- fdk against ground truth
@pytest.mark.parametrize("name", sorted(FDK_SCENES))
def test_fdk_composition_recovers_the_volume(name):
    drr, images, rot, xyz, truth = fdk_scene(name)
    volume = diffdrr_amd.fdk(drr, images, rot, xyz, **KW)
    assert volume.dtype == torch.float64 and volume.shape == truth.shape
    rmse, scale = quality(volume, truth)
    print(f"{name}: rmse / rmse(0) = {rmse:.3f}, least-squares scale = {scale:.3f}")
    assert rmse <= 0.2
    assert 0.95 <= scale <= 1.05
    # the filtered axis is the one tangent to the orbit
    orb = analytic.orbit_of(analytic.view_geometry(drr, rot, xyz, **KW))
    assert orb.axis == (1 if name == "row_tangent_orbit" else 0) and orb.tilt < 1e-3


def test_fdk_hann_window_and_explicit_taps():
    drr, images, rot, xyz, truth = fdk_scene("cube_32")
    hann = diffdrr_amd.fdk(drr, images, rot, xyz, window="hann", **KW)
    rmse, scale = quality(hann, truth)
    print(f"hann: rmse / rmse(0) = {rmse:.3f}, least-squares scale = {scale:.3f}")
    assert rmse <= 0.2 and 0.95 <= scale <= 1.05
    taps = diffdrr_amd.ramp_taps(64, "hann")
    assert torch.equal(diffdrr_amd.fdk(drr, images, rot, xyz, window=taps, **KW), hann)
    # the three layouts a DRR hands out, and a RigidTransform for the poses
    flat = diffdrr_amd.fdk(drr, images.reshape(60, 1, -1), diffdrr_amd.convert(rot, xyz, **KW), window="hann")
    assert torch.equal(flat, hann)
    assert torch.equal(diffdrr_amd.fdk(drr, images[:, 0], rot, xyz, window="hann", **KW), hann)
    # equal weights given by hand are the default's (to the float32 rounding of the orbit's angles)
    w = torch.full((60,), math.pi / 60, dtype=torch.float64)
    assert torch.allclose(diffdrr_amd.fdk(drr, images, rot, xyz, window="hann", view_weights=w, **KW), hann,
                          rtol=0, atol=1e-5 * float(hann.abs().max()))


# ------------------------------------------------------------------------------------------------- errors
def test_fdk_errors():
    drr, images, rot, xyz, _ = fdk_scene("cube_32")
    arc_rot, arc_xyz = orbit(20, 0, 0.0, math.radians(150))
    with pytest.raises(ValueError, match="not a\\s+full orbit"):
        diffdrr_amd.fdk(drr, images[:20], arc_rot, arc_xyz, **KW)
    short = diffdrr_amd.fdk(drr, images[:20], arc_rot, arc_xyz, view_weights=torch.full((20,), 0.1), **KW)
    assert torch.isfinite(short).all()  # (with weights of the caller's the arc is theirs to answer for)
    with pytest.raises(ValueError, match="at least 3 views"):
        diffdrr_amd.fdk(drr, images[:2], rot[:2], xyz[:2], **KW)
    sub = synthetic_subject((32, 32, 32), "phantom")
    with pytest.raises(ValueError, match="whole detector grids"):
        diffdrr_amd.fdk(DRR(sub, sdd=1020.0, height=48, width=64, delx=1.0, p_subsample=0.5), images, rot, xyz, **KW)
    with pytest.raises(ValueError, match="whole detector grids"):
        diffdrr_amd.backproject(DRR(sub, sdd=1020.0, height=48, width=64, delx=1.0, patch_size=8), images, rot, xyz,
                                **KW)
    for bad in (images[:, :, :40], images.reshape(60, -1), images.reshape(60, 1, 64, 48), images[:, 0, :, :, None]):
        with pytest.raises(ValueError, match="images must be"):
            diffdrr_amd.fdk(drr, bad, rot, xyz, **KW)
    with pytest.raises(ValueError, match="images for"):
        diffdrr_amd.fdk(drr, images[:30], rot, xyz, **KW)
    tilted = rot.clone()
    tilted[:, 2] = math.radians(20)  # the detector turned about its optical axis
    with pytest.raises(ValueError, match="degrees out of it"):
        diffdrr_amd.fdk(drr, images, tilted, xyz, **KW)
    assert analytic.orbit_of(analytic.view_geometry(drr, tilted, xyz, **KW)).tilt == pytest.approx(20.0, abs=1e-3)
    with pytest.raises(ValueError, match="view_weights"):
        diffdrr_amd.fdk(drr, images, rot, xyz, view_weights=torch.ones(7), **KW)
    with pytest.raises(ValueError):
        diffdrr_amd.fdk(drr, images, rot, xyz, window="shepp", **KW)
    with pytest.raises(TypeError, match="calibration"):
        diffdrr_amd.fdk(drr, images, rot, xyz, calibration=None, **KW)


# ------------------------------------------------------------------------------------------------ dispatch
def test_dispatch_rule(monkeypatch):
    drr, images, rot, xyz, _ = fdk_scene("cube_32")
    calls = []

    def filter_(images, axis, taps, scale, **kw):
        calls.append(("filter", images.dtype, axis, kw["cosine_weight"], taps.dtype))
        return images.clone()

    def backproject_(images, views, shape, *, distance_weight, out, accumulate):
        calls.append(("backproject", views.dtype, tuple(views.shape), distance_weight, accumulate))
        return torch.zeros(shape) if out is None else out

    monkeypatch.setattr(ops, "fbp_filter", filter_)
    monkeypatch.setattr(ops, "fbp_backproject", backproject_)
    # CPU tensors and float64 never reach the kernels
    diffdrr_amd.fdk(drr, images, rot, xyz, **KW)
    diffdrr_amd.fdk(drr, images.float(), rot, xyz, **KW)
    diffdrr_amd.backproject(drr, images.float(), rot, xyz, **KW)
    assert calls == []
    monkeypatch.setattr(ops, "on_device", lambda t: True)  # "device" tensors
    diffdrr_amd.fdk(drr, images, rot, xyz, **KW)  # float64 on the device: the composition
    strided = images.float().permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    diffdrr_amd.backproject(drr, strided, rot, xyz, **KW)  # not contiguous: the composition
    assert calls == []
    diffdrr_amd.fdk(drr, images.float(), rot, xyz, **KW)
    assert calls == [("filter", torch.float32, 0, True, torch.float32),
                     ("backproject", torch.float32, (60, 16), True, False)]
    del calls[:]
    out = torch.zeros(32, 32, 32)
    assert diffdrr_amd.backproject(drr, images.float(), rot, xyz, out=out, accumulate=True, **KW) is out
    assert calls == [("backproject", torch.float32, (60, 16), False, True)]
    del calls[:]
    diffdrr_amd.backproject(drr, images.float(), rot, xyz, out=out.double(), **KW)  # a float64 target: composition
    assert calls == []


def test_ops_check_their_arguments_before_any_launch(monkeypatch):
    monkeypatch.setattr(ops, "_require_gpu", lambda t: None)
    monkeypatch.setattr(ops, "_launch_on", lambda *a: pytest.fail("launched"))
    img, taps = torch.zeros(2, 4, 6), torch.zeros(11)
    for bad in (lambda: ops.fbp_filter(img.double(), 0, taps), lambda: ops.fbp_filter(img, 2, taps),
                lambda: ops.fbp_filter(img, 1, taps), lambda: ops.fbp_filter(img[0], 0, taps),
                lambda: ops.fbp_filter(img, 0, taps, out=torch.zeros(2, 4, 5)),
                lambda: ops.fbp_filter(torch.zeros(1, 1, 4097), 0, torch.zeros(8193)),
                lambda: ops.fbp_backproject(img, torch.zeros(2, 12), (2, 2, 2)),
                lambda: ops.fbp_backproject(img, torch.zeros(2, 16)),
                lambda: ops.fbp_backproject(img, torch.zeros(2, 16), (2, 2, 2), accumulate=True),
                lambda: ops.fbp_backproject(img, torch.zeros(2, 16), (2, 2, 2), out=torch.zeros(2, 2, 3)),
                lambda: ops.fbp_backproject(img, torch.zeros(2, 16), (1, 1, 65536))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError, match="CPU"):
        monkeypatch.undo()
        ops.fbp_filter(img, 0, taps)


# ------------------------------------------------------------------------------------ public names, from_fdk
def test_public_names():
    for name in ("fdk", "backproject", "fbp_filter", "ramp_taps"):
        assert getattr(diffdrr_amd, name) is getattr(analytic, name)
    assert callable(Reconstruction.from_fdk)


def test_from_fdk_clamps_and_copies():
    drr, images, rot, xyz, truth = fdk_scene("cube_32")
    start = diffdrr_amd.fdk(drr, images, rot, xyz, **KW)
    assert float(start.min()) < 0 < 0.5 < float(start.max())  # (the ramp rings: there is something to clamp)
    recon = Reconstruction.from_fdk(drr, images, rot, xyz, upper=0.5, **KW)
    assert isinstance(recon.density, torch.nn.Parameter) and recon.density.dtype == torch.float32
    assert (recon.lower, recon.upper) == (0.0, 0.5)
    assert torch.equal(recon.density.detach(), start.clamp(0.0, 0.5).float())
    assert float(recon.density.detach().min()) == 0.0 and float(recon.density.detach().max()) == 0.5
    free = Reconstruction.from_fdk(drr, images, rot, xyz, window="hann", lower=None, **KW)
    assert torch.equal(free.density.detach(), diffdrr_amd.fdk(drr, images, rot, xyz, window="hann", **KW).float())
    assert free.density.data_ptr() != drr.density.data_ptr() and not torch.equal(free.density.detach(), drr.density)
    rmse, _ = quality(recon.density.detach().clamp(max=10), truth.clamp(max=0.5))
    assert rmse < 0.2
