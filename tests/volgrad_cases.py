"""Scenes, incoming gradients and the float64 reference for the brick volume gradients
(ddrr_siddon_backward_volume_bricks, ddrr_trilinear_backward_volume_bricks and their two channel
variants; csrc/bricks.hip LdsAbsAddT / LdsAbsAddHigh, volgrad_prepare_kernel).

The four entries accumulate a brick of the gradient in LDS as int32 fixed point whose scale is
chosen once per launch from a bound on the largest sum a voxel can receive.  What the scale, the
rounding of every add and the switch to float accumulators do to a voxel is only visible against a
reference that knows, per voxel, how many adds it received and how large they were.  This module
has that reference: a plain float64 walk of the same float32 rays (`walk`), pinned to the oracle by
tests/test_volgrad_cases.py, which returns per voxel

    g64  the gradient,
    A    sum of |contribution|  (what the accumulator's bound must cover),
    T    the absolute rounding scale of float32 arithmetic: a Siddon contribution g L dalpha carries
         the absolute error of a difference of two O(1) alphas, so its error scales with |g| L; a
         marcher's corner contribution g L step w with |g| L step,
    n    the number of adds (hits with a weight), so that n / 2 quanta bound the rounding of the fixed
         point.

Everything here is numpy / CPU torch: the rays are made once, on the CPU, and the device tests upload
these very float32 arrays.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import torch

import oracle

SHIFT, EPS = 0.5, 1e-8  # voxel_shift and eps as the renderers pass them
KINDS = ("siddon", "marcher", "siddon_channels", "marcher_channels")
PATTERNS = ("G1", "G2", "G3", "G3p", "G4")
N_LABELS, N_CHANNELS = 9, 7  # labels 7 and 8 have no channel: they weigh 0
FIXED_COUNTS = {"siddon": 2.0e9, "marcher": 2.0e9, "siddon_channels": 7.8e6, "marcher_channels": 2.0e9}

# rho32 = max_v |per-ray float32 kernel - g64| / T_v: the yardstick of float32 arithmetic in the gate
# of tests/test_gpu_volume_gradient_bricks.py.  The cap keeps a broken yardstick from widening the gate:
# 4 x the largest value measured on an MI355X over every (scene, entry, pattern), per renderer.  (Siddon: a few
# units of 2^-24 = 6e-8, the error of a difference of two alphas.  The marcher: a corner weight is a product of
# fractions of index coordinates of up to 70 that carry ~100 * 2^-24 themselves.)
RHO32_MEASURED = {"siddon": 1.398e-7, "marcher": 1.344e-5}  # (far3 Siddon G4, thick marcher G4)
RHO32_CAP = {k: 4 * v for k, v in RHO32_MEASURED.items()}

# name -> (volume, detector, rot, xyz, x0, y0, fixed path expected)
V1 = dict(dims=(40, 70, 33), spacing=(1.0, 1.5, 2.0), n_points=70)
V2 = dict(dims=(24, 24, 9), spacing=(0.5, 0.5, 5.0), n_points=40)
DET1 = dict(sdd=300.0, height=24, width=31, delx=2.0)
FAR3 = ([[0.01, 0.02, -0.01], [0.6, -0.4, 0.9], [1.5, 0.2, 0.1]],
        [[0.3, 200.0, 0.2], [4.0, 180.0, -6.0], [1.0, 210.0, 2.0]])
# The y face of V1 is 52.5 mm from the centre and a voxel is 1.5 mm deep there: the source of `near` is 1.5
# voxels from the face, that of `near_float` -- 1.5 mm closer -- 0.5 (the float path: no bound within one voxel
# of the volume).
# A pixel of 12 mm keeps the bound on the rays through one voxel (volgrad_prepare_kernel's R) under 16384
# for the marcher too with the source that close; at the 2 mm of the other scenes R alone would force the
# float path long before the one-voxel rule does.
NEAR_DET = dict(sdd=300.0, height=24, width=31, delx=12.0)
# (Neither this pose nor that of `switch` is axis-aligned and centred: in such a pose rays cross two planes at
# exactly the same alpha, float32 and float64 round the coincidence apart differently, and the float32 walks
# deposit grazing segments of ~1e-8 of a ray in voxels the float64 walk never enters.)
NEAR_ROT = [0.03, -0.02, 0.05]
SWITCH_DET = dict(sdd=300.0, height=16, width=16, delx=1.0)
SWITCH_POSE = ([0.04, -0.03, 0.02], [1.7, 240.0, -1.1])
# ceil(R) of one pose of `switch` as the device reports it (word 2 of launch_ws after a one-pose launch),
# and B_lo = floor(16384 / ceil(R)): B_lo poses still take the fixed path, B_lo + 1 the float path.
SWITCH_R = {"siddon": 58, "marcher": 173}  # (R = 57.16 and 172.15: B_lo = 282 and 94)

SCENES = {
    "far3": (V1, DET1, *FAR3, 0.0, 0.0, True),
    "inside": (V1, DET1, [[0.2, 0.1, 0.0], [0.0, 0.3, 0.1]], [[2.0, 5.0, -3.0], [0.0, 40.0, 1.0]], 0.0, 0.0, False),
    "near": (V1, NEAR_DET, [NEAR_ROT], [[1.3, 54.763, -0.7]], 0.0, 0.0, True),
    "near_float": (V1, NEAR_DET, [NEAR_ROT], [[1.3, 53.263, -0.7]], 0.0, 0.0, False),
    "offcentre": (V1, DET1, [FAR3[0][1]], [FAR3[1][1]], 25.0, -20.0, True),
    "thick": (V2, dict(sdd=300.0, height=20, width=20, delx=0.5),
              [[0.1, 0.2, np.pi / 4], [-0.3, 0.1, -np.pi / 4]], [[1.0, 150.0, 2.0], [-2.0, 160.0, 1.0]], 0.0, 0.0,
              True),
}
SCENE_NAMES = tuple(SCENES) + ("switch_lo", "switch_hi")


def renderer_of(kind):
    return kind.split("_")[0]


def switch_poses(kind, name):
    b_lo = 16384 // SWITCH_R[renderer_of(kind)]
    return b_lo if name == "switch_lo" else b_lo + 1


def _volume(dims):
    return torch.rand(*dims, generator=torch.Generator().manual_seed(1))


def _labels(dims):
    g = torch.Generator().manual_seed(2)
    coarse = torch.randint(0, N_LABELS, tuple(d // 8 + 1 for d in dims), generator=g)
    for ax in range(3):
        coarse = coarse.repeat_interleave(8, ax)
    return coarse[: dims[0], : dims[1], : dims[2]].contiguous().to(torch.uint8).numpy()


@functools.lru_cache(maxsize=None)
def scene(name, kind="siddon"):
    """The float32 rays of a scene in voxel coordinates, made on the CPU.  `kind` only matters for the two
    `switch` scenes (the number of poses depends on the renderer's bound).
    -> namespace: dims, volume, labels, source (U, 1, 3), target (U, N, 3), img (U, N) of the U distinct poses,
    pose_of (B,) which of them each pose of the batch is, det, n_points, amin, amax (float32), fixed"""
    from diffdrr_amd import DRR, convert
    from diffdrr_amd.data import make_subject

    if name.startswith("switch"):
        vol, det, rot, xyz, x0, y0, fixed = V1, SWITCH_DET, [SWITCH_POSE[0]], [SWITCH_POSE[1]], 0.0, 0.0, \
            name == "switch_lo"
        B = switch_poses(kind, name)
    else:
        vol, det, rot, xyz, x0, y0, fixed = SCENES[name]
        B = len(rot)
    density = _volume(vol["dims"])
    drr = DRR(make_subject(density, spacing=vol["spacing"]), x0=x0, y0=y0, **det)
    with torch.no_grad():
        pose = convert(torch.tensor(rot, dtype=torch.float32), torch.tensor(xyz, dtype=torch.float32),
                       parameterization="euler_angles", convention="ZXY")
        source, target = drr.detector(pose, None)
        img = (target - source).norm(dim=-1)
        source, target = drr.affine_inverse(source), drr.affine_inverse(target)
    sc = SimpleNamespace(name=name, dims=vol["dims"], volume=density.numpy(), labels=_labels(vol["dims"]),
                         source=source.contiguous().numpy(), target=target.contiguous().numpy(),
                         img=img.contiguous().numpy(), det=(det["height"], det["width"]),
                         n_points=vol["n_points"], fixed=fixed, B=B)
    U = sc.source.shape[0]
    sc.pose_of = np.arange(B) if U == B else np.zeros(B, np.int64)
    sc.N = sc.target.shape[1]
    lo, hi = oracle.alpha_minmax(sc.source, sc.target, sc.dims, voxel_shift=SHIFT, eps=EPS)  # (float32)
    sc.amin, sc.amax = np.float32(lo.min()), np.float32(hi.max())
    return sc


def batch(sc):
    """The (B, ...) float32 arrays a launch takes."""
    return sc.source[sc.pose_of], sc.target[sc.pose_of], sc.img[sc.pose_of]


def grad_out(sc, kind, pattern, seed=7):
    """-> grad_out float32 (B, N) or (B, C, N), and `bright` (B, N): the pixels that are not faint."""
    H, W = sc.det
    shape = (sc.B, N_CHANNELS, H, W) if kind.endswith("channels") else (sc.B, H, W)
    g = torch.Generator().manual_seed(seed + PATTERNS.index(pattern))
    r = torch.randn(*shape, generator=g).numpy()
    bright = np.ones((sc.B, H, W), bool)
    if pattern == "G2":
        r = np.ones_like(r)
    elif pattern in ("G3", "G3p"):
        r[..., W // 2:] *= 1e-4 if pattern == "G3" else 1e-6
        bright[..., W // 2:] = False
    elif pattern == "G4":
        r *= 1e-3
        r[..., H // 2, W // 3] = 1e3  # (every pose, every channel)
        bright[:] = False
        bright[:, H // 2, W // 3] = True
    return np.ascontiguousarray(r.reshape(*shape[:-2], H * W), dtype=np.float32), bright.reshape(sc.B, H * W)


# ------------------------------------------------------------------------------------ the float64 walk

def _grid_coord(x, D):
    g = 2.0 * (x + SHIFT) / D - 1.0  # the reference normalises,
    return ((g + 1.0) * D - 1.0) / 2.0  # grid_sample (align_corners=False) un-normalises


def _flat(ix, dims):
    """Flat voxel index of integer-valued float coordinates (..., 3), -1 outside the volume."""
    D = np.asarray(dims, np.float64)
    inside = ((ix >= 0) & (ix < D)).all(-1)
    i = np.where(inside[..., None], ix, 0).astype(np.int64)
    return np.where(inside, (i[..., 0] * dims[1] + i[..., 1]) * dims[2] + i[..., 2], -1)


def _siddon_hits(sc, u):
    """Every plane crossing of the rays of pose u, sorted; the segments' midpoints mapped to a voxel."""
    s, t, L = (a[u].astype(np.float64) for a in (sc.source, sc.target, sc.img))
    d = t - s + EPS  # (N, 3)
    alphas = [((np.arange(sc.dims[a] + 1) - SHIFT)[None, :] - s[0, a]) / d[:, a:a + 1] for a in range(3)]
    alphas = np.sort(np.concatenate(alphas, 1), 1)
    a0, a1 = alphas[:, :-1], alphas[:, 1:]
    mid = (a0 + a1) / 2.0
    x = s[0] + mid[..., None] * d[:, None, :]
    ix = np.rint(np.stack([_grid_coord(x[..., a], sc.dims[a]) for a in range(3)], -1))  # (half to even)
    flat = _flat(ix, sc.dims)
    da = a1 - a0
    lab = np.where(flat >= 0, sc.labels.reshape(-1)[np.maximum(flat, 0)], 0)
    return dict(flat=flat, coef=L[:, None] * da, tscale=np.broadcast_to(L[:, None], da.shape), lab=lab,
                size=da * np.linalg.norm(d, axis=1)[:, None])


def _reference_nearest(sc, u):
    """The nearest voxel of every sample of pose u, (N, P, 3).  This one lookup is discontinuous -- a sample on a
    voxel boundary belongs to one label or the other -- and the reference decides it by its own chain of separately
    rounded float32 tensor operations (alphas = linspace * span + alphamin, x = s + alpha d, normalise, grid_sample's
    un-normalise, round half to even), which csrc/trilinear_core.h march_exact_coord restates.  So the walk takes
    this decision, and nothing else, in float32: a float64 lookup would define a different function."""
    f = np.float32
    P, m = sc.n_points, np.arange(sc.n_points)
    lstep = f(1) / f(P - 1)
    lin = np.where(m < P // 2, m.astype(f) * lstep, f(1) - (P - 1 - m).astype(f) * lstep).astype(f)
    al = lin * f(sc.amax - sc.amin) + sc.amin
    s, t = sc.source[u, 0], sc.target[u]
    d = (t - s) + f(EPS)
    x = s[None, None, :] + al[None, :, None] * d[:, None, :]
    D = np.asarray(sc.dims, f)
    nrm = f(2) * (x + f(SHIFT)) / D + f(-1)
    un = ((nrm + f(1)) * D + f(-1)) / f(2)
    assert un.dtype == f
    return np.rint(un).astype(np.float64)


def _marcher_hits(sc, u):
    """The n_points samples of [alphamin, alphamax] of the rays of pose u, eight corners each."""
    s, t, L = (a[u].astype(np.float64) for a in (sc.source, sc.target, sc.img))
    d = t - s + EPS
    span = float(sc.amax) - float(sc.amin)
    step = span / (sc.n_points - 1)
    al = oracle.linspace01(sc.n_points).astype(np.float64) * span + float(sc.amin)  # (P,)
    x = s[0] + al[None, :, None] * d[:, None, :]  # (N, P, 3)
    g = np.stack([_grid_coord(x[..., a], sc.dims[a]) for a in range(3)], -1)
    f = np.floor(g)
    frac = g - f
    near = _flat(_reference_nearest(sc, u), sc.dims)  # the sample's nearest voxel: its label selects the channel
    slab = np.where(near >= 0, sc.labels.reshape(-1)[np.maximum(near, 0)], 0)  # (0 outside the volume)
    flats, ws = [], []
    for c in range(8):
        o = np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], np.float64)
        w = np.where(o > 0, frac, 1.0 - frac)
        ws.append(w[..., 0] * w[..., 1] * w[..., 2])
        flats.append(_flat(f + o, sc.dims))
    flat, w = np.stack(flats, -1), np.stack(ws, -1)  # (N, P, 8)
    N = flat.shape[0]
    k = L[:, None, None] * step
    return dict(flat=flat.reshape(N, -1), coef=(k * w).reshape(N, -1),
                tscale=np.broadcast_to(k, w.shape).reshape(N, -1),
                lab=np.broadcast_to(slab[..., None], w.shape).reshape(N, -1), size=w.reshape(N, -1))


_hit_cache = {}


def hits(sc, renderer, u=0):
    """The hits of the rays of distinct pose u, each (N, K): `flat` voxel (-1: none), `coef` (the contribution
    is the ray's weight times it), `tscale`, `lab` (the label that selects the weight's channel) and `size`
    (Siddon: the segment's length in voxels; marcher: the corner's weight)."""
    key = (sc.name, sc.B, renderer, u)
    if key not in _hit_cache:
        _hit_cache[key] = (_siddon_hits if renderer == "siddon" else _marcher_hits)(sc, u)
    return _hit_cache[key]


def walk(sc, kind, go, bright=None):
    """The float64 volume gradient of `kind` for grad_out `go` on the scene's rays.
    -> namespace of (Dx, Dy, Dz) float64 arrays: g64, A, T, n and, with `bright` (B, N), nb: the adds that come
    from bright pixels."""
    renderer, channels = renderer_of(kind), kind.endswith("channels")
    nvox = int(np.prod(sc.dims))
    out = {k: np.zeros(nvox) for k in ("g64", "A", "T", "n", "nb")}
    go = np.asarray(go, np.float64)
    for u in range(sc.source.shape[0]):
        poses = np.nonzero(sc.pose_of == u)[0]
        h = hits(sc, renderer, u)
        flat, lab = h["flat"], h["lab"]
        n_ray = np.arange(flat.shape[0])[:, None]
        gsum, gabs = go[poses].sum(0), np.abs(go[poses]).sum(0)  # poses that share their rays: summed first
        if channels:
            pad = np.zeros((1, gsum.shape[1]))
            row = np.minimum(lab, N_CHANNELS)  # labels without a channel weigh 0
            wsum, wabs = np.concatenate([gsum, pad])[row, n_ray], np.concatenate([gabs, pad])[row, n_ray]
            counted = (flat >= 0) & (lab < N_CHANNELS)
        else:
            wsum, wabs = gsum[:, None], gabs[:, None]
            counted = flat >= 0
        counted = counted & (h["coef"] > 0)
        idx = flat[counted]
        shape = flat.shape
        for key, val in (("g64", wsum * h["coef"]), ("A", wabs * h["coef"]), ("T", wabs * h["tscale"]),
                         ("n", np.full(shape, float(len(poses)))),
                         ("nb", None if bright is None else np.broadcast_to(
                             bright[poses].sum(0).astype(np.float64)[:, None], shape))):
            if val is not None:
                np.add.at(out[key], idx, np.broadcast_to(val, shape)[counted])
    return SimpleNamespace(**{k: v.reshape(sc.dims) for k, v in out.items()})


def oracle_volume_gradient(sc, kind, go):
    """The oracle's g_volume on the float64 casts of the same inputs (None: the oracle has no such entry)."""
    s, t, L = (a.astype(np.float64) for a in batch(sc))
    vol, go = sc.volume.astype(np.float64), np.asarray(go, np.float64)
    kw = dict(voxel_shift=SHIFT, eps=EPS)
    if kind == "siddon":
        return oracle.siddon(vol, s, t, L, grad_out=go, want_volume_grad=True, **kw)["g_volume"]
    if kind == "marcher":
        return oracle.trilinear(vol, s, t, L, n_points=sc.n_points, alphamin=float(sc.amin), alphamax=float(sc.amax),
                                grad_out=go, want_volume_grad=True, **kw)["g_volume"]
    if kind == "siddon_channels":
        return oracle.siddon_channels_grad(vol, sc.labels, s, t, L, go, **kw)["g_volume"]
    return None


def ray_voxels(sc, kind, b, n, min_size):
    """The voxels that ray n of pose b contributes to with a weight: -> (those with a hit of at least `min_size`,
    everything within one voxel of any of its hits), boolean volumes."""
    h = hits(sc, renderer_of(kind), int(sc.pose_of[b]))
    flat, size, lab = h["flat"][n], h["size"][n], h["lab"][n]
    ok = flat >= 0
    big = ok & (size >= min_size) & ((lab < N_CHANNELS) | (not kind.endswith("channels")))
    sure = np.zeros(int(np.prod(sc.dims)), bool)
    sure[flat[big]] = True
    any_hit = np.zeros(int(np.prod(sc.dims)), bool)
    any_hit[flat[ok]] = True
    any_hit = any_hit.reshape(sc.dims)
    p = np.pad(any_hit, 1)
    close = np.zeros_like(any_hit)
    for dx in range(3):
        for dy in range(3):
            for dz in range(3):
                close |= p[dx:dx + sc.dims[0], dy:dy + sc.dims[1], dz:dz + sc.dims[2]]
    return sure.reshape(sc.dims), close


def source_gap(sc, u=0):
    """Distance from the source of pose u to the volume's box in voxels (volgrad_prepare_kernel's rho)."""
    s = sc.source[u, 0].astype(np.float64)
    hi = np.asarray(sc.dims, np.float64) - SHIFT
    return float(np.linalg.norm(np.maximum(np.maximum(-SHIFT - s, s - hi), 0.0)))


def rays_through_a_voxel(sc, renderer, u=0):
    """volgrad_prepare_kernel's bound R on the rays of pose u that can cross one voxel, in float64: ceil(R) is
    what a pose adds to n_sum.  inf within one voxel of the volume."""
    s, t = sc.source[u, 0].astype(np.float64), sc.target[u].astype(np.float64)
    rho, W = source_gap(sc, u), sc.det[1]
    e_min = min(np.linalg.norm(t[W] - t[0]), np.linalg.norm(t[1] - t[0]))
    reach = max(np.linalg.norm(t[0] - s), np.linalg.norm(t[-1] - s))
    if not (rho > 1.0 and e_min > 0.0):
        return np.inf
    return ((3.4642 if renderer == "marcher" else 1.7321) * reach / (rho * e_min) + 2.0) ** 2
