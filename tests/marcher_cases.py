"""What tests/test_marcher.py (host emulation) and tests/test_gpu_marcher.py (MI355X) share: scenes, the float64
reference, the float32 yardstick, the per-pixel scales and the checks of the marcher's brick entries
(ddrr_trilinear_forward_bricks with and without its record, ddrr_trilinear_backward_rays, the two channel variants)
and of the per-ray entries they are compared with (ddrr_trilinear_forward / _backward), written once for either
device.  Every check takes (device, ops) as lm_cases.check_* do.

Reference: oracle.trilinear in float64 on the scene's float32 rays, volume and range (the sources expanded per ray, so
that g_source comes back per ray; the pair g_alpha, which the oracle sums over the rays, from one call per ray).
Yardstick of float32 arithmetic: the same calls in float32.  rho32 = max_p |oracle32 - oracle64| / S_p per quantity,
measured on the CPU, from the oracle alone.  Its largest value over every case is written down (RHO32_MEASURED) and
capped at 4 x that, so that a broken yardstick cannot widen a gate; a case is gated with the rho32 of its OWN rays,
which is never more: the constructed scenes lose 1 .. 8 x 2^-24 and are held to that, not to what a volume one voxel
thick seen from 200 voxels away loses (3000 x 2^-24).

Gate, for every pixel p of every entry:   |kernel - oracle64| <= 2 rho32 S_p + 8 * 2^-24 S_p.

The scales S_p are sums of magnitudes over the float64 sample positions g_m = s + alpha_m d + shift - 1/2:

    A_m     the zero-padded trilinear interpolant of |V| at g_m, plus the steepest slope of the interpolant there per
            axis (the largest |difference| along one of the cell's four edges of that axis) times the float32
            rounding of the sample's index coordinate, r_a = 2^-24 (|s_a| + |alpha_m d_a|);
    D_m,a   the same for dT / dg_a, the record's term: sum_c |V_c| |dw_c / dg_a| over the 8 corners, plus the bound
            4 max_c |V_c| on its slope across the other two axes times their r_b;

    forward     L |step| sum_m A_m
    g_img       |g| |step| sum_m A_m
    g_target    |g| L |step| sum_m |alpha_m| D_m,a              (the record: k sum alpha dT)
    g_source    |g| L |step| sum_m (1 + |alpha_m|) D_m,a        (the record: k (sum dT - sum alpha dT))
    g_alpha     |g| L (|step| sum_m sum_a D_m,a |d_a| (1 + (|alpha_m| + |alphamin|) / |span|) + sum_m A_m / (P - 1))
                (the record: sum u dT.d = (sum alpha dT.d - alphamin sum dT.d) / span; span = 0: that term is 0)

g_source and g_alpha are scaled by the terms the record holds (sum dT and sum alpha dT), not by their difference:
the entries that work from the record subtract the two, and the rounding of each is what is left.  A pixel whose ray
has no sample inside (-1, D) on all axes has S_p = 0 and must be exactly 0.

Cell faces: dT jumps there, and float32 puts a sample that is a rounding error away from a face on either side.  For
the GRADIENT gates a ray is left out when the float64 index coordinate of one of its in-volume samples lies within
DELTA = 4e-5 of an integer without being that integer; at most 2 % of a generic scene's rays (asserted; measured
shares in LEFT_OUT_MEASURED).  The forward gate leaves out nothing.
The constructed scenes are exact in float32: a sample ON a face is on it for the kernels, which form g = x + shift -
1/2 directly.  Not so for the oracle, in either precision: it takes x through the reference's normalise / un-normalise
round trip, which returns some such samples one rounding error BELOW the face, and then differentiates the
neighbouring cell.  Rays with a sample the float64 oracle moves like that are left out of the gradient gates (the
scenes are placed so that there are none, see LEFT_OUT_MEASURED), and rays with any sample within DELTA of a face,
on it or not, out of the float32 yardstick's gradients.  At P = 41 the samples' alphas are the rounded m / 40, the
first rule applies to those 9-ray scenes too, and the 2 % cap cannot (one ray is 11 %): what P = 41 adds is the
forward gate.

Everything here is numpy / CPU torch: the rays are made once, on the CPU, and the device tests upload these arrays."""
from __future__ import annotations

import copy
import functools
from types import SimpleNamespace

import numpy as np
import torch

import oracle
import volgrad_cases as vc

EPS = 1e-8
DELTA = 4e-5
U = 2.0 ** -24
QUANTITIES = ("forward", "g_target", "g_source", "g_img", "g_alpha")
N_LABELS = 6  # every label has a channel: the channel sum is the plain forward

# max_p |oracle32 - oracle64| / S_p over CASES (test_marcher.py::test_rho32_and_left_out_shares re-measures and
# prints them), on the CPU, from the oracle alone
# (the largest: extents_32_1_31, a volume one voxel thick seen from 200 voxels away -- an index coordinate there
# carries 2.4e-5 of rounding, the interpolant falls from V to 0 within one voxel, and one or two samples make the
# pixel; the constructed scenes measure 1 .. 8 x 2^-24, the other generic ones 20 .. 95 x 2^-24)
RHO32_MEASURED = {"forward": 1.732e-4, "g_target": 3.527e-5, "g_source": 7.730e-6, "g_img": 1.733e-4,
                  "g_alpha": 6.123e-6}
RHO32_CAP = {k: 4 * v for k, v in RHO32_MEASURED.items()}
# share of the rays of each generic scene that the gradient gates leave out (cap: 2 %)
LEFT_OUT_MEASURED = {"flat_oblique3": 0.0070, "flat_inner": 0.0117, "tall_three": 0.0095, "extents_30_31_32": 0.0070,
                     "flat_oblique3-range0.75_0.25": 0.0070,
                     # (9 rays, alphas m / 40 as float32 rounds them: no cap, see above)
                     "brick_edge-P41": 0.5556, "brick_edge_reversed-P41": 0.5556, "brick_corner-P41": 0.5556,
                     "brick_corner_reversed-P41": 0.5556}
LEFT_OUT_CAP = 0.02

OBLIQUE = ([0.3, 0.2, -0.1], [5.0, 200.0, -3.0])
OBLIQUE2 = ([-0.7, 0.4, 1.1], [-4.0, 180.0, 6.0])
NEAR_AXIS = ([0.003, -0.002, 0.001], [0.3, 200.0, 0.2])
INSIDE = ([0.2, 0.1, 0.0], [2.0, 5.0, -3.0])
GLOBAL, INNER, PAST = None, (0.31, 0.77), (-0.2, 1.3)

# name -> (dims, spacing, detector, delx, poses, voxel_shift, n_points, range)
GENERIC = {
    "flat_oblique3": ((40, 44, 8), (1.0, 1.0, 2.5), (13, 11), 2.0, (OBLIQUE, OBLIQUE2, NEAR_AXIS), 0.5, 40, GLOBAL),
    "flat_inner": ((40, 44, 8), (1.0, 1.0, 2.5), (13, 11), 2.0, (OBLIQUE, NEAR_AXIS, OBLIQUE2), 0.5, 41, INNER),
    "flat_2x2_two_samples": ((40, 44, 8), (1.0, 1.0, 2.5), (2, 2), 2.0, (NEAR_AXIS,), 0.0, 2, (0.62, 0.70)),
    "tall_three": ((33, 62, 35), (1.0, 1.0, 1.0), (7, 10), 2.0, (OBLIQUE, NEAR_AXIS, INSIDE), 0.5, 41, GLOBAL),
    "tall_inside_past": ((33, 62, 35), (1.0, 1.0, 1.0), (7, 10), 2.0, (INSIDE,), 0.0, 41, PAST),
    "extents_30_31_32": ((30, 31, 32), (1.0, 1.0, 1.0), (13, 11), 2.0, (OBLIQUE2,), 0.5, 40, GLOBAL),
    "extents_32_1_31": ((32, 1, 31), (1.0, 1.0, 1.0), (7, 10), 2.0, (OBLIQUE, OBLIQUE2, INSIDE), 0.0, 41, GLOBAL),
    "extents_31_30_1": ((31, 30, 1), (1.0, 1.0, 1.0), (2, 2), 2.0, (OBLIQUE2,), 0.5, 3, (0.55, 0.65)),
}

# The constructed scenes: a shared source, a 3 x 3 target grid around a centre, column and row steps; every number
# is exact in float32 (and so are the samples' alphas m / (P - 1) when P - 1 is a power of two).
# name -> (dims, source, centre, column step, row step)
STEP_XY, STEP_Z, STEP_Y = (0.5, 0.5, 0.0), (0.0, 0.0, 0.5), (0.0, 0.5, 0.0)
CONSTRUCTED = {
    # the centre ray passes (30, 30, 3.25) at alpha 1/2: the edge shared by four bricks (boundaries at index 30), with
    # mixed signs, so the brick that owns the sample (base cell (30, 30)) is touched in that point only
    "brick_edge": ((40, 44, 8), (20.0, 40.0, 3.25), (40.0, 20.0, 3.25), STEP_XY, STEP_Z),
    "brick_edge_reversed": ((40, 44, 8), (40.0, 20.0, 3.25), (20.0, 40.0, 3.25), STEP_XY, STEP_Z),
    # ... with |d| = (18, 12): the two slab bounds of the owning brick are 9 * (1 / 18) and 6 * (1 / 12), each product
    # of a rounded reciprocal, equal only to an ulp
    "brick_edge_skew": ((40, 44, 8), (21.0, 36.0, 3.25), (39.0, 24.0, 3.25), STEP_XY, STEP_Z),
    # ... (30, 30, 30): the corner shared by eight bricks
    "brick_corner": ((40, 44, 40), (20.0, 40.0, 22.0), (40.0, 20.0, 38.0), STEP_XY, STEP_Z),
    "brick_corner_reversed": ((40, 44, 40), (40.0, 20.0, 38.0), (20.0, 40.0, 22.0), STEP_XY, STEP_Z),
    # all nine rays lie in the boundary plane x = 30
    "brick_plane": ((40, 44, 8), (30.0, 4.5, 2.25), (30.0, 40.5, 5.25), STEP_Y, STEP_Z),
    # samples on the corners of cells inside one brick: (8, 9, 2) + k (4, 4, 1) at P = 5
    "cell_faces": ((40, 44, 8), (8.0, 9.0, 2.0), (24.0, 25.0, 6.0), (0.5, -0.5, 0.0), STEP_Z),
    # first sample on g_x = -1, last on g_x = D - 1/2 = 39.5, for all nine rays
    "padding_faces": ((40, 44, 8), (-1.0, 10.25, 3.25), (39.5, 20.25, 4.25), STEP_Y, STEP_Z),
    # the centre ray touches the owner box [31, 40) x [31, 44) of the volume gradient's brick (1, 1) in (31, 31)
    "owner_box": ((40, 44, 8), (21.0, 41.0, 3.25), (41.0, 21.0, 3.25), STEP_XY, STEP_Z),
}
EXACT_P = {"brick_edge": (3, 5, 9, 41), "brick_edge_skew": (3, 5, 9), "brick_edge_reversed": (3, 5, 9, 41), "brick_corner": (3, 5, 9, 41),
           "brick_corner_reversed": (3, 5, 9, 41), "brick_plane": (5, 9), "cell_faces": (5, 9),
           "padding_faces": (3, 9), "owner_box": (3, 5)}
REVERSED_RANGE, EMPTY_RANGE = (0.75, 0.25), (0.5, 0.5)

# (scene, n_points or None for the scene's own, range or None for the scene's own)
CASES = [(n, p, None) for n in CONSTRUCTED for p in EXACT_P[n]] + [(n, None, None) for n in GENERIC] + \
    [(n, p, r) for n, p in (("brick_edge", 5), ("flat_oblique3", None)) for r in (REVERSED_RANGE, EMPTY_RANGE)]
CHANNEL_CASES = [(n, p, None) for n in CONSTRUCTED for p in EXACT_P[n][:2]] + [("flat_oblique3", None, None)] + \
    [("brick_edge", 5, REVERSED_RANGE), ("brick_edge", 5, EMPTY_RANGE)]
ORDERING_CASES = [("flat_oblique3", None, None), ("tall_three", None, None), ("extents_32_1_31", None, None)]
OWNER_BOX_CASES = [("owner_box", 3, None), ("owner_box", 5, None), ("owner_box", 5, REVERSED_RANGE),
                   ("owner_box", 5, EMPTY_RANGE), ("flat_oblique3", None, REVERSED_RANGE)]


def case_id(case):
    name, p, rng = case
    return name + (f"-P{p}" if p else "") + (f"-range{rng[0]:g}_{rng[1]:g}" if rng else "")


def _labels(dims):
    g = torch.Generator().manual_seed(2)
    coarse = torch.randint(0, N_LABELS, tuple(d // 8 + 1 for d in dims), generator=g)
    for ax in range(3):
        coarse = coarse.repeat_interleave(8, ax)
    return coarse[: dims[0], : dims[1], : dims[2]].contiguous().to(torch.uint8).numpy()


def _volume(dims):
    return (torch.rand(*dims, generator=torch.Generator().manual_seed(1)) + 0.5).numpy()


def _generic_rays(name):
    from diffdrr_amd import DRR, convert
    from diffdrr_amd.data import make_subject

    dims, spacing, det, delx, poses, shift, P, rng = GENERIC[name]
    volume = _volume(dims)
    drr = DRR(make_subject(torch.from_numpy(volume), spacing=spacing), sdd=300.0, height=det[0], width=det[1],
              delx=delx)
    with torch.no_grad():
        pose = convert(torch.tensor([p[0] for p in poses], dtype=torch.float32),
                       torch.tensor([p[1] for p in poses], dtype=torch.float32), parameterization="euler_angles",
                       convention="ZXY")
        source, target = drr.detector(pose, None)
        img = (target - source).norm(dim=-1)
        source, target = drr.affine_inverse(source), drr.affine_inverse(target)
    return dims, volume, source.contiguous().numpy(), target.contiguous().numpy(), img.contiguous().numpy(), det, \
        shift, P, rng


def _constructed_rays(name):
    dims, src, centre, col, row = CONSTRUCTED[name]
    f = np.float32
    t = np.array([[f(centre[a]) + f(j - 1) * f(col[a]) + f(i - 1) * f(row[a]) for a in range(3)]
                  for i in range(3) for j in range(3)], f)[None]
    s = np.array(src, f).reshape(1, 1, 3)
    img = np.linalg.norm((t - s).astype(np.float64), axis=-1).astype(f)
    return dims, _volume(dims), s, t, img, (3, 3), 0.5, None, (0.0, 1.0)


@functools.lru_cache(maxsize=None)
def scene(case):
    """-> namespace: dims, volume, labels, source (B, 1, 3), target (B, N, 3), img (B, N), det, shift, n_points, amin,
    amax (float32), exact (constructed, and P - 1 a power of two), constructed; and the fields volgrad_cases.walk
    reads (name, B, pose_of)."""
    name, p, rng = case
    constructed = name in CONSTRUCTED
    dims, volume, s, t, img, det, shift, P, own = (_constructed_rays if constructed else _generic_rays)(name)
    P = p or P
    rng = rng or own
    sc = SimpleNamespace(name=case_id(case), case=case, dims=dims, volume=volume, labels=_labels(dims), source=s,
                         target=t, img=img, det=det, shift=shift, n_points=P, constructed=constructed,
                         exact=constructed and (P - 1) & (P - 2) == 0, B=t.shape[0], N=t.shape[1])
    sc.pose_of = np.arange(sc.B)
    if rng is None:  # the batch-global range of the reference (renderers.py:220-223), in float32
        lo, hi = oracle.alpha_minmax(s, t, dims, voxel_shift=shift, eps=EPS)
        rng = (lo.min(), hi.max())
    sc.amin, sc.amax = np.float32(rng[0]), np.float32(rng[1])
    return sc


def grad_out(sc, channels=0):
    g = torch.Generator().manual_seed(7)
    shape = (sc.B, channels, sc.N) if channels else (sc.B, sc.N)
    return (torch.rand(*shape, generator=g) + 0.25).numpy() * np.where(np.arange(sc.N) % 3 == 1, -1.0, 1.0).astype(
        np.float32)


# ------------------------------------------------------------------------------------------ reference and scales
def _oracle(sc, dtype, go):
    """oracle.trilinear in `dtype` on the scene's float32 arrays -> dict of (B, N[, 3 | 2]) float64 arrays."""
    src = np.broadcast_to(sc.source, sc.target.shape)  # expanded: g_source per ray
    kw = dict(n_points=sc.n_points, alphamin=float(sc.amin), alphamax=float(sc.amax), voxel_shift=sc.shift, eps=EPS)
    a = [x.astype(dtype) for x in (sc.volume, src, sc.target, sc.img)]
    r = oracle.trilinear(*a, grad_out=go, **kw)
    res = {"forward": r["out"].reshape(sc.B, sc.N), "g_target": r["g_target"], "g_source": r["g_source"],
           "g_img": r["g_img"].reshape(sc.B, sc.N)}
    ga = np.zeros((sc.B, sc.N, 2))
    for b in range(sc.B):
        for n in range(sc.N):  # (the oracle sums the pair over the rays of a call)
            one = oracle.trilinear(a[0], a[1][b:b + 1, n:n + 1], a[2][b:b + 1, n:n + 1], a[3][b:b + 1, n:n + 1],
                                   grad_out=go[b:b + 1, n:n + 1], **kw)
            ga[b, n] = one["g_alphamin"], one["g_alphamax"]
    res["g_alpha"] = ga
    return {k: np.asarray(v, np.float64) for k, v in res.items()}


def _scales(sc, go):
    """-> ({quantity: S (B, N[, 1])}, left_out (B, N) bool) from the float64 sample positions."""
    s, t, L = (x.astype(np.float64) for x in (sc.source, sc.target, sc.img))
    V = np.pad(sc.volume.astype(np.float64), 1)  # zero padding: voxel i sits at V[i + 1]
    P, amin, span = sc.n_points, float(sc.amin), float(sc.amax) - float(sc.amin)
    step = span / (P - 1)
    d = t - s + EPS  # (B, N, 3)
    al = oracle.linspace01(P).astype(np.float64) * span + amin  # (P,)
    ad = al[None, None, :, None] * d[:, :, None, :]
    g = s[:, :, None, :] + ad + (sc.shift - 0.5)  # (B, N, P, 3)
    r = U * (np.abs(s[:, :, None, :]) + np.abs(ad))  # float32 rounding of the index coordinate
    D = np.asarray(sc.dims, np.float64)
    inside = ((g > -1) & (g < D)).all(-1)  # (B, N, P)
    f = np.floor(g)
    frac = g - f
    i0 = np.clip(f, -1, D - 1).astype(np.int64) + 1  # (cells outside: any; they are masked by `inside`)
    corner = np.empty(g.shape[:-1] + (2, 2, 2))
    for c in range(8):
        o = ((c >> 2) & 1, (c >> 1) & 1, c & 1)
        corner[..., o[0], o[1], o[2]] = V[i0[..., 0] + o[0], i0[..., 1] + o[1], i0[..., 2] + o[2]]
    corner = np.where(inside[..., None, None, None], corner, 0.0)
    ax = ((slice(None), None, None), (None, slice(None), None), (None, None, slice(None)))
    w = [np.stack([1 - frac[..., a], frac[..., a]], -1)[(Ellipsis,) + ax[a]] for a in range(3)]  # (..., 2, 1, 1) ...
    W = w[0] * w[1] * w[2]
    av = np.abs(corner)
    A = (av * W).sum((-3, -2, -1))
    vmax = av.max((-3, -2, -1))
    Dm = np.empty(g.shape)
    for a in range(3):
        slope = np.abs(np.diff(corner, axis=-3 + a)).max((-3, -2, -1))
        A = A + slope * r[..., a]
        b, c = (x for x in range(3) if x != a)
        Wa = np.broadcast_to(w[b] * w[c], W.shape)  # |dw / dg_a| of a corner: the other two axes' weights
        Dm[..., a] = (av * Wa).sum((-3, -2, -1)) + 4 * vmax * (r.sum(-1) - r[..., a])
    Dm = np.where(inside[..., None], Dm, 0.0)
    A = np.where(inside, A, 0.0)
    sumA = A.sum(-1)
    ag, k = np.abs(go.astype(np.float64)), abs(step)
    aal = np.abs(al)[None, None, :, None]
    dd = (Dm * np.abs(d)[:, :, None, :]).sum(-1)  # (B, N, P)
    through_x = (dd * (1 + ((np.abs(al) + abs(amin)) / abs(span) if span != 0 else 0.0))).sum(-1)
    S = {"forward": L * k * sumA, "g_img": ag * k * sumA,
         "g_target": (ag * L * k)[..., None] * (aal * Dm).sum(2),
         "g_source": (ag * L * k)[..., None] * ((1 + aal) * Dm).sum(2),
         "g_alpha": (ag * L * (k * through_x + sumA / (P - 1)))[..., None]}
    dist = np.abs(g - np.rint(g))
    near_face = ((dist > 0) & (dist < DELTA)).any(-1) & inside
    # the float64 oracle takes its index coordinates through the reference's normalise / un-normalise round trip
    # (renderers.py:148-152, then grid_sample): a sample that sits ON a face may come back one rounding error below
    # it, and the oracle then differentiates the neighbouring cell
    x = s[:, :, None, :] + ad
    g_oracle = ((2.0 * (x + sc.shift) / D - 1.0 + 1.0) * D - 1.0) / 2.0
    moved = ((np.floor(g_oracle) != f).any(-1) & inside).any(-1)
    left_out = moved | (np.zeros((sc.B, sc.N), bool) if sc.exact else near_face.any(-1))
    # the yardstick's own gradients: the float32 oracle takes every index coordinate through the reference's
    # normalise / un-normalise round trip, which does not return a sample that sits ON a face to the face
    return S, left_out, ((dist < DELTA).any(-1) & inside).any(-1)


_refs = {}


def reference(case):
    """-> namespace: sc, go (B, N) float32, o64 / o32 {quantity: array}, S {quantity: scale}, left_out (B, N), rho32
    {quantity: this case's}.  Computed once per process and left unchanged."""
    if case not in _refs:
        sc = scene(case)
        go = grad_out(sc)
        o64, o32 = _oracle(sc, np.float64, go), _oracle(sc, np.float32, go)
        S, left_out, left_out32 = _scales(sc, go)
        rho = {}
        for q in QUANTITIES:
            live = np.broadcast_to(S[q] > 0, o64[q].shape)
            if q != "forward":
                live = live & ~left_out32.reshape(left_out32.shape + (1,) * (o64[q].ndim - 2))
            err = np.abs(o32[q] - o64[q])
            rho[q] = float((err[live] / np.broadcast_to(S[q], err.shape)[live]).max()) if live.any() else 0.0
        _refs[case] = SimpleNamespace(sc=sc, go=go, o64=o64, o32=o32, S=S, left_out=left_out, rho32=rho)
    return _refs[case]


@functools.lru_cache(maxsize=None)
def rho32_all():
    """max over CASES of each quantity's rho32, from the oracle alone."""
    return {q: max(reference(c).rho32[q] for c in CASES) for q in QUANTITIES}


def rho32(ref, q):
    """The yardstick of quantity q on the case's own rays (never more than the largest value over all cases, which
    has its cap)."""
    assert ref.rho32[q] <= RHO32_CAP[q], f"the float32 yardstick of {q} is {ref.rho32[q]:.3e} from float64: over its cap"
    return ref.rho32[q]


def gate(tag, q, got, ref, extra=0.0):
    """-> problems of `got` (B, N[, k]) against the float64 reference of quantity q; prints worst error / allowance.
    `extra`: a further allowance in units of S_p (the channel entries' 16-bit staging)."""
    got = np.asarray(got, np.float64).reshape(ref.o64[q].shape)
    S = np.broadcast_to(ref.S[q], got.shape)
    tol = (2 * rho32(ref, q) + 8 * U + extra) * S
    err = np.abs(got - ref.o64[q])
    keep = np.ones(got.shape, bool)
    if q != "forward":
        keep &= ~ref.left_out.reshape(ref.left_out.shape + (1,) * (got.ndim - 2))
    problems = []
    if not np.isfinite(got).all():
        problems.append(f"{tag} {q}: non-finite values")
    dark = keep & (S == 0)
    if (got[dark] != 0).any():
        problems.append(f"{tag} {q}: {int((got[dark] != 0).sum())} entries of rays without a sample in the volume are "
                        f"not 0 (largest {np.abs(got[dark]).max():.3e})")
    lit = keep & (S > 0)
    worst = float((err[lit] / tol[lit]).max()) if lit.any() else 0.0
    print(f"{tag} {q}: worst error / allowance {worst:.3f} ({int(lit.sum())} entries, rho32 {rho32(ref, q):.3e})")
    over = lit & ~(err <= tol)
    if over.any():
        at = np.unravel_index(np.argmax(np.where(over, err / np.maximum(tol, 1e-300), 0)), got.shape)
        problems.append(f"{tag} {q}: {int(over.sum())} entries over the allowance, worst {worst:.2f} x at {at}: got "
                        f"{got[at]:.9e} float64 {ref.o64[q][at]:.9e} S {S[at]:.3e}")
    return problems


def check_left_out(ref):
    share = float(ref.left_out.mean())
    if not ref.sc.constructed:
        assert share <= LEFT_OUT_CAP, f"{ref.sc.name}: {share:.2%} of the rays lie within {DELTA} of a cell face"
    return share


# ------------------------------------------------------------------------------------------------------- checks
def _upload(sc, device, poses=None):
    sel = slice(None) if poses is None else poses
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    return SimpleNamespace(V=dev(sc.volume), labels=dev(sc.labels), s=dev(sc.source[sel]), t=dev(sc.target[sel]),
                           L=dev(sc.img[sel]), a0=dev(np.array([sc.amin])), a1=dev(np.array([sc.amax])),
                           kw=dict(n_points=sc.n_points, voxel_shift=sc.shift, eps=EPS))


def _host(device):
    return torch.device(device).type == "cpu"


def _np(x):
    return x.detach().cpu().numpy()


def one_brick(sc):
    """(B, N) bool: every in-volume sample of the ray has its base cell in one and the same brick of 31^3 cells from
    -1 (csrc/tri_brick.h), also when it is moved by DELTA either way; rays without a sample in the volume count."""
    s, t = sc.source.astype(np.float64), sc.target.astype(np.float64)
    span = float(sc.amax) - float(sc.amin)
    al = oracle.linspace01(sc.n_points).astype(np.float64) * span + float(sc.amin)
    g = s[:, :, None, :] + al[None, None, :, None] * (t - s + EPS)[:, :, None, :] + (sc.shift - 0.5)
    inside = ((g > -1 - DELTA) & (g < np.asarray(sc.dims) + DELTA)).all(-1)
    lo, hi = (np.floor((np.floor(g + e) + 1) / 31.0) for e in (-DELTA, DELTA))
    lo_min = np.where(inside[..., None], lo, np.inf).min(2)
    hi_max = np.where(inside[..., None], hi, -np.inf).max(2)
    return ~inside.any(-1) | (lo_min == hi_max).all(-1)


def check_forward(case, device, ops):
    """The per-ray entry and the brick entry with and without its record against float64, per pixel; the two brick
    launches equal each other bit for bit."""
    ref = reference(case)
    sc, tag = ref.sc, f"[{ref.sc.name}]"
    r = _upload(sc, device)
    per_ray = ops.trilinear_forward(r.V, r.s, r.t, r.L, r.a0, r.a1, **r.kw)
    plain = ops.trilinear_forward_bricks(r.V, r.s, r.t, r.L, r.a0, r.a1, sc.det, **r.kw)
    with_rec, _ = ops.trilinear_forward_bricks(r.V, r.s, r.t, r.L, r.a0, r.a1, sc.det, want_aux=True, **r.kw)
    problems = gate(tag + " per-ray", "forward", _np(per_ray), ref)
    problems += gate(tag + " bricks", "forward", _np(plain), ref)
    problems += gate(tag + " bricks + record", "forward", _np(with_rec), ref)
    # With the record the launch sums T over the bricks and forms L step sum T once; without, every brick adds its own
    # L step T: the same bits wherever ONE brick holds all of a ray's samples, the same value to rounding elsewhere
    # (gated above).  One brick: every in-volume sample's base cell, taken DELTA either way, falls in the same brick.
    same = one_brick(sc)
    print(f"{tag} rays whose samples one brick holds: {int(same.sum())} of {same.size}")
    if not torch.equal(plain.cpu()[torch.from_numpy(same)], with_rec.cpu()[torch.from_numpy(same)]):
        problems.append(f"{tag} the brick forward with and without the record differ on rays that one brick holds")
    assert float(np.abs(ref.o64["forward"]).max()) > 0 or sc.amin == sc.amax
    assert not problems, "\n".join(problems)


def check_ray_gradients(case, device, ops):
    """g_source, g_target, g_img and g_alpha from the record (ddrr_trilinear_backward_rays) and from the per-ray
    re-march (ddrr_trilinear_backward) against float64, per pixel."""
    ref = reference(case)
    sc, tag = ref.sc, f"[{ref.sc.name}]"
    share = check_left_out(ref)
    print(f"{tag} rays left out of the gradient gates: {share:.2%}")
    r = _upload(sc, device)
    go = torch.from_numpy(ref.go).to(device)
    _, aux = ops.trilinear_forward_bricks(r.V, r.s, r.t, r.L, r.a0, r.a1, sc.det, want_aux=True, **r.kw)
    rec = ops.trilinear_backward_rays(aux, go, r.s, r.t, r.L, r.a0, r.a1, n_points=sc.n_points, eps=EPS)
    march = ops.trilinear_backward(r.V, r.s, r.t, r.L, go, r.a0, r.a1, **r.kw)
    problems = []
    for name, res in (("record", rec), ("re-march", march)):
        for q in QUANTITIES[1:]:
            problems += gate(f"{tag} {name}", q, _np(res[q]), ref)
    assert not problems, "\n".join(problems)


def check_channels(case, device, ops):
    """ddrr_trilinear_forward_channels_bricks per channel against ddrr_trilinear_forward_channels per pixel and its
    channel sum against the float64 forward; ddrr_trilinear_backward_channels_bricks against
    ddrr_trilinear_backward_channels.
    The brick forward stages values rounded to nearest at 16 significant bits (csrc/brick_step.h pack_voxel_label):
    half a unit of the last place is 2^-17 of the binade's upper end and 2^-16 of its lower, so 2^-16 S_p more.  Two float32 entries against each other: each is within the gate of the
    exact value, so twice the gate (for the ray gradients with max_c |grad_out| as the pixel's weight)."""
    ref = reference(case)
    sc, tag = ref.sc, f"[{ref.sc.name}]"
    r = _upload(sc, device)
    C, q16 = N_LABELS, 2.0 ** -16
    ch = _np(ops.trilinear_forward_channels_bricks(r.V, r.labels, C, r.s, r.t, r.L, r.a0, r.a1, sc.det, **r.kw))
    per_ray = _np(ops.trilinear_forward_channels(r.V, r.labels, C, r.s, r.t, r.L, r.a0, r.a1, **r.kw))
    problems = gate(tag + " channel sum, bricks", "forward", ch.astype(np.float64).sum(1), ref, extra=q16)
    problems += gate(tag + " channel sum, per-ray", "forward", per_ray.astype(np.float64).sum(1), ref)
    S = ref.S["forward"][:, None, :]
    tol = (2 * (2 * rho32(ref, "forward") + 8 * U) + q16) * S
    err = np.abs(ch.astype(np.float64) - per_ray)
    worst = float((err / np.maximum(tol, 1e-300))[np.broadcast_to(S > 0, err.shape)].max()) if (S > 0).any() else 0.0
    print(f"{tag} channels, bricks against per-ray: worst error / allowance {worst:.3f}")
    if not (err <= tol).all():
        problems.append(f"{tag} channels: {int((~(err <= tol)).sum())} entries of bricks and per-ray differ by more "
                        f"than the allowance, worst {worst:.2f} x")
    if ((per_ray == 0) & (ch != 0)).any():
        problems.append(f"{tag} channels: the bricks fill channels the per-ray entry leaves 0")
    goc = grad_out(sc, C)
    god = torch.from_numpy(goc).to(device)
    rb = ops.trilinear_backward_channels_bricks(r.V, r.labels, r.s, r.t, r.L, god, r.a0, r.a1, sc.det, **r.kw)
    rp = ops.trilinear_backward_channels(r.V, r.labels, r.s, r.t, r.L, god, r.a0, r.a1, **r.kw)
    weight = np.abs(goc).max(1) / np.abs(ref.go)  # (B, N): the scales are linear in |grad_out|
    keep = ~ref.left_out
    for q in QUANTITIES[1:]:
        a, b = _np(rb[q]).astype(np.float64), _np(rp[q]).astype(np.float64)
        Sq = np.broadcast_to(ref.S[q] * weight.reshape(weight.shape + (1,) * (ref.S[q].ndim - 2)), a.shape)
        tolq = 2 * (2 * rho32(ref, q) + 8 * U) * Sq
        k = np.broadcast_to(keep.reshape(keep.shape + (1,) * (a.ndim - 2)), a.shape)
        e = np.abs(a - b)
        worst = float((e / np.maximum(tolq, 1e-300))[k & (Sq > 0)].max()) if (k & (Sq > 0)).any() else 0.0
        print(f"{tag} channels {q}, bricks against per-ray: worst error / allowance {worst:.3f}")
        if not (e <= tolq)[k].all():
            problems.append(f"{tag} channels {q}: bricks and per-ray differ by {worst:.2f} x the allowance")
    assert not problems, "\n".join(problems)


def check_ordering(case, device, ops):
    """A pixel's value must not depend on which other poses are in the batch: every pose rendered alone (with the
    batch's range) against its rows of the batch -- bit for bit on the host, within the gate on the device."""
    ref = reference(case)
    sc, tag = ref.sc, f"[{ref.sc.name}]"
    assert sc.B == 3
    r = _upload(sc, device)
    whole, aux = ops.trilinear_forward_bricks(r.V, r.s, r.t, r.L, r.a0, r.a1, sc.det, want_aux=True, **r.kw)
    go = torch.from_numpy(ref.go).to(device)
    grads = ops.trilinear_backward_rays(aux, go, r.s, r.t, r.L, r.a0, r.a1, n_points=sc.n_points, eps=EPS)
    alone = {q: [] for q in QUANTITIES}
    for b in range(sc.B):
        p = _upload(sc, device, slice(b, b + 1))
        out, aux1 = ops.trilinear_forward_bricks(p.V, p.s, p.t, p.L, p.a0, p.a1, sc.det, want_aux=True, **p.kw)
        g1 = ops.trilinear_backward_rays(aux1, go[b:b + 1], p.s, p.t, p.L, p.a0, p.a1, n_points=sc.n_points, eps=EPS)
        alone["forward"].append(out)
        for q in QUANTITIES[1:]:
            alone[q].append(g1[q])
    problems = []
    for q in QUANTITIES:
        a = torch.cat(alone[q])
        if _host(device):
            if not torch.equal(a, whole if q == "forward" else grads[q]):
                problems.append(f"{tag} {q}: a pose alone differs from the same pose in the batch")
        else:
            problems += gate(f"{tag} alone", q, _np(a), ref)
    assert not problems, "\n".join(problems)


def check_owner_box(case, device, ops):
    """ddrr_trilinear_backward_volume_bricks against the oracle's g_volume per voxel, with the gate of
    tests/test_gpu_volume_gradient_bricks.py: |got - g64| <= 2 rho32 T + (n + 2) Q / 2 on the fixed-point path,
    8 * 2^-24 T in place of the quanta on the float path (the host emulation accumulates in float); rho32 from the
    per-ray kernel's volume gradient, capped by volgrad_cases.RHO32_CAP."""
    ref = reference(case)
    sc, tag = ref.sc, f"[{ref.sc.name}]"
    assert sc.shift == vc.SHIFT
    r = _upload(sc, device)
    go = torch.from_numpy(ref.go).to(device)
    kept, real = [], ops.launch_workspace
    ops.launch_workspace = lambda shape, dev: kept.append(real(shape, dev)) or kept[-1]
    try:
        got = _np(ops.trilinear_backward_volume_bricks(sc.dims, r.s, r.t, r.L, go, r.a0, r.a1, sc.det, **r.kw))
    finally:
        ops.launch_workspace = real
    Q = 0.0
    if not _host(device):  # the launch's bound, read back to size the quantum as the volume-gradient tests do
        wmax, n_sum = (float(v) for v in _np(kept[-1][1:3].view(torch.float32)))
        if 0 < wmax < 1e30 and 0 < n_sum <= 16384:
            Q = n_sum * wmax / vc.FIXED_COUNTS["marcher"]
    src = np.broadcast_to(sc.source, sc.target.shape)
    g64 = oracle.trilinear(*(x.astype(np.float64) for x in (sc.volume, src, sc.target, sc.img)), grad_out=ref.go,
                           want_volume_grad=True, n_points=sc.n_points, alphamin=float(sc.amin),
                           alphamax=float(sc.amax), voxel_shift=sc.shift, eps=EPS)["g_volume"]
    # per voxel: T, the rounding scale, and n, the number of adds -- from the walk of the same samples (for
    # alphamax < alphamin: of the range the right way round, whose samples sit at the same places and weigh -step)
    flip = sc.amax < sc.amin
    wsc = copy.copy(sc)
    if flip:
        wsc.name, wsc.amin, wsc.amax = sc.name + "-sorted", sc.amax, sc.amin
    w = vc.walk(wsc, "marcher", ref.go)
    scale = np.abs(g64).max()
    if sc.amax == sc.amin:
        assert scale == 0 and not w.n.any()
    else:  # the walk is the oracle (walked backwards: to the float32 linspace table's 1 - u_m != u_(P-1-m), 6e-8 of |d|)
        assert scale > 0 and np.abs((-w.g64 if flip else w.g64) - g64).max() <= (1e-4 if flip else 1e-10) * scale
    V = torch.from_numpy(sc.volume).to(device)
    ref32 = _np(ops.trilinear_backward(V, r.s, r.t, r.L, go, r.a0, r.a1, want_rays=False, want_img=False,
                                       want_alpha=False, want_volume=True, det=sc.det, **r.kw)["g_volume"])
    hit = w.n > 0
    rho = float((np.abs(ref32 - g64)[hit] / w.T[hit]).max()) if hit.any() else 0.0
    assert rho <= vc.RHO32_CAP["marcher"], f"{tag} the per-ray float32 yardstick is {rho:.3e} from float64"
    tol = 2 * rho * w.T + ((w.n + 2) * Q / 2 if Q > 0 else 8 * U * w.T)
    err = np.abs(got.astype(np.float64) - g64)
    worst = float((err[hit] / tol[hit]).max()) if hit.any() else 0.0
    print(f"{tag} volume gradient on the owner bricks ({'fixed' if Q else 'float'} path): rho32 {rho:.3e}, worst "
          f"error / allowance {worst:.3f}")
    assert not got[~hit].any(), f"{tag} voxels no sample reaches are not 0"
    assert (err[hit] <= tol[hit]).all(), f"{tag} {int((err[hit] > tol[hit]).sum())} voxels over the allowance, worst " \
                                         f"{worst:.2f} x"
