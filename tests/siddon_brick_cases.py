"""What tests/test_siddon_bricks.py (host emulation) and tests/test_gpu_siddon_bricks.py (MI355X) share: scenes, the
float64 reference, the float32 yardsticks, the per-pixel scales and the checks of the Siddon brick entries
(ddrr_siddon_forward_bricks with and without its record, masked, with the packed record; record_planes of the blocked
record; ddrr_siddon_backward_rays on either record; ddrr_siddon_forward_channels_bricks), written once for either
device.  Every check takes (..., device, ops) as marcher_cases.check_* do.

Reference: `walk64`, a plain float64 walk of the scene's float32 rays, volume and lengths on the lines of
volgrad_cases._siddon_hits: all plane crossings alpha = ((i - 1/2) - s_a) / d_a, d = t - s + eps, of a ray, sorted
(stable: x before y before z at equal alphas, as the oracle's merge) and tagged with their axis; the voxel of a segment
from its midpoint; per ray
    I    = sum_k V_k (alpha_k+1 - alpha_k)
    S0_a = sum over the crossings c of axis a of dV_c = V_before - V_after       (csrc/siddon_core.h:212-217)
    S1_a = sum over the same crossings of dV_c alpha_c
    g_img = g I,   g_source_a = g L (S1_a - S0_a) / d_a,   g_target_a = -g L S1_a / d_a.
test_siddon_bricks.py::test_walk_is_the_oracle pins out, g_img, g_source and g_target of the walk to oracle.siddon in
float64 (the source expanded per ray) to 1e-12 of each pixel's scale: the walk defines nothing of its own.

Gate, for every pixel p and quantity q:   |kernel - walk64| <= (2 rho32_q + 8 * 2^-24) S_p,q [+ the storage's term].
rho32_q = max_p |float32 result - walk64| / S_p,q, from references alone, on the CPU: oracle.siddon on float32 arrays
for forward, g_img, g_source and g_target; the per-ray kernel ddrr_siddon_forward with its record on the host emulation
(a 3-way merge over the whole volume: another walk than the bricks') for the planes I, S0x, S0z, S1x, S1z.  The largest
value over CASES is RHO32_MEASURED (test_rho32_tie_and_left_out_shares re-measures and prints), RHO32_CAP is 4 x that,
and a case is gated with the rho32 of its OWN rays, which has to stay under the cap.  The factors 2 and 8 * 2^-24 are
marcher_cases'.

Scales, from the float64 walk alone.  A = sum_k |V_k| (alpha_k+1 - alpha_k); over the crossings c of axis a
C0_a = sum_c |dV_c| and C1_a = sum_c |dV_c| |alpha_c|; T = A + sum_a C1_a:
    plane I  T            image  L T            g_img  |g| T
The S planes and the ray gradients are WIDER than C0_a, C1_a, on the evidence of the float32 references: every walk
forms a crossing's term from its two voxels separately (csrc/siddon_core.h: S1x += w1x v per voxel; csrc/brick_step.h:
dv a_cur), so what rounds is |V_before| |alpha| + |V_after| |alpha|, not |dV| |alpha|.  Between two nearly equal
voxels the per-ray kernel on the host emulation is 2.4e-5 C1_z from float64 (generic_21x19, pose 1, ray 156:
dV = 4e-4 at alpha 0.6), 400 x 2^-24, and 1e-6 C0_x; with W0_a = sum_c (|V_before| + |V_after|) and
W1_a = sum_c (|V_before| + |V_after|) |alpha_c| in their place it is 5e-8 .. 8e-8 on every scene (RHO32_MEASURED), and
a gate of (2 rho32 + 8 * 2^-24) W is fifty times tighter than one of (2 * 2.4e-5) C1.
The ray's y is formed from the record's x, z and I (csrc/record_layout.h rec_blocked_load: S0y = -(S0x + S0z),
S1y = I - (S1x + S1z)), so y carries the rounding of all three axes and of I: Wy = (sum_a W0_a, A + sum_a W1_a).
    S0x, S0z  W0_x, W0_z                        S1x, S1z  W1_x, W1_z
    g_target_a  |g| L W1_a / |d_a|              g_source_a  |g| L (W0_a + W1_a) / |d_a|       (y: Wy)
A brick's piece of z is formed likewise, from its x, y and I (csrc/brick_step.h step_walk: S0z = -(S0x + S0y),
S1z = I - (S1x + S1y)).  The float32 references sum z directly, so z keeps its own scale; what the subtraction itself
rounds is added to the z allowances as a term of its own, 2^-24 sum_a W0_a (S0z) and 2^-24 (A + sum_a W1_a) (S1z),
weighted like the scales for g_source_z and g_target_z -- also on a ray that crosses no z plane, where the scale is 0.
A pixel with scale 0 -- no segment of its ray inside the volume, or only zeros -- must be exactly 0, at masked-out
pixels likewise; outputs the entries are documented to write everywhere are filled with NaN before the launch.

Identities, on EVERY ray: sum_a S0_a = 0 and sum_a S1_a = I hold on the blocked record by construction; on the
gradients returned from it  sum_a d_a g_target_a = -g L I  is gated at |g| L (A + sum_a W1_a) with rho32 of plane I,
and  sum_a d_a (g_source_a + g_target_a) = 0  at |g| L (sum_a W0_a + A + sum_a W1_a).

Ties.  Two crossings of different axes whose order float32 cannot decide are attributed either way, and S0_a, S1_a,
g_source, g_target jump by O(|V|); I, the image and g_img do not.  The per-axis gates leave out a ray when two
consecutive crossings of different axes, one of them at least next to an in-volume segment, are closer in alpha than
TIE; the forward, I, g_img and identity gates leave out nothing.  TIE is fixed from the references alone: rho32 of
g_source / g_target is measured with a generous margin (TIE_PLATEAU, where it no longer falls), and TIE is the
smallest power of two at which the float32 oracle's gradients on the kept rays of every generic scene stay under
RHO32_CAP (half of it does not: asserted).  At most LEFT_OUT_CAP = 2 % of a generic scene's rays are left out
(asserted; the poses were chosen by the float64 walk for it; LEFT_OUT_MEASURED).  The constructed scenes are ties by
construction: they take the forward, I, g_img, identity and exact-zero gates only.  brick_plane, nine rays inside the
voxel plane x = 31.5, is DROPPED: the float32 and the float64 oracle assign such a ray to either side, and their images
differ by 3.1e-3 of the scale (asserted to be over the cap).

Storage terms.  16-bit storages: a stored voxel is within Q = (Q16_RANGE_OVER_LEVEL / 131070) level(brick) of its
value (conftest.brick_levels; 0 in a brick that takes the fp32 path), so the I gates get L | g times the walk's line
integral of Q and nothing else, and in the S planes and ray gradients a crossing's two voxels are off by
Q_before + Q_after, summed like W0 / W1 (y: all of them and the integral).  The brick grid is
32 x 32 x 64 (q16, q16p) or 32 x 64 x 32 (q16y, q16py) on the device and 32^3 on the host emulation, and
ops.brick_fallbacks is asserted against brick_levels' flags (a volume of fewer than four slices is rendered from its
fp32 values by the general kernel, builds no workspace and gets no term: brick_fallbacks must say None).
Packed record (csrc/record_pack.h): fields are rint(S0 q) and rint(S1 q / A) with 1 / q = 2 vmax (Dx + Dy + Dz + 3)
/ 2^30 and A = max(1, max |alpha| in the volume); one piece per brick the ray passes (bricks holding an in-volume
segment of the walk), half a quantum each: S0_a +- n / 2q, S1_a +- n A / 2q, y twice that.  Two launches give the
same bits.  Channels: the staged word keeps 16 significant bits (csrc/brick_step.h pack_voxel_label, round to
nearest): 2^-16 of the pixel's scale.

Everything here is numpy / CPU torch: the rays are made once, on the CPU, and the device tests upload these arrays."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import torch

import oracle
import volgrad_cases as vc
from conftest import Q16_RANGE_OVER_LEVEL, brick_levels, build_emu

EPS = 1e-8
SHIFT = 0.5
U = 2.0 ** -24
N_LABELS = 6  # every label has a channel: the channel sum is the plain forward
PLANES = ("I", "S0x", "S0z", "S1x", "S1z")
QUANTITIES = ("forward", "g_img", "g_source", "g_target") + PLANES
TIED_QUANTITIES = ("g_source", "g_target", "S0x", "S0z", "S1x", "S1z")

# max_p |float32 reference - walk64| / S_p over CASES, on the CPU, from the references alone
# (test_siddon_bricks.py::test_rho32_tie_and_left_out_shares re-measures and prints them)
RHO32_MEASURED = {"forward": 6.281e-8, "g_img": 6.280e-8, "g_source": 1.918e-8, "g_target": 5.860e-8, "I": 6.280e-8,
                  "S0x": 7.752e-8, "S0z": 5.824e-8, "S1x": 7.984e-8, "S1z": 8.274e-8}
RHO32_CAP = {k: 4 * v for k, v in RHO32_MEASURED.items()}
# measured: with TIE = 2^-24 the float32 oracle's g_source / g_target are 5.3e-4 / 1.5e-3 of the scale from float64 on
# poses33_8x6 and 2.8e-3 / 1.2e-2 on poses8_21x19 (a flipped pair each), with 2^-23 and anything wider 1.9e-8 / 5.9e-8
# on every generic scene; the per-ray kernel's planes flip from 2^-26 down
TIE = 2.0 ** -23
TIE_PLATEAU = 2.0 ** -14
# share of the rays of each generic scene that the per-axis gates leave out (cap: 2 %)
LEFT_OUT_MEASURED = {"generic_21x19": 0.002506, "generic_24x20": 0.000833, "extents_32_1_31": 0.0,
                     "extents_31_30_1": 0.0, "extents_33_65_33": 0.0, "sparse": 0.010417,
                     "poses33_8x6": 0.005682, "poses8_21x19": 0.008145, "poses9_21x19": 0.008633}
LEFT_OUT_CAP = 0.02

STORAGES_HOST = ("f32", "q16", "q16p")
STORAGES_DEVICE = STORAGES_HOST + ("q16y", "q16py")

# (rotation ZXY, translation): oblique, near-axis, mostly beside the volume, along z, source inside the volume
OBLIQUE = ([0.55, -0.35, 0.8], [3.0, 245.0, -5.0])
NEAR_AXIS = ([0.003, -0.002, 0.001], [0.3, 250.0, 0.2])
BESIDE = ([0.1, 0.05, -0.2], [27.0, 250.0, 5.0])
ALONG_Z = ([0.1, 1.22, 0.62], [-1.0, 253.0, -4.0])
INSIDE = ([0.2, 0.1, 0.0], [2.0, 5.0, -3.0])
FIVE = (OBLIQUE, NEAR_AXIS, BESIDE, ALONG_Z, INSIDE)
# ... and four more: 8 poses is the last launch the fp32 storage hands to the general kernel's sibling and the 16-bit
# storages to their few-poses instantiation (csrc/bricks_fwd.hip launch_fwd_bricks, launch_q16), 9 the first beyond
NINE = FIVE + (([-0.7, 0.4, 1.1], [-4.0, 240.0, 6.0]), ([0.3, 0.2, -0.1], [5.0, 250.0, -3.0]),
               ([1.5, 0.1, 0.0], [0.0, 245.0, 0.0]), ([0.0, 1.45, 0.2], [2.0, 240.0, 1.0]))

# name -> (dims, volume kind, detector, delx, sdd, poses)
GENERIC = {
    "generic_21x19": ((40, 70, 70), "noise", (21, 19), 1.5, 400.0, FIVE),
    "generic_24x20": ((40, 70, 70), "noise", (24, 20), 1.5, 400.0, FIVE),
    "extents_32_1_31": ((32, 1, 31), "noise", (7, 10), 1.5, 400.0, (OBLIQUE, NEAR_AXIS)),
    "extents_31_30_1": ((31, 30, 1), "noise", (7, 10), 1.5, 400.0, (OBLIQUE, NEAR_AXIS)),
    "extents_33_65_33": ((33, 65, 33), "noise", (7, 10), 2.5, 400.0, (OBLIQUE, ALONG_Z)),
    "sparse": ((64, 64, 128), "sparse", (16, 15), 4.0, 600.0, (([0.5, -0.3, 0.2], [5.0, 380.0, -8.0]),
                                                                ([-0.7, 0.4, 1.1], [-12.0, 420.0, 6.0]))),
    "poses33_8x6": ((40, 70, 70), "noise", (8, 6), 5.0, 400.0, 33),
    "poses8_21x19": ((40, 70, 70), "noise", (21, 19), 1.5, 400.0, NINE[1:]),
    "poses9_21x19": ((40, 70, 70), "noise", (21, 19), 1.5, 400.0, NINE),
}

# The constructed scenes: a shared source, a 3 x 3 target grid around a centre, column and row steps; every number is
# exact in float32.  Planes lie at i - 1/2; the 32^3 bricks meet at 31.5, the 16-bit bricks' long axis at 63.5.
# name -> (dims, source, centre, column step, row step)
STEP_XY, STEP_Z, STEP_Y = (0.5, 0.5, 0.0), (0.0, 0.0, 0.5), (0.0, 0.5, 0.0)
CONSTRUCTED = {
    # the centre ray through the edge x = y = 31.5 shared by four bricks, at alpha 1/2, with mixed signs
    "brick_edge": ((40, 44, 8), (21.5, 41.5, 3.25), (41.5, 21.5, 3.25), STEP_XY, STEP_Z),
    "brick_edge_reversed": ((40, 44, 8), (41.5, 21.5, 3.25), (21.5, 41.5, 3.25), STEP_XY, STEP_Z),
    # ... through the corner (31.5, 31.5, 31.5) shared by eight 32^3 bricks
    "brick_corner": ((40, 44, 40), (21.5, 41.5, 23.5), (41.5, 21.5, 39.5), STEP_XY, STEP_Z),
    "brick_corner_reversed": ((40, 44, 40), (41.5, 21.5, 39.5), (21.5, 41.5, 23.5), STEP_XY, STEP_Z),
    # ... (31.5, 31.5, 63.5): a corner of the z-long 16-bit bricks too; (31.5, 63.5, 31.5): of the y-long ones
    "brick_corner_z64": ((40, 44, 70), (21.5, 41.5, 55.5), (41.5, 21.5, 71.5), STEP_XY, STEP_Z),
    "brick_corner_y64": ((40, 70, 40), (21.5, 73.5, 23.5), (41.5, 53.5, 39.5), STEP_XY, STEP_Z),
    # all nine rays lie in the boundary plane x = 31.5
    "brick_plane": ((40, 44, 8), (31.5, 4.25, 2.25), (31.5, 40.25, 5.25), STEP_Y, STEP_Z),
    # the centre ray x + y = 63.5 cuts brick (1, 1, 0) in the corner voxel (32, 32) only
    "corner_voxel": ((40, 44, 8), (21.75, 41.75, 3.25), (41.75, 21.75, 3.25), STEP_XY, STEP_Z),
    "corner_voxel_reversed": ((40, 44, 8), (41.75, 21.75, 3.25), (21.75, 41.75, 3.25), STEP_XY, STEP_Z),
}
# constructed scenes on which the float32 and the float64 oracle disagree on the IMAGE beyond RHO32_CAP (a ray inside
# a voxel plane is assigned to either side): dropped, see test_rho32_tie_and_left_out_shares
DROPPED = ("brick_plane",)

CASES = [n for n in GENERIC] + [n for n in CONSTRUCTED if n not in DROPPED]
GENERIC_CASES = [n for n in GENERIC]
CHANNEL_CASES = ["generic_21x19", "extents_33_65_33", "sparse", "brick_edge", "brick_corner", "corner_voxel"]
PACKED_CASES = ["generic_21x19", "generic_24x20", "poses9_21x19", "sparse", "extents_32_1_31", "brick_corner"]
MASKS = ("half", "single", "none")


# ------------------------------------------------------------------------------------------------------ scenes
def _volume(dims, kind):
    v = (torch.rand(*dims, generator=torch.Generator().manual_seed(7)) + 0.25).numpy()
    if kind == "sparse":  # whole bricks of zeros (skipped) and of one value next to bricks of noise; the faces at 32
        v[:32] = 0.0      # and 64 are brick faces of every grid, and the crossing into a skipped brick carries dV != 0
        v[32:, :32, :64] = 0.37
    return np.ascontiguousarray(v, np.float32)


def _labels(dims):
    g = torch.Generator().manual_seed(2)
    coarse = torch.randint(0, N_LABELS, tuple(d // 8 + 1 for d in dims), generator=g)
    for ax in range(3):
        coarse = coarse.repeat_interleave(8, ax)
    return coarse[: dims[0], : dims[1], : dims[2]].contiguous().to(torch.uint8).numpy()


def _poses(poses):
    if isinstance(poses, int):  # random poses around the oblique one
        g = torch.Generator().manual_seed(5)
        rot = torch.tensor(OBLIQUE[0]) + (torch.rand(poses, 3, generator=g) - 0.5) * 0.6
        xyz = torch.tensor(OBLIQUE[1]) + (torch.rand(poses, 3, generator=g) - 0.5) * 16.0
        return rot, xyz
    return (torch.tensor([p[0] for p in poses], dtype=torch.float32),
            torch.tensor([p[1] for p in poses], dtype=torch.float32))


def _generic_rays(name):
    from diffdrr_amd import DRR, convert
    from diffdrr_amd.data import make_subject

    dims, kind, det, delx, sdd, poses = GENERIC[name]
    volume = _volume(dims, kind)
    drr = DRR(make_subject(torch.from_numpy(volume)), sdd=sdd, height=det[0], width=det[1], delx=delx)
    rot, xyz = _poses(poses)
    with torch.no_grad():
        pose = convert(rot, xyz, parameterization="euler_angles", convention="ZXY")
        source, target = drr.detector(pose, None)
        img = (target - source).norm(dim=-1)
        source, target = drr.affine_inverse(source), drr.affine_inverse(target)
    return dims, volume, source.contiguous().numpy(), target.contiguous().numpy(), img.contiguous().numpy(), det, \
        (drr, rot, xyz)


def _constructed_rays(name):
    dims, src, centre, col, row = CONSTRUCTED[name]
    f = np.float32
    t = np.array([[f(centre[a]) + f(j - 1) * f(col[a]) + f(i - 1) * f(row[a]) for a in range(3)]
                  for i in range(3) for j in range(3)], f)[None]
    s = np.array(src, f).reshape(1, 1, 3)
    img = np.linalg.norm((t - s).astype(np.float64), axis=-1).astype(f)
    return dims, _volume(dims, "noise"), s, t, img, (3, 3), None


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> namespace: dims, volume, labels, source (B, 1, 3), target (B, N, 3), img (B, N), det, constructed, module
    (the DRR, rot, xyz of a generic scene)."""
    constructed = name in CONSTRUCTED
    dims, volume, s, t, img, det, module = (_constructed_rays if constructed else _generic_rays)(name)
    return SimpleNamespace(name=name, dims=dims, volume=volume, labels=_labels(dims), source=s, target=t, img=img,
                           det=det, constructed=constructed, B=t.shape[0], N=t.shape[1], module=module)


def grad_out(sc):
    g = torch.Generator().manual_seed(7)
    return (torch.rand(sc.B, sc.N, generator=g) + 0.25).numpy() * np.where(np.arange(sc.N) % 3 == 1, -1.0, 1.0).astype(
        np.float32)


# --------------------------------------------------------------------------------- the float64 walk and its sums
def walk64(sc):
    """Every plane crossing of every ray, sorted and tagged: al (B, N, M) alphas, ax (B, N, M) axes, flat (B, N, M - 1)
    the voxel of each segment (-1: outside), d (B, N, 3)."""
    s, t = (np.broadcast_to(x, sc.target.shape).astype(np.float64) for x in (sc.source, sc.target))
    d = t - s + EPS
    al = np.concatenate([((np.arange(sc.dims[a] + 1) - SHIFT) - s[..., a:a + 1]) / d[..., a:a + 1]
                         for a in range(3)], -1)
    ax = np.concatenate([np.full(sc.dims[a] + 1, a) for a in range(3)])
    order = np.argsort(al, -1, kind="stable")
    al, ax = np.take_along_axis(al, order, -1), ax[order]
    mid = (al[..., :-1] + al[..., 1:]) / 2.0
    x = s[..., None, :] + mid[..., None] * d[..., None, :]
    ix = np.rint(np.stack([vc._grid_coord(x[..., a], sc.dims[a]) for a in range(3)], -1))  # (half to even)
    return SimpleNamespace(al=al, ax=ax, flat=vc._flat(ix, sc.dims), d=d)


def sums(w, values, pair=False):
    """The walk's sums over a volume of `values`: I, A (B, N), S0, S1, C0, C1 (B, N, 3).  pair: a crossing counts
    v_before + v_after instead of their difference (the 16-bit quantum of a dV), C0 and C1 only."""
    v = np.where(w.flat >= 0, np.asarray(values, np.float64).reshape(-1)[np.maximum(w.flat, 0)], 0.0)
    da = w.al[..., 1:] - w.al[..., :-1]
    pad = [(0, 0)] * (v.ndim - 1)
    before, after = np.pad(v, pad + [(1, 0)]), np.pad(v, pad + [(0, 1)])
    dv = before + after if pair else before - after
    on = [w.ax == a for a in range(3)]
    r = SimpleNamespace(I=(v * da).sum(-1), A=(np.abs(v) * da).sum(-1))
    r.S0 = np.stack([(dv * m).sum(-1) for m in on], -1)
    r.S1 = np.stack([(dv * w.al * m).sum(-1) for m in on], -1)
    r.C0 = np.stack([(np.abs(dv) * m).sum(-1) for m in on], -1)
    r.C1 = np.stack([(np.abs(dv) * np.abs(w.al) * m).sum(-1) for m in on], -1)
    return r


def tied(w, tie):
    """(B, N) bool: two consecutive crossings of different axes, at least one of them next to an in-volume segment,
    closer in alpha than `tie`."""
    inside = w.flat >= 0
    pad = [(0, 0)] * (inside.ndim - 1)
    cross_in = np.pad(inside, pad + [(1, 0)]) | np.pad(inside, pad + [(0, 1)])  # (B, N, M)
    near = (w.al[..., 1:] - w.al[..., :-1] < tie) & (w.ax[..., 1:] != w.ax[..., :-1])
    return (near & (cross_in[..., 1:] | cross_in[..., :-1])).any(-1)


def _values(sm, go, L, d):
    """{quantity: the walk's value} from the sums of the volume."""
    g, L = go.astype(np.float64), L.astype(np.float64)
    gl = (g * L)[..., None]
    return {"forward": L * sm.I, "I": sm.I, "g_img": g * sm.I, "S0x": sm.S0[..., 0], "S0z": sm.S0[..., 2],
            "S1x": sm.S1[..., 0], "S1z": sm.S1[..., 2], "g_source": gl * (sm.S1 - sm.S0) / d,
            "g_target": -gl * sm.S1 / d, "ident_t": -g * L * sm.I, "ident_s": np.zeros_like(sm.I)}


_emu = []


def _scales(A, C1, W0, W1, go, L, d):
    """({quantity: scale}, {quantity: what forming z from x, y and I rounds, absolute}) from A (B, N), C1 and the
    widened W0, W1 (B, N, 3)."""
    g, L = np.abs(go.astype(np.float64)), L.astype(np.float64)
    T = A + C1.sum(-1)
    all0, all1 = W0.sum(-1), A + W1.sum(-1)
    w0, w1 = W0.copy(), W1.copy()
    w0[..., 1], w1[..., 1] = all0, all1  # the ray's y is formed from the record's x, z and I
    gl = (g * L)[..., None]
    S = {"forward": L * T, "I": T, "g_img": g * T, "S0x": w0[..., 0], "S0z": w0[..., 2], "S1x": w1[..., 0],
         "S1z": w1[..., 2], "g_target": gl * w1 / np.abs(d), "g_source": gl * (w0 + w1) / np.abs(d),
         "ident_t": g * L * all1, "ident_s": g * L * (all0 + all1)}
    # a brick's piece of z is one subtraction from its x, y and I: 2^-24 of what is subtracted
    z0, z1 = np.zeros_like(W0), np.zeros_like(W1)
    z0[..., 2], z1[..., 2] = U * all0, U * all1
    Z = {"S0z": z0[..., 2], "S1z": z1[..., 2], "g_target": gl * z1 / np.abs(d), "g_source": gl * (z0 + z1) / np.abs(d)}
    return S, Z


def _per_ray_record32(sc):
    """The (B, N, 8) record of the per-ray kernel: ops.siddon_forward(..., want_aux=True) with its launch routed to
    the host emulation for the call (as conftest.emulated_ops does), whatever device the test runs on."""
    from diffdrr_amd import ops
    from diffdrr_amd._lib import DdrrLibrary

    if not _emu:
        _emu.append(DdrrLibrary(build_emu()))
    V, s, t, L = (torch.from_numpy(np.ascontiguousarray(x)) for x in (sc.volume, sc.source, sc.target, sc.img))
    real = ops._require_gpu, ops._launch
    ops._require_gpu = lambda volume: None
    ops._launch = lambda name, device, *a: _emu[0].call(name, *a, None)
    try:
        _, aux, _ = ops.siddon_forward(V, s, t, L, voxel_shift=SHIFT, eps=EPS, want_aux=True)
    finally:
        ops._require_gpu, ops._launch = real
    return aux.numpy().astype(np.float64)


def oracle_rays(sc, dtype, go, volume=None):
    """oracle.siddon in `dtype` on the scene's float32 arrays, the source expanded per ray."""
    src = np.broadcast_to(sc.source, sc.target.shape)
    a = [np.ascontiguousarray(x, dtype) for x in (sc.volume if volume is None else volume, src, sc.target, sc.img)]
    r = oracle.siddon(*a, grad_out=go, voxel_shift=SHIFT, eps=EPS)
    return {"forward": r["out"].reshape(sc.B, sc.N).astype(np.float64), "g_img": r["g_img"].reshape(sc.B, sc.N),
            "g_source": r["g_source"], "g_target": r["g_target"]}


_refs = {}


def reference(name):
    """-> namespace: sc, go, w (the walk), o64 {quantity: value}, S {quantity: scale}, r32 {quantity: float32
    reference}, tied / tied_plateau (B, N), rho32 {quantity: this case's}.  Once per process, left unchanged."""
    if name not in _refs:
        sc = scene(name)
        go = grad_out(sc)
        w = walk64(sc)
        sm = sums(w, sc.volume)
        wide = sums(w, np.abs(sc.volume), pair=True)
        o64 = _values(sm, go, sc.img, w.d)
        S, Z = _scales(sm.A, sm.C1, wide.C0, wide.C1, go, sc.img, w.d)
        r32 = oracle_rays(sc, np.float32, go)
        rec = _per_ray_record32(sc)
        r32.update({"I": rec[..., 0], "S0x": rec[..., 1], "S0z": rec[..., 3], "S1x": rec[..., 4], "S1z": rec[..., 6]})
        ref = SimpleNamespace(sc=sc, go=go, w=w, sm=sm, o64=o64, S=S, Z=Z, r32=r32, tied=tied(w, TIE),
                              tied_plateau=tied(w, TIE_PLATEAU))
        ref.rho32 = {q: rho_of(ref, q, ref.tied) for q in QUANTITIES}
        ref.rho32["ident_t"], ref.rho32["ident_s"] = ref.rho32["I"], ref.rho32["I"]
        _refs[name] = ref
    return _refs[name]


def rho_of(ref, q, left_out):
    """max |float32 reference - walk64| / S of quantity q over the rays not `left_out` (tie-sensitive quantities
    only; a constructed scene is all ties: 0)."""
    err, S = np.abs(ref.r32[q] - ref.o64[q]), ref.S[q]
    live = S > 0
    if q in TIED_QUANTITIES:
        if ref.sc.constructed:
            return 0.0
        live = live & ~left_out.reshape(left_out.shape + (1,) * (err.ndim - 2))
    return float((err[live] / S[live]).max()) if live.any() else 0.0


def rho32(ref, q):
    key = "I" if q.startswith("ident") else q
    assert ref.rho32[q] <= RHO32_CAP[key], \
        f"[{ref.sc.name}] the float32 yardstick of {q} is {ref.rho32[q]:.3e} from float64: over its cap"
    return ref.rho32[q]


def brick_dims(storage, host):
    if storage == "f32" or host:
        return (32, 32, 32)
    return (32, 64, 32) if storage.endswith("y") else (32, 32, 64)


@functools.lru_cache(maxsize=None)
def q16_terms(name, bdims):
    """({quantity: allowance of the 16-bit quantisation on the `bdims` grid}, brick_levels' fallback flags)."""
    ref = reference(name)
    level, flags = brick_levels(ref.sc.volume, bdims)
    Q = (Q16_RANGE_OVER_LEVEL / 131070.0) * level
    sq = sums(ref.w, Q, pair=True)
    g, L, d = np.abs(ref.go.astype(np.float64)), ref.sc.img.astype(np.float64), np.abs(ref.w.d)
    gl = (g * L)[..., None]
    p0, p1 = sq.C0.copy(), sq.C1.copy()  # a crossing's two voxels: Q_before + Q_after, summed like W0 / W1
    p0[..., 1], p1[..., 1] = sq.C0.sum(-1), sq.A + sq.C1.sum(-1)  # y is formed from x, z and I
    return {"forward": L * sq.A, "I": sq.A, "g_img": g * sq.A, "S0x": p0[..., 0], "S0z": p0[..., 2], "S1x": p1[..., 0],
            "S1z": p1[..., 2], "g_target": gl * p1 / d, "g_source": gl * (p0 + p1) / d, "ident_t": g * L * sq.A,
            "ident_s": np.zeros_like(L)}, flags


@functools.lru_cache(maxsize=None)
def packed_terms(name, bdims):
    """{quantity: allowance of the packed record's fixed point} for pieces from the `bdims` grid (gradients only)."""
    ref = reference(name)
    sc, w = ref.sc, ref.w
    vmax = float(np.abs(sc.volume).max())
    res = 2.0 * vmax * (sum(sc.dims) + 3) / 2.0 ** 30
    inside = w.flat >= 0
    i = np.maximum(w.flat, 0)
    ixyz = np.stack([i // (sc.dims[1] * sc.dims[2]), i // sc.dims[2] % sc.dims[1], i % sc.dims[2]], -1)
    b = ixyz // np.asarray(bdims)
    bid = np.where(inside, (b[..., 0] * 64 + b[..., 1]) * 64 + b[..., 2], -1)
    srt = np.sort(bid, -1)
    n = ((srt[..., 1:] != srt[..., :-1]) & (srt[..., 1:] >= 0)).sum(-1) + (srt[..., 0] >= 0)  # bricks passed
    pad = [(0, 0)] * (inside.ndim - 1)
    cross_in = np.pad(inside, pad + [(1, 0)]) | np.pad(inside, pad + [(0, 1)])
    Amax = np.maximum(1.0, np.where(cross_in, np.abs(w.al), 0.0).max(-1))
    e0 = np.repeat((n * res / 2.0)[..., None], 3, -1)
    e1 = e0 * Amax[..., None]
    e0[..., 1], e1[..., 1] = 2 * e0[..., 1], 2 * e1[..., 1]  # y = -(x + z)
    g, L = np.abs(ref.go.astype(np.float64)), sc.img.astype(np.float64)
    gl = (g * L)[..., None]
    zero = np.zeros_like(L)
    return {"g_img": zero, "forward": zero, "g_target": gl * e1 / np.abs(w.d), "g_source": gl * (e0 + e1) / np.abs(w.d),
            "ident_t": zero, "ident_s": zero}, vmax


def check_left_out(ref):
    share = float(ref.tied.mean())
    if not ref.sc.constructed:
        assert share <= LEFT_OUT_CAP, f"{ref.sc.name}: {share:.2%} of the rays hold a tie closer than {TIE}"
    return share


# --------------------------------------------------------------------------------------------------------- gate
def gate(tag, q, got, ref, terms=(), rendered=None, extra=0.0):
    """-> problems of `got` against the walk's quantity q; prints the worst kernel error / allowance.  `terms`: dicts of
    storage allowances to add; `rendered` (N,) bool: the masked entry's pixels (the others must be exactly 0);
    `extra`: a further allowance in units of S_p."""
    want, S = ref.o64[q], ref.S[q]
    got = np.asarray(got, np.float64).reshape(want.shape)
    term = sum((t[q] for t in terms), np.zeros_like(S)) + ref.Z.get(q, 0.0)
    tol = (2 * rho32(ref, q) + 8 * U + extra) * S + term
    err = np.abs(got - want)
    wide = lambda m: np.broadcast_to(m.reshape(m.shape + (1,) * (got.ndim - m.ndim)), got.shape)  # noqa: E731
    keep = np.ones(got.shape, bool)
    if q in TIED_QUANTITIES:
        keep &= ~wide(np.ones_like(ref.tied) if ref.sc.constructed else ref.tied)
    problems = []
    if rendered is not None:
        on = wide(np.broadcast_to(rendered, (ref.sc.B, ref.sc.N)))
        if (got[~on] != 0).any():
            problems.append(f"{tag} {q}: {int((got[~on] != 0).sum())} entries of masked-out pixels are not 0")
        keep &= on
    if not np.isfinite(got).all():
        problems.append(f"{tag} {q}: {int((~np.isfinite(got)).sum())} non-finite values")
    dark = keep & (tol == 0)
    if (got[dark] != 0).any():
        problems.append(f"{tag} {q}: {int((got[dark] != 0).sum())} entries of rays without a segment in the volume are "
                        f"not 0 (largest {np.abs(got[dark]).max():.3e})")
    lit = keep & (tol > 0)
    worst = float((err[lit] / tol[lit]).max()) if lit.any() else 0.0
    print(f"{tag} {q}: kernel error / allowance {worst:.3f} ({int(lit.sum())} entries, rho32 {rho32(ref, q):.3e})")
    over = lit & ~(err <= tol)
    if over.any():
        at = np.unravel_index(np.argmax(np.where(over, err / np.maximum(tol, 1e-300), 0)), got.shape)
        problems.append(f"{tag} {q}: {int(over.sum())} entries over the allowance, worst {worst:.2f} x at {at}: got "
                        f"{got[at]:.9e} float64 {want[at]:.9e} S {S[at]:.3e}")
    return problems


def gate_gradients(tag, grads, ref, terms=(), rendered=None):
    """g_source, g_target per ray and component, g_img, and the two identities of the record on every ray."""
    gs, gt, gi = (_np(x).astype(np.float64) for x in grads)
    problems = gate(tag, "g_img", gi, ref, terms, rendered)
    problems += gate(tag, "g_source", gs, ref, terms, rendered)
    problems += gate(tag, "g_target", gt, ref, terms, rendered)
    problems += gate(tag, "ident_t", (ref.w.d * gt).sum(-1), ref, terms, rendered)
    problems += gate(tag, "ident_s", (ref.w.d * (gs + gt)).sum(-1), ref, terms, rendered)
    return problems


# ------------------------------------------------------------------------------------------------------- checks
def _upload(sc, device):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    return SimpleNamespace(V=dev(sc.volume), labels=dev(sc.labels), s=dev(sc.source), t=dev(sc.target), L=dev(sc.img))


def _host(device):
    return torch.device(device).type == "cpu"


def _np(x):
    return x.detach().cpu().numpy()


def _nan_out(sc, device):
    return torch.full((sc.B, sc.N), float("nan"), dtype=torch.float32, device=device)


def _nan_record(sc, device, ops):
    return ops.brick_record_buffer(sc.B, sc.N, device).fill_(float("nan"))


def _storage_terms(name, storage, device):
    """(the storage's allowances, brick_levels' flags); a volume of fewer than four slices is rendered from its fp32
    values whatever the storage (ops.brick_storage_applies): no term, and no workspace to report from."""
    if storage == "f32" or scene(name).dims[2] < 4:
        return (), None
    terms, flags = q16_terms(name, brick_dims(storage, _host(device)))
    return (terms,), flags


def _check_fallbacks(tag, ops, V, storage, flags):
    if flags is None:
        assert storage == "f32" or ops.brick_fallbacks(V, storage) is None, f"{tag}: a workspace no launch has built"
    else:
        assert ops.brick_fallbacks(V, storage) == (int(flags.sum()), flags.size), \
            f"{tag}: bricks on the fp32 path {ops.brick_fallbacks(V, storage)}, brick_levels {int(flags.sum())}"


def check_forward_and_record(name, storage, device, ops):
    """The forward-only walk, the walk with the record (image, the five planes, the ray gradients from them) and the
    record alone, per pixel against float64."""
    ref = reference(name)
    sc, tag = ref.sc, f"[{name} {storage}]"
    share = check_left_out(ref)
    print(f"{tag} rays left out of the per-axis gates: {share:.2%}")
    r = _upload(sc, device)
    terms, flags = _storage_terms(name, storage, device)
    go = torch.from_numpy(ref.go).to(device)
    plain, none = ops.siddon_forward_bricks(r.V, r.s, r.t, r.L, sc.det, storage=storage, out=_nan_out(sc, device))
    assert none is None
    problems = gate(tag + " forward only", "forward", _np(plain), ref, terms)
    _check_fallbacks(tag, ops, r.V, storage, flags)
    out, aux = ops.siddon_forward_bricks(r.V, r.s, r.t, r.L, sc.det, storage=storage, want_aux=True,
                                         out=_nan_out(sc, device), aux=_nan_record(sc, device, ops))
    assert aux.shape == (-(-sc.B * sc.N // 16), 80)
    problems += gate(tag + " with the record", "forward", _np(out), ref, terms)
    planes = _np(ops.record_planes(aux, sc.B, sc.N))
    for k, q in enumerate(PLANES):
        problems += gate(tag + " record", q, planes[k], ref, terms)
    problems += gate_gradients(tag + " record", ops.siddon_backward_rays(aux, go, r.s, r.t, r.L), ref, terms)
    nothing, aux2 = ops.siddon_forward_bricks(r.V, r.s, r.t, r.L, sc.det, storage=storage, want_aux=True,
                                              want_image=False, aux=_nan_record(sc, device, ops))
    assert nothing is None
    planes2 = _np(ops.record_planes(aux2, sc.B, sc.N))
    for k, q in enumerate(PLANES):
        problems += gate(tag + " record alone", q, planes2[k], ref, terms)
    assert float(np.abs(ref.o64["forward"]).max()) > 0
    assert not problems, "\n".join(problems)


def check_packed_record(name, storage, device, ops):
    """The packed fixed-point record (record_vmax > 0): the ray gradients from it per ray and component, the image of
    its launch, and the same bits from two launches."""
    ref = reference(name)
    sc, tag = ref.sc, f"[{name} {storage} packed]"
    r = _upload(sc, device)
    terms, flags = _storage_terms(name, storage, device)
    fixed, vmax = packed_terms(name, brick_dims(storage, _host(device)))
    go = torch.from_numpy(ref.go).to(device)
    kw = dict(storage=storage, want_aux=True, record_vmax=vmax)
    out, aux = ops.siddon_forward_bricks(r.V, r.s, r.t, r.L, sc.det, out=_nan_out(sc, device), **kw)
    assert aux.shape == (7, sc.B, sc.N)
    _check_fallbacks(tag, ops, r.V, storage, flags)
    problems = gate(tag, "forward", _np(out), ref, terms)
    problems += gate_gradients(tag, ops.siddon_backward_rays(aux, go, r.s, r.t, r.L), ref, terms + (fixed,))
    _, again = ops.siddon_forward_bricks(r.V, r.s, r.t, r.L, sc.det, **kw)
    if not torch.equal(aux[:4].view(torch.int32), again[:4].view(torch.int32)):
        problems.append(f"{tag}: two launches give different fixed-point planes")
    assert not problems, "\n".join(problems)


def pixel_mask(sc, kind):
    """(N,) bool of the rendered pixels: a random half, one pixel, none."""
    on = np.zeros(sc.N, bool)
    if kind == "half":
        on[np.random.default_rng(3).permutation(sc.N)[: sc.N // 2]] = True
    elif kind == "single":
        on[(sc.det[0] // 2) * sc.det[1] + sc.det[1] // 2] = True
    return on


def check_masked(name, kind, storage, device, ops):
    """ddrr_siddon_forward_bricks_masked: the rendered pixels pass the same gates, everything else is exactly 0."""
    ref = reference(name)
    sc, tag = ref.sc, f"[{name} {storage} mask {kind}]"
    r = _upload(sc, device)
    terms, _ = _storage_terms(name, storage, device)
    on = pixel_mask(sc, kind)
    mask = ops.pixel_mask_of(torch.from_numpy(np.flatnonzero(on)).to(device), sc.N)
    go = torch.from_numpy(ref.go).to(device)
    kw = dict(storage=storage, pixel_mask=mask)
    plain, _ = ops.siddon_forward_bricks(r.V, r.s, r.t, r.L, sc.det, out=_nan_out(sc, device), **kw)
    problems = gate(tag + " forward only", "forward", _np(plain), ref, terms, on)
    out, aux = ops.siddon_forward_bricks(r.V, r.s, r.t, r.L, sc.det, want_aux=True, out=_nan_out(sc, device),
                                         aux=_nan_record(sc, device, ops), **kw)
    problems += gate(tag + " with the record", "forward", _np(out), ref, terms, on)
    planes = _np(ops.record_planes(aux, sc.B, sc.N))
    for k, q in enumerate(PLANES):
        problems += gate(tag + " record", q, planes[k], ref, terms, on)
    problems += gate_gradients(tag + " record", ops.siddon_backward_rays(aux, go, r.s, r.t, r.L), ref, terms, on)
    assert not problems, "\n".join(problems)


def check_cleared(name, device, ops):
    """A record buffer and a launch workspace brought by the caller, cleared by ddrr_pose_raygen_forward's launch
    (as lm_cases.render_record does), then the record alone with cleared=True."""
    from diffdrr_amd.pose import _AXIS

    ref = reference(name)
    sc, tag = ref.sc, f"[{name} cleared]"
    drr, rot, xyz = sc.module
    r = _upload(sc, device)
    P = drr._calibrated_points().to(device)
    Ainv = (drr._affine_inverse[0, :3, :] if drr._affine_inverse.dim() == 3 else drr._affine_inverse[:3, :]).to(device)
    reorient34 = drr.detector._reorient[:3, :].contiguous().to(device)
    aux = _nan_record(sc, device, ops)
    ws = ops.launch_workspace(r.V.shape, r.V.device)
    _, s, t, L = ops.pose_raygen_forward(rot.to(device), xyz.to(device), tuple(_AXIS[c] for c in "ZXY"), reorient34,
                                         Ainv, P, clear=aux, clear_launch_ws=ws)
    assert not _np(aux).any(), f"{tag}: the record is not cleared"
    # (the launch's own rays are the scene's to float32 rounding; the render takes the scene's, which the walk has)
    assert np.abs(_np(t) - sc.target).max() <= 1e-3 and np.abs(_np(L) - sc.img).max() <= 1e-3
    nothing, same = ops.siddon_forward_bricks(r.V, r.s, r.t, r.L, sc.det, want_aux=True, want_image=False, aux=aux,
                                              launch_ws=ws, cleared=True)
    assert nothing is None and same is aux
    planes = _np(ops.record_planes(aux, sc.B, sc.N))
    problems = []
    for k, q in enumerate(PLANES):
        problems += gate(tag + " record", q, planes[k], ref)
    go = torch.from_numpy(ref.go).to(device)
    problems += gate_gradients(tag + " record", ops.siddon_backward_rays(aux, go, r.s, r.t, r.L), ref)
    assert not problems, "\n".join(problems)


_channel_refs = {}


def channel_reference(name):
    """Per channel c the walk's image of the volume with every other label set to 0, its scale, and rho32 from the
    float32 oracle on the same volume: (want (B, C, N), S (B, C, N), rho32)."""
    if name not in _channel_refs:
        ref = reference(name)
        sc = ref.sc
        want, S, rho = [], [], 0.0
        L = sc.img.astype(np.float64)
        for c in range(N_LABELS):
            vol = np.where(sc.labels == c, sc.volume, np.float32(0))
            sm = sums(ref.w, vol)
            want.append(L * sm.I)
            S.append(L * (sm.A + sm.C1.sum(-1)))
            o32 = oracle_rays(sc, np.float32, ref.go, vol)["forward"]
            live = S[-1] > 0
            if live.any():
                rho = max(rho, float((np.abs(o32 - want[-1])[live] / S[-1][live]).max()))
        _channel_refs[name] = (np.stack(want, 1), np.stack(S, 1), rho)
    return _channel_refs[name]


def check_channels(name, device, ops):
    """ddrr_siddon_forward_channels_bricks: every channel image per pixel against the walk of that label's voxels, and
    the channel sum against the plain forward; the staged words keep 16 significant bits: 2^-16 S_p more."""
    ref = reference(name)
    sc, tag = ref.sc, f"[{name} channels]"
    r = _upload(sc, device)
    want, S, rho = channel_reference(name)
    assert rho <= RHO32_CAP["forward"], f"{tag} the float32 yardstick of the channels is {rho:.3e} from float64"
    ch = _np(ops.siddon_forward_channels_bricks(r.V, r.labels, N_LABELS, r.s, r.t, r.L, sc.det)).astype(np.float64)
    assert ch.shape == want.shape
    problems = gate(tag + " channel sum", "forward", ch.sum(1), ref, extra=2.0 ** -16)
    tol = (2 * rho + 8 * U + 2.0 ** -16) * S
    err = np.abs(ch - want)
    lit = S > 0
    worst = float((err[lit] / tol[lit]).max()) if lit.any() else 0.0
    print(f"{tag} per channel: kernel error / allowance {worst:.3f} ({int(lit.sum())} entries, rho32 {rho:.3e})")
    if not np.isfinite(ch).all():
        problems.append(f"{tag}: non-finite values")
    if (ch[~lit] != 0).any():
        problems.append(f"{tag}: {int((ch[~lit] != 0).sum())} entries of channels the ray does not meet are not 0")
    if not (err[lit] <= tol[lit]).all():
        problems.append(f"{tag}: {int((err[lit] > tol[lit]).sum())} entries over the allowance, worst {worst:.2f} x")
    assert not problems, "\n".join(problems)
