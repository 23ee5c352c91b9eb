"""What tests/test_mvlm.py (host emulation) and tests/test_gpu_mvlm.py (MI355X) share: the host build of
csrc/mvlm_core.h (tests/emu/mvlm_emu.cpp), the views, the yardsticks of the multi-view Levenberg-Marquardt kernels
(include/diffdrr_mvlm_hip.h) and the checks, written once as ``check_*(..., device, ops)``.

The scenes (lm_cases.SUM_CASES), the gate of the sums (|kernel - truth| <= 2 |float32 route - truth| + FLOOR x the
Cauchy-Schwarz scale of the sum, FLOOR = 1e-6), the step's measure (``ulps32`` <= 2), the step sequences and the
convergence target are tests/lm_cases.py's.  A rendered pose is ``b = s * V + v``; start ``s`` of a case is row ``s`` of
the case's three parameter rows and view ``v`` is orbit angle ``ANGLES[v]``, whatever (S, V) is, so that the float64
yardstick of a scene -- one-hot autograd through ``view_poses`` for all nine (start, view) pairs -- is computed once per
scene and device and shared by the four (S, V) of that scene.  The float32 route (one-hot calls of the existing
``ddrr_siddon_backward_pose_euler`` with ``Ro_v``) reads the record of the batch under test on the device, where two
renders differ in their last bits; the host build renders reproducibly, so there it is taken once from the record of
the nine pairs, and the kernel's rows are asserted equal to it bit for bit."""
import contextlib
import copy
import functools
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import lm_cases
from conftest import ROOT
from diffdrr_amd import MultiViewLevenbergMarquardt, Registration, _lib, convert
from diffdrr_amd.registration import (
    multiview_normal_equations_reference, normal_equations_reference, relative_views, view_poses,
)
from lm_cases import FLOOR, HYPER, OFFSET, TRUTH, _reached, sums_of, ulps32

EMU_SRC = os.path.join(ROOT, "tests", "emu", "mvlm_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "_build", "libmvlm_emu.so")
GROUP = _lib.MVLM_GROUP_RAYS
ANGLES = (0.0, math.pi / 2, 2.2)  # orbit angles about the first Euler axis
SV = ((1, 1), (1, 2), (2, 3), (3, 2))
SV_IDS = [f"S{s}_V{v}" for s, v in SV]
NAMES = sorted(lm_cases.SUM_CASES)


@functools.lru_cache(maxsize=None)
def emu_library():
    """The host build of the three entries (tests/emu/mvlm_emu.cpp), bound through the product's own binding."""
    csrc = os.path.join(ROOT, "diffdrr_amd", "csrc")
    deps = [EMU_SRC, lm_cases.EMU_LOOPS]
    deps += [os.path.join(ROOT, "include", f) for f in ("diffdrr_mvlm_hip.h", "diffdrr_lm_hip.h")]
    deps += [os.path.join(csrc, f) for f in ("mvlm_core.h", "lm_core.h", "siddon_core.h", "raygen_core.h",
                                             "record_layout.h", "ddrr_common.h")]
    if not (os.path.exists(EMU_SO) and all(os.path.getmtime(d) <= os.path.getmtime(EMU_SO) for d in deps)):
        os.makedirs(os.path.dirname(EMU_SO), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-mfma", "-ffp-contract=off",
                        "-Wno-unknown-pragmas", EMU_SRC, "-o", EMU_SO], check=True)
    return _lib.mvlm_library(EMU_SO)


def route_mvlm_to_emulation(monkeypatch, ops):
    """The launcher patch of the host tests: ops' multi-view Levenberg-Marquardt launches go to the host build."""
    lib = emu_library()
    monkeypatch.setattr(ops, "_launch_mvlm", lambda name, device, *a: lib.call(name, *a, None))
    monkeypatch.setattr(ops, "_query_mvlm", lambda name, *a: lib.query(name, *a))


@contextlib.contextmanager
def launches(ops):
    """the names of the C-ABI entries launched inside the block: the main library's and the LM libraries'"""
    names, real = [], {k: getattr(ops, k) for k in ("_launch", "_launch_lm", "_launch_wlm", "_launch_mvlm")}
    for k, fn in real.items():
        setattr(ops, k, lambda name, device, *a, _fn=fn: (names.append(name), _fn(name, device, *a))[1])
    try:
        yield names
    finally:
        for k, fn in real.items():
            setattr(ops, k, fn)


# ------------------------------------------------------------------------------------------------ views and scenes
def orbit_views(conv, angles=ANGLES, distance=400.0):
    """K_v = E_0^-1 E(angle_v), (V, 4, 4) float64: E(a) the Euler pose (a, 0, 0), (0, distance, 0) -- the C-arm
    moved by `a` about the first Euler axis around the isocentre, so that every view sees the volume."""
    rot = torch.tensor([[a, 0.0, 0.0] for a in angles], dtype=torch.float64)
    xyz = torch.tensor([[0.0, distance, 0.0]], dtype=torch.float64).expand(len(angles), 3)
    return relative_views(convert(rot, xyz, parameterization="euler_angles", convention=conv))


def reorients(drr, K):
    """Ro_v = (K_v @ reorient)[:3] in float64, rounded once: (V, 3, 4) float32 on the module's device"""
    Ro = drr.detector._reorient.detach().double().cpu()
    return (K.double().cpu() @ Ro)[:, :3, :].to(torch.float32).contiguous().to(drr.density.device)


@functools.lru_cache(maxsize=None)
def starts(name):
    """the three parameter rows of a case (seeded), around the isocentre pose"""
    g = torch.Generator().manual_seed(17 + len(name))
    rot = (torch.rand(3, 3, generator=g) - 0.5) * 0.6
    xyz = torch.tensor([0.0, 400.0, 0.0]) + (torch.rand(3, 3, generator=g) - 0.5) * 20
    return rot, xyz


def render(drr, rot, xyz, conv, Ro, ops, clear=True):
    """The first two launches of a multi-view step at (rot, xyz) (S, 3) and Ro (V, 3, 4): everything
    ddrr_mvlm_normal_sums reads -> (aux, args, kw, x32 (S V, N), (target, img))"""
    from diffdrr_amd.pose import _AXIS

    det = drr.detector
    P = drr._calibrated_points()
    Ainv = drr._affine_inverse[0, :3, :] if drr._affine_inverse.dim() == 3 else drr._affine_inverse[:3, :]
    cfg = drr.renderer._cfg(False, det=(det.height, det.width))
    axes = tuple(_AXIS[c] for c in conv)
    B, N = rot.shape[0] * Ro.shape[0], P.shape[0]
    aux = ops.brick_record_buffer(B, N, rot.device)
    launch_ws = ops.launch_workspace(drr.density.shape, drr.density.device)
    if clear:
        Mw, source, target, img = ops.mvlm_raygen(rot, xyz, axes, Ro, Ainv, P, clear=aux, clear_launch_ws=launch_ws)
    else:  # (the clears by torch: the record the check of the clears compares with)
        aux.zero_()
        launch_ws.zero_()
        Mw, source, target, img = ops.mvlm_raygen(rot, xyz, axes, Ro, Ainv, P)
    ops.siddon_forward_bricks(drr.density, source, target, img, cfg["det"], voxel_shift=cfg["voxel_shift"],
                              eps=cfg["eps"], want_aux=True, storage="f32", want_image=False, aux=aux,
                              launch_ws=launch_ws, cleared=True)
    x32 = img * ops.record_planes(aux, B, N)[0]
    args = dict(source=source, Mw=Mw, Ainv=Ainv, P=P, rot=rot, xyz=xyz, axes=axes, reorient_v=Ro)
    return aux, args, dict(eps=cfg["eps"], with_img_path=not cfg["stop_gradients"]), x32, (target, img)


def float64_pairs(drr, rot, xyz, K, conv):
    """x (S, V, N) and J (S, V, N, 6) from the package's float64 render route at view_poses(...), one-hot
    autograd.grad per pixel.  The chain is cut at the S V pose matrices, so that the N one-hot calls walk the render
    alone: d image / d matrix per pixel by autograd.grad, d matrix / d theta of view_poses once per (start, view) pair
    by autograd's jacobian, and their product.  (A pair has a row of its own: nothing is summed over a start's views.)"""
    d64 = copy.deepcopy(drr).to(torch.float64)
    S, V = rot.shape[0], K.shape[0]
    theta = torch.cat([rot, xyz], 1).double().cpu()

    def matrix(th, v):
        return view_poses(th[None, :3], th[None, 3:], K[v:v + 1], conv).matrix[0]

    dM = torch.stack([torch.autograd.functional.jacobian(lambda th, v=v: matrix(th, v), theta[s])
                      for s in range(S) for v in range(V)])  # (S V, 4, 4, 6)
    with torch.no_grad():
        mats = view_poses(rot.double(), xyz.double(), K, conv).matrix
    mats = mats.clone().requires_grad_()
    flat = d64(convert(mats, parameterization="matrix")).reshape(S * V, -1)
    N = flat.shape[1]
    G = torch.zeros(S * V, N, 4, 4, dtype=torch.float64)
    hot = torch.zeros_like(flat)
    for n in range(N):
        hot[:, n] = 1.0
        G[:, n] = torch.autograd.grad(flat, mats, grad_outputs=hot, retain_graph=True)[0].cpu()
        hot[:, n] = 0.0
    J = torch.einsum("bnij,bijk->bnk", G, dM)
    return flat.detach().cpu().reshape(S, V, N).numpy(), J.reshape(S, V, N, 6).numpy()


def float32_route(aux, args, kw, ops):
    """J (S V, N, 6) from one-hot calls of the existing float32 entry, ddrr_siddon_backward_pose_euler, once per view
    on the whole batch with reorient34 = Ro_v and the theta rows repeated; pose b takes the call of view b % V."""
    Ro = args["reorient_v"]
    V, S = Ro.shape[0], args["rot"].shape[0]
    B, N = S * V, args["P"].shape[0]
    one = {k: args[k] for k in ("source", "Mw", "Ainv", "P", "axes")}
    one["rot"], one["xyz"] = args["rot"].repeat_interleave(V, 0), args["xyz"].repeat_interleave(V, 0)
    J = torch.zeros(B, N, 6, dtype=torch.float32)
    hot = torch.zeros(B, N, dtype=torch.float32, device=Ro.device)
    for v in range(V):
        for n in range(N):
            hot[:, n] = 1.0
            g_r, g_t = ops.siddon_backward_pose_euler(aux, hot, **one, reorient34=Ro[v].contiguous(), **kw)
            hot[:, n] = 0.0
            J[v::V, n, :3], J[v::V, n, 3:] = g_r.cpu()[v::V], g_t.cpu()[v::V]
    return J.numpy()


_scenes = {}


def scene(name, device, ops):
    """A case of lm_cases.SUM_CASES on `device` with its three starts and three views: the module, the fixed images
    (the views of the isocentre pose) and the yardsticks of the nine pairs (computed once, never modified)."""
    key = (name, str(device))
    if key not in _scenes:
        drr_cpu, _, _, conv = lm_cases.sum_scene(name)
        drr = copy.deepcopy(drr_cpu).to(device)
        rot, xyz = (t.to(device) for t in starts(name))
        K = orbit_views(conv)
        Ro = reorients(drr, K)
        with torch.no_grad():
            fixed = drr(view_poses(torch.zeros(1, 3, device=device), torch.tensor([[0.0, 400.0, 0.0]], device=device),
                                   K, conv)).reshape(3, -1).contiguous()
        assert float(fixed.abs().amax(1).min()) > 0  # (every view sees the volume)
        _scenes[key] = dict(drr=drr, conv=conv, rot=rot, xyz=xyz, K=K, Ro=Ro, fixed=fixed, N=fixed.shape[1])
    return _scenes[key]


def yardsticks(sc, device, ops):
    """x64 (3, 3, N), J64 (3, 3, N, 6) of a scene's nine pairs and, on the host build, J32 (3, 3, N, 6) of the same:
    there a ray's record does not depend on the batch it is rendered in, so the one-hot calls run on one record per
    view (three poses each), a third of the work of the nine poses' record."""
    if "J64" not in sc:
        sc["x64"], sc["J64"] = float64_pairs(sc["drr"], sc["rot"], sc["xyz"], sc["K"], sc["conv"])
        if device.type == "cpu":
            per_view = []
            for v in range(3):
                aux, args, kw, _, _ = render(sc["drr"], sc["rot"], sc["xyz"], sc["conv"], sc["Ro"][v:v + 1], ops)
                per_view.append(float32_route(aux, args, kw, ops))  # (3, N, 6)
            sc["J32"] = np.stack(per_view, axis=1)
    return sc


def batch(sc, S, V, ops, **more):
    """the (S, V) batch of a scene, rendered: its first S starts seen from its first V views"""
    rot, xyz, Ro = sc["rot"][:S].contiguous(), sc["xyz"][:S].contiguous(), sc["Ro"][:V].contiguous()
    aux, args, kw, x32, rays = render(sc["drr"], rot, xyz, sc["conv"], Ro, ops, **more)
    return dict(S=S, V=V, N=sc["N"], aux=aux, args=args, kw=kw, x32=x32, rays=rays,
                fixed=sc["fixed"][:V].contiguous())


# ------------------------------------------------------------------------------------------------ ray generation
def check_raygen(name, S, V, device, ops):
    """Mw, source, target and img of pose (s, v) equal, bit for bit, what ops.pose_raygen_forward(rot_s, xyz_s, axes,
    Ro_v, ...) writes; the clears leave `clear_floats` floats and the first 16 bytes of the launch workspace zero and
    nothing beyond; the record of the render behind the clears is the record behind torch's zero-fill."""
    sc = scene(name, device, ops)
    b = batch(sc, S, V, ops)
    a, (target, img) = b["args"], b["rays"]
    N = b["N"]
    assert a["Mw"].shape == (S * V, 3, 4) and a["source"].shape == (S * V, 1, 3)
    assert target.shape == (S * V, N, 3) and img.shape == (S * V, N)
    for s in range(S):
        for v in range(V):
            Mw, source, tgt, im = ops.pose_raygen_forward(a["rot"][s:s + 1], a["xyz"][s:s + 1], a["axes"],
                                                          a["reorient_v"][v].contiguous(), a["Ainv"], a["P"])
            p = s * V + v
            assert torch.equal(a["Mw"][p], Mw[0]) and torch.equal(a["source"][p], source[0]), (s, v)
            assert torch.equal(target[p], tgt[0]) and torch.equal(img[p], im[0]), (s, v)
    # the clears: 1003 floats (three quads' worth of tail) of 1024, 16 bytes of 32
    junk = torch.full((1024,), 7.0, device=device)
    counter = torch.full((8,), 5, dtype=torch.int32, device=device)
    ops.mvlm_raygen(a["rot"], a["xyz"], a["axes"], a["reorient_v"], a["Ainv"], a["P"], clear=junk[:1003],
                    clear_launch_ws=counter)
    assert not bool(junk[:1003].any()) and bool((junk[1003:] == 7.0).all())
    assert counter.tolist() == [0, 0, 0, 0, 5, 5, 5, 5]
    if device.type == "cpu":  # (a render is reproducible on the host build alone)
        assert torch.equal(batch(sc, S, V, ops, clear=False)["aux"], b["aux"])
    else:
        planes = ops.record_planes(b["aux"], S * V, N)
        other = ops.record_planes(batch(sc, S, V, ops, clear=False)["aux"], S * V, N)
        assert torch.allclose(planes, other, rtol=1e-4, atol=1e-4 * float(other.abs().max()))


# ------------------------------------------------------------------------------------------------ sums
def mv_sums(b, ops, **more):
    return ops.mvlm_normal_sums(b["aux"], b["fixed"], **b["args"], **b["kw"], **more)


def check_sums_bit_for_bit(name, S, V, device, ops):
    """On ONE record: ops.lm_normal_sums on the whole batch once per view, with reorient34 = Ro_v, the theta rows
    repeated and view v's fixed image; its rows with b % V == v equal the new entry's partials and jac bit for bit.
    A second call gives the same bits; a neighbouring start's parameters do not enter a start's rows."""
    sc = scene(name, device, ops)
    b = batch(sc, S, V, ops)
    a, N = b["args"], b["N"]
    ws, jac = mv_sums(b, ops, want_jacobian=True)
    assert ws.shape == (S * V, -(-N // GROUP), _lib.MVLM_SUMS) and jac.shape == (S * V, N, 6)
    assert ws.dtype == torch.float64 and bool(torch.isfinite(ws).all())
    one = {k: a[k] for k in ("source", "Mw", "Ainv", "P", "axes")}
    one["rot"], one["xyz"] = a["rot"].repeat_interleave(V, 0), a["xyz"].repeat_interleave(V, 0)
    for v in range(V):
        ws_v, jac_v = ops.lm_normal_sums(b["aux"], b["fixed"][v:v + 1], **one, reorient34=a["reorient_v"][v].contiguous(),
                                         **b["kw"], want_jacobian=True)
        assert torch.equal(ws_v[v::V], ws[v::V]), (v, float((ws_v[v::V] - ws[v::V]).abs().max()))
        assert torch.equal(jac_v[v::V], jac[v::V]), v
        if V > 1:  # (another view's rows differ: a swapped b / V and b % V cannot pass)
            w = (v + 1) % V
            assert not torch.equal(ws_v[w::V], ws[w::V]) and not torch.equal(jac_v[w::V], jac[w::V])
    again, _ = mv_sums(b, ops)
    assert torch.equal(again, ws)
    if S > 1:  # start 1 somewhere else, the record as it is: the other starts' rows keep their bits
        moved = dict(b, args=dict(a, rot=a["rot"].clone(), xyz=a["xyz"].clone()))
        moved["args"]["rot"][1] += 0.05
        moved["args"]["xyz"][1] -= 3.0
        ws_m, jac_m = mv_sums(moved, ops, want_jacobian=True)
        keep = torch.tensor([p // V != 1 for p in range(S * V)], device=device)
        assert torch.equal(ws_m[keep], ws[keep]) and torch.equal(jac_m[keep], jac[keep])
        assert not torch.equal(jac_m[~keep], jac[~keep])


def check_sums_against_float64(name, S, V, device, ops):
    """The 44 sums and the per-ray Jacobian of every pose against the float64 route at view_poses(...), under
    lm_cases' gate with the float32 route (one-hot ddrr_siddon_backward_pose_euler with Ro_v) on the same record."""
    sc = yardsticks(scene(name, device, ops), device, ops)
    b = batch(sc, S, V, ops)
    N, B = b["N"], S * V
    ws, jac = mv_sums(b, ops, want_jacobian=True)
    got = ws.sum(1).cpu().numpy()
    jac = jac.cpu().numpy().astype(np.float64)
    x64, J64 = sc["x64"][:S, :V].reshape(B, N), sc["J64"][:S, :V].reshape(B, N, 6)
    if device.type == "cpu":
        J32 = np.ascontiguousarray(sc["J32"][:S, :V]).reshape(B, N, 6)
        assert np.array_equal(jac, J32.astype(np.float64))  # (the same record, the same operations: the same bits)
    else:
        J32 = float32_route(b["aux"], b["args"], b["kw"], ops)
    f = np.tile(b["fixed"].cpu().numpy().astype(np.float64), (S, 1))  # pose s V + v reads image v
    truth, scale = sums_of(J64, x64, f)
    route, _ = sums_of(J32, b["x32"].cpu().numpy(), f)
    err, own = np.abs(got - truth), np.abs(route - truth)
    print(f"{name} S={S} V={V}: sums, worst (kernel error - 2 x float32 route's) / scale = "
          f"{((err - 2 * own) / scale).max():.2e}; kernel error / scale max {(err / scale).max():.2e}, float32 route's "
          f"{(own / scale).max():.2e}")
    assert (err <= 2 * own + FLOOR * scale).all(), np.argwhere(err > 2 * own + FLOOR * scale)
    jscale = np.abs(J64).max(axis=1, keepdims=True)
    jerr, jown = np.abs(jac - J64), np.abs(J32 - J64)
    print(f"{name} S={S} V={V}: jacobian, kernel error / column max {(jerr / jscale).max():.2e}, float32 route's "
          f"{(jown / jscale).max():.2e}")
    assert (jerr <= 2 * jown + FLOOR * jscale).all(), float(((jerr - 2 * jown) / jscale).max())


# ------------------------------------------------------------------------------------------------ step
# lm_cases.check_step_sequences' sequences: (calls of per-start feeds, hyper-parameters, starts)
CLAMP = dict(HYPER, damping_min=0.2, damping_max=1.5)
SEQUENCES = (
    ([[(1, 0.8)], [(2, 0.3)], [(3, 0.6)], [(4, 0.1)]], HYPER, 1),                # first call, accept, reject, accept
    ([[(1, 0.8)], [(2, 0.3)], [(3, 0.6)], [(5, 0.7)], [(6, 0.9)]], CLAMP, 1),    # both clamps
    ([["flat"], [(2, 0.3)]], HYPER, 1),                                          # a failed factorisation, first
    ([[(1, 0.8)], ["flat"]], HYPER, 1),                                          # ... and after a valid pose
    ([[(1, 0.8), (2, 0.3), "flat"], [(2, 0.3), (1, 0.8), (3, 0.2)], [(3, 0.6), (4, 0.1), (4, 0.1)]], HYPER, 3),
)
STEP_N = 1500  # two workgroups' partials
STEP_START = np.array([0.08, -0.06, 0.07, 6.0, 391.0, 5.0], dtype=np.float32)


def view_feed(feed, v):
    """view v of a start's feed: the same closeness on another image pair"""
    if feed == "flat":
        return 99 + 7 * v, 0.5
    return feed[0] + 100 * v, feed[1] * (1.0 + 0.25 * v)


def view_data(feed, v, device):
    """(J, x, f) and the (G, 44) partials of one view; "flat": H = 0 (A is negative semi-definite in every view)"""
    seed, closeness = view_feed(feed, v)
    J, x, f = lm_cases.synthetic_pair(seed, STEP_N, closeness)
    p = lm_cases.partials_of(J, x, f, device)
    if feed == "flat":
        p[:, :21] = 0.0
    return (J, x, f), p


def fresh(S, device, ops, lam0=1.0):
    return (ops.lm_state(S, lam0, device), torch.tensor(np.tile(STEP_START[:3], (S, 1)), device=device),
            torch.tensor(np.tile(STEP_START[3:], (S, 1)), device=device))


def check_step_one_view_is_lm_step(device, ops):
    """V = 1 on fed partials: state, theta and the NCC equal ddrr_lm_step's bit for bit over every sequence."""
    for feeds, hyper, S in SEQUENCES:
        mine, theirs = fresh(S, device, ops), fresh(S, device, ops)
        views = torch.zeros(S, 1, device=device)
        for call in feeds:
            ws = torch.stack([view_data(feed, 0, device)[1] for feed in call]).contiguous()
            ncc_m = ops.mvlm_step(ws, *mine, 1, STEP_N, **hyper, ncc_views=views)
            ncc_t = ops.lm_step(ws, *theirs, STEP_N, **hyper)
            assert torch.equal(ncc_m, ncc_t)
            for m, t in zip(mine, theirs):
                assert torch.equal(m, t), (call, m, t)
            # (ncc_views is of the render just judged: the state's where it was accepted)
            acc = mine[0][:, 36] != 0
            assert torch.equal(views[acc, 0], mine[0][acc, 6].to(torch.float32))


def mv_reference_update(ref, theta, J, x, f, hyper):
    """lm_cases.reference_update with the normal equations of multiview_normal_equations_reference: J (V, N, 6),
    x, f (V, N) of one start -> (the next trial parameters in float64, unrounded; ncc_views (V,))"""
    ncc, A, g, ncc_v = (t.numpy() for t in multiview_normal_equations_reference(
        torch.tensor(J)[None], torch.tensor(x)[None], torch.tensor(f), hyper["ncc_eps"]))
    ncc, A, g = float(ncc[0]), A[0], g[0]
    if not ref["valid"] or ncc > ref["ncc"]:
        ref.update(best=theta.copy(), ncc=ncc, A=A, g=g, valid=True, accepted=True)
        ref["lam"] = max(ref["lam"] * hyper["down"], hyper["damping_min"])
    else:
        ref["accepted"] = False
        ref["lam"] = min(ref["lam"] * hyper["up"], hyper["damping_max"])
    M = ref["A"] + ref["lam"] * np.diag(np.diag(ref["A"])) + 1e-30 * np.eye(6)
    try:
        Lc = np.linalg.cholesky(M)
        delta = np.linalg.solve(Lc.T, np.linalg.solve(Lc, -ref["g"]))
    except np.linalg.LinAlgError:
        delta = np.zeros(6)
        ref["lam"] = min(ref["lam"] * hyper["up"], hyper["damping_max"])
    return ref["best"] + delta, ncc_v[0]


def check_step_sequences(V, device, ops):
    """ddrr_mvlm_step with V > 1 views on fed partials against multiview_normal_equations_reference + the update of
    lm_cases.reference_update, over lm_cases.check_step_sequences' sequences: theta within 2 ulps of float32, the
    damping exactly, accept / reject, the best mean NCC, and ncc_views of every render."""
    traces = []
    for feeds, hyper, S in SEQUENCES:
        state, rot, xyz = fresh(S, device, ops)
        refs = [dict(valid=False, lam=1.0, ncc=0.0) for _ in range(S)]
        views = torch.full((S, V), -2.0, device=device)
        trace = []
        for call in feeds:
            theta = torch.cat([rot, xyz], 1).cpu().numpy().astype(np.float64)
            parts, want = [], []
            for s, feed in enumerate(call):
                data = [view_data(feed, v, device) for v in range(V)]
                parts += [p for _, p in data]
                want.append(None if feed == "flat" else mv_reference_update(
                    refs[s], theta[s], *(np.stack([d[0][k] for d in data]) for k in range(3)), hyper))
            ws = torch.stack(parts).contiguous()  # (S V, G, 44): pose s V + v
            lam_before, valid_before = state[:, 34].cpu().numpy().copy(), state[:, 35].cpu().numpy().copy()
            ncc = ops.mvlm_step(ws, state, rot, xyz, V, STEP_N, **hyper, ncc_views=views)
            got, st, nv = torch.cat([rot, xyz], 1).cpu().numpy(), state.cpu().numpy(), views.cpu().numpy()
            for s, feed in enumerate(call):
                if feed == "flat":  # delta = 0: the next trial is the best itself; lambda: the move, then up
                    assert np.array_equal(got[s], st[s, :6].astype(np.float32)), (got[s], st[s, :6])
                    moved = max(lam_before[s] * hyper["down"], hyper["damping_min"]) if not valid_before[s] or \
                        st[s, 36] else min(lam_before[s] * hyper["up"], hyper["damping_max"])
                    assert st[s, 34] == min(moved * hyper["up"], hyper["damping_max"]), (st[s, 34], moved)
                    if refs[s]["valid"] is False and st[s, 36]:
                        refs[s].update(valid=True, best=theta[s].copy(), ncc=st[s, 6], A=None, g=None)
                    refs[s]["lam"] = st[s, 34]
                    continue
                trial, ncc_v = want[s]
                u = ulps32(got[s], trial)
                assert (u <= 2).all(), (s, feed, got[s], trial, u)
                assert st[s, 34] == refs[s]["lam"], (s, feed, st[s, 34], refs[s]["lam"])  # exactly
                assert bool(st[s, 36]) == refs[s]["accepted"] and st[s, 35] == 1.0
                assert abs(st[s, 6] - refs[s]["ncc"]) <= 1e-12 and float(ncc[s]) == np.float32(st[s, 6])
                assert (ulps32(nv[s], ncc_v) <= 1).all(), (s, nv[s], ncc_v)
            trace.append((st[:, 34].copy(), st[:, 36].copy()))
        traces.append(trace)
    # the outcomes the sequences are there for (the second view is farther from its image than the first: the
    # order of the mean NCC is the order of the closeness)
    d = HYPER["down"]
    assert [bool(a[0]) for _, a in traces[0]] == [True, True, False, True]
    assert [lam[0] for lam, _ in traces[0]] == [d, d * d, d * d * 4.0, d * d * 4.0 * d]
    assert [lam[0] for lam, _ in traces[1]] == [1 / 3, 0.2, 0.8, 1.5, 1.5]
    assert [list(a.astype(bool)) for _, a in traces[4]][1][:2] == [True, False]


# ------------------------------------------------------------------------------------------------ the reference
def check_reference():
    """multiview_normal_equations_reference's A and g against the autograd Gauss-Newton model of the stacked
    residual (z(x_v(theta)) - z(f_v))_v for x linear in theta, in float64; N sum_v (1 - ncc_v) = 1/2 |r|^2 up to
    eps; one view is normal_equations_reference."""
    g = torch.Generator().manual_seed(6)
    V, N, eps = 3, 40, 1e-5
    J = torch.randn(V, N, 6, generator=g, dtype=torch.float64)
    x0 = torch.rand(V, N, generator=g, dtype=torch.float64)
    f = torch.rand(V, N, generator=g, dtype=torch.float64) * torch.tensor([[1.0], [5.0], [0.2]], dtype=torch.float64)

    def z(v):
        return (v - v.mean(-1, keepdim=True)) / (v.var(-1, unbiased=False, keepdim=True) + eps).sqrt()

    def residual(theta):
        return (z(x0 + J @ theta) - z(f)).reshape(-1)

    theta = torch.zeros(6, dtype=torch.float64)
    Jr = torch.autograd.functional.jacobian(residual, theta)
    ncc, A, grad, ncc_v = multiview_normal_equations_reference(J[None], x0[None], f, eps)
    assert ncc.shape == (1,) and A.shape == (1, 6, 6) and grad.shape == (1, 6) and ncc_v.shape == (1, V)
    assert torch.allclose(A[0], Jr.T @ Jr, rtol=1e-10, atol=1e-12)
    assert torch.allclose(grad[0], Jr.T @ residual(theta), rtol=1e-10, atol=1e-12)
    # 1/2 |z(x) - z(f)|^2 = N (rho_x / 2 + rho_f / 2 - ncc) per view, rho = var / (var + eps): N (1 - ncc) up to eps
    rho = sum(v.var(-1, unbiased=False) / (v.var(-1, unbiased=False) + eps) for v in (x0, f)) / 2
    assert abs(float(0.5 * residual(theta).pow(2).sum()) - N * float((rho - ncc_v[0]).sum())) < 1e-9
    assert float((1 - rho).max()) < 1e-2
    assert abs(float(ncc[0]) - float(ncc_v.mean())) <= 1e-15
    n1, A1, g1 = normal_equations_reference(J[1], x0[1], f[1], eps)
    m1, B1, h1, v1 = multiview_normal_equations_reference(J[None, 1:2], x0[None, 1:2], f[1:2], eps)
    assert torch.equal(B1[0], A1) and torch.equal(h1[0], g1) and float(m1[0]) == float(n1) == float(v1[0, 0])
    # two starts: each its own
    n2, A2, g2, v2 = multiview_normal_equations_reference(torch.stack([J, 2 * J]), torch.stack([x0, x0]), f, eps)
    assert torch.equal(A2[0], A[0]) and torch.allclose(A2[1], 4 * A[0], rtol=1e-12) and v2.shape == (2, V)


def check_view_poses():
    """view_poses: pose s V + v is M(theta_s) @ K_v, differentiable, in the parameters' dtype; relative_views:
    E_0^-1 E_v in float64 with the identity first."""
    rot = torch.tensor([[0.1, -0.2, 0.3], [0.0, 0.4, -0.1]], dtype=torch.float64, requires_grad=True)
    xyz = torch.tensor([[1.0, 400.0, -2.0], [3.0, 380.0, 5.0]], dtype=torch.float64)
    K = orbit_views("ZXY")
    assert K.dtype == torch.float64 and K.shape == (3, 4, 4) and torch.equal(K[0], torch.eye(4, dtype=torch.float64))
    E = convert(torch.tensor([[a, 0.0, 0.0] for a in ANGLES], dtype=torch.float64),
                torch.tensor([[0.0, 400.0, 0.0]] * 3, dtype=torch.float64), parameterization="euler_angles",
                convention="ZXY").matrix
    assert torch.allclose(E[0] @ K, E, rtol=0, atol=1e-10)
    poses = view_poses(rot, xyz, K, "ZXY")
    M = convert(rot, xyz, parameterization="euler_angles", convention="ZXY").matrix
    assert len(poses) == 6 and poses.matrix.dtype == torch.float64
    for s in range(2):
        for v in range(3):
            assert torch.allclose(poses.matrix[s * 3 + v], M[s] @ K[v], rtol=0, atol=1e-12)
    poses.matrix[4, 0, 3].backward()
    assert float(rot.grad[1].abs().sum()) > 0 and float(rot.grad[0].abs().sum()) == 0
    assert view_poses(rot.detach().float(), xyz.float(), K).matrix.dtype == torch.float32
    # at the isocentre pose view v is the orbit pose itself
    iso = view_poses(torch.zeros(1, 3, dtype=torch.float64), torch.tensor([[0.0, 400.0, 0.0]], dtype=torch.float64), K)
    assert torch.allclose(iso.matrix, E, rtol=0, atol=1e-10)
    with pytest.raises(ValueError, match="relative_views"):
        relative_views(torch.eye(4))


# ------------------------------------------------------------------------------------------------ conditioning
def _start(device, S=1):
    return [(TRUTH[k] + OFFSET[k]).to(device).repeat(S, 1) for k in (0, 1)]


def mv_scene(device, angles=(0.0, math.pi / 2)):
    """lm_cases.convergence_scene seen from `angles`: the module, the fixed images (V, 1, 48, 48), the views"""
    drr, _ = lm_cases.convergence_scene(device)
    K = orbit_views("ZXY", angles)
    with torch.no_grad():
        fixed = drr(view_poses(TRUTH[0].to(device), TRUTH[1].to(device), K, "ZXY"))
    return drr, fixed.reshape(len(angles), 1, 48, 48).contiguous(), K


def normal_matrix(lm):
    """A (6, 6) of start 0 as the kernels formed it: one step from a fresh state, which accepts (state[7:28])"""
    lm.step()
    st = lm._state[0].cpu().numpy()
    assert st[35] == 1.0 and st[36] == 1.0
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = st[7:28]
    return A + np.triu(A, 1).T


def check_conditioning(device):
    """On the 64^3 -> 48^2 convergence scene at truth + (0.01 rad, 0.5 mm): (A^-1)[4, 4], the variance of the
    translation along view 0's axis, from the kernels' sums is at least 100 x smaller with views (0, pi / 2) than
    with view 0 alone (measured 7.2e2 on the host build; the margin covers float32 record differences)."""
    drr, fixed, K = mv_scene(device)
    at = [(TRUTH[0] + 0.01).to(device), (TRUTH[1] + 0.5).to(device)]
    out = []
    for V in (1, 2):
        reg = Registration(drr, at[0].clone(), at[1].clone(), parameterization="euler_angles", convention="ZXY")
        A = normal_matrix(MultiViewLevenbergMarquardt(reg, fixed[:V], K[:V]))
        out.append((np.linalg.cond(A), np.linalg.inv(A)[4, 4]))
    (c1, v1), (c2, v2) = out
    print(f"view 0 alone: cond(A) {c1:.3g}, (A^-1)[4,4] {v1:.4g}; views (0, pi/2): cond(A) {c2:.3g}, (A^-1)[4,4] "
          f"{v2:.4g}; ratio {v1 / v2:.4g}")
    assert v1 > 0 and v2 > 0 and v1 >= 100.0 * v2, (v1, v2)
    return v1 / v2


# ------------------------------------------------------------------------------------------------ registration
def check_registration(device, ops):
    """lm_cases.convergence_scene, views (0, pi / 2), from OFFSET: lm_cases._reached (mean NCC >= 0.9999 within
    0.01 rad / 0.5 mm) inside 60 steps; commit() writes the best parameters; a step is the four launches."""
    drr, fixed, K = mv_scene(device)
    rot, xyz = _start(device)
    reg = Registration(drr, rot.clone(), xyz.clone(), parameterization="euler_angles", convention="ZXY")
    lm = MultiViewLevenbergMarquardt(reg, fixed, K)
    assert lm.view_ncc.shape == (1, 2) and float(lm.view_ncc.abs().max()) == 0
    steps = None
    with launches(ops) as names:
        for it in range(1, 61):  # the hard cap: a stall fails
            ncc = float(lm.step()[0])
            if it == 1:
                assert names == ["ddrr_mvlm_raygen", "ddrr_siddon_forward_bricks", "ddrr_mvlm_normal_sums",
                                 "ddrr_mvlm_step"], names
                first = ncc
            if _reached(ncc, *lm.best_parameters):
                steps = it
                break
    print(f"two views (0, pi/2): mean NCC {ncc:.6f} after {it} steps; per view {lm.view_ncc.tolist()}")
    assert steps is not None, f"mean NCC {ncc} after 60 steps"
    assert len(names) == 4 * steps and ncc > first and lm.steps_done == steps
    assert not any(n.startswith(("ddrr_lm_", "ddrr_wlm_", "ddrr_pose_raygen")) for n in names)
    trial = reg.rotation.detach().clone()
    lm.commit()
    assert torch.equal(reg.rotation.detach(), lm.best_parameters[0])
    assert torch.equal(reg.translation.detach(), lm.best_parameters[1])
    assert _reached(ncc, reg.rotation.detach(), reg.translation.detach())
    assert float(lm.best_ncc[0]) >= 0.9999 and not torch.equal(trial, reg.rotation.detach()) or bool(lm.accepted[0])
    return steps


def check_multi_starts(device, ops):
    """S = 3 starts, two views.  On the host build each runs as it runs alone, bit for bit (a render is reproducible
    there; on the device the record is summed with float atomics and two runs of ONE start differ).  What holds on
    either, bit for bit and on one record: a start's step does not depend on its neighbours' sums
    (check_sums_bit_for_bit has the same for the sums themselves)."""
    drr, fixed, K = mv_scene(device)
    rots = torch.tensor([[0.08, -0.06, 0.07], [-0.05, 0.04, 0.02], [0.03, 0.0, -0.02]], device=device)
    xyzs = torch.tensor([[6.0, 391.0, 5.0], [-4.0, 405.0, 3.0], [2.0, 398.0, -3.0]], device=device)

    def build(b=slice(0, 3)):
        reg = Registration(drr, rots[b].clone(), xyzs[b].clone(), parameterization="euler_angles", convention="ZXY")
        return reg, MultiViewLevenbergMarquardt(reg, fixed, K, damping=2.0)

    reg, lm = build()
    assert torch.equal(lm.damping, torch.full((3,), 2.0, dtype=torch.float64, device=device))
    J = lm.jacobian()
    assert J.shape == (3, 2, 48 * 48, 6) and bool(torch.isfinite(J).all()) and float(J.abs().max()) > 0
    assert torch.equal(reg.rotation.detach(), rots) and lm.steps_done == 0  # (jacobian() moves nothing)
    history = [lm.step().clone() for _ in range(6)]
    assert history[0].shape == (3,) and not history[0].requires_grad
    assert all((b >= a).all() for a, b in zip(history, history[1:]))  # the best mean NCC never falls
    assert lm.view_ncc.shape == (3, 2) and lm.accepted.shape == (3,) and lm.best_ncc.shape == (3,)
    for s in range(3):
        reg_s, lm_s = build(slice(s, s + 1))
        for _ in range(6):
            last = lm_s.step()
        print(f"start {s} in the batch and alone after six steps: best mean NCC {float(history[-1][s]):.7f} / "
              f"{float(last[0]):.7f}, damping {float(lm.damping[s]):.3g} / {float(lm_s.damping[0]):.3g}")
        if device.type == "cpu":
            assert torch.equal(lm._state[s], lm_s._state[0])
            assert torch.equal(reg.rotation.detach()[s], reg_s.rotation.detach()[0])
            assert torch.equal(reg.translation.detach()[s], reg_s.translation.detach()[0])
            assert torch.equal(lm.view_ncc[s], lm_s.view_ncc[0])
        assert float(last[0]) > float(history[0][s])  # (it moved, and for the better)
    # one record's sums, start 1's replaced by another image pair's: starts 0 and 2 step to the same bits
    args, kw = lm._render()
    ws, _ = ops.mvlm_normal_sums(args.pop("aux"), lm.fixed, **args, **kw)
    other = ws.clone()
    other[2:4] = torch.stack([lm_cases.partials_of(*lm_cases.synthetic_pair(3 + v, 48 * 48, 0.4), device)
                              for v in range(2)])
    outs = []
    for w in (ws, other):
        state, rot, xyz = lm._state.clone(), rots.clone(), xyzs.clone()
        views = torch.zeros(3, 2, device=device)
        ncc = ops.mvlm_step(w.contiguous(), state, rot, xyz, 2, 48 * 48, **HYPER, ncc_views=views)
        outs.append((state, rot, xyz, views, ncc))
    for a, b in zip(*outs):
        assert torch.equal(a[[0, 2]], b[[0, 2]]) and bool(torch.isfinite(b).all())
    assert not torch.equal(outs[0][3][1], outs[1][3][1])


# ------------------------------------------------------------------------------------------------ surface
def check_errors(device, elsewhere):
    """ValueErrors of the constructor name the condition.  `elsewhere`: a device the parameters are not on."""
    drr, fixed, K = mv_scene(device)

    def build(fixed=fixed, views=K, S=1, par="euler_angles", conv="ZXY", rot=None, **kw):
        rot_, xyz_ = _start(device, S)
        reg = Registration(drr, (rot_ if rot is None else rot).clone(), xyz_.clone(), parameterization=par,
                           convention=conv)
        return MultiViewLevenbergMarquardt(reg, fixed, views, **kw)

    lm = build()
    assert (lm.S, lm.V, lm.N) == (1, 2, 48 * 48) and lm.fixed.shape == (2, 48 * 48)
    assert lm._reorient_v.shape == (2, 3, 4) and lm._reorient_v.dtype == torch.float32
    assert build(views=K.float()).V == 2  # (float32 views are taken, to their own tolerance)
    shear, scaled, mirror, bottom, nan = (K.clone() for _ in range(5))
    shear[1, 0, 1] += 0.01
    scaled[1, :3, :3] *= 1.001
    mirror[1, :3, 0] *= -1.0
    bottom[1, 3, 0] = 0.5
    nan[0, 1, 3] = float("nan")
    for kw, what in ((dict(views=K[0]), "V, 4, 4"), (dict(views=K[:, :3]), "V, 4, 4"), (dict(views=K[:0]), "V, 4, 4"),
                     (dict(views=K.long()), "V, 4, 4"), (dict(views=K.numpy() if device.type == "cpu" else None),
                                                         "V, 4, 4"),
                     (dict(views=nan), "finite"), (dict(views=bottom), "bottom row"), (dict(views=shear), "orthonormal"),
                     (dict(views=scaled), "orthonormal"), (dict(views=mirror), "orthonormal"),
                     (dict(fixed=fixed[:1]), "fixed"), (dict(fixed=fixed[:, :, :40]), "fixed"),
                     (dict(fixed=fixed.double()), "fixed"), (dict(fixed=fixed[:, 0]), "fixed"),
                     (dict(fixed=torch.zeros(2, 1, 48, 48, device=elsewhere)), "device"),
                     (dict(S=17), "rendered poses"), (dict(S=0), "rendered poses"),
                     (dict(par="axis_angle", conv=None), "euler_angles"), (dict(rot=_start(device)[0].double()), "float32"),
                     (dict(up=1.0), "damping"), (dict(damping=1e7), "damping"), (dict(eps=-1.0), "eps")):
        with pytest.raises(ValueError, match=what):
            build(**kw)
    with pytest.raises(ValueError):
        build(conv="ZZY")
    with pytest.raises(TypeError):
        build(weight=torch.ones(2, 1, 48, 48, device=device))  # (no pixel weights here)


def check_ops_errors(ops):
    """The ops refuse what the entries would misread, without a launch."""
    S, V, N = 2, 3, 1500
    state = ops.lm_state(S, 1.0, "cpu")
    rot, xyz = torch.zeros(S, 3), torch.zeros(S, 3)
    ws = ops.mvlm_workspace(S, V, N, "cpu")
    assert ws.shape == (S * V, 2, 44) and ws.dtype == torch.float64
    assert ops.mvlm_workspace(0, 2, 100, "cpu").numel() == 0
    Ro = torch.zeros(V, 3, 4)
    with launches(ops) as launched:
        with pytest.raises(ValueError, match="ws"):
            ops.mvlm_step(ws[:, :1].contiguous(), state, rot, xyz, V, N)
        with pytest.raises(ValueError, match="ws"):
            ops.mvlm_step(ws, state, rot, xyz, V - 1, N)
        with pytest.raises(ValueError, match="V >= 1"):
            ops.mvlm_step(ws, state, rot, xyz, 0, N)
        with pytest.raises(ValueError, match="state"):
            ops.mvlm_step(ws, state.float(), rot, xyz, V, N)
        with pytest.raises(ValueError, match="state"):
            ops.mvlm_step(ws, ops.lm_state(S * V, 1.0, "cpu"), rot, xyz, V, N)
        with pytest.raises(ValueError, match="pose parameters"):
            ops.mvlm_step(ws, state, rot.double(), xyz, V, N)
        with pytest.raises(ValueError, match="up > 1"):
            ops.mvlm_step(ws, state, rot, xyz, V, N, down=1.5)
        with pytest.raises(ValueError, match="ncc_views"):
            ops.mvlm_step(ws, state, rot, xyz, V, N, ncc_views=torch.zeros(V, S))
        pose = dict(source=torch.zeros(S * V, 1, 3), Mw=torch.zeros(S * V, 3, 4), Ainv=torch.zeros(3, 4),
                    P=torch.zeros(N, 3), rot=rot, xyz=xyz, axes=(2, 0, 1), reorient_v=Ro)
        aux, x1 = ops.brick_record_buffer(S * V, N, "cpu"), torch.ones(V, N)
        for bad in (torch.ones(N), torch.ones(1, N), torch.ones(S * V, N), torch.ones(V, N + 1), torch.ones(V, 1, N),
                    torch.ones(V, N).double(), None):
            with pytest.raises(ValueError, match="fixed"):
                ops.mvlm_normal_sums(aux, bad, **pose)
        with pytest.raises(ValueError, match="device"):
            ops.mvlm_normal_sums(aux, torch.ones(V, N, device="meta"), **pose)
        with pytest.raises(ValueError, match="reorient_v"):
            ops.mvlm_normal_sums(aux, x1, **dict(pose, reorient_v=Ro[0]))
        with pytest.raises(ValueError, match="reorient_v"):
            ops.mvlm_raygen(rot, xyz, (2, 0, 1), Ro.double(), pose["Ainv"], pose["P"])
        with pytest.raises(ValueError, match="S \\* V"):
            ops.mvlm_normal_sums(aux, x1, **dict(pose, Mw=torch.zeros(S, 3, 4)))
        with pytest.raises(ValueError, match="ws"):
            ops.mvlm_normal_sums(aux, x1, **pose, ws=ops.lm_workspace(S, N, "cpu"))
        with pytest.raises(ValueError, match="pose parameters"):
            ops.mvlm_raygen(rot.double(), xyz, (2, 0, 1), Ro, pose["Ainv"], pose["P"])
        with pytest.raises(ValueError, match="65535"):
            ops.mvlm_raygen(torch.zeros(300, 3), torch.zeros(300, 3), (2, 0, 1), torch.zeros(300, 3, 4), pose["Ainv"],
                            pose["P"])
        with pytest.raises(ValueError, match="empty batch"):
            ops.mvlm_raygen(rot[:0], xyz[:0], (2, 0, 1), Ro, pose["Ainv"], pose["P"], clear=torch.zeros(4))
        out = ops.mvlm_step(ops.mvlm_workspace(0, 2, 100, "cpu"), ops.lm_state(0, 1.0, "cpu"), torch.zeros(0, 3),
                            torch.zeros(0, 3), 2, 100)
        Mw, source, target, img = ops.mvlm_raygen(rot[:0], xyz[:0], (2, 0, 1), Ro, pose["Ainv"], pose["P"])
    assert out.shape == (0,) and Mw.shape == (0, 3, 4) and img.shape == (0, N) and not launched
