"""What tests/test_wmvlm.py (host emulation) and tests/test_gpu_wmvlm.py (MI355X) share: the host build of
csrc/wmvlm_core.h (tests/emu/wmvlm_emu.cpp), the per-view detectors and weights, the yardsticks of the weighted
multi-view Levenberg-Marquardt kernels (include/diffdrr_wmvlm_hip.h) and the checks, written once as
``check_*(..., device, ops)``.

The scenes (lm_cases.SUM_CASES), the gate of the sums (|kernel - truth| <= 2 |float32 route - truth| + FLOOR x the
Cauchy-Schwarz scale of the sum, FLOOR = 1e-6), the step's measure (``ulps32`` <= 2) and the convergence target are
tests/lm_cases.py's; the weight patterns, ``poison`` and the weighted yardsticks of the sums tests/wlm_cases.py's; the
views, the starts, the (S, V) batches and the step sequences tests/mvlm_cases.py's; the pose error ``_q``
tests/wncc_cases.py's.  A rendered pose is ``b = s * V + v``: start ``s`` is row ``s`` of the scene's three parameter
rows, view ``v`` is orbit angle ``ANGLES[v]`` with detector ``v`` of :func:`detectors` (view 0 the module's own, view 1
another source-detector distance, pitch and principal point, view 2 another distance) and row ``v`` of the weights."""
import contextlib
import copy
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import lm_cases
import mvlm_cases
import wlm_cases
from conftest import ROOT
from diffdrr_amd import (
    Detector, MultiViewLevenbergMarquardt, Registration, WeightedMultiViewLevenbergMarquardt, _lib,
)
from diffdrr_amd.registration import (
    multiview_normal_equations_reference, view_poses, weighted_multiview_normal_equations_reference,
    weighted_normal_equations_reference,
)
from lm_cases import FLOOR, HYPER, OFFSET, TRUTH, ulps32
from mvlm_cases import SEQUENCES, STEP_N, SV, SV_IDS, fresh, view_feed  # noqa: F401  (SV, SV_IDS: the test files')
from wlm_cases import poison, wsums_of
from wncc_cases import _q

EMU_SRC = os.path.join(ROOT, "tests", "emu", "wmvlm_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "_build", "libwmvlm_emu.so")
GROUP = _lib.WMVLM_GROUP_RAYS
SMALL = ("6_rays", "780_rays_zxy", "780_rays_zyx_stop")  # the scenes with a float64 route
NAMES = SMALL + ("4087_rays_four_workgroups", "1025_rays")  # ... and the ones for bit-for-bit checks only


@functools.lru_cache(maxsize=None)
def emu_library():
    """The host build of the three entries (tests/emu/wmvlm_emu.cpp), bound through the product's own binding."""
    csrc = os.path.join(ROOT, "diffdrr_amd", "csrc")
    deps = [EMU_SRC, lm_cases.EMU_LOOPS]
    deps += [os.path.join(ROOT, "include", f) for f in ("diffdrr_wmvlm_hip.h", "diffdrr_mvlm_hip.h",
                                                        "diffdrr_wlm_hip.h", "diffdrr_lm_hip.h")]
    deps += [os.path.join(csrc, f) for f in ("wmvlm_core.h", "mvlm_core.h", "wlm_core.h", "lm_core.h", "siddon_core.h",
                                             "raygen_core.h", "record_layout.h", "ddrr_common.h")]
    if not (os.path.exists(EMU_SO) and all(os.path.getmtime(d) <= os.path.getmtime(EMU_SO) for d in deps)):
        os.makedirs(os.path.dirname(EMU_SO), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-mfma", "-ffp-contract=off",
                        "-Wno-unknown-pragmas", EMU_SRC, "-o", EMU_SO], check=True)
    return _lib.wmvlm_library(EMU_SO)


def route_wmvlm_to_emulation(monkeypatch, ops):
    """The launcher patch of the host tests: ops' weighted multi-view launches go to the host build."""
    lib = emu_library()
    monkeypatch.setattr(ops, "_launch_wmvlm", lambda name, device, *a: lib.call(name, *a, None))
    monkeypatch.setattr(ops, "_query_wmvlm", lambda name, *a: lib.query(name, *a))


@contextlib.contextmanager
def launches(ops):
    """the names of the C-ABI entries launched inside the block: the main library's and the four LM libraries'"""
    keys = ("_launch", "_launch_lm", "_launch_wlm", "_launch_mvlm", "_launch_wmvlm")
    names, real = [], {k: getattr(ops, k) for k in keys}
    for k, fn in real.items():
        setattr(ops, k, lambda name, device, *a, _fn=fn: (names.append(name), _fn(name, device, *a))[1])
    try:
        yield names
    finally:
        for k, fn in real.items():
            setattr(ops, k, fn)


# ------------------------------------------------------------------------------------------------ detectors, scenes
def detectors(drr):
    """The detector of view 0 (the module's own), of view 1 (sdd x 1.15, delx x 0.9, dely x 1.1, principal point
    (3, -2)) and of view 2 (sdd x 0.9), on the module's device"""
    d = drr.detector

    def make(sdd, delx, dely, x0, y0):
        return Detector(sdd, d.height, d.width, delx, dely, x0, y0, d._reorient.detach().cpu().clone(),
                        reverse_x_axis=d.reverse_x_axis).to(drr.density.device)

    return (d, make(d.sdd * 1.15, d.delx * 0.9, d.dely * 1.1, 3.0, -2.0), make(d.sdd * 0.9, d.delx, d.dely, -d.x0, -d.y0))


def with_detector(drr, det):
    """a copy of the module that renders with `det`"""
    other = copy.deepcopy(drr)
    other.detector = copy.deepcopy(det).to(drr.density.device)
    return other


def points_of(det):
    return det.calibration(det.full_target())[0].detach().to(torch.float32).contiguous()


_scenes = {}


def scene(name, device, ops):
    """mvlm_cases.scene (module, three starts, three views, the fixed images with the module's detector) and, for the
    per-view detectors, their calibrated points P3 (3, N, 3) and the fixed images fixed3 (3, N) they see from the
    isocentre pose.  Computed once per case and device, never modified."""
    key = (name, str(device))
    if key not in _scenes:
        base = mvlm_cases.scene(name, device, ops)
        drr, K, conv = base["drr"], base["K"], base["conv"]
        dets = detectors(drr)
        P3 = torch.stack([points_of(d) for d in dets]).contiguous()
        assert torch.equal(P3[0], drr._calibrated_points()) and not torch.equal(P3[1], P3[0])
        iso = (torch.zeros(1, 3, device=device), torch.tensor([[0.0, 400.0, 0.0]], device=device))
        with torch.no_grad():
            fixed3 = torch.cat([with_detector(drr, dets[v])(view_poses(*iso, K[v:v + 1], conv)).reshape(1, -1)
                                for v in range(3)]).contiguous()
        assert float(fixed3.abs().amax(1).min()) > 0  # (every view sees the volume)
        assert torch.equal(fixed3[0], base["fixed"][0]) or device.type != "cpu"
        H, W = lm_cases.SUM_CASES[name][0]
        _scenes[key] = dict(base=base, drr=drr, conv=conv, K=K, Ro=base["Ro"], rot=base["rot"], xyz=base["xyz"],
                            N=base["N"], H=H, W=W, dets=dets, P3=P3, P1=drr._calibrated_points(),
                            fixed1=base["fixed"], fixed3=fixed3)
    return _scenes[key]


def render(sc, S, V, per_view, ops, clear=True, rot=None, xyz=None):
    """The first two launches of a step for the first S starts seen from the first V views, every view on its own
    detector (`per_view`: P (V, N, 3)) or all on the module's (P (N, 3)): everything ddrr_wmvlm_normal_sums reads."""
    from diffdrr_amd.pose import _AXIS

    drr, conv = sc["drr"], sc["conv"]
    det = drr.detector
    rot = sc["rot"][:S].contiguous() if rot is None else rot
    xyz = sc["xyz"][:S].contiguous() if xyz is None else xyz
    Ro = sc["Ro"][:V].contiguous()
    P = sc["P3"][:V].contiguous() if per_view else sc["P1"]
    Ainv = drr._affine_inverse[0, :3, :] if drr._affine_inverse.dim() == 3 else drr._affine_inverse[:3, :]
    cfg = drr.renderer._cfg(False, det=(det.height, det.width))
    axes = tuple(_AXIS[c] for c in conv)
    B, N = S * V, sc["N"]
    aux = ops.brick_record_buffer(B, N, rot.device)
    launch_ws = ops.launch_workspace(drr.density.shape, drr.density.device)
    if clear:
        Mw, source, target, img = ops.wmvlm_raygen(rot, xyz, axes, Ro, Ainv, P, clear=aux, clear_launch_ws=launch_ws)
    else:  # (the clears by torch: the record the check of the clears compares with)
        aux.zero_()
        launch_ws.zero_()
        Mw, source, target, img = ops.wmvlm_raygen(rot, xyz, axes, Ro, Ainv, P)
    ops.siddon_forward_bricks(drr.density, source, target, img, cfg["det"], voxel_shift=cfg["voxel_shift"],
                              eps=cfg["eps"], want_aux=True, storage="f32", want_image=False, aux=aux,
                              launch_ws=launch_ws, cleared=True)
    x32 = img * ops.record_planes(aux, B, N)[0]
    args = dict(source=source, Mw=Mw, Ainv=Ainv, P=P, rot=rot, xyz=xyz, axes=axes, reorient_v=Ro)
    return dict(S=S, V=V, N=N, aux=aux, args=args, x32=x32, rays=(target, img), per_view=per_view,
                kw=dict(eps=cfg["eps"], with_img_path=not cfg["stop_gradients"]),
                fixed=(sc["fixed3"] if per_view else sc["fixed1"])[:V].contiguous())


def points(b, v):
    """the detector points view v of a batch reads"""
    P = b["args"]["P"]
    return P[v].contiguous() if P.dim() == 3 else P


def wmv_sums(b, w, ops, fixed=None, **more):
    return ops.wmvlm_normal_sums(b["aux"], b["fixed"] if fixed is None else fixed, w, **b["args"], **b["kw"], **more)


# ------------------------------------------------------------------------------------------------ weights
PATTERNS = ("ones", "disc", "smooth", "half", "workgroup 1 empty", "view 0 empty", "last view empty",
            "all views empty")


def weights(pattern, V, H, W, per_view, device):
    """((V | 1), N) float32 weights; None where the pattern does not apply.  The first five are wlm_cases.weights' with
    a view in the place of a pose; `view 0 empty`, `last view empty`: per-view smooth weights with that row at 0 (a
    shared weight cannot empty one view); `all views empty`: zeros."""
    if pattern in wlm_cases.PATTERNS:
        return wlm_cases.weights(pattern, V, H, W, per_view, device)
    if pattern == "all views empty":
        return torch.zeros(V if per_view else 1, H * W, device=device)
    if not per_view:
        return None
    w = wlm_cases.weights("smooth", V, H, W, True, torch.device("cpu")).clone()
    w[0 if pattern == "view 0 empty" else -1] = 0.0
    return w.to(device).contiguous()


def all_weights(V, H, W, device, patterns=PATTERNS):
    out = []
    for pattern in patterns:
        for per_view in (False, True):
            w = weights(pattern, V, H, W, per_view, device)
            if w is not None:
                out.append((f"{pattern} {'per view' if per_view else 'shared'}", w))
    return out


def row(w, v):
    """the (1, N) weight view v reads"""
    return w[v:v + 1] if w.shape[0] > 1 else w


# ------------------------------------------------------------------------------------------------ ray generation
def check_raygen(name, S, V, device, ops):
    """Mw, source, target and img of pose (s, v) equal, bit for bit, what ops.pose_raygen_forward(rot_s, xyz_s, axes,
    Ro_v, Ainv, P_v) writes; with one detector, what ops.mvlm_raygen writes; with per-view detectors view 1's targets
    are not those of P_0; the clears leave `clear_floats` floats and the first 16 bytes of the launch workspace zero
    and nothing beyond; the record of the render behind the clears is the record behind torch's zero-fill."""
    sc = scene(name, device, ops)
    for per_view in (False, True):
        b = render(sc, S, V, per_view, ops)
        a, (target, img) = b["args"], b["rays"]
        N = b["N"]
        assert a["Mw"].shape == (S * V, 3, 4) and a["source"].shape == (S * V, 1, 3)
        assert target.shape == (S * V, N, 3) and img.shape == (S * V, N)
        for s in range(S):
            for v in range(V):
                Mw, source, tgt, im = ops.pose_raygen_forward(a["rot"][s:s + 1], a["xyz"][s:s + 1], a["axes"],
                                                              a["reorient_v"][v].contiguous(), a["Ainv"], points(b, v))
                p = s * V + v
                assert torch.equal(a["Mw"][p], Mw[0]) and torch.equal(a["source"][p], source[0]), (s, v)
                assert torch.equal(target[p], tgt[0]) and torch.equal(img[p], im[0]), (s, v)
                if per_view and v == 1:  # (P_1 is read, not P_0)
                    other = ops.pose_raygen_forward(a["rot"][s:s + 1], a["xyz"][s:s + 1], a["axes"],
                                                    a["reorient_v"][v].contiguous(), a["Ainv"], sc["P1"])[2]
                    assert not torch.equal(target[p], other[0])
        if not per_view:
            for mine, theirs in zip((a["Mw"], a["source"], target, img),
                                    ops.mvlm_raygen(a["rot"], a["xyz"], a["axes"], a["reorient_v"], a["Ainv"], a["P"])):
                assert torch.equal(mine, theirs)
        # the clears: 1003 floats (three quads' worth of tail) of 1024, 16 bytes of 32
        junk = torch.full((1024,), 7.0, device=device)
        counter = torch.full((8,), 5, dtype=torch.int32, device=device)
        ops.wmvlm_raygen(a["rot"], a["xyz"], a["axes"], a["reorient_v"], a["Ainv"], a["P"], clear=junk[:1003],
                         clear_launch_ws=counter)
        assert not bool(junk[:1003].any()) and bool((junk[1003:] == 7.0).all())
        assert counter.tolist() == [0, 0, 0, 0, 5, 5, 5, 5]
        if device.type == "cpu":  # (a render is reproducible on the host build alone)
            assert torch.equal(render(sc, S, V, per_view, ops, clear=False)["aux"], b["aux"])
        else:
            planes = ops.record_planes(b["aux"], S * V, N)
            other = ops.record_planes(render(sc, S, V, per_view, ops, clear=False)["aux"], S * V, N)
            assert torch.allclose(planes, other, rtol=1e-4, atol=1e-4 * float(other.abs().max()))


# ------------------------------------------------------------------------------------------------ sums
def one_view_sums(b, w, v, ops, P=None, fixed=None):
    """ops.wlm_normal_sums on the whole batch's record with view v's reorient, detector points, image and weight and
    the theta rows repeated: its rows v::V are what the new entry is defined by"""
    a, V = b["args"], b["V"]
    return ops.wlm_normal_sums(
        b["aux"], (b["fixed"] if fixed is None else fixed)[v:v + 1], row(w, v).contiguous(), source=a["source"],
        Mw=a["Mw"], Ainv=a["Ainv"], P=points(b, v) if P is None else P, rot=a["rot"].repeat_interleave(V, 0),
        xyz=a["xyz"].repeat_interleave(V, 0), axes=a["axes"], reorient34=a["reorient_v"][v].contiguous(), **b["kw"],
        want_jacobian=True)


def check_sums_bit_for_bit(name, S, V, device, ops):
    """On ONE record per detector setting: under every weight pattern, shared and per view, and with one detector and
    a detector per view, the partials and jac of pose (s, v) equal ddrr_wlm_normal_sums' with Ro_v, P_v, view v's image
    and weight bit for bit, and not another view's (nor, per-view detectors, the rows P_0 gives); a second call gives
    the same bits; 4 w and w / 4 give exactly 4 x and 1/4 x; column 44 holds the sums of the weights (the ray counts
    under w == 1); start 1 somewhere else leaves the other starts' rows as they are; with w == 1 and one detector the
    44 sums are ddrr_mvlm_normal_sums' (asserted on the host build, printed on the device)."""
    sc = scene(name, device, ops)
    N, G = sc["N"], -(-sc["N"] // GROUP)
    counts = torch.tensor([min(GROUP, N - g * GROUP) for g in range(G)], dtype=torch.float64, device=device)
    for per_view in (False, True):
        b = render(sc, S, V, per_view, ops)
        a = b["args"]
        for label, w in all_weights(V, sc["H"], sc["W"], device):
            ws, jac = wmv_sums(b, w, ops, want_jacobian=True)
            assert ws.shape == (S * V, G, _lib.WMVLM_SUMS) and jac.shape == (S * V, N, 6), label
            assert ws.dtype == torch.float64 and bool(torch.isfinite(ws).all()), label
            empty = not bool(w.any())
            for v in range(V):
                ws_v, jac_v = one_view_sums(b, w, v, ops)
                assert torch.equal(ws_v[v::V], ws[v::V]), (label, v, float((ws_v[v::V] - ws[v::V]).abs().max()))
                assert torch.equal(jac_v[v::V], jac[v::V]), (label, v)
                if V > 1:  # (another view's rows differ: a swapped b / V and b % V cannot pass)
                    o = (v + 1) % V
                    assert not torch.equal(jac_v[o::V], jac[o::V]), (label, v)
                    assert empty or not torch.equal(ws_v[o::V], ws[o::V]), (label, v)
                if per_view and v == 1:  # (P_1 is read, not P_0)
                    ws_0, jac_0 = one_view_sums(b, w, v, ops, P=sc["P1"])
                    assert not torch.equal(jac_0[v::V], jac[v::V]), label
                    assert not bool(row(w, v).any()) or not torch.equal(ws_0[v::V], ws[v::V]), label
                # column 44: the sum of the view's weights over the workgroup's rays; ray counts under w == 1
                wv = row(w, v).double().reshape(-1)
                want = torch.stack([wv[g * GROUP:(g + 1) * GROUP].sum() for g in range(G)])
                assert torch.allclose(ws[v::V, :, 44], want.expand(S, -1), rtol=1e-12, atol=0), (label, v)
                if label.startswith("ones"):
                    assert torch.equal(ws[v::V, :, 44], counts.expand(S, -1)), label
            again, _ = wmv_sums(b, w, ops)
            assert torch.equal(again, ws), (label, "second call")
            for c in (4.0, 0.25):
                scaled, _ = wmv_sums(b, (c * w).contiguous(), ops)
                assert torch.equal(scaled, c * ws), (label, c)
            if label.startswith("workgroup 1 empty"):
                assert not bool(ws[:, 1].any())
            if label.startswith("ones") and not per_view:
                theirs, jac_t = ops.mvlm_normal_sums(b["aux"], b["fixed"], **a, **b["kw"], want_jacobian=True)
                same = torch.equal(ws[..., :44], theirs) and torch.equal(jac, jac_t)
                print(f"{name} S={S} V={V}: with w == 1 and one detector the 44 sums and jac equal those of "
                      f"ddrr_mvlm_normal_sums bit for bit: {same}")
                assert same or device.type != "cpu"
        if S > 1:  # start 1 somewhere else, the record as it is: the other starts' rows keep their bits
            w = weights("smooth", V, sc["H"], sc["W"], True, device)
            ws, jac = wmv_sums(b, w, ops, want_jacobian=True)
            moved = dict(b, args=dict(a, rot=a["rot"].clone(), xyz=a["xyz"].clone()))
            moved["args"]["rot"][1] += 0.05
            moved["args"]["xyz"][1] -= 3.0
            ws_m, jac_m = wmv_sums(moved, w, ops, want_jacobian=True)
            keep = torch.tensor([p // V != 1 for p in range(S * V)], device=device)
            assert torch.equal(ws_m[keep], ws[keep]) and torch.equal(jac_m[keep], jac[keep])
            assert not torch.equal(jac_m[~keep], jac[~keep])


def step_of(b, ws, ops, lam0=1.0):
    """One ddrr_wmvlm_step from a fresh state on copies of the batch's parameters
    -> (ncc, state, rot, xyz, ncc_views, sw_views)"""
    S, V = b["S"], b["V"]
    dev = ws.device
    state = ops.lm_state(S, lam0, dev)
    rot, xyz = b["args"]["rot"].clone(), b["args"]["xyz"].clone()
    nv, sw = torch.full((S, V), -2.0, device=dev), torch.full((S, V), -2.0, dtype=torch.float64, device=dev)
    ncc = ops.wmvlm_step(ws, state, rot, xyz, V, b["N"], **HYPER, ncc_views=nv, sw_views=sw)
    return ncc, state, rot, xyz, nv, sw


def check_masked_pixels_are_not_read(name, S, V, device, ops):
    """NaN and +-Inf in the fixed images under w == 0 change no bit of the sums, the state, the parameters, ncc_views
    or sw_views, and all of them are finite."""
    sc = scene(name, device, ops)
    done = 0
    for per_view in (False, True):
        b = render(sc, S, V, per_view, ops)
        for label, w in all_weights(V, sc["H"], sc["W"], device, ("disc", "half", "workgroup 1 empty", "view 0 empty",
                                                                  "last view empty", "all views empty")):
            if not bool((w == 0).any()):
                continue
            dirty = poison(b["fixed"], w)
            assert not bool(torch.isfinite(dirty).all())
            runs = []
            for fixed in (b["fixed"], dirty):
                ws, _ = wmv_sums(b, w, ops, fixed=fixed)
                runs.append((ws, *step_of(b, ws, ops)))
            for k, (clean, other) in enumerate(zip(*runs)):
                assert torch.equal(clean, other), (name, label, k)
                assert bool(torch.isfinite(other).all()), (name, label, k)
            done += 1
    assert done


# ------------------------------------------------------------------------------------------------ float64
def float64_pairs(sc):
    """x (3, 3, N) and J (3, 3, N, 6) of the scene's nine (start, view) pairs with view v on detector v, from float64
    copies of the module with detector = det_v rendered at view_poses(...): mvlm_cases.float64_pairs per view."""
    xs, Js = [], []
    for v in range(3):
        x, J = mvlm_cases.float64_pairs(with_detector(sc["drr"], sc["dets"][v]), sc["rot"], sc["xyz"], sc["K"][v:v + 1],
                                        sc["conv"])
        xs.append(x[:, 0])
        Js.append(J[:, 0])
    return np.stack(xs, axis=1), np.stack(Js, axis=1)


def float32_route(b, ops):
    """J (S V, N, 6) from one-hot calls of the existing float32 entry, ddrr_siddon_backward_pose_euler, once per view
    on the whole batch with reorient34 = Ro_v, P_v and the theta rows repeated; pose b takes the call of view b % V."""
    a, V, S, N = b["args"], b["V"], b["S"], b["N"]
    one = dict(source=a["source"], Mw=a["Mw"], Ainv=a["Ainv"], axes=a["axes"], rot=a["rot"].repeat_interleave(V, 0),
               xyz=a["xyz"].repeat_interleave(V, 0))
    J = torch.zeros(S * V, N, 6, dtype=torch.float32)
    hot = torch.zeros(S * V, N, dtype=torch.float32, device=a["rot"].device)
    for v in range(V):
        for n in range(N):
            hot[:, n] = 1.0
            g_r, g_t = ops.siddon_backward_pose_euler(b["aux"], hot, **one, P=points(b, v),
                                                      reorient34=a["reorient_v"][v].contiguous(), **b["kw"])
            hot[:, n] = 0.0
            J[v::V, n, :3], J[v::V, n, 3:] = g_r.cpu()[v::V], g_t.cpu()[v::V]
    return J.numpy()


def yardsticks(sc, device, ops):
    """x64 (3, 3, N), J64 (3, 3, N, 6) of the scene's nine pairs with a detector per view (once per scene and device)
    and, on the host build where a ray's record does not depend on its batch, J32 of the same from the nine pairs'
    record."""
    if "J64" not in sc:
        sc["x64"], sc["J64"] = float64_pairs(sc)
        if device.type == "cpu":
            sc["J32"] = float32_route(render(sc, 3, 3, True, ops), ops).reshape(3, 3, sc["N"], 6)
    return sc


def check_sums_against_float64(name, S, V, device, ops):
    """The 45 weighted sums and the per-ray Jacobian of every pose, a detector per view, against the float64 route
    (float64 copies of the module with detector = det_v at view_poses(...)), under lm_cases' gate with the float32
    route (one-hot ddrr_siddon_backward_pose_euler with Ro_v and P_v) on the same record and the weights in both
    yardsticks; with one detector for all views against mvlm_cases' yardsticks of the same scene."""
    sc = yardsticks(scene(name, device, ops), device, ops)
    base = mvlm_cases.yardsticks(sc["base"], device, ops)
    N, B = sc["N"], S * V
    for per_view, ys in ((True, sc), (False, base)):
        b = render(sc, S, V, per_view, ops)
        x64, J64 = ys["x64"][:S, :V].reshape(B, N), ys["J64"][:S, :V].reshape(B, N, 6)
        J32 = np.ascontiguousarray(ys["J32"][:S, :V]).reshape(B, N, 6) if device.type == "cpu" else float32_route(b, ops)
        f = np.tile(b["fixed"].cpu().numpy().astype(np.float64), (S, 1))  # pose s V + v reads image v
        x32 = b["x32"].cpu().numpy()
        for label, w in all_weights(V, sc["H"], sc["W"], device):
            ws, jac = wmv_sums(b, w, ops, want_jacobian=True)
            got = ws.sum(1).cpu().numpy()
            wn = np.tile(np.broadcast_to(w.cpu().numpy().astype(np.float64), (V, N)), (S, 1))
            truth, scale = wsums_of(J64, x64, f, wn)
            route, _ = wsums_of(J32, x32, f, wn)
            err, own = np.abs(got - truth), np.abs(route - truth)
            safe = np.where(scale > 0, scale, 1.0)
            print(f"{name} S={S} V={V} {'detector per view' if per_view else 'one detector'}, {label}: sums, worst "
                  f"(kernel error - 2 x float32 route's) / scale = {((err - 2 * own) / safe).max():.2e}; kernel error / "
                  f"scale max {(err / safe).max():.2e}, float32 route's {(own / safe).max():.2e}")
            assert np.isfinite(got).all()
            assert (err <= 2 * own + FLOOR * scale).all(), (label, np.argwhere(err > 2 * own + FLOOR * scale))
        jac = jac.cpu().numpy().astype(np.float64)  # (weights do not enter j_n: the last pattern's serves)
        if device.type == "cpu":
            assert np.array_equal(jac, J32.astype(np.float64))  # (the same record, the same operations)
        jscale = np.abs(J64).max(axis=1, keepdims=True)
        jerr, jown = np.abs(jac - J64), np.abs(J32 - J64)
        print(f"{name} S={S} V={V} {'detector per view' if per_view else 'one detector'}: jacobian, kernel error / "
              f"column max {(jerr / jscale).max():.2e}, float32 route's {(jown / jscale).max():.2e}")
        assert (jerr <= 2 * jown + FLOOR * jscale).all(), float(((jerr - 2 * jown) / jscale).max())


# ------------------------------------------------------------------------------------------------ the reference
def check_reference():
    """weighted_multiview_normal_equations_reference's A and g against autograd of the stacked residual
    (sqrt(w_v) (z_w(x_v(theta)) - z_w(f_v)))_v for an x linear in theta, zero weights (with NaN under them) included;
    sum_v Sw_v (1 - ncc_v) = 1/2 |r|^2 up to eps; the judged ncc is the Sw-weighted mean; at w == 1 A and g are
    multiview_normal_equations_reference's to 1e-12; one view is weighted_normal_equations_reference; an empty view
    is skipped, a single non-empty view's ncc is taken as it is, no view left gives zeros."""
    g = torch.Generator().manual_seed(8)
    V, N, eps = 3, 40, 1e-5
    J = torch.randn(V, N, 6, generator=g, dtype=torch.float64)
    x0 = torch.rand(V, N, generator=g, dtype=torch.float64)
    f = torch.rand(V, N, generator=g, dtype=torch.float64) * torch.tensor([[1.0], [5.0], [0.2]], dtype=torch.float64)
    w = 0.25 + 1.5 * torch.rand(V, N, generator=g, dtype=torch.float64)
    w[torch.rand(V, N, generator=g) < 0.3] = 0.0
    w[1] *= 3.0  # (a view that counts three times)
    on = w != 0
    assert int((~on).sum(1).min()) >= 3

    def z(v, wv):
        mu = (wv * v).sum() / wv.sum()
        return (v - mu) / ((wv * (v - mu) ** 2).sum() / wv.sum() + eps).sqrt()

    def residual(theta):
        return torch.cat([w[v][on[v]].sqrt() * (z(x0[v][on[v]] + J[v][on[v]] @ theta, w[v][on[v]])
                                                - z(f[v][on[v]], w[v][on[v]])) for v in range(V)])

    theta = torch.zeros(6, dtype=torch.float64)
    Jr = torch.autograd.functional.jacobian(residual, theta)
    nan = torch.full_like(x0, float("nan"))
    Jn, xn, fn = torch.where(on[..., None], J, nan[..., None]), torch.where(on, x0, nan), torch.where(on, f, nan)
    ncc, A, grad, ncc_v, sw_v = weighted_multiview_normal_equations_reference(Jn[None], xn[None], fn, w, eps)
    assert ncc.shape == (1,) and A.shape == (1, 6, 6) and grad.shape == (1, 6)
    assert ncc_v.shape == (1, V) and sw_v.shape == (1, V) and ncc.dtype == A.dtype == sw_v.dtype == torch.float64
    assert torch.allclose(A[0], Jr.T @ Jr, rtol=1e-10, atol=1e-12)
    assert torch.allclose(grad[0], Jr.T @ residual(theta), rtol=1e-10, atol=1e-12)
    assert torch.equal(sw_v[0], w.sum(1))
    # 1/2 |r_v|^2 = Sw_v (rho_x / 2 + rho_f / 2 - ncc_v), rho = var_w / (var_w + eps): Sw_v (1 - ncc_v) up to eps

    def rho(t):
        var = torch.stack([(w[v][on[v]] * (t[v][on[v]] - (w[v][on[v]] * t[v][on[v]]).sum() / w[v].sum()) ** 2).sum()
                           / w[v].sum() for v in range(V)])
        return var / (var + eps)

    rho = (rho(x0) + rho(f)) / 2
    half = float(0.5 * residual(theta).pow(2).sum())
    assert abs(half - float((sw_v[0] * (rho - ncc_v[0])).sum())) < 1e-9
    assert float((1 - rho).max()) < 1e-2
    assert abs(half - float((sw_v[0] * (1 - ncc_v[0])).sum())) <= float((sw_v[0] * (1 - rho)).sum()) + 1e-9
    assert abs(float(ncc[0]) - float((sw_v[0] * ncc_v[0]).sum() / sw_v[0].sum())) <= 1e-15
    assert abs(float(ncc[0]) - float(ncc_v.mean())) > 1e-6  # (not the plain mean)
    # w == 1: the unweighted multi-view reference's A and g; its mean ncc (every Sw_v is N)
    m0, A0, g0, v0 = multiview_normal_equations_reference(J[None], x0[None], f, eps)
    m1, A1, g1, v1, s1 = weighted_multiview_normal_equations_reference(J[None], x0[None], f, torch.ones(1, N), eps)
    assert float((A1 - A0).abs().max()) <= 1e-12 * float(A0.abs().max())
    assert float((g1 - g0).abs().max()) <= 1e-12 * float(g0.abs().max())
    assert abs(float(m1 - m0)) <= 1e-14 and float((v1 - v0).abs().max()) <= 1e-14 and bool((s1 == N).all())
    # one view: weighted_normal_equations_reference itself
    n1, B1, h1, S1 = weighted_normal_equations_reference(Jn[1], xn[1], fn[1], w[1], eps)
    m, B, h, nv, sv = weighted_multiview_normal_equations_reference(Jn[None, 1:2], xn[None, 1:2], fn[1:2], w[1:2], eps)
    assert torch.equal(B[0], B1) and torch.equal(h[0], h1) and float(m[0]) == float(n1) == float(nv[0, 0])
    assert float(sv[0, 0]) == float(S1)
    # an empty view is skipped: the call without it; a single view left: its ncc itself; none left: zeros
    for k in range(V):
        we = w.clone()
        we[k] = 0.0
        rest = [v for v in range(V) if v != k]
        a = weighted_multiview_normal_equations_reference(Jn[None], xn[None], fn, we, eps)
        c = weighted_multiview_normal_equations_reference(Jn[None, rest], xn[None, rest], fn[rest], w[rest], eps)
        assert all(torch.equal(p, q) for p, q in zip(a[:3], c[:3]))
        assert torch.equal(a[3][:, rest], c[3]) and float(a[3][0, k]) == 0 and float(a[4][0, k]) == 0
    we = w.clone()
    we[[0, 2]] = 0.0
    a = weighted_multiview_normal_equations_reference(Jn[None], xn[None], fn, we, eps)
    assert float(a[0][0]) == float(n1) and torch.equal(a[1][0], B1)
    a = weighted_multiview_normal_equations_reference(Jn[None], xn[None], fn, torch.zeros(1, N), eps)
    assert all(not bool(t.any()) for t in a)
    # two starts: each its own; all weights x 4: A and g x 4, ncc as it was
    b2 = weighted_multiview_normal_equations_reference(torch.stack([J, 2 * J]), torch.stack([x0, x0]), f, w, eps)
    assert torch.equal(b2[1][0], A[0]) and torch.allclose(b2[1][1], 4 * A[0], rtol=1e-12) and b2[3].shape == (2, V)
    a4 = weighted_multiview_normal_equations_reference(J[None], x0[None], f, 4 * w, eps)
    assert torch.allclose(a4[1], 4 * A, rtol=1e-12) and abs(float(a4[0] - ncc)) <= 1e-15


# ------------------------------------------------------------------------------------------------ step
EMPTY_SEQUENCES = (
    ([["empty"], ["empty"]], HYPER, 1),                 # nothing left of a start: as a first call, and again
    ([[(1, 0.8)], ["empty"], [(2, 0.3)]], HYPER, 1),    # ... and after a valid render
    ([[(1, 0.8), "empty", (2, 0.3)], ["empty", (1, 0.8), (3, 0.2)]], HYPER, 3),
)
W_SEQUENCES = SEQUENCES + EMPTY_SEQUENCES


def view_data(feed, v, device, scale=1.0, ones=False):
    """(J, x, f, w) and the (G, 45) weighted partials of one view of a start's feed: mvlm_cases.view_feed's image
    pair under wlm_cases.synthetic_weights of its seed (times `scale`; `ones`: w == 1).  "flat": H = 0 (A is negative
    semi-definite in every view); "empty": w == 0."""
    seed, closeness = view_feed((7, 0.5) if feed == "empty" else feed, v)
    J, x, f = lm_cases.synthetic_pair(seed, STEP_N, closeness)
    w = np.ones(STEP_N) if ones else np.zeros(STEP_N) if feed == "empty" else scale * wlm_cases.synthetic_weights(
        seed, STEP_N)
    p = wlm_cases.partials_of(J, x, f, w, device)
    if feed == "flat":
        p[:, :21] = 0.0
    return (J, x, f, w), p


def reference_update(ref, theta, J, x, f, w, hyper):
    """lm_cases.reference_update with the normal equations of weighted_multiview_normal_equations_reference: J
    (V, N, 6), x, f, w (V, N) of one start -> (the next trial parameters in float64, unrounded; ncc_views, sw_views)"""
    ncc, A, g, ncc_v, sw_v = (t.numpy() for t in weighted_multiview_normal_equations_reference(
        torch.tensor(J)[None], torch.tensor(x)[None], torch.tensor(f), torch.tensor(w), hyper["ncc_eps"]))
    ncc, A, g = float(ncc[0]), A[0], g[0]
    ref["Sw"], ref["last"] = float(sw_v.sum()), (ncc, A, g)
    if not ref["valid"] or ncc > ref["ncc"]:
        ref["margin"] = abs(ncc - ref["ncc"]) if ref["valid"] else np.inf
        ref.update(best=theta.copy(), ncc=ncc, A=A, g=g, valid=True, accepted=True)
        ref["lam"] = max(ref["lam"] * hyper["down"], hyper["damping_min"])
    else:
        ref["margin"] = abs(ncc - ref["ncc"])
        ref["accepted"] = False
        ref["lam"] = min(ref["lam"] * hyper["up"], hyper["damping_max"])
    M = ref["A"] + ref["lam"] * np.diag(np.diag(ref["A"])) + 1e-30 * np.eye(6)
    try:
        Lc = np.linalg.cholesky(M)
        delta = np.linalg.solve(Lc.T, np.linalg.solve(Lc, -ref["g"]))
    except np.linalg.LinAlgError:
        delta = np.zeros(6)
        ref["lam"] = min(ref["lam"] * hyper["up"], hyper["damping_max"])
    return ref["best"] + delta, ncc_v[0], sw_v[0]


def check_step_sequences(V, device, ops):
    """ddrr_wmvlm_step with V > 1 views on fed weighted partials against weighted_multiview_normal_equations_reference
    + the float64 update, over mvlm_cases.SEQUENCES and the sequences with a start emptied of its weights: theta
    within 2 ulps of float32, the damping exactly, accept / reject, the best NCC, state[37], ncc_views within 1 ulp,
    sw_views to 1e-12; an empty start stays where it is and reports 0."""
    start = np.concatenate([mvlm_cases.STEP_START[:3], mvlm_cases.STEP_START[3:]])
    traces = []
    for feeds, hyper, S in W_SEQUENCES:
        state, rot, xyz = fresh(S, device, ops)
        refs = [dict(valid=False, lam=1.0, ncc=0.0) for _ in range(S)]
        views = torch.full((S, V), -2.0, device=device)
        sws = torch.full((S, V), -2.0, dtype=torch.float64, device=device)
        trace = []
        for call in feeds:
            theta = torch.cat([rot, xyz], 1).cpu().numpy().astype(np.float64)
            parts, want = [], []
            for s, feed in enumerate(call):
                data = [view_data(feed, v, device) for v in range(V)]
                parts += [p for _, p in data]
                want.append(None if feed == "flat" else reference_update(
                    refs[s], theta[s], *(np.stack([d[0][k] for d in data]) for k in range(4)), hyper))
            ws = torch.stack(parts).contiguous()  # (S V, G, 45): pose s V + v
            lam_before, valid_before = state[:, 34].cpu().numpy().copy(), state[:, 35].cpu().numpy().copy()
            ncc = ops.wmvlm_step(ws, state, rot, xyz, V, STEP_N, **hyper, ncc_views=views, sw_views=sws)
            got, st = torch.cat([rot, xyz], 1).cpu().numpy(), state.cpu().numpy()
            nv, sv = views.cpu().numpy(), sws.cpu().numpy()
            assert np.isfinite(st).all() and np.isfinite(got).all() and np.isfinite(nv).all() and np.isfinite(sv).all()
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
                trial, ncc_v, sw_v = want[s]
                u = ulps32(got[s], trial)
                assert (u <= 2).all(), (s, feed, got[s], trial, u)
                assert st[s, 34] == refs[s]["lam"], (s, feed, st[s, 34], refs[s]["lam"])  # exactly
                assert bool(st[s, 36]) == refs[s]["accepted"] and st[s, 35] == 1.0
                assert abs(st[s, 6] - refs[s]["ncc"]) <= 1e-12 and float(ncc[s]) == np.float32(st[s, 6])
                assert abs(st[s, 37] - refs[s]["Sw"]) <= 1e-12 * max(1.0, refs[s]["Sw"])
                assert (ulps32(nv[s], ncc_v) <= 1).all(), (s, nv[s], ncc_v)
                assert (np.abs(sv[s] - sw_v) <= 1e-12 * np.maximum(1.0, sw_v)).all(), (s, sv[s], sw_v)
                if feed == "empty":  # (the render judged is worth 0 and solves nothing)
                    assert st[s, 37] == 0.0 and not nv[s].any() and not sv[s].any()
                    if not valid_before[s]:
                        assert np.array_equal(got[s], start) and st[s, 6] == 0.0 and float(ncc[s]) == 0.0
            trace.append((st[:, 34].copy(), st[:, 36].copy(), got.copy()))
        traces.append(trace)
    d = HYPER["down"]
    assert [bool(a[0]) for _, a, _ in traces[0]] == [True, True, False, True]
    assert [lam[0] for lam, _, _ in traces[0]] == [d, d * d, d * d * 4.0, d * d * 4.0 * d]
    assert [lam[0] for lam, _, _ in traces[1]] == [1 / 3, 0.2, 0.8, 1.5, 1.5]
    assert [list(a.astype(bool)) for _, a, _ in traces[4]][1][:2] == [True, False]
    # nothing left of the start, twice: parameters unchanged, first accepted (a first render is), then not
    assert all(np.array_equal(got[0], start) for _, _, got in traces[5])
    assert [bool(a[0]) for _, a, _ in traces[5]] == [True, False]


def check_step_one_view_is_wlm_step(device, ops):
    """V = 1 on fed partials: state, theta and the NCC equal ddrr_wlm_step's bit for bit over every sequence; ncc_views
    and sw_views are the render's."""
    for feeds, hyper, S in W_SEQUENCES:
        mine, theirs = fresh(S, device, ops), fresh(S, device, ops)
        views = torch.zeros(S, 1, device=device)
        sws = torch.zeros(S, 1, dtype=torch.float64, device=device)
        for call in feeds:
            ws = torch.stack([view_data(feed, 0, device)[1] for feed in call]).contiguous()
            ncc_m = ops.wmvlm_step(ws, *mine, 1, STEP_N, **hyper, ncc_views=views, sw_views=sws)
            ncc_t = ops.wlm_step(ws, *theirs, STEP_N, **hyper)
            assert torch.equal(ncc_m, ncc_t)
            for m, t in zip(mine, theirs):
                assert torch.equal(m, t), (call, m, t)
            acc = mine[0][:, 36] != 0
            assert torch.equal(views[acc, 0], mine[0][acc, 6].to(torch.float32))
            assert torch.equal(sws[:, 0], mine[0][:, 37])


def ulps64(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def check_step_with_unit_weights_is_mvlm_step(V, device, ops):
    """Partials of w == 1 (the 44 sums and the ray counts): theta, the damping and accept / reject equal
    ddrr_mvlm_step's bit for bit over mvlm_cases.SEQUENCES and the best NCC is within 4 double ulps (C / Sw against
    (sum ncc_v) / V).  First, with the float64 reference: no judgement of these sequences is within 1e-12 of a tie,
    so that the last bits of the NCC cannot change an outcome."""
    for feeds, hyper, S in SEQUENCES:
        mine, theirs = fresh(S, device, ops), fresh(S, device, ops)
        refs = [dict(valid=False, lam=1.0, ncc=0.0) for _ in range(S)]
        for call in feeds:
            parts, plain = [], []
            for s, feed in enumerate(call):
                data = [view_data(feed, v, device, ones=True) for v in range(V)]
                parts += [p for _, p in data]
                plain += [p[:, :44] for _, p in data]
                if feed != "flat":
                    reference_update(refs[s], np.zeros(6), *(np.stack([d[0][k] for d in data]) for k in range(4)), hyper)
                    assert refs[s]["margin"] > 1e-12, (feed, refs[s]["margin"])
            ws, ws0 = torch.stack(parts).contiguous(), torch.stack(plain).contiguous()
            assert torch.equal(ws[..., 44].sum(1), torch.full((S * V,), float(STEP_N), dtype=torch.float64, device=device))
            ncc_m = ops.wmvlm_step(ws, *mine, V, STEP_N, **hyper)
            ncc_t = ops.mvlm_step(ws0, *theirs, V, STEP_N, **hyper)
            sm, st = mine[0].cpu().numpy(), theirs[0].cpu().numpy()
            assert torch.equal(mine[1], theirs[1]) and torch.equal(mine[2], theirs[2]), (call, mine[1:], theirs[1:])
            assert np.array_equal(sm[:, :6], st[:, :6]) and np.array_equal(sm[:, 7:37], st[:, 7:37])
            assert (ulps64(sm[:, 6], st[:, 6]) <= 4).all(), (sm[:, 6], st[:, 6])
            assert (ulps32(ncc_m.cpu().numpy(), ncc_t.cpu().numpy()) <= 1).all()
            assert np.array_equal(sm[:, 37], np.full(S, float(V * STEP_N)))


def check_step_skips_empty_views(device, ops):
    """A view whose partials are all zero -- the first, a middle, the last of three: state, parameters, NCC and the
    other views' ncc_views and sw_views equal, bit for bit, the call with that view removed, over every call of the
    three-start sequence; its own ncc_views and sw_views are 0."""
    feeds, hyper, S = SEQUENCES[4]
    for k in range(3):
        rest = [v for v in range(3) if v != k]
        full, less = fresh(S, device, ops), fresh(S, device, ops)
        nv3, sw3 = torch.full((S, 3), -2.0, device=device), torch.full((S, 3), -2.0, dtype=torch.float64, device=device)
        nv2, sw2 = torch.full((S, 2), -2.0, device=device), torch.full((S, 2), -2.0, dtype=torch.float64, device=device)
        for call in feeds:
            parts = [[view_data(feed, v, device)[1] for v in range(3)] for feed in call]
            for p in parts:
                p[k] = torch.zeros_like(p[k])
            ws3 = torch.stack([p for start in parts for p in start]).contiguous()
            ws2 = torch.stack([start[v] for start in parts for v in rest]).contiguous()
            a = ops.wmvlm_step(ws3, *full, 3, STEP_N, **hyper, ncc_views=nv3, sw_views=sw3)
            b = ops.wmvlm_step(ws2, *less, 2, STEP_N, **hyper, ncc_views=nv2, sw_views=sw2)
            assert torch.equal(a, b), (k, call)
            for m, t in zip(full, less):
                assert torch.equal(m, t), (k, call)
            assert torch.equal(nv3[:, rest], nv2) and torch.equal(sw3[:, rest], sw2), (k, call)
            assert not bool(nv3[:, k].any()) and not bool(sw3[:, k].any())
        assert bool((full[0][:, 35] == 1).all())


def normal_equations_of(state):
    """A (6, 6) and g (6) as the step kept them for the best render (state[7:28], state[28:34])"""
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = state[7:28]
    return A + np.triu(A, 1).T, state[28:34].copy()


def check_step_scaling(V, device, ops):
    """One view's partials x 4: A and g of the accepted render equal the reference's with that view's weight x 4
    (to 1e-9 of their largest entry: both are float64, the kernel's from sums whose cancellation, for these images'
    means and variances, costs at most a few digits of the 16), and that view counts four times in the judged NCC.
    All views x 4: the judged NCC keeps its value (to 4 double ulps) and the next trial is within 1 float32 ulp of the
    unscaled step's, as wlm_cases.check_power_of_four_scaling."""
    feed = (2, 0.3)
    outs = {}
    for label, scales in [("as they are", [1.0] * V), ("all x 4", [4.0] * V)] + [
            (f"view {k} x 4", [4.0 if v == k else 1.0 for v in range(V)]) for k in range(V)]:
        data = [view_data(feed, v, device, scale=scales[v]) for v in range(V)]
        ws = torch.stack([p for _, p in data]).contiguous()
        state, rot, xyz = fresh(1, device, ops)
        ops.wmvlm_step(ws, state, rot, xyz, V, STEP_N, **HYPER)
        st = state.cpu().numpy()[0]
        ncc, A, g, _, sw_v = (t.numpy() for t in weighted_multiview_normal_equations_reference(
            *(torch.tensor(np.stack([d[0][k] for d in data]))[None] if k < 2 else torch.tensor(
                np.stack([d[0][k] for d in data])) for k in range(4)), HYPER["ncc_eps"]))
        mine_A, mine_g = normal_equations_of(st)
        assert st[36] == 1.0 and abs(st[6] - float(ncc[0])) <= 1e-12 and abs(st[37] - sw_v.sum()) <= 1e-12 * sw_v.sum()
        assert np.abs(mine_A - A[0]).max() <= 1e-9 * np.abs(A[0]).max(), (label, np.abs(mine_A - A[0]).max())
        assert np.abs(mine_g - g[0]).max() <= 1e-9 * np.abs(g[0]).max(), (label, np.abs(mine_g - g[0]).max())
        outs[label] = (st, torch.cat([rot, xyz], 1).cpu().numpy()[0], mine_A)
    (s1, t1, A1), (s4, t4, A4) = outs["as they are"], outs["all x 4"]
    print(f"V={V}: the next trial under 4 w in every view equals the one under w bit for bit: {np.array_equal(t1, t4)}")
    assert (ulps32(t1, t4) <= 1).all() and s4[37] == 4 * s1[37] and ulps64(s1[6], s4[6]) <= 4
    assert np.abs(A4 - 4 * A1).max() <= 1e-12 * np.abs(A4).max()
    assert not np.array_equal(t1, mvlm_cases.STEP_START)
    for k in range(V):  # (a view that counts four times pulls the judged NCC towards its own)
        assert not np.array_equal(outs[f"view {k} x 4"][1], t1) and outs[f"view {k} x 4"][0][6] != s1[6]


def check_step_neighbours(device, ops):
    """A start's outputs do not depend on its neighbours' partials: three starts, two views, start 1's partials
    replaced by another image pair's and then emptied; starts 0 and 2 step to the same bits."""
    V, call = 2, [(1, 0.8), (2, 0.3), (3, 0.2)]
    runs = []
    for middle in ((2, 0.3), (5, 0.9), "empty"):
        parts = [view_data(middle if s == 1 else feed, v, device)[1] for s, feed in enumerate(call) for v in range(V)]
        state, rot, xyz = fresh(3, device, ops)
        nv, sw = torch.zeros(3, V, device=device), torch.zeros(3, V, dtype=torch.float64, device=device)
        ncc = ops.wmvlm_step(torch.stack(parts).contiguous(), state, rot, xyz, V, STEP_N, **HYPER, ncc_views=nv,
                             sw_views=sw)
        runs.append((ncc, state, rot, xyz, nv, sw))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a[[0, 2]], b[[0, 2]]) and bool(torch.isfinite(b).all())
        assert not torch.equal(runs[0][4][1], other[4][1])


# ------------------------------------------------------------------------------------------------ registration
def _start(device, S=1):
    return [(TRUTH[k] + OFFSET[k]).to(device).repeat(S, 1) for k in (0, 1)]


def occluded_biplane(device):
    """mvlm_cases.mv_scene (lm_cases.convergence_scene seen from 0 and pi / 2) with a bright bar over rows 10-17 of
    view 0's fixed image and over columns 20-27 of view 1's, and the per-view weight that masks each
    -> (module, clean images (2, 1, 48, 48), occluded images, weight, views)"""
    drr, fixed, K = mvlm_cases.mv_scene(device)
    occluded, weight = fixed.clone(), torch.ones_like(fixed)
    occluded[0, :, 10:18, :] = 2 * fixed.max()
    occluded[1, :, :, 20:28] = 2 * fixed.max()
    weight[0, :, 10:18, :] = 0.0
    weight[1, :, :, 20:28] = 0.0
    return drr, fixed, occluded, weight, K


def run(lm, steps=60, stop=True):
    """-> (the trial parameters rendered [(rot, xyz)], the best NCC after every step, (the smallest q of the best
    parameters, its step))"""
    track, nccs, best = [], [], (float("inf"), 0)
    for it in range(1, steps + 1):
        track.append((lm.reg.rotation.detach().clone(), lm.reg.translation.detach().clone()))
        nccs.append(float(lm.step()[0]))
        q = _q(*lm.best_parameters)
        best = min(best, (q, it))
        if stop and nccs[-1] >= 0.9999 and q <= 1.0:
            break
    return track, nccs, best


def _reg(drr, device, S=1):
    rot, xyz = _start(device, S)
    return Registration(drr, rot.clone(), xyz.clone(), parameterization="euler_angles", convention="ZXY")


MASKED_DAMPING_MIN = 0.1  # (check_occluded_biplane's docstring)
Q_PLAIN_FLOOR = 3.61  # a third of the smaller closest approach measured (check_occluded_biplane: 10.83 and 11.32)


def check_occluded_biplane(device, ops):
    """On the occluded biplane pair from TRUTH + OFFSET: the masked object reaches a best NCC >= 0.9999 within one
    tolerance (wncc_cases._q <= 1) inside 60 steps; its first step is the four launches and nothing of the other
    Levenberg-Marquardt libraries; on the host build its trajectory on the occluded images equals the one on the
    clean images bit for bit (on the device, where the record is summed with float atomics and no two runs step
    alike, the clean run is printed).  The existing unmasked MultiViewLevenbergMarquardt on the occluded images never
    comes close in 60 steps: its closest approach q_plain, measured 10.83 (step 8) on the host build and 11.32 (step 7)
    on the MI355X from a start at q = 18, is asserted >= 3.61, a third of the smaller of the two (the margin wlm_cases
    took: measured 15, asserted 5).

    The masked objects run with ``damping_min=MASKED_DAMPING_MIN`` (0.1), not the default floor of 1e-7.  The scene's
    truth is the axis-aligned pose, where the rays run along the voxel planes: the fixed images carry that pose's
    aliasing, and the float32 objective has a needle there, 1e-4 rad wide in the second Euler angle and 1.5e-4 of NCC
    high, all the way along the first Euler angle (scanned on the host build at rot = (0.0229, 6e-5, 0.0018)).  With
    the default floor the last steps are pure Gauss-Newton steps, which can land the second angle inside the needle
    while the first is still 2.3 tolerances off; every further step leaves the needle, is rejected, and the run ends at
    NCC 0.99946, q = 2.29: 9 of 40 and 4 of 30 runs on the MI355X (each with its own float-atomic noise), 1 of 40 on
    the host build from starts jittered by 1e-4, and likewise with unit weights on the clean images.  A floor makes
    the iteration near the solution a linear contraction of all six parameters at one rate (about lambda / (1 +
    lambda) per step), so that no parameter gets 400 times ahead of another: 0 of 40 runs on the MI355X stall, 19 to 25
    steps.  The bounds are the issue's: NCC >= 0.9999, q <= 1, 60 steps."""
    drr, fixed, occluded, weight, K = occluded_biplane(device)
    lm = WeightedMultiViewLevenbergMarquardt(_reg(drr, device), occluded, K, weight=weight)
    assert lm.view_ncc.shape == (1, 2) and lm.view_weight_sum.shape == (1, 2) and lm.weight_sum.shape == (1,)
    assert float(lm.view_weight_sum.abs().max()) == 0 and lm.view_weight_sum.dtype == torch.float64
    with launches(ops) as names:
        lm.step()
    assert names == ["ddrr_wmvlm_raygen", "ddrr_siddon_forward_bricks", "ddrr_wmvlm_normal_sums",
                     "ddrr_wmvlm_step"], names
    lm = WeightedMultiViewLevenbergMarquardt(_reg(drr, device), occluded, K, weight=weight,
                                             damping_min=MASKED_DAMPING_MIN)
    with launches(ops) as names:
        track, nccs, (q, it) = run(lm)
    print(f"masked biplane LM on the occluded images: best NCC {nccs[-1]:.6f}, q = {_q(*lm.best_parameters):.3g} "
          f"after {len(track)} steps; per view {lm.view_ncc.tolist()}")
    assert nccs[-1] >= 0.9999 and _q(*lm.best_parameters) <= 1.0, (nccs[-1], q, it)
    assert len(names) == 4 * len(track) and lm.steps_done == len(track)
    assert not any(n.startswith(("ddrr_lm_", "ddrr_wlm_", "ddrr_mvlm_", "ddrr_pose_raygen")) for n in names)
    # bookkeeping: the sums of the weights, commit
    want = weight.reshape(2, -1).double().sum(1)
    assert torch.allclose(lm.view_weight_sum[0], want, rtol=1e-12, atol=0)
    assert float(lm.weight_sum[0]) == float(lm.view_weight_sum[0].sum())
    trial = lm.reg.rotation.detach().clone()
    lm.commit()
    assert torch.equal(lm.reg.rotation.detach(), lm.best_parameters[0])
    assert torch.equal(lm.reg.translation.detach(), lm.best_parameters[1])
    assert _q(lm.reg.rotation, lm.reg.translation) <= 1.0
    assert not torch.equal(trial, lm.reg.rotation.detach()) or bool(lm.accepted[0])

    plain = MultiViewLevenbergMarquardt(_reg(drr, device), occluded, K)
    _, plain_nccs, (q_plain, it_plain) = run(plain, stop=False)
    print(f"unmasked biplane LM on the occluded images: best mean NCC {plain_nccs[-1]:.4f}, closest approach q_plain = "
          f"{q_plain:.4g} at step {it_plain} of 60")
    assert q_plain >= Q_PLAIN_FLOOR, (q_plain, it_plain)

    on_host = device.type == "cpu"
    clean = WeightedMultiViewLevenbergMarquardt(_reg(drr, device), fixed, K, weight=weight,
                                                damping_min=MASKED_DAMPING_MIN)
    clean_track, clean_nccs, _ = run(clean, steps=len(track) if on_host else 60, stop=not on_host)
    if on_host:
        assert len(clean_track) == len(track) and clean_nccs == nccs
        assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(track, clean_track))
        assert torch.equal(clean._state, lm._state) and torch.equal(clean.view_ncc, lm.view_ncc)
    else:
        print(f"masked biplane LM on the clean images: best NCC {clean_nccs[-1]:.6f}, q = "
              f"{_q(*clean.best_parameters):.3g} after {len(clean_track)} steps")
    return q_plain


def check_calibrated_biplane(device, ops):
    """View 1 rendered and registered with the view-1 detector of :func:`detectors` (another source-detector distance,
    pitch and principal point): the object with ``detectors=(None, det_1)`` reaches best NCC >= 0.9999 with q <= 1
    inside 60 steps.  Printed, not asserted: what the object without ``detectors`` reaches on the same images."""
    drr, fixed, K = mvlm_cases.mv_scene(device)
    det1 = detectors(drr)[1]
    with torch.no_grad():
        lateral = with_detector(drr, det1)(view_poses(TRUTH[0].to(device), TRUTH[1].to(device), K[1:2], "ZXY"))
    images = torch.cat([fixed[:1], lateral.reshape(1, 1, 48, 48)]).contiguous()
    assert float(images.abs().amax((1, 2, 3)).min()) > 0 and not torch.equal(images[1], fixed[1])
    lm = WeightedMultiViewLevenbergMarquardt(_reg(drr, device), images, K, detectors=(None, det1))
    assert lm._P.shape == (2, 48 * 48, 3) and not torch.equal(lm._P[0], lm._P[1])
    track, nccs, (q, it) = run(lm)
    print(f"calibrated biplane LM: best NCC {nccs[-1]:.6f}, q = {_q(*lm.best_parameters):.3g} after {len(track)} "
          f"steps; per view {lm.view_ncc.tolist()}")
    assert nccs[-1] >= 0.9999 and _q(*lm.best_parameters) <= 1.0, (nccs[-1], q, it)
    assert float(lm.view_weight_sum.min()) == 48 * 48 and float(lm.weight_sum[0]) == 2 * 48 * 48
    same = WeightedMultiViewLevenbergMarquardt(_reg(drr, device), images, K, detectors=(None, None))
    assert same._P is None
    _, wrong_nccs, (q_wrong, it_wrong) = run(same, stop=False)
    print(f"the same images without `detectors`: best NCC {wrong_nccs[-1]:.6f}, closest approach q = {q_wrong:.3g} at "
          f"step {it_wrong} of 60")


def check_multi_starts(device, ops):
    """S = 3 starts, two views, per-view weights and detectors.  On the host build each runs as it runs alone, bit for
    bit (a render is reproducible there; on the device the record is summed with float atomics and two runs of ONE
    start differ).  jacobian() is (S, V, N, 6), does not depend on the weight and moves nothing; without weight and
    detectors it is the parent's; the best NCC never falls; weight_sum is the sum of view_weight_sum, which holds the
    weights' float64 sums."""
    drr, fixed, occluded, weight, K = occluded_biplane(device)
    det1 = detectors(drr)[1]
    w = weight * (0.5 + torch.rand(2, 1, 48, 48, generator=torch.Generator().manual_seed(5)).to(device))
    rots = torch.tensor([[0.08, -0.06, 0.07], [-0.05, 0.04, 0.02], [0.03, 0.0, -0.02]], device=device)
    xyzs = torch.tensor([[6.0, 391.0, 5.0], [-4.0, 405.0, 3.0], [2.0, 398.0, -3.0]], device=device)

    def build(b=slice(0, 3), **kw):
        reg = Registration(drr, rots[b].clone(), xyzs[b].clone(), parameterization="euler_angles", convention="ZXY")
        return reg, WeightedMultiViewLevenbergMarquardt(reg, occluded, K, damping=2.0, **kw)

    reg, lm = build(weight=w, detectors=[None, det1])
    assert torch.equal(lm.damping, torch.full((3,), 2.0, dtype=torch.float64, device=device))
    assert lm.weight.shape == (2, 48 * 48) and (lm.S, lm.V, lm.N) == (3, 2, 48 * 48)
    J = lm.jacobian()
    assert J.shape == (3, 2, 48 * 48, 6) and bool(torch.isfinite(J).all()) and float(J.abs().max()) > 0
    assert torch.equal(reg.rotation.detach(), rots) and lm.steps_done == 0  # (jacobian() moves nothing)
    J1 = build(detectors=[None, det1])[1].jacobian()  # (no weight: ones)
    Jp = build()[1].jacobian()
    J0 = MultiViewLevenbergMarquardt(Registration(drr, rots.clone(), xyzs.clone(), parameterization="euler_angles",
                                                  convention="ZXY"), occluded, K).jacobian()
    if device.type == "cpu":
        assert torch.equal(J, J1) and torch.equal(Jp, J0) and torch.equal(J[:, 0], J0[:, 0])
    assert float((J - J1).abs().max()) <= 1e-4 * float(J.abs().max())  # (two renders: float atomics on the device)
    assert float((Jp - J0).abs().max()) <= 1e-4 * float(J0.abs().max())
    assert float((J[:, 1] - J0[:, 1]).abs().max()) > 1e-2 * float(J0.abs().max())  # (view 1 is on its own detector)
    history = [lm.step().clone() for _ in range(6)]
    assert history[0].shape == (3,) and not history[0].requires_grad
    assert all((b >= a).all() for a, b in zip(history, history[1:]))  # the best NCC never falls
    assert lm.view_ncc.shape == (3, 2) and lm.accepted.shape == (3,) and lm.best_ncc.shape == (3,)
    want = w.reshape(2, -1).double().sum(1)
    assert torch.allclose(lm.view_weight_sum, want.expand(3, -1), rtol=1e-12, atol=0)
    assert torch.equal(lm.weight_sum, lm.view_weight_sum[:, 0] + lm.view_weight_sum[:, 1])
    for s in range(3):
        reg_s, lm_s = build(slice(s, s + 1), weight=w, detectors=[None, det1])
        for _ in range(6):
            last = lm_s.step()
        print(f"start {s} in the batch and alone after six steps: best NCC {float(history[-1][s]):.7f} / "
              f"{float(last[0]):.7f}, damping {float(lm.damping[s]):.3g} / {float(lm_s.damping[0]):.3g}")
        if device.type == "cpu":
            assert torch.equal(lm._state[s], lm_s._state[0])
            assert torch.equal(reg.rotation.detach()[s], reg_s.rotation.detach()[0])
            assert torch.equal(reg.translation.detach()[s], reg_s.translation.detach()[0])
            assert torch.equal(lm.view_ncc[s], lm_s.view_ncc[0])
            assert torch.equal(lm.view_weight_sum[s], lm_s.view_weight_sum[0])
        assert float(last[0]) > float(history[0][s])  # (it moved, and for the better)
    lm.commit()
    assert torch.equal(reg.rotation.detach(), lm.best_parameters[0])
    # the weight is read in place at every step: emptied, the next render is worth 0 and is rejected
    shared = torch.ones(1, 1, 48, 48, device=device)
    reg, lm = build(slice(0, 1), weight=shared)
    assert lm.weight.data_ptr() == shared.data_ptr()
    lm.step()
    shared.zero_()
    lm.step()
    assert float(lm.weight_sum[0]) == 0 and not bool(lm.accepted[0]) and not bool(lm.view_ncc.any())


# ------------------------------------------------------------------------------------------------ surface
def check_errors(device, elsewhere):
    """ValueErrors of the constructor name the condition: the weight's shape, dtype, device, sign, NaN, Inf; the
    detectors' number, grid, subsample and type; and what the parent class refuses.  `elsewhere`: a device the
    parameters are not on."""
    drr, fixed, K = mvlm_cases.mv_scene(device)
    dets = detectors(drr)
    d = drr.detector

    def build(fixed=fixed, views=K, S=1, par="euler_angles", conv="ZXY", rot=None, **kw):
        rot_, xyz_ = _start(device, S)
        reg = Registration(drr, (rot_ if rot is None else rot).clone(), xyz_.clone(), parameterization=par,
                           convention=conv)
        return WeightedMultiViewLevenbergMarquardt(reg, fixed, views, **kw)

    lm = build()
    assert (lm.S, lm.V, lm.N) == (1, 2, 48 * 48) and lm.fixed.shape == (2, 48 * 48)
    assert lm.weight.shape == (1, 48 * 48) and bool((lm.weight == 1).all()) and lm._P is None
    assert lm._ws.shape == (2, 3, _lib.WMVLM_SUMS) and isinstance(lm, MultiViewLevenbergMarquardt)
    ones = torch.ones(2, 1, 48, 48, device=device)
    assert build(weight=ones).weight.shape == (2, 48 * 48) and build(weight=ones[:1]).weight.shape == (1, 48 * 48)
    assert build(detectors=[None, dets[1]])._P.shape == (2, 48 * 48, 3)
    assert build(detectors=(d, None))._P is None  # (the module's own detector for every view: one set of points)
    neg, nan, inf = ones.clone(), ones.clone(), ones.clone()
    neg[1, 0, 3, 4] = -1.0
    nan[0, 0, 5, 6] = float("nan")
    inf[1, 0, 5, 6] = float("inf")
    small = Detector(d.sdd, 40, 48, d.delx, d.dely, 0.0, 0.0, d._reorient.detach().cpu().clone()).to(device)
    sparse = Detector(d.sdd, 48, 48, d.delx, d.dely, 0.0, 0.0, d._reorient.detach().cpu().clone(),
                      n_subsample=100).to(device)
    for kw, what in ((dict(weight=ones[:, :, :40]), "shape"), (dict(weight=ones[0]), "shape"),
                     (dict(weight=torch.ones(3, 1, 48, 48, device=device)), "shape"),
                     (dict(weight=ones.double()), "float32"),
                     (dict(weight=ones.numpy() if device.type == "cpu" else 1.0), "float32"),
                     (dict(weight=torch.ones(2, 1, 48, 48, device=elsewhere)), "device"), (dict(weight=neg), "negative"),
                     (dict(weight=nan), "finite"), (dict(weight=inf), "finite"),
                     (dict(detectors=[None]), "sequence of 2"), (dict(detectors=[None, None, None]), "sequence of 2"),
                     (dict(detectors=dets[1]), "sequence of 2"), (dict(detectors=[None, small]), "height x width"),
                     (dict(detectors=[sparse, None]), "n_subsample"), (dict(detectors=[None, "lateral"]), "Detector"),
                     (dict(detectors=[None, 3.0]), "Detector"),
                     # ... and everything the parent class refuses
                     (dict(views=K[0]), "V, 4, 4"), (dict(views=K[:0]), "V, 4, 4"), (dict(views=K.long()), "V, 4, 4"),
                     (dict(fixed=fixed[:1]), "fixed"), (dict(fixed=fixed.double()), "fixed"),
                     (dict(fixed=torch.zeros(2, 1, 48, 48, device=elsewhere)), "device"),
                     (dict(S=17), "rendered poses"), (dict(S=0), "rendered poses"),
                     (dict(par="axis_angle", conv=None), "euler_angles"), (dict(rot=_start(device)[0].double()), "float32"),
                     (dict(up=1.0), "damping"), (dict(damping=1e7), "damping"), (dict(eps=-1.0), "eps")):
        with pytest.raises(ValueError, match=what):
            build(**kw)
    shear = K.clone()
    shear[1, 0, 1] += 0.01
    with pytest.raises(ValueError, match="WeightedMultiViewLevenbergMarquardt: views must be rigid"):
        build(views=shear)
    with pytest.raises(TypeError):  # (the parent class takes no weight, as before)
        MultiViewLevenbergMarquardt(_reg(drr, device), fixed, K, weight=ones)


def check_ops_errors(ops):
    """The ops refuse what the entries would misread, without a launch; S = 0 is a no-op."""
    S, V, N = 2, 3, 1500
    state = ops.lm_state(S, 1.0, "cpu")
    rot, xyz = torch.zeros(S, 3), torch.zeros(S, 3)
    ws = ops.wmvlm_workspace(S, V, N, "cpu")
    assert ws.shape == (S * V, 2, 45) and ws.dtype == torch.float64
    assert ops.wmvlm_workspace(0, 2, 100, "cpu").numel() == 0
    Ro = torch.zeros(V, 3, 4)
    with launches(ops) as launched:
        for bad in (ws[:, :1].contiguous(), ops.mvlm_workspace(S, V, N, "cpu"), ops.wlm_workspace(S, N, "cpu"),
                    ops.lm_workspace(S * V, N, "cpu"), ws.float(), ws.reshape(-1)):
            with pytest.raises(ValueError, match="ws"):
                ops.wmvlm_step(bad, state, rot, xyz, V, N)
        with pytest.raises(ValueError, match="ws"):
            ops.wmvlm_step(ws, state, rot, xyz, V - 1, N)
        with pytest.raises(ValueError, match="V >= 1"):
            ops.wmvlm_step(ws, state, rot, xyz, 0, N)
        with pytest.raises(ValueError, match="state"):
            ops.wmvlm_step(ws, state.float(), rot, xyz, V, N)
        with pytest.raises(ValueError, match="state"):
            ops.wmvlm_step(ws, ops.lm_state(S * V, 1.0, "cpu"), rot, xyz, V, N)
        with pytest.raises(ValueError, match="device"):
            ops.wmvlm_step(ws, ops.lm_state(S, 1.0, "meta"), rot, xyz, V, N)
        with pytest.raises(ValueError, match="pose parameters"):
            ops.wmvlm_step(ws, state, rot.double(), xyz, V, N)
        with pytest.raises(ValueError, match="up > 1"):
            ops.wmvlm_step(ws, state, rot, xyz, V, N, down=1.5)
        with pytest.raises(ValueError, match="ncc_views"):
            ops.wmvlm_step(ws, state, rot, xyz, V, N, ncc_views=torch.zeros(V, S))
        with pytest.raises(ValueError, match="sw_views"):
            ops.wmvlm_step(ws, state, rot, xyz, V, N, sw_views=torch.zeros(S, V))  # (float32: doubles expected)
        with pytest.raises(ValueError, match="sw_views"):
            ops.wmvlm_step(ws, state, rot, xyz, V, N, sw_views=torch.zeros(S, V, dtype=torch.float64, device="meta"))
        pose = dict(source=torch.zeros(S * V, 1, 3), Mw=torch.zeros(S * V, 3, 4), Ainv=torch.zeros(3, 4),
                    P=torch.zeros(N, 3), rot=rot, xyz=xyz, axes=(2, 0, 1), reorient_v=Ro)
        aux, x1, w = ops.brick_record_buffer(S * V, N, "cpu"), torch.ones(V, N), torch.ones(1, N)
        for bad in (torch.ones(N), torch.ones(1, N), torch.ones(S * V, N), torch.ones(V, N + 1), torch.ones(V, 1, N),
                    torch.ones(V, N).double(), None):
            with pytest.raises(ValueError, match="fixed"):
                ops.wmvlm_normal_sums(aux, bad, w, **pose)
        for bad in (torch.ones(N), torch.ones(2, N), torch.ones(S * V, N), torch.ones(V, N + 1), torch.ones(1, 1, N),
                    torch.ones(V, N).double(), None):  # (w_stride is N or 0: V rows or one)
            with pytest.raises(ValueError, match="weight"):
                ops.wmvlm_normal_sums(aux, x1, bad, **pose)
        for bad in (torch.zeros(N, 4), torch.zeros(2, N, 3), torch.zeros(S * V, N, 3), torch.zeros(V, N, 3).double(),
                    torch.zeros(3 * N), None):  # (P_stride is 3 N or 0: V sets of points or one)
            with pytest.raises(ValueError, match="detector points"):
                ops.wmvlm_normal_sums(aux, x1, w, **dict(pose, P=bad))
            with pytest.raises(ValueError, match="detector points"):
                ops.wmvlm_raygen(rot, xyz, (2, 0, 1), Ro, pose["Ainv"], bad)
        for k, t in (("fixed", torch.ones(V, N, device="meta")), ("weight", torch.ones(1, N, device="meta")),
                     ("P", torch.zeros(N, 3, device="meta"))):
            with pytest.raises(ValueError, match="device"):
                ops.wmvlm_normal_sums(aux, **dict(dict(pose, fixed=x1, weight=w), **{k: t}))
        with pytest.raises(ValueError, match="device"):
            ops.wmvlm_raygen(rot, xyz, (2, 0, 1), Ro, pose["Ainv"], torch.zeros(V, N, 3, device="meta"))
        with pytest.raises(ValueError, match="reorient_v"):
            ops.wmvlm_normal_sums(aux, x1, w, **dict(pose, reorient_v=Ro[0]))
        with pytest.raises(ValueError, match="reorient_v"):
            ops.wmvlm_raygen(rot, xyz, (2, 0, 1), Ro.double(), pose["Ainv"], pose["P"])
        with pytest.raises(ValueError, match="S \\* V"):
            ops.wmvlm_normal_sums(aux, x1, w, **dict(pose, Mw=torch.zeros(S, 3, 4)))
        for bad in (ops.mvlm_workspace(S, V, N, "cpu"), ops.wlm_workspace(S, N, "cpu"), ops.lm_workspace(S, N, "cpu")):
            with pytest.raises(ValueError, match="ws"):
                ops.wmvlm_normal_sums(aux, x1, w, **pose, ws=bad)
        with pytest.raises(ValueError, match="pose parameters"):
            ops.wmvlm_raygen(rot.double(), xyz, (2, 0, 1), Ro, pose["Ainv"], pose["P"])
        with pytest.raises(ValueError, match="65535"):
            ops.wmvlm_raygen(torch.zeros(300, 3), torch.zeros(300, 3), (2, 0, 1), torch.zeros(300, 3, 4), pose["Ainv"],
                             pose["P"])
        with pytest.raises(ValueError, match="empty batch"):
            ops.wmvlm_raygen(rot[:0], xyz[:0], (2, 0, 1), Ro, pose["Ainv"], pose["P"], clear=torch.zeros(4))
        out = ops.wmvlm_step(ops.wmvlm_workspace(0, 2, 100, "cpu"), ops.lm_state(0, 1.0, "cpu"), torch.zeros(0, 3),
                             torch.zeros(0, 3), 2, 100)
        Mw, source, target, img = ops.wmvlm_raygen(rot[:0], xyz[:0], (2, 0, 1), Ro, pose["Ainv"], pose["P"])
        ws0, jac0 = ops.wmvlm_normal_sums(ops.brick_record_buffer(0, N, "cpu"), x1, w, **dict(
            pose, source=torch.zeros(0, 1, 3), Mw=torch.zeros(0, 3, 4), rot=rot[:0], xyz=xyz[:0]), want_jacobian=True)
    assert out.shape == (0,) and Mw.shape == (0, 3, 4) and img.shape == (0, N) and not launched
    assert ws0.numel() == 0 and jac0.shape == (0, N, 6)


def check_entries_refuse_bad_arguments():
    """The C entries themselves (the host build: the same checks as the gfx950 build, wmvlm_core.h) return -1 with a
    message, before anything runs, for strides other than 0 | N and 0 | 3 N, more than 65535 poses and misaligned
    buffers; S == 0 returns 0."""
    import ctypes

    lib = emu_library()
    N = 8
    f = (ctypes.c_float * (64 * N))()
    d = (ctypes.c_double * 256)()
    p, q = ctypes.addressof(f), ctypes.addressof(d)

    def sums(w_stride=0, P_stride=0, S=1, V=2, ws=q):
        return lib.cdll.ddrr_wmvlm_normal_sums(p, p, p, w_stride, p, p, p, p, P_stride, p, p, 2, 0, 1, p, S, V, N, 1e-8,
                                               1, ws, None, None)

    def raygen(P_stride=0, S=1, V=2):
        return lib.cdll.ddrr_wmvlm_raygen(p, p, 2, 0, 1, p, p, p, P_stride, S, V, N, p, p, p, p, None, 0, None, None)

    def message():
        return lib.cdll.ddrr_wmvlm_last_error().decode()

    assert sums(w_stride=N + 1) == -1 and "w_stride" in message()
    assert sums(w_stride=3 * N) == -1 and "w_stride" in message()
    assert sums(P_stride=N) == -1 and "P_stride" in message()
    assert raygen(P_stride=3 * N + 3) == -1 and "P_stride" in message()
    assert sums(S=300, V=300) == -1 and "65535" in message()
    assert raygen(S=65536, V=1) == -1 and "65535" in message()
    assert sums(ws=q + 4) == -1 and "aligned" in message()
    assert sums(S=0) == 0 and raygen(S=0) == 0 and sums(S=0, w_stride=N, P_stride=3 * N) == 0
    assert lib.cdll.ddrr_wmvlm_step(q, q, p, p, 1, 2, N, 1e-5, 4.0, 1 / 3, 1e-7, 1e6, p, None, q + 4, None) == -1
    assert "aligned" in message()
    assert lib.cdll.ddrr_wmvlm_step(q, q, p, p, 0, 2, N, 1e-5, 4.0, 1 / 3, 1e-7, 1e6, p, None, None, None) == 0
    assert lib.query("ddrr_wmvlm_workspace_bytes", 2, 3, 1500) == 2 * 3 * 2 * 45 * 8
    assert lib.query("ddrr_wmvlm_workspace_bytes", 300, 300, 10) == 0 == lib.query("ddrr_wmvlm_workspace_bytes", 1, 0, 9)
