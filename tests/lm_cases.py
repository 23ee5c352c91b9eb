"""What tests/test_lm.py (host emulation) and tests/test_gpu_lm.py (MI355X) share: the host build of
csrc/lm_core.h, the scenes, the float64 yardsticks and the checks themselves, written once for either device.

The gate of the sums follows the project's rule for gradients: the float32 route the package already has
(one-hot calls of ``ddrr_siddon_backward_pose_euler`` on the SAME record) has an error of its own against the
float64 render route; the kernel may be off by at most twice that, plus a floor of 1e-6 of the entry's scale
(the Cauchy-Schwarz bound of the sum: sqrt(sum u_p^2 sum u_q^2) for sum u_p u_q)."""
import copy
import functools
import os
import subprocess

import numpy as np
import torch

from conftest import ROOT
from diffdrr_amd import DRR, LevenbergMarquardt, Registration, _lib
from diffdrr_amd.data import synthetic_subject
from diffdrr_amd.registration import normal_equations_reference

EMU_SRC = os.path.join(ROOT, "tests", "emu", "lm_emu.cpp")
EMU_LOOPS = os.path.join(ROOT, "tests", "emu", "lm_emu_loops.h")  # the loops of the four host builds
EMU_SO = os.path.join(ROOT, "tests", "emu", "_build", "liblm_emu.so")
FLOOR = 1e-6

# name -> (detector (H, W), delx, poses, convention, stop_gradients_through_grid_sample); 40^3 phantom, sdd 600
SUM_CASES = {
    "780_rays_zxy": ((30, 26), 3.0, 3, "ZXY", False),
    "780_rays_zyx": ((30, 26), 3.0, 3, "ZYX", False),
    "780_rays_zxy_stop": ((30, 26), 3.0, 3, "ZXY", True),
    "780_rays_zyx_stop": ((30, 26), 3.0, 3, "ZYX", True),
    "4087_rays_four_workgroups": ((67, 61), 1.3, 2, "ZXY", False),
    "6_rays": ((2, 3), 20.0, 1, "ZXY", False),
    # two workgroups, the second of a single ray: fewer rays than slices, and three of a thread's four rays clamped
    "1025_rays": ((25, 41), 2.4, 2, "ZYX", False),
}


@functools.lru_cache(maxsize=None)
def emu_library():
    """The host build of the two entries (tests/emu/lm_emu.cpp), bound through the product's own binding."""
    csrc = os.path.join(ROOT, "diffdrr_amd", "csrc")
    deps = [EMU_SRC, EMU_LOOPS, os.path.join(ROOT, "include", "diffdrr_lm_hip.h")] + [
        os.path.join(csrc, f) for f in ("lm_core.h", "siddon_core.h", "raygen_core.h", "record_layout.h",
                                        "ddrr_common.h")]
    if not (os.path.exists(EMU_SO) and all(os.path.getmtime(d) <= os.path.getmtime(EMU_SO) for d in deps)):
        os.makedirs(os.path.dirname(EMU_SO), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-mfma", "-ffp-contract=off",
                        "-Wno-unknown-pragmas", EMU_SRC, "-o", EMU_SO], check=True)
    return _lib.lm_library(EMU_SO)


def route_lm_to_emulation(monkeypatch, ops):
    """The launcher patch of the host tests: ops' Levenberg-Marquardt launches go to the host build."""
    lib = emu_library()
    monkeypatch.setattr(ops, "_launch_lm", lambda name, device, *a: lib.call(name, *a, None))
    monkeypatch.setattr(ops, "_query_lm", lambda name, *a: lib.query(name, *a))


# ------------------------------------------------------------------------------------------------ sums
def pair_table():
    """(44, 2): sum k is sum_n u_n[p] u_n[q] of u = (j0 .. j5, x, f, 1) (include/diffdrr_lm_hip.h's order)."""
    pairs = [(p, q) for p in range(6) for q in range(p, 6)]
    pairs += [(p, 8) for p in range(6)] + [(6, p) for p in range(6)] + [(7, p) for p in range(6)]
    pairs += [(6, 8), (7, 8), (6, 6), (7, 7), (6, 7)]
    return np.array(pairs)


def sums_of(J, x, f):
    """The 44 sums (B, 44) and their scales from J (B, N, 6), x (B, N), f (B, N), in float64."""
    J, x, f = (np.asarray(t, dtype=np.float64) for t in (J, x, f))
    u = np.concatenate([J, x[..., None], f[..., None], np.ones_like(x)[..., None]], axis=-1)  # (B, N, 9)
    pq = pair_table()
    S = np.einsum("bnk,bnk->bk", u[:, :, pq[:, 0]], u[:, :, pq[:, 1]])
    sq = np.einsum("bnk,bnk->bk", u, u)
    return S, np.sqrt(sq[:, pq[:, 0]] * sq[:, pq[:, 1]])


@functools.lru_cache(maxsize=None)
def sum_scene(name):
    """The CPU side of a case: module, poses, fixed image (seeded; shared by every test of the case)."""
    (H, W), delx, B, conv, stop = SUM_CASES[name]
    g = torch.Generator().manual_seed(5 + len(name))
    drr = DRR(synthetic_subject(40, kind="phantom", seed=3), sdd=600.0, height=H, width=W, delx=delx,
              stop_gradients_through_grid_sample=stop)
    rot = (torch.rand(B, 3, generator=g) - 0.5) * 0.6
    xyz = torch.tensor([0.0, 400.0, 0.0]) + (torch.rand(B, 3, generator=g) - 0.5) * 20
    return drr, rot, xyz, conv


def render_record(drr, rot, xyz, conv, ops):
    """The first two launches of a step at (rot, xyz): everything ddrr_lm_normal_sums reads."""
    from diffdrr_amd.pose import _AXIS

    det = drr.detector
    P = drr._calibrated_points()
    Ainv = drr._affine_inverse[0, :3, :] if drr._affine_inverse.dim() == 3 else drr._affine_inverse[:3, :]
    cfg = drr.renderer._cfg(False, det=(det.height, det.width))
    axes = tuple(_AXIS[c] for c in conv)
    reorient34 = det._reorient[:3, :].contiguous()
    B, N = rot.shape[0], P.shape[0]
    aux = ops.brick_record_buffer(B, N, rot.device)
    launch_ws = ops.launch_workspace(drr.density.shape, drr.density.device)
    Mw, source, target, img = ops.pose_raygen_forward(rot, xyz, axes, reorient34, Ainv, P, clear=aux,
                                                      clear_launch_ws=launch_ws)
    ops.siddon_forward_bricks(drr.density, source, target, img, cfg["det"], voxel_shift=cfg["voxel_shift"],
                              eps=cfg["eps"], want_aux=True, storage="f32", want_image=False, aux=aux,
                              launch_ws=launch_ws, cleared=True)
    x32 = img * ops.record_planes(aux, B, N)[0]
    args = dict(source=source, Mw=Mw, Ainv=Ainv, P=P, rot=rot, xyz=xyz, axes=axes, reorient34=reorient34)
    return aux, args, dict(eps=cfg["eps"], with_img_path=not cfg["stop_gradients"]), x32


def float64_jacobian(drr, rot, xyz, conv):
    """x (B, N) and J (B, N, 6) from the package's float64 render route, one-hot autograd.grad per pixel (the
    poses are independent: one call serves the pixel of every pose)."""
    d64 = copy.deepcopy(drr).to(torch.float64)
    r = rot.double().clone().requires_grad_()
    t = xyz.double().clone().requires_grad_()
    img = d64(r, t, parameterization="euler_angles", convention=conv)
    B = r.shape[0]
    flat = img.reshape(B, -1)
    N = flat.shape[1]
    J = torch.zeros(B, N, 6, dtype=torch.float64)
    hot = torch.zeros_like(flat)
    for n in range(N):
        hot[:, n] = 1.0
        g_r, g_t = torch.autograd.grad(flat, (r, t), grad_outputs=hot, retain_graph=True)
        hot[:, n] = 0.0
        J[:, n, :3], J[:, n, 3:] = g_r.cpu(), g_t.cpu()
    return flat.detach().cpu().numpy(), J.numpy()


def float32_route_jacobian(aux, args, kw, ops):
    """J (B, N, 6) from one-hot calls of the existing float32 entry, ddrr_siddon_backward_pose_euler."""
    B, N = args["rot"].shape[0], args["P"].shape[0]
    J = torch.zeros(B, N, 6, dtype=torch.float32)
    hot = torch.zeros(B, N, dtype=torch.float32, device=args["rot"].device)
    for n in range(N):
        hot[:, n] = 1.0
        g_r, g_t = ops.siddon_backward_pose_euler(aux, hot, **args, **kw)
        hot[:, n] = 0.0
        J[:, n, :3], J[:, n, 3:] = g_r.cpu(), g_t.cpu()
    return J.numpy()


_yardsticks = {}


def check_sums_and_jacobian(name, device, ops):
    """One case of SUM_CASES on `device` through `ops`: the 44 sums, the per-ray Jacobian and sum_n w_n j_n
    against float64, gated by the float32 route's own error; a shared fixed image against per-pose copies;
    two calls bit for bit."""
    drr_cpu, rot, xyz, conv = sum_scene(name)
    drr = copy.deepcopy(drr_cpu).to(device)
    rot, xyz = rot.to(device), xyz.to(device)
    B = rot.shape[0]
    with torch.no_grad():
        fixed = drr(rot[:1] * 0, torch.tensor([[0.0, 400.0, 0.0]], device=device), parameterization="euler_angles",
                    convention=conv).reshape(1, -1).contiguous()
    aux, args, kw, x32 = render_record(drr, rot, xyz, conv, ops)
    N = fixed.shape[1]
    key = (name, str(device))
    if key not in _yardsticks:  # (computed once per case and device, never modified)
        x64, J64 = float64_jacobian(drr, rot, xyz, conv)
        J32 = float32_route_jacobian(aux, args, kw, ops)
        _yardsticks[key] = (x64, J64, J32)
    x64, J64, J32 = _yardsticks[key]
    f = fixed.cpu().numpy().astype(np.float64).repeat(B, axis=0)

    ws, jac = ops.lm_normal_sums(aux, fixed, **args, **kw, want_jacobian=True)
    assert ws.shape == (B, -(-N // _lib.LM_GROUP_RAYS), _lib.LM_SUMS) and jac.shape == (B, N, 6)
    got = ws.sum(1).cpu().numpy()
    jac = jac.cpu().numpy().astype(np.float64)
    truth, scale = sums_of(J64, x64, f)
    route, _ = sums_of(J32, x32.cpu().numpy(), f)
    err, own = np.abs(got - truth), np.abs(route - truth)
    print(f"{name}: sums, worst (kernel error - 2 x float32 route's) / scale = {((err - 2 * own) / scale).max():.2e}; "
          f"kernel error / scale max {(err / scale).max():.2e}, float32 route's {(own / scale).max():.2e}")
    assert (err <= 2 * own + FLOOR * scale).all(), np.argwhere(err > 2 * own + FLOOR * scale)

    # the Jacobian itself, per entry, scaled by its column's largest entry of the pose
    jscale = np.abs(J64).max(axis=1, keepdims=True)
    jerr, jown = np.abs(jac - J64), np.abs(J32 - J64)
    print(f"{name}: jacobian, kernel error / column max {(jerr / jscale).max():.2e}, float32 route's "
          f"{(jown / jscale).max():.2e}")
    assert (jerr <= 2 * jown + FLOOR * jscale).all(), float(((jerr - 2 * jown) / jscale).max())
    # (a row is computed by the operations of the existing entry on a one-hot gradient: the same bits where
    # the compiler contracts nothing differently -- always on the host build)
    print(f"{name}: jacobian rows equal to the one-hot calls of the existing entry bit for bit: "
          f"{np.array_equal(jac, J32.astype(np.float64))}")
    if device.type == "cpu":
        assert np.array_equal(jac, J32.astype(np.float64))

    # sum_n w_n j_n against the existing backward entry with grad_out = w
    w = torch.randn(B, N, generator=torch.Generator().manual_seed(11)).to(device)
    g_r, g_t = ops.siddon_backward_pose_euler(aux, w, **args, **kw)
    w64 = w.cpu().numpy().astype(np.float64)
    want = np.einsum("bn,bnk->bk", w64, J64)
    entry = np.concatenate([g_r.cpu().numpy(), g_t.cpu().numpy()], axis=1).astype(np.float64)
    mine = np.einsum("bn,bnk->bk", w64, jac)
    wscale = np.sqrt((w64 ** 2).sum(1, keepdims=True) * (J64 ** 2).sum(1))
    werr, wown = np.abs(mine - want), np.abs(entry - want)
    print(f"{name}: sum w j, kernel error / scale {(werr / wscale).max():.2e}, existing entry's "
          f"{(wown / wscale).max():.2e}")
    assert (werr <= 2 * wown + FLOOR * wscale).all()

    # per-pose copies of the fixed image: the same bits; a second call: the same bits
    ws_b, jac_b = ops.lm_normal_sums(aux, fixed.expand(B, -1).contiguous(), **args, **kw, want_jacobian=True)
    assert torch.equal(ws_b, ws) and np.array_equal(jac_b.cpu().numpy().astype(np.float64), jac)
    ws_c, _ = ops.lm_normal_sums(aux, fixed, **args, **kw)
    assert torch.equal(ws_c, ws)


# ------------------------------------------------------------------------------------------------ step
HYPER = dict(ncc_eps=1e-5, up=4.0, down=1.0 / 3.0, damping_min=1e-7, damping_max=1e6)


def synthetic_pair(seed, N, closeness):
    """J (N, 6), x, f (N,) in float64: a smooth-ish image pair, x = f + closeness * noise."""
    g = np.random.default_rng(seed)
    f = g.random(N) * 3.0 + 1.0
    x = f + closeness * g.standard_normal(N)
    J = g.standard_normal((N, 6)) * np.array([40.0, 30.0, 50.0, 0.5, 0.1, 0.7]) + np.array([3.0, -2.0, 1.0, 0.1, 0.0, 0.05])
    return J, x, f


def partials_of(J, x, f, device):
    """(G, 44) per-workgroup partial sums as ddrr_lm_normal_sums would lay them out, from float64 data."""
    N = x.shape[0]
    rows = [sums_of(J[None, a:a + _lib.LM_GROUP_RAYS], x[None, a:a + _lib.LM_GROUP_RAYS],
                    f[None, a:a + _lib.LM_GROUP_RAYS])[0][0] for a in range(0, N, _lib.LM_GROUP_RAYS)]
    return torch.tensor(np.stack(rows), dtype=torch.float64, device=device)


def reference_update(ref, theta, J, x, f, hyper):
    """The float64 restatement of ddrr_lm_step for one pose.  `ref`: dict(best, ncc, A, g, lam, valid);
    `theta` the rendered pose (6 float32 values as float64) -> the next trial pose (float64, unrounded)."""
    ncc, A, g = (t.numpy() for t in normal_equations_reference(torch.tensor(J), torch.tensor(x), torch.tensor(f),
                                                               hyper["ncc_eps"]))
    if not ref["valid"] or ncc > ref["ncc"]:
        ref.update(best=theta.copy(), ncc=float(ncc), A=A, g=g, valid=True, accepted=True)
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
    return ref["best"] + delta


def ulps32(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def check_step_sequences(device, ops):
    """ddrr_lm_step against normal_equations_reference + reference_update over sequences of fed sums: first
    call, accept, reject, both clamps, a failed factorisation, three poses with mixed outcomes."""
    N = 1500  # two workgroups' partials
    start = np.array([0.08, -0.06, 0.07, 6.0, 391.0, 5.0], dtype=np.float32)

    def run(feeds, hyper, B=1, lam0=1.0):
        """feeds: per call, per pose (seed, closeness) | "flat" (H = 0: the factorisation fails)"""
        state = ops.lm_state(B, lam0, device)
        rot = torch.tensor(np.tile(start[:3], (B, 1)), device=device)
        xyz = torch.tensor(np.tile(start[3:], (B, 1)), device=device)
        refs = [dict(valid=False, lam=lam0, ncc=0.0) for _ in range(B)]
        trace = []
        for call in feeds:
            theta = torch.cat([rot, xyz], 1).cpu().numpy().astype(np.float64)
            parts, want = [], []
            for b, feed in enumerate(call):
                if feed == "flat":
                    J, x, f = synthetic_pair(99, N, 0.5)
                    p = partials_of(J, x, f, device)
                    p[:, :21] = 0.0  # H = 0 with a, c, d as they are: A is negative semi-definite
                    want.append(None)
                else:
                    J, x, f = synthetic_pair(feed[0], N, feed[1])
                    p = partials_of(J, x, f, device)
                    want.append(reference_update(refs[b], theta[b], J, x, f, hyper))
                parts.append(p)
            ws = torch.stack(parts).contiguous()
            lam_before = state[:, 34].cpu().numpy().copy()
            valid_before = state[:, 35].cpu().numpy().copy()
            ncc = ops.lm_step(ws, state, rot, xyz, N, **hyper)
            got = torch.cat([rot, xyz], 1).cpu().numpy()
            st = state.cpu().numpy()
            for b, feed in enumerate(call):
                if feed == "flat":
                    # delta = 0: the next trial is the best pose itself; lambda: the accept / reject move, then up
                    assert np.array_equal(got[b], st[b, :6].astype(np.float32)), (got[b], st[b, :6])
                    moved = max(lam_before[b] * hyper["down"], hyper["damping_min"]) if not valid_before[b] or \
                        st[b, 36] else min(lam_before[b] * hyper["up"], hyper["damping_max"])
                    assert st[b, 34] == min(moved * hyper["up"], hyper["damping_max"]), (st[b, 34], moved)
                    if refs[b]["valid"] is False and st[b, 36]:
                        refs[b].update(valid=True, best=theta[b].copy(), ncc=st[b, 6], A=None, g=None)
                    refs[b]["lam"] = st[b, 34]
                    continue
                u = ulps32(got[b], want[b])
                assert (u <= 2).all(), (b, feed, got[b], want[b], u)
                assert st[b, 34] == refs[b]["lam"], (b, feed, st[b, 34], refs[b]["lam"])  # exactly
                assert bool(st[b, 36]) == refs[b]["accepted"] and st[b, 35] == 1.0
                assert abs(st[b, 6] - refs[b]["ncc"]) <= 1e-12 and float(ncc[b]) == np.float32(st[b, 6])
            trace.append((st[:, 34].copy(), st[:, 36].copy()))
        return trace

    # first call (accept), a closer image (accept), a worse one (reject), closer again
    t = run([[(1, 0.8)], [(2, 0.3)], [(3, 0.6)], [(4, 0.1)]], HYPER)
    assert [bool(a[0]) for _, a in t] == [True, True, False, True]
    d = HYPER["down"]
    assert [lam[0] for lam, _ in t] == [d, d * d, d * d * 4.0, d * d * 4.0 * d]
    # both clamps
    clamp = dict(HYPER, damping_min=0.2, damping_max=1.5)
    t = run([[(1, 0.8)], [(2, 0.3)], [(3, 0.6)], [(5, 0.7)], [(6, 0.9)]], clamp)
    assert [lam[0] for lam, _ in t] == [1 / 3, 0.2, 0.8, 1.5, 1.5]
    # H = 0: the factorisation fails on the first pivot, as a first call and after a valid pose
    run([["flat"], [(2, 0.3)]], HYPER)
    t = run([[(1, 0.8)], ["flat"]], HYPER)
    # three poses, mixed outcomes per call
    t = run([[(1, 0.8), (2, 0.3), "flat"], [(2, 0.3), (1, 0.8), (3, 0.2)], [(3, 0.6), (4, 0.1), (4, 0.1)]], HYPER, B=3)
    assert [list(a.astype(bool)) for _, a in t][1][:2] == [True, False]


# ------------------------------------------------------------------------------------------------ convergence
TRUTH = (torch.zeros(1, 3), torch.tensor([[0.0, 400.0, 0.0]]))
OFFSET = (torch.tensor([[0.08, -0.06, 0.07]]), torch.tensor([[6.0, -9.0, 5.0]]))


def convergence_scene(device):
    drr = DRR(synthetic_subject(64, kind="phantom", seed=3), sdd=600.0, height=48, width=48, delx=2.5).to(device)
    with torch.no_grad():
        fixed = drr(TRUTH[0].to(device), TRUTH[1].to(device), parameterization="euler_angles", convention="ZXY")
    return drr, fixed


def _reached(ncc, rot, xyz):
    return (ncc >= 0.9999 and float((rot.cpu() - TRUTH[0]).abs().max()) <= 0.01
            and float((xyz.cpu() - TRUTH[1]).abs().max()) <= 0.5)


def check_convergence(device):
    """LM reaches NCC >= 0.9999 within 0.01 rad / 0.5 mm inside 60 renders, in at most half the iterations
    the reference's Adam loop (1e-1 / 5e0, maximize, capped at 400) needs on the same scene."""
    drr, fixed = convergence_scene(device)
    start = [(TRUTH[k] + OFFSET[k]).to(device) for k in (0, 1)]
    reg = Registration(drr, start[0].clone(), start[1].clone(), parameterization="euler_angles", convention="ZXY")
    lm = LevenbergMarquardt(reg, fixed)
    lm_renders = None
    for it in range(1, 61):  # the hard cap: a stall fails
        ncc = float(lm.step()[0])
        if _reached(ncc, *lm.best_parameters):
            lm_renders = it
            break
    assert lm_renders is not None, f"LM: NCC {ncc} after 60 renders"
    lm.commit()
    assert _reached(ncc, reg.rotation.detach(), reg.translation.detach())

    reg = Registration(drr, start[0].clone(), start[1].clone(), parameterization="euler_angles", convention="ZXY")
    opt = torch.optim.Adam([{"params": [reg._rotation], "lr": 1e-1}, {"params": [reg._translation], "lr": 5e0}],
                           maximize=True)
    adam_iterations = 400
    for it in range(1, 401):
        opt.zero_grad()
        value = drr.ncc(fixed, reg._rotation, reg._translation, convention="ZXY")
        if _reached(float(value.detach()), reg.rotation.detach(), reg.translation.detach()):
            adam_iterations = it
            break
        value.sum().backward()
        opt.step()
    print(f"renders to NCC >= 0.9999 within 0.01 rad / 0.5 mm: LM {lm_renders}, Adam {adam_iterations} (cap 400)")
    assert 2 * lm_renders <= adam_iterations, (lm_renders, adam_iterations)
