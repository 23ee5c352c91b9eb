"""What tests/test_wlm.py (host emulation) and tests/test_gpu_wlm.py (MI355X) share: the host build of
csrc/wlm_core.h (tests/emu/wlm_emu.cpp), the weight patterns, the float64 yardsticks of the weighted
Levenberg-Marquardt kernels (include/diffdrr_wlm_hip.h) and the checks, written once as ``check_*(device, ops)``.

The scenes, the float64 and float32 Jacobian routes, the gate of the sums (|kernel - truth| <= 2 |float32 route -
truth| + FLOOR x the Cauchy-Schwarz scale of the sum, FLOOR = 1e-6), the step's measure (``ulps32`` <= 2) and the
convergence target are tests/lm_cases.py's; the occluded scene and the pose error ``_q`` are tests/wncc_cases.py's.
The weight enters both yardsticks of a sum the same way: sum_n w_n u_p u_q over the rays with w_n != 0, scale
sqrt(sum w u_p^2 sum w u_q^2)."""
import contextlib
import copy
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import lm_cases
import wncc_cases
from conftest import ROOT
from diffdrr_amd import LevenbergMarquardt, Registration, _lib
from diffdrr_amd.registration import normal_equations_reference, weighted_normal_equations_reference
from lm_cases import FLOOR, HYPER, OFFSET, TRUTH, float32_route_jacobian, float64_jacobian, render_record, sum_scene
from wncc_cases import _q, occluded_scene

EMU_SRC = os.path.join(ROOT, "tests", "emu", "wlm_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "_build", "libwlm_emu.so")
SUM_NAMES = ("6_rays", "780_rays_zxy", "780_rays_zyx_stop", "4087_rays_four_workgroups")
GROUP = _lib.WLM_GROUP_RAYS


@functools.lru_cache(maxsize=None)
def emu_library():
    """The host build of the two entries (tests/emu/wlm_emu.cpp), bound through the product's own binding."""
    csrc = os.path.join(ROOT, "diffdrr_amd", "csrc")
    deps = [EMU_SRC, lm_cases.EMU_LOOPS]
    deps += [os.path.join(ROOT, "include", f) for f in ("diffdrr_wlm_hip.h", "diffdrr_lm_hip.h")]
    deps += [os.path.join(csrc, f) for f in ("wlm_core.h", "lm_core.h", "siddon_core.h", "raygen_core.h",
                                             "record_layout.h", "ddrr_common.h")]
    if not (os.path.exists(EMU_SO) and all(os.path.getmtime(d) <= os.path.getmtime(EMU_SO) for d in deps)):
        os.makedirs(os.path.dirname(EMU_SO), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-mfma", "-ffp-contract=off",
                        "-Wno-unknown-pragmas", EMU_SRC, "-o", EMU_SO], check=True)
    return _lib.wlm_library(EMU_SO)


def route_wlm_to_emulation(monkeypatch, ops):
    """The launcher patch of the host tests: ops' weighted Levenberg-Marquardt launches go to the host build."""
    lib = emu_library()
    monkeypatch.setattr(ops, "_launch_wlm", lambda name, device, *a: lib.call(name, *a, None))
    monkeypatch.setattr(ops, "_query_wlm", lambda name, *a: lib.query(name, *a))


@contextlib.contextmanager
def launches(ops):
    """the names of the C-ABI entries launched inside the block: the main library's and both LM libraries'"""
    names, real = [], {k: getattr(ops, k) for k in ("_launch", "_launch_lm", "_launch_wlm")}
    for k, fn in real.items():
        setattr(ops, k, lambda name, device, *a, _fn=fn: (names.append(name), _fn(name, device, *a))[1])
    try:
        yield names
    finally:
        for k, fn in real.items():
            setattr(ops, k, fn)


# ------------------------------------------------------------------------------------------------ weights
PATTERNS = ("ones", "disc", "smooth", "half", "one pose empty", "workgroup 1 empty")


def weights(pattern, B, H, W, per_pose, device):
    """((B | 1), N) float32 weights; None where the pattern does not apply.  The first five are
    wncc_cases.weights'; `workgroup 1 empty`: smooth weights with every ray of workgroup 1 at 0 (more than one
    workgroup needed)."""
    if pattern != "workgroup 1 empty":
        return wncc_cases.weights(pattern, B, H, W, per_pose, device)
    if H * W <= 2 * GROUP:
        return None
    w = wncc_cases.weights("smooth", B, H, W, per_pose, torch.device("cpu")).clone()
    w[:, GROUP:2 * GROUP] = 0.0
    return w.to(device).contiguous()


def all_weights(B, H, W, device, patterns=PATTERNS):
    out = []
    for pattern in patterns:
        for per_pose in (False, True):
            w = weights(pattern, B, H, W, per_pose, device)
            if w is not None:
                out.append((f"{pattern} {'per pose' if per_pose else 'shared'}", w))
    return out


def poison(t, w):
    """`t` with NaN, +Inf and -Inf (in turn) wherever w == 0"""
    bad = torch.tensor([float("nan"), float("inf"), -float("inf")], device=t.device)[
        torch.arange(t.shape[-1], device=t.device) % 3]
    return torch.where(w.expand_as(t) == 0, bad.expand_as(t), t).contiguous()


# ------------------------------------------------------------------------------------------------ sums
def pair_table():
    """(45, 2): lm_cases.pair_table and (8, 8) for sum w (include/diffdrr_wlm_hip.h's order)"""
    return np.concatenate([lm_cases.pair_table(), [[8, 8]]])


def rows_of(J, x, f, w):
    """u (B, N, 9) = (j, x, f, 1) in float64 with the rays of weight 0 selected out (rows of zeros), and w (B, N)"""
    J, x, f, w = (np.asarray(t, dtype=np.float64) for t in (J, x, f, w))
    w = np.broadcast_to(w, x.shape)
    u = np.concatenate([J, x[..., None], np.broadcast_to(f, x.shape)[..., None], np.ones_like(x)[..., None]], axis=-1)
    return np.where((w != 0)[..., None], u, 0.0), w


def wsums_of(J, x, f, w):
    """The 45 weighted sums (B, 45) and their weighted Cauchy-Schwarz scales, in float64."""
    u, w = rows_of(J, x, f, w)
    pq = pair_table()
    S = np.einsum("bn,bnk,bnk->bk", w, u[:, :, pq[:, 0]], u[:, :, pq[:, 1]])
    sq = np.einsum("bn,bnk,bnk->bk", w, u, u)
    return S, np.sqrt(sq[:, pq[:, 0]] * sq[:, pq[:, 1]])


def partials_in_kernel_order(u, w):
    """(B, G, 45) from rows u (B, N, 9) and weights w (B, N), float64 torch on the CPU: per workgroup five
    interleaved slices, each w (u_p u_q) added in ascending ray order, then the slices in ascending order."""
    pq = torch.tensor(pair_table())
    B, N = w.shape
    G = -(-N // GROUP)
    want = torch.zeros(B, G, 45, dtype=torch.float64)
    for b in range(B):
        for g in range(G):
            rows, wt = u[b, g * GROUP:(g + 1) * GROUP], w[b, g * GROUP:(g + 1) * GROUP]
            prod = wt[:, None] * (rows[:, pq[:, 0]] * rows[:, pq[:, 1]])  # inner product exact, then one rounding
            total = None
            for s in range(5):
                acc = torch.zeros(45, dtype=torch.float64)
                for row in prod[s::5]:
                    acc = acc + row
                total = acc if total is None else total + acc
            want[b, g] = total
    return want


_scenes = {}


def scene(name, device, ops):
    """One case of lm_cases.SUM_CASES on `device`: module, poses, ONE record, the fixed images, and the yardsticks
    of that record (computed once per case and device, never modified)."""
    key = (name, str(device))
    if key not in _scenes:
        drr_cpu, rot, xyz, conv = sum_scene(name)
        drr = copy.deepcopy(drr_cpu).to(device)
        rot, xyz = rot.to(device), xyz.to(device)
        with torch.no_grad():
            fixed = drr(rot[:1] * 0, torch.tensor([[0.0, 400.0, 0.0]], device=device),
                        parameterization="euler_angles", convention=conv).reshape(1, -1).contiguous()
        aux, args, kw, x32 = render_record(drr, rot, xyz, conv, ops)
        x64, J64 = float64_jacobian(drr, rot, xyz, conv)
        J32 = float32_route_jacobian(aux, args, kw, ops)
        H, W = lm_cases.SUM_CASES[name][0]
        _scenes[key] = dict(B=rot.shape[0], N=fixed.shape[1], H=H, W=W, fixed=fixed, aux=aux, args=args, kw=kw,
                            x32=x32, x64=x64, J64=J64, J32=J32)
    return _scenes[key]


def _sums(sc, ops, fixed, w, **more):
    return ops.wlm_normal_sums(sc["aux"], fixed, w, **sc["args"], **sc["kw"], **more)


def check_sums_and_jacobian(name, device, ops):
    """The 45 sums under every weight pattern, shared and per pose, and the per-ray Jacobian against float64,
    gated by the float32 route's own error with the weights in both yardsticks."""
    sc = scene(name, device, ops)
    B, N = sc["B"], sc["N"]
    f = sc["fixed"].cpu().numpy().astype(np.float64)
    x32 = sc["x32"].cpu().numpy()
    for label, w in all_weights(B, sc["H"], sc["W"], device):
        ws, jac = _sums(sc, ops, sc["fixed"], w, want_jacobian=True)
        assert ws.shape == (B, -(-N // GROUP), _lib.WLM_SUMS) and jac.shape == (B, N, 6)
        got = ws.sum(1).cpu().numpy()
        wn = w.cpu().numpy()
        truth, scale = wsums_of(sc["J64"], sc["x64"], f, wn)
        route, _ = wsums_of(sc["J32"], x32, f, wn)
        err, own = np.abs(got - truth), np.abs(route - truth)
        safe = np.where(scale > 0, scale, 1.0)
        print(f"{name} {label}: sums, worst (kernel error - 2 x float32 route's) / scale = "
              f"{((err - 2 * own) / safe).max():.2e}; kernel error / scale max {(err / safe).max():.2e}, "
              f"float32 route's {(own / safe).max():.2e}")
        assert np.isfinite(got).all()
        assert (err <= 2 * own + FLOOR * scale).all(), (label, np.argwhere(err > 2 * own + FLOOR * scale))
        # the Jacobian: every ray whatever its weight, under lm_cases' rule
        jac = jac.cpu().numpy().astype(np.float64)
        jscale = np.abs(sc["J64"]).max(axis=1, keepdims=True)
        jerr, jown = np.abs(jac - sc["J64"]), np.abs(sc["J32"] - sc["J64"])
        assert (jerr <= 2 * jown + FLOOR * jscale).all(), (label, float(((jerr - 2 * jown) / jscale).max()))
        if device.type == "cpu":
            assert np.array_equal(jac, sc["J32"].astype(np.float64))
    print(f"{name}: jacobian, kernel error / column max {(jerr / jscale).max():.2e}, float32 route's "
          f"{(jown / jscale).max():.2e}")


def check_bit_for_bit_properties(name, device, ops):
    """w == 1: the sums of the unweighted library and the ray counts (asserted on the host build, printed on the
    device); a shared weight against its per-pose copies; a second call; 4 w and w / 4; a pose emptied of its weights
    leaves its neighbours' sums and steps as they were."""
    sc = scene(name, device, ops)
    B, N = sc["B"], sc["N"]
    ones = torch.ones(1, N, device=device)
    ws1, _ = _sums(sc, ops, sc["fixed"], ones)
    ws0, _ = ops.lm_normal_sums(sc["aux"], sc["fixed"], **sc["args"], **sc["kw"])
    counts = torch.tensor([min(GROUP, N - g * GROUP) for g in range(ws1.shape[1])], dtype=torch.float64, device=device)
    same = torch.equal(ws1[..., :44], ws0)
    print(f"{name}: with w == 1 the 44 sums equal those of ddrr_lm_normal_sums bit for bit: {same}")
    if device.type == "cpu":
        assert same
    assert torch.equal(ws1[..., 44], counts.expand(B, -1))  # (sums of ones: exact in any order)
    assert float(ws1[..., 44].sum(1)[0]) == N
    for label, w in all_weights(B, sc["H"], sc["W"], device):
        ws, jac = _sums(sc, ops, sc["fixed"], w, want_jacobian=True)
        again, _ = _sums(sc, ops, sc["fixed"], w)
        assert torch.equal(ws, again), (label, "second call")
        if w.shape[0] == 1:
            copies, jac_b = _sums(sc, ops, sc["fixed"].expand(B, -1).contiguous(), w.expand(B, -1).contiguous(),
                                  want_jacobian=True)
            assert torch.equal(ws, copies) and torch.equal(jac, jac_b), (label, "per-pose copies")
        for c in (4.0, 0.25):
            scaled, _ = _sums(sc, ops, sc["fixed"], (c * w).contiguous())
            assert torch.equal(scaled, c * ws), (label, c)
        if w.shape[0] == B > 1:  # nothing left of the last pose: its neighbours' sums and steps keep their bits
            emptied = w.clone()
            emptied[-1] = 0.0
            ws_e, _ = _sums(sc, ops, sc["fixed"], emptied)
            assert torch.equal(ws_e[:-1], ws[:-1]) and not bool(ws_e[-1].any()), label
            for a, e in zip(fresh_step(sc, ops, ws, device), fresh_step(sc, ops, ws_e, device)):
                assert torch.equal(a[:-1], e[:-1]), label
                assert bool(torch.isfinite(e).all()), label


def check_device_sums_from_the_devices_own_rows(name, device, ops):
    """From the kernel's own per-ray rows (jac, x, f) and w the host forms w (u_p u_q) in float64 in the header's
    order: the partials must be equal bit for bit (exact products, one rounding by w, additions in a fixed order)."""
    sc = scene(name, device, ops)
    B, N = sc["B"], sc["N"]
    fixed = torch.rand(B, N, generator=torch.Generator().manual_seed(4)).to(device)
    for label, w in all_weights(B, sc["H"], sc["W"], device, ("smooth", "half", "workgroup 1 empty")):
        ws, jac = _sums(sc, ops, fixed, w, want_jacobian=True)
        u, wn = rows_of(jac.cpu().numpy(), sc["x32"].cpu().numpy(), fixed.cpu().numpy(), w.cpu().numpy())
        want = partials_in_kernel_order(torch.tensor(u), torch.tensor(np.ascontiguousarray(wn)))
        assert torch.equal(ws.cpu(), want), (label, float((ws.cpu() - want).abs().max()))
        if label.startswith("workgroup 1 empty"):
            assert bool((ws[:, 1] == 0).all())


def fresh_step(sc, ops, ws, device, lam0=1.0):
    """One ddrr_wlm_step from a fresh state on copies of the scene's poses -> (ncc, state, rot, xyz)"""
    state = ops.lm_state(sc["B"], lam0, device)
    rot, xyz = sc["args"]["rot"].clone(), sc["args"]["xyz"].clone()
    ncc = ops.wlm_step(ws, state, rot, xyz, sc["N"], **HYPER)
    return ncc, state, rot, xyz


def check_masked_pixels_are_not_read(name, device, ops):
    """NaN and +-Inf in the fixed image under w == 0 change no bit of the sums or of the step's outputs, and every
    output is finite."""
    sc = scene(name, device, ops)
    B, N = sc["B"], sc["N"]
    done = 0
    for label, w in all_weights(B, sc["H"], sc["W"], device, ("disc", "half", "one pose empty", "workgroup 1 empty")):
        if not bool((w == 0).any()):
            continue
        clean = sc["fixed"] if w.shape[0] == 1 else sc["fixed"].expand(B, -1).contiguous()
        dirty = poison(clean, w)
        assert not bool(torch.isfinite(dirty).all())
        runs = []
        for fixed in (clean, dirty):
            ws, _ = _sums(sc, ops, fixed, w)
            runs.append((ws, *fresh_step(sc, ops, ws, device)))
        for k, (a, b) in enumerate(zip(*runs)):
            assert torch.equal(a, b), (name, label, k)
            assert bool(torch.isfinite(b).all()), (name, label, k)
        done += 1
    assert done or name == "6_rays"


def check_power_of_four_scaling(name, device, ops):
    """4 w: A and g are 4 times as large, exactly; the Cholesky square roots stay exact and DDRR_LM_TINY is absorbed
    in the pivots, so the next trial parameters are expected bit for bit.  Asserted: <= 1 float32 ulp."""
    sc = scene(name, device, ops)
    for label, w in all_weights(sc["B"], sc["H"], sc["W"], device, ("smooth", "half")):
        outs = []
        for c in (1.0, 4.0):
            ws, _ = _sums(sc, ops, sc["fixed"], (c * w).contiguous())
            outs.append(fresh_step(sc, ops, ws, device))
        (n1, s1, r1, x1), (n4, s4, r4, x4) = outs
        equal = torch.equal(r1, r4) and torch.equal(x1, x4)
        print(f"{name} {label}: the next trial under 4 w equals the one under w bit for bit: {equal}")
        u = lm_cases.ulps32(torch.cat([r1, x1], 1).cpu().numpy(), torch.cat([r4, x4], 1).cpu().numpy())
        assert (u <= 1).all(), (label, u)
        assert torch.equal(4 * s1[:, 37], s4[:, 37]) and torch.equal(n1, n4)
        assert not torch.equal(r1, sc["args"]["rot"])  # (the step moved the poses)


# ------------------------------------------------------------------------------------------------ step
def synthetic_weights(seed, N):
    """w (N,) in float64 holding float32 values: smooth positive, a third of the pixels at 0"""
    g = np.random.default_rng(1000 + seed)
    w = (0.25 + 1.5 * g.random(N)).astype(np.float32).astype(np.float64)
    w[g.random(N) < 1.0 / 3.0] = 0.0
    return w


def partials_of(J, x, f, w, device):
    """(G, 45) per-workgroup partial sums as ddrr_wlm_normal_sums would lay them out, from float64 data."""
    rows = [wsums_of(J[None, a:a + GROUP], x[None, a:a + GROUP], f[None, a:a + GROUP], w[None, a:a + GROUP])[0][0]
            for a in range(0, x.shape[0], GROUP)]
    return torch.tensor(np.stack(rows), dtype=torch.float64, device=device)


def reference_update(ref, theta, J, x, f, w, hyper):
    """lm_cases.reference_update on weighted_normal_equations_reference: the float64 restatement of ddrr_wlm_step."""
    ncc, A, g, Sw = (t.numpy() for t in weighted_normal_equations_reference(
        torch.tensor(J), torch.tensor(x), torch.tensor(f), torch.tensor(w), hyper["ncc_eps"]))
    ref["Sw"] = float(Sw)
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


def check_step_sequences(device, ops):
    """ddrr_wlm_step against weighted_normal_equations_reference + reference_update over sequences of fed sums, as
    lm_cases.check_step_sequences: first call, accept, reject, both clamps, a failed factorisation, an empty pose,
    three poses with mixed outcomes.  Its measure (ulps32) and its bound (2)."""
    N = 1500  # two workgroups' partials
    start = np.array([0.08, -0.06, 0.07, 6.0, 391.0, 5.0], dtype=np.float32)

    def run(feeds, hyper, B=1, lam0=1.0):
        """feeds: per call, per pose (seed, closeness) | "flat" (H = 0: the factorisation fails) | "empty" (w = 0)"""
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
                    J, x, f = lm_cases.synthetic_pair(99, N, 0.5)
                    p = partials_of(J, x, f, synthetic_weights(99, N), device)
                    p[:, :21] = 0.0  # H = 0 with a, c, d as they are: A is negative semi-definite
                    want.append(None)
                else:
                    seed, closeness = (7, 0.5) if feed == "empty" else feed
                    J, x, f = lm_cases.synthetic_pair(seed, N, closeness)
                    w = np.zeros(N) if feed == "empty" else synthetic_weights(seed, N)
                    p = partials_of(J, x, f, w, device)
                    want.append(reference_update(refs[b], theta[b], J, x, f, w, hyper))
                parts.append(p)
            ws = torch.stack(parts).contiguous()
            lam_before = state[:, 34].cpu().numpy().copy()
            valid_before = state[:, 35].cpu().numpy().copy()
            ncc = ops.wlm_step(ws, state, rot, xyz, N, **hyper)
            got = torch.cat([rot, xyz], 1).cpu().numpy()
            st = state.cpu().numpy()
            assert np.isfinite(st).all() and np.isfinite(got).all()
            for b, feed in enumerate(call):
                if feed == "flat":
                    assert np.array_equal(got[b], st[b, :6].astype(np.float32)), (got[b], st[b, :6])
                    moved = max(lam_before[b] * hyper["down"], hyper["damping_min"]) if not valid_before[b] or \
                        st[b, 36] else min(lam_before[b] * hyper["up"], hyper["damping_max"])
                    assert st[b, 34] == min(moved * hyper["up"], hyper["damping_max"]), (st[b, 34], moved)
                    if refs[b]["valid"] is False and st[b, 36]:
                        refs[b].update(valid=True, best=theta[b].copy(), ncc=st[b, 6], A=None, g=None)
                    refs[b]["lam"] = st[b, 34]
                    continue
                u = lm_cases.ulps32(got[b], want[b])
                assert (u <= 2).all(), (b, feed, got[b], want[b], u)
                assert st[b, 34] == refs[b]["lam"], (b, feed, st[b, 34], refs[b]["lam"])  # exactly
                assert bool(st[b, 36]) == refs[b]["accepted"] and st[b, 35] == 1.0
                assert abs(st[b, 6] - refs[b]["ncc"]) <= 1e-12 and float(ncc[b]) == np.float32(st[b, 6])
                assert abs(st[b, 37] - refs[b]["Sw"]) <= 1e-12 * max(1.0, refs[b]["Sw"])
                if feed == "empty":
                    assert st[b, 37] == 0.0
            trace.append((st[:, 34].copy(), st[:, 36].copy(), got.copy()))
        return trace

    # first call (accept), a closer image (accept), a worse one (reject), closer again
    t = run([[(1, 0.8)], [(2, 0.3)], [(3, 0.6)], [(4, 0.1)]], HYPER)
    assert [bool(a[0]) for _, a, _ in t] == [True, True, False, True]
    d = HYPER["down"]
    assert [lam[0] for lam, _, _ in t] == [d, d * d, d * d * 4.0, d * d * 4.0 * d]
    # both clamps
    clamp = dict(HYPER, damping_min=0.2, damping_max=1.5)
    t = run([[(1, 0.8)], [(2, 0.3)], [(3, 0.6)], [(5, 0.7)], [(6, 0.9)]], clamp)
    assert [lam[0] for lam, _, _ in t] == [1 / 3, 0.2, 0.8, 1.5, 1.5]
    # H = 0: the factorisation fails on the first pivot, as a first call and after a valid pose
    run([["flat"], [(2, 0.3)]], HYPER)
    run([[(1, 0.8)], ["flat"]], HYPER)
    # nothing left of a pose: ncc 0, it stays where it is -- as a first call, again, and after a valid pose
    t = run([["empty"], ["empty"]], HYPER)
    assert all(np.array_equal(got[0], start) for _, _, got in t) and [bool(a[0]) for _, a, _ in t] == [True, False]
    run([[(1, 0.8)], ["empty"], [(2, 0.3)]], HYPER)
    # three poses, mixed outcomes per call
    t = run([[(1, 0.8), (2, 0.3), "flat", "empty"], [(2, 0.3), (1, 0.8), (3, 0.2), (5, 0.4)],
             [(3, 0.6), (4, 0.1), (4, 0.1), "empty"]], HYPER, B=4)
    assert [list(a.astype(bool)) for _, a, _ in t][1][:2] == [True, False]


# ------------------------------------------------------------------------------------------------ the reference
def check_reference():
    """weighted_normal_equations_reference against autograd of r = sqrt(w) (z_w(x(theta)) - z_w(f)) for an x that
    is linear in theta, zero weights (with NaN under them) included; Sw (1 - ncc) = 1/2 |r|^2 up to eps; at w = 1
    the unweighted reference."""
    g = torch.Generator().manual_seed(2)
    N, eps = 50, 1e-5
    J = torch.randn(N, 6, generator=g, dtype=torch.float64)
    x0, f = torch.rand(N, generator=g, dtype=torch.float64), torch.rand(N, generator=g, dtype=torch.float64)
    w = 0.25 + 1.5 * torch.rand(N, generator=g, dtype=torch.float64)
    w[torch.rand(N, generator=g) < 0.3] = 0.0
    assert int((w == 0).sum()) >= 5
    on = w != 0

    def z(v):  # on the selected pixels alone
        mu = (w[on] * v).sum() / w[on].sum()
        return (v - mu) / ((w[on] * (v - mu) ** 2).sum() / w[on].sum() + eps).sqrt()

    def residual(theta):
        return w[on].sqrt() * (z(x0[on] + J[on] @ theta) - z(f[on]))

    theta = torch.zeros(6, dtype=torch.float64)
    Jr = torch.autograd.functional.jacobian(residual, theta)
    nan = torch.full_like(x0, float("nan"))
    ncc, A, grad, Sw = weighted_normal_equations_reference(
        torch.where(on[:, None], J, nan[:, None]), torch.where(on, x0, nan), torch.where(on, f, nan), w, eps)
    assert torch.allclose(A, Jr.T @ Jr, rtol=1e-10, atol=1e-12)
    assert torch.allclose(grad, Jr.T @ residual(theta), rtol=1e-10, atol=1e-12)
    assert float(Sw) == float(w.sum())
    assert abs(float(0.5 * residual(theta).pow(2).sum()) - float(Sw) * (1 - float(ncc))) < 20 * float(Sw) * eps
    # w = 1: the unweighted reference; batched, with an empty pose
    n0, A0, g0 = normal_equations_reference(J, x0, f, eps)
    n1, A1, g1, S1 = weighted_normal_equations_reference(J, x0, f, torch.ones(N), eps)
    assert torch.allclose(A1, A0, rtol=1e-12, atol=1e-14) and torch.allclose(g1, g0, rtol=1e-12, atol=1e-14)
    assert abs(float(n1 - n0)) <= 1e-14 and float(S1) == N
    wb = torch.stack([w, torch.zeros(N, dtype=torch.float64)])
    nb, Ab, gb, Sb = weighted_normal_equations_reference(J.expand(2, N, 6), x0.expand(2, N), f.expand(2, N), wb, eps)
    assert torch.equal(Ab[0], A) and torch.equal(gb[0], grad) and nb.shape == (2,)
    assert float(nb[1]) == 0 and float(Sb[1]) == 0 and not bool(Ab[1].any()) and not bool(gb[1].any())


# ------------------------------------------------------------------------------------------------ registration
def _start(device):
    return [(TRUTH[k] + OFFSET[k]).to(device) for k in (0, 1)]


def lm_run(drr, image, weight, device, renders=60, stop=True):
    """LevenbergMarquardt from TRUTH + OFFSET -> (the trial poses rendered [(rot, xyz)], the best NCC after every
    step, the smallest q of a best pose and its render, the object)"""
    rot, xyz = _start(device)
    reg = Registration(drr, rot.clone(), xyz.clone(), parameterization="euler_angles", convention="ZXY")
    lm = LevenbergMarquardt(reg, image, weight=weight)
    track, nccs, best = [], [], (float("inf"), 0)
    for it in range(1, renders + 1):
        track.append((reg.rotation.detach().clone(), reg.translation.detach().clone()))
        nccs.append(float(lm.step()[0]))
        q = _q(*lm.best_parameters)
        best = min(best, (q, it))
        if stop and nccs[-1] >= 0.9999 and q <= 1.0:
            break
    return track, nccs, best, lm


def check_registration(device, ops):
    """On wncc_cases.occluded_scene from TRUTH + OFFSET: the masked LM on the occluded image reaches a best weighted
    NCC >= 0.9999 within one tolerance (q <= 1) inside 60 renders; the unmasked LM on the occluded image never comes
    closer than q = 5 in 60 renders.  The host build renders reproducibly: the masked trajectories on the clean and
    on the occluded image are equal bit for bit.  On the device (float atomics in the record) both reach the target.
    Beside it, not asserted: the iterations of the masked Adam loop (DRR.ncc(weight=))."""
    drr, fixed, occluded, weight = occluded_scene(device)
    with launches(ops) as names:
        track, nccs, (q, it), lm = lm_run(drr, occluded, weight, device)
    print(f"masked LM on the occluded image: best weighted NCC {nccs[-1]:.6f}, q = {_q(*lm.best_parameters):.3g} "
          f"after {len(track)} renders")
    assert nccs[-1] >= 0.9999 and _q(*lm.best_parameters) <= 1.0, (nccs[-1], q, it)
    assert "ddrr_wlm_step" in names and not any(n.startswith("ddrr_lm_") for n in names)
    assert float(lm.weight_sum[0]) == float(weight.sum())
    lm.commit()
    assert _q(lm.reg.rotation, lm.reg.translation) <= 1.0

    _, plain_nccs, (q_plain, it_plain), _ = lm_run(drr, occluded, None, device, stop=False)
    print(f"unmasked LM on the occluded image: best NCC {plain_nccs[-1]:.4f}, closest approach q = {q_plain:.3g} at "
          f"render {it_plain} of 60")
    assert q_plain >= 5.0, (q_plain, it_plain)

    # (the host build repeats the occluded run render for render; the device run has the 60-render cap of its own)
    on_host = device.type == "cpu"
    clean_track, clean_nccs, _, clean_lm = lm_run(drr, fixed, weight, device, renders=len(track) if on_host else 60,
                                                  stop=not on_host)
    if device.type == "cpu":
        assert len(clean_track) == len(track) and clean_nccs == nccs
        assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(track, clean_track))
    else:
        print(f"masked LM on the clean image: best weighted NCC {clean_nccs[-1]:.6f} after {len(clean_track)} renders")
        assert clean_nccs[-1] >= 0.9999 and _q(*clean_lm.best_parameters) <= 1.0

    _, (q_adam, it_adam) = wncc_cases.adam_loop(
        drr, lambda r, x: drr.ncc(occluded, r, x, convention="ZXY", weight=weight), device, stop_at=1.0)
    print(f"renders to q <= 1 on the occluded image with the mask: LM {len(track)}, Adam (DRR.ncc(weight=), 1e-1 / "
          f"5e0, cap 250) {it_adam} (q = {q_adam:.3g})")


def check_python_surface(device, ops):
    """Which entries a step launches with and without a weight; jacobian() does not depend on the weight; three
    starts with per-pose weights, one of them empty, run as they run alone; the empty pose stays where it is.
    "As alone" is asserted on the host build, as tests/test_lm.py does for the unweighted object: on the device the
    record is summed with float atomics, two renders of one pose differ in their last bits, and six accept / reject
    decisions later two runs of the SAME start need not hold the same damping.  What holds on either device, bit for
    bit, is that a pose's sums and step do not depend on its neighbours' weights: check_bit_for_bit_properties."""
    drr, fixed = lm_cases.convergence_scene(device)
    H = W = 48
    rots = torch.tensor([[0.08, -0.06, 0.07], [-0.05, 0.04, 0.02], [0.03, 0.0, -0.02]], device=device)
    xyzs = torch.tensor([[6.0, 391.0, 5.0], [-4.0, 405.0, 3.0], [2.0, 398.0, -3.0]], device=device)
    w = wncc_cases.weights("disc", 3, H, W, True, device).reshape(3, 1, H, W).clone()
    w[0] *= 0.5 + torch.rand(1, H, W, generator=torch.Generator().manual_seed(3)).to(device)
    w[1] = 0.0

    def build(b=slice(0, 3), weight=w):
        reg = Registration(drr, rots[b].clone(), xyzs[b].clone(), parameterization="euler_angles", convention="ZXY")
        return reg, LevenbergMarquardt(reg, fixed, damping=2.0, weight=None if weight is None else weight[b])

    reg, lm = build()
    reg0, lm0 = build(weight=None)
    assert float(lm.weight_sum.abs().max()) == 0 and lm.weight_sum.shape == (3,)
    with launches(ops) as none:
        J, J0 = lm.jacobian(), lm0.jacobian()
    assert torch.equal(J, J0) or device.type != "cpu"
    assert float((J - J0).abs().max()) <= 1e-4 * float(J0.abs().max())  # (two renders: float atomics on the device)
    assert "ddrr_lm_normal_sums" in none and not any(n.startswith("ddrr_wlm") for n in none)
    assert torch.equal(reg.rotation.detach(), rots)
    with launches(ops) as with_w:
        first = lm.step().clone()
    with launches(ops) as without:
        lm0.step()
    assert with_w[-2:] == ["ddrr_wlm_normal_sums", "ddrr_wlm_step"] and len(with_w) == 4, with_w
    assert without[-2:] == ["ddrr_lm_normal_sums", "ddrr_lm_step"] and len(without) == 4, without
    assert with_w[:2] == without[:2] == ["ddrr_pose_raygen_forward", "ddrr_siddon_forward_bricks"]
    assert not any(n.startswith("ddrr_lm_") for n in with_w)
    assert not any(n.startswith("ddrr_wlm") for n in without)
    assert float(lm0.weight_sum.abs().max()) == 0
    history = [first] + [lm.step().clone() for _ in range(5)]
    assert all((b >= a).all() for a, b in zip(history, history[1:]))
    assert torch.allclose(lm.weight_sum, w.reshape(3, -1).double().sum(1), rtol=1e-12, atol=0)
    assert bool(torch.isfinite(lm.weight_sum).all())
    # the empty pose: where it was, ncc 0, weight_sum 0
    assert float(history[-1][1]) == 0 and float(lm.weight_sum[1]) == 0 and float(lm.best_ncc[1]) == 0
    assert torch.equal(reg.rotation.detach()[1], rots[1]) and torch.equal(reg.translation.detach()[1], xyzs[1])
    assert torch.equal(lm.best_parameters[0][1], rots[1])
    # ... and its neighbours run as they run alone
    for b in (0, 2):
        reg_b, lm_b = build(slice(b, b + 1))
        for _ in range(6):
            last = lm_b.step()
        print(f"start {b} in the batch and alone after six steps: best NCC {float(history[-1][b]):.7f} / "
              f"{float(last[0]):.7f}, damping {float(lm.damping[b]):.3g} / {float(lm_b.damping[0]):.3g}")
        if device.type == "cpu":  # (a render is reproducible on the host build alone: see the docstring)
            assert abs(float(history[-1][b]) - float(last[0])) <= 1e-6
            assert float(lm.damping[b]) == float(lm_b.damping[0])
            assert torch.allclose(reg.rotation.detach()[b], reg_b.rotation.detach()[0], atol=1e-6)
        assert float(last[0]) > float(first[b])  # (they moved, and for the better)
    lm.commit()
    assert torch.equal(reg.rotation.detach(), lm.best_parameters[0])


def check_weight_errors(device, elsewhere):
    """ValueErrors of the constructor name the condition: shape, dtype, device, negative, NaN.  `elsewhere`: a
    device the parameters are not on."""
    drr, fixed = lm_cases.convergence_scene(device)
    ones = torch.ones(1, 1, 48, 48, device=device)

    def build(weight):
        reg = Registration(drr, _start(device)[0].clone(), _start(device)[1].clone(), parameterization="euler_angles",
                           convention="ZXY")
        return LevenbergMarquardt(reg, fixed, weight=weight)

    assert build(ones).weight.shape == (1, 48 * 48)
    bad = ones.clone()
    bad[0, 0, 3, 4] = -1.0
    nan = ones.clone()
    nan[0, 0, 5, 6] = float("nan")
    inf = ones.clone()
    inf[0, 0, 5, 6] = float("inf")
    for weight, what in ((ones[:, :, :40], "shape"), (ones[0], "shape"), (ones.expand(2, -1, -1, -1), "shape"),
                         (ones.double(), "float32"), (ones.numpy() if device.type == "cpu" else 1.0, "float32"),
                         (torch.ones(1, 1, 48, 48, device=elsewhere), "device"), (bad, "negative"), (nan, "finite"),
                         (inf, "finite")):
        with pytest.raises(ValueError, match=what):
            build(weight)


def check_ops_errors(ops):
    """The ops refuse what the entries would misread, without a launch."""
    B, N = 2, 1500
    state = ops.lm_state(B, 1.0, "cpu")
    rot, xyz = torch.zeros(B, 3), torch.zeros(B, 3)
    ws = ops.wlm_workspace(B, N, "cpu")
    assert ws.shape == (B, 2, 45) and ws.dtype == torch.float64
    assert ops.wlm_workspace(0, 100, "cpu").numel() == 0
    with launches(ops) as launched:
        with pytest.raises(ValueError, match="ws"):
            ops.wlm_step(ws[:, :1].contiguous(), state, rot, xyz, N)
        with pytest.raises(ValueError, match="ws"):
            ops.wlm_step(ops.lm_workspace(B, N, "cpu"), state, rot, xyz, N)
        with pytest.raises(ValueError, match="state"):
            ops.wlm_step(ws, state.float(), rot, xyz, N)
        with pytest.raises(ValueError, match="pose parameters"):
            ops.wlm_step(ws, state, rot.double(), xyz, N)
        with pytest.raises(ValueError, match="up > 1"):
            ops.wlm_step(ws, state, rot, xyz, N, down=1.5)
        pose = dict(source=torch.zeros(B, 1, 3), Mw=torch.zeros(B, 3, 4), Ainv=torch.zeros(3, 4), P=torch.zeros(N, 3),
                    rot=rot, xyz=xyz, axes=(2, 0, 1), reorient34=torch.zeros(3, 4))
        aux, x1, w = ops.brick_record_buffer(B, N, "cpu"), torch.ones(1, N), torch.ones(1, N)
        for bad in (torch.ones(N), torch.ones(1, N + 1), torch.ones(3, N), torch.ones(1, 1, N),
                    torch.ones(1, N).double()):
            with pytest.raises(ValueError, match="fixed"):
                ops.wlm_normal_sums(aux, bad, w, **pose)
            with pytest.raises(ValueError, match="weight"):
                ops.wlm_normal_sums(aux, x1, bad, **pose)
        with pytest.raises(ValueError, match="weight"):
            ops.wlm_normal_sums(aux, x1, None, **pose)
        with pytest.raises(ValueError, match="device"):
            ops.wlm_normal_sums(aux, x1, torch.ones(1, N, device="meta"), **pose)
        with pytest.raises(ValueError, match="ws"):
            ops.wlm_normal_sums(aux, x1, w, **pose, ws=ops.lm_workspace(B, N, "cpu"))
        out = ops.wlm_step(ops.wlm_workspace(0, 100, "cpu"), ops.lm_state(0, 1.0, "cpu"), torch.zeros(0, 3),
                           torch.zeros(0, 3), 100)
    assert out.shape == (0,) and not launched
