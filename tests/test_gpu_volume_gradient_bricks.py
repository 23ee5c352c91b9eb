"""On the MI355X: the four brick volume gradients (ddrr_siddon_backward_volume_bricks,
ddrr_trilinear_backward_volume_bricks and the two channel variants) against the float64 walk of
tests/volgrad_cases.py, voxel by voxel.

The entries accumulate in int32 fixed point under a per-launch bound n_sum * wmax
(csrc/bricks.hip volgrad_prepare_kernel) and in float where no bound exists.  Every voxel must be within

    |got - g64|  <=  2 rho32 T  +  (n + 2) Q / 2          Q = n_sum wmax / 2.0e9  (7.8e6: Siddon channels)

of the reference: twice what the package's own per-ray float32 kernel loses on the same rays (rho32, in units
of the voxel's rounding scale T, capped by volgrad_cases.RHO32_CAP) plus half a quantum per add, two adds
spare for grazing hits that only the float32 walk sees.  On the float path 8 * 2^-24 T takes the place of the
quanta.  Voxels no ray reaches are exactly 0.  The bound itself (words 1 and 2 of the launch workspace) is read
back to say which path ran and to size Q, never as an expected value; on the fixed path it must cover the
largest sum of |contributions| any voxel receives, so that the accumulator cannot wrap.

The figures a run prints (-s): rho32, the slack n_sum wmax / max A of the bound, and -- for incoming gradients
with faint pixels next to bright ones -- the error of the voxels only faint rays cross relative to their own
largest value: the fixed point's quantum is absolute, so such voxels keep fewer digits (the precision contract
in include/diffdrr_hip.h)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import volgrad_cases as vc
from diffdrr_amd import ops

pytestmark = pytest.mark.gpu

RETUNE = "re-tune the scene in tests/volgrad_cases.py (not this test) until it lands on the intended path"


@pytest.fixture()
def workspaces(monkeypatch):
    """Every launch workspace the test's brick launches were given, newest last."""
    kept, real = [], ops.launch_workspace

    def keeping(shape, device):
        kept.append(real(shape, device))
        return kept[-1]

    monkeypatch.setattr(ops, "launch_workspace", keeping)
    return kept


def voxel_rays(sc, gpu):
    """The scene's CPU-made float32 rays, as the launches take them."""
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    s, t, L = (dev(a) for a in vc.batch(sc))
    return SimpleNamespace(s=s, t=t, L=L, V=dev(sc.volume), labels=dev(sc.labels), amin=dev(np.array([sc.amin])),
                           amax=dev(np.array([sc.amax])))


def bricks(kind, sc, r, go):
    if kind == "siddon":
        return ops.siddon_backward_volume_bricks(sc.dims, r.s, r.t, r.L, go, sc.det)
    if kind == "marcher":
        return ops.trilinear_backward_volume_bricks(sc.dims, r.s, r.t, r.L, go, r.amin, r.amax, sc.det,
                                                    n_points=sc.n_points)
    if kind == "siddon_channels":
        return ops.siddon_backward_channels_volume_bricks(r.labels, r.s, r.t, r.L, go, sc.det)
    return ops.trilinear_backward_channels_volume_bricks(r.labels, r.s, r.t, r.L, go, r.amin, r.amax, sc.det,
                                                         n_points=sc.n_points)


def per_ray(kind, sc, r, go):
    """The same gradient from the per-ray kernels (global float32 atomics): the yardstick of float32 arithmetic."""
    if kind == "siddon":
        return ops.siddon_backward_volume(r.V, r.s, r.t, r.L, go, det=sc.det)
    no_rays = dict(want_rays=False, want_img=False, want_volume=True, det=sc.det)
    if kind == "marcher":
        return ops.trilinear_backward(r.V, r.s, r.t, r.L, go, r.amin, r.amax, n_points=sc.n_points, want_alpha=False,
                                      **no_rays)["g_volume"]
    if kind == "siddon_channels":
        return ops.siddon_backward_channels(r.V, r.labels, r.s, r.t, r.L, go, **no_rays)[3]
    return ops.trilinear_backward_channels(r.V, r.labels, r.s, r.t, r.L, go, r.amin, r.amax, n_points=sc.n_points,
                                           want_alpha=False, **no_rays)["g_volume"]


def bound_of(kind, ws):
    """(n_sum * wmax, Q, n_sum) of the launch that was given workspace `ws`, by the kernel's own switch restated
    (csrc/bricks.hip siddon_brick_kernel `fixq`).  Q = 0: the launch took the float path."""
    torch.cuda.synchronize()
    wmax, n_sum = (np.float32(v) for v in ws[1:3].view(torch.float32).cpu().numpy())
    counts = np.float32(vc.FIXED_COUNTS[kind])
    with np.errstate(all="ignore"):
        q = counts / (n_sum * wmax) if 0 < wmax < 1e30 and 0 < n_sum <= 16384 else np.float32(0)
    if not np.isfinite(q) or q == 0:
        return float(n_sum) * float(wmax), 0.0, float(n_sum)
    return float(n_sum) * float(wmax), float(n_sum) * float(wmax) / float(counts), float(n_sum)


def rho32_of(ref32, w):
    live = w.T > 0
    return float((np.abs(ref32.astype(np.float64) - w.g64)[live] / w.T[live]).max())


def gate(got, w, rho32, Q, where=None):
    """-> the problems of `got` against the walk `w` (voxels of `where` only), and the worst error in units of the
    allowance."""
    got = got.astype(np.float64)
    tol = 2 * rho32 * w.T + ((w.n + 2) * Q / 2 if Q > 0 else 8 * 2.0 ** -24 * w.T)
    err = np.abs(got - w.g64)
    where = np.ones(got.shape, bool) if where is None else where
    hit, problems = (w.n > 0) & where, []
    stray = (w.n == 0) & where & (got != 0)
    if stray.any():
        problems.append(f"{int(stray.sum())} voxels no ray reaches are not 0 (largest {np.abs(got[stray]).max():.3e})")
    if not np.isfinite(got[where]).all():
        problems.append("non-finite values")
    over = hit & ~(err <= tol)
    worst = float((err[hit] / tol[hit]).max()) if hit.any() else 0.0
    if over.any():
        v = np.unravel_index(np.argmax(np.where(over, err / np.maximum(tol, 1e-300), 0)), got.shape)
        problems.append(f"{int(over.sum())} voxels over the allowance, worst {worst:.2f} x at {v}: got {got[v]:.9e} "
                        f"g64 {w.g64[v]:.9e} T {w.T[v]:.3e} n {w.n[v]:.0f} Q {Q:.3e} rho32 {rho32:.3e}")
    return problems, worst


_walks = {}


def walk_of(sc, kind, pattern):
    key = (sc.name, kind, pattern)
    if key not in _walks:
        go, bright = vc.grad_out(sc, kind, pattern)
        _walks[key] = (go, vc.walk(sc, kind, go, bright))
    return _walks[key]


@pytest.mark.parametrize("kind", vc.KINDS)
@pytest.mark.parametrize("name", vc.SCENE_NAMES)
def test_every_voxel_within_float32_and_half_a_quantum_per_add(gpu, name, kind, workspaces):
    """The per-voxel gate, the path, the bound and bit-reproducibility, for G1 .. G4 on one scene and entry."""
    sc = vc.scene(name, kind)
    r = voxel_rays(sc, gpu)
    problems = []
    for pattern in vc.PATTERNS:
        go_np, w = walk_of(sc, kind, pattern)
        go = torch.from_numpy(go_np).to(gpu)
        ref32 = per_ray(kind, sc, r, go).cpu().numpy()
        out = bricks(kind, sc, r, go)
        bound, Q, n_sum = bound_of(kind, workspaces[-1])
        got = out.cpu().numpy()
        rho32 = rho32_of(ref32, w)
        tag = f"[{name} {kind} {pattern}]"
        print(f"{tag} path {'fixed' if Q else 'float'} n_sum {n_sum:.0f} rho32 {rho32:.3e} = {rho32 * 2 ** 24:.2f} x 2^-24"
              f" slack n_sum wmax / max A {bound / w.A.max():.2f}")
        if bool(Q) != sc.fixed:
            problems.append(f"{tag} ran on the {'fixed' if Q else 'float'} path (n_sum {n_sum}): {RETUNE}")
        if name.startswith("switch") and n_sum != sc.B * vc.SWITCH_R[vc.renderer_of(kind)]:
            problems.append(f"{tag} n_sum {n_sum} is not {sc.B} x {vc.SWITCH_R[vc.renderer_of(kind)]}: {RETUNE}")
        if Q and not w.A.max() <= bound:
            problems.append(f"{tag} the bound {bound:.6e} does not cover the largest voxel sum {w.A.max():.6e}")
        if not rho32 <= vc.RHO32_CAP[vc.renderer_of(kind)]:
            problems.append(f"{tag} the float32 yardstick is {rho32:.3e} from float64, over its cap")
        bad, worst = gate(got, w, rho32, Q)
        problems += [f"{tag} {p}" for p in bad]
        faint = (w.n > 0) & (w.nb == 0)
        if pattern in ("G3", "G3p", "G4"):
            own = np.abs(w.g64[faint]).max()
            print(f"{tag} worst error / allowance {worst:.2f}; {int(faint.sum())} voxels only faint rays cross: error "
                  f"{np.abs(got - w.g64)[faint].max() / own:.2e} of their largest value (per-ray float32: "
                  f"{np.abs(ref32 - w.g64)[faint].max() / own:.2e})")
        else:
            print(f"{tag} worst error / allowance {worst:.2f}")
        if Q:  # integer sums are associative: the same bits from every launch, on any stream
            again = bricks(kind, sc, r, go)
            if not torch.equal(out, again):
                problems.append(f"{tag} two launches differ")
            if pattern == "G1":
                torch.cuda.synchronize()
                side = torch.cuda.Stream()
                with torch.cuda.stream(side):
                    third = bricks(kind, sc, r, go)
                side.synchronize()
                if not torch.equal(out, third):
                    problems.append(f"{tag} a launch on a second stream differs")
    if name == "switch_lo":
        assert sc.B > 64  # at least three pose chunks of 32
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("scale", [1e-33, 1e-20, 1e20, 1e25])
@pytest.mark.parametrize("kind", ["siddon", "marcher"])
def test_any_scale_of_grad_out(gpu, kind, scale, workspaces):
    """grad_out times 1e-33 .. 1e25: finite, and after division by the scale within the same gate; the smallest --
    voxel values near 1e-31, ordinary float32 numbers -- does not come back as zeros."""
    sc = vc.scene("far3", kind)
    r = voxel_rays(sc, gpu)
    go_np = (vc.grad_out(sc, kind, "G1")[0] * np.float32(scale)).astype(np.float32)
    assert np.isfinite(go_np).all() and (go_np != 0).all()
    w = vc.walk(sc, kind, go_np.astype(np.float64) / scale)
    go = torch.from_numpy(go_np).to(gpu)
    ref32 = per_ray(kind, sc, r, go).cpu().numpy().astype(np.float64) / scale
    got32 = bricks(kind, sc, r, go).cpu().numpy()
    bound, Q, n_sum = bound_of(kind, workspaces[-1])
    got = got32.astype(np.float64) / scale
    rho32 = rho32_of(ref32, w)
    print(f"[far3 {kind} x{scale:g}] path {'fixed' if Q else 'float'} n_sum wmax {bound:.3e} rho32 {rho32:.3e} "
          f"largest |got| {np.abs(got32).max():.3e}")
    assert np.isfinite(got32).all()
    assert np.abs(got32).max() > 0, "an all-zero gradient"
    assert rho32 <= vc.RHO32_CAP[vc.renderer_of(kind)]
    problems, _ = gate(got, w, rho32, Q / scale)
    assert not problems, "\n".join(problems)


def _one_pixel(sc, kind, value):
    """G1 with pixel (H / 2, W / 2) of pose 0 set to `value` in every channel -> (grad_out, the same with that
    pixel zeroed, the pixel)."""
    H, W = sc.det
    n = (H // 2) * W + W // 2
    go = vc.grad_out(sc, kind, "G1")[0].copy()
    zeroed = go.copy()
    go[0, ..., n], zeroed[0, ..., n] = value, 0.0
    return go, zeroed, n


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
@pytest.mark.parametrize("kind", vc.KINDS)
def test_a_non_finite_pixel_reaches_its_ray_and_nothing_else(gpu, kind, value, workspaces):
    """One NaN (+inf) pixel of grad_out: every voxel its ray crosses with a float64 segment longer than 1e-3 voxels
    (a marcher's corner weight above 1e-3) is NaN (not finite), as the per-ray kernel and the reference have it;
    every voxel farther than one voxel from the ray is finite and within the gate for that pixel zeroed."""
    sc = vc.scene("far3", kind)
    r = voxel_rays(sc, gpu)
    go_np, zeroed, n = _one_pixel(sc, kind, value)
    sure, close = vc.ray_voxels(sc, kind, 0, n, 1e-3)
    assert sure.sum() >= 10 and (~close).sum() > 1000
    w = vc.walk(sc, kind, zeroed)
    rho32 = rho32_of(per_ray(kind, sc, r, torch.from_numpy(zeroed).to(gpu)).cpu().numpy(), w)
    got = bricks(kind, sc, r, torch.from_numpy(go_np).to(gpu)).cpu().numpy()
    bound, Q, n_sum = bound_of(kind, workspaces[-1])
    on_ray = np.isnan(got[sure]) if np.isnan(value) else ~np.isfinite(got[sure])
    print(f"[far3 {kind} pixel {value}] path {'fixed' if Q else 'float'} n_sum wmax {bound:.3e}: {int(on_ray.sum())} of "
          f"{int(sure.sum())} voxels of the ray are not finite")
    assert on_ray.all(), f"{int((~on_ray).sum())} of {int(sure.sum())} voxels of the pixel's ray are finite"
    assert rho32 <= vc.RHO32_CAP[vc.renderer_of(kind)]
    problems, _ = gate(np.where(close, 0.0, got), w, rho32, Q, where=~close)
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("kind", vc.KINDS)
def test_zero_grad_out_gives_zeros(gpu, kind):
    sc = vc.scene("far3", kind)
    r = voxel_rays(sc, gpu)
    go = torch.zeros(vc.grad_out(sc, kind, "G1")[0].shape, device=gpu)
    got = bricks(kind, sc, r, go)
    assert got.shape == tuple(sc.dims) and not got.any()
