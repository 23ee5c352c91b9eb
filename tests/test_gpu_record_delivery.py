"""The float backward record of the brick kernels as deliver_record_blocked (csrc/brick_shared.h)
delivers it -- a half-wave exchange that brings both halves of a run's 64-byte line into one atomic
instruction -- against the per-ray kernels' record on the same rays, at sizes where the batches
are ragged: partial bricks, rows that end in partial runs, fewer than 32 hits per brick (the
pooled batch alone, instruction Y empty), both brick storages; the callers in bricks.hip (the
marcher's record, the channels' ray backward); and ``DRR.ncc`` against the composition."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from diffdrr_amd import DRR, NormalizedCrossCorrelation2d, convert, ops
from diffdrr_amd.data import make_subject, synthetic_subject

pytestmark = pytest.mark.gpu

DIMS = (40, 36, 70)  # 2 x 2 x 2 bricks of 32^3 (2 x 2 x 2 of 32 x 32 x 64 for the 16-bit storage), partial ones
CASES = [(19, 21, 3), (5, 7, 1)]  # (H, W, B): W no multiple of 8; 35 rays: fewer than 32 hits per brick


def voxel_rays(drr, rot, xyz):
    with torch.no_grad():
        pose = convert(rot, xyz, parameterization="euler_angles", convention="ZXY")
        source, target = drr.detector(pose, None)
        L = (target - source).norm(dim=-1)
        return (drr.affine_inverse(source).contiguous(), drr.affine_inverse(target).contiguous(),
                L.contiguous())


# Euler angles / translations per case.  The per-ray walk and the brick walk both evaluate every
# crossing as the reference's quotient (k - shift - s) / d to within an ulp, so where two crossings
# of a ray lie closer than fp32 resolves, their order -- hence the voxel between them, hence S0 / S1
# of ONE ray -- is arbitrary in either kernel (tests/test_gpu_parity.py compares "where the rays
# agree" for that reason: ~1 ray in 1000 at these sizes).  These poses were drawn at random and kept
# when, in float64, no ray of theirs has two crossings closer than 4e-6 of alpha (30 ulp):
# crossing_gap() below states that and scene() asserts it, so every ray is compared.
POSES = {
    (19, 21, 3): ([[0.01, 0.0, -0.48], [0.01, 0.05, 0.42], [0.05, 0.02, 0.38]],
                  [[-4.7, 252.1, 1.5], [8.2, 252.5, 3.8], [5.5, 253.3, -0.1]]),
    (5, 7, 1): ([[-0.15, 0.23, 0.47]], [[1.3, 259.6, 2.2]]),
}
MIN_GAP = 4e-6
# (those poses look almost along a volume axis -- fewer pairs of crossings --, where the gradient of a
# ray that runs inside a plane is ill-conditioned: the gradient tests of the other callers use plain
# oblique poses and the yardstick the suite has for rays with ties, conftest.py
# check_channel_backward_on_bricks: 99 % of the rays within 2e-3 of the largest gradient)
OBLIQUE = ([[0.31, -0.22, 0.13], [0.6, -0.4, 0.9], [-0.5, 0.4, 0.9]],
           [[2.0, 260.0, -3.0], [4.0, 250.0, -6.0], [-3.0, 270.0, 4.0]])


def crossing_gap(s, t):
    """Smallest distance between two plane crossings of a ray inside the volume, relative to
    alpha, per ray (float64 geometry alone; inf: the ray misses the volume)."""
    s, t = s.double().cpu().numpy(), t.double().cpu().numpy()
    out = np.full(t.shape[:2], np.inf)
    for b in range(t.shape[0]):
        d = t[b] - s[b, 0] + 1e-8
        al = [(np.arange(DIMS[a] + 1)[None, :] - 0.5 - s[b, 0, a]) / d[:, a:a + 1] for a in range(3)]
        lo = np.max([np.minimum(x[:, 0], x[:, -1]) for x in al], 0)
        hi = np.min([np.maximum(x[:, 0], x[:, -1]) for x in al], 0)
        allv = np.concatenate(al, 1)
        allv = np.sort(np.where((allv >= lo[:, None]) & (allv <= hi[:, None]), allv, np.inf), 1)
        with np.errstate(invalid="ignore"):
            g = np.diff(allv, axis=1) / np.abs(allv[:, 1:])
        out[b] = np.where(hi > lo, np.min(np.where(np.isfinite(g), g, np.inf), 1), np.inf)
    return out


_scenes = {}


def scene(gpu, H, W, B, oblique=False):
    """Noise volume DIMS and the B poses of POSES (oblique: the first B of OBLIQUE): (drr, rays, the
    per-ray kernel's image and record)."""
    key = (H, W, B, oblique)
    if key not in _scenes:
        vol = torch.rand(*DIMS, generator=torch.Generator().manual_seed(7))
        drr = DRR(make_subject(vol), sdd=400.0, height=H, width=W, delx=1.5).to(gpu)
        rot, xyz = (torch.tensor(v[:B], device=gpu) for v in (OBLIQUE if oblique else POSES[(H, W, B)]))
        s, t, L = voxel_rays(drr, rot, xyz)
        if not oblique:
            gap = crossing_gap(s, t)
            assert np.isfinite(gap).mean() > 0.9 and gap.min() >= MIN_GAP, gap.min()
        ref, aux_ref, _ = ops.siddon_forward(drr.density, s, t, L, want_aux=True)
        _scenes[key] = (drr, s, t, L, ref, aux_ref)
    return _scenes[key]


@pytest.mark.parametrize("storage", ["q16p", "f32"])
@pytest.mark.parametrize("H,W,B", CASES)
def test_blocked_record_equals_the_per_ray_record(gpu, H, W, B, storage):
    """Every plane of the blocked record of every ray at the tolerances test_gpu_parity.py holds the
    blocked record to: rtol 1e-4, atol 1e-5 of the plane's scale.  fp32 bricks: all five planes (the
    same voxel values and quotients as the per-ray walk, summed per brick).  16-bit bricks: plane I
    the same; S0 / S1 are sums of DIFFERENCES of voxels that the storage holds to 2^-17 of a brick's
    range (7.6e-6 per voxel of this noise volume: measured 2e-5 of the plane's scale after ~100
    crossings), so they get the tolerance test_gpu_parity.py has for those planes, 1e-3 of the plane's
    scale -- on every ray here, not on 97 % of them.  A plane delivered to the wrong place, twice or
    not at all is off by the plane's scale.  Then the ray gradients formed from the record."""
    drr, s, t, L, ref, aux_ref = scene(gpu, H, W, B)
    V = drr.density
    assert ops.brick_storage_applies(V) or storage == "f32"
    out, aux = ops.siddon_forward_bricks(V, s, t, L, (H, W), want_aux=True, storage=storage)
    assert aux.shape == (-(-B * H * W // 16), 80)
    planes = ops.record_planes(aux, B, H * W)
    # planes I, S0x, S0z, S1x, S1z of the interleaved record {I, S0xyz, S1xyz}
    for k, col in ((0, 0), (1, 1), (2, 3), (3, 4), (4, 6)):
        want = aux_ref[..., col]
        scale = float(want.abs().max())
        err = float((planes[k] - want).abs().max())
        print(f"{storage} {H}x{W} B={B} plane {k}: max |diff| {err:.3e}, scale {scale:.3e}")
        if k == 0 or storage == "f32":
            assert torch.allclose(planes[k], want, rtol=1e-4, atol=1e-5 * scale), (k, err, scale)
        else:
            assert err <= 1e-3 * scale, (k, err, scale)
    # what lies behind the last ray of the last block stays zero: inactive lanes add nothing
    flat = aux.reshape(-1, 5, 16)
    tail = B * H * W % 16
    if tail:
        last = flat[-1]
        assert float(last[4, tail:].abs().max()) == 0.0
        used = torch.zeros(4, 16, dtype=torch.bool, device=gpu)
        for r in range(tail):
            for p in range(4):
                used[(r >> 3) * 2 + (p >> 1), (p & 1) * 8 + (r & 7)] = True
        assert float(last[:4][~used].abs().max()) == 0.0
    go = torch.rand(B, H * W, device=gpu, generator=torch.Generator(gpu).manual_seed(0))
    gsb, gtb, gib = ops.siddon_backward_rays(aux, go, s, t, L)
    gsg, gtg, gig = ops.siddon_backward_rays(aux_ref, go, s, t, L)
    # (d / d img is plane I; the ray gradients are linear in S0 / S1: the planes' tolerances)
    assert rel_err(gib.cpu().numpy(), gig.cpu().numpy()) < 1e-4
    tol = 1e-4 if storage == "f32" else 1e-3
    for a, b in ((gtb, gtg), (gsb, gsg)):
        close = (a - b).abs().amax(-1) <= tol * b.abs().max()
        print(f"{storage} {H}x{W} B={B} ray gradients: {rel_err(a.cpu().numpy(), b.cpu().numpy()):.3e}")
        assert close.float().mean().item() > 0.99


@pytest.mark.parametrize("H,W,B", CASES)
def test_marcher_record_on_bricks(gpu, H, W, B):
    """bricks.hip's other record, the marcher's planar one, at the same sizes: ray gradients from it
    against the per-ray marcher's."""
    drr, s, t, L, _, _ = scene(gpu, H, W, B, oblique=True)
    V, P = drr.density, 96
    amin, amax = (a.min().reshape(1).contiguous() if i == 0 else a.max().reshape(1).contiguous()
                  for i, a in enumerate(ops.trilinear_alpha_range(s, t, V.shape)))
    go = torch.rand(B, H * W, device=gpu, generator=torch.Generator(gpu).manual_seed(2))
    out, aux = ops.trilinear_forward_bricks(V, s, t, L, amin, amax, (H, W), n_points=P, want_aux=True)
    ref = ops.trilinear_forward(V, s, t, L, amin, amax, n_points=P)
    assert rel_err(out.cpu().numpy(), ref.cpu().numpy()) < 1e-5
    mine = ops.trilinear_backward_rays(aux, go, s, t, L, amin, amax, n_points=P)
    want = ops.trilinear_backward(V, s, t, L, go, amin, amax, n_points=P)
    for k in ("g_source", "g_target", "g_img"):
        e = rel_err(mine[k].cpu().numpy(), want[k].cpu().numpy())
        print(f"marcher {H}x{W} B={B} {k}: {e:.3e}")
        assert e < 1e-4, (k, e)


@pytest.mark.parametrize("H,W,B", CASES)
def test_channel_ray_backward_on_bricks(gpu, H, W, B):
    """The channels' ray backward (BRICK_CHANNELS_AUX: the record weighted by every voxel's own
    incoming gradient, delivered by deliver_record_blocked) against the per-ray channel backward."""
    drr, s, t, L, _, _ = scene(gpu, H, W, B, oblique=True)
    V, C = drr.density, 5
    lab = torch.randint(0, C, DIMS, generator=torch.Generator().manual_seed(3), dtype=torch.uint8).to(gpu)
    go = torch.rand(B, C, H * W, device=gpu, generator=torch.Generator(gpu).manual_seed(4))
    gs, gt, gi = ops.siddon_backward_channels_bricks(V, lab, s, t, L, go, (H, W))
    ps, pt, pi, _ = ops.siddon_backward_channels(V, lab, s, t, L, go, det=(H, W))
    for name, a, b in (("g_img", gi, pi), ("g_target", gt, pt), ("g_source", gs, ps)):
        e = rel_err(a.cpu().numpy(), b.cpu().numpy())
        print(f"channels {H}x{W} B={B} {name}: {e:.3e}")
        if name == "g_img":
            assert e < 1e-4, e
        else:
            same = (a - b).abs().amax(-1) <= 2e-3 * b.abs().max()
            assert same.float().mean().item() > 0.99, (name, e)


def test_fused_ncc_step_small(gpu):
    """``DRR.ncc`` (forward + record launch, image and NCC from the record, pose gradients from it)
    against the composition at 64^3 -> 24 x 19, B = 3: values to 2e-6, gradients to 2e-4 of their
    largest entry (the bounds of conftest.check_fused_ncc_step)."""
    H, W, B = 24, 19, 3
    drr = DRR(synthetic_subject(64, kind="phantom", seed=3), sdd=500.0, height=H, width=W, delx=2.5).to(gpu)
    rot0 = torch.tensor([[0.2, -0.1, 0.3], [0.0, 0.0, 0.0], [-0.4, 0.25, 0.1]], device=gpu)
    xyz0 = torch.tensor([[3.0, 300.0, -2.0], [0.0, 310.0, 0.0], [-4.0, 320.0, 5.0]], device=gpu)
    with torch.no_grad():
        fixed = drr(torch.zeros(1, 3, device=gpu), torch.tensor([[0.0, 305.0, 0.0]], device=gpu),
                    parameterization="euler_angles", convention="ZXY")
    w = torch.tensor([0.7, -1.3, 2.1], device=gpu)
    res = []
    for fused in (True, False):
        r, x = rot0.clone().requires_grad_(), xyz0.clone().requires_grad_()
        if fused:
            val = drr.ncc(fixed, r, x, convention="ZXY")
            assert type(val.grad_fn).__name__.startswith("_EulerSiddonNccFn")
        else:
            val = NormalizedCrossCorrelation2d()(fixed.expand(B, -1, -1, -1),
                                                 drr(r, x, parameterization="euler_angles", convention="ZXY"))
        (val * w).sum().backward()
        res.append((val.detach().cpu().numpy(), r.grad.cpu().numpy(), x.grad.cpu().numpy()))
    (v1, gr1, gx1), (v0, gr0, gx0) = res
    print("ncc", np.abs(v1 - v0).max(), rel_err(gr1, gr0), rel_err(gx1, gx0))
    assert np.abs(v1 - v0).max() < 2e-6
    assert rel_err(gr1, gr0) < 2e-4 and rel_err(gx1, gx0) < 2e-4
