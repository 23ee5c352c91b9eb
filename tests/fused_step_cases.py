"""What tests/test_fused_step.py (host emulation) and tests/test_gpu_fused_step.py (MI355X) share: the scenes of
the fused registration step (csrc/pose_ncc.hip on raygen_core.h: ddrr_pose_raygen_forward, the brick kernel,
ddrr_siddon_ncc_forward, ddrr_siddon_ncc_backward_pose | ddrr_siddon_backward_pose_euler, ddrr_pose_adam_step),
its definition in float64 and the checks, written once as ``check_*(device, ops)``.

The definition is plain torch in float64 on the same device, from the same float32 inputs -- rot, xyz, the
detector's reorientation, the volume's inverse affine, the calibrated detector points and the five planes of the
REAL blocked record of a render (ops.record_planes) -- with the chain written out, no autograd of a render:

    R = E(a0, th0) E(a1, th1) E(a2, th2);  v = Ro[:, 3] + xyz;  Mw = [R Ro3 | R v]
    sw = Mw[:, 3];  u = Mw3 P_n;  tw = u + sw;  L = |u|;  tv = Ainv tw;  sv = Ainv sw
    S0 = (S0x, -(S0x + S0z), S0z);  S1 = (S1x, I - (S1x + S1z), S1z);  inv_a = 1 / ((tv_a - sv_a) + eps)
    x2 = L I;  ncc and d ncc / d x2 as reference metrics.py:21-44
    per-pixel weight g:  gl = g L;  gs = gl (S1 - S0) inv;  gt = -gl S1 inv;  k = g I / L  (0 without the path
    through the ray length);  g_tw = Ainv3^T gt + k u;  g_sw = Ainv3^T gs - k u
    gMw[:, :3] = sum_n g_tw (x) P_n;  gMw[:, 3] = sum_n (g_tw + g_sw)
    GR = gMw[:, :3] Ro3^T + gMw[:, 3] (x) v;  g_xyz = R^T gMw[:, 3];  g_th_k = <GR, dR / dth_k>

Next to it runs its bound, ``fine``: the same chain with every factor replaced by its absolute value and every
difference by the sum of the absolute values -- the largest magnitude the definition allows per output.

The gate is the project's: a kernel may be as far from float64 as twice the float32 torch composition of the same
chain is (``own``), or 8 * 2^-24 of ``fine`` (four float32 ulps of the largest magnitude), whichever is larger.
Every check prints err and own in units of 2^-24 fine before it asserts."""
import types

import numpy as np
import torch

from diffdrr_amd import DRR
from diffdrr_amd.data import synthetic_subject
from diffdrr_amd.pose import _AXIS

U = 2.0 ** -24       # half a float32 ulp, relative
FLOOR = 8 * U
CHUNK = 32           # poses per render call
NCC_EPS = 1e-5
F64, F32 = torch.float64, torch.float32

# name -> (poses, detector H, W, pixel size): 40^3 noise subject, sdd 600, source 400 from the centre; the pixel
# size keeps the detector (half extent 7.5) inside the volume's shadow at every pose (rot +-0.3, xyz +-10): every
# ray crosses the whole subject, I >= 0.019 (at half extent 12 a few of 511 poses have corner rays that miss)
CASES = {
    "1x2x3": (1, 2, 3, 4.0),
    "3x30x26": (3, 30, 26, 0.5),
    "2x67x61": (2, 67, 61, 0.22),
    "2x64x65": (2, 64, 65, 0.22),
    "511x30x26": (511, 30, 26, 0.5),
    "512x30x26": (512, 30, 26, 0.5),
    "256x68x63": (256, 68, 63, 0.22),
    "256x67x65": (256, 67, 65, 0.22),
}
HOST_CASES = ("1x2x3", "3x30x26", "2x67x61", "2x64x65")  # (the emulation has no dispatch: small cases only)
# name -> (rays, 16-byte path, (forward quads per thread, workgroups per pose), (backward rays per workgroup,
# workgroups per pose)): what the case was chosen for
DISPATCH = {
    "1x2x3": (6, False, (1, 1), (1024, 1)),
    "3x30x26": (780, True, (1, 1), (1024, 1)),
    "2x67x61": (4087, False, (1, 4), (1024, 4)),
    "2x64x65": (4160, True, (1, 5), (1024, 5)),
    "511x30x26": (780, True, (1, 1), (1024, 1)),
    "512x30x26": (780, True, (4, 1), (2048, 1)),
    "256x68x63": (4284, True, (4, 2), (2048, 3)),
    "256x67x65": (4355, False, (4, 2), (2048, 3)),
}
WORKGROUPS_WANTED = 512  # csrc/pose_ncc.hip kStepWorkgroupsWanted


def forward_variant(B, N):
    """ddrr_siddon_ncc_forward's choice: (quads per thread, workgroups per pose)."""
    big = B * -(-N // 4096) >= WORKGROUPS_WANTED
    return (4, -(-N // 4096)) if big else (1, -(-N // 1024))


def backward_variant(B, N):
    """The two backward entries' choice: (rays per workgroup, workgroups per pose)."""
    big = B * -(-N // 2048) >= WORKGROUPS_WANTED
    return (2048, -(-N // 2048)) if big else (1024, -(-N // 1024))


# ------------------------------------------------------------------------------------------------ scenes
_modules, _scenes = {}, {}


def module(H, W, delx, device):
    key = (H, W, delx, str(device))
    if key not in _modules:
        _modules[key] = DRR(synthetic_subject(40, kind="noise", seed=3), sdd=600.0, height=H, width=W,
                            delx=delx).to(device)
    return _modules[key]


def geometry(drr):
    det = drr.detector
    P = drr._calibrated_points().contiguous()
    Ainv = (drr._affine_inverse[0, :3, :] if drr._affine_inverse.dim() == 3 else drr._affine_inverse[:3, :]).contiguous()
    return P, Ainv, det._reorient[:3, :].contiguous(), drr.renderer._cfg(False, det=(det.height, det.width))


def _render(name, device, ops, conv, rot, xyz):
    """The real blocked record of the B poses (CHUNK per call, concatenated) and everything the epilogues read."""
    B, H, W, delx = CASES[name]
    N = H * W
    drr = module(H, W, delx, device)
    P, Ainv, Ro, cfg = geometry(drr)
    axes = tuple(_AXIS[c] for c in conv)
    parts = []
    for a in range(0, B, CHUNK):
        r, x = rot[a:a + CHUNK].contiguous(), xyz[a:a + CHUNK].contiguous()
        aux = ops.brick_record_buffer(r.shape[0], N, device)
        launch_ws = ops.launch_workspace(drr.density.shape, drr.density.device)
        Mw, source, target, img = ops.pose_raygen_forward(r, x, axes, Ro, Ainv, P, clear=aux, clear_launch_ws=launch_ws)
        ops.siddon_forward_bricks(drr.density, source, target, img, cfg["det"], voxel_shift=cfg["voxel_shift"],
                                  eps=cfg["eps"], want_aux=True, storage="f32", want_image=False, aux=aux,
                                  launch_ws=launch_ws, cleared=True)
        parts.append((aux, Mw, source, target, img))
    aux, Mw, source, target, img = (torch.cat(t).contiguous() for t in zip(*parts))
    assert aux.shape == (ops.record_blocks(B, N), 80)
    planes = ops.record_planes(aux, B, N).contiguous()
    if len(parts) > 1:
        # CHUNK N is a multiple of 16: the chunks' records, one after the other, are the record of the batch
        chunks = torch.cat([ops.record_planes(p[0], p[1].shape[0], N) for p in parts], dim=1)
        assert torch.equal(planes, chunks)
    sc = types.SimpleNamespace(name=name, B=B, N=N, H=H, W=W, conv=conv, axes=axes, device=device, drr=drr, rot=rot,
                               xyz=xyz, P=P, Ainv=Ainv, Ro=Ro, eps=float(cfg["eps"]), aux=aux, Mw=Mw, source=source,
                               target=target, img=img, planes=planes, cache={})
    sc.entry = dict(source=source, Mw=Mw, Ainv=Ainv, P=P, rot=rot, xyz=xyz, axes=axes, reorient34=Ro)
    return sc


def _draw(gen, B, device):
    rot = ((torch.rand(B, 3, generator=gen) - 0.5) * 0.6).to(device)
    xyz = (torch.tensor([0.0, 400.0, 0.0]) + (torch.rand(B, 3, generator=gen) - 0.5) * 20).to(device)
    return rot, xyz


def _poses(name, device, ops):
    """The poses of a case: rot uniform in +-0.3, xyz = (0, 400, 0) +- 10, distinct per pose -- and, decided in
    float64 alone, such that the edge-hot weights (:func:`edge_weights`) are a sharp check at every pose: a ray
    that crosses a voxel plane at a grazing angle has a gradient thousands of times its neighbours' (1 / (tv_a -
    sv_a) with tv_a - sv_a ~ 0), and next to it in a pose's edge set no other ray is visible.  Such a pose (1 to
    3 % of them) is drawn again."""
    key = (name, str(device))
    if key not in _scenes:
        B, H, W, _ = CASES[name]
        gen = torch.Generator().manual_seed(7 + 1000 * B + H * W)
        rot, xyz = _draw(gen, B, device)
        for _ in range(10):
            sc = _render(name, device, ops, "ZXY", rot, xyz)
            ok = edge_hot_is_sharp(sc)[0]
            print(f"{name}: {int((~ok).sum())} of {B} poses drawn again (a grazing ray in their edge set)")
            if bool(ok.all()):
                break
            again = _draw(gen, B, device)
            rot, xyz = torch.where(ok[:, None], rot, again[0]), torch.where(ok[:, None], xyz, again[1])
        else:
            sc = _render(name, device, ops, "ZXY", rot, xyz)  # (the check asserts the condition itself)
        _scenes[key] = (rot, xyz, sc)
    return _scenes[key]


def scene(name, device, ops, conv="ZXY"):
    """The inputs of a case on `device`, rendered once per (case, convention, device) and never modified.  Asserts
    the dispatch the case stands for."""
    key = (name, conv, str(device))
    if key in _scenes:
        return _scenes[key]
    B, H, W, delx = CASES[name]
    N = H * W
    rays, vector, fwd, bwd = DISPATCH[name]
    assert N == rays and (N % 4 == 0) == vector, name
    assert forward_variant(B, N) == fwd and backward_variant(B, N) == bwd, (name, forward_variant(B, N),
                                                                           backward_variant(B, N))
    rot, xyz, zxy = _poses(name, device, ops)
    sc = zxy if conv == "ZXY" else _render(name, device, ops, conv, rot, xyz)
    # fixed images: one per pose (a neighbour's render, modulated) and one for the batch
    x2 = sc.img * sc.planes[0]
    mod = 1.0 + 0.3 * torch.rand(B, N, generator=torch.Generator().manual_seed(3 + N)).to(device)
    sc.x1_per_pose = (x2.roll(1, 0) * mod).contiguous()
    sc.x1_shared = sc.x1_per_pose[:1].clone()
    _scenes[key] = sc
    return sc


def inputs(sc, dtype):
    """The float32 inputs of the definition as `dtype` (float64: the definition, float32: the composition)."""
    if dtype not in sc.cache:
        sc.cache[dtype] = types.SimpleNamespace(rot=sc.rot.to(dtype), xyz=sc.xyz.to(dtype), Ro=sc.Ro.to(dtype),
                                                Ainv=sc.Ainv.to(dtype), P=sc.P.to(dtype),
                                                planes=sc.planes.to(dtype))
    return sc.cache[dtype]


# ------------------------------------------------------------------------------------------------ the definition
def elem(axis, th, deriv=False):
    """E(axis, th) (..., 3, 3), or dE / dth."""
    c, s = torch.cos(th), torch.sin(th)
    cc, ss = (-s, c) if deriv else (c, s)
    E = th.new_zeros(th.shape + (3, 3))
    p, q = (axis + 1) % 3, (axis + 2) % 3
    if not deriv:
        E[..., axis, axis] = 1.0
    E[..., p, p] = cc
    E[..., q, q] = cc
    E[..., p, q] = -ss
    E[..., q, p] = ss
    return E


def pose_of(rot, xyz, axes, Ro):
    """Steps 1-3 and their bounds, in the dtype of the arguments."""
    E = [elem(axes[k], rot[:, k]) for k in range(3)]
    D = [elem(axes[k], rot[:, k], True) for k in range(3)]
    aE, aD = [e.abs() for e in E], [d.abs() for d in D]
    R = E[0] @ E[1] @ E[2]
    dR = torch.stack([D[0] @ E[1] @ E[2], E[0] @ D[1] @ E[2], E[0] @ E[1] @ D[2]], 1)      # (B, 3, 3, 3)
    aR = aE[0] @ aE[1] @ aE[2]
    adR = torch.stack([aD[0] @ aE[1] @ aE[2], aE[0] @ aD[1] @ aE[2], aE[0] @ aE[1] @ aD[2]], 1)
    v, av = Ro[:, 3] + xyz, Ro[:, 3].abs() + xyz.abs()
    Mw = torch.cat([R @ Ro[:, :3], R @ v[..., None]], -1)
    aMw = torch.cat([aR @ Ro[:, :3].abs(), aR @ av[..., None]], -1)
    return types.SimpleNamespace(R=R, dR=dR, v=v, Mw=Mw, aR=aR, adR=adR, av=av, aMw=aMw, Ro=Ro)


def rays_of(po, Ainv, P):
    """Steps 4-5 and their bounds: u, L, tv (B, n, .), sv (B, 1, 3)."""
    A3, a = Ainv[:, :3], Ainv[:, 3]
    sw = po.Mw[:, :, 3]
    u = torch.einsum("bij,nj->bni", po.Mw[:, :, :3], P)
    au = torch.einsum("bij,nj->bni", po.aMw[:, :, :3], P.abs())
    tw = u + sw[:, None]
    atw = au + po.aMw[:, None, :, 3]
    return types.SimpleNamespace(u=u, au=au, L=u.norm(dim=-1), aL=au.norm(dim=-1), tv=tw @ A3.T + a,
                                 atv=atw @ A3.abs().T + a.abs(), sv=(sw @ A3.T + a)[:, None],
                                 asv=(po.aMw[:, :, 3] @ A3.abs().T + a.abs())[:, None])


def to_parameters(po, gM, absolute=False):
    """Step 11 on gM (B, [n,] 3, 4) -> (B, [n,] 6) = (g_rot, g_xyz); absolute: its bound from the bound of gM."""
    R, dR, v = (po.aR, po.adR, po.av) if absolute else (po.R, po.dR, po.v)
    Ro3 = po.Ro[:, :3].abs() if absolute else po.Ro[:, :3]
    if gM.dim() == 4:
        R, dR, v = R[:, None], dR[:, None], v[:, None]
    GR = gM[..., :3] @ Ro3.T + gM[..., 3, None] * v[..., None, :]
    g_xyz = (R.transpose(-1, -2) @ gM[..., 3, None])[..., 0]
    g_th = torch.einsum("...ij,...kij->...k", GR, dR)
    return torch.cat([g_th, g_xyz], -1)


def pose_gradient(sc, g, g_abs=None, *, with_img_path=True, dtype=F64, cols=None, per_ray=False):
    """Steps 1-7, 10, 11 for the per-pixel weight g (B, n) in `dtype` -> (gradient (B, 6), fine (B, 6)).
    cols: the rays g is given on (every other ray has weight 0); per_ray: every ray's own share (B, n, 6)
    instead of the sum (the chain is linear in g)."""
    q = inputs(sc, dtype)
    P, planes = (q.P, q.planes) if cols is None else (q.P[cols], q.planes[:, :, cols])
    g = g.to(dtype)
    ga = g.abs() if g_abs is None else g_abs.to(dtype)
    po = pose_of(q.rot, q.xyz, sc.axes, q.Ro)
    ry = rays_of(po, q.Ainv, P)
    A3 = q.Ainv[:, :3]
    I, S0x, S0z, S1x, S1z = planes
    S0 = torch.stack([S0x, -(S0x + S0z), S0z], -1)
    S1 = torch.stack([S1x, I - (S1x + S1z), S1z], -1)
    aS0 = torch.stack([S0x.abs(), S0x.abs() + S0z.abs(), S0z.abs()], -1)
    aS1 = torch.stack([S1x.abs(), I.abs() + S1x.abs() + S1z.abs(), S1z.abs()], -1)
    inv = 1.0 / ((ry.tv - ry.sv) + sc.eps)
    gl, agl = (g * ry.L)[..., None], (ga * ry.L)[..., None]
    gs, gt = gl * (S1 - S0) * inv, -gl * S1 * inv
    ags, agt = agl * (aS1 + aS0) * inv.abs(), agl * aS1 * inv.abs()
    if with_img_path:
        ku, aku = (g * I / ry.L)[..., None] * ry.u, (ga * I.abs() / ry.L)[..., None] * ry.au
    else:
        ku, aku = torch.zeros_like(gs), torch.zeros_like(gs)
    g_tw, g_sw = gt @ A3 + ku, gs @ A3 - ku            # (Ainv3^T x)_a = sum_c Ainv3[c, a] x_c
    f_tw, f_sw = agt @ A3.abs() + aku, ags @ A3.abs() + aku
    if per_ray:
        gM = torch.cat([g_tw[..., None] * P[None, :, None, :], (g_tw + g_sw)[..., None]], -1)   # (B, n, 3, 4)
        return to_parameters(po, gM), None
    gM = torch.cat([torch.einsum("bni,nj->bij", g_tw, P), (g_tw + g_sw).sum(1)[..., None]], -1)
    fM = torch.cat([torch.einsum("bni,nj->bij", f_tw, P.abs()), (f_tw + f_sw).sum(1)[..., None]], -1)
    return to_parameters(po, gM), to_parameters(po, fM, absolute=True)


def ncc_of(sc, x1, g_out=None, dtype=F64):
    """Steps 8-9: stats (B, 5) = (mu1, s1, mu2, s2, ncc) of x1 ((1 | B), N) and x2 = L I; with g_out ((B,) or
    0-dim) the per-pixel gradient of sum_b g_out_b ncc_b w.r.t. x2 and its bound."""
    q = inputs(sc, dtype)
    ry = rays_of(pose_of(q.rot, q.xyz, sc.axes, q.Ro), q.Ainv, q.P)
    x1 = x1.to(dtype).expand(sc.B, -1)
    x2 = ry.L * q.planes[0]
    mu1, mu2 = x1.mean(-1, keepdim=True), x2.mean(-1, keepdim=True)
    s1 = (((x1 - mu1) ** 2).mean(-1, keepdim=True) + NCC_EPS).sqrt()
    s2 = (((x2 - mu2) ** 2).mean(-1, keepdim=True) + NCC_EPS).sqrt()
    z1, z2 = (x1 - mu1) / s1, (x2 - mu2) / s2
    ncc = (z1 * z2).mean(-1, keepdim=True)
    stats = torch.cat([mu1, s1, mu2, s2, ncc], -1)
    if g_out is None:
        return stats
    go = g_out.to(dtype).reshape(-1, 1).expand(sc.B, 1)
    g = go * (z1 - z2 * ncc) / (sc.N * s2)
    g_abs = go.abs() * ((x1.abs() + mu1.abs()) / s1 + (x2.abs() + mu2.abs()) / s2 * ncc.abs()) / (sc.N * s2)
    return stats, g, g_abs


# ------------------------------------------------------------------------------------------------ gates
def allowance(want, own, mag):
    return torch.maximum(2 * (own.double() - want).abs(), FLOOR * mag)


def hold(label, got, want, own, mag):
    """err <= max(2 own, 8 * 2^-24 mag) per entry, printed in units of 2^-24 mag first."""
    got, own, mag = got.double(), own.double(), mag.double().expand_as(want)
    err, o = (got - want).abs(), (own - want).abs()
    unit = (U * mag).clamp_min(1e-300)
    print(f"{label}: err / (2^-24 fine) max {float((err / unit).max()):.3g}, own / (2^-24 fine) max "
          f"{float((o / unit).max()):.3g}")
    assert torch.isfinite(got).all(), label
    bad = err > torch.maximum(2 * o, FLOOR * mag)
    assert not bool(bad.any()), (label, float((err / unit).max()), float((o / unit).max()), int(bad.sum()))


def workspace_is_zero(ops, sc):
    """The caller-owned accumulators and tickets: zero after every call (bit for bit)."""
    if sc.device.type == "cuda":
        torch.cuda.synchronize()
    ws = ops.siddon_ncc_workspace(sc.B, sc.device)
    assert not bool(ws.view(torch.int64).any()), "the step's workspace was not left zero"


def ulps32(a, b):
    a, b = a.detach().cpu().numpy().astype(np.float32), b.detach().cpu().numpy().astype(np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def unaligned(t):
    """A contiguous copy of `t` at an odd float offset of a larger buffer (no 16-byte loads from it)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


# ------------------------------------------------------------------------------------------------ 1 forward
def check_forward(name, device, ops):
    """ddrr_siddon_ncc_forward in every call form against steps 8-9."""
    sc = scene(name, device, ops)
    assert bool((sc.planes[0] > 0).all()), "every ray of the scene goes through the subject"
    image = sc.img * sc.planes[0]
    results = {}
    for label, x1 in (("shared", sc.x1_shared), ("per pose", sc.x1_per_pose)):
        want, own = ncc_of(sc, x1), ncc_of(sc, x1, dtype=F32)
        mag = torch.stack([want[:, 0].abs(), want[:, 1], want[:, 2].abs(), want[:, 3], torch.ones_like(want[:, 4])], -1)
        for form, x in (("aligned", x1), ("odd offset", unaligned(x1))):
            for want_image in (False, True):
                for want_sum in (False, True):
                    res = ops.siddon_ncc_forward(sc.aux, sc.img, x, NCC_EPS, want_image=want_image, want_sum=want_sum)
                    workspace_is_zero(ops, sc)
                    ncc, stats, out = res[:3]
                    tag = f"{name} forward, x1 {label} {form}, image {want_image}, sum {want_sum}"
                    hold(tag + ": stats", stats, want, own, mag)
                    assert torch.equal(ncc, stats[:, 4])
                    assert (out is None) if not want_image else torch.equal(out, image), tag
                    if want_sum:
                        total = float(res[3]) - float(ncc.double().sum())
                        print(f"{tag}: sum - float64 sum of the values = {total:.3g}")
                        assert abs(total) <= FLOOR * sc.B, tag
                    results[(label, form)] = (ncc, stats)
    # a per-pose copy of the shared image: the same values (the moments are double sums: 1 ulp)
    ncc, stats, _ = ops.siddon_ncc_forward(sc.aux, sc.img, sc.x1_shared.expand(sc.B, -1).contiguous(), NCC_EPS)
    workspace_is_zero(ops, sc)
    assert (ulps32(ncc, results[("shared", "aligned")][0]) <= 1).all()
    assert (ulps32(stats, results[("shared", "aligned")][1]) <= 1).all()


# ------------------------------------------------------------------------------------------------ 2 NCC route
def check_ncc_backward(name, device, ops):
    """ddrr_siddon_ncc_backward_pose against steps 1-11: g_out per pose and shared, both image paths, two
    conventions, a shared and a per-pose fixed image."""
    for conv in ("ZXY", "ZYX"):
        sc = scene(name, device, ops, conv)
        gen = torch.Generator().manual_seed(31)
        per_pose = (torch.randn(sc.B, generator=gen) + 0.25).to(device)
        for x_label, x1 in (("shared", sc.x1_shared), ("per pose", sc.x1_per_pose)):
            _, stats, _ = ops.siddon_ncc_forward(sc.aux, sc.img, x1, NCC_EPS)
            for g_label, g_out in (("per pose", per_pose), ("shared", torch.tensor(1.7, device=device))):
                for path in (True, False):
                    _, g, g_abs = ncc_of(sc, x1, g_out)
                    want, fine = pose_gradient(sc, g, g_abs, with_img_path=path)
                    _, g32, _ = ncc_of(sc, x1, g_out, dtype=F32)
                    own, _ = pose_gradient(sc, g32, with_img_path=path, dtype=F32)
                    g_rot, g_xyz = ops.siddon_ncc_backward_pose(
                        sc.aux, sc.img, x1, stats, g_out, sc.source, sc.target, sc.Mw, sc.Ainv, sc.P, sc.rot, sc.xyz,
                        sc.axes, sc.Ro, eps=sc.eps, with_img_path=path)
                    workspace_is_zero(ops, sc)
                    hold(f"{name} {conv} NCC backward, x1 {x_label}, g_out {g_label}, length path {path}",
                         torch.cat([g_rot, g_xyz], 1), want, own, fine)


# ------------------------------------------------------------------------------------------------ 3 explicit
def edge_set(N):
    """The rays next to every boundary a partition of the rays could have."""
    e = {0, 1, 3, 4, N - 5, N - 4, N - 1}
    for S in (256, 1024, 2048, 4096):
        for m in range(1, N // S + 2):
            e |= {m * S - 1, m * S}
    return sorted(n for n in e if 0 <= n < N)


def edge_weights(B, N):
    """-> (cols (E,), w (B, E)): distinct values with |w| in [0.5, 1.5] and random signs on the edge set; pose 0
    has all of it, pose b >= 1 the third b % 3."""
    cols = edge_set(N)
    E = len(cols)
    gen = torch.Generator().manual_seed(17 + N)
    mag = 0.5 + (torch.randperm(B * E, generator=gen).reshape(B, E).double() + 0.5) / (B * E)
    sign = torch.randint(0, 2, (B, E), generator=gen).double() * 2 - 1
    keep = (torch.arange(E)[None, :] % 3 == torch.arange(B)[:, None] % 3)
    keep[0] = True
    return torch.tensor(cols), (mag * sign * keep).float()


def edge_hot_is_sharp(sc):
    """-> (per pose: every weighted ray, removed alone, moves one of the six outputs by more than 4 allowances; the
    smallest such move in allowances; cols, w, and the float64 value, float32 composition and bound of the case)"""
    cols, w = edge_weights(sc.B, sc.N)
    cols, w = cols.to(sc.device), w.to(sc.device)
    want, fine = pose_gradient(sc, w, cols=cols)
    own, _ = pose_gradient(sc, w, cols=cols, dtype=F32)
    share, _ = pose_gradient(sc, w, cols=cols, per_ray=True)
    moves = (share.abs() / allowance(want, own, fine)[:, None, :]).amax(-1)
    moves = torch.where(w != 0, moves, torch.full_like(moves, float("inf")))
    return (moves > 4).all(1), float(moves.min()), cols, w, want, own, fine


def check_explicit_backward(name, device, ops):
    """ddrr_siddon_backward_pose_euler against steps 1-7, 10, 11 with (a) dense and (b) edge-hot weights."""
    sc = scene(name, device, ops)
    assert bool((sc.planes[0] > 0).all())
    dense = torch.randn(sc.B, sc.N, generator=torch.Generator().manual_seed(11)).to(device)
    for path in (True, False):
        want, fine = pose_gradient(sc, dense, with_img_path=path)
        own, _ = pose_gradient(sc, dense, with_img_path=path, dtype=F32)
        g_rot, g_xyz = ops.siddon_backward_pose_euler(sc.aux, dense, **sc.entry, eps=sc.eps, with_img_path=path)
        workspace_is_zero(ops, sc)
        hold(f"{name} explicit backward, dense, length path {path}", torch.cat([g_rot, g_xyz], 1), want, own, fine)
    # edge-hot: the rays at the boundaries carry the result.  The condition, in float64, before the kernel is
    # looked at: without any one weighted ray at least one of the six outputs moves by more than 4 x its allowance
    ok, margin, cols, w, want, own, fine = edge_hot_is_sharp(sc)
    print(f"{name} edge-hot: the least visible weighted ray moves an output by {margin:.3g} allowances")
    assert bool(ok.all()), (name, margin)
    full = torch.zeros(sc.B, sc.N, device=device)
    full[:, cols] = w
    assert bool((sc.planes[0][:, cols] > 0).all())
    g_rot, g_xyz = ops.siddon_backward_pose_euler(sc.aux, full, **sc.entry, eps=sc.eps)
    workspace_is_zero(ops, sc)
    hold(f"{name} explicit backward, edge-hot", torch.cat([g_rot, g_xyz], 1), want, own, fine)


# ------------------------------------------------------------------------------------------------ 4 repeat
def check_workspace_and_repeat(name, device, ops):
    """Every entry twice in a row: the workspace zero after each call, the second call's results within the gates
    of the first (a stale ticket or accumulator would show)."""
    sc = scene(name, device, ops)
    x1 = sc.x1_shared
    want_s, own_s = ncc_of(sc, x1), ncc_of(sc, x1, dtype=F32)
    mag = torch.stack([want_s[:, 0].abs(), want_s[:, 1], want_s[:, 2].abs(), want_s[:, 3], torch.ones_like(want_s[:, 4])], -1)
    g_out = torch.linspace(0.5, 1.5, sc.B).to(device)
    _, g, g_abs = ncc_of(sc, x1, g_out)
    want_n, fine_n = pose_gradient(sc, g, g_abs)
    own_n, _ = pose_gradient(sc, ncc_of(sc, x1, g_out, dtype=F32)[1], dtype=F32)
    dense = torch.randn(sc.B, sc.N, generator=torch.Generator().manual_seed(12)).to(device)
    want_e, fine_e = pose_gradient(sc, dense)
    own_e, _ = pose_gradient(sc, dense, dtype=F32)
    workspace_is_zero(ops, sc)
    for call in (1, 2):
        ncc, stats, _, total = ops.siddon_ncc_forward(sc.aux, sc.img, x1, NCC_EPS, want_sum=True)
        workspace_is_zero(ops, sc)
        hold(f"{name} call {call}: stats", stats, want_s, own_s, mag)
        assert abs(float(total) - float(ncc.double().sum())) <= FLOOR * sc.B
        g_rot, g_xyz = ops.siddon_ncc_backward_pose(sc.aux, sc.img, x1, stats, g_out, sc.source, sc.target, sc.Mw,
                                                    sc.Ainv, sc.P, sc.rot, sc.xyz, sc.axes, sc.Ro, eps=sc.eps)
        workspace_is_zero(ops, sc)
        hold(f"{name} call {call}: NCC backward", torch.cat([g_rot, g_xyz], 1), want_n, own_n, fine_n)
        g_rot, g_xyz = ops.siddon_backward_pose_euler(sc.aux, dense, **sc.entry, eps=sc.eps)
        workspace_is_zero(ops, sc)
        hold(f"{name} call {call}: explicit backward", torch.cat([g_rot, g_xyz], 1), want_e, own_e, fine_e)


# ------------------------------------------------------------------------------------------------ 5 Euler pose
CONVENTIONS = [(a0, a1, a2) for a0 in range(3) for a1 in range(3) for a2 in range(3) if a1 != a0 and a1 != a2]


def check_pose_euler(device, ops):
    """ddrr_pose_euler_forward / _backward alone: the 12 conventions, 257 poses (one more than a workgroup), angles
    over the whole circle with poses pinned at 0, +-pi/2 on the middle angle and pi, xyz up to +-500, a generic
    and the detector's reorientation, a random matrix gradient; then ddrr_pose_raygen_forward against
    ddrr_pose_euler_forward + ddrr_raygen_forward."""
    assert len(CONVENTIONS) == 12
    B = 257
    drr = module(30, 26, 0.5, device)
    P, Ainv, Ro_det, _ = geometry(drr)
    gen = torch.Generator().manual_seed(23)
    rot = (torch.rand(B, 3, generator=gen) * 2 - 1) * np.pi
    rot[0] = 0.0
    rot[1, 1], rot[2, 1] = np.pi / 2, -np.pi / 2
    rot[3] = np.pi
    xyz = (torch.rand(B, 3, generator=gen) * 2 - 1) * 500
    gM = torch.randn(B, 3, 4, generator=gen)
    rot, xyz, gM = rot.to(device), xyz.to(device), gM.to(device)
    generic = torch.randn(3, 4, generator=gen).to(device)
    for axes in CONVENTIONS:
        for r_label, Ro in (("generic", generic), ("detector", Ro_det)):
            po = pose_of(rot.double(), xyz.double(), axes, Ro.double())
            po32 = pose_of(rot, xyz, axes, Ro)
            tag = f"pose_euler {axes} reorient {r_label}"
            hold(tag + " forward", ops.pose_euler_forward(rot, xyz, axes, Ro), po.Mw, po32.Mw, po.aMw)
            g_rot, g_xyz = ops.pose_euler_backward(rot, xyz, axes, Ro, gM)
            hold(tag + " backward", torch.cat([g_rot, g_xyz], 1), to_parameters(po, gM.double()),
                 to_parameters(po32, gM), to_parameters(po, gM.double().abs(), absolute=True))
    # the fused launch against the two it replaces, and all of them against steps 1-5
    for axes in ((2, 0, 1), (2, 1, 0)):
        Mw = ops.pose_euler_forward(rot, xyz, axes, Ro_det)
        two = (Mw,) + tuple(ops.raygen_forward(Mw, Ainv, P))
        one = ops.pose_raygen_forward(rot, xyz, axes, Ro_det, Ainv, P)
        same = [torch.equal(a, b) for a, b in zip(one, two)]
        print(f"pose_raygen_forward {axes} equals pose_euler_forward + raygen_forward bit for bit "
              f"(Mw, source, target, img): {same}")
        if device.type == "cpu":
            assert all(same)
        po, po32 = pose_of(rot.double(), xyz.double(), axes, Ro_det.double()), pose_of(rot, xyz, axes, Ro_det)
        ry, ry32 = rays_of(po, Ainv.double(), P.double()), rays_of(po32, Ainv, P)
        for label, (m, s, t, L) in (("fused", one), ("two launches", two)):
            hold(f"pose_raygen {axes} {label}: Mw", m, po.Mw, po32.Mw, po.aMw)
            hold(f"pose_raygen {axes} {label}: source", s, ry.sv, ry32.sv, ry.asv)
            hold(f"pose_raygen {axes} {label}: target", t, ry.tv, ry32.tv, ry.atv)
            hold(f"pose_raygen {axes} {label}: length", L, ry.L, ry32.L, ry.aL)


# ------------------------------------------------------------------------------------------------ 6 clears
def check_clears(device, ops):
    """What ddrr_pose_raygen_forward clears for the render behind it: exactly `clear`, whatever its length modulo
    4, below the launch's thread count and above it (the stride loop: 10 007 floats behind 256 threads)."""
    drr = module(2, 3, 4.0, device)
    P, Ainv, Ro, _ = geometry(drr)
    assert P.shape[0] == 6
    rot = torch.zeros(1, 3, device=device)
    xyz = torch.tensor([[0.0, 400.0, 0.0]], device=device)
    first = ops.pose_raygen_forward(rot, xyz, (2, 0, 1), Ro, Ainv, P)
    for n in (1, 2, 3, 100, 101, 102, 103, 1024, 1025, 10004, 10005, 10006, 10007):
        buf = torch.full((n + 64,), float("nan"), device=device)
        assert buf.data_ptr() % 16 == 0
        out = ops.pose_raygen_forward(rot, xyz, (2, 0, 1), Ro, Ainv, P, clear=buf[:n])
        assert bool((buf[:n] == 0).all()), n
        assert bool(torch.isnan(buf[n:]).all()), n
        assert all(torch.equal(a, b) for a, b in zip(out, first)), n
    # more threads than floats to clear, several workgroups in both grid dimensions
    sc = scene("3x30x26", device, ops)
    for n in (5, 780, 781, 782, 783, 3 * 1024 + 2):
        buf = torch.full((n + 64,), float("nan"), device=device)
        ops.pose_raygen_forward(sc.rot, sc.xyz, sc.axes, sc.Ro, sc.Ainv, sc.P, clear=buf[:n])
        assert bool((buf[:n] == 0).all()) and bool(torch.isnan(buf[n:]).all()), n


# ------------------------------------------------------------------------------------------------ 7 Adam
def check_pose_adam(device, ops):
    """ddrr_pose_adam_step against torch.optim.Adam in float64 on the same float32 gradients: 1 ... 300 poses (6 B >
    256: the stride loop from 43 poses on), ten steps, a learning-rate change midway, the two step counters
    started apart.  Yardstick: torch's float32 Adam; floors: lr 2^-22 for the parameters (lr: the group's largest),
    steps 2^-23 max |moment| for the moments (two roundings per step)."""
    steps, start = 10, (0.0, 3.0)
    # (the entry takes its hyper-parameters as floats: values a float holds exactly, the same for both sides)
    betas, eps = (float(np.float32(0.9)), float(np.float32(0.999))), float(np.float32(1e-8))
    lrs = lambda it: (0.125 if it < 5 else 0.03125, 5.0)  # noqa: E731
    for B in (1, 42, 43, 300):
        for maximize in (False, True):
            gen = torch.Generator().manual_seed(100 + B)
            p0 = [torch.randn(B, 3, generator=gen), torch.randn(B, 3, generator=gen) * 50.0]
            grads = [[torch.randn(B, 3, generator=gen) * 10.0 ** (it % 3 - 1), torch.randn(B, 3, generator=gen) * 1e-3]
                     for it in range(steps)]

            def torch_loop(dtype):
                ps = [torch.nn.Parameter(p.to(dtype).clone()) for p in p0]
                opt = torch.optim.Adam([{"params": [ps[0]], "lr": 0.125}, {"params": [ps[1]], "lr": 5.0}], betas=betas,
                                       eps=eps, maximize=maximize, foreach=False)
                for p, s0 in zip(ps, start):
                    opt.state[p] = dict(step=torch.tensor(s0), exp_avg=torch.zeros_like(p),
                                        exp_avg_sq=torch.zeros_like(p))
                for it in range(steps):
                    for p, gr, group, lr in zip(ps, grads[it], opt.param_groups, lrs(it)):
                        p.grad = gr.to(dtype).clone()
                        group["lr"] = lr
                    opt.step()
                return [(p.detach().double(), opt.state[p]["exp_avg"].double(), opt.state[p]["exp_avg_sq"].double(),
                         float(opt.state[p]["step"])) for p in ps]

            ref64, ref32 = torch_loop(F64), torch_loop(F32)
            p = [t.clone().to(device) for t in p0]
            m = [torch.zeros_like(t) for t in p]
            v = [torch.zeros_like(t) for t in p]
            st = [torch.tensor([s0], device=device) for s0 in start]
            for it in range(steps):
                gr = [t.to(device) for t in grads[it]]
                ops.pose_adam_step(p[0], p[1], gr[0], gr[1], m[0], v[0], m[1], v[1], st[0], st[1], lr_rot=lrs(it)[0],
                                   lr_xyz=lrs(it)[1], betas=betas, eps=eps, maximize=maximize)
            for k, (group, lr) in enumerate((("rotation", 0.125), ("translation", 5.0))):
                p64, m64, v64, n64 = ref64[k]
                p32, m32, v32, _ = ref32[k]
                assert float(st[k]) == n64 == start[k] + steps
                for what, mine, f32, f64, floor in (
                        ("param", p[k], p32, p64, lr * 2.0 ** -22),
                        ("exp_avg", m[k], m32, m64, steps * 2.0 ** -23 * float(m64.abs().max())),
                        ("exp_avg_sq", v[k], v32, v64, steps * 2.0 ** -23 * float(v64.abs().max()))):
                    err = float((mine.double().cpu() - f64).abs().max())
                    own = float((f32 - f64).abs().max())
                    print(f"pose_adam B={B} maximize={maximize} {group} {what}: err {err:.3g} torch float32 {own:.3g} "
                          f"floor {floor:.3g}")
                    assert err <= 2 * own + floor, (B, maximize, group, what, err, own, floor)


# ------------------------------------------------------------------------------------------------ 8 unfused
def check_unfused_entry(device, ops):
    """ddrr_siddon_backward_pose + ddrr_pose_euler_backward on the blocked record and on the same numbers as an
    interleaved (B, N, 8) record, at 4087 rays: the gradient gate of the same float64 value."""
    sc = scene("2x67x61", device, ops)
    dense = torch.randn(sc.B, sc.N, generator=torch.Generator().manual_seed(13)).to(device)
    want, fine = pose_gradient(sc, dense)
    own, _ = pose_gradient(sc, dense, dtype=F32)
    I, S0x, S0z, S1x, S1z = sc.planes
    rec = torch.stack([I, S0x, -(S0x + S0z), S0z, S1x, I - (S1x + S1z), S1z, torch.zeros_like(I)], -1).contiguous()
    for label, aux in (("blocked", sc.aux), ("interleaved", rec)):
        gMw = ops.siddon_backward_pose(aux, dense, sc.source, sc.target, sc.img, sc.Mw, sc.Ainv, sc.P, eps=sc.eps)
        g_rot, g_xyz = ops.pose_euler_backward(sc.rot, sc.xyz, sc.axes, sc.Ro, gMw)
        hold(f"unfused backward, {label} record", torch.cat([g_rot, g_xyz], 1), want, own, fine)


# ------------------------------------------------------------------------------------------------ the model
def check_chain_against_autograd(device, ops):
    """The written-out chain against float64 autograd of the model it differentiates: a ray's integral linear in
    its voxel-space end points around the rendered pose (the record holds the slopes), times the ray's length."""
    for name, conv, path in (("3x30x26", "ZXY", True), ("3x30x26", "ZYX", False), ("1x2x3", "ZXY", True)):
        sc = scene(name, device, ops, conv)
        q = inputs(sc, F64)
        w = torch.randn(sc.B, sc.N, generator=torch.Generator().manual_seed(5)).to(device).double()
        want, fine = pose_gradient(sc, w, with_img_path=path)
        rot, xyz = q.rot.clone().requires_grad_(), q.xyz.clone().requires_grad_()

        def rays(rot, xyz):
            R = elem(sc.axes[0], rot[:, 0]) @ elem(sc.axes[1], rot[:, 1]) @ elem(sc.axes[2], rot[:, 2])
            M = torch.cat([R, (R @ xyz[..., None])], -1) @ torch.cat([q.Ro, q.Ro.new_tensor([[0, 0, 0, 1.0]])])
            tw = q.P @ M[:, :, :3].transpose(1, 2) + M[:, None, :, 3]
            sw = M[:, None, :, 3]
            to_voxels = lambda x: x @ q.Ainv[:, :3].T + q.Ainv[:, 3]  # noqa: E731
            return (tw - sw).norm(dim=-1), to_voxels(sw), to_voxels(tw)

        with torch.no_grad():
            L0, sv0, tv0 = rays(rot, xyz)
        I, S0x, S0z, S1x, S1z = q.planes
        S0 = torch.stack([S0x, -(S0x + S0z), S0z], -1)
        S1 = torch.stack([S1x, I - (S1x + S1z), S1z], -1)
        inv = 1.0 / ((tv0 - sv0) + sc.eps)
        L, sv, tv = rays(rot, xyz)
        line = I + (((S1 - S0) * inv) * (sv - sv0)).sum(-1) - ((S1 * inv) * (tv - tv0)).sum(-1)
        image = (L if path else L0) * line
        g_rot, g_xyz = torch.autograd.grad((w * image).sum(), (rot, xyz))
        got = torch.cat([g_rot, g_xyz], 1)
        rel = float(((got - want).abs() / fine).max())
        print(f"{name} {conv}: chain - autograd of the model, largest / fine = {rel:.3g}")
        assert rel <= 1e-13, rel


# ------------------------------------------------------------------------------------------------ layouts
def check_layout_errors(ops):
    """The three entries that read the blocked record alone refuse every other record and every other x1 (no
    launch happens)."""
    import pytest

    B, N = 2, 24
    blocked = torch.zeros(ops.record_blocks(B, N), 80)
    img = torch.ones(B, N)
    x1 = torch.ones(1, N)
    stats = torch.zeros(B, 5)
    pose = dict(source=torch.zeros(B, 1, 3), Mw=torch.zeros(B, 3, 4), Ainv=torch.zeros(3, 4), P=torch.zeros(N, 3),
                rot=torch.zeros(B, 3), xyz=torch.zeros(B, 3), axes=(2, 0, 1), reorient34=torch.zeros(3, 4))
    launched = []
    real = ops._launch
    ops._launch = lambda name, *a: launched.append(name)
    try:
        for bad in (torch.zeros(B, N, 8), torch.zeros(7, B, N), torch.zeros(ops.record_blocks(B, N) + 1, 80),
                    torch.zeros(B * N * 5)):
            with pytest.raises(ValueError, match="aux"):
                ops.siddon_ncc_forward(bad, img, x1, NCC_EPS)
            with pytest.raises(ValueError, match="aux"):
                ops.siddon_ncc_backward_pose(bad, img, x1, stats, torch.ones(B), target=torch.zeros(B, N, 3), **pose)
            with pytest.raises(ValueError, match="aux"):
                ops.siddon_backward_pose_euler(bad, img, **pose)
        for bad in (torch.ones(N), torch.ones(1, N + 1), torch.ones(3, N), torch.ones(1, 1, N), torch.ones(B, 4, 6)):
            with pytest.raises(ValueError, match="x1"):
                ops.siddon_ncc_forward(blocked, img, bad, NCC_EPS)
            with pytest.raises(ValueError, match="x1"):
                ops.siddon_ncc_backward_pose(blocked, img, bad, stats, torch.ones(B), target=torch.zeros(B, N, 3),
                                             **pose)
        assert not launched
    finally:
        ops._launch = real
