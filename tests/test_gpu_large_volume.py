"""Volumes above 2^30 voxels on the MI355X ("Volume size").

Three shapes: A = 1024 x 1024 x 1040 (1.09e9 voxels, 4.4 GB), B = 1400 x 1280 x 1280 (2.29e9,
9.2 GB: flat indices beyond 2^31, where a signed 32-bit index overflows) and C = 4200 x 1024 x 1024
(4.40e9, 17.6 GB: beyond 2^32, where an unsigned 32-bit index wraps).

* Cropped oracle.  The volume is zero except blocks of distinct, position-dependent values along x,
  one wholly beyond each of 2^30, 2^31 and 2^32 voxels that the shape reaches.  Outside the blocks
  every voxel is zero, so the fp64 CPU oracle run on the bounding box of the blocks (a one-voxel zero
  margin, rays shifted by the box's origin) gives the exact result without copying the volume to the
  host.  One pose runs along +x, one along -x (negative steps).
* Slab equivalence.  A noise-plus-phantom volume is cut into x slabs of at most 2^30 voxels; each is
  rendered on the 32-bit kernels with the rays shifted by -k0 (the marcher with the full volume's
  sampling range): the slab images and ray gradients add up to the full render's, the slab volume
  gradients concatenate to the full one.  32 poses, 256^2, rays in every direction.
* The DRR module on shape A against itself on the cropped subject (the same world geometry: the
  crop's affine is the full volume's, moved to the crop's first voxel).

Each case runs under a Python alarm (the module's fixtures included); the suite is run under an
outer `timeout` as well, which also ends a call blocked in the device."""
import signal

import numpy as np
import pytest
import torch

import oracle
from conftest import rel_err
from diffdrr_amd import DRR, ops
from diffdrr_amd.data import make_subject, centered_affine

pytestmark = pytest.mark.gpu

SHAPES = {"A": (1024, 1024, 1040), "B": (1400, 1280, 1280), "C": (4200, 1024, 1024)}
YZ = (400, 440)
DET = (64, 64)
GATE = 1e-4
# Volume and ray gradients against the fp64 oracle: a ray here is up to ~7000 voxels long, so a
# segment is ~1.4e-4 in alpha, which fp32 resolves to ~4e-4 of itself near alpha = 0.5 (the oracle
# does not round it)
VOL_GATE = 1e-3
LIMIT_S = 600


class _Alarm:
    """SIGALRM after `seconds`: the time limit of one case or fixture."""

    def __init__(self, seconds):
        self.seconds = seconds

    def __enter__(self):
        def expire(*_):
            raise TimeoutError("large-volume case over its time limit")
        self.old = signal.signal(signal.SIGALRM, expire)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        signal.signal(signal.SIGALRM, self.old)


@pytest.fixture(autouse=True)
def time_limit():
    with _Alarm(LIMIT_S):
        yield


def _blocks(shape):
    """(x0, x1, level): one block near the front, one wholly beyond each of 2^30, 2^31, 2^32 voxels."""
    stride = shape[1] * shape[2]
    out = [(100, 140, 1.0)]
    for k, level in ((30, 2.0), (31, 3.0), (32, 4.0)):
        x0 = -(-(1 << k) // stride) + 2
        if x0 + 12 <= shape[0]:
            out.append((x0, x0 + 10, level))
    return out


def _blocks_volume(shape, blocks, device):
    vol = torch.zeros(shape, dtype=torch.float32, device=device)
    y0, y1 = YZ
    y = torch.arange(y0, y1, device=device, dtype=torch.float32)
    for x0, x1, level in blocks:
        x = torch.arange(x0, x1, device=device, dtype=torch.float32)
        pat = (x[:, None, None] * 7 + y[None, :, None] * 13 + y[None, None, :] * 17) % 11
        vol[x0:x1, y0:y1, y0:y1] = level + 0.01 * pat
    return vol


def _rays(shape, device):
    """A det_h x det_w affine target grid per pose through every block: pose 0 runs along +x,
    pose 1 along -x."""
    h, w = DET
    i = torch.arange(h, dtype=torch.float64)[:, None].expand(h, w)
    j = torch.arange(w, dtype=torch.float64)[None, :].expand(h, w)
    src, tgt = [], []
    for b, (sx, tx) in enumerate(((-1500.0, shape[0] + 1600.0), (shape[0] + 1500.0, -1600.0))):
        s = torch.tensor([sx, 420.3 + 3 * b, 419.7 - 2 * b], dtype=torch.float64)
        t = torch.stack([torch.full_like(i, tx), 380.2 + 80 * i / (h - 1), 380.6 + 80 * j / (w - 1)],
                        -1).reshape(-1, 3)
        src.append(s[None])
        tgt.append(t)
    s = torch.stack(src).float().to(device)
    t = torch.stack(tgt).float().to(device)
    L = (t - s).norm(dim=-1)
    return s.contiguous(), t.contiguous(), L.contiguous()


def _make_scene(name):
    device = torch.device("cuda")
    shape = SHAPES[name]
    blocks = _blocks(shape)
    vol = _blocks_volume(shape, blocks, device)
    assert vol.numel() > 1 << 30
    # the last block lies wholly beyond 2^30 / 2^31 / 2^32 voxels
    assert blocks[-1][0] * shape[1] * shape[2] >= {"A": 1 << 30, "B": 1 << 31, "C": 1 << 32}[name]
    s, t, L = _rays(shape, device)
    lo = np.array([blocks[0][0] - 1, YZ[0] - 1, YZ[0] - 1])
    hi = np.array([blocks[-1][1] + 1, YZ[1] + 1, YZ[1] + 1])
    crop = vol[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]].double().cpu().numpy()
    o = torch.tensor(lo, dtype=torch.float64)
    s64, t64, L64 = (s.double().cpu() - o).numpy(), (t.double().cpu() - o).numpy(), L.double().cpu().numpy()
    return dict(name=name, vol=vol, s=s, t=t, L=L, crop=crop, lo=lo, hi=hi, s64=s64, t64=t64, L64=L64)


@pytest.fixture(scope="module", params=sorted(SHAPES))
def scene(request):
    with _Alarm(LIMIT_S):
        sc = _make_scene(request.param)
    yield sc
    sc.clear()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def scene_a():
    with _Alarm(LIMIT_S):
        sc = _make_scene("A")
    yield sc
    sc.clear()
    torch.cuda.empty_cache()


def _img(x):
    return x.detach().double().cpu().numpy().reshape(x.shape[0], -1)


def _box(scene):
    lo, hi = scene["lo"], scene["hi"]
    return slice(lo[0], hi[0]), slice(lo[1], hi[1]), slice(lo[2], hi[2])


def test_siddon_forward_routes_match_the_cropped_oracle(scene):
    vol, s, t, L = scene["vol"], scene["s"], scene["t"], scene["L"]
    args = (scene["crop"], scene["s64"], scene["t64"], scene["L64"])
    ref = oracle.siddon(*args)["out"].reshape(2, -1)
    ref_max = oracle.siddon(*args, reducefn="max")["out"].reshape(2, -1)
    ref_bil = oracle.siddon(*args, mode="bilinear")["out"].reshape(2, -1)
    assert np.abs(ref).max() > 0
    got = {
        "per-ray sum": (ops.siddon_forward(vol, s, t, L, det=DET)[0], ref),
        "per-ray max": (ops.siddon_forward(vol, s, t, L, reducefn="max")[0], ref_max),
        "per-ray sources": (ops.siddon_forward(vol, s.expand(-1, t.shape[1], -1).contiguous(), t, L)[0], ref),
        "midpoint bilinear": (ops.siddon_forward(vol, s, t, L, lookup="mid_trilinear")[0], ref_bil),
        # (align_corners=True scales the grid by (D - 1) / D: a crop is another grid, so the midpoint
        # nearest lookup is checked with align_corners=False, where it equals the stepping walk)
        "midpoint nearest": (ops.siddon_forward(vol, s, t, L, lookup="mid_nearest")[0], ref),
    }
    for storage in ("f32", "q16", "q16p"):
        got[f"bricks {storage}"] = (ops.siddon_forward_bricks(vol, s, t, L, DET, storage=storage)[0], ref)
    for name, (out, r) in got.items():
        e = rel_err(_img(out), r)
        # (reducefn="max" returns ONE segment's term: it carries the fp32 error of that segment's length,
        # which a sum telescopes away -- VOL_GATE above)
        assert e < (VOL_GATE if "max" in name else GATE), f"{name}: {e:.3g}"


def test_siddon_gradients_match_the_cropped_oracle(scene):
    vol, s, t, L = scene["vol"], scene["s"], scene["t"], scene["L"]
    box = _box(scene)
    g = torch.randn(2, t.shape[1], device=vol.device, generator=torch.Generator(vol.device).manual_seed(3))
    g64 = g.double().cpu().numpy()
    args = (scene["crop"], scene["s64"], scene["t64"], scene["L64"])
    ref = oracle.siddon(*args, grad_out=g64, want_volume_grad=True)
    # per-ray path: the forward record, then the ray and volume gradients
    _, aux, _ = ops.siddon_forward(vol, s, t, L, want_aux=True)
    gs, gt, gi = ops.siddon_backward_rays(aux, g, s, t, L)
    assert rel_err(gs.sum(1, keepdim=True).cpu(), ref["g_source"]) < VOL_GATE
    assert rel_err(gt.cpu(), ref["g_target"]) < VOL_GATE
    gv = ops.siddon_backward_volume(vol, s, t, L, g)
    assert rel_err(gv[box].cpu(), ref["g_volume"]) < VOL_GATE
    # brick path: the blocked record and the LDS-accumulated volume gradient
    _, baux = ops.siddon_forward_bricks(vol, s, t, L, DET, want_aux=True)
    bs, bt, _ = ops.siddon_backward_rays(baux, g, s, t, L)
    assert rel_err(bs.sum(1, keepdim=True).cpu(), ref["g_source"]) < VOL_GATE
    assert rel_err(bt.cpu(), ref["g_target"]) < VOL_GATE
    bv = ops.siddon_backward_volume_bricks(vol.shape, s, t, L, g, DET)
    assert rel_err(bv[box].cpu(), ref["g_volume"]) < VOL_GATE
    # the two volume gradients agree everywhere (outside the box too), at the volume's far end
    far = (slice(vol.shape[0] - 24, vol.shape[0]), slice(380, 460), slice(380, 460))
    assert gv[far].abs().max() > 0
    assert rel_err(bv[far].cpu(), gv[far].cpu()) < VOL_GATE
    del bv
    # reducefn="max": the scatter puts g L seg* on the arg-max voxel of each ray.  Which of two nearly
    # equal terms wins is decided by rounding (fp32 here, fp64 in the oracle), so the check is that each
    # ray's gradient lands on a voxel holding ITS value V*: sum_x gv(x) V(x) = sum_rays g out_max.
    del gv
    gv = ops.siddon_backward_volume(vol, s, t, L, g, reducefn="max")
    out_max = ops.siddon_forward(vol, s, t, L, reducefn="max")[0]
    lhs = float((gv[box].double() * vol[box].double()).sum())
    rhs = float((g.double() * out_max.double()).sum())
    assert abs(lhs - rhs) < GATE * float((g.double() * out_max.double()).abs().sum())
    assert float(gv.abs().sum()) == pytest.approx(float(gv[box].abs().sum()))  # nothing outside the blocks
    del gv
    # the midpoint lookups' backward (one more walk), with and without the volume gradient.  The render is
    # linear in the volume, so its volume gradient is checked by adjointness, sum_x gv(x) V(x) = sum g out
    # (a scatter to a wrong address breaks it); the nearest lookup's ray gradients are those of the
    # stepping walk (the oracle's; its ray gradient has no midpoint-position path for the bilinear lookup)
    for lookup in ("mid_trilinear", "mid_nearest"):
        ms, mt, mi, mv = ops.siddon_backward_midpoint(vol, s, t, L, g, lookup=lookup, want_volume=True)
        out = ops.siddon_forward(vol, s, t, L, lookup=lookup)[0]
        gout = (g.double() * out.double())
        lhs = float((mv[box].double() * vol[box].double()).sum())
        assert abs(lhs - float(gout.sum())) < GATE * float(gout.abs().sum()), lookup
        if lookup == "mid_nearest":
            assert rel_err(ms.sum(1, keepdim=True).cpu(), ref["g_source"]) < VOL_GATE
            assert rel_err(mt.cpu(), ref["g_target"]) < VOL_GATE
        del mv
        ms2, mt2, _, mv2 = ops.siddon_backward_midpoint(vol, s, t, L, g, lookup=lookup, want_volume=False)
        assert mv2 is None
        assert rel_err(ms2.cpu(), ms.cpu()) < 1e-6 and rel_err(mt2.cpu(), mt.cpu()) < 1e-6
    torch.cuda.empty_cache()


def test_trilinear_routes_match_the_cropped_oracle(scene):
    vol, s, t, L = scene["vol"], scene["s"], scene["t"], scene["L"]
    box = _box(scene)
    P = 1200
    amin, amax = (a.reshape(1).contiguous() for a in ops.trilinear_alpha_range(s, t, vol.shape))
    a0, a1 = float(amin), float(amax)
    g = torch.randn(2, t.shape[1], device=vol.device, generator=torch.Generator(vol.device).manual_seed(5))
    ref = oracle.trilinear(scene["crop"], scene["s64"], scene["t64"], scene["L64"], n_points=P, alphamin=a0,
                           alphamax=a1, grad_out=g.double().cpu().numpy(), want_volume_grad=True)
    out = ops.trilinear_forward(vol, s, t, L, amin, amax, n_points=P)
    assert rel_err(_img(out), ref["out"].reshape(2, -1)) < GATE
    outb = ops.trilinear_forward_bricks(vol, s, t, L, amin, amax, DET, n_points=P)
    assert rel_err(_img(outb), ref["out"].reshape(2, -1)) < GATE
    r = ops.trilinear_backward(vol, s, t, L, g, amin, amax, n_points=P, want_volume=True)
    assert rel_err(r["g_source"].sum(1, keepdim=True).cpu(), ref["g_source"]) < VOL_GATE
    assert rel_err(r["g_target"].cpu(), ref["g_target"]) < VOL_GATE
    gv = r["g_volume"]
    assert rel_err(gv[box].cpu(), ref["g_volume"]) < VOL_GATE
    del gv, r
    bv = ops.trilinear_backward_volume_bricks(vol.shape, s, t, L, g, amin, amax, DET, n_points=P)
    assert rel_err(bv[box].cpu(), ref["g_volume"]) < VOL_GATE
    del bv
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------- slab equivalence

def _phantom_noise(shape, device, seed=0):
    """Uniform noise in [0, 0.1) plus an ellipsoid of 1.0 and a smaller one of 0.5, built slab by slab."""
    g = torch.Generator(device).manual_seed(seed)
    vol = torch.empty(shape, dtype=torch.float32, device=device)
    c = [(d - 1) / 2 for d in shape]
    yy = ((torch.arange(shape[1], device=device) - c[1]) / (0.45 * shape[1]))[:, None] ** 2
    zz = ((torch.arange(shape[2], device=device) - c[2]) / (0.4 * shape[2]))[None, :] ** 2
    for x0 in range(0, shape[0], 64):
        x1 = min(shape[0], x0 + 64)
        xx = ((torch.arange(x0, x1, device=device) - c[0]) / (0.42 * shape[0]))[:, None, None] ** 2
        r2 = xx + yy[None] + zz[None]
        part = torch.rand((x1 - x0,) + tuple(shape[1:]), generator=g, device=device) * 0.1
        part += (r2 < 1).float() + 0.5 * (4 * r2 < 1).float()
        vol[x0:x1] = part
    return vol


def _cone_rays(shape, B, H, device, seed=0):
    """B cone-beam poses from every direction around the volume, an H x H affine target grid each."""
    g = torch.Generator().manual_seed(seed)
    c = torch.tensor([(d - 1) / 2 for d in shape], dtype=torch.float64)
    R = 1.6 * max(shape)
    W = 1.4 * max(shape)
    src, tgt = [], []
    for b in range(B):
        u = torch.randn(3, generator=g, dtype=torch.float64)
        u /= u.norm()
        e1 = torch.linalg.cross(u, torch.tensor([0.3, 0.5, 0.8], dtype=torch.float64))
        e1 /= e1.norm()
        e2 = torch.linalg.cross(u, e1)
        lin = torch.linspace(-0.5, 0.5, H, dtype=torch.float64) * W
        t = (c - R * u)[None, None] + lin[:, None, None] * e1 + lin[None, :, None] * e2
        src.append((c + R * u)[None])
        tgt.append(t.reshape(-1, 3))
    # on a 2^-10 grid (|coordinates| < 2^13): a ray shifted by an integer k0 is then the same ray in fp32,
    # bit for bit, and so are its plane crossings ((k - shift) - s is exact on both sides); the
    # detector stays affine within 5e-4 voxel
    q = 1024.0
    s = (torch.stack(src) * q).round() / q
    t = (torch.stack(tgt) * q).round() / q
    assert float(torch.cat([s.abs().flatten(), t.abs().flatten()]).max()) < 2 ** 13
    s, t = s.float().to(device).contiguous(), t.float().to(device).contiguous()
    return s, t, (t - s).norm(dim=-1).contiguous()


def _slabs(shape):
    # cuts on the 32-voxel brick grid, so that a slab's bricks are the full volume's
    n = -(-shape[0] * shape[1] * shape[2] // (1 << 30))
    cuts = [min(shape[0], 32 * round(k * shape[0] / n / 32)) for k in range(n)] + [shape[0]]
    assert all((k1 - k0) * shape[1] * shape[2] <= 1 << 30 for k0, k1 in zip(cuts, cuts[1:]))
    return list(zip(cuts, cuts[1:]))


def _shift(s, t, k0):
    off = torch.tensor([float(k0), 0.0, 0.0], device=s.device)
    return (s - off).contiguous(), (t - off).contiguous()


@pytest.mark.parametrize("name", ["A", "B"])
def test_slabs_add_up_to_the_full_render(name):
    shape = SHAPES[name]
    device = torch.device("cuda")
    B, H = 32, 256
    vol = _phantom_noise(shape, device)
    s, t, L = _cone_rays(shape, B, H, device)
    det = (H, H)
    g = torch.randn(B, H * H, device=device, generator=torch.Generator(device).manual_seed(7))
    slabs = _slabs(shape)
    assert len(slabs) == {"A": 2, "B": 3}[name]

    # Siddon, per-ray and on the bricks: image, ray gradients from the record, volume gradient
    for bricks in (False, True):
        def render(v, ss, tt):
            if bricks:
                out, aux = ops.siddon_forward_bricks(v, ss, tt, L, det, want_aux=True)
                gvol = ops.siddon_backward_volume_bricks(v.shape, ss, tt, L, g, det)
            else:
                out, aux, _ = ops.siddon_forward(v, ss, tt, L, want_aux=True, det=det)
                gvol = ops.siddon_backward_volume(v, ss, tt, L, g, det=det)
            gs, gt, _ = ops.siddon_backward_rays(aux, g, ss, tt, L)
            return out, gs, gt, gvol

        full = render(vol, s, t)
        parts = [render(vol[k0:k1], *_shift(s, t, k0)) for k0, k1 in slabs]
        what = "bricks" if bricks else "per-ray"
        assert rel_err(sum(p[0] for p in parts).cpu(), full[0].cpu()) < GATE, what
        # (ray by ray: the pose sums of 65536 random-sign terms cancel to a few per cent of their terms)
        assert rel_err(sum(p[1] for p in parts).cpu(), full[1].cpu()) < VOL_GATE, what
        assert rel_err(sum(p[2] for p in parts).cpu(), full[2].cpu()) < VOL_GATE, what
        assert rel_err(torch.cat([p[3] for p in parts]).cpu(), full[3].cpu()) < VOL_GATE, what
        del full, parts
        torch.cuda.empty_cache()

    # Trilinear (zero padding makes the marcher linear in the volume), with the full volume's range
    P = 600
    amin, amax = (a.reshape(1).contiguous() for a in ops.trilinear_alpha_range(s, t, shape))
    for bricks in (False, True):
        def march(v, ss, tt):
            if bricks:
                out = ops.trilinear_forward_bricks(v, ss, tt, L, amin, amax, det, n_points=P)
                gvol = ops.trilinear_backward_volume_bricks(v.shape, ss, tt, L, g, amin, amax, det, n_points=P)
                return out, None, None, gvol
            out = ops.trilinear_forward(v, ss, tt, L, amin, amax, n_points=P, det=det)
            r = ops.trilinear_backward(v, ss, tt, L, g, amin, amax, n_points=P, want_volume=True, det=det)
            return out, r["g_source"], r["g_target"], r["g_volume"]

        full = march(vol, s, t)
        parts = [march(vol[k0:k1], *_shift(s, t, k0)) for k0, k1 in slabs]
        what = "bricks" if bricks else "per-ray"
        assert rel_err(sum(p[0] for p in parts).cpu(), full[0].cpu()) < GATE, what
        if not bricks:
            # (the interpolant's gradient jumps at every cell face, and a sample x = s + alpha d of a
            # shifted ray rounds differently: a ray with one of its 600 samples within rounding of a face
            # differs by that jump -- 0.3 % of the rays at shape A, 0.6 % at B, by up to 7 % of the
            # largest ray gradient; every other ray agrees to 1e-4 of it)
            for k in (1, 2):
                err = (sum(p[k] for p in parts) - full[k]).abs().amax(-1) / full[k].abs().max()
                assert float((err > 1e-4).float().mean()) < 2e-2, (k, float(err.max()))
                assert float(err.max()) < 0.2, k
        assert rel_err(torch.cat([p[3] for p in parts]).cpu(), full[3].cpu()) < VOL_GATE, what
        del full, parts
        torch.cuda.empty_cache()
    del vol
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------ DRR module

def _drr_pair(vol, lo, hi, **kw):
    spacing = (0.5, 0.5, 0.5)
    A = centered_affine(vol.shape, spacing)
    Ac = A.copy()
    Ac[:3, 3] += A[:3, :3] @ np.asarray(lo, dtype=np.float64)
    crop = vol[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]].contiguous()
    # a field that takes in the whole volume: every block is on the detector
    geo = dict(sdd=1020.0, height=128, delx=8.0, **kw)
    torch.manual_seed(11)  # (p_subsample: the same pixels for both)
    full = DRR(make_subject(vol, spacing, "AP", affine=A), **geo).cuda()
    torch.manual_seed(11)
    small = DRR(make_subject(crop, spacing, "AP", affine=Ac), **geo).cuda()
    return full, small


# Oblique poses.  A Siddon pose gradient sums, over the crossings of axis a, terms with 1 / d_a: a ray
# nearly parallel to a voxel plane (the central rays of a pose near AP) gains or loses a crossing, and
# a term of any size, with a shift of 1e-4 voxel -- and the crop's voxel rays round differently.
ROT = [[0.45, 0.35, -0.5], [-0.4, 0.5, 0.45]]
XYZ = [[0.0, 850.0, 0.0], [4.0, 845.0, 3.0]]


def test_drr_module_above_2_30_voxels(scene_a):
    vol, lo, hi = scene_a["vol"], scene_a["lo"], scene_a["hi"]
    full, small = _drr_pair(vol, lo, hi)
    rot, xyz = torch.tensor(ROT, device="cuda"), torch.tensor(XYZ, device="cuda")
    with torch.no_grad():
        a = full(rot, xyz, parameterization="euler_angles", convention="ZXY")
        b = small(rot, xyz, parameterization="euler_angles", convention="ZXY")
    assert b.abs().max() > 0
    assert rel_err(_img(a), _img(b)) < GATE
    # one differentiable Euler step and DRR.ncc: the brick route (the fused Euler / NCC kernels) against
    # the per-ray route (Off64 walkers) on the same full volume and the same rays.  (Not against the crop:
    # a Siddon pose gradient sums terms with 1 / d_a over the crossings of axis a, and the crop's voxel
    # rays, rounded differently, gain or lose crossings of planes they nearly touch.)
    fixed = b.detach()[:1].flip(-1) + 0.1  # (not a pose's own image: no pose sits at the optimum)
    res = []
    for path in ("bricks", "per-ray"):
        full.renderer.grid_path = path
        r, x = rot.clone().requires_grad_(), xyz.clone().requires_grad_()
        full(r, x, parameterization="euler_angles", convention="ZXY").sum().backward()
        r2, x2 = rot.clone().requires_grad_(), xyz.clone().requires_grad_()
        v = full.ncc(fixed, r2, x2, convention="ZXY")
        v.sum().backward()
        res.append((r.grad, x.grad, v.detach(), r2.grad, x2.grad))
    full.renderer.grid_path = "bricks"
    # (1e-2: the allowance of tests/test_gpu_gradient_routes.py for Siddon pose gradients of two routes)
    for p, q in zip(*res):
        assert rel_err(p.cpu(), q.cpu()) < 1e-2
    # the NCC values against the crop's
    with torch.no_grad():
        assert rel_err(full.ncc(fixed, rot, xyz, convention="ZXY").cpu(),
                       small.ncc(fixed, rot, xyz, convention="ZXY").cpu()) < 1e-3
    del full, small
    torch.cuda.empty_cache()


@pytest.mark.parametrize("lever", [dict(patch_size=40), dict(p_subsample=0.3)])
def test_drr_levers_on_the_bricks_above_2_30_voxels(scene_a, lever):
    vol, lo, hi = scene_a["vol"], scene_a["lo"], scene_a["hi"]
    full, small = _drr_pair(vol, lo, hi, **lever)
    out = []
    for drr in (full, small):
        torch.manual_seed(12)  # (the same subsample for both)
        r = torch.tensor(ROT, device="cuda").requires_grad_()
        x = torch.tensor(XYZ, device="cuda").requires_grad_()
        img = drr(r, x, parameterization="euler_angles", convention="ZXY")
        img.square().sum().backward()
        out.append((img.detach(), r.grad, x.grad))
    assert out[1][0].abs().max() > 0
    assert rel_err(_img(out[0][0]), _img(out[1][0])) < GATE
    for p, q in zip(out[0][1:], out[1][1:]):
        assert rel_err(p.cpu(), q.cpu()) < 1e-3
    del full, small
    torch.cuda.empty_cache()


def test_capped_routes_refuse_before_launch(scene_a):
    vol, s, t, L = scene_a["vol"], scene_a["s"], scene_a["t"], scene_a["L"]
    labels = torch.zeros(vol.shape, dtype=torch.uint8, device=vol.device)
    with pytest.raises(RuntimeError, match="2\\^30"):
        ops.siddon_forward_channels(vol, labels, 1, s, t, L)
    with pytest.raises(RuntimeError, match="2\\^30"):
        ops.siddon_segments(vol, s, t, L)
    del labels
    torch.cuda.empty_cache()


def test_peak_memory_of_a_brick_forward(scene_a):
    """The first q16p forward of a volume, the build of its packed copy included, allocates at most
    5 % of volume + packed copy beyond the two."""
    vol = scene_a["vol"].clone()  # (a tensor no earlier case has rendered: no workspace yet)
    s, t, L = scene_a["s"], scene_a["t"], scene_a["L"]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    ops.siddon_forward_bricks(vol, s, t, L, DET, storage="q16p")
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before  # everything the first forward allocated
    ws, _ = ops.brick_workspace(vol, "q16p")
    vol_bytes, ws_bytes = vol.numel() * 4, ws.numel() * ws.element_size()
    assert ws_bytes < 0.55 * vol_bytes  # the packed copy: +52 % of the volume
    assert vol_bytes + peak <= 1.05 * (vol_bytes + ws_bytes)
    del vol, ws
    torch.cuda.empty_cache()
