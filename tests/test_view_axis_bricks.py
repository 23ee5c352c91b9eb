"""The 16-bit bricks whose long axis is y (32 x 64 x 32: include/diffdrr_hip.h DDRR_BRICKS_Q16_Y /
_PACKED_Y, ``Siddon.brick_axis``): another brick grid, fp32 halves along y, a workspace of its own and its
own run width of the record's length classes -- the image and the float record stay what the per-ray
kernel and the float64 oracle give, on any view.

Comparisons and bounds are those of tests/test_record_grouping.py (which has them from
tests/test_gpu_parity.py): images against the oracle FWD_TOL = 1e-4, against the per-ray kernel 2e-5,
d / d img 2e-5, per-pose sums of the ray gradients 5e-3 (max |a - b| / max |b|) without the axis-aligned
pose 0 (exact ties, see there) and with every other; ``DRR.ncc`` against the composition: values 2e-6, pose
gradients 2e-4.  Shapes: two ragged y-long bricks per axis (40 x 70 x 36, 33 x 65 x 33) and two full ones
along the long axis (32 x 128 x 32); detectors whose width is and is not a multiple of the run width."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import oracle
from conftest import rel_err
from diffdrr_amd import DRR, NormalizedCrossCorrelation2d, convert
from diffdrr_amd.data import centered_affine, make_subject, synthetic_subject

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD_TOL = 1e-4  # tests/test_gpu_parity.py
VOLUMES = [(40, 70, 36), (33, 65, 33), (32, 128, 32)]
DETS = [(21, 19), (32, 32)]
Y_STORAGES = ["q16y", "q16py"]
# axis-aligned (exact ties), oblique, mostly beside the volume (tests/test_record_grouping.py), and a view
# along z: the wrong axis for the shape.  (The last was kept from a dozen candidates by the REFERENCES alone:
# on the device the per-ray kernel's per-pose sums of the ray gradients agree with float64's to 1e-6 on
# all six scenes below.  With e.g. (0.3, 1.3, 0.2) / (2, 250, -3) the per-ray kernel itself is 2e-2 from
# float64 on 40 x 70 x 36 -> 32 x 32 -- a ray with two crossings that fp32 cannot order, see
# tests/test_record_grouping.py -- and so are the z-long and the y-long bricks, each its own way.)
ROT = [[0.0, 0.0, 0.0], [0.55, -0.35, 0.8], [0.1, 0.05, -0.2], [0.1, 1.22, 0.62]]
XYZ = [[0.0, 250.0, 0.0], [3.0, 245.0, -5.0], [27.0, 250.0, 5.0], [-1.0, 253.0, -4.0]]


def lds_image_bytes(bx, by, bz):
    """csrc/bricks_fwd.hip FwdCfg::BRICK_BYTES of a 16-bit brick: rows and planes padded by one voxel."""
    sy = bz * 2 + 2
    sx = by * sy + 2
    return (bx * sx + 15) // 16 * 16


def n_bricks(dims, brick):
    return math.prod(-(-d // b) for d, b in zip(dims, brick))


# ----------------------------------------------------------------------------- no device needed

@pytest.mark.parametrize("dims", [(40, 70, 36), (33, 65, 33), (512, 512, 512)])
def test_workspace_bytes_follow_the_storage_shape(dims):
    from diffdrr_amd import _lib, ops

    q = lambda s: int(ops._query("ddrr_brick_workspace_bytes", *dims, s))  # noqa: E731
    assert q(_lib.BRICKS_F32) == 0
    assert q(_lib.BRICKS_Q16_Y) == q(_lib.BRICKS_Q16) > 0  # header, (min, max), flags, fingerprint: any grid fits
    assert q(_lib.BRICKS_Q16_PACKED) - q(_lib.BRICKS_Q16) == n_bricks(dims, (32, 32, 64)) * lds_image_bytes(32, 32, 64)
    assert q(_lib.BRICKS_Q16_PACKED_Y) - q(_lib.BRICKS_Q16_Y) == n_bricks(dims, (32, 64, 32)) * lds_image_bytes(32, 64, 32)
    assert (_lib.BRICKS_Q16_Y, _lib.BRICKS_Q16_PACKED_Y) == (3, 4)
    assert ops._BRICK_STORAGE["q16y"] == 3 and ops._BRICK_STORAGE["q16py"] == 4


def test_auto_takes_the_view_axis():
    from diffdrr_amd import renderers
    from diffdrr_amd.renderers import _brick_axis, _resolve_brick_axis

    vol = torch.rand(40, 70, 36)
    for orientation in ("AP", "PA"):
        drr = DRR(make_subject(vol, orientation=orientation), sdd=400.0, height=16, delx=2.0)
        assert drr.renderer.brick_axis == "auto" and drr.renderer.view_axis == "y"
        cfg = drr.renderer._cfg(False)
        assert cfg["brick_axis"] == "auto" and cfg["view_axis"] == "y"
        assert _brick_axis(drr.density, cfg) == "z"  # a CPU tensor: never changed
    # an affine that permutes the voxel axes: the view falls on z, or on x
    A = np.asarray(centered_affine(vol.shape, (1.0, 1.0, 1.0)), dtype=np.float64)
    for perm, axis in (([0, 2, 1], "z"), ([1, 0, 2], "x")):
        P = np.eye(4)
        P[:3, :3] = np.eye(3)[perm]  # world y is spanned by voxel axis z (x)
        drr = DRR(make_subject(vol, affine=A @ P), sdd=400.0, height=16, delx=2.0)
        assert drr.renderer.view_axis == axis
    big, cus = (512, 512, 512), 256
    want = "y" if renderers.VIEW_AXIS_AUTO else "z"
    assert _resolve_brick_axis("auto", "y", big, cus) == want
    # ... from the measured pose count on (few poses per launch: the z-long bricks are faster)
    assert renderers.VIEW_AXIS_MIN_POSES == 16
    assert _resolve_brick_axis("auto", "y", big, cus, 32) == _resolve_brick_axis("auto", "y", big, cus, 16) == want
    assert _resolve_brick_axis("auto", "y", big, cus, 1) == _resolve_brick_axis("auto", "y", big, cus, 15) == "z"
    assert _resolve_brick_axis("y", "y", big, cus, 1) == "y"
    assert _resolve_brick_axis("auto", "z", big, cus) == "z" and _resolve_brick_axis("auto", "x", big, cus) == "z"
    assert _resolve_brick_axis("auto", None, big, cus) == "z"
    # fewer than 4 double bricks per CU (the storage table's regime): 512 x 512 x 133 has 3.1
    assert _resolve_brick_axis("auto", "y", (512, 512, 133), cus) == "z"
    assert _resolve_brick_axis("auto", "y", (256, 256, 256), cus) == "z"
    # explicit settings win, whatever the view and the size
    for view in ("x", "y", "z", None):
        assert _resolve_brick_axis("y", view, (64, 64, 64), cus) == "y"
        assert _resolve_brick_axis("z", view, big, cus) == "z"
    with pytest.raises(ValueError):
        _resolve_brick_axis("x", "y", big, cus)


def test_host_route_keeps_the_z_long_bricks(emulated_ops):
    """A CPU tensor (the host emulation of the kernels) is rendered from the z-long bricks whatever the
    module asks for: same image, and the workspace in use is the z-long one."""
    ops = emulated_ops
    drr = DRR(make_subject(torch.rand(40, 70, 36, generator=torch.Generator().manual_seed(1))), sdd=400.0,
              height=12, width=11, delx=2.5)
    rot, xyz = torch.tensor(ROT[1:2]), torch.tensor(XYZ[1:2])
    imgs = []
    for axis in ("auto", "y", "z"):
        drr.renderer.brick_axis = axis
        with torch.no_grad():
            imgs.append(drr(rot, xyz, parameterization="euler_angles", convention="ZXY").clone())
    assert torch.equal(imgs[0], imgs[2]) and torch.equal(imgs[1], imgs[2])
    assert ops._workspace_entry(drr.density, "q16py") is None and ops._workspace_entry(drr.density, "q16y") is None
    source, target = drr.detector(convert(rot, xyz, parameterization="euler_angles", convention="ZXY"), None)
    s, t = drr.affine_inverse(source).contiguous(), drr.affine_inverse(target).contiguous()
    L = (target - source).norm(dim=-1).contiguous()
    a, _ = ops.siddon_forward_bricks(drr.density, s, t, L, (12, 11), storage="q16", axis="y")
    b, _ = ops.siddon_forward_bricks(drr.density, s, t, L, (12, 11), storage="q16", axis="z")
    assert torch.equal(a, b) and ops._workspace_entry(drr.density, "q16y") is None


def test_model_counts_hits_and_batches_of_y_long_bricks():
    """tools/record_requests.py --brick 32,64,32 at 64 x 128 x 64 -> 32^2, 3 poses, every brick: its hits
    are the candidates of a brute-force pass over ALL pixels of every (pose, brick) pair (the projected,
    aligned pixel box loses none), and a brick's batches are ceil(hits / 64): full batches of 64 from the
    class queues, the rest pooled and cut into 64s."""
    sys.path.insert(0, ROOT)
    from tools import record_requests as rr

    D, H, B = 64, 32, 3
    src, tgt = rr.bench_rays(B, D, H)
    dims, brick = (D, 2 * D, D), (32, 64, 32)
    r = rr.model(src, tgt, dims, H, H, every=1, group=2, align=2, brick=brick)
    assert r["sampled_bricks"] == r["bricks"] == 8
    grids = [rr.pose_grid(src[b], tgt[b], H, H) for b in range(B)]
    hits = batches = 0
    for bx in range(2):
        for by in range(2):
            for bz in range(2):
                lo = [bx * 32, by * 64, bz * 32]
                hi = [lo[0] + 32, lo[1] + 64, lo[2] + 32]
                n = sum(int(rr.brick_candidates(g, (0, H - 1, 0, H - 1), lo, hi, H)[1].sum()) for g in grids)
                hits += n
                batches += -(-n // 64)
    assert hits > 1000 and r["hits"] == hits and r["batches"] == batches
    # the z-long default is what it was
    z = rr.model(src, tgt, dims, H, H, every=1, group=4, align=4)
    assert z["bricks"] == 8 and z["hits"] != r["hits"]


def test_run_width_constants_of_both_configurations():
    """csrc/brick_shared.h: the z-long product keeps 4 | 4 and 22 / 48; the y-long one has its own run
    width, alignment (4 | 4 as well) and thresholds (26 / 56), and FwdCfg takes them by the axis of its halves."""
    shared = open(os.path.join(ROOT, "diffdrr_amd", "csrc", "brick_shared.h")).read()
    fwd = open(os.path.join(ROOT, "diffdrr_amd", "csrc", "bricks_fwd.hip")).read()
    product = shared.split("#else")  # (the tools-build overrides stand in front of each #else)
    m = re.search(r"constexpr int kRecordGroup = (\d), kRecordGroupY = (\d);", product[1])
    a = re.search(r"constexpr int kRecordAlign = (\d), kRecordAlignY = (\d);", product[2])
    t = re.search(r"constexpr float kBrickT1Y = ([\d.]+)f, kBrickT2Y = ([\d.]+)f;", shared)
    assert m and a and t
    assert (int(m.group(1)), int(a.group(1))) == (4, 4)
    assert (int(m.group(2)), int(a.group(2))) == (4, 4)  # (chosen by the clock: profiles/r09/view_axis_bricks.txt)
    assert (float(t.group(1)), float(t.group(2))) == (26.0, 56.0)
    assert "DDRR_RECORD_GROUP" in product[0] and "DDRR_RECORD_ALIGN" in product[1]  # the tools overrides
    assert "RECORD_GROUP = HAXIS == 1 ? kRecordGroupY : kRecordGroup" in fwd
    assert "RECORD_ALIGN = HAXIS == 1 ? kRecordAlignY : kRecordAlign" in fwd
    assert "T1 = DOUBLE_Q16 ? (HAXIS == 1 ? kBrickT1Y : 22.f) : 18.f" in fwd
    assert "T2 = DOUBLE_Q16 ? (HAXIS == 1 ? kBrickT2Y : 48.f) : 40.f" in fwd
    assert "using CfgQ16Y64 = FwdCfg<32, 64, 32, 1024, true>;" in fwd.split("#if defined(DDRR_EXPERIMENTS) || defined(DDRR_BRICK_PROFILE)\nusing")[0]


# ----------------------------------------------------------------------------- on the device

_scenes = {}


def scene(ops, device, dims, det, spike=None):
    """Rays of the four poses, the oracle's float64 results and the per-ray kernel's image and record:
    computed once per device, volume and detector, shared by the tests, never written to."""
    key = (str(device), dims, det, spike)
    if key not in _scenes:
        H, W = det
        vol = torch.rand(*dims, generator=torch.Generator().manual_seed(7))
        if spike is not None:
            vol = 0.2 + 0.1 * vol
            vol[spike] = 6.0  # (range = 23 x the brick level, the guard stops at 12 x: brick_step.h q16_usable)
        drr = DRR(make_subject(vol), sdd=400.0, height=H, width=W, delx=1.5).to(device)
        rot, xyz = torch.tensor(ROT, device=device), torch.tensor(XYZ, device=device)
        with torch.no_grad():
            pose = convert(rot, xyz, parameterization="euler_angles", convention="ZXY")
            source, target = drr.detector(pose, None)
            L = (target - source).norm(dim=-1).contiguous()
            s, t = drr.affine_inverse(source).contiguous(), drr.affine_inverse(target).contiguous()
        go = torch.rand(len(ROT), H * W, generator=torch.Generator().manual_seed(0)).to(device)
        o = oracle.siddon(drr.density.double().cpu().numpy(), s.double().expand_as(t).cpu().numpy(),
                          t.double().cpu().numpy(), L.double().cpu().numpy(), grad_out=go.double().cpu().numpy())
        ref, aux_ref, _ = ops.siddon_forward(drr.density, s, t, L, want_aux=True, det=(H, W))
        g_ref = ops.siddon_backward_rays(aux_ref, go, s, t, L)
        through = (o["out"].reshape(len(ROT), -1) > 0).mean(1)
        d = (t[:, (H // 2) * W + W // 2] - s[:, 0]).abs()
        assert through[0] == 1.0 and through[1] > 0.4 and 0.0 < through[2] < 0.6 and through[3] > 0.4, through
        assert int(d[3].argmax()) == 2 and int(d[0].argmax()) == 1, d  # pose 3 looks along z
        _scenes[key] = (drr, s, t, L, go, o, ref, g_ref)
    return _scenes[key]


def check_image(out, o, ref, B, what):
    want = o["out"].reshape(B, -1)
    e_o, e_r = rel_err(out.cpu().numpy(), want), rel_err(out.cpu().numpy(), ref.cpu().numpy())
    print(f"{what}: image vs oracle {e_o:.3e}, vs per-ray kernel {e_r:.3e}")
    assert e_o < FWD_TOL and e_r < 2e-5


def check_forward_and_record(ops, device, dims, det, storage, spike=None):
    H, W = det
    drr, s, t, L, go, o, ref, g_ref = scene(ops, device, dims, det, spike)
    B, V = len(ROT), drr.density
    what = f"{storage} {dims} {H}x{W}"
    fwd, none = ops.siddon_forward_bricks(V, s, t, L, (H, W), storage=storage)
    assert none is None
    check_image(fwd, o, ref, B, what + " forward only")
    out, aux = ops.siddon_forward_bricks(V, s, t, L, (H, W), want_aux=True, storage=storage)
    assert aux.shape == (-(-B * H * W // 16), 80)
    check_image(out, o, ref, B, what + " with the record")
    want = o["out"].reshape(B, -1)
    plane_i = ops.record_planes(aux, B, H * W)[0] * L.reshape(B, -1)
    assert rel_err(plane_i.cpu().numpy(), want) < FWD_TOL and rel_err(plane_i.cpu().numpy(), ref.cpu().numpy()) < 2e-5
    g = ops.siddon_backward_rays(aux, go, s, t, L)
    e_i = rel_err(g[2].cpu().numpy(), g_ref[2].cpu().numpy())
    e_io = rel_err(g[2].cpu().numpy(), o["g_img"].reshape(B, -1))
    print(f"{what}: d / d img vs per-ray record {e_i:.3e}, vs oracle {e_io:.3e}")
    assert e_i < 2e-5 and e_io < FWD_TOL
    # the ray gradients without pose 0 (exact ties: tests/test_record_grouping.py) and with every other
    sums = [a[1:].double().sum(1).cpu().numpy() for a in g[:2]]
    sums_ref = [a[1:].double().sum(1).cpu().numpy() for a in g_ref[:2]]
    sums_o = [o[k].reshape(B, -1, 3)[1:].sum(1) for k in ("g_source", "g_target")]
    for name, a, b, c in zip(("g_source", "g_target"), sums, sums_ref, sums_o):
        print(f"{what}: per-pose {name} vs per-ray record {rel_err(a, b):.3e}, vs oracle {rel_err(a, c):.3e}")
        assert rel_err(a, b) < 5e-3 and rel_err(a, c) < 5e-3, name
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("storage", Y_STORAGES)
@pytest.mark.parametrize("det", DETS, ids=lambda d: f"{d[0]}x{d[1]}")
@pytest.mark.parametrize("dims", VOLUMES, ids=lambda d: "x".join(map(str, d)))
def test_forward_and_record_against_per_ray_kernel_and_oracle(gpu, dims, det, storage):
    from diffdrr_amd import ops

    check_forward_and_record(ops, gpu, dims, det, storage)
    drr = scene(ops, gpu, dims, det)[0]
    assert ops.brick_fallbacks(drr.density, storage) == (0, n_bricks(dims, (32, 64, 32)))


@pytest.mark.gpu
@pytest.mark.parametrize("storage", Y_STORAGES)
@pytest.mark.parametrize("spike", [(5, 9, 7), (36, 68, 34)], ids=["first", "ragged_last"])
def test_spiked_brick_takes_the_fp32_halves_along_y(gpu, spike, storage):
    """One voxel of 6 among 0.2 ... 0.3: the guard sends its brick -- the full first one (two halves
    along y), or the ragged last one, 8 x 6 x 4 voxels (one half) -- to the fp32 path."""
    from diffdrr_amd import ops

    dims, det = (40, 70, 36), (21, 19)
    check_forward_and_record(ops, gpu, dims, det, storage, spike)
    assert ops.brick_fallbacks(scene(ops, gpu, dims, det, spike)[0].density, storage) == (1, 8)


@pytest.mark.gpu
@pytest.mark.parametrize("poses", [1, 9])
def test_few_poses_and_a_pixel_mask(gpu, poses):
    """1 pose (the PRE instantiation, with the look-ahead on the packed storage) and 9 (the other), all
    pixels and a subsample of them (SUB), forward only and with the record."""
    from diffdrr_amd import ops

    dims, (H, W) = (40, 70, 36), (21, 19)
    drr, s, t, L, go, o, ref, g_ref = scene(ops, gpu, dims, (H, W))
    idx = [(1 + k) % len(ROT) for k in range(poses)]  # (pose 1 first: the oblique one alone at one pose)
    s, t, L, ref = s[idx].contiguous(), t[idx].contiguous(), L[idx].contiguous(), ref[idx]
    want = o["out"].reshape(len(ROT), -1)[idx]
    keep = torch.arange(0, H * W, 3, device=gpu)
    mask = ops.pixel_mask_of(keep, H * W)
    sel = torch.zeros(H * W, dtype=torch.bool, device=gpu)
    sel[keep] = True
    for storage in Y_STORAGES:
        for want_aux in (False, True):
            out, _ = ops.siddon_forward_bricks(drr.density, s, t, L, (H, W), want_aux=want_aux, storage=storage)
            e_o, e_r = rel_err(out.cpu().numpy(), want), rel_err(out.cpu().numpy(), ref.cpu().numpy())
            sub, _ = ops.siddon_forward_bricks(drr.density, s, t, L, (H, W), want_aux=want_aux, storage=storage,
                                               pixel_mask=mask)
            e_s = rel_err(sub[:, sel].cpu().numpy(), ref[:, sel].cpu().numpy())
            print(f"{storage} {poses} poses, record {want_aux}: vs oracle {e_o:.3e}, per-ray {e_r:.3e}, masked {e_s:.3e}")
            assert e_o < FWD_TOL and e_r < 2e-5 and e_s < 2e-5
            assert float(sub[:, ~sel].abs().max()) == 0.0


@pytest.mark.gpu
def test_ncc_step_of_33_poses_on_y_long_bricks(gpu):
    """tests/test_record_grouping.py check_ncc_two_chunks with ``brick_axis`` = "y": 33 poses in one fused
    launch (two chunks of the pose table), 64^3 -> 40 x 40, against the composition on the same bricks."""
    from diffdrr_amd import ops

    H = W = 40
    B = 33
    drr = DRR(synthetic_subject(64, kind="phantom", seed=3), sdd=500.0, height=H, width=W, delx=2.0).to(gpu)
    drr.renderer.brick_axis = "y"
    g = torch.Generator().manual_seed(5)
    rot0 = ((torch.rand(B, 3, generator=g) - 0.5) * 1.0).to(gpu)
    xyz0 = (torch.tensor([0.0, 305.0, 0.0]) + (torch.rand(B, 3, generator=g) - 0.5) * 16.0).to(gpu)
    w = (torch.rand(B, generator=g) * 2.0 - 1.0).to(gpu)
    with torch.no_grad():
        fixed = drr(torch.zeros(1, 3, device=gpu), torch.tensor([[0.0, 305.0, 0.0]], device=gpu),
                    parameterization="euler_angles", convention="ZXY")
    drr.FUSED_NCC_MAX_POSES = B  # (the module stops at 32 for speed, not for correctness)
    res = []
    for fused in (True, False):
        r, x = rot0.clone().requires_grad_(), xyz0.clone().requires_grad_()
        if fused:
            val = drr.ncc(fixed, r, x, convention="ZXY")
            assert type(val.grad_fn).__name__.startswith("_EulerSiddonNccFn")  # the fused route
        else:
            val = NormalizedCrossCorrelation2d()(fixed.expand(B, -1, -1, -1),
                                                 drr(r, x, parameterization="euler_angles", convention="ZXY"))
        (val * w).sum().backward()
        res.append((val.detach().cpu().numpy(), r.grad.cpu().numpy(), x.grad.cpu().numpy()))
    (v1, gr1, gx1), (v0, gr0, gx0) = res
    print(f"ncc 33 poses: values {np.abs(v1 - v0).max():.3e}, gradients {rel_err(gr1, gr0):.3e} {rel_err(gx1, gx0):.3e}")
    assert v1.shape == (B,) and np.abs(v1 - v0).max() < 2e-6
    assert rel_err(gr1, gr0) < 2e-4 and rel_err(gx1, gx0) < 2e-4
    # the module rendered from the y-long packed bricks, and reports them under the storage's name
    assert ops._workspace_entry(drr.density, "q16py") is not None and ops._workspace_entry(drr.density, "q16p") is None
    assert ops.brick_fallbacks(drr.density, "q16p") == ops.brick_fallbacks(drr.density, "q16py")
    assert ops.brick_fallbacks(drr.density, "q16p")[1] == 4


@pytest.mark.gpu
@pytest.mark.parametrize("dims", VOLUMES[:2], ids=lambda d: "x".join(map(str, d)))
def test_y_long_and_z_long_renders_agree_within_both_quantisations(gpu, dims):
    """The same scene from 32 x 64 x 32 and from 32 x 32 x 64 bricks.  A stored voxel is off by at most its
    brick's range / 131070 (include/diffdrr_hip.h); the volume's values lie in [0, 1), so any brick's range
    is below 1, and a ray's integral over a chord of length c (world units; at most the volume's diagonal)
    is off by at most c / 131070 per quantisation.  On top, each kernel's fp32 sum is within 2e-5 of the
    image scale of the per-ray kernel's (the bound above)."""
    from diffdrr_amd import ops

    H, W = 21, 19
    drr, s, t, L, go, o, ref, g_ref = scene(ops, gpu, dims, (H, W))
    y, _ = ops.siddon_forward_bricks(drr.density, s, t, L, (H, W), storage="q16py")
    z, _ = ops.siddon_forward_bricks(drr.density, s, t, L, (H, W), storage="q16p")
    chord = math.sqrt(sum(d * d for d in dims))  # (unit spacing)
    bound = 2.0 * chord / 131070.0 + 2.0 * 2e-5 * float(ref.abs().max())
    diff = float((y - z).abs().max())
    print(f"{dims}: y-long vs z-long {diff:.3e}, bound {bound:.3e}")
    assert diff <= bound
    assert ops.brick_fallbacks(drr.density, "q16p") == (0, n_bricks(dims, (32, 32, 64)))  # (z-long: used last)
    assert ops.brick_fallbacks(drr.density, "q16py") == (0, n_bricks(dims, (32, 64, 32)))


@pytest.mark.gpu
def test_in_place_edit_is_seen_by_the_y_workspace(gpu):
    """``volume.data.mul_`` moves no version counter: the host hands the launch a workspace it believes
    built, and the launch's comparison of the fingerprint renders every brick from the live fp32 values."""
    from diffdrr_amd import Siddon, ops

    H, W = 21, 19
    vol = 0.2 + torch.rand(40, 70, 36, generator=torch.Generator().manual_seed(2))
    drr = DRR(make_subject(vol), sdd=400.0, height=H, width=W, delx=1.5).to(gpu)
    V = drr.density
    with torch.no_grad():
        pose = convert(torch.tensor(ROT[1:3], device=gpu), torch.tensor(XYZ[1:3], device=gpu),
                       parameterization="euler_angles", convention="ZXY")
        source, target = drr.detector(pose, None)
        L = (target - source).norm(dim=-1).contiguous()
        s, t = drr.affine_inverse(source).contiguous(), drr.affine_inverse(target).contiguous()
    render = lambda: ops.siddon_forward_bricks(V, s, t, L, (H, W), storage="q16p", axis="y")[0].clone()  # noqa: E731
    img0 = render()
    assert ops.brick_workspace(V, "q16py")[1] == 1 and ops.brick_workspace_stale(V, "q16py") == 0
    assert ops._workspace_entry(V, "q16p") is None and ops.brick_fallbacks(V, "q16p") == (0, 8)
    version = V._version
    V.data.mul_(2.0)
    assert V._version == version and ops.brick_workspace(V, "q16py")[1] == 1  # the host sees nothing ...
    img1 = render()
    assert rel_err(img1.cpu().numpy(), 2.0 * img0.cpu().numpy()) < 2e-5      # ... the launch does
    assert ops.brick_workspace_stale(V, "q16py") == 1 and ops.brick_workspace_stale(V, "q16p") == 1
    Siddon.volume_changed(V)
    assert ops.brick_workspace(V, "q16py")[1] == 0
    img2 = render()
    assert rel_err(img2.cpu().numpy(), 2.0 * img0.cpu().numpy()) < 2e-5
    assert ops.brick_workspace_stale(V, "q16py") == 0
