"""The length classes of the forward + record brick kernel (csrc/brick_shared.h kRecordGroup,
kRecordAlign) only decide which batch walks a hit: whatever the run width and the row alignment, the
image and the float record stay what the per-ray kernel and the float64 oracle give.  Small shapes at
which the bookkeeping can still go wrong -- two ragged bricks per axis, detector widths that are and
are not multiples of the run width, a pose with exact ties, one whose rays mostly miss, every brick
storage -- and one launch of 33 poses (two chunks of the pose table) through ``DRR.ncc``.

The bounds are those of tests/test_gpu_parity.py test_brick_kernel_small_and_ragged_volumes and
test_q16_bricks_small_ragged_sparse_and_many_poses: images against the oracle FWD_TOL, against the
per-ray kernel 2e-5, d / d img 2e-5, per-pose sums of the ray gradients 5e-3 (max |a - b| / max |b|);
and those of conftest.check_fused_ncc_step: values 2e-6, pose gradients 2e-4.

Each body runs on the host emulation of the kernel cores (the same headers, compiled for the CPU; it
walks hit by hit, so it checks the references and the shapes) and, marked ``gpu``, on the device."""
import numpy as np
import pytest
import torch

import oracle
from conftest import rel_err
from diffdrr_amd import DRR, NormalizedCrossCorrelation2d, convert
from diffdrr_amd.data import make_subject, synthetic_subject

FWD_TOL = 1e-4  # tests/test_gpu_parity.py
DIMS = (40, 36, 70)  # two ragged bricks per axis: 32^3 (fp32) and 32 x 32 x 64 (16-bit)
DETS = [(21, 19), (24, 20)]  # (H, W): a width that is no multiple of 8 or 4, and one of 4
STORAGES = ["f32", "q16", "q16p"]
# exactly axis-aligned (ties: the central rays run inside voxel planes), oblique, mostly beside the volume
# (poses 1 and 2 were kept from a handful of candidates because no ray of theirs has two crossings
# that fp32 cannot order -- the two kernels' ray gradients agree to 1e-6 on the host emulation; with
# one such ray, as at (0.6, -0.4, 0.9), the per-pose sums move by 2e-3 to 9e-3 with the tie)
ROT = [[0.0, 0.0, 0.0], [0.55, -0.35, 0.8], [0.1, 0.05, -0.2]]
XYZ = [[0.0, 250.0, 0.0], [3.0, 245.0, -5.0], [27.0, 250.0, 5.0]]

_scenes = {}


def scene(ops, device, det):
    """The rays of the three poses, the oracle's float64 results and the per-ray kernel's image and
    record: computed once per device and detector, shared by the storages, never written to."""
    key = (str(device), det)
    if key not in _scenes:
        H, W = det
        vol = torch.rand(*DIMS, generator=torch.Generator().manual_seed(7))
        drr = DRR(make_subject(vol), sdd=400.0, height=H, width=W, delx=1.5).to(device)
        rot, xyz = torch.tensor(ROT, device=device), torch.tensor(XYZ, device=device)
        with torch.no_grad():
            pose = convert(rot, xyz, parameterization="euler_angles", convention="ZXY")
            source, target = drr.detector(pose, None)
            L = (target - source).norm(dim=-1).contiguous()
            s, t = drr.affine_inverse(source).contiguous(), drr.affine_inverse(target).contiguous()
        go = torch.rand(len(ROT), H * W, generator=torch.Generator().manual_seed(0)).to(device)
        # (a source per ray: the oracle then returns d / d source per ray, as the kernels do)
        o = oracle.siddon(drr.density.double().cpu().numpy(), s.double().expand_as(t).cpu().numpy(), t.double().cpu().numpy(),
                          L.double().cpu().numpy(), grad_out=go.double().cpu().numpy())
        ref, aux_ref, _ = ops.siddon_forward(drr.density, s, t, L, want_aux=True, det=(H, W))
        g_ref = ops.siddon_backward_rays(aux_ref, go, s, t, L)
        through = (o["out"].reshape(len(ROT), -1) > 0).mean(1)
        assert through[0] == 1.0 and through[1] > 0.5 and 0.0 < through[2] < 0.5, through
        _scenes[key] = (drr, s, t, L, go, o, ref, g_ref)
    return _scenes[key]


def check_record_grouping(ops, device, det, storage):
    H, W = det
    drr, s, t, L, go, o, ref, g_ref = scene(ops, device, det)
    B, V = len(ROT), drr.density
    out, aux = ops.siddon_forward_bricks(V, s, t, L, (H, W), want_aux=True, storage=storage)
    assert aux.shape == (-(-B * H * W // 16), 80)
    want = o["out"].reshape(B, -1)
    e_o, e_r = rel_err(out.cpu().numpy(), want), rel_err(out.cpu().numpy(), ref.cpu().numpy())
    print(f"{storage} {H}x{W}: image vs oracle {e_o:.3e}, vs per-ray kernel {e_r:.3e}")
    assert e_o < FWD_TOL and e_r < 2e-5
    # plane I of the record times the ray's length is the image; the other four through the ray
    # gradients they give
    plane_i = ops.record_planes(aux, B, H * W)[0] * L.reshape(B, -1)
    assert rel_err(plane_i.cpu().numpy(), want) < FWD_TOL and rel_err(plane_i.cpu().numpy(), ref.cpu().numpy()) < 2e-5
    g = ops.siddon_backward_rays(aux, go, s, t, L)
    e_i = rel_err(g[2].cpu().numpy(), g_ref[2].cpu().numpy())
    e_io = rel_err(g[2].cpu().numpy(), o["g_img"].reshape(B, -1))
    print(f"{storage} {H}x{W}: d / d img vs per-ray record {e_i:.3e}, vs oracle {e_io:.3e}")
    assert e_i < 2e-5 and e_io < FWD_TOL
    # The ray gradients without pose 0, as tests/test_gpu_parity.py test_brick_kernel_equals_generic_walk
    # compares them ("pose 0: on a symmetry plane, exact ties"): its source sits on the volume's axis,
    # so a ray through a diagonal pixel meets an x plane and a z plane at the same alpha at every step
    # and the centre row and column run inside voxel planes.  Which voxel lies between two tied
    # crossings is decided by the last bit of each walk's quotients, S0 / S1 jump with it, and the
    # per-ray kernel, the brick kernel and float64 each decide their own way (measured on the host
    # emulation, 21 x 19: the sums differ by twice their size).  Pose 0's image and d / d img, which
    # do not depend on the order of tied crossings, are compared above like any other's.
    sums = [a[1:].double().sum(1).cpu().numpy() for a in g[:2]]
    sums_ref = [a[1:].double().sum(1).cpu().numpy() for a in g_ref[:2]]
    sums_o = [o[k].reshape(B, -1, 3)[1:].sum(1) for k in ("g_source", "g_target")]
    for name, a, b, c in zip(("g_source", "g_target"), sums, sums_ref, sums_o):
        print(f"{storage} {H}x{W}: per-pose {name} vs per-ray record {rel_err(a, b):.3e}, vs oracle {rel_err(a, c):.3e}")
        assert rel_err(a, b) < 5e-3 and rel_err(a, c) < 5e-3, name


def check_ncc_two_chunks(device):
    """33 poses in one fused launch (more than one chunk of the brick kernel's pose table), 64^3 ->
    40 x 40: ``DRR.ncc`` against the composition, the bounds of conftest.check_fused_ncc_step."""
    H = W = 40
    B = 33
    drr = DRR(synthetic_subject(64, kind="phantom", seed=3), sdd=500.0, height=H, width=W, delx=2.0).to(device)
    g = torch.Generator().manual_seed(5)
    rot0 = ((torch.rand(B, 3, generator=g) - 0.5) * 1.0).to(device)
    xyz0 = (torch.tensor([0.0, 305.0, 0.0]) + (torch.rand(B, 3, generator=g) - 0.5) * 16.0).to(device)
    w = (torch.rand(B, generator=g) * 2.0 - 1.0).to(device)
    with torch.no_grad():
        fixed = drr(torch.zeros(1, 3, device=device), torch.tensor([[0.0, 305.0, 0.0]], device=device),
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


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("det", DETS, ids=lambda d: f"{d[0]}x{d[1]}")
def test_record_against_per_ray_kernel_and_oracle_emulated(emulated_ops, det, storage):
    check_record_grouping(emulated_ops, "cpu", det, storage)


def test_ncc_step_of_33_poses_emulated(emulated_ops):
    check_ncc_two_chunks("cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("det", DETS, ids=lambda d: f"{d[0]}x{d[1]}")
def test_record_against_per_ray_kernel_and_oracle(gpu, det, storage):
    from diffdrr_amd import ops

    check_record_grouping(ops, gpu, det, storage)


@pytest.mark.gpu
def test_ncc_step_of_33_poses(gpu):
    check_ncc_two_chunks(gpu)


def test_model_of_the_run_width():
    """tools/record_requests.py, the CPU model behind profiles/r08/record_grouping.txt: whatever the run
    width, every hit is walked exactly once; classes per hit never put a hit into a longer class than
    classes per run do, so the batches' wave-steps do not grow; rows align to the width asked for."""
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tools import record_requests as rr

    rng = np.random.default_rng(3)
    units, steps_of = [], {}
    for u in range(48):
        ray = np.arange(u * 64, u * 64 + 64)
        hit = rng.random(64) < 0.8
        n_est = rng.uniform(2.0, 70.0, 64).astype(np.float32)
        units.append((ray, hit, n_est))
        steps_of.update(zip(ray[hit].tolist(), (n_est[hit] + 2).tolist()))
    steps = {}
    for group in (8, 4, 2, 1):
        batches, _, _, hits = rr.brick_batches(units, group=group)
        walked = sorted(r for bt in batches for r in bt)
        assert walked == sorted(steps_of) and hits == len(steps_of), group
        assert all(len(bt) <= 64 for bt in batches)
        steps[group] = rr.walk_steps(batches, steps_of)[0]
    assert steps[1] < steps[2] < steps[4] < steps[8], steps
    assert rr.align_pixbox_rows((3, 9, 13, 18), 30) == (3, 9, 8, 23)
    assert rr.align_pixbox_rows((3, 9, 13, 18), 30, 4) == (3, 9, 12, 19)
    assert rr.align_pixbox_rows((3, 9, 13, 29), 30, 4) == (3, 9, 12, 29)  # (clipped to the detector)
    assert rr.align_pixbox_rows((3, 9, 13, 18), 30, 1) == (3, 9, 13, 18)
