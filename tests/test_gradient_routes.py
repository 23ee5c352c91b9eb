"""Every gradient route ``DRR.forward`` can take, and the layout invariance of the public entries.

A. The route matrix: renderer (Siddon, the trilinear marcher) x lever (dense, ``patch_size`` with
   ragged chunks, ``p_subsample`` with ``reshape`` True / False, both levers together) x
   ``mask_to_channels`` x ``stop_gradients_through_grid_sample`` (Siddon) x route (the fused pose
   entry, ``fuse_ray_generation=False``).  Each case backpropagates ``(img * w).sum()`` with a
   random ``w`` over the WHOLE output -- the undrawn pixels of a scattered subsample included --
   and checks
     * image and volume gradient against the fp64 oracle on exactly the rays the reference renders
       (the subsample's rays, chunk by chunk, the marcher's range per chunk; reference
       drr.py:142-147, 218-225), with ``w`` restricted to those rays;
     * the pose gradient against the same module moved ``.to(torch.float64)`` (the f64 kernels,
       the unfused per-chunk loop);
     * the two routes against each other.
B. Layout invariance: a call on strided views (chunks of the rays with B > 1, an expanded source,
   ``[::2]`` volumes and label maps, column slices of the marching range, channel slices of NCC
   inputs, pose parameters sliced out of one (B, 6) leaf) against the same call on
   ``.contiguous()`` copies -- outputs and the gradients of every leaf.  The kernels take raw
   pointers: a wrapper that forgets ``.contiguous()`` reads the wrong memory.

This file runs the host emulation of the kernel cores (conftest ``emulated_ops``), where B demands
bit-equality; tests/test_gpu_gradient_routes.py runs the same checks on the device at a size where
the brick grid matters.
"""
import copy

import numpy as np
import pytest
import torch

import oracle
from conftest import _topk_sum, rel_err
from diffdrr_amd import DRR, Siddon, Trilinear, convert
from diffdrr_amd.data import make_subject, phantom_volume
from diffdrr_amd.metrics import (GradientNormalizedCrossCorrelation2d, MultiscaleNormalizedCrossCorrelation2d,
                                 NormalizedCrossCorrelation2d)

FWD_TOL, GRAD_TOL = 1e-4, 1e-3  # image / gradient against the fp64 oracle
POSE_TOL = 2e-3                  # fp32 pose gradient against the float64 module, fused vs general

# ------------------------------------------------------------------ A. the route matrix

LEVERS = {  # name -> DRR keywords (patch_size: filled in per scene, its chunks are ragged)
    "dense": {},
    "patch": {"patch_size": True},
    "sub": {"p_subsample": True},
    "sub_flat": {"p_subsample": True, "reshape": False},
    "patch_sub": {"patch_size": True, "p_subsample": True},
    "patch_sub_flat": {"patch_size": True, "p_subsample": True, "reshape": False},
}

# (renderer, lever, mask_to_channels, stop_gradients_through_grid_sample)
ROUTE_CASES = [(r, lever, mask, stop)
               for r in ("siddon", "trilinear") for lever in LEVERS for mask in (False, True)
               for stop in ((False, True) if r == "siddon" else (False,))]


def route_case_id(case):
    r, lever, mask, stop = case
    return f"{r}-{lever}" + ("-channels" if mask else "") + ("-stop" if stop else "")


def _labels(dims, n_labels, seed):
    """piecewise-constant labels: coarse random blocks (as data.synthetic_subject)"""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randint(0, n_labels, tuple(max(1, d // 8) for d in dims), generator=g)
    for ax, d in enumerate(dims):
        coarse = coarse.index_select(ax, (torch.arange(d) * coarse.shape[ax] // d).clamp_max(coarse.shape[ax] - 1))
    return coarse


def host_scene():
    """volumes <= 30^3, detectors <= 20^2, B <= 3: 154 pixels, patch 5 -> 6 chunks of 26, 26, 26, 26, 26, 24
    rays (no chunk ends on a detector row); 30 % subsample -> 46 rays, with patches 6 chunks of 8 / 6."""
    dims = (24, 30, 20)
    vol = phantom_volume(dims, seed=3)
    return dict(
        subject=make_subject(vol, (1.0, 1.0, 1.0), "AP", _labels(dims, 5, 4)),
        geo=dict(sdd=300.0, height=14, width=11, delx=2.0), patch_size=5, p_subsample=0.3, n_points=70,
        rot=torch.tensor([[0.2, -0.1, 0.3], [0.0, 0.4, -0.2]]),
        xyz=torch.tensor([[3.0, 210.0, -2.0], [-4.0, 190.0, 5.0]]))


def build_route_drr(scene, renderer, lever, stop, device):
    kw = {}
    for k, v in LEVERS[lever].items():
        kw[k] = scene[k] if v is True else v
    if renderer == "siddon":
        kw["stop_gradients_through_grid_sample"] = stop
    torch.manual_seed(1234)  # (the subsample drawn at construction)
    drr = DRR(scene["subject"], renderer=renderer, **scene["geo"], **kw).to(device)
    drr.density.requires_grad_()
    return drr


def to_float64(drr):
    """the same module in float64 (reference drr.py:71-75), its volume a leaf that takes a gradient"""
    d64 = copy.deepcopy(drr).to(torch.float64)
    d64.density = d64.density.detach().requires_grad_(drr.density.requires_grad)
    return d64


def _render(drr, rot0, xyz0, call, w=None, calls=None, launch_owner=None, one_weight_per_pixel=False):
    """-> (image, rot.grad, xyz.grad, density.grad | None, w): one forward + backward of (img * w).sum();
    ``w`` random over the whole output, or (``one_weight_per_pixel``) random per pixel, the same in
    every channel"""
    dt = drr.density.dtype
    rot = rot0.to(dt).clone().requires_grad_()
    xyz = xyz0.to(dt).clone().requires_grad_()
    drr.density.grad = None
    if calls is not None:
        calls.clear()
        real = launch_owner._launch
        launch_owner._launch = lambda n, d, *a: (calls.append(n), real(n, d, *a))[1]
    try:
        img = drr(rot, xyz, parameterization="euler_angles", convention="ZXY", **call)
        if w is None:
            shape = (img.shape[0], 1) + img.shape[2:] if one_weight_per_pixel else img.shape
            w = torch.rand(shape, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
            w = w.expand(img.shape).contiguous()
        (img * w.to(img)).sum().backward()
    finally:
        if calls is not None:
            launch_owner._launch = real
    g = drr.density.grad
    return img.detach(), rot.grad, xyz.grad, (None if g is None else g.detach().clone()), w


def _np(t):
    return None if t is None else t.detach().cpu().double().numpy()


def oracle_truth(drr, rot, xyz, w, renderer, mask, n_points, want_volume):
    """Image and volume gradient from the fp64 oracle on the rays the reference renders: the
    detector's rays (the subsample's, in its order), cut into the reference's chunks
    (``target.chunk(n_patches, dim=1)``), each chunk one renderer call (the marcher's range over its
    own rays).  ``w`` (the module's output shape) restricted to those rays.  -> (image in the module's
    output layout, volume gradient | None); trilinear channels: the image summed over the channels
    (with one weight per pixel in every channel, the plain march's gradients)."""
    d64 = to_float64(drr)
    det = d64.detector
    with torch.no_grad():
        pose = convert(rot.double().to(d64.device), xyz.double().to(d64.device),
                       parameterization="euler_angles", convention="ZXY")
        src, tgt = det(pose, None)
        L = (tgt - src).norm(dim=-1)
        s, t = d64.affine_inverse(src), d64.affine_inverse(tgt)
    s, t, L = (x.cpu().numpy() for x in (s, t, L))
    B, n = L.shape
    H, W = det.height, det.width
    idx = det.subsample_index()
    idx = None if idx is None else idx.cpu().numpy()
    w = w.cpu().numpy()
    C = w.shape[1]
    # w over the rendered rays, in render order: (B, C, n)
    if idx is not None and drr.reshape:
        w_rays = w.reshape(B, C, H * W)[:, :, idx]
    else:
        w_rays = w.reshape(B, C, n)
    vol = drr.density.detach().cpu().double().numpy()
    labels = None if not mask else drr.mask.cpu().numpy()
    chunks = np.arange(n) if drr.patch_size is None else None
    parts = [chunks] if chunks is not None else [c.numpy() for c in torch.arange(n).chunk(drr.n_patches)]
    out = np.zeros((B, C if renderer == "siddon" else 1, n))
    gv = np.zeros(vol.shape) if want_volume else None
    for c in parts:
        tc, Lc, wc = t[:, c], L[:, c], w_rays[:, :, c]
        if renderer == "siddon" and mask:
            out[:, :, c] = oracle.siddon_channels(vol, labels, s, tc, Lc, n_channels=C)
            if want_volume:
                gv += oracle.siddon_channels_grad(vol, labels, s, tc, Lc, wc)["g_volume"]
        elif renderer == "siddon":
            r = oracle.siddon(vol, s, tc, Lc, grad_out=wc[:, 0], want_volume_grad=want_volume)
            out[:, :, c] = r["out"]
            if want_volume:
                gv += r["g_volume"]
        else:
            # (with channels: the plain march, which the channels sum to)
            r = oracle.trilinear(vol, s, tc, Lc, n_points=n_points, grad_out=wc[:, 0],
                                 want_volume_grad=want_volume)
            out[:, :, c] = r["out"]
            if want_volume:
                gv += r["g_volume"]
    if idx is not None and drr.reshape:
        full = np.zeros((B, out.shape[1], H * W))
        full[:, :, idx] = out
        out = full
    return out, gv


def expected_entries(drr, renderer, fused, mask, stop):
    """(entries the render must have taken, entries it must not have taken)"""
    sub = drr.detector.n_subsample is not None
    patched_general = drr.patch_size is not None and not fused and (renderer == "trilinear" or sub)
    must, must_not = set(), set()
    if fused or not (sub or patched_general):
        # a detector grid: the volume-stationary kernels (the fused route renders the whole grid once)
        per_ray = {"ddrr_siddon_forward", "ddrr_trilinear_forward", "ddrr_siddon_forward_channels",
                   "ddrr_trilinear_forward_channels"}
        must_not |= per_ray
        if renderer == "siddon" and not mask:
            must.add("ddrr_siddon_forward_bricks_masked" if (sub and fused) else "ddrr_siddon_forward_bricks")
            if not stop:
                must.add("ddrr_siddon_backward_volume_bricks")
        elif renderer == "siddon":
            must.add("ddrr_siddon_forward_channels_bricks")
        else:
            must.add("ddrr_trilinear_forward_channels_bricks" if mask else "ddrr_trilinear_forward_bricks")
    else:
        # the reference's chunks / subsample as ray lists: the per-ray kernels and their ray backward
        if renderer == "siddon" and not mask:
            must |= {"ddrr_siddon_forward", "ddrr_siddon_backward_rays"}
            if not stop:
                must.add("ddrr_siddon_backward_volume")
        elif renderer == "siddon":
            must.add("ddrr_siddon_forward_channels")
        else:
            must.add("ddrr_trilinear_forward_channels" if mask else "ddrr_trilinear_forward")
    return must, must_not


def check_route_case(scene, case, device, launch_owner, pose_tol=POSE_TOL):
    """One row of the matrix (both routes).  ``launch_owner``: the module whose ``_launch`` the
    C-ABI calls go through (diffdrr_amd.ops, emulated or not).  The marcher's channels take one weight
    per pixel in every channel: which channel a sample at a label boundary lands in is decided by the
    last bits of its position (the fp32 and fp64 lookups disagree there), while the weighted sum over
    the channels is the plain march -- the oracle's, with no label lookup at all."""
    renderer, lever, mask, stop = case
    drr = build_route_drr(scene, renderer, lever, stop, device)
    call = {"n_points": scene["n_points"]} if renderer == "trilinear" else {}
    if mask:
        call["mask_to_channels"] = True
    rot, xyz = scene["rot"].to(device), scene["xyz"].to(device)
    if mask and drr.detector.n_subsample is not None and drr.reshape:
        # (B, C, n) channels do not scatter into a (B, 1, H, W) grid (index_copy refuses them) -- nor does the reference's
        # `drr[:, idx] = img` (drr.py:142-147) for C > 1: both routes refuse the call
        for fused in (True, False):
            drr.fuse_ray_generation = fused
            with pytest.raises(IndexError):
                _render(drr, rot, xyz, call)
        return
    res, calls = {}, []
    w = None
    for fused in (True, False):
        drr.fuse_ray_generation = fused
        assert drr._fused_ok(mask, {k: v for k, v in call.items() if k != "mask_to_channels"}) == fused
        *res[fused], w = _render(drr, rot, xyz, call, w, calls, launch_owner,
                                 one_weight_per_pixel=renderer == "trilinear" and mask)
        must, must_not = expected_entries(drr, renderer, fused, mask, stop)
        assert must <= set(calls), (fused, sorted(must - set(calls)))
        assert not must_not & set(calls), (fused, sorted(must_not & set(calls)))
    d64 = to_float64(drr)
    img64, rot64, xyz64, _, _ = _render(d64, rot, xyz, call, w)
    want_volume = not stop
    ref_img, ref_gv = oracle_truth(drr, rot, xyz, w, renderer, mask, scene["n_points"], want_volume)
    fused, general = res[True], res[False]
    for name, (img, g_rot, g_xyz, g_vol) in (("fused", fused), ("general", general)):
        mine = _np(img)
        if renderer == "trilinear" and mask:
            mine = mine.sum(1, keepdims=True)
        assert mine.shape[0] == ref_img.shape[0] and mine.size == ref_img.size, (name, mine.shape)
        assert rel_err(mine.reshape(ref_img.shape), ref_img) < FWD_TOL, (name, rel_err(mine.reshape(ref_img.shape), ref_img))
        assert rel_err(_np(g_rot), _np(rot64)) < pose_tol, (name, rel_err(_np(g_rot), _np(rot64)))
        assert rel_err(_np(g_xyz), _np(xyz64)) < pose_tol, (name, rel_err(_np(g_xyz), _np(xyz64)))
        if stop:
            assert g_vol is None or float(g_vol.abs().max()) == 0.0, name
            continue
        assert g_vol is not None, name
        assert rel_err(_np(g_vol), ref_gv) < GRAD_TOL, (name, rel_err(_np(g_vol), ref_gv))
    # the two routes: the existing fused-vs-general tolerances
    if renderer == "trilinear" and mask:
        # (the routes' rays differ in the last bits: a sample on a label boundary may change channels --
        # 4e-4 at the device's size -- the channels' sum may not)
        assert rel_err(_np(fused[0]).sum(1), _np(general[0]).sum(1)) < 1e-5
        assert rel_err(_np(fused[0]), _np(general[0])) < 1e-3
    else:
        assert rel_err(_np(fused[0]), _np(general[0])) < 1e-5
    assert rel_err(_np(fused[1]), _np(general[1])) < pose_tol
    assert rel_err(_np(fused[2]), _np(general[2])) < pose_tol
    if not stop:
        assert rel_err(_np(fused[3]), _np(general[3])) < 1e-4, rel_err(_np(fused[3]), _np(general[3]))


@pytest.fixture(scope="module")
def scene():
    return host_scene()


@pytest.mark.parametrize("case", ROUTE_CASES, ids=route_case_id)
def test_gradient_route(emulated_ops, scene, case):
    check_route_case(scene, case, "cpu", emulated_ops)


# ------------------------------------------------------------------ B. layout invariance

def _same(a, b, exact, tol, what):
    """bit-equal (``exact``), else within ``tol`` of max |b| (the reordering of float atomics)"""
    if a is None or b is None:
        assert a is None and b is None, what
        return
    a, b = a.detach().cpu(), b.detach().cpu()
    assert a.shape == b.shape, what
    if exact:
        assert torch.equal(a, b), (what, rel_err(a.double().numpy(), b.double().numpy()))
    else:
        assert rel_err(a.double().numpy(), b.double().numpy()) <= tol, (what, rel_err(a.double().numpy(), b.double().numpy()))


def _pair(base):
    """two leaves with the same values: one for the strided call, one for the contiguous one"""
    return base.clone().requires_grad_(), base.clone().requires_grad_()


def layout_rays(device, dims=(20, 24, 16), det=(6, 7), B=3, seed=5):
    """(source (1, 1, 3), target (B, 2 N, 3), img (B, 1, 2 N)) in voxel space: one source, per pose two
    row-major detector grids of det[0] x det[1] rays (so that either half of the rays is a grid the brick
    kernels take) through the volume"""
    g = torch.Generator().manual_seed(seed)
    H, W = det
    Dx, Dy, Dz = dims
    src = torch.tensor([[[-45.0, Dy / 2 + 1.0, Dz / 2 - 0.5]]])
    i = torch.arange(H, dtype=torch.float32).view(H, 1)
    j = torch.arange(W, dtype=torch.float32).view(1, W)
    grids = []
    for b in range(B):
        for half in range(2):
            o = torch.rand(3, generator=g)
            y = (Dy * 0.1 + o[0] * 3 + i * (Dy * 0.8 / (H - 1))).expand(H, W)
            z = (Dz * 0.1 + o[1] * 3 + j * (Dz * 0.8 / (W - 1)) + 0.2 * b).expand(H, W)
            x = torch.full((H, W), Dx + 30.0 + 5 * o[2].item() + half)
            grids.append(torch.stack([x, y, z], -1).reshape(H * W, 3))
    tgt = torch.stack([torch.cat(grids[2 * b:2 * b + 2]) for b in range(B)])
    img = (tgt - src).norm(dim=-1).unsqueeze(1) * 0.5
    return src.to(device), tgt.to(device), img.to(device)


# (name, module class, ctor keywords, call keywords); fp32 and fp64 each
LAYOUT_CASES = [
    ("siddon_sum", Siddon, {}, {}),
    ("siddon_max", Siddon, {"reducefn": "max"}, {}),
    ("siddon_callable", Siddon, {"reducefn": _topk_sum}, {}),
    ("siddon_bilinear", Siddon, {"mode": "bilinear"}, {}),
    ("siddon_align_corners", Siddon, {}, {"align_corners": True}),
    ("siddon_stop", Siddon, {"stop_gradients_through_grid_sample": True}, {}),
    ("siddon_max_stop", Siddon, {"reducefn": "max", "stop_gradients_through_grid_sample": True}, {}),
    ("siddon_mask", Siddon, {}, {"mask": True}),
    ("trilinear_sum", Trilinear, {}, {"n_points": 40}),
    ("trilinear_max", Trilinear, {"reducefn": "max"}, {"n_points": 40}),
    ("trilinear_callable", Trilinear, {"reducefn": _topk_sum}, {"n_points": 40}),
    ("trilinear_nearest", Trilinear, {"mode": "nearest"}, {"n_points": 40}),
    ("trilinear_align_corners", Trilinear, {}, {"n_points": 40, "align_corners": True}),
    ("trilinear_mask", Trilinear, {}, {"n_points": 40, "mask": True}),
    ("trilinear_range", Trilinear, {}, {"n_points": 40, "range": True}),
    ("trilinear_range_mask", Trilinear, {}, {"n_points": 40, "range": True, "mask": True}),
]
LAYOUT_IDS = [(name, dt, grid) for name, *_ in LAYOUT_CASES for dt in ("f32", "f64") for grid in (False, True)]


def check_renderer_layout(name, dtype, grid, device, exact, tol=1e-5, exact_volume=False, B=3):
    """``Siddon`` / ``Trilinear`` on strided inputs against ``.contiguous()`` copies: the rays of one
    half of a (B, 2 N, 3) target and (B, 1, 2 N) img (``chunk(2, dim=1)`` with B > 1: strided), an
    expanded source, ``[::2]`` volume and label map, the range as column slices of one (1, 2) tensor.
    ``grid``: the half is promised as a detector grid (the volume-stationary kernels take it)."""
    _, cls, ctor, call = next(c for c in LAYOUT_CASES if c[0] == name)
    dt = torch.float32 if dtype == "f32" else torch.float64
    dims = (20, 24, 16)
    det = (6, 7)
    src0, tgt0, img0 = layout_rays(device, dims, det, B)
    # (the [::2] slices are a phantom and its label map; the odd slices something else)
    vol0 = torch.stack([phantom_volume(dims, seed=2), phantom_volume(dims, seed=9)], 1).reshape(2 * dims[0], *dims[1:])
    lab0 = torch.stack([_labels(dims, 5, 3), _labels(dims, 4, 8)], 1).reshape(2 * dims[0], *dims[1:])
    vol0, lab0 = vol0.to(device, dt), lab0.to(device, dt)
    call = dict(call)
    want_mask, want_range = call.pop("mask", False), call.pop("range", False)
    ab0 = torch.tensor([[0.12, 0.9]], dtype=dt, device=device)
    outs = []
    for strided in (True, False):
        v, s, t, i = (x.clone().requires_grad_() for x in (vol0, src0.to(dt), tgt0.to(dt), img0.to(dt)))
        ab = ab0.clone().requires_grad_()
        leaves = [v, s, t, i, ab]
        lay = (lambda x: x) if strided else (lambda x: x.contiguous())
        kw = dict(call)
        if want_mask:
            kw["mask"] = lay(lab0[::2])
        if want_range:
            kw["alphamin"], kw["alphamax"] = lay(ab[:, 0]), lay(ab[:, 1])
        vol = lay(v[::2])
        source = lay(s.expand(B, 1, 3))
        target = lay(t.chunk(2, dim=1)[1])
        img = lay(i.chunk(2, dim=-1)[1])
        if strided:
            assert not any(x.is_contiguous() for x in (vol, target, img))
        mod = cls(**ctor)
        if grid:
            mod.detector_shape = det
        out = mod(vol, source, target, img, **kw)
        w = torch.rand(out.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64).to(out)
        grads = torch.autograd.grad((out * w).sum(), leaves, allow_unused=True)
        outs.append((out, grads))
    (o1, g1), (o2, g2) = outs
    _same(o1, o2, exact, tol, (name, "out"))
    for leaf, a, b in zip(("volume", "source", "target", "img", "range"), g1, g2):
        both_zero = a is not None and b is not None and float(a.abs().max()) == float(b.abs().max()) == 0.0
        if not both_zero:
            _same(a, b, exact or (exact_volume and leaf == "volume"), tol, (name, leaf))


@pytest.mark.parametrize("name,dtype,grid", LAYOUT_IDS)
def test_renderer_layout_invariance(emulated_ops, name, dtype, grid):
    check_renderer_layout(name, dtype, grid, "cpu", exact=True)


NCC_CASES = {
    "ncc": lambda: NormalizedCrossCorrelation2d(),
    "ncc_patch": lambda: NormalizedCrossCorrelation2d(patch_size=5),
    "multiscale": lambda: MultiscaleNormalizedCrossCorrelation2d([None, 5], [0.5, 0.5]),
    "gradient": lambda: GradientNormalizedCrossCorrelation2d(sigma=1.0),
    "gradient_patch": lambda: GradientNormalizedCrossCorrelation2d(patch_size=7, sigma=0.0),
}


def check_ncc_layout(name, device, exact, tol=1e-5):
    """the NCC criteria on channel slices ``x[:, 1:2]`` of (B, 3, H, W) leaves against contiguous copies"""
    g = torch.Generator().manual_seed(6)
    base1, base2 = torch.rand(3, 3, 18, 20, generator=g), torch.rand(3, 3, 18, 20, generator=g)
    base1, base2 = base1.to(device), base2.to(device)
    outs = []
    for strided in (True, False):
        a, b = base1.clone().requires_grad_(), base2.clone().requires_grad_()
        x1, x2 = a[:, 1:2], b[:, 1:2]
        if strided:
            assert not x1.is_contiguous()
        else:
            x1, x2 = x1.contiguous(), x2.contiguous()
        val = NCC_CASES[name]()(x1, x2)
        w = torch.arange(1, val.numel() + 1, dtype=val.dtype, device=device).reshape(val.shape)
        outs.append((val,) + torch.autograd.grad((val * w).sum(), [a, b]))
    for what, p, q in zip(("value", "g_x1", "g_x2"), *outs):
        _same(p, q, exact, tol, (name, what))


@pytest.mark.parametrize("name", sorted(NCC_CASES))
def test_ncc_layout_invariance(emulated_ops, name):
    check_ncc_layout(name, "cpu", exact=True)


DRR_LAYOUT_LEVERS = ["dense", "sub", "patch_sub_flat"]


def check_drr_pose_layout(scene, renderer, lever, device, exact, tol=1e-5, exact_volume=lambda fused: False,
                          n_poses=None, pose_tol=None):
    """``drr(rot, xyz)`` with ``rot, xyz = p[:, :3], p[:, 3:]`` of one (B, 6) leaf against contiguous
    copies, both routes: image, the leaf's gradient (within ``pose_tol``, default ``tol``), the volume
    gradient (bit-equal where ``exact_volume(fused)``)"""
    drr = build_route_drr(scene, renderer, lever, False, device)
    call = {"n_points": scene["n_points"]} if renderer == "trilinear" else {}
    p0 = torch.cat([scene["rot"], scene["xyz"]], 1)[:n_poses].to(device)
    for fused in (True, False):
        drr.fuse_ray_generation = fused
        outs = []
        for strided in (True, False):
            p = p0.clone().requires_grad_()
            rot, xyz = p[:, :3], p[:, 3:]
            if not strided:
                rot, xyz = rot.contiguous(), xyz.contiguous()
            drr.density.grad = None
            img = drr(rot, xyz, parameterization="euler_angles", convention="ZXY", **call)
            w = torch.rand(img.shape, generator=torch.Generator().manual_seed(8), dtype=torch.float64).to(img)
            (img * w).sum().backward()
            outs.append((img.detach(), p.grad, drr.density.grad.clone()))
        (i1, p1, v1), (i2, p2, v2) = outs
        _same(i1, i2, exact, tol, (renderer, lever, fused, "image"))
        _same(p1, p2, exact, tol if pose_tol is None else pose_tol, (renderer, lever, fused, "pose"))
        _same(v1, v2, exact or exact_volume(fused), tol, (renderer, lever, fused, "volume"))


@pytest.mark.parametrize("lever", DRR_LAYOUT_LEVERS)
@pytest.mark.parametrize("renderer", ["siddon", "trilinear"])
def test_drr_pose_slices_layout_invariance(emulated_ops, scene, renderer, lever):
    check_drr_pose_layout(scene, renderer, lever, "cpu", exact=True)


def check_drr_ncc_layout(scene, device, exact, tol=1e-5):
    """``drr.ncc`` with ``fixed`` a channel slice of a (1, 3, H, W) tensor against a contiguous copy"""
    drr = DRR(scene["subject"], **scene["geo"]).to(device)
    H, W = drr.detector.height, drr.detector.width
    F = torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(2)).to(device)
    outs = []
    for strided in (True, False):
        fixed = F[:, 1:2] if strided else F[:, 1:2].contiguous()
        rot = scene["rot"].to(device).clone().requires_grad_()
        xyz = scene["xyz"].to(device).clone().requires_grad_()
        val = drr.ncc(fixed, rot, xyz, convention="ZXY")
        k = torch.arange(val.numel(), dtype=val.dtype, device=device)
        (val * (k + 1) * (1 - 2 * (k % 2))).sum().backward()  # (weights 1, -2, 3, ...)
        outs.append((val.detach(), rot.grad, xyz.grad))
    for what, p, q in zip(("ncc", "rot", "xyz"), *outs):
        _same(p, q, exact, tol, what)


def test_drr_ncc_fixed_slice_layout_invariance(emulated_ops, scene):
    check_drr_ncc_layout(scene, "cpu", exact=True)
