"""The weighted (masked) MutualInformation kernels (csrc/wmi.hip, include/diffdrr_wmi_hip.h) on the MI355X.

The yardstick is diffdrr_amd.metrics.weighted_mutual_information in float64 on the device; the gates are the project's
own (tests/mi_cases.py): |value - f64| <= 2 |f32 composition - f64| + 2e-6 and rel_err(gradient, f64) <
2 rel_err(f32 composition, f64) + 2e-5.  The float64 value has no NaN in any case used.  wmi.hip keeps mi.hip's
launch geometry, so the cases of tests/test_gpu_mi_dispatch.py reach the same paths here (mi_cases.describe)."""
import copy

import pytest
import torch

import wmi_cases as C
from diffdrr_amd import MutualInformation, Registration, ops
from mi_cases import GRAD_FLOOR, VALUE_FLOOR, _grad_gate, _images, _value_gate, describe, geometry
from wncc_cases import PATTERNS, adam_loop, occluded_scene, poison

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64


def _gated(name, crit, fixed, moving, weight, g_w, grad_of):
    """One call of the module under both gates -> the printed figures"""
    B, _, H, W = moving.shape
    (v32, g32), (v64, g64) = C.references(crit, fixed, moving, weight, g_w)
    with C.launches(ops) as names:
        v, grads = C.run(lambda a, b, w: crit(a, b, weight=w), fixed, moving, weight, g_w, grad_of)
    which = {"fixed": (0,), "moving": (1,), "both": (0, 1)}[grad_of]
    assert names == ["ddrr_wmi_forward"] + ["ddrr_wmi_backward"] * len(which), (name, names)
    fig = {"value": _value_gate(v, v32, v64)}
    for mine, i in zip(grads, which):
        assert mine.dtype == F32 and mine.shape == g64[i].shape and bool(torch.isfinite(mine).all())
        fig[("fixed", "moving")[i]] = _grad_gate(mine, g32[i], g64[i], (name, grad_of, i))
        off = (weight == 0).expand(B, 1, H, W)
        if i == 1:
            assert bool((mine[off] == 0).all()), name  # exactly 0 where the weight is 0
    return fig


# ------------------------------------------------------------------------------------------- (a) every dispatch
BIN_COUNTS = (2, 3, 9, 32, 33, 65, 129, 256)  # every NS of the backward, every nb of the forward
SETTINGS = ((0.1, True), (0.03, False), (0.1, False), (0.03, True))
GRAD_OFS = ("both", "moving", "fixed")


@pytest.mark.parametrize("K", BIN_COUNTS)
def test_every_dispatch_under_every_weight_pattern(gpu, K):
    """B = 3, 19 x 23 (N = 437), images partly outside [0, 1]; the six weight patterns shared and per pose.  The
    crossing is thinned to stay in seconds: every K meets every pattern, both sigmas, both normalisations, g_out per
    pose and the gradient of a sum, and the gradients to fixed, moving and both -- the setting moves on by one from
    pattern to pattern and starts one further at every K."""
    B, H, W = 3, 19, 23
    g = torch.Generator().manual_seed(1000 + K)
    fixed, moving = (t.to(gpu) for t in _images("outside", B, H, W, g))
    g_out = (torch.rand(B, generator=g) + 0.5).to(gpu)
    crits = [MutualInformation(sigma=s, num_bins=K, normalize=n).to(gpu) for s, n in SETTINGS]
    lines, seen = [], set()
    for i, (label, weight) in enumerate(C.all_weights(B, H, W, gpu)):
        j = i + BIN_COUNTS.index(K)
        crit, g_w, grad_of = crits[j % 4], (g_out, None)[(j // 4 + i) % 2], GRAD_OFS[j % 3]
        seen.add((j % 4, g_w is None, grad_of))
        fig = _gated(f"K={K} {label}", crit, fixed, moving, weight, g_w, grad_of)
        lines.append(f"  {label}, sigma {SETTINGS[j % 4][0]}, normalize {SETTINGS[j % 4][1]}, "
                     f"{'sum' if g_w is None else 'per pose'}, d/d {grad_of}: "
                     + "; ".join(f"{k} kernel {e:.2e} float32 composition {e32:.2e}" for k, (e, e32) in fig.items()))
    assert {s[0] for s in seen} == {0, 1, 2, 3} and {s[1] for s in seen} == {True, False}
    assert {s[2] for s in seen} == set(GRAD_OFS) and len(lines) == 2 * len(PATTERNS) - 1
    print(f"\ndispatch | {describe(B, H * W, K)}\n" + "\n".join(lines))


# ------------------------------------------------------------------------------------------- (b) w = 1: mi.hip's bits
CHUNK_CASES = ((70, 32, 32, 256), (24, 32, 32, 256), (300, 12, 14, 100), (1100, 6, 7, 64), (8, 64, 64, 256))


@pytest.mark.parametrize("case", CHUNK_CASES, ids=["B%d_%dx%d_K%d" % c for c in CHUNK_CASES])
def test_unit_weight_gives_the_unweighted_librarys_bits(gpu, case):
    """The check that ties the duplicated kernels together: with w = 1 everywhere, shared or per pose, value and both
    gradients are those of libdiffdrr_mi_hip.so bit for bit, at the chunk geometries of tests/test_gpu_mi_dispatch.py
    (the largest with 8 poses instead of 32: 4 chunks of 1024 px, NS = 128)."""
    B, H, W, K = case
    g = torch.Generator().manual_seed(B + H * W + K)
    fixed, moving = (t.to(gpu) for t in _images("unit", B, H, W, g))
    g_out = (torch.rand(B, generator=g) + 0.5).to(gpu)
    crit = MutualInformation(num_bins=K).to(gpu)
    with C.launches(ops) as names:
        want = C.run(lambda a, b, w: crit(a, b), fixed, moving, None, g_out, "both")
    assert names == ["ddrr_mi_forward", "ddrr_mi_backward", "ddrr_mi_backward"], names
    assert float(want[1][0].abs().max()) > 0 and float(want[1][1].abs().max()) > 0
    for ones in (torch.ones(1, 1, H, W, device=gpu), torch.ones(B, 1, H, W, device=gpu)):
        with C.launches(ops) as names:
            got = C.run(lambda a, b, w: crit(a, b, weight=w), fixed, moving, ones, g_out, "both")
        assert names == ["ddrr_wmi_forward", "ddrr_wmi_backward", "ddrr_wmi_backward"], names
        assert torch.equal(got[0], want[0]), case
        assert torch.equal(got[1][0], want[1][0]) and torch.equal(got[1][1], want[1][1]), case
    print(f"\nunit weight | {describe(B, H * W, K)} | value and both gradients: the unweighted library's bits")


# ------------------------------------------------------------------------------------------- (c) masked pixels
@pytest.mark.parametrize("K", [33, 256])
def test_masked_pixels_are_not_read(gpu, K):
    """NaN, Inf and 1e30 in both images wherever w == 0 change no bit of the value or of either gradient, and the
    gradients are exactly 0 there."""
    B, H, W = 3, 19, 23
    g = torch.Generator().manual_seed(77 + K)
    _, moving = (t.to(gpu) for t in _images("outside", B, H, W, g))
    fixed = (torch.rand(B, 1, H, W, generator=g) * 1.6 - 0.3).to(gpu)  # (per pose: it takes per-pose poison)
    g_out = (torch.rand(B, generator=g) + 0.5).to(gpu)
    crit = MutualInformation(num_bins=K).to(gpu)
    checked = 0
    for label, weight in C.all_weights(B, H, W, gpu, ("disc", "half", "edge-hot", "one pose empty")):
        off = (weight == 0).expand(B, 1, H, W)
        assert bool(off.any()), label
        fn = lambda a, b, w: crit(a, b, weight=w)  # noqa: E731
        clean = C.run(fn, fixed, moving, weight, g_out, "both")
        dirty = C.run(fn, poison(fixed, weight), poison(moving, weight), weight, g_out, "both")
        assert bool(torch.isnan(poison(moving, weight)[off]).any()) and bool(torch.isinf(poison(fixed, weight)[off]).any())
        assert torch.equal(clean[0], dirty[0]) and bool(torch.isfinite(dirty[0]).all()), label
        for a, b in zip(clean[1], dirty[1]):
            assert torch.equal(a, b) and bool(torch.isfinite(b).all()), label
            assert bool((b[off] == 0).all()) and float(b.abs().max()) > 0, label
        checked += 1
    assert checked == 7


# ------------------------------------------------------------------------------------------- (d) scaling, repetition
def test_scaling_repetition_and_batch_permutation(gpu):
    """4 w against w: within the two floors of each other (not bit for bit: the epsilons do not scale).  Two
    identical calls, and a permutation of the batch, give equal bits: no atomics, nothing left in the workspace, no
    offset that mixes pairs (the geometry depends on (B, N, K) only)."""
    B, H, W, K = 5, 37, 53, 100
    g = torch.Generator().manual_seed(55)
    x1 = torch.rand(B, 1, H, W, generator=g).to(gpu)
    x2 = (torch.rand(B, 1, H, W, generator=g) * 1.4 - 0.2).to(gpu)
    g_out = (torch.rand(B, generator=g) + 0.5).to(gpu)
    crit = MutualInformation(num_bins=K).to(gpu)
    fn = lambda a, b, w: crit(a, b, weight=w)  # noqa: E731
    for label, weight in C.all_weights(B, H, W, gpu, ("smooth", "half", "disc")):
        weight = weight.expand(B, -1, -1, -1).contiguous()
        v, (g1, g2) = C.run(fn, x1, x2, weight, g_out, "both")
        again = C.run(fn, x1, x2, weight, g_out, "both")
        assert torch.equal(again[0], v) and torch.equal(again[1][0], g1) and torch.equal(again[1][1], g2), label
        v4, (g1_4, g2_4) = C.run(fn, x1, x2, 4 * weight, g_out, "both")
        dv = float((v4 - v).abs().max())
        dg = max(float((a - b).abs().max() / b.abs().max()) for a, b in ((g1_4, g1), (g2_4, g2)))
        print(f"\n4 w against w, {label}: values differ by {dv:.2e}, gradients by {dg:.2e} of the largest")
        assert dv <= VALUE_FLOOR and dg <= GRAD_FLOOR, (label, dv, dg)
        perm = torch.tensor([3, 0, 4, 1, 2], device=gpu)
        vp, (g1p, g2p) = C.run(fn, x1[perm].contiguous(), x2[perm].contiguous(), weight[perm].contiguous(),
                               g_out[perm].contiguous(), "both")
        assert torch.equal(vp, v[perm]) and torch.equal(g1p, g1[perm]) and torch.equal(g2p, g2[perm]), label
        assert len(set(v.tolist())) == B


# ------------------------------------------------------------------------------------------- (e) strides
SIZES = ((1, 2), (7, 9), (1, 257), (19, 27))


@pytest.mark.parametrize("size", SIZES, ids=["N%d" % (h * w) for h, w in SIZES])
def test_weight_and_image_strides(gpu, size):
    """N = 2, 63, 257, 513.  One weight for the batch given as (1, 1, H, W), `expand`ed (both read in place, stride 0)
    and materialised (stride N) through the module, then raw: the weight and the moving images as rows of larger
    buffers at stride 2 N with NaN in the gaps.  Everything agrees bit for bit."""
    H, W = size
    B, K, N = 3, 9, H * W
    assert geometry(B, N, K)["chunks"] == {257: 2, 513: 3}.get(N, 1)
    g = torch.Generator().manual_seed(100 * H + W)
    fixed, moving = (t.to(gpu) for t in _images("unit", B, H, W, g))
    g_out = (torch.rand(B, generator=g) + 0.5).to(gpu)
    weight = (0.25 + 1.5 * torch.rand(1, 1, H, W, generator=g)).to(gpu)
    weight[..., -1] = 0.0 if N > 2 else 1.0
    crit = MutualInformation(num_bins=K).to(gpu)
    fn = lambda a, b, w: crit(a, b, weight=w)  # noqa: E731
    want = C.run(fn, fixed, moving, weight, g_out, "both")
    (v32, _), (v64, _) = C.references(crit, fixed, moving, weight, g_out)
    _value_gate(want[0], v32, v64)  # (the gradients' gate is test (a)'s: at N = 2 they are rounding noise around 0)
    for form in (weight.expand(B, -1, -1, -1), weight.expand(B, -1, -1, -1).contiguous()):
        got = C.run(fn, fixed, moving, form, g_out, "both")
        assert torch.equal(got[0], want[0]) and all(torch.equal(a, b) for a, b in zip(got[1], want[1])), size
    x1, flat, w1 = fixed.reshape(N).contiguous(), moving.reshape(B, N).contiguous(), weight.reshape(N).contiguous()
    xbuf = torch.full((B, 2 * N), float("nan"), device=gpu)
    xbuf[:, :N] = flat
    wbuf = torch.full((B, 2 * N), float("nan"), device=gpu)
    wbuf[:, :N] = w1
    # (the strided batch as the moving and as the fixed image: each against the same call from contiguous buffers)
    for packed, strided in (((x1, 0, flat, N, w1, 0), (x1, 0, xbuf, 2 * N, wbuf, 2 * N)),
                            ((flat, N, x1, 0, w1, 0), (xbuf, 2 * N, x1, 0, wbuf, 2 * N))):
        ref = C.raw(ops, gpu, *packed, B, H, W, crit, g_out)
        got = C.raw(ops, gpu, *strided, B, H, W, crit, g_out)
        for k, (a, b) in enumerate(zip(got, ref)):
            assert torch.equal(a, b) and bool(torch.isfinite(a).all()), (size, k)
        if packed[1] == 0:  # the raw call is the module's
            assert torch.equal(ref[0], want[0]) and torch.equal(ref[4], want[1][1].reshape(B, H, W))


# ------------------------------------------------------------------------------------------- (f) one pose empty
@pytest.mark.parametrize("K", [9, 64])
def test_one_pose_empty(gpu, K):
    """The emptied pair: value 0, gradient 0, an all-zero state; the other pairs' bits are those of the batch without
    it (B = 3 and B = 2 have the same launch geometry here); weight_sum is the float64 sum of the weights."""
    B, H, W = 3, 19, 23
    N = H * W
    same = ("Kp", "nb", "chunks", "cp", "tpw", "NS", "waves")
    assert {k: geometry(B, N, K)[k] for k in same} == {k: geometry(B - 1, N, K)[k] for k in same}
    g = torch.Generator().manual_seed(9 + K)
    fixed, moving = (t.to(gpu) for t in _images("outside", B, H, W, g))
    g_out = (torch.rand(B, generator=g) + 0.5).to(gpu)
    weight = C.weight4("one pose empty", B, H, W, True, gpu) * (0.25 + 1.5 * torch.rand(B, 1, H, W, generator=g)).to(gpu)
    assert float(weight[-1].abs().max()) == 0 and float(weight[:-1].sum()) > 0
    crit = MutualInformation(num_bins=K).to(gpu)
    x1, flat, w = fixed.reshape(N).contiguous(), moving.reshape(B, N).contiguous(), weight.reshape(B, N).contiguous()
    out, state, wsum, g1, g2 = C.raw(ops, gpu, x1, 0, flat, N, w, N, B, H, W, crit, g_out)
    assert float(out[-1]) == 0 and bool((state[-1] == 0).all()) and bool((g1[-1] == 0).all()) and bool((g2[-1] == 0).all())
    assert float(wsum[-1]) == 0
    want = w.double().sum(1)
    assert bool(((wsum - want).abs() <= 1e-12 * want).all()), (wsum, want)
    rest = C.raw(ops, gpu, x1, 0, flat[:-1].contiguous(), N, w[:-1].contiguous(), N, B - 1, H, W, crit,
                 g_out[:-1].contiguous())
    for k, (a, b) in enumerate(zip((out, state, wsum, g1, g2), rest)):
        assert torch.equal(a[:-1], b) and bool(torch.isfinite(b).all()), k
    assert float(g1[:-1].abs().max()) > 0 and float(g2[:-1].abs().max()) > 0
    # ... and through the module, under the gates (the expected value of the emptied pair is 0 by definition)
    fig = _gated(f"one pose empty K={K}", crit, fixed, moving, weight, g_out, "both")
    print(f"\none pose empty | {describe(B, N, K)} | "
          + "; ".join(f"{k} kernel {e:.2e} float32 composition {e32:.2e}" for k, (e, e32) in fig.items()))


# ------------------------------------------------------------------------------------------- (g) module routes
def test_module_routes(gpu):
    B, H, W = 3, 19, 23
    g = torch.Generator().manual_seed(12)
    fixed, moving = (t.to(gpu) for t in _images("outside", B, H, W, g))
    a = fixed.expand(B, -1, -1, -1)
    weight = C.weight4("smooth", B, H, W, True, gpu) * C.weight4("disc", B, H, W, False, gpu)
    crit = MutualInformation(num_bins=32).to(gpu)
    # float32 on the device with a detached weight: the kernels
    with C.launches(ops) as names:
        x = moving.clone().requires_grad_()
        v = crit(a, x, weight=weight)
        v.sum().backward()
    assert names == ["ddrr_wmi_forward", "ddrr_wmi_backward"] and type(v.grad_fn).__name__.startswith("_WeightedMIFn")
    with torch.no_grad(), C.launches(ops) as names:
        v0 = crit(a, moving, weight=weight)
    assert names == ["ddrr_wmi_forward"] and torch.equal(v0, v.detach())
    # weight=None: what the call without the keyword launches, and its bits
    with torch.no_grad(), C.launches(ops) as without:
        p0 = crit(a, moving)
    with torch.no_grad(), C.launches(ops) as with_none:
        p1 = crit(a, moving, weight=None)
    assert without == with_none == ["ddrr_mi_forward"] and torch.equal(p0, p1)
    # a weight that takes a gradient, float64, more than 256 bins: the composition, no launch, its exact values
    wg = weight.clone().requires_grad_()
    with C.launches(ops) as names:
        x = moving.clone().requires_grad_()
        v1 = crit(a, x, weight=wg)
        v1.sum().backward()
    assert not names and wg.grad is not None and bool(torch.isfinite(wg.grad).all()) and float(wg.grad.abs().max()) > 0
    assert torch.equal(v1.detach(), C.composition(crit, a, moving, weight, F32))
    _value_gate(v.detach(), v1.detach(), C.composition(crit, a, moving, weight, F64))
    d64 = copy.deepcopy(crit).double()
    with C.launches(ops) as names:
        v2 = d64(a.double(), moving.double(), weight=weight.double())
    assert not names and v2.dtype == F64 and torch.equal(v2, C.composition(crit, a, moving, weight, F64))
    big = MutualInformation(num_bins=300).to(gpu)
    with C.launches(ops) as names:
        v3 = big(a, moving, weight=weight)
    assert not names and torch.equal(v3, C.composition(big, a, moving, weight, F32))
    assert float((v3.double() - C.composition(big, a, moving, weight, F64)).abs().max()) <= 1e-4
    with C.launches(ops) as names, pytest.raises(ValueError, match=r"weight has shape .* expected"):
        crit(a, moving, weight=torch.ones(1, H, W, device=gpu))
    assert not names


# ------------------------------------------------------------------------------------------- (h) captured iteration
def _scaled_mi(top, device, num_bins=32):
    """MutualInformation for images in [0, top]: the bins and the kernel width scaled (they are buffers)"""
    crit = MutualInformation(sigma=0.1 * top, num_bins=num_bins).to(device)
    with torch.no_grad():
        crit.bins.mul_(top)
    return crit


def test_graphed_iteration_replays_the_eager_steps(gpu):
    """GraphedIteration(reg, MutualInformation(num_bins=32), opt, fixed, weight=w): ten replays against ten eager
    iterations from the same start under plain gradient ascent (wncc_cases.check_graphed_iteration's scheme: SGD's
    step is lr times the gradient, so after ten steps the parameters differ by lr times the sum of the ten gradients'
    differences).  Both routes run the same kernels on the same inputs; only the record's float atomics are summed in
    another order, which leaves each pose gradient within its gate of float64 -- the project's gradient gate, per
    block of parameters: 2 x the float32 composition's largest error + 2e-5 of the largest gradient -- so two of them
    are at most two gates apart and ten steps 10 * 2 * lr * gate.  The gate is taken at the start pose."""
    import fused_step_cases as F
    from diffdrr_amd import GraphedIteration

    sc = F.scene("3x30x26", gpu, ops)
    drr = copy.deepcopy(sc.drr)
    drr.renderer.brick_storage = "f32"  # (eager and captured renders from the same bricks)
    d64 = copy.deepcopy(drr).to(F64)
    B, H, W = sc.B, sc.H, sc.W
    # (MutualInformation takes images of one shape: the shared fixed image `expand`ed, read in place)
    fixed = sc.x1_shared.reshape(1, 1, H, W).contiguous().expand(B, -1, -1, -1)
    weight = C.weight4("disc", B, H, W, False, gpu)
    crit = _scaled_mi(float(fixed.max()), gpu)
    kw = dict(parameterization="euler_angles", convention="ZXY")

    def pose_gradient(module, dtype):
        r, x = sc.rot.to(dtype).clone().requires_grad_(), sc.xyz.to(dtype).clone().requires_grad_()
        v = C.composition(crit, fixed.expand(B, -1, -1, -1), module(r, x, **kw), weight, dtype)
        v.sum().backward()
        return r.grad.double(), x.grad.double()

    want, own = pose_gradient(d64, F64), pose_gradient(drr, F32)
    gates = [2 * float((o - w_).abs().max()) + GRAD_FLOOR * float(w_.abs().max()) for o, w_ in zip(own, want)]
    assert all(float(w_.abs().max()) > 0 for w_ in want)
    lrs = (1e-4 / float(want[0].abs().max()), 1e-2 / float(want[1].abs().max()))  # ten steps: <= 1e-3 rad / 0.1 mm

    def fresh():
        reg = Registration(drr, sc.rot.clone(), sc.xyz.clone(), **kw)
        return reg, torch.optim.SGD([{"params": [reg._rotation], "lr": lrs[0]},
                                     {"params": [reg._translation], "lr": lrs[1]}], maximize=True)

    reg, opt = fresh()
    with C.launches(ops) as names:
        for _ in range(10):
            opt.zero_grad()
            crit(fixed, reg(), weight=weight).sum().backward()
            opt.step()
    assert names == ["ddrr_wmi_forward", "ddrr_wmi_backward"] * 10, names
    eager = (reg.rotation.detach().clone(), reg.translation.detach().clone())
    reg, opt = fresh()
    step = GraphedIteration(reg, crit, opt, fixed, weight=weight)
    assert step.fused_similarity is False
    assert torch.equal(reg.rotation.detach(), sc.rot) and torch.equal(reg.translation.detach(), sc.xyz)
    for _ in range(10):
        loss = step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all()) and step.iterations_done == 10
    for label, a, b, start, lr, gate, g in (
            ("rotation", reg.rotation.detach(), eager[0], sc.rot, lrs[0], gates[0], want[0]),
            ("translation", reg.translation.detach(), eager[1], sc.xyz, lrs[1], gates[1], want[1])):
        err, tol, moved = float((a - b).abs().max()), 10 * 2 * lr * gate, float((a - start).abs().max())
        print(f"\ngraphed against eager after ten steps, {label}: largest difference {err:.3g}, allowed {tol:.3g}, "
              f"moved {moved:.3g}")
        assert err <= tol, (label, err, tol)
        # (the steps moved the parameters; unlike the NCC's, MI's pose gradient is not constant over ten steps -- the
        # Gaussian kernels are 0.1 of the range wide -- so only the order of ten times lr times the start gradient)
        assert lr * float(g.abs().max()) < moved < 20 * lr * float(g.abs().max()), (label, moved)


# ------------------------------------------------------------------------------------------- (i) the occluded scene
def test_occluded_scene_masked_gradient_is_zero_under_the_bar(gpu):
    """wncc_cases.occluded_scene (64^3 -> 48^2, a bright bar over rows 10-17 of the fixed image): Adam on MI with and
    without the mask that covers the bar; both final pose errors are printed, and the masked run's gradient with
    respect to the moving image is 0 under the bar.

    That the masked run ends closer to the truth is NOT asserted: on the MI355X neither run converges on this scene
    under this loop (Adam, 1e-1 / 5e0).  Measured with the bins over [0, max fixed] and over twice that, num_bins in
    {16, 32, 64}, sigma in {0.05, 0.1, 0.2} of the range, 250 iterations: no run -- masked, unmasked, or on the clean
    image without the bar -- ends within 5 tolerances (the best: clean 5.5, masked 11.3, unmasked 12.4), a few pass
    within 1 tolerance on the way (clean 0.82 at iteration 54, masked 0.96 at 191) and leave again, and sigma = 0.2
    runs away (700 tolerances).  With num_bins = 32, sigma = 0.1 two runs of this test gave masked 33.7 against
    unmasked 43.0, then 44.1 against 22.0: the renders sum with float atomics and the loop amplifies their last bits."""
    import lm_cases

    drr, fixed, occluded, weight = occluded_scene(gpu)
    crit = _scaled_mi(float(fixed.max()), gpu)
    kw = dict(parameterization="euler_angles", convention="ZXY")

    def final_q(track):
        rot, xyz = track[-1]
        return max(float((rot.cpu() - lm_cases.TRUTH[0]).abs().max()) / 0.01,
                   float((xyz.cpu() - lm_cases.TRUTH[1]).abs().max()) / 0.5)

    masked, best_m = adam_loop(drr, lambda r, x: crit(occluded, drr(r, x, **kw), weight=weight), gpu, cap=150)
    plain, best_p = adam_loop(drr, lambda r, x: crit(occluded, drr(r, x, **kw)), gpu, cap=150)
    q_m, q_p = final_q(masked), final_q(plain)
    print(f"\noccluded scene, MI, 150 Adam iterations, pose error in tolerances of 0.01 rad / 0.5 mm: masked ends at "
          f"{q_m:.3g} (closest {best_m[0]:.3g} at iteration {best_m[1]}), unmasked ends at {q_p:.3g} (closest "
          f"{best_p[0]:.3g} at iteration {best_p[1]})")
    rot, xyz = masked[-1]
    img = drr(rot, xyz, **kw).detach().requires_grad_()
    crit(occluded, img, weight=weight).sum().backward()
    assert bool((img.grad[:, :, 10:18, :] == 0).all()) and float(img.grad.abs().max()) > 0
