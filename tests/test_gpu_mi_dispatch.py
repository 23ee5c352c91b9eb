"""MutualInformation on the MI355X at every point where csrc/mi.hip's host code decides something: the backward
instance and its partly filled last wave (from K), the forward's padding and block count (from K), its pixel chunks
(from B, K and N), the backward's tiles per workgroup (from B and N), the image strides and the batch itself.

Every comparison is the project's: the torch composition (diffdrr_amd.metrics.mutual_information) in float64 on the
device is the yardstick, the same in float32 is the reference's own error, and the kernels hold
|value - f64| <= 2 |f32 - f64| + 2e-6 and rel_err(gradient, f64) < 2 rel_err(f32, f64) + 2e-5 (tests/mi_cases.py).
Each test asserts that the float64 value has no NaN and prints the kernels' error next to the float32 composition's,
with the path the case takes (mi_cases.describe)."""
import pytest
import torch

from diffdrr_amd import MutualInformation, _lib, ops
from mi_cases import _grad_gate, _images, _references, _run, _value_gate, describe, geometry

pytestmark = pytest.mark.gpu


def _counted(monkeypatch):
    """ops.mi_forward / ops.mi_backward wrapped to record their calls."""
    calls = []
    fwd, bwd = ops.mi_forward, ops.mi_backward
    monkeypatch.setattr(ops, "mi_forward", lambda *a, **k: (calls.append("f"), fwd(*a, **k))[1])
    monkeypatch.setattr(ops, "mi_backward", lambda *a, **k: (calls.append("b"), bwd(*a, **k))[1])
    return calls


def _workspace_matches(B, H, W, K):
    """The restated forward geometry is the library's (its workspace is sized by the chunk count)."""
    got = int(_lib.get_mi_lib().query("ddrr_mi_workspace_bytes", B, H, W, K))
    assert got == 4 * geometry(B, H * W, K)["workspace_floats"], (got, geometry(B, H * W, K))


def _check(name, crit, fixed, moving, weights, grad_ofs=("both",), calls=None):
    """Value and gradients of `crit` under the two gates, for every weighting in `weights` (None: v.sum(), whose
    g_out has stride 0) and every set of differentiated images in `grad_ofs`; one printed line."""
    B, _, H, W = moving.shape
    _workspace_matches(B, H, W, crit.bins.numel())
    worst = {"value": (0.0, 0.0), "fixed": (0.0, 0.0), "moving": (0.0, 0.0)}

    def note(key, pair):
        worst[key] = (max(worst[key][0], pair[0]), max(worst[key][1], pair[1]))

    for w in weights:
        (v32, g32), (v64, g64) = _references(crit, fixed, moving, w)
        for grad_of in grad_ofs:
            if calls is not None:
                calls.clear()
            v, gm = _run(crit, fixed, moving, w, grad_of)
            if calls is not None:
                assert calls.count("f") == 1 and calls.count("b") == (2 if grad_of == "both" else 1), calls
            note("value", _value_gate(v, v32, v64))
            which = {"fixed": (0,), "moving": (1,), "both": (0, 1)}[grad_of]
            for mine, i in zip(gm, which):
                assert mine.dtype == torch.float32 and mine.shape == g64[i].shape
                assert bool(torch.isfinite(mine).all())
                note(("fixed", "moving")[i], _grad_gate(mine, g32[i], g64[i], (name, grad_of, i)))
    print(f"\n{name} | {describe(B, H * W, crit.bins.numel())} | "
          + "; ".join(f"{k}: kernel {e:.2e}, float32 composition {e32:.2e}" for k, (e, e32) in worst.items()))
    return worst


# ------------------------------------------------------------------------------------------- 1. every dispatch
BIN_COUNTS = (2, 3, 8, 9, 16, 31, 32, 33, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256)


@pytest.mark.parametrize("normalize", [True, False], ids=["normalised", "plain"])
@pytest.mark.parametrize("sigma", [0.1, 0.03])
@pytest.mark.parametrize("K", BIN_COUNTS)
def test_every_bin_count_dispatch(gpu, monkeypatch, K, sigma, normalize):
    """Every backward instance (NS = 1 ... 128) at both ends of its range of K, partly filled last waves, every
    number of forward blocks and a single live bin in the last block row (K = 65, 129, 193).  B = 3, 19 x 23:
    N = 437 is a multiple of neither 8 nor 32."""
    B, H, W = 3, 19, 23
    g = torch.Generator().manual_seed(1000 * K + int(1000 * sigma) + int(normalize))
    fixed, moving = (t.to(gpu) for t in _images("outside", B, H, W, g))
    w = (torch.rand(B, generator=g) + 0.5).to(gpu)
    crit = MutualInformation(sigma=sigma, num_bins=K, normalize=normalize).to(gpu)
    calls = _counted(monkeypatch)
    _check(f"dispatch K={K} sigma={sigma} normalize={normalize}", crit, fixed, moving, (w, None),
           ("fixed", "moving", "both"), calls)


# ------------------------------------------------------------------------------------------- 2. one bin
def test_one_bin(gpu):
    """K = 1, plain: the value under the gate.  The value is ~1e-9 and its gradient rounding noise (the float32
    composition's own gradient error on this scene is 2e2 to 1e3 relative), so the gradients only have to be
    finite.  K = 1 normalised is 0 / 0 and stays out."""
    g = torch.Generator().manual_seed(1)
    fixed, moving = (t.to(gpu) for t in _images("outside", 3, 19, 23, g))
    w = (torch.rand(3, generator=g) + 0.5).to(gpu)
    crit = MutualInformation(num_bins=1, normalize=False).to(gpu)
    for weights in (w, None):
        (v32, _), (v64, _) = _references(crit, fixed, moving, weights)
        v, grads = _run(crit, fixed, moving, weights, "both")
        e, e32 = _value_gate(v, v32, v64)
        print(f"\none bin | {describe(3, 437, 1)} | value: kernel {e:.2e}, float32 composition {e32:.2e}")
        assert len(grads) == 2 and all(bool(torch.isfinite(x).all()) for x in grads)
        assert grads[0].shape == fixed.shape and grads[1].shape == moving.shape


# ------------------------------------------------------------------------------------------- 3. chunk geometry
# (B, H, W, K) -> what the host code must make of it
CHUNK_CASES = {
    (70, 32, 32, 256): dict(nb=4, chunks=1, cp=1024, tpw=9, grad_chunks=4),      # B nb^2 = 1120 >= 1024
    (24, 32, 32, 256): dict(nb=4, chunks=3, cp=344, tpw=3, grad_chunks=11),      # 3 x 344 > 1024; 32 = 10 x 3 + 2
    (300, 12, 14, 100): dict(nb=2, chunks=1, tpw=8, ntiles=6, grad_chunks=1),    # tpw > ntiles
    (1100, 6, 7, 64): dict(nb=1, chunks=1, tpw=9, ntiles=2, grad_chunks=1),      # grid.z = 1100
    (32, 64, 64, 256): dict(nb=4, chunks=2, NS=128),                             # the project's pose batch
}


@pytest.mark.parametrize("case", list(CHUNK_CASES), ids=["B%d_%dx%d_K%d" % c for c in CHUNK_CASES])
def test_chunk_geometry(gpu, case):
    B, H, W, K = case
    geo = geometry(B, H * W, K)
    assert {k: geo[k] for k in CHUNK_CASES[case]} == CHUNK_CASES[case], geo
    g = torch.Generator().manual_seed(B + H * W + K)
    fixed, moving = (t.to(gpu) for t in _images("unit", B, H, W, g))
    w = (torch.rand(B, generator=g) + 0.5).to(gpu)
    crit = MutualInformation(num_bins=K, normalize=True).to(gpu)
    _check("chunks (%d, %d, %d, %d)" % case, crit, fixed, moving, (w,))


# ------------------------------------------------------------------------------------------- 4. tiny images
SIZES = ((1, 2), (1, 3), (1, 7), (2, 4), (3, 3), (1, 31), (4, 8), (3, 11), (15, 17), (16, 16), (1, 257), (19, 27))


@pytest.mark.parametrize("K", [9, 64])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_tiny_and_threshold_image_sizes(gpu, size, K):
    """N = 2, 3, 7, 8, 9, 31, 32, 33, 255, 256, 257, 513: forward waves without a pixel, one partial backward tile,
    the 1 -> 2 chunk edge and a chunk remainder."""
    H, W = size
    geo = geometry(3, H * W, K)
    assert geo["chunks"] == {257: 2, 513: 3}.get(H * W, 1), geo
    g = torch.Generator().manual_seed(100 * H + W + K)
    fixed, moving = (t.to(gpu) for t in _images("unit", 3, H, W, g))
    w = (torch.rand(3, generator=g) + 0.5).to(gpu)
    crit = MutualInformation(num_bins=K).to(gpu)
    _check(f"size {H}x{W} K={K}", crit, fixed, moving, (w,))


# ------------------------------------------------------------------------------------------- 5. independent pairs
def test_pairs_are_independent(gpu):
    """The geometry depends on (B, N, K) only, so permuting the batch permutes values and gradients bit for bit,
    and one pair repeated gives identical results: no workspace or state offset mixes pairs."""
    B, H, W, K = 5, 37, 53, 100
    g = torch.Generator().manual_seed(55)
    x1 = torch.rand(B, 1, H, W, generator=g).to(gpu)
    x2 = torch.rand(B, 1, H, W, generator=g).to(gpu)
    w = (torch.rand(B, generator=g) + 0.5).to(gpu)
    crit = MutualInformation(num_bins=K).to(gpu)
    (v32, _), (v64, _) = _references(crit, x1, x2, w)
    v, (g1, g2) = _run(crit, x1, x2, w, "both")
    e, e32 = _value_gate(v, v32, v64)
    print(f"\nindependent pairs | {describe(B, H * W, K)} | value: kernel {e:.2e}, float32 composition {e32:.2e}")
    assert len(set(v.tolist())) == B and float(g1.abs().max()) > 0 and float(g2.abs().max()) > 0
    perm = torch.tensor([3, 0, 4, 1, 2], device=gpu)
    vp, (g1p, g2p) = _run(crit, x1[perm].contiguous(), x2[perm].contiguous(), w[perm].contiguous(), "both")
    assert torch.equal(vp, v[perm]) and torch.equal(g1p, g1[perm]) and torch.equal(g2p, g2[perm])
    for k in (0, 2, 4):  # ... and pair k at every position of the batch
        r1, r2 = x1[k:k + 1].repeat(B, 1, 1, 1), x2[k:k + 1].repeat(B, 1, 1, 1)
        vr, (g1r, g2r) = _run(crit, r1, r2, None, "both")
        assert torch.equal(vr, v[k].expand(B))
        assert torch.equal(g1r, g1r[:1].expand_as(g1r)) and torch.equal(g2r, g2r[:1].expand_as(g2r))
        assert float(g1r.abs().max()) > 0 and float(g2r.abs().max()) > 0


# ------------------------------------------------------------------------------------------- 6. roles swapped
def test_roles_swapped(gpu):
    """MI(a, b) and MI(b, a) against ONE float64 value and ONE float64 gradient per image: the `which` /
    `transpose` / `m_offset` paths on a padded J (K = 100: Kp = 128, 2 x 2 blocks, 36 live bins in the last)."""
    B, H, W, K = 3, 37, 53, 100
    g = torch.Generator().manual_seed(66)
    a = torch.rand(B, 1, H, W, generator=g).to(gpu)
    b = (torch.rand(B, 1, H, W, generator=g) * 1.4 - 0.2).to(gpu)
    w = (torch.rand(B, generator=g) + 0.5).to(gpu)
    crit = MutualInformation(num_bins=K).to(gpu)
    (v32, (ga32, gb32)), (v64, (ga64, gb64)) = _references(crit, a, b, w)
    v_ab, (ga_first, gb_second) = _run(crit, a, b, w, "both")
    v_ba, (gb_first, ga_second) = _run(crit, b, a, w, "both")
    res = {"MI(a, b)": _value_gate(v_ab, v32, v64), "MI(b, a)": _value_gate(v_ba, v32, v64),
           "d/da as first": _grad_gate(ga_first, ga32, ga64, "a first"),
           "d/da as second": _grad_gate(ga_second, ga32, ga64, "a second"),
           "d/db as first": _grad_gate(gb_first, gb32, gb64, "b first"),
           "d/db as second": _grad_gate(gb_second, gb32, gb64, "b second")}
    print(f"\nroles swapped | {describe(B, H * W, K)} | "
          + "; ".join(f"{k}: kernel {e:.2e}, float32 composition {e32:.2e}" for k, (e, e32) in res.items()))


# ------------------------------------------------------------------------------------------- 7. buffers, images
@pytest.mark.parametrize("normalize", [True, False], ids=["normalised", "plain"])
def test_unsorted_nonuniform_bins(gpu, normalize):
    """bins = rand * 1.5 - 0.2: unsorted, non-uniform, beyond [0, 1] (the kernels take them as they are)."""
    g = torch.Generator().manual_seed(37)
    fixed, moving = (t.to(gpu) for t in _images("outside", 3, 19, 23, g))
    w = (torch.rand(3, generator=g) + 0.5).to(gpu)
    crit = MutualInformation(sigma=0.08, num_bins=37, normalize=normalize).to(gpu)
    with torch.no_grad():
        crit.bins.copy_((torch.rand(37, generator=g) * 1.5 - 0.2).to(gpu))
    assert bool((crit.bins[1:] < crit.bins[:-1]).any()) and float(crit.bins.max()) > 1 and float(crit.bins.min()) < 0
    _check(f"random bins normalize={normalize}", crit, fixed, moving, (w,))


@pytest.mark.parametrize("K", [256, 64])
def test_narrow_kernel_most_values_underflow(gpu, K):
    g = torch.Generator().manual_seed(5 + K)
    fixed, moving = (t.to(gpu) for t in _images("outside", 3, 19, 23, g))
    w = (torch.rand(3, generator=g) + 0.5).to(gpu)
    crit = MutualInformation(sigma=0.005, num_bins=K).to(gpu)
    _check(f"sigma=0.005 K={K}", crit, fixed, moving, (w,))


@pytest.mark.parametrize("kind", ["background", "on_bins"])
def test_background_and_on_bin_images(gpu, kind):
    g = torch.Generator().manual_seed(32)
    crit = MutualInformation(num_bins=32).to(gpu)
    fixed, moving = (t.to(gpu) for t in _images(kind, 3, 19, 23, g, bins=crit.bins))
    if kind == "background":
        assert float(fixed[..., :5].abs().max()) == 0 and float(moving[..., :6].abs().max()) == 0
    else:
        assert bool(torch.isin(moving, crit.bins).all())
    w = (torch.rand(3, generator=g) + 0.5).to(gpu)
    _check(f"{kind} images K=32", crit, fixed, moving, (w,))


# ------------------------------------------------------------------------------------------- 8. strides
def _raw_forward_backward(dev, x1, s1, x2, s2, B, H, W, crit, g_out):
    """ddrr_mi_forward and both ddrr_mi_backward through the binding, the way ops.mi_forward / ops.mi_backward
    call them, with the image pointers and strides as given.  -> out, state, grad x1, grad x2"""
    lib = _lib.get_mi_lib()
    bins, sigma = crit.bins.contiguous(), crit.sigma.contiguous()
    K = bins.numel()
    out = torch.empty(B, dtype=torch.float32, device=dev)
    state = torch.empty(B, int(lib.query("ddrr_mi_state_floats", K)), dtype=torch.float32, device=dev)
    n = int(lib.query("ddrr_mi_workspace_bytes", B, H, W, K))
    ws = torch.empty((n + 15) // 16, 4, dtype=torch.float32, device=dev)
    ops._launch_on(lib, "ddrr_mi_forward", dev, (
        x1.data_ptr(), s1, x2.data_ptr(), s2, B, H, W, bins.data_ptr(), K, sigma.data_ptr(), float(crit.epsilon),
        int(crit.normalize), ws.data_ptr(), ws.numel() * 4, out.data_ptr(), state.data_ptr()))
    grads = []
    for which in (0, 1):
        grad = torch.empty(B, H, W, dtype=torch.float32, device=dev)
        ops._launch_on(lib, "ddrr_mi_backward", dev, (
            x1.data_ptr(), s1, x2.data_ptr(), s2, B, H, W, bins.data_ptr(), K, sigma.data_ptr(), state.data_ptr(),
            which, g_out.data_ptr(), 1, grad.data_ptr()))
        grads.append(grad)
    torch.cuda.synchronize(dev)
    return out, state, grads[0], grads[1]


def test_strides_the_header_allows(gpu):
    """include/diffdrr_mi_hip.h: an image stride is 0 or any value >= H W.  The moving images as rows of a larger
    buffer at stride 2 N and at N + 1 (rows at odd dword offsets), the gaps filled with NaN so that a pixel read
    past a row shows: out, state and both gradients equal the contiguous call's bit for bit."""
    B, H, W, K = 4, 20, 24, 64
    N = H * W
    g = torch.Generator().manual_seed(88)
    fixed, moving = (t.to(gpu) for t in _images("unit", B, H, W, g))
    w = (torch.rand(B, generator=g) + 0.5).to(gpu)
    crit = MutualInformation(num_bins=K).to(gpu)
    x1 = fixed.reshape(N).contiguous()
    flat = moving.reshape(B, N).contiguous()
    want = _raw_forward_backward(gpu, x1, 0, flat, N, B, H, W, crit, w)
    with torch.no_grad():  # the raw call is the module's
        assert torch.equal(want[0], crit(fixed.expand(B, -1, -1, -1), moving))
    assert all(bool(torch.isfinite(t).all()) for t in want) and float(want[3].abs().max()) > 0
    for stride in (2 * N, N + 1):
        buf = torch.full((B, stride), float("nan"), device=gpu)
        buf[:, :N] = flat
        got = _raw_forward_backward(gpu, x1, 0, buf, stride, B, H, W, crit, w)
        for name, x, y in zip(("out", "state", "grad x1", "grad x2"), got, want):
            assert torch.equal(x, y), (stride, name)
        # ... and with the strided batch in the other role
        swapped = _raw_forward_backward(gpu, buf, stride, x1, 0, B, H, W, crit, w)
        ref = _raw_forward_backward(gpu, flat, N, x1, 0, B, H, W, crit, w)
        for name, x, y in zip(("out", "state", "grad x1", "grad x2"), swapped, ref):
            assert torch.equal(x, y), (stride, "swapped", name)


# ------------------------------------------------------------------------------------------- 9. empty batch
def test_empty_batch_launches_nothing(gpu, monkeypatch):
    launched = []
    monkeypatch.setattr(ops, "_launch_on", lambda lib, name, *a: launched.append(name))
    x1 = torch.zeros(0, 1, 8, 8, device=gpu, requires_grad=True)
    x2 = torch.zeros(0, 1, 8, 8, device=gpu, requires_grad=True)
    crit = MutualInformation(num_bins=64).to(gpu)
    v = crit(x1, x2)
    assert v.shape == (0,) and v.dtype == torch.float32 and v.requires_grad
    g1, g2 = torch.autograd.grad(v.sum(), [x1, x2])
    assert g1.shape == x1.shape and g2.shape == x2.shape
    assert not launched
