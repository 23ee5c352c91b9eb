"""What tests/test_wmi.py (the definition, no GPU) and tests/test_gpu_wmi.py (MI355X) share: the weighted mutual
information's torch composition (diffdrr_amd.metrics.weighted_mutual_information) as the yardstick, the scenes and
gates of tests/mi_cases.py, the weight patterns of tests/wncc_cases.py and the raw call of the library's entries.

The gates are mi_cases': the composition in float64 on the device is the yardstick, the same in float32 has an error
of its own against it, and the fused kernels may be off by at most twice that plus 2e-6 on a value and 2e-5 of the
largest gradient.  csrc/wmi.hip keeps csrc/mi.hip's launch geometry, so mi_cases.geometry / describe say which path
a case takes; only the workspace is larger, by the per-chunk sums of weights (:func:`workspace_floats`)."""
import contextlib

import torch

import mi_cases
from diffdrr_amd import _lib
from diffdrr_amd.metrics import weighted_mutual_information
from wncc_cases import PATTERNS, weights

F64, F32 = torch.float64, torch.float32


def workspace_floats(B, N, K):
    """ddrr_wmi_workspace_bytes / 4, restated: mi.hip's workspace and B (chunks + 1) doubles."""
    g = mi_cases.geometry(B, N, K)
    return g["workspace_floats"] + 2 * B * (g["chunks"] + 1)


def composition(crit, x1, x2, weight, dtype):
    return weighted_mutual_information(x1.to(dtype), x2.to(dtype), weight.to(dtype), crit.bins.to(dtype),
                                       crit.sigma.to(dtype), crit.epsilon, crit.normalize)


def weight4(pattern, B, H, W, per_pose, device):
    """wncc_cases.weights as ((1 | B), 1, H, W); None where the pattern does not apply"""
    w = weights(pattern, B, H, W, per_pose, device)
    return None if w is None else w.reshape(-1, 1, H, W)


def all_weights(B, H, W, device, patterns=PATTERNS):
    """[(label, weight ((1 | B), 1, H, W))]: every pattern shared and per pose"""
    out = []
    for pattern in patterns:
        for per_pose in (False, True):
            w = weight4(pattern, B, H, W, per_pose, device)
            if w is not None:
                out.append((f"{pattern} {'per pose' if per_pose else 'shared'}", w))
    return out


def run(fn, x1, x2, weight, g_w, grad_of):
    """value and d (v g_w).sum() / d the images in `grad_of` ('moving', 'fixed', 'both') of fn(x1 expanded, x2,
    weight); the leaves are the float32 images whatever `fn` computes in (mi_cases._run with a weight)."""
    a = x1.clone().requires_grad_(grad_of in ("fixed", "both"))
    b = x2.clone().requires_grad_(grad_of in ("moving", "both"))
    v = fn(a.expand(x2.shape[0], -1, -1, -1), b, weight)
    wanted = [t for t in (a, b) if t.requires_grad]
    grads = torch.autograd.grad((v * g_w).sum() if g_w is not None else v.sum(), wanted)
    return v.detach(), grads


def references(crit, x1, x2, weight, g_w):
    """(v32, (g32 fixed, g32 moving)), (v64, (g64 fixed, g64 moving)) of the composition; the float64 value has no
    NaN, so the NaN-matching branch of mi_cases._value_gate excuses nothing."""
    r32 = run(lambda a, b, w: composition(crit, a, b, w, F32), x1, x2, weight, g_w, "both")
    r64 = run(lambda a, b, w: composition(crit, a, b, w, F64), x1, x2, weight, g_w, "both")
    assert r64[0].dtype == F64 and not bool(torch.isnan(r64[0]).any()), r64[0]
    return r32, r64


@contextlib.contextmanager
def launches(ops):
    """the names of the entries of the weighted and of the unweighted MutualInformation library launched inside the
    block (wncc_cases.launches' scheme)"""
    names, real_w, real_on = [], ops._launch_wmi, ops._launch_on
    ops._launch_wmi = lambda name, device, *a: (names.append(name), real_w(name, device, *a))[1]
    ops._launch_on = lambda lib, name, device, args: (
        names.append(name) if name.startswith("ddrr_mi_") else None, real_on(lib, name, device, args))[1]
    try:
        yield names
    finally:
        ops._launch_wmi, ops._launch_on = real_w, real_on


def raw(ops, dev, x1, s1, x2, s2, w, sw, B, H, W, crit, g_out):
    """ddrr_wmi_forward and both ddrr_wmi_backward through the binding with the pointers and strides as given
    -> out, state, weight_sum, grad x1, grad x2"""
    lib = _lib.get_wmi_lib()
    bins, sigma = crit.bins.contiguous(), crit.sigma.contiguous()
    K = bins.numel()
    out = torch.empty(B, dtype=F32, device=dev)
    state = torch.empty(B, int(lib.query("ddrr_wmi_state_floats", K)), dtype=F32, device=dev)
    wsum = torch.empty(B, dtype=F64, device=dev)
    n = int(lib.query("ddrr_wmi_workspace_bytes", B, H, W, K))
    assert n == 4 * workspace_floats(B, H * W, K), (n, B, H, W, K)
    ws = torch.empty((n + 15) // 16, 4, dtype=F32, device=dev)
    ops._launch_on(lib, "ddrr_wmi_forward", dev, (
        x1.data_ptr(), s1, x2.data_ptr(), s2, w.data_ptr(), sw, B, H, W, bins.data_ptr(), K, sigma.data_ptr(),
        float(crit.epsilon), int(crit.normalize), ws.data_ptr(), ws.numel() * 4, out.data_ptr(), state.data_ptr(),
        wsum.data_ptr()))
    grads = []
    for which in (0, 1):
        grad = torch.empty(B, H, W, dtype=F32, device=dev)
        ops._launch_on(lib, "ddrr_wmi_backward", dev, (
            x1.data_ptr(), s1, x2.data_ptr(), s2, w.data_ptr(), sw, B, H, W, bins.data_ptr(), K, sigma.data_ptr(),
            state.data_ptr(), which, g_out.data_ptr(), 1, grad.data_ptr()))
        grads.append(grad)
    torch.cuda.synchronize(dev)
    return out, state, wsum, grads[0], grads[1]
