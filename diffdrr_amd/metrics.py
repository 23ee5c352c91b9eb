"""Image similarities of the registration / sweep paths.

Normalised cross-correlation -- whole-image, patch-wise, multiscale -- and its gradient
variant (reference ``diffdrr/metrics.py:16-104``), pinned to ``tests/golden/metrics.npz``, values
and autograd gradients of the unmodified reference; and mutual information (reference
``metrics.py:110-139``, kornia's ``marginal_pdf`` / ``joint_pdf`` restated), pinned to a float64
restatement of its formula (tests/test_mutual_information.py).  The geodesic pose metrics are out
of scope.
"""
from __future__ import annotations

import torch

from . import _lib, ops


class _NCCFn(torch.autograd.Function):
    """Whole-image NCC of single-channel image pairs as one kernel each way
    (ddrr_ncc_forward / ddrr_ncc_backward).  x1 (B or 1, N), x2 (B, N) -> (B,)."""

    @staticmethod
    def forward(ctx, x1, x2, eps):
        out, stats = ops.ncc_forward(x1, x2, eps)
        ctx.save_for_backward(x1, x2, stats)
        return out

    @staticmethod
    def backward(ctx, g):
        x1, x2, stats = ctx.saved_tensors
        need1, need2 = ctx.needs_input_grad[:2]
        shared = x1.shape[0] == 1 and x2.shape[0] != 1
        if need1 and shared:
            # a fixed image shared by the batch: its gradient is a sum over the batch;
            # rare (the fixed image is data), so take the general route
            g1, g2 = ops.ncc_backward(x1.expand_as(x2).contiguous(), x2, stats, g, True, need2)
            return g1.sum(0, keepdim=True), g2, None
        g1, g2 = ops.ncc_backward(x1, x2, stats, g, need1, need2)
        return g1, g2, None


class _PatchNCCFn(torch.autograd.Function):
    """Patch-wise NCC (``patch_size = p``) of single-channel image pairs without the reference's
    (B, windows, p, p) tensors: ddrr_ncc_patch_forward / ddrr_ncc_patch_backward.
    x1 (B or 1, H, W), x2 (B, H, W) -> (B,).  The gradient w.r.t. the moving image x2 is one launch;
    one w.r.t. x1 (the fixed image is data: rare) is the same two launches with the roles swapped --
    the similarity is symmetric."""

    @staticmethod
    def forward(ctx, x1, x2, p, eps):
        out, coef = ops.ncc_patch_forward(x1, x2, p, eps, want_coef=ctx.needs_input_grad[1])
        ctx.p, ctx.eps = p, eps
        ctx.save_for_backward(x1, x2, coef)
        return out

    @staticmethod
    def backward(ctx, g):
        x1, x2, coef = ctx.saved_tensors
        g1 = g2 = None
        if ctx.needs_input_grad[1]:
            g2 = ops.ncc_patch_backward(x1, x2, coef, g, ctx.p)
        if ctx.needs_input_grad[0]:
            a = x1.expand_as(x2).contiguous()
            _, coef1 = ops.ncc_patch_forward(x2, a, ctx.p, ctx.eps)
            g1 = ops.ncc_patch_backward(x2, a, coef1, g, ctx.p)
            if x1.shape[0] == 1 and x2.shape[0] != 1:
                g1 = g1.sum(0, keepdim=True)
        return g1, g2, None, None


class _WeightedNCCFn(torch.autograd.Function):
    """Whole-image NCC under per-pixel weights (include/diffdrr_wncc_hip.h: ddrr_wncc_forward /
    ddrr_wncc_backward).  x1 (B or 1, N), x2 (B, N), w (B or 1, N) -> (B,); no gradient w.r.t. w."""

    @staticmethod
    def forward(ctx, x1, x2, w, eps):
        out, stats = ops.wncc_forward(x1, x2, w, eps)
        ctx.save_for_backward(x1, x2, w, stats)
        return out

    @staticmethod
    def backward(ctx, g):
        x1, x2, w, stats = ctx.saved_tensors
        need1, need2 = ctx.needs_input_grad[:2]
        if need1 and x1.shape[0] == 1 and x2.shape[0] != 1:
            # (a fixed image shared by the batch: its gradient is a sum over the batch, as in _NCCFn)
            g1, g2 = ops.wncc_backward(x1.expand_as(x2).contiguous(), x2, w, stats, g, True, need2)
            return g1.sum(0, keepdim=True), g2, None, None
        g1, g2 = ops.wncc_backward(x1, x2, w, stats, g, need1, need2)
        return g1, g2, None, None


def weighted_ncc(x1, x2, weight, eps=1e-5):
    """The weighted NCC of include/diffdrr_wncc_hip.h as a torch composition: x1, x2 (B, C, H, W), weight
    ((1 | B), 1, H, W) >= 0 -> (B,), the mean over the channels of
        (sum_V w x1 x2 / Sw - mu1 mu2) / (s1 s2),  mu = sum_V w x / Sw,  s = sqrt(sum_V w (x - mu)^2 / Sw + eps),
    V = {w != 0}: a pixel outside V is selected out (NaN there is safe), a channel with Sw <= 0 scores 0.
    Differentiable in x1, x2 and the weight."""
    on = weight != 0
    w = torch.where(on, weight, torch.zeros_like(weight))
    Sw = w.sum(dim=(-1, -2), keepdim=True)
    some = Sw > 0
    inv = torch.where(some, 1.0 / torch.where(some, Sw, torch.ones_like(Sw)), torch.zeros_like(Sw))

    def centred(x):
        x = torch.where(on, x, torch.zeros_like(x))
        d = torch.where(on, x - (w * x).sum(dim=(-1, -2), keepdim=True) * inv, torch.zeros_like(x))
        return d, ((w * d * d).sum(dim=(-1, -2), keepdim=True) * inv + eps).sqrt()

    (d1, s1), (d2, s2) = centred(x1), centred(x2)
    ncc = (w * d1 * d2).sum(dim=(-1, -2), keepdim=True) * inv / (s1 * s2)
    return ncc.flatten(1).mean(dim=1)


def to_patches(x, patch_size):
    """Every ``patch_size`` x ``patch_size`` window (stride 1) becomes one channel
    whose spatial extent is the window, so that :meth:`norm` z-scores each window
    on its own (local NCC), as in reference metrics.py:16-18."""
    x = x.unfold(2, patch_size, 1).unfold(3, patch_size, 1)  # b c h' w' p1 p2
    b, c, h, w, p1, p2 = x.shape
    return x.reshape(b, c * h * w, p1, p2)


class NormalizedCrossCorrelation2d(torch.nn.Module):
    """Mean of the product of the two z-scored images (global or patch-wise)."""

    def __init__(self, patch_size=None, eps=1e-5):
        super().__init__()
        self.patch_size = patch_size
        self.eps = eps

    def forward(self, x1, x2, weight=None):
        """``weight`` ((1 | B), 1, H, W), >= 0 and finite: the weighted (masked) NCC of
        include/diffdrr_wncc_hip.h -- pixels with weight 0 are not read (NaN there is safe), the same weight
        for every channel, the mean of the channels' values.  float32 images on the device and a weight that
        takes no gradient go through the kernels, everything else through :func:`weighted_ncc`."""
        if weight is not None:
            return self._weighted(x1, x2, weight)
        if (self.patch_size is not None and not getattr(self, "_no_patch_kernel", False)
                and x1.dim() == 4 and x1.shape == x2.shape and ops.on_device(x2)
                and x1.device == x2.device and x1.dtype == x2.dtype == torch.float32
                and 1 <= int(self.patch_size) <= min(x2.shape[-2], x2.shape[-1], 64)):
            # local NCC without `to_patches`: every window z-scored in LDS; the channels are
            # independent images (the reference's mean over (c h' w') windows = the mean over channels
            # of the per-channel means); an `expand`ed fixed image is read once, in place
            b, c, h, w = x2.shape
            shared = b > 1 and x1.stride(0) == 0 and c == 1
            a = (x1[:1] if shared else x1).reshape(1 if shared else b * c, h, w)
            val = _PatchNCCFn.apply(a, x2.reshape(b * c, h, w), int(self.patch_size), self.eps)
            return val.reshape(b, c).mean(dim=1) if c > 1 else val
        if self.patch_size is not None:
            x1 = to_patches(x1, self.patch_size)
            x2 = to_patches(x2, self.patch_size)
        assert x1.shape == x2.shape, "Input images must be the same size"
        _, c, h, w = x1.shape
        if (self.patch_size is None and c == 1 and ops.on_device(x2) and x1.device == x2.device
                and x1.dtype == x2.dtype == torch.float32):
            # one fused kernel per direction; an `expand`ed fixed image is read once per pose
            # from the same memory instead of being materialised
            b = x2.shape[0]
            shared = b > 1 and x1.stride(0) == 0
            a = (x1[:1] if shared else x1).reshape(1 if shared else b, h * w)
            return _NCCFn.apply(a, x2.reshape(b, h * w), self.eps)
        score = (self.norm(x1) * self.norm(x2)).flatten(1).sum(1)
        return score / (c * h * w)

    def _weighted(self, x1, x2, weight):
        if self.patch_size is not None:
            raise ValueError("a weight with patch_size is not supported: weighted windows are out of scope")
        assert x1.shape == x2.shape, "Input images must be the same size"
        b, c, h, w = x2.shape
        if weight.dim() != 4 or weight.shape[0] not in (1, b) or tuple(weight.shape[1:]) != (1, h, w):
            raise ValueError(f"weight has shape {tuple(weight.shape)}: (1 | {b}, 1, {h}, {w}) expected")
        if (ops.on_device(x2) and x1.device == x2.device == weight.device
                and x1.dtype == x2.dtype == weight.dtype == torch.float32
                and b * c <= _lib.WNCC_MAX_POSES  # (pairs of one launch; beyond: the composition)
                and not (torch.is_grad_enabled() and weight.requires_grad)):
            shared = b > 1 and x1.stride(0) == 0 and c == 1
            a = (x1[:1] if shared else x1).reshape(1 if shared else b * c, h * w)
            # (one weight for the batch, given so or `expand`ed, is read in place; per-pose weights repeat per channel)
            if weight.shape[0] == 1 or (b > 1 and weight.stride(0) == 0):
                wt = weight[:1].reshape(1, h * w)
            else:
                wt = weight.expand(b, c, h, w).reshape(b * c, h * w)
            val = _WeightedNCCFn.apply(a, x2.reshape(b * c, h * w), wt, self.eps)
            return val.reshape(b, c).mean(dim=1) if c > 1 else val
        return weighted_ncc(x1, x2, weight, self.eps)

    def norm(self, x):
        mu = x.mean(dim=[-1, -2], keepdim=True)
        var = x.var(dim=[-1, -2], keepdim=True, correction=0) + self.eps
        return (x - mu) / var.sqrt()


class _SobelFn(torch.autograd.Function):
    """(B, 1, H, W) -> (B, 2, H, W) Sobel responses, zero padding: ddrr_sobel_forward / its
    adjoint ddrr_sobel_backward (reference metrics.py:69-94, torch.nn.Conv2d(1, 2, 3, padding=1))."""

    @staticmethod
    def forward(ctx, x):
        return ops.sobel_forward(x[:, 0])

    @staticmethod
    def backward(ctx, g):
        return ops.sobel_backward(g).unsqueeze(1)


class _BlurSobelFn(torch.autograd.Function):
    """(B, 1, H, W) -> (B, 2, H, W): Gaussian blur (reflect padding) + Sobel pair, one launch each way:
    ddrr_blur_sobel_forward / ddrr_blur_sobel_backward (reference metrics.py:88-93)."""

    @staticmethod
    def forward(ctx, x, taps):
        ctx.taps = taps
        return ops.blur_sobel_forward(x[:, 0], taps)

    @staticmethod
    def backward(ctx, g):
        return ops.blur_sobel_backward(g, ctx.taps).unsqueeze(1), None


def gaussian_taps(kernel_size, sigma, dtype=torch.float32, device=None):
    """The 1-D taps of torchvision's gaussian_blur (see :func:`gaussian_blur`)."""
    half = (kernel_size - 1) * 0.5
    x = torch.linspace(-half, half, steps=kernel_size, dtype=dtype, device=device)
    k1 = torch.exp(-0.5 * (x / sigma).pow(2))
    return k1 / k1.sum()


def gaussian_blur(img, kernel_size, sigma):
    """torchvision.transforms.functional.gaussian_blur as the reference's ``Sobel`` calls it
    (metrics.py:66, 88-92; torchvision is a third-party dependency that is neither vendored by
    the reference nor installed here: restated from its published algorithm): taps exp(-x^2 / 2 sigma^2) on
    linspace(-(k-1)/2, (k-1)/2, k), normalised, separable, REFLECT padding by k // 2.  A few tensor
    ops on (B, 1, H, W) images; differentiable by autograd."""
    k1 = gaussian_taps(kernel_size, sigma, img.dtype, img.device)
    c = img.shape[-3]
    kernel = torch.mm(k1[:, None], k1[None, :]).expand(c, 1, kernel_size, kernel_size)
    pad = [kernel_size // 2] * 4
    return torch.nn.functional.conv2d(torch.nn.functional.pad(img, pad, mode="reflect"), kernel, groups=c)


class Sobel(torch.nn.Module):
    """Optional Gaussian blur, then the x / y Sobel responses (reference metrics.py:69-94)."""

    def __init__(self, sigma: float):
        super().__init__()
        self.sigma = sigma
        self._taps = {}  # device -> the blur's taps there (computed on the host as torchvision does)

    def forward(self, img):
        x = img
        if self.sigma > 0:
            k = int(6 * self.sigma + 1) | 1
            if (img.dim() == 4 and img.shape[1] == 1 and ops.on_device(img) and img.dtype == torch.float32
                    and k <= 31 and k // 2 < min(img.shape[-2:]) and not getattr(self, "_no_blur_kernel", False)):
                key = (img.device, float(self.sigma))
                if key not in self._taps:
                    self._taps = {key: gaussian_taps(k, self.sigma).to(img.device)}
                return _BlurSobelFn.apply(img, self._taps[key])
            x = gaussian_blur(img, k, self.sigma)
        if (x.shape[1] == 1 and ops.on_device(x) and x.dtype == torch.float32):
            return _SobelFn.apply(x)
        Gx = torch.tensor([[1, 0, -1], [2, 0, -2], [1, 0, -1]], dtype=x.dtype, device=x.device)
        Gy = torch.tensor([[1, 2, 1], [0, 0, 0], [-1, -2, -1]], dtype=x.dtype, device=x.device)
        return torch.nn.functional.conv2d(x, torch.stack([Gx, Gy]).unsqueeze(1), padding=1)


class GradientNormalizedCrossCorrelation2d(NormalizedCrossCorrelation2d):
    """NCC between the image gradients of two batches of images (reference metrics.py:97-104):
    the Sobel pair by one kernel each way, the two channels' whole-image NCCs by the fused NCC
    kernels (their mean is the reference's sum over (c, h, w) / (c h w))."""

    def __init__(self, patch_size=None, sigma=1.0, **kwargs):
        super().__init__(patch_size, **kwargs)
        self.sobel = Sobel(sigma)

    def forward(self, x1, x2, weight=None):
        g1, g2 = self.sobel(x1), self.sobel(x2)
        if weight is not None:  # (the same weight for both Sobel channels, through the weighted kernels)
            return self._weighted(g1, g2, weight)
        b, c, h, w = g2.shape
        if (self.patch_size is None and c == 2 and ops.on_device(g2) and g1.shape == g2.shape
                and g2.dtype == torch.float32):
            # every channel is z-scored on its own: 2 B single-channel pairs for the fused kernels
            val = _NCCFn.apply(g1.reshape(b * c, h * w), g2.reshape(b * c, h * w), self.eps)
            return val.reshape(b, c).mean(dim=1)
        return super().forward(g1, g2)


class MultiscaleNormalizedCrossCorrelation2d(torch.nn.Module):
    """Weighted sum of NCCs at several patch sizes (``None`` = whole image)."""

    def __init__(self, patch_sizes=[None], patch_weights=[1.0], eps=1e-5):
        super().__init__()
        assert len(patch_sizes) == len(patch_weights), "Each scale must have a weight"
        # (like the reference, metrics.py:53-55, the members keep the default eps)
        self.nccs = [NormalizedCrossCorrelation2d(p) for p in patch_sizes]
        self.patch_weights = patch_weights

    def forward(self, x1, x2, weight=None):
        # sum_i w_i ncc_i (reference metrics.py:58-63: the weighted scores stacked and summed) with one
        # launch per scale: the first scaled, the others added with their weight as `alpha`
        if weight is not None and any(ncc.patch_size is not None for ncc in self.nccs):
            raise ValueError("a weight applies to whole-image scales only: weighted windows are out of scope")
        total = None
        for w, ncc in zip(self.patch_weights, self.nccs):
            v = ncc(x1, x2) if weight is None else ncc(x1, x2, weight=weight)
            if total is None:
                total = v * w
            elif isinstance(w, (int, float)):
                total = torch.add(total, v, alpha=w)
            else:  # (a tensor weight)
                total = total + v * w
        return total


def _mi_image_grads(ctx, g, backward):
    """The backward of :class:`_MIFn` and :class:`_WeightedMIFn`: one launch of `backward` per image that wants a
    gradient; an image shared by the batch gets the sum over the poses."""
    *inputs, state = ctx.saved_tensors  # x1, x2, [w,] bins, sigma
    grads = [None, None]
    for which in (0, 1):
        if ctx.needs_input_grad[which]:
            gx = backward(*inputs, state, g, which, ctx.B)
            grads[which] = gx.sum(0, keepdim=True) if (inputs[which].shape[0] == 1 and ctx.B != 1) else gx
    return (*grads, *[None] * (len(inputs) + 1))


class _MIFn(torch.autograd.Function):
    """MutualInformation of single-channel image pairs without the reference's (B, H W, K) kernel-value
    tensors: ddrr_mi_forward / ddrr_mi_backward (include/diffdrr_mi_hip.h).  x1, x2 (B or 1, H, W) -> (B,)
    (B given: both images may be one shared image);
    bins and sigma are the module's buffers, read on the device.  The gradient w.r.t. either image is one
    launch (the similarity is symmetric: the same kernel with the roles swapped)."""

    @staticmethod
    def forward(ctx, x1, x2, bins, sigma, epsilon, normalize, B):
        want = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        out, state = ops.mi_forward(x1, x2, bins, sigma, epsilon, normalize, B, want_state=want)
        ctx.B = B
        ctx.save_for_backward(x1, x2, bins, sigma, state)
        return out

    @staticmethod
    def backward(ctx, g):
        return _mi_image_grads(ctx, g, ops.mi_backward)


def mutual_information(x1, x2, bins, sigma, epsilon=1e-10, normalize=True):
    """The reference's MutualInformation as a torch composition (kornia's marginal_pdf / joint_pdf
    restated): x1, x2 (B, 1, H, W) -> (B,).  Materialises (B, H W, K) kernel values."""
    B = x1.shape[0]
    k1 = torch.exp(-0.5 * ((x1.reshape(B, -1, 1) - bins) / sigma).pow(2))
    k2 = torch.exp(-0.5 * ((x2.reshape(B, -1, 1) - bins) / sigma).pow(2))
    p1 = k1.mean(dim=1)
    p1 = p1 / (p1.sum(dim=1, keepdim=True) + epsilon)
    p2 = k2.mean(dim=1)
    p2 = p2 / (p2.sum(dim=1, keepdim=True) + epsilon)
    joint = torch.matmul(k1.transpose(1, 2), k2)
    p12 = joint / (joint.sum(dim=(1, 2)).view(-1, 1, 1) + 1e-10)  # (joint_pdf's own epsilon)
    h1 = -(p1 * (p1 + epsilon).log2()).sum(dim=1)
    h2 = -(p2 * (p2 + epsilon).log2()).sum(dim=1)
    h12 = -(p12 * (p12 + epsilon).log2()).sum(dim=(1, 2))
    mi = h1 + h2 - h12
    if normalize:
        mi = 2 * mi / (h1 + h2)
    return mi


class _WeightedMIFn(torch.autograd.Function):
    """:class:`_MIFn` under per-pixel weights: ddrr_wmi_forward / ddrr_wmi_backward (include/diffdrr_wmi_hip.h).
    x1, x2, w (B or 1, H, W) -> (B,); no gradient w.r.t. w."""

    @staticmethod
    def forward(ctx, x1, x2, w, bins, sigma, epsilon, normalize, B):
        want = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        out, state = ops.wmi_forward(x1, x2, w, bins, sigma, epsilon, normalize, B, want_state=want)
        ctx.B = B
        ctx.save_for_backward(x1, x2, w, bins, sigma, state)
        return out

    @staticmethod
    def backward(ctx, g):
        return _mi_image_grads(ctx, g, ops.wmi_backward)


def weighted_mutual_information(x1, x2, weight, bins, sigma, epsilon=1e-10, normalize=True):
    """The weighted mutual information of include/diffdrr_wmi_hip.h as a torch composition: x1, x2 (B, 1, H, W),
    weight ((1 | B), 1, H, W) >= 0 -> (B,).  :func:`mutual_information` with every sum over the pixels weighted,
    and the mean of the marginals taken with Sw = sum_n w[n]:
        P1[k] = sum_n w[n] k1[n,k] / Sw,   J[k,l] = sum_n w[n] k1[n,k] k2[n,l].
    A pixel of weight 0 is selected out (NaN or Inf there is safe, its gradient is exactly 0); a pair with Sw = 0
    scores 0 with a zero gradient.  With weight = 1 everywhere: :func:`mutual_information`'s value and gradient.
    Any dtype, any device; differentiable in x1, x2 and the weight.  Materialises (B, H W, K) kernel values."""
    B = x1.shape[0]
    w = weight.expand(B, -1, -1, -1).reshape(B, -1, 1)
    on = w != 0
    w = torch.where(on, w, torch.zeros_like(w))
    Sw = w.sum(dim=1)  # (B, 1)
    some = Sw > 0
    Sw1 = torch.where(some, Sw, torch.ones_like(Sw))

    def kernel_values(x):
        x = torch.where(on, x.reshape(B, -1, 1), torch.zeros_like(w))
        return torch.exp(-0.5 * ((x - bins) / sigma).pow(2))

    k1, k2 = kernel_values(x1), kernel_values(x2)
    wk1 = torch.where(on, w * k1, torch.zeros_like(k1))
    p1 = wk1.sum(dim=1) / Sw1
    p1 = p1 / (p1.sum(dim=1, keepdim=True) + epsilon)
    p2 = torch.where(on, w * k2, torch.zeros_like(k2)).sum(dim=1) / Sw1
    p2 = p2 / (p2.sum(dim=1, keepdim=True) + epsilon)
    joint = torch.matmul(wk1.transpose(1, 2), k2)
    p12 = joint / (joint.sum(dim=(1, 2)).view(-1, 1, 1) + 1e-10)  # (joint_pdf's own epsilon)
    h1 = -(p1 * (p1 + epsilon).log2()).sum(dim=1)
    h2 = -(p2 * (p2 + epsilon).log2()).sum(dim=1)
    h12 = -(p12 * (p12 + epsilon).log2()).sum(dim=(1, 2))
    mi = h1 + h2 - h12
    some = some.reshape(B)
    if normalize:
        # (an empty pair has h1 + h2 = 0: the divisor is selected, so there is no 0 / 0 in the graph)
        mi = 2 * mi / torch.where(some, h1 + h2, torch.ones_like(h1))
    return torch.where(some, mi, torch.zeros_like(mi))


class MutualInformation(torch.nn.Module):
    """(Normalised) mutual information of two batches of single-channel images from Gaussian-kernel
    density estimates of their marginal and joint intensity distributions (reference metrics.py:110-139).
    float32 images on the device take the fused kernels (num_bins <= 256); everything else -- CPU,
    float64, more bins, ``bins`` / ``sigma`` that require grad (the kernels differentiate the images
    only) -- the torch composition :func:`mutual_information`.  With ``weight=``: the weighted (masked)
    criterion, see :meth:`forward`."""

    def __init__(self, sigma=0.1, num_bins=256, epsilon=1e-10, normalize=True):
        super().__init__()
        self.register_buffer("sigma", torch.tensor(sigma))
        self.register_buffer("bins", torch.linspace(0.0, 1.0, num_bins))
        self.epsilon = epsilon
        self.normalize = normalize

    def forward(self, x1, x2, weight=None):
        """``weight`` ((1 | B), 1, H, W), >= 0 and finite: the weighted (masked) mutual information of
        include/diffdrr_wmi_hip.h -- pixels with weight 0 are not read (NaN there is safe) and get the gradient
        0, a pair whose weights are all 0 scores 0.  float32 images, buffers and weight on the device, with a
        weight that takes no gradient, go through the kernels of that library (num_bins <= 256); everything else
        through :func:`weighted_mutual_information`."""
        if x1.shape != x2.shape:
            raise ValueError(f"Input images must be the same size: {tuple(x1.shape)} and {tuple(x2.shape)}")
        if x1.dim() != 4 or x1.shape[1] != 1:
            raise ValueError(f"MutualInformation takes (B, 1, H, W) images, got {tuple(x1.shape)}")
        if weight is not None:
            return self._weighted(x1, x2, weight)
        if self._fused(x1, x2):
            # (the batch size is passed: both images may be expanded)
            return _MIFn.apply(*self._images(x1, x2), self.bins, self.sigma, float(self.epsilon),
                               bool(self.normalize), x1.shape[0])
        return mutual_information(x1, x2, self.bins, self.sigma, self.epsilon, self.normalize)

    def _fused(self, x1, x2, *weight):
        """Whether the kernels serve the call: float32 images, buffers (and weight) on the device, a bin count
        the library takes, and no gradient wanted for anything but the images."""
        H, W = x2.shape[-2:]
        buffers = (self.bins, self.sigma, *weight)
        return (ops.on_device(x2) and all(t.device == x2.device and t.dtype == torch.float32 for t in (x1, x2, *buffers))
                and self.sigma.numel() == 1 and H * W > 0
                and 1 <= self.bins.numel() <= (_lib.WMI_MAX_BINS if weight else _lib.MI_MAX_BINS)
                and not (torch.is_grad_enabled() and any(t.requires_grad for t in buffers)))

    @staticmethod
    def _images(x1, x2):
        """(B | 1, H, W) of each: an `expand`ed image (the fixed one, usually) is read once per pose from the same
        memory"""
        B = x2.shape[0]
        return tuple(x[:1, 0] if (B > 1 and x.stride(0) == 0) else x[:, 0] for x in (x1, x2))

    def _weighted(self, x1, x2, weight):
        B, _, H, W = x2.shape
        if weight.dim() != 4 or weight.shape[0] not in (1, B) or tuple(weight.shape[1:]) != (1, H, W):
            raise ValueError(f"weight has shape {tuple(weight.shape)}: (1 | {B}, 1, {H}, {W}) expected")
        if self._fused(x1, x2, weight):
            a, b = self._images(x1, x2)
            # (one weight for the batch, given so or `expand`ed, is read in place)
            w = weight[:1, 0] if (weight.shape[0] == 1 or (B > 1 and weight.stride(0) == 0)) else weight[:, 0]
            return _WeightedMIFn.apply(a, b, w.detach(), self.bins, self.sigma, float(self.epsilon),
                                       bool(self.normalize), B)
        return weighted_mutual_information(x1, x2, weight, self.bins, self.sigma, self.epsilon, self.normalize)
