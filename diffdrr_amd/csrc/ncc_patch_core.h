// ncc_patch_core.h -- NormalizedCrossCorrelation2d(patch_size = p) per window / per pixel.
//
// Reference: diffdrr/metrics.py:16-44.  `to_patches` turns every p x p window (stride 1) of an
// (H, W) image into a channel; `norm` z-scores each window on its own (mean, biased variance + eps)
// and the score is the mean over windows and window pixels of z1 z2:
//     score = (1 / W') sum_w ncc_w,   ncc_w = (1 / n) sum_i (a_i - mu_a)(b_i - mu_b) / (s_a s_b),
//     n = p^2,  W' = (H - p + 1)(W - p + 1),  s = sqrt(var + eps).
// The reference materialises both images as (B, W', p, p) tensors (256^2, p = 13: 40 MB per image
// and pose) and a dozen more of that size in autograd; here a window is two passes over its p^2
// pixels in LDS (the reference's own two-pass arithmetic: mean, then centred moments), and the
// gradient w.r.t. the moving image b follows per pixel j from four per-window coefficients:
//     d score / d b_j = (1 / (W' n)) sum over the windows holding j of [ c1 (a_j - mu_a) - c3 (b_j - mu_b) ],
//     c1 = 1 / (s_a s_b),  c3 = ncc_w / s_b^2;  the window stores {c1, mu_a, c3, mu_b}.
// Radiographs have means of hundreds to thousands and vary by a fraction of a percent across a window,
// so nothing of the size of the mean is ever summed: the window's mean is taken relative to its first
// pixel (pivot a0: mu_a = a0 + mean(a - a0), a_i - mu_a = (a_i - a0) - mean(a - a0); the differences
// are exact or nearly so, the mean's rounding error scales with the window's variation), and the
// backward centres every term on its window's means before it adds them (the expanded form
// a_j S1 - sum(mu_a c1) - ... cancels p^2 products of size mean * c to a result of size (a - mu_a) c:
// 1e-4 of the largest gradient entry at p = 13 on such images, against 1e-6 for the fp32 composition).
// A window outside the grid is staged as four zeros and adds 0 * (a_j - 0) = 0 exactly.
// `fa(y, x)` / `fb(y, x)`: pixel (y, x) of the window (LDS tile on the device, the image on the host).
#pragma once

#include "ddrr_common.h"

namespace ddrr {

// P > 0: the window size as a compile-time constant (the rows unrolled: LDS offsets become immediates
// and the loop arithmetic goes -- the common sizes are instantiated, pose_ncc.hip), else `p`.
template <int P = 0, class FA, class FB>
DDRR_HD float ncc_patch_window(const FA &fa, const FB &fb, int p_rt, float eps, float coef[4]) {
    const int p = P > 0 ? P : p_rt;
    const float a0 = fa(0, 0), b0 = fb(0, 0);
    float sa = 0.f, sb = 0.f;
    for (int y = 0; y < p; ++y)
#pragma unroll
        for (int x = 0; x < (P > 0 ? P : p); ++x) {
            sa += fa(y, x) - a0;
            sb += fb(y, x) - b0;
        }
    const float inv_n = 1.0f / (float)(p * p);
    const float ra = sa * inv_n, rb = sb * inv_n, mua = a0 + ra, mub = b0 + rb;
    float va = 0.f, vb = 0.f, cab = 0.f;
    for (int y = 0; y < p; ++y)
#pragma unroll
        for (int x = 0; x < (P > 0 ? P : p); ++x) {
            const float da = (fa(y, x) - a0) - ra, db = (fb(y, x) - b0) - rb;
            va = fmaf(da, da, va);
            vb = fmaf(db, db, vb);
            cab = fmaf(da, db, cab);
        }
    const float var_b = fmaf(vb, inv_n, eps);
    const float stda = sqrtf(fmaf(va, inv_n, eps)), stdb = sqrtf(var_b);
    const float c1 = 1.0f / (stda * stdb);
    const float ncc = cab * inv_n * c1;
    coef[0] = c1;
    coef[1] = mua;
    coef[2] = ncc / var_b;
    coef[3] = mub;
    return ncc;
}

// `fc(wy, wx, k)`: coefficient k of the window whose top-left pixel is (wy, wx), 0 outside the
// window grid; the windows holding pixel (y, x) are wy in [y - p + 1, y], wx in [x - p + 1, x].
template <int P = 0, class FC>
DDRR_HD float ncc_patch_pixel_grad(const FC &fc, int y, int x, int p_rt, float a, float b) {
    const int p = P > 0 ? P : p_rt;
    float S1 = 0.f, S2 = 0.f, S3 = 0.f, S4 = 0.f;
    for (int wy = y - p + 1; wy <= y; ++wy)
#pragma unroll
        for (int k = 0; k < (P > 0 ? P : p); ++k) {
            const int wx = x - p + 1 + k;
            S1 = fmaf(fc(wy, wx, 0), a - fc(wy, wx, 1), S1);
            S3 = fmaf(fc(wy, wx, 2), b - fc(wy, wx, 3), S3);
        }
    return S1 - S3;
}

}  // namespace ddrr
