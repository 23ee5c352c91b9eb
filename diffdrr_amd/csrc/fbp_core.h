// fbp_core.h -- the per-pixel and per-voxel arithmetic of include/diffdrr_fbp_hip.h, shared by the
// gfx950 kernels (fbp.hip) and the host build the tests loop over volumes and image lines
// (tests/emu/fbp_emu.cpp).  Plain C++: no HIP types, no memory model.
#pragma once

#include <float.h>
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FBP_HD __host__ __device__ __forceinline__
#else
#define FBP_HD inline
#endif

namespace fbp {

// 1 / x to within an ulp: on the device the hardware's reciprocal and one Newton step (a correctly rounded
// division is ten more instructions, four times per voxel and view, with denormals honoured)
FBP_HD float reciprocal(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float r = __builtin_amdgcn_rcpf(x);
    return fmaf(fmaf(-x, r, 1.f), r, r);
#else
    return 1.f / x;
#endif
}

// ------------------------------------------------------------------------------------------ filter
// images[r, c] * cw(r, c), rounded to float once: what a line holds before it is convolved
FBP_HD float weighted_pixel(float pixel, int r, int c, float u0, float du, float v0, float dv, float sdd,
                            int cosine_weight) {
    if (!cosine_weight) return pixel;
    const double u = fma((double)c, (double)du, (double)u0), v = fma((double)r, (double)dv, (double)v0);
    const double s = (double)sdd;
    return (float)((double)pixel * (s / sqrt(fma(u, u, fma(v, v, s * s)))));
}

// scale * sum_k taps[(n - k) + L - 1] line[k], k ascending; the products are exact in double, the sum is
// rounded to float once
FBP_HD float convolve(const float *line, const float *taps, int L, int n, float scale) {
    const float *t = taps + n + L - 1;  // t[-k] = the tap of lag n - k
    double s = 0.0;
    for (int k = 0; k < L; ++k) s = fma((double)t[-k], (double)line[k], s);
    return (float)(s * (double)scale);
}

// ---------------------------------------------------------------------------------- backprojection
// What the voxels (i, j, .) share of one view's homogeneous pixel coordinates: the (i, j, 1) part of
// M (i, j, k, 1)^T.  k comes last (accumulate_view()), so every voxel's coordinates are three fused
// multiply-adds per component from the matrix -- none is stepped from a neighbour's.
struct Row {
    double a, b, u;
};

FBP_HD Row row_of(const float *view, int i, int j) {
    Row p;
    p.a = fma((double)view[1], (double)j, fma((double)view[0], (double)i, (double)view[3]));
    p.b = fma((double)view[5], (double)j, fma((double)view[4], (double)i, (double)view[7]));
    p.u = fma((double)view[9], (double)j, fma((double)view[8], (double)i, (double)view[11]));
    return p;
}

// floor(q) and the fraction q - floor(q) of q = num / den, where `approx` is num / den to a few float
// ulps and `rden` is 1 / den as a float: the fraction comes from the exact remainder num - floor den, so
// it is good to 2^-22 ABSOLUTE, wherever on the detector q is (a float q itself is good to 2^-18 at
// column 64: forty times the rounding of everything that follows).
FBP_HD void split(double num, double den, float approx, float rden, int &whole, float &frac) {
    float w = floorf(approx);
    frac = (float)fma(-(double)w, den, num) * rden;
    if (frac < 0.f) w -= 1.f, frac += 1.f;         // (approx was on the other side of an integer)
    else if (frac >= 1.f) w += 1.f, frac -= 1.f;
    whole = (int)w;
}

FBP_HD float pixel_or_zero(const float *img, int H, int W, int r, int c) {
    const bool inside = r >= 0 && r < H && c >= 0 && c < W;
    const int rc = r < 0 ? 0 : (r >= H ? H - 1 : r), cc = c < 0 ? 0 : (c >= W ? W - 1 : c);
    const float v = img[(long)rc * W + cc];  // (always a pixel of the image: H, W >= 1)
    return inside ? v : 0.f;
}

// acc + w_b (distance_weight ? 1 / U^2 : 1) bilinear(img, row, col) for the voxel k of `p`'s row;
// `acc` itself where the view contributes nothing.  H, W >= 1.  Straight-line code: a view that contributes
// nothing is carried as a flag and its four loads go to clamped addresses, so a lane's gathers for its
// voxels are all in flight together instead of one voxel's after another's.
FBP_HD float accumulate_view(float acc, const float *img, int H, int W, const float *view, const Row &p, int k,
                             int distance_weight) {
    const double a = fma((double)view[2], (double)k, p.a);
    const double b = fma((double)view[6], (double)k, p.b);
    const double u = fma((double)view[10], (double)k, p.u);
    const float uf = (float)u;
    bool ok = uf > 0.f && uf <= FLT_MAX;  // (not behind the source, and a number)
    const float rden = reciprocal(ok ? uf : 1.f);
    float qc = (float)a * rden, qr = (float)b * rden;
    // (one pixel of margin for the approximation; NaN and infinities fail the comparisons)
    ok = ok && qc > -2.f && qc < (float)W + 1.f && qr > -2.f && qr < (float)H + 1.f;
    qc = ok ? qc : 0.f, qr = ok ? qr : 0.f;
    int c0, r0;
    float fc, fr;
    split(a, u, qc, rden, c0, fc);
    split(b, u, qr, rden, r0, fr);
    ok = ok && c0 >= -1 && c0 < W && r0 >= -1 && r0 < H;  // (else all four neighbours are outside)
    const float i00 = pixel_or_zero(img, H, W, r0, c0), i01 = pixel_or_zero(img, H, W, r0, c0 + 1);
    const float i10 = pixel_or_zero(img, H, W, r0 + 1, c0), i11 = pixel_or_zero(img, H, W, r0 + 1, c0 + 1);
    const float gc = 1.f - fc, gr = 1.f - fr;
    const float top = fmaf(i01, fc, i00 * gc), bottom = fmaf(i11, fc, i10 * gc);
    const float value = fmaf(bottom, fr, top * gr);
    const float w = distance_weight ? view[12] * (rden * rden) : view[12];
    return ok ? fmaf(w, value, acc) : acc;
}

}  // namespace fbp
