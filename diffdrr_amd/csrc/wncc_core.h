// wncc_core.h -- the arithmetic of the weighted (masked) NCC kernels (wncc.hip; include/diffdrr_wncc_hip.h
// has the definitions): the update of the six raw moments with the w == 0 select, their finalisation to the
// statistics of a pair, the per-pixel gradient coefficient, a ray's share of dL/dMw, and the argument rules of
// the entries.  Host and device (DDRR_HD): tests/emu/wncc_emu.cpp compiles the same functions for the CPU.
// The ray and pose derivatives are siddon_core.h's and raygen_core.h's own functions, composed.
#pragma once

#include "../../include/diffdrr_wncc_hip.h"
#include "raygen_core.h"
#include "record_layout.h"
#include "siddon_core.h"

namespace ddrr_wncc {

constexpr int kGroupRays = DDRR_WNCC_GROUP_RAYS;
constexpr int kBlock = 256;
constexpr int kPer = kGroupRays / kBlock;  // pixels of a thread
constexpr int kMoments = 6;                // Sw, sum w x1, sum w x2, sum w x1^2, sum w x2^2, sum w x1 x2
constexpr int kStats = DDRR_WNCC_STATS;    // mu1, s1, mu2, s2, ncc, Sw
constexpr int kGrad = 12;                  // dL/dMw
static_assert(kMoments * sizeof(double) == DDRR_WNCC_SLOT_BYTES && kGrad * sizeof(float) == DDRR_WNCC_SLOT_BYTES,
              "a workspace slot holds the moments or the matrix gradient of one workgroup");

inline int groups_of(int N) { return (N + kGroupRays - 1) / kGroupRays; }

// One pixel into the moments.  A pixel with w == 0 is SELECTED out: its x1 and x2 (NaN, Inf: dead pixels) reach
// no sum.  w a, w a a, ... : w * a is exact in double (two 24-bit significands), the second factor goes in
// through the fma, so for w == 1 these are ncc_fwd_kernel's own operations (pose_ncc.hip).
DDRR_HD void moments_take(double m[kMoments], float w, float a, float c) {
    const bool on = w != 0.f;
    const double dw = on ? (double)w : 0.0, da = on ? (double)a : 0.0, dc = on ? (double)c : 0.0;
    const double wa = dw * da, wc = dw * dc;
    m[0] += dw;
    m[1] += wa;
    m[2] += wc;
    m[3] = fma(wa, da, m[3]);
    m[4] = fma(wc, dc, m[4]);
    m[5] = fma(wa, dc, m[5]);
}

// The statistics of a pair from its summed moments; Sw <= 0: nothing is left of the pair.
DDRR_HD void finalize(const double t[kMoments], float eps, float st[kStats]) {
    if (!(t[0] > 0.0)) {
        st[0] = 0.f, st[1] = sqrtf(eps), st[2] = 0.f, st[3] = sqrtf(eps), st[4] = 0.f, st[5] = 0.f;
        return;
    }
    const double inv = 1.0 / t[0];
    const double mu1 = t[1] * inv, mu2 = t[2] * inv;
    const double v1 = t[3] * inv - mu1 * mu1, v2 = t[4] * inv - mu2 * mu2;
    const double c12 = t[5] * inv - mu1 * mu2;
    const float s1 = sqrtf((float)v1 + eps), s2 = sqrtf((float)v2 + eps);
    st[0] = (float)mu1, st[1] = s1, st[2] = (float)mu2, st[3] = s2;
    st[4] = (float)c12 / (s1 * s2);
    st[5] = (float)t[0];
}

// g_out / Sw, the factor every pixel of a pair shares (0 for a pair with nothing left)
DDRR_HD float grad_scale(float g_out, float Sw) { return Sw > 0.f ? g_out / Sw : 0.f; }

// d (g_out ncc) / d xb[n] = gn w (za - zb ncc) / sb, exactly 0 at w == 0 whatever xa, xb hold there
// (xb = x2, xa = x1 for the moving image's gradient; the roles swapped for the fixed image's)
DDRR_HD float grad_pixel(float gn, float w, float xa, float mua, float sa, float xb, float mub, float sb, float ncc) {
    const float za = (xa - mua) / sa, zb = (xb - mub) / sb;
    return w != 0.f ? gn * w * (za - zb * ncc) / sb : 0.f;
}

// One ray of the fused step's backward into acc (12): the weighted d ncc / d x2, the record's endpoint gradients,
// the ray generation's adjoint -- siddon_ncc_bwd_pose_kernel's chain with the weight in g.
DDRR_HD void ray_backward(const float rec[8], const float s[3], const float *Mw, const float *Ainv, const float P[3],
                          float w, float x1, const float st[kStats], float gn, float eps, int with_img_path,
                          bool in, float acc[kGrad]) {
    const ddrr::RayGenOut ray = ddrr::raygen_ray(Mw, Ainv, P);
    const float L = ray.L;
    const float g = in ? grad_pixel(gn, w, x1, st[0], st[1], L * rec[0], st[2], st[3], st[4]) : 0.f;
    float gs[3], gt[3];
    ddrr::siddon_backward_ray<ddrr::REDUCE_SUM>(rec, s, ray.tv, eps, g * L, gs, gt);
    ddrr::raygen_ray_adjoint(Mw, Ainv, P, gt, gs, with_img_path ? g * rec[0] : 0.f, L, acc);
}

// ------------------------------------------------------------------------------------------- argument rules
// (host only; nullptr: fine, otherwise the message of the -1)
inline const char *check_sizes(int B, int N) {
    if (B < 0 || N < 1) return "bad batch / image size";
    if (B > DDRR_WNCC_MAX_POSES) return "at most 65535 pairs per call";
    return nullptr;
}
inline const char *check_rows(long x1_stride, long w_stride, int N) {
    if (x1_stride != 0 && x1_stride != N) return "x1_stride must be N, or 0 for a shared image";
    if (w_stride != 0 && w_stride != N) return "w_stride must be N, or 0 for a shared weight";
    return nullptr;
}
inline const char *check_eps(float eps) {
    return (eps >= 0.f && isfinite(eps)) ? nullptr : "eps must be >= 0 and finite";
}
inline const char *check_ws(const void *ws) {
    return (reinterpret_cast<uintptr_t>(ws) & 7) ? "ws must be 8-byte aligned" : nullptr;
}
inline const char *check_g_stride(int g_stride) {
    return (g_stride != 0 && g_stride != 1) ? "g_stride must be 1, or 0 for one value shared by the batch" : nullptr;
}
inline const char *check_axes(int a0, int a1, int a2) {
    return (a0 < 0 || a0 > 2 || a1 < 0 || a1 > 2 || a2 < 0 || a2 > 2 || a1 == a0 || a1 == a2)
               ? "invalid Euler convention" : nullptr;
}

}  // namespace ddrr_wncc
