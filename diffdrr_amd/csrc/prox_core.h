// prox_core.h -- the per-voxel arithmetic of the TV proximal operator (include/diffdrr_prox_hip.h): D^T r and the
// projection onto the box, D x, the two projections of the dual, the momentum step and FISTA's extrapolation; and
// what the entry checks before any launch.  Host and device (DDRR_HD): csrc/prox.hip wraps the same functions in
// the tile march, tests/emu/prox_emu.cpp in plain loops over the voxels.  Every product that feeds a sum is an
// explicit fmaf and nothing else is contracted, so both builds round alike.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/diffdrr_prox_hip.h"
#include "ddrr_common.h"

namespace ddrr_prox {

constexpr long kMaxVoxels = 1L << 34;

// What a launch needs besides the pointers: everything a voxel's arithmetic reads.
struct Params {
    int Dx, Dy, Dz;
    float isx, isy, isz;     // 1 / spacing: D x
    float lsx, lsy, lsz;     // lambda / spacing: lambda D^T r
    float inv;               // 1 / (Lip lambda)
    float lower, upper;
};

inline double lipschitz(double sx, double sy, double sz) {
    return 4.0 * (1.0 / (sx * sx) + 1.0 / (sy * sy) + 1.0 / (sz * sz));
}

inline Params make_params(int Dx, int Dy, int Dz, float sx, float sy, float sz, float lambda, float lower,
                          float upper) {
    Params q;
    q.Dx = Dx, q.Dy = Dy, q.Dz = Dz;
    q.isx = (float)(1.0 / sx), q.isy = (float)(1.0 / sy), q.isz = (float)(1.0 / sz);
    q.lsx = (float)((double)lambda / sx), q.lsy = (float)((double)lambda / sy), q.lsz = (float)((double)lambda / sz);
    q.inv = lambda > 0.f ? (float)(1.0 / (lipschitz(sx, sy, sz) * (double)lambda)) : 0.f;
    q.lower = lower, q.upper = upper;
    return q;
}

// t_{k+1} of t_k, and the momentum (t_k - 1) / t_{k+1} of step k (t_0 = 1: step 0 has none)
inline double next_t(double t) { return 0.5 * (1.0 + sqrt(1.0 + 4.0 * t * t)); }

DDRR_HD float box(float v, float lower, float upper) {
    v = v < lower ? lower : v;  // (NaN stays NaN, as torch.clamp leaves it)
    return v > upper ? upper : v;
}

// x = P_C(b - lambda D^T r) from r at the voxel (r*) and at its three lower neighbours (r*_lo), each already
// zero where it does not contribute (index -1, the last plane of its axis)
DDRR_HD float primal(float b, float rx, float rx_lo, float ry, float ry_lo, float rz, float rz_lo, const Params &q) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float div = fmaf(rz_lo - rz, q.lsz, fmaf(ry_lo - ry, q.lsy, (rx_lo - rx) * q.lsx));
    return box(b - div, q.lower, q.upper);
}

// one component of D x; `ok`: the upper neighbour exists
DDRR_HD float difference(float x, float x_up, float is, bool ok) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return ok ? (x_up - x) * is : 0.f;
}

// p_new = Pi(r + d / (Lip lambda)), r_new = p_new + c (p_new - p_old): p and r in place
template <int MODE>
DDRR_HD void dual_step(const float d[3], float inv, float c, float p[3], float r[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    float v[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) v[a] = fmaf(d[a], inv, r[a]);
    if (MODE == DDRR_PROX_TV_ISOTROPIC) {
        const float n2 = fmaf(v[0], v[0], fmaf(v[1], v[1], v[2] * v[2]));
        const float s = n2 > 1.f ? 1.f / sqrtf(n2) : 1.f;
#pragma unroll
        for (int a = 0; a < 3; ++a) v[a] = v[a] * s;
    } else {
#pragma unroll
        for (int a = 0; a < 3; ++a) v[a] = box(v[a], -1.f, 1.f);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        r[a] = fmaf(c, v[a] - p[a], v[a]);
        p[a] = v[a];
    }
}

// FISTA's y = x + beta (x - x_prev)
DDRR_HD float extrapolate(float x, float x_prev, float beta) { return fmaf(beta, x - x_prev, x); }

// ------------------------------------------------------------------------------------------ the entry's checks
inline const char *dims_error(int Dx, int Dy, int Dz) {
    if (Dx < 0 || Dy < 0 || Dz < 0) return "Dx, Dy, Dz must be >= 0";
    if (Dx > DDRR_PROX_MAX_DIM || Dy > DDRR_PROX_MAX_DIM || Dz > DDRR_PROX_MAX_DIM)
        return "Dx, Dy, Dz must be <= 65535";
    if ((long)Dx * Dy * Dz > kMaxVoxels) return "Dx Dy Dz must be <= 2^34";
    return nullptr;
}

inline long workspace_bytes(int Dx, int Dy, int Dz, int iterations) {
    return iterations > 0 ? 3L * Dx * Dy * Dz * (long)sizeof(float) : 0;
}

inline bool overlap(const void *a, long a_bytes, const void *b, long b_bytes) {
    if (!a || !b || a_bytes <= 0 || b_bytes <= 0) return false;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}

inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// the message of the first rule of include/diffdrr_prox_hip.h the arguments break, or nullptr
inline const char *argument_error(const float *b, int Dx, int Dy, int Dz, float sx, float sy, float sz, int mode,
                                  float lambda, int iterations, float lower, float upper, const float *dual,
                                  const float *scratch, long scratch_bytes, const float *x_out, const float *x_prev,
                                  float beta, const float *y_out) {
    if (!b) return "null b pointer";
    if (!dual) return "null dual pointer";
    if (!x_out) return "null x_out pointer";
    if ((x_prev == nullptr) != (y_out == nullptr)) return "x_prev and y_out must both be given or both be null";
    if (const char *what = dims_error(Dx, Dy, Dz)) return what;
    if (!(sx > 0.f && sy > 0.f && sz > 0.f) || !isfinite(sx) || !isfinite(sy) || !isfinite(sz))
        return "sx, sy, sz must be > 0 and finite";
    if (mode != DDRR_PROX_TV_ISOTROPIC && mode != DDRR_PROX_TV_ANISOTROPIC)
        return "mode must be DDRR_PROX_TV_ISOTROPIC or DDRR_PROX_TV_ANISOTROPIC";
    if (!(lambda >= 0.f) || !isfinite(lambda)) return "lambda must be >= 0 and finite";
    if (iterations < 0) return "iterations must be >= 0";
    if (!(lower <= upper)) return "lower must be <= upper (and neither NaN)";
    if (x_prev && !isfinite(beta)) return "beta must be finite";
    if (!aligned4(b) || !aligned4(dual) || !aligned4(scratch) || !aligned4(x_out) || !aligned4(x_prev) ||
        !aligned4(y_out))
        return "b, dual, scratch, x_out, x_prev and y_out must be 4-byte aligned";
    const long n = (long)Dx * Dy * Dz * (long)sizeof(float);
    const bool iterate = iterations > 0 && lambda > 0.f;
    if (iterate && n > 0) {
        if (!scratch) return "null scratch pointer";
        if (scratch_bytes < workspace_bytes(Dx, Dy, Dz, iterations))
            return "scratch_bytes is smaller than ddrr_prox_workspace_bytes()";
    }
    const long s = iterate ? 3 * n : 0;
    if (overlap(x_out, n, b, n)) return "x_out must not overlap b";
    if (overlap(y_out, n, b, n)) return "y_out must not overlap b";
    if (overlap(dual, 3 * n, b, n)) return "dual must not overlap b";
    if (overlap(scratch, s, b, n)) return "scratch must not overlap b";
    if (overlap(x_out, n, x_prev, n) || overlap(x_out, n, dual, 3 * n) || overlap(x_out, n, scratch, s))
        return "x_out must not overlap x_prev, dual or scratch";
    if (overlap(y_out, n, x_out, n) || overlap(y_out, n, dual, 3 * n) || overlap(y_out, n, scratch, s))
        return "y_out must not overlap x_out, dual or scratch";
    if (overlap(scratch, s, dual, 3 * n)) return "scratch must not overlap dual";
    if (overlap(x_prev, n, dual, 3 * n) || overlap(x_prev, n, scratch, s))
        return "x_prev must not overlap dual or scratch";
    return nullptr;
}

}  // namespace ddrr_prox
