// lm_core.h -- the arithmetic of the Levenberg-Marquardt kernels (lm.hip; include/diffdrr_lm_hip.h has
// the definitions): a ray's pose Jacobian row from the brick kernel's backward record, the products it
// adds to the 44 sums of the normal equations, and the accept / reject / solve step on those sums.
// Host and device (DDRR_HD): tests/emu/lm_emu.cpp compiles the same functions for the CPU.  The argument checks of
// the single-view entries (lm.hip, wlm.hip) are here too, each condition once.
// The ray and pose derivatives are siddon_core.h's and raygen_core.h's own functions, composed.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/diffdrr_lm_hip.h"
#include "raygen_core.h"
#include "record_layout.h"
#include "siddon_core.h"

namespace ddrr_lm {

constexpr int kSums = DDRR_LM_SUMS;
constexpr int kGroupRays = DDRR_LM_GROUP_RAYS;
constexpr int kBlock = 256;
constexpr int kPer = kGroupRays / kBlock;  // rays of a thread
constexpr int kState = DDRR_LM_STATE_DOUBLES;
constexpr double kTiny = 1e-30;
// offsets into the sums and into a pose's state
constexpr int kSumA = 21, kSumC = 27, kSumD = 33, kSumM = 39;
constexpr int kStTheta = 0, kStNcc = 6, kStA = 7, kStG = 28, kStLambda = 34, kStValid = 35, kStAccepted = 36;

// index of (p, q), p <= q, in a row-major upper triangle of a 6 x 6 matrix
DDRR_HD constexpr int tri(int p, int q) { return p * 6 - p * (p - 1) / 2 + (q - p); }

constexpr int kPoseFloats = 39;  // a PoseEulerAdjoint: R (9), v (3), dR / dth_k (27)

// j_n (6) and x_n of one ray: the record's endpoint gradients for a unit image gradient, chained through
// the ray generation (a_n, 12 values) and through the pose (pose_euler_backward's second half on the
// pose's PoseEulerAdjoint `pose`, 39 floats): op for op what ddrr_siddon_backward_pose_euler computes for a
// grad_out that is 1 at this ray and 0 elsewhere.
DDRR_HD void ray_jacobian(const float rec[8], const float s[3], const float *Mw, const float *Ainv,
                          const float P[3], float eps, int with_img_path, const float *pose, const float *Ro,
                          float j[6], float &x) {
    const ddrr::RayGenOut ray = ddrr::raygen_ray(Mw, Ainv, P);
    float gs[3], gt[3], a[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) a[k] = 0.f;
    ddrr::siddon_backward_ray<ddrr::REDUCE_SUM>(rec, s, ray.tv, eps, ray.L, gs, gt);
    ddrr::raygen_ray_adjoint(Mw, Ainv, P, gt, gs, with_img_path ? rec[0] : 0.f, ray.L, a);
    ddrr::pose_euler_adjoint_apply(pose, pose + 9, pose + 12, Ro, a, j, j + 3);
    x = ray.L * rec[0];
}

// The 44 sums are the products of pairs of u_n = (j_n[0..5], x_n, f_n, 1) (all 45 but 1 * 1): sum k is
// sum_n u_n[p] u_n[q] with (p, q) = sum_pair(k), q == 8 standing for the constant 1.
DDRR_HD void sum_pair(int k, int &p, int &q) {
    if (k < kSumA) {  // H, upper triangle, row-major
        p = 0;
        for (int len = 6; k >= len; --len, ++p) k -= len;
        q = p + k;
    } else if (k < kSumC) {
        p = k - kSumA, q = 8;  // a = sum j
    } else if (k < kSumD) {
        p = 6, q = k - kSumC;  // c = sum x j
    } else if (k < kSumM) {
        p = 7, q = k - kSumD;  // d = sum f j
    } else {  // sum x, sum f, sum x^2, sum f^2, sum x f
        const int m = k - kSumM;
        p = (m == 1 || m == 3) ? 7 : 6;
        q = m < 2 ? 8 : (m == 2 ? 6 : 7);
    }
}

// Slice `slice` of sum k over the `count` rays of a workgroup whose (j, x, f) are staged in u (8 floats
// per ray): rays slice, slice + kSlices, ... in ascending order, in double (a product of two floats is
// exact there, so only the additions round).
constexpr int kSlices = 5;  // 5 x 44 = 220 of the 256 threads
DDRR_HD double slice_sum(const float *u, int count, int k, int slice) {
    int p, q;
    sum_pair(k, p, q);
    double v = 0.0;
    for (int n = slice; n < count; n += kSlices) {
        const double a = (double)u[8 * n + p], c = q < 8 ? (double)u[8 * n + q] : 1.0;
        v += a * c;
    }
    return v;
}

// What lm_kernels.h's normal-sums body is written on: how many sums a workgroup takes and one (sum, slice) of them
// from the staged rows (wlm_core.h has the weighted one, which reads the plane of weights `w` as well).
struct PlainSums {
    static constexpr bool kWeighted = false;
    static constexpr int kCount = kSums;
    DDRR_HD static double slice(const float *u, const float *, int count, int k, int sl) {
        return slice_sum(u, count, k, sl);
    }
};

// ncc, A (upper triangle) and g of the residual z(x) - z(f) from the 44 sums: step 1 of ddrr_lm_step, with n
// the number of rays (wlm_core.h: the sum of their weights, every sum weighted)
DDRR_HD void normal_equations(const double *S, double n, double ncc_eps, double &ncc, double A[21], double g[6]) {
    const double mx = S[kSumM] / n, mf = S[kSumM + 1] / n;
    const double vx = S[kSumM + 2] / n - mx * mx, vf = S[kSumM + 3] / n - mf * mf;
    const double sx = sqrt(vx + ncc_eps), sf = sqrt(vf + ncc_eps);
    ncc = (S[kSumM + 4] / n - mx * mf) / (sx * sf);
    const double rho = vx / (vx + ncc_eps);
    double u[6], w[6];
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        u[p] = (S[kSumC + p] - mx * S[kSumA + p]) / sx;
        w[p] = (S[kSumD + p] - mf * S[kSumA + p]) / sf;
        g[p] = ((1.0 - rho + ncc) * u[p] - w[p]) / sx;
    }
#pragma unroll
    for (int p = 0; p < 6; ++p)
#pragma unroll
        for (int q = p; q < 6; ++q)
            A[tri(p, q)] = (S[tri(p, q)] - S[kSumA + p] * S[kSumA + q] / n - (2.0 - rho) * u[p] * u[q] / n) /
                           (sx * sx);
}

DDRR_HD void normal_equations(const double *S, int N, double ncc_eps, double &ncc, double A[21], double g[6]) {
    normal_equations(S, (double)N, ncc_eps, ncc, A, g);
}

// (A + lambda diag(A) + tiny I) delta = -g by Cholesky; false (delta = 0) on a pivot that is not > 0
DDRR_HD bool solve_damped(const double A[21], const double g[6], double lambda, double delta[6]) {
    double Lm[6][6];
#pragma unroll
    for (int jn = 0; jn < 6; ++jn) {
        double d = A[tri(jn, jn)] + lambda * A[tri(jn, jn)] + kTiny;
#pragma unroll
        for (int k = 0; k < jn; ++k) d -= Lm[jn][k] * Lm[jn][k];
        if (!(d > 0.0)) {
#pragma unroll
            for (int p = 0; p < 6; ++p) delta[p] = 0.0;
            return false;
        }
        const double r = sqrt(d);
        Lm[jn][jn] = r;
#pragma unroll
        for (int i = jn + 1; i < 6; ++i) {
            double v = A[tri(jn, i)];
#pragma unroll
            for (int k = 0; k < jn; ++k) v -= Lm[i][k] * Lm[jn][k];
            Lm[i][jn] = v / r;
        }
    }
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double v = -g[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v -= Lm[i][k] * y[k];
        y[i] = v / Lm[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double v = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) v -= Lm[k][i] * delta[k];
        delta[i] = v / Lm[i][i];
    }
    return true;
}

// steps 2-4 of ddrr_lm_step for one pose, from the rendered pose's ncc, A and g
DDRR_HD void judge_and_solve(double ncc, const double A[21], const double g[6], double up, double down,
                             double lambda_min, double lambda_max, double *st, float *rot, float *xyz,
                             float *ncc_out) {
    double lambda = st[kStLambda];
    if (st[kStValid] == 0.0 || ncc > st[kStNcc]) {
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            st[kStTheta + p] = (double)rot[p];
            st[kStTheta + 3 + p] = (double)xyz[p];
        }
        st[kStNcc] = ncc;
#pragma unroll
        for (int i = 0; i < 21; ++i) st[kStA + i] = A[i];
#pragma unroll
        for (int p = 0; p < 6; ++p) st[kStG + p] = g[p];
        st[kStValid] = 1.0;
        st[kStAccepted] = 1.0;
        lambda = fmax(lambda * down, lambda_min);
    } else {
        st[kStAccepted] = 0.0;
        lambda = fmin(lambda * up, lambda_max);
    }
    double delta[6];
    if (!solve_damped(st + kStA, st + kStG, lambda, delta)) lambda = fmin(lambda * up, lambda_max);
    st[kStLambda] = lambda;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        rot[p] = (float)(st[kStTheta + p] + delta[p]);
        xyz[p] = (float)(st[kStTheta + 3 + p] + delta[3 + p]);
    }
    *ncc_out = (float)st[kStNcc];
}

// steps 1-4 of ddrr_lm_step for one pose, from its summed S
DDRR_HD void step_pose(const double *S, int N, double ncc_eps, double up, double down, double lambda_min,
                       double lambda_max, double *st, float *rot, float *xyz, float *ncc_out) {
    double ncc, A[21], g[6];
    normal_equations(S, N, ncc_eps, ncc, A, g);
    judge_and_solve(ncc, A, g, up, down, lambda_min, lambda_max, st, rot, xyz, ncc_out);
}

// What both builds check before anything runs -> the message, or nullptr.  `own` is the message of a condition of
// the caller's own (wlm_core.h's weight stride): it is reported where that condition stands in the caller's order.
inline const char *check_axes(int a0, int a1, int a2) {
    if (a0 < 0 || a0 > 2 || a1 < 0 || a1 > 2 || a2 < 0 || a2 > 2 || a1 == a0 || a1 == a2)
        return "invalid Euler convention";
    return nullptr;
}

inline const char *check_hyper(double ncc_eps, double up, double down, double lambda_min, double lambda_max) {
    if (!(ncc_eps >= 0.0 && isfinite(ncc_eps))) return "ncc_eps must be >= 0 and finite";
    if (!(up > 1.0 && isfinite(up) && down > 0.0 && down < 1.0)) return "up must be > 1 and finite, down in (0, 1)";
    if (!(lambda_min > 0.0 && lambda_min <= lambda_max && isfinite(lambda_max)))
        return "0 < lambda_min <= lambda_max, finite, expected";
    return nullptr;
}

inline const char *check_sums_args(const void *aux, const void *x1, long x1_stride, const void *source_v,
                                   const void *Mw, const void *Ainv, const void *P, const void *rot, const void *xyz,
                                   int a0, int a1, int a2, const void *reorient34, int B, int N, const void *ws,
                                   const char *own = nullptr) {
    if (!aux || !x1 || !source_v || !Mw || !Ainv || !P || !rot || !xyz || !reorient34 || !ws) return "null pointer";
    if (const char *bad = check_axes(a0, a1, a2)) return bad;
    if (B < 0 || N < 1) return "bad batch / image size";
    if (x1_stride != 0 && x1_stride != N) return "x1_stride must be N, or 0 for a shared image";
    if (own) return own;
    if (reinterpret_cast<uintptr_t>(ws) & 7) return "ws must be 8-byte aligned";
    if (B > DDRR_LM_MAX_POSES) return "at most 65535 poses per call";
    return nullptr;
}

inline const char *check_step_args(const void *ws, const void *state, const void *rot, const void *xyz, int B, int N,
                                   double ncc_eps, double up, double down, double lambda_min, double lambda_max,
                                   const void *ncc_out) {
    if (!ws || !state || !rot || !xyz || !ncc_out) return "null pointer";
    if (B < 0 || N < 1) return "bad batch / image size";
    if (const char *bad = check_hyper(ncc_eps, up, down, lambda_min, lambda_max)) return bad;
    if ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(state)) & 7)
        return "ws and state must be 8-byte aligned";
    if (B > DDRR_LM_MAX_POSES) return "at most 65535 poses per call";
    return nullptr;
}

}  // namespace ddrr_lm
