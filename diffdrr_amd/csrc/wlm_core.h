// wlm_core.h -- the arithmetic the weighted Levenberg-Marquardt kernels (wlm.hip; include/diffdrr_wlm_hip.h
// has the definitions) add to lm_core.h: a slice of one of the 45 weighted sums from the staged rows, and the
// step on those sums with n = Sw.  The ray's Jacobian row (ray_jacobian), the pairs of the sums (sum_pair, tri),
// the normal equations, the damped solve (solve_damped) and the state's offsets are lm_core.h's own.
// Host and device (DDRR_HD): tests/emu/wlm_emu.cpp compiles the same functions for the CPU.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/diffdrr_wlm_hip.h"
#include "lm_core.h"

namespace ddrr_wlm {

using namespace ddrr_lm;

static_assert(DDRR_WLM_SUMS == DDRR_LM_SUMS + 1 && DDRR_WLM_GROUP_RAYS == DDRR_LM_GROUP_RAYS &&
                  DDRR_WLM_STATE_DOUBLES == DDRR_LM_STATE_DOUBLES && DDRR_WLM_MAX_POSES == DDRR_LM_MAX_POSES,
              "the weighted sums are the 44 of lm_core.h and sum w, on its launch shape, state and pose cap");

constexpr int kWSums = DDRR_WLM_SUMS;
constexpr int kSumW = DDRR_LM_SUMS;  // [44] = sum w
constexpr int kStSw = 37;            // the state's slot for Sw of the render just judged

// Slice `slice` of weighted sum k over the `count` rays of a workgroup whose (j, x, f) are staged in u (8 floats
// per ray) and whose weights in w: rays slice, slice + kSlices, ... in ascending order.  The product of the two
// floats is exact in double, the multiplication by the weight rounds once, the addition once: nothing is fused
// (a contracted w * (a c) + v would not round the product, and the host could not restate the sum).
// A ray of weight 0 is staged as a row of zeros: it adds +0.  `one` points to a float 1 next to the staged rows:
// the constant of u_n is read from it at stride 0, so that the loop has no branch and its three reads are
// independent of one another.
DDRR_HD double wslice_sum(const float *u, const float *w, const float *one, int count, int k, int slice) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    int p = 8, q = 8;
    if (k < kSumW) sum_pair(k, p, q);
    const float *pa = p < 8 ? u + p : one, *pc = q < 8 ? u + q : one;
    const int sa = p < 8 ? 8 : 0, sc = q < 8 ? 8 : 0;
    double v = 0.0;
#pragma unroll 4
    for (int n = slice; n < count; n += kSlices) {
        const double pr = (double)pa[sa * n] * (double)pc[sc * n];
        const double t = (double)w[n] * pr;
        v = v + t;
    }
    return v;
}

// steps 1-4 of ddrr_wlm_step for one pose, from its summed S (45)
DDRR_HD void wstep_pose(const double *S, double ncc_eps, double up, double down, double lambda_min,
                        double lambda_max, double *st, float *rot, float *xyz, float *ncc_out) {
    const double Sw = S[kSumW];
    double ncc = 0.0, A[21], g[6];
    if (Sw > 0.0) {
        normal_equations(S, Sw, ncc_eps, ncc, A, g);
    } else {  // nothing left of the pose: no division
#pragma unroll
        for (int i = 0; i < 21; ++i) A[i] = 0.0;
#pragma unroll
        for (int p = 0; p < 6; ++p) g[p] = 0.0;
    }
    st[kStSw] = Sw > 0.0 ? Sw : 0.0;
    judge_and_solve(ncc, A, g, up, down, lambda_min, lambda_max, st, rot, xyz, ncc_out);
}

// lm_core.h's PlainSums for the 45 weighted sums: `w` is the plane of weights with the constant 1 behind it
struct WeightedSums {
    static constexpr bool kWeighted = true;
    static constexpr int kCount = kWSums;
    DDRR_HD static double slice(const float *u, const float *w, int count, int k, int sl) {
        return wslice_sum(u, w, w + kGroupRays, count, k, sl);
    }
};

// what both builds check before anything runs -> the message, or nullptr: lm_core.h's conditions with the weight's
// (the step's are lm_core.h's check_step_args as they stand)
inline const char *check_sums_args(const void *aux, const void *x1, long x1_stride, const void *w, long w_stride,
                                   const void *source_v, const void *Mw, const void *Ainv, const void *P,
                                   const void *rot, const void *xyz, int a0, int a1, int a2, const void *reorient34,
                                   int B, int N, const void *ws) {
    if (!w) return "null pointer";
    return ddrr_lm::check_sums_args(
        aux, x1, x1_stride, source_v, Mw, Ainv, P, rot, xyz, a0, a1, a2, reorient34, B, N, ws,
        w_stride != 0 && w_stride != N ? "w_stride must be N, or 0 for a shared weight" : nullptr);
}

}  // namespace ddrr_wlm
