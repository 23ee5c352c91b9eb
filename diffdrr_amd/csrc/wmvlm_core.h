// wmvlm_core.h -- what the weighted multi-view Levenberg-Marquardt kernels (wmvlm.hip; include/diffdrr_wmvlm_hip.h
// has the definitions) add to lm_core.h and wlm_core.h: which start and which view a rendered pose belongs to, the
// sum of the non-empty views' weighted normal equations of a start with the Sw-weighted mean of their ncc, and the
// argument checks.  The ray's Jacobian row (ray_jacobian), the weighted sums (wslice_sum), the normal equations of a
// view (normal_equations with n = Sw), the judgement and the damped solve (judge_and_solve) and the state's offsets
// are lm_core.h's and wlm_core.h's own; the pose and the rays are raygen_core.h's.
// Host and device (DDRR_HD): tests/emu/wmvlm_emu.cpp compiles the same functions for the CPU.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/diffdrr_wmvlm_hip.h"
#include "mvlm_core.h"
#include "wlm_core.h"

static_assert(DDRR_WMVLM_MAX_POSES == DDRR_MVLM_MAX_POSES, "mvlm_core.h's check_shape holds for this library");

namespace ddrr_wmvlm {

using namespace ddrr_wlm;

static_assert(DDRR_WMVLM_SUMS == DDRR_WLM_SUMS && DDRR_WMVLM_GROUP_RAYS == DDRR_WLM_GROUP_RAYS &&
                  DDRR_WMVLM_STATE_DOUBLES == DDRR_WLM_STATE_DOUBLES && DDRR_WMVLM_MAX_POSES == DDRR_WLM_MAX_POSES,
              "a view's sums are the 45 of wlm_core.h on its launch shape; a start's state is a pose's");

// the normal equations of a start, added over its non-empty views: C = sum Sw_v ncc_v, A (21), g (6), Sw = sum Sw_v,
// the number of non-empty views so far, and the ncc of the first of them (the judged ncc where it stays the only one)
constexpr int kAccC = 0, kAccA = 1, kAccG = 22, kAccSw = 28, kAccViews = 29, kAccFirst = 30, kAcc = 31;

DDRR_HD void clear_views(double *acc) { acc[kAccViews] = 0.0; }

// View v of a start from its 45 sums.  Sw_v > 0: (ncc_v, A_v, g_v) by lm_core.h with n = Sw_v, added to `acc` in
// the order of the views (the first non-empty view initialises: 0 + a is a, but -0 would not survive it).
// Otherwise the view is empty and skipped.  -> ncc_v; sw_v = Sw_v, 0 for an empty view
DDRR_HD double add_wview(const double *S, double ncc_eps, double *acc, double &sw_v) {
    const double Sw = S[kSumW];
    if (!(Sw > 0.0)) {
        sw_v = 0.0;
        return 0.0;
    }
    double ncc, A[21], g[6];
    normal_equations(S, Sw, ncc_eps, ncc, A, g);
    const bool first = acc[kAccViews] == 0.0;
    const double c = Sw * ncc;
    acc[kAccC] = first ? c : acc[kAccC] + c;
    acc[kAccSw] = first ? Sw : acc[kAccSw] + Sw;
    if (first) acc[kAccFirst] = ncc;
#pragma unroll
    for (int i = 0; i < 21; ++i) acc[kAccA + i] = first ? A[i] : acc[kAccA + i] + A[i];
#pragma unroll
    for (int p = 0; p < 6; ++p) acc[kAccG + p] = first ? g[p] : acc[kAccG + p] + g[p];
    acc[kAccViews] += 1.0;
    sw_v = Sw;
    return ncc;
}

// the judged ncc, state[37] = Sw and steps 2-4 of ddrr_lm_step for one start, from the sum over its non-empty views
DDRR_HD void wstep_start(const double *acc, double up, double down, double lambda_min, double lambda_max, double *st,
                         float *rot, float *xyz, float *ncc_out) {
    const double views = acc[kAccViews];
    if (views == 0.0) {  // nothing left of the start: no division (wlm_core.h's empty pose)
        double A[21], g[6];
#pragma unroll
        for (int i = 0; i < 21; ++i) A[i] = 0.0;
#pragma unroll
        for (int p = 0; p < 6; ++p) g[p] = 0.0;
        st[kStSw] = 0.0;
        judge_and_solve(0.0, A, g, up, down, lambda_min, lambda_max, st, rot, xyz, ncc_out);
        return;
    }
    const double ncc = views == 1.0 ? acc[kAccFirst] : acc[kAccC] / acc[kAccSw];
    st[kStSw] = acc[kAccSw];
    judge_and_solve(ncc, acc + kAccA, acc + kAccG, up, down, lambda_min, lambda_max, st, rot, xyz, ncc_out);
}

inline int groups_of(int N) { return (N + kGroupRays - 1) / kGroupRays; }

// what both builds check before anything runs -> the message, or nullptr: mvlm_core.h's conditions with the strides
// of the weight and the detector points (in their place after the shape) and with sw_views in the step's alignment
using ddrr_mvlm::check_shape;

inline const char *check_strides(long w_stride, long P_stride, int N) {
    if (w_stride != 0 && w_stride != N) return "w_stride must be N, or 0 for a weight shared by the views";
    if (P_stride != 0 && P_stride != 3L * N) return "P_stride must be 3 N, or 0 for a detector shared by the views";
    return nullptr;
}

inline const char *check_raygen_args(const void *rot, const void *xyz, int a0, int a1, int a2, const void *reorient_v,
                                     const void *Ainv, const void *P, long P_stride, int S, int V, int N,
                                     const void *Mw, const void *source_v, const void *target_v, const void *img,
                                     const void *clear, long clear_floats, const void *clear_launch_ws) {
    return ddrr_mvlm::check_raygen_args(rot, xyz, a0, a1, a2, reorient_v, Ainv, P, S, V, N, Mw, source_v, target_v, img,
                                        clear, clear_floats, clear_launch_ws, check_strides(0, P_stride, N));
}

inline const char *check_sums_args(const void *aux, const void *x1, const void *w, long w_stride,
                                   const void *source_v, const void *Mw, const void *Ainv, const void *P,
                                   long P_stride, const void *rot, const void *xyz, int a0, int a1, int a2,
                                   const void *reorient_v, int S, int V, int N, const void *ws) {
    if (!w) return "null pointer";
    return ddrr_mvlm::check_sums_args(aux, x1, source_v, Mw, Ainv, P, rot, xyz, a0, a1, a2, reorient_v, S, V, N, ws,
                                      check_strides(w_stride, P_stride, N));
}

inline const char *check_step_args(const void *ws, const void *state, const void *rot, const void *xyz, int S, int V,
                                   int N, double ncc_eps, double up, double down, double lambda_min,
                                   double lambda_max, const void *ncc_out, const void *sw_views) {
    if (const char *bad = ddrr_mvlm::check_step_values(ws, state, rot, xyz, S, V, N, ncc_eps, up, down, lambda_min,
                                                       lambda_max, ncc_out))
        return bad;
    if ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(sw_views)) &
        7)
        return "ws, state and sw_views must be 8-byte aligned";
    return nullptr;
}

}  // namespace ddrr_wmvlm
