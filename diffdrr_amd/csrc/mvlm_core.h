// mvlm_core.h -- what the multi-view Levenberg-Marquardt kernels (mvlm.hip; include/diffdrr_mvlm_hip.h has the
// definitions) add to lm_core.h: which start and which view a rendered pose belongs to, the sum of the views'
// normal equations of a start, and the argument checks.  The ray's Jacobian row (ray_jacobian), the sums
// (slice_sum), the normal equations of a view (normal_equations), the judgement and the damped solve
// (judge_and_solve) and the state's offsets are lm_core.h's own; the pose and the rays are raygen_core.h's.
// Host and device (DDRR_HD): tests/emu/mvlm_emu.cpp compiles the same functions for the CPU.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/diffdrr_mvlm_hip.h"
#include "lm_core.h"

namespace ddrr_mvlm {

using namespace ddrr_lm;

static_assert(DDRR_MVLM_SUMS == DDRR_LM_SUMS && DDRR_MVLM_GROUP_RAYS == DDRR_LM_GROUP_RAYS &&
                  DDRR_MVLM_STATE_DOUBLES == DDRR_LM_STATE_DOUBLES && DDRR_MVLM_MAX_POSES == DDRR_LM_MAX_POSES,
              "a view's sums are the 44 of lm_core.h on its launch shape; a start's state is a pose's");

// the normal equations of a start, added over its views: ncc (the sum, not yet the mean), A (21), g (6)
constexpr int kAccNcc = 0, kAccA = 1, kAccG = 22, kAcc = 28;

// View v of a start from its 44 sums: (ncc_v, A_v, g_v) by lm_core.h, added to `acc` in the order of the views
// (view 0 initialises: 0 + a is a, but -0 would not survive it).  -> ncc_v
DDRR_HD double add_view(const double *S, int N, double ncc_eps, int v, double *acc) {
    double ncc, A[21], g[6];
    normal_equations(S, N, ncc_eps, ncc, A, g);
    acc[kAccNcc] = v == 0 ? ncc : acc[kAccNcc] + ncc;
#pragma unroll
    for (int i = 0; i < 21; ++i) acc[kAccA + i] = v == 0 ? A[i] : acc[kAccA + i] + A[i];
#pragma unroll
    for (int p = 0; p < 6; ++p) acc[kAccG + p] = v == 0 ? g[p] : acc[kAccG + p] + g[p];
    return ncc;
}

// steps 2-4 of ddrr_mvlm_step for one start, from the sum over its V views
DDRR_HD void step_start(const double *acc, int V, double up, double down, double lambda_min, double lambda_max,
                        double *st, float *rot, float *xyz, float *ncc_out) {
    judge_and_solve(acc[kAccNcc] / (double)V, acc + kAccA, acc + kAccG, up, down, lambda_min, lambda_max, st, rot,
                    xyz, ncc_out);
}

inline int groups_of(int N) { return (N + kGroupRays - 1) / kGroupRays; }

// What both builds check before anything runs -> the message, or nullptr.  `own` is the message of a condition of
// the caller's own (wmvlm_core.h's strides): it is reported where that condition stands in the caller's order.
inline const char *check_shape(int S, int V, int N) {
    if (S < 0 || V < 1 || N < 1) return "bad batch / view count / image size (S >= 0, V >= 1, N >= 1)";
    if ((long)S * V > DDRR_MVLM_MAX_POSES) return "at most 65535 poses (S * V) per call";
    return nullptr;
}

inline const char *check_raygen_args(const void *rot, const void *xyz, int a0, int a1, int a2, const void *reorient_v,
                                     const void *Ainv, const void *P, int S, int V, int N, const void *Mw,
                                     const void *source_v, const void *target_v, const void *img, const void *clear,
                                     long clear_floats, const void *clear_launch_ws, const char *own = nullptr) {
    if (!rot || !xyz || !reorient_v || !Ainv || !P || !Mw || !source_v || !target_v || !img) return "null pointer";
    if (const char *bad = check_axes(a0, a1, a2)) return bad;
    if (const char *bad = check_shape(S, V, N)) return bad;
    if (own) return own;
    if (clear_floats < 0 || (clear_floats > 0 && !clear)) return "clear_floats without a buffer";
    if ((reinterpret_cast<uintptr_t>(clear) & 15) || (reinterpret_cast<uintptr_t>(clear_launch_ws) & 15))
        return "the buffers to clear must be 16-byte aligned";
    if ((clear_floats > 0 || clear_launch_ws) && S == 0)
        return "nothing is launched for an empty batch: clear the buffers yourself";
    return nullptr;
}

inline const char *check_sums_args(const void *aux, const void *x1, const void *source_v, const void *Mw,
                                   const void *Ainv, const void *P, const void *rot, const void *xyz, int a0, int a1,
                                   int a2, const void *reorient_v, int S, int V, int N, const void *ws,
                                   const char *own = nullptr) {
    if (!aux || !x1 || !source_v || !Mw || !Ainv || !P || !rot || !xyz || !reorient_v || !ws) return "null pointer";
    if (const char *bad = check_axes(a0, a1, a2)) return bad;
    if (const char *bad = check_shape(S, V, N)) return bad;
    if (own) return own;
    if (reinterpret_cast<uintptr_t>(ws) & 7) return "ws must be 8-byte aligned";
    return nullptr;
}

// (the step's conditions but the alignment, whose message names the pointers of the entry)
inline const char *check_step_values(const void *ws, const void *state, const void *rot, const void *xyz, int S,
                                     int V, int N, double ncc_eps, double up, double down, double lambda_min,
                                     double lambda_max, const void *ncc_out) {
    if (!ws || !state || !rot || !xyz || !ncc_out) return "null pointer";
    if (const char *bad = check_shape(S, V, N)) return bad;
    return check_hyper(ncc_eps, up, down, lambda_min, lambda_max);
}

inline const char *check_step_args(const void *ws, const void *state, const void *rot, const void *xyz, int S, int V,
                                   int N, double ncc_eps, double up, double down, double lambda_min,
                                   double lambda_max, const void *ncc_out) {
    if (const char *bad = check_step_values(ws, state, rot, xyz, S, V, N, ncc_eps, up, down, lambda_min, lambda_max,
                                            ncc_out))
        return bad;
    if ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(state)) & 7)
        return "ws and state must be 8-byte aligned";
    return nullptr;
}

}  // namespace ddrr_mvlm
