/*
 * diffdrr_mvlm_hip.h -- C ABI of libdiffdrr_mvlm_hip.so: the three kernels of a multi-view (biplane)
 * Levenberg-Marquardt registration step (gfx950): the rays of S starts seen from V views, the normal-equations sums
 * of the S * V rendered poses from the brick kernel's backward record, and the accept / reject / solve step on the
 * sums added over the views of a start.
 *
 * A library of its own, next to libdiffdrr_lm_hip.so (include/diffdrr_lm_hip.h: one view; its five entries take
 * one reorient per launch and stay what they are) and libdiffdrr_wlm_hip.so (include/diffdrr_wlm_hip.h): they share
 * no symbol, no state and no version number.  Its kernels include the Levenberg-Marquardt library's csrc/lm_core.h
 * (and siddon_core.h, raygen_core.h, record_layout.h) and define none of that arithmetic again.
 *
 * Definitions.  S starts, V views, rendered pose b = s * V + v.  A start has ONE parameter vector
 *   theta_s = (rot[s], xyz[s]) in R^6,      M(theta) as ddrr_pose_euler_forward defines it (include/diffdrr_hip.h),
 * and view v has a fixed rigid offset K_v from the reference view: its world matrix is
 *   Mw_b = M(theta_s) K_v reorient = pose_euler_forward(rot[s], xyz[s], axes, Ro_v),   Ro_v = (K_v reorient)[:3],
 * with Ro_v = reorient_v[v] (V, 3, 4) floats formed by the caller (in float64, rounded once).  Pose b is therefore
 * the Euler pose of include/diffdrr_lm_hip.h with (rot[s], xyz[s], Ro_v): Mw, source_v, the record `aux`, P_n, x_n
 * and the Jacobian row j_n in R^6 of pixel n -- the derivative of x_n with respect to the SHARED theta_s -- are
 * those of that header, computed by the same functions.  The fixed image of pose b is row v of x1 (V, N): one image
 * per view, shared by the starts.  All views share the detector (Ainv, P).
 *
 * The objective of a start is sum_v 1/2 |z(x_v) - z(f_v)|^2 with every view normalised on its own (detectors have
 * their own gain): N sum_v (1 - ncc_v) up to ncc_eps.
 *
 * ddrr_mvlm_raygen writes, for the S * V poses, what ddrr_pose_raygen_forward writes for (rot[s], xyz[s], Ro_v):
 * Mw (S V, 3, 4), source_v (S V, 3), target_v (S V, N, 3), img (S V, N), and clears under the same contract:
 * `clear`: clear_floats floats (the record of ddrr_siddon_forward_bricks), clear_launch_ws: the first 16 bytes of
 * that call's launch workspace (its brick counter); either may be NULL, both 16-byte aligned.  The brick kernel can
 * then follow with DDRR_BRICKS_CLEARED.
 *
 * ddrr_mvlm_normal_sums writes the 44 sums of include/diffdrr_lm_hip.h of every pose as per-workgroup partials, in
 * the launch shape and order of ddrr_lm_normal_sums: workgroup g of pose b covers the rays [g * DDRR_MVLM_GROUP_RAYS,
 * (g + 1) * DDRR_MVLM_GROUP_RAYS) and writes the doubles ws[(b * G + g) * DDRR_MVLM_SUMS + k], G = ceil(N /
 * DDRR_MVLM_GROUP_RAYS); within a workgroup five interleaved slices of its rays, each in ascending order, then the
 * slices in ascending order, every product and sum in double.  The fixed image and Ro are selected by b % V, theta
 * by b / V.  A pose's partials and Jacobian rows are bit for bit those of ddrr_lm_normal_sums called with
 * reorient34 = Ro_v, the theta rows repeated and view v's image.  With jac != NULL it also writes j_n as
 * (S V, N, 6) floats.  No atomics, no zero-fill of `ws`.
 *
 * ddrr_mvlm_step, per start, everything in double:
 *   1. for v = 0 .. V - 1: the partials of pose (s, v) added in ascending g -> its 44 sums -> (ncc_v, A_v, g_v) by
 *      the formulas of ddrr_lm_step step 1;  A = sum_v A_v, g = sum_v g_v, added in ascending v and initialised
 *      with view 0's values (not with 0);  ncc = (sum_v ncc_v) / V, the sum taken the same way.
 *      ncc_views[s * V + v] = (float)ncc_v where ncc_views != NULL (of the render just judged, accepted or not).
 *   2-4. steps 2-4 of ddrr_lm_step on (ncc, A, g): accept or reject against the best pose so far, the damped
 *      Cholesky solve, theta_s <- best + delta rounded to float in place, ncc_out[s] = (float) best mean ncc;
 *      on the state of DDRR_MVLM_STATE_DOUBLES = 40 doubles per START with the offsets of include/diffdrr_lm_hip.h.
 * With V = 1 and K = I this is ddrr_lm_step bit for bit.
 *
 * Conventions
 *  - pointers are DEVICE pointers (HIP, gfx950), borrowed for the call only; `ws` and `state` are 8-byte aligned;
 *    the library keeps nothing on the device;
 *  - S >= 0, V >= 1, N >= 1, S * V <= 65535; S == 0 is a valid no-op (nothing launched, nothing written; asking
 *    ddrr_mvlm_raygen to clear with S == 0 is an argument error: nothing would be cleared);
 *  - a0, a1, a2 in {0: X, 1: Y, 2: Z} with a1 != a0 and a1 != a2 (as ddrr_pose_euler_forward);
 *  - `stream` is a hipStream_t (NULL = default stream); calls are asynchronous and never synchronise with the host;
 *  - return value: 0 on success, -1 for an argument error (checked before any launch), otherwise a hipError_t;
 *    ddrr_mvlm_last_error() describes the last failure (thread-local).
 * Not here: pixel weights (include/diffdrr_wlm_hip.h has them for one view), per-view detectors.
 */
#ifndef DIFFDRR_MVLM_HIP_H
#define DIFFDRR_MVLM_HIP_H

#define DDRR_MVLM_ABI_VERSION 1
#define DDRR_MVLM_SUMS 44
#define DDRR_MVLM_GROUP_RAYS 1024
#define DDRR_MVLM_STATE_DOUBLES 40
#define DDRR_MVLM_MAX_POSES 65535

#ifdef __cplusplus
extern "C" {
#endif

int ddrr_mvlm_abi_version(void);
const char *ddrr_mvlm_last_error(void);

/* bytes of the partial sums ddrr_mvlm_normal_sums writes for S starts, V views and N rays (0 for S < 1, V < 1,
 * N < 1 or S * V > DDRR_MVLM_MAX_POSES) */
long ddrr_mvlm_workspace_bytes(int S, int V, int N);

/* pose -> matrix -> rays of the S * V poses, and the clears of the render behind it. */
int ddrr_mvlm_raygen(const float *rot, const float *xyz, int a0, int a1, int a2, const float *reorient_v,
                     const float *Ainv, const float *P, int S, int V, int N, float *Mw, float *source_v,
                     float *target_v, float *img, float *clear, long clear_floats, void *clear_launch_ws,
                     void *stream);

/* the 44 sums of every pose as per-workgroup partials in `ws`; with jac != NULL also j_n as (S V, N, 6) floats. */
int ddrr_mvlm_normal_sums(const float *aux, const float *x1, const float *source_v, const float *Mw,
                          const float *Ainv, const float *P, const float *rot, const float *xyz, int a0, int a1,
                          int a2, const float *reorient_v, int S, int V, int N, float eps, int with_img_path,
                          void *ws, float *jac, void *stream);

/* add the views' normal equations of every start, accept or reject, solve, write the next trial parameters.
 * up > 1, 0 < down < 1, 0 < lambda_min <= lambda_max, ncc_eps >= 0, all finite.  ncc_views may be NULL. */
int ddrr_mvlm_step(const void *ws, void *state, float *rot, float *xyz, int S, int V, int N, double ncc_eps,
                   double up, double down, double lambda_min, double lambda_max, float *ncc_out,
                   float *ncc_views, void *stream);

#ifdef __cplusplus
}
#endif

#endif
