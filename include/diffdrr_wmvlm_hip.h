/*
 * diffdrr_wmvlm_hip.h -- C ABI of libdiffdrr_wmvlm_hip.so: the three kernels of a multi-view (biplane)
 * Levenberg-Marquardt registration step with a pixel weight and a detector per view (gfx950): the rays of S starts
 * seen from V views, the weighted normal-equations sums of the S * V rendered poses from the brick kernel's backward
 * record, and the accept / reject / solve step on the sums added over the views of a start.
 *
 * A library of its own, next to libdiffdrr_lm_hip.so (include/diffdrr_lm_hip.h: one view, no weight),
 * libdiffdrr_wlm_hip.so (include/diffdrr_wlm_hip.h: one view, a weight) and libdiffdrr_mvlm_hip.so
 * (include/diffdrr_mvlm_hip.h: V views, no weight, one detector), which stay what they are: the four share no symbol,
 * no state and no version number.  Its kernels include csrc/lm_core.h and csrc/wlm_core.h (and through them
 * siddon_core.h, raygen_core.h, record_layout.h) and define none of that arithmetic again.
 *
 * Definitions.  S starts, V views, rendered pose b = s * V + v.  A start has ONE parameter vector
 *   theta_s = (rot[s], xyz[s]) in R^6,      M(theta) as ddrr_pose_euler_forward defines it (include/diffdrr_hip.h).
 * View v has
 *   - a fixed rigid offset K_v from the reference view and a detector orientation reorient_v: its world matrix is
 *       Mw_b = pose_euler_forward(rot[s], xyz[s], axes, Ro_v),   Ro_v = (K_v reorient_v)[:3] = reorient_v[v],
 *     (V, 3, 4) floats formed by the caller in float64 and rounded once;
 *   - a fixed image: row v of x1 (V, N), shared by the starts;
 *   - a weight: w_vn = w[v * w_stride + n], w_stride = N, or 0 for one weight image shared by all views;
 *     w >= 0 and finite (the caller's to ensure: the kernels do not look);
 *   - calibrated detector points P_v = P + v * P_stride, (N, 3) floats each, P_stride = 3 N, or 0 for one detector
 *     shared by all views.
 * All views have the same N = H x W rays.  Pose b is the Euler pose of include/diffdrr_wlm_hip.h with (rot[s],
 * xyz[s], Ro_v, P_v): Mw, source_v, the record `aux`, x_n, and the Jacobian row j_n in R^6 of pixel n -- the
 * derivative of x_n with respect to the SHARED theta_s -- are those of that header, computed by the same functions.
 * The brick kernel (ddrr_siddon_forward_bricks) is unchanged: it takes per-pose rays, and the targets of each pose
 * are still an affine grid.
 *
 * The objective of a start is
 *   sum_v 1/2 sum_n w_vn (z_w(x_v)_n - z_w(f_v)_n)^2  =  sum_v Sw_v (1 - ncc_v)   up to ncc_eps,
 * every view the weighted problem of include/diffdrr_wlm_hip.h on its own (weighted mean, weighted biased variance,
 * Sw_v = sum_n w_vn), and the residual of a start the stack of its views' weighted residuals.  Consequently
 *   - a pixel of weight 1 counts the same in whichever view it lies;
 *   - scaling ONE view's weight by c makes that view count c times (a per-view confidence); scaling ALL views'
 *     weights by c scales A, g and the objective by c and changes neither the judged ncc nor the step.
 *
 * ddrr_wmvlm_raygen is ddrr_mvlm_raygen with (P, P_stride): for pose (s, v) it writes what
 * ddrr_pose_raygen_forward(rot[s], xyz[s], Ro_v, Ainv, P_v) writes, bit for bit -- Mw (S V, 3, 4), source_v (S V, 3),
 * target_v (S V, N, 3), img (S V, N) -- and with P_stride == 0 what ddrr_mvlm_raygen writes.  It clears under the
 * same contract: `clear`: clear_floats floats (the record of ddrr_siddon_forward_bricks), clear_launch_ws: the first
 * 16 bytes of that call's launch workspace (its brick counter); either may be NULL, both 16-byte aligned.  The brick
 * kernel can then follow with DDRR_BRICKS_CLEARED.
 *
 * ddrr_wmvlm_normal_sums writes the 45 weighted sums of include/diffdrr_wlm_hip.h of every pose as per-workgroup
 * partials, in the launch shape, slice order and rounding of ddrr_wlm_normal_sums: workgroup g of pose b covers the
 * rays [g * DDRR_WMVLM_GROUP_RAYS, (g + 1) * DDRR_WMVLM_GROUP_RAYS) and writes the doubles
 * ws[(b * G + g) * DDRR_WMVLM_SUMS + k], G = ceil(N / DDRR_WMVLM_GROUP_RAYS); the product of two floats exact in
 * double, the multiplication by w rounding once, nothing contracted; a ray of weight 0 is selected out (staged as a
 * row of zeros): x1 may hold NaN or Inf there.  The fixed image, the weight, Ro and P are selected by b % V, theta by
 * b / V.  A pose's partials and Jacobian rows are bit for bit those of ddrr_wlm_normal_sums called with
 * reorient34 = Ro_v, P_v, the theta rows repeated and view v's image and weight.  With jac != NULL it also writes j_n
 * as (S V, N, 6) floats for EVERY ray, whatever its weight.  No atomics, no zero-fill of `ws`.
 *
 * ddrr_wmvlm_step, per start, everything in double:
 *   1. for v = 0 .. V - 1: the partials of pose (s, v) added in ascending g -> its 45 sums S_v, Sw_v = S_v[44].
 *      Sw_v > 0: (ncc_v, A_v, g_v) by the formulas of ddrr_wlm_step step 1 (n = Sw_v).  Otherwise the view is EMPTY
 *      and skipped: ncc_v = 0, and it adds nothing.
 *      Over the non-empty views in ascending v, the first of them initialising (not added to 0):
 *        A = sum A_v,   g = sum g_v,   Sw = sum Sw_v,   C = sum Sw_v * ncc_v.
 *      The judged ncc: exactly one non-empty view -> that view's ncc_v itself (the weighted mean of one number is
 *      that number: V = 1 is ddrr_wlm_step bit for bit); more than one -> C / Sw, the Sw-weighted mean, so that
 *      accept / reject judges the objective the step minimises; none -> ncc = 0, A = 0, g = 0, Sw = 0: such a start
 *      never moves and reports 0, as an empty pose of ddrr_wlm_step does.
 *   2. state[37] = Sw; then steps 2-4 of ddrr_lm_step on (ncc, A, g): accept or reject against the best so far, the
 *      damped Cholesky solve, theta_s <- best + delta rounded to float in place, ncc_out[s] = (float) best ncc; on
 *      the state of DDRR_WMVLM_STATE_DOUBLES = 40 doubles per START with the offsets of include/diffdrr_lm_hip.h.
 *   3. ncc_views[s * V + v] = (float)ncc_v and sw_views[s * V + v] = Sw_v (a double; 0 for an empty view), both of
 *      the render just judged, accepted or not; either may be NULL.
 *
 * Conventions
 *  - pointers are DEVICE pointers (HIP, gfx950), borrowed for the call only; `ws`, `state` and `sw_views` are 8-byte
 *    aligned; the library keeps nothing on the device;
 *  - S >= 0, V >= 1, N >= 1, S * V <= 65535; S == 0 is a valid no-op (nothing launched, nothing written; asking
 *    ddrr_wmvlm_raygen to clear with S == 0 is an argument error: nothing would be cleared);
 *  - w_stride is 0 or N; P_stride is 0 or 3 N;
 *  - a0, a1, a2 in {0: X, 1: Y, 2: Z} with a1 != a0 and a1 != a2 (as ddrr_pose_euler_forward);
 *  - `stream` is a hipStream_t (NULL = default stream); calls are asynchronous and never synchronise with the host;
 *  - return value: 0 on success, -1 for an argument error (checked before any launch), otherwise a hipError_t;
 *    ddrr_wmvlm_last_error() describes the last failure (thread-local).
 * Not here: a weight per start (w has no start index), the step as a captured graph, a fused multi-view NCC of the
 * first-order loop.
 */
#ifndef DIFFDRR_WMVLM_HIP_H
#define DIFFDRR_WMVLM_HIP_H

#define DDRR_WMVLM_ABI_VERSION 1
#define DDRR_WMVLM_SUMS 45
#define DDRR_WMVLM_GROUP_RAYS 1024
#define DDRR_WMVLM_STATE_DOUBLES 40
#define DDRR_WMVLM_MAX_POSES 65535

#ifdef __cplusplus
extern "C" {
#endif

int ddrr_wmvlm_abi_version(void);
const char *ddrr_wmvlm_last_error(void);

/* bytes of the partial sums ddrr_wmvlm_normal_sums writes for S starts, V views and N rays (0 for S < 1, V < 1,
 * N < 1 or S * V > DDRR_WMVLM_MAX_POSES) */
long ddrr_wmvlm_workspace_bytes(int S, int V, int N);

/* pose -> matrix -> rays of the S * V poses, view v on the detector points P + v * P_stride, and the clears of the
 * render behind it. */
int ddrr_wmvlm_raygen(const float *rot, const float *xyz, int a0, int a1, int a2, const float *reorient_v,
                      const float *Ainv, const float *P, long P_stride, int S, int V, int N, float *Mw,
                      float *source_v, float *target_v, float *img, float *clear, long clear_floats,
                      void *clear_launch_ws, void *stream);

/* the 45 weighted sums of every pose as per-workgroup partials in `ws`; with jac != NULL also j_n as (S V, N, 6)
 * floats. */
int ddrr_wmvlm_normal_sums(const float *aux, const float *x1, const float *w, long w_stride, const float *source_v,
                           const float *Mw, const float *Ainv, const float *P, long P_stride, const float *rot,
                           const float *xyz, int a0, int a1, int a2, const float *reorient_v, int S, int V, int N,
                           float eps, int with_img_path, void *ws, float *jac, void *stream);

/* add the non-empty views' normal equations of every start, accept or reject, solve, write the next trial
 * parameters.  up > 1, 0 < down < 1, 0 < lambda_min <= lambda_max, ncc_eps >= 0, all finite.  ncc_views (S V floats)
 * and sw_views (S V doubles) may each be NULL. */
int ddrr_wmvlm_step(const void *ws, void *state, float *rot, float *xyz, int S, int V, int N, double ncc_eps,
                    double up, double down, double lambda_min, double lambda_max, float *ncc_out,
                    float *ncc_views, double *sw_views, void *stream);

#ifdef __cplusplus
}
#endif

#endif
