/*
 * diffdrr_wlm_hip.h -- C ABI of libdiffdrr_wlm_hip.so: the two kernels of a Levenberg-Marquardt registration
 * step with a per-pixel weight (gfx950): the weighted normal-equations sums of a rendered pose from the brick
 * kernel's backward record, and the accept / reject / solve step on them.
 *
 * A library of its own, next to libdiffdrr_lm_hip.so (include/diffdrr_lm_hip.h, whose five entries, 44 sums and
 * launches stay what they are) and libdiffdrr_wncc_hip.so (include/diffdrr_wncc_hip.h, the weighted NCC of the
 * first-order loop): they share no symbol, no state and no version number.  Its kernels include the
 * Levenberg-Marquardt library's csrc/lm_core.h (and through it siddon_core.h, raygen_core.h, record_layout.h) and
 * define none of that arithmetic again.
 *
 * Definitions, per pose b.  theta, Mw, source_v, the blocked float record `aux`, P_n, x_n, f_n and the Jacobian
 * row j_n in R^6 of pixel n are those of include/diffdrr_lm_hip.h, computed by the same functions.  The weight of
 * pixel n is
 *   w_n = w[b * w_stride + n]       (w_stride: 0 = one weight image for all poses, or N),  w_n >= 0 and finite.
 * Negative or non-finite weights are the caller's to exclude: the kernels do not look for them.
 *
 * The weighted problem.  With V = {n : w_n != 0}, Sw = sum_V w_n,
 *   mu_x = sum_V w x / Sw,   v_x = sum_V w x^2 / Sw - mu_x^2,   s_x = sqrt(v_x + ncc_eps),   z_w(x) = (x - mu_x) / s_x
 * (the weighted mean and the weighted biased variance, as include/diffdrr_wncc_hip.h), likewise f, the residual is
 *   r_n = sqrt(w_n) (z_w(x)_n - z_w(f)_n),       ncc_w = sum_V w z_w(x) z_w(f) / Sw,
 * and its objective 1/2 |r|^2 is Sw (1 - ncc_w) up to ncc_eps.  A = J_r^T J_r and g = J_r^T r of this residual are
 * the formulas of include/diffdrr_lm_hip.h step 1 with every sum carrying w_n and with N replaced by Sw: sqrt(w)
 * enters every product of two residual rows as w, and the derivative of the weighted mean and variance is the
 * unweighted one with 1 / N -> w_n / Sw.
 *
 * The 45 sums of a pose, in this order (DDRR_WLM_SUMS doubles):
 *   [0, 44)   the 44 sums of include/diffdrr_lm_hip.h in its order, every product multiplied by w_n:
 *             H = sum w j j^T (upper triangle, row-major), a = sum w j, c = sum w x j, d = sum w f j,
 *             sum w x, sum w f, sum w x^2, sum w f^2, sum w x f
 *   [44]      Sw = sum w
 * With u_n = (j_n, x_n, f_n, 1), sum k is sum_n (double)w_n * ((double)u_n[p] * (double)u_n[q]), (p, q) the pair
 * of sum k ((8, 8) for k = 44).  The inner product of two floats is exact in double; the multiplication by w_n
 * rounds once (to double), then the sum is taken in double: three operations, none of them fused.
 *
 * Zero weights.  A ray with w_n == 0 is selected out of every sum, not multiplied by zero: x1 may hold NaN or Inf
 * there.  (The kernels stage the row (0, ..., 0) with weight 0 for it, which adds +0 to every sum: the same bits.)
 *
 * ddrr_wlm_normal_sums writes the sums as per-workgroup partials, in the launch shape and order of
 * ddrr_lm_normal_sums: workgroup g of pose b covers the rays [g * DDRR_WLM_GROUP_RAYS, (g + 1) *
 * DDRR_WLM_GROUP_RAYS) and writes the doubles ws[(b * G + g) * DDRR_WLM_SUMS + k], G = ceil(N /
 * DDRR_WLM_GROUP_RAYS); within a workgroup five interleaved slices of its rays (ray i of the workgroup in slice
 * i mod 5), each in ascending order, then the slices in ascending order.  ddrr_wlm_step adds the partials of a pose
 * in ascending g.  No atomics, no zero-fill of `ws` (every call writes all it later reads): the results are bitwise
 * reproducible.
 * With jac != NULL it also writes j_n as (B, N, 6) floats for EVERY ray, whatever its weight: weights do not enter
 * j_n.
 *
 * ddrr_wlm_step, per pose, everything in double: steps 1-4 of ddrr_lm_step (include/diffdrr_lm_hip.h) with n = Sw
 * in place of N, on the same state of DDRR_WLM_STATE_DOUBLES = 40 doubles with the same offsets (best theta, its
 * ncc, A, g, lambda, valid, accepted), so that a state is read the same way whichever library stepped it.  Two
 * differences:
 *   - state[37], unused by ddrr_lm_step, takes Sw of the render just judged;
 *   - Sw <= 0 (nothing left of a pose): ncc = 0, A = 0, g = 0, nothing is divided.  Such a pose never moves
 *     (delta = 0: every pivot is DDRR_LM_TINY) and reports ncc 0.
 *
 * Properties (tests/test_wlm.py, tests/test_gpu_wlm.py):
 *   - with w == 1 everywhere the sums [0, 44) and the step are those of the Levenberg-Marquardt library (1 * v
 *     rounds nothing), and the partial [44] of a workgroup is its ray count, Sw == N, exactly;
 *   - c * w scales all 45 sums by c exactly for c a power of two.
 *
 * Conventions
 *  - pointers are DEVICE pointers (HIP, gfx950), borrowed for the call only; `ws` and `state` are
 *    8-byte aligned; the library keeps nothing on the device;
 *  - 0 <= B <= 65535, N >= 1; B == 0 is a valid no-op (nothing launched, nothing written);
 *  - x1_stride is 0 (one fixed image) or N; w_stride is 0 (one weight image) or N;
 *  - a0, a1, a2 in {0: X, 1: Y, 2: Z} with a1 != a0 and a1 != a2 (as ddrr_pose_euler_forward);
 *  - `stream` is a hipStream_t (NULL = default stream); calls are asynchronous and never synchronise
 *    with the host;
 *  - return value: 0 on success, -1 for an argument error (checked before any launch), otherwise a
 *    hipError_t; ddrr_wlm_last_error() describes the last failure (thread-local).
 */
#ifndef DIFFDRR_WLM_HIP_H
#define DIFFDRR_WLM_HIP_H

#define DDRR_WLM_ABI_VERSION 1
#define DDRR_WLM_SUMS 45
#define DDRR_WLM_GROUP_RAYS 1024
#define DDRR_WLM_STATE_DOUBLES 40
#define DDRR_WLM_MAX_POSES 65535

#ifdef __cplusplus
extern "C" {
#endif

int ddrr_wlm_abi_version(void);
const char *ddrr_wlm_last_error(void);

/* bytes of the partial sums ddrr_wlm_normal_sums writes for B poses of N rays (0 for B < 1 or N < 1) */
long ddrr_wlm_workspace_bytes(int B, int N);

/* the 45 weighted sums of every pose as per-workgroup partials in `ws`; with jac != NULL also j_n as (B, N, 6)
 * floats. */
int ddrr_wlm_normal_sums(const float *aux, const float *x1, long x1_stride, const float *w, long w_stride,
                         const float *source_v, const float *Mw, const float *Ainv, const float *P,
                         const float *rot, const float *xyz, int a0, int a1, int a2, const float *reorient34,
                         int B, int N, float eps, int with_img_path, void *ws, float *jac, void *stream);

/* accept or reject the rendered poses, solve, write the next trial poses.
 * up > 1, 0 < down < 1, 0 < lambda_min <= lambda_max, ncc_eps >= 0, all finite. */
int ddrr_wlm_step(const void *ws, void *state, float *rot, float *xyz, int B, int N, double ncc_eps,
                  double up, double down, double lambda_min, double lambda_max, float *ncc_out,
                  void *stream);

#ifdef __cplusplus
}
#endif

#endif
