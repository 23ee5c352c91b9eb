/*
 * diffdrr_lm_hip.h -- C ABI of libdiffdrr_lm_hip.so: the two kernels a Levenberg-Marquardt registration
 * step adds behind the renderer (gfx950): the normal-equations sums of a rendered pose from the brick
 * kernel's backward record, and the accept / reject / solve step on them.
 *
 * A library of its own, next to libdiffdrr_hip.so (include/diffdrr_hip.h), libdiffdrr_mi_hip.so,
 * libdiffdrr_recon_hip.so and libdiffdrr_fbp_hip.so: they share no symbol, no state and no version
 * number.  Its kernels include the main library's shared headers (csrc/siddon_core.h, raygen_core.h,
 * record_layout.h) and define none of their arithmetic again.
 *
 * Definitions, per pose b.  theta = (rot, xyz) in R^6, radians and mm.  Mw (3, 4), source_v (3) and the
 * blocked float record `aux` (csrc/record_layout.h) are what ddrr_pose_raygen_forward and
 * ddrr_siddon_forward_bricks (include/diffdrr_hip.h) produced for theta.  For pixel n with calibrated
 * detector point P_n:
 *   ray  = raygen_ray(Mw, Ainv, P_n)
 *   x_n  = ray.L * rec_n[0]                       the image value, as ddrr_siddon_ncc_forward forms it
 *   f_n  = x1[b * x1_stride + n]                  the fixed image (x1_stride: 0 = one for all poses, or N)
 *   a_n  in R^12: what these calls add to a zeroed accumulator,
 *            siddon_backward_ray<REDUCE_SUM>(rec_n, source_v, ray.tv, eps, ray.L, gs, gt)
 *            raygen_ray_adjoint(Mw, Ainv, P_n, gt, gs, with_img_path ? rec_n[0] : 0, ray.L, .)
 *   j_n  = D^T a_n in R^6, D the 12 x 6 derivative of pose_euler_forward at theta, applied as
 *          pose_euler_backward applies it: j_n = pose_euler_adjoint_apply(pose_euler_adjoint_setup(theta), a_n)
 *          (csrc/raygen_core.h) -- the operations ddrr_siddon_backward_pose_euler performs for a grad_out
 *          that is 1 at pixel n and 0 elsewhere
 * so that sum_n w_n j_n is what ddrr_siddon_backward_pose_euler returns for grad_out = w, up to the order
 * of that sum.
 *
 * The 44 sums of a pose, in this order (DDRR_LM_SUMS doubles):
 *   [0, 21)   H = sum j j^T, upper triangle, row-major: (0,0) (0,1) ... (0,5) (1,1) ... (5,5)
 *   [21, 27)  a = sum j          [27, 33)  c = sum x j          [33, 39)  d = sum f j
 *   [39, 44)  sum x, sum f, sum x^2, sum f^2, sum x f
 * They are the products of pairs of u_n = (j_n, x_n, f_n, 1).  ddrr_lm_normal_sums writes them as
 * per-workgroup partials: workgroup w of pose b covers the rays [w * DDRR_LM_GROUP_RAYS,
 * (w + 1) * DDRR_LM_GROUP_RAYS) and writes the doubles ws[(b * G + w) * DDRR_LM_SUMS + .],
 * G = ceil(N / DDRR_LM_GROUP_RAYS).  j_n and x_n are float; every product is formed in double (exact) and
 * every sum is taken in double, in a fixed order: within a workgroup five interleaved slices of its rays
 * (ray i of the workgroup in slice i mod 5), each in ascending order, then the slices in ascending order.
 * ddrr_lm_step adds the partials of a pose in ascending w.  No atomics: the results are bitwise
 * reproducible.
 *
 * ddrr_lm_step, per pose, everything in double:
 *   1. S = the 44 sums.  mu_x = Sx / N, v_x = Sxx / N - mu_x^2, s_x = sqrt(v_x + ncc_eps); likewise f.
 *        ncc = (Sxf / N - mu_x mu_f) / (s_x s_f),     rho = v_x / (v_x + ncc_eps)
 *        u = (c - mu_x a) / s_x,     w = (d - mu_f a) / s_f
 *        A = [H - a a^T / N - (2 - rho) u u^T / N] / s_x^2
 *        g = [(1 - rho + ncc) u - w] / s_x
 *      -- J_r^T J_r and J_r^T r of the residual r = z(x) - z(f), z = (. - mean) / sqrt(var + ncc_eps),
 *      whose objective 1/2 |r|^2 is N (1 - ncc) up to ncc_eps.
 *   2. With the pose's state (DDRR_LM_STATE_DOUBLES doubles, caller-owned, all zero before the first
 *      call except lambda):
 *        [0, 6) best theta   [6] its ncc   [7, 28) its A (upper triangle, as H)   [28, 34) its g
 *        [34] lambda   [35] valid (0 / 1)   [36] accepted (0 / 1: what the last call did)   [37, 40) unused
 *      not valid, or ncc > ncc_best: the rendered pose (rot, xyz as they are) becomes the best one with
 *      its ncc, A, g; valid = accepted = 1; lambda <- max(lambda * down, lambda_min).
 *      Otherwise accepted = 0 and lambda <- min(lambda * up, lambda_max).
 *   3. (A + lambda diag(A) + DDRR_LM_TINY I) delta = -g of the best pose, by Cholesky (lower triangle,
 *      column by column).  A pivot that is not > 0 gives delta = 0 and once more
 *      lambda <- min(lambda * up, lambda_max).   DDRR_LM_TINY is 1e-30.
 *   4. (rot, xyz) <- theta_best + delta, rounded to float, in place; ncc_out[b] = ncc_best.
 * Every render is thus either an accepted or a rejected trial; nothing is read back by the host and no
 * launch depends on data, so a step can be captured in a graph.
 *
 * Conventions
 *  - pointers are DEVICE pointers (HIP, gfx950), borrowed for the call only; `ws` and `state` are
 *    8-byte aligned; the library keeps nothing on the device;
 *  - 0 <= B <= 65535, N >= 1; B == 0 is a valid no-op (nothing launched, nothing written);
 *  - a0, a1, a2 in {0: X, 1: Y, 2: Z} with a1 != a0 and a1 != a2 (as ddrr_pose_euler_forward);
 *  - `stream` is a hipStream_t (NULL = default stream); calls are asynchronous and never synchronise
 *    with the host;
 *  - return value: 0 on success, -1 for an argument error (checked before any launch), otherwise a
 *    hipError_t; ddrr_lm_last_error() describes the last failure.
 */
#ifndef DIFFDRR_LM_HIP_H
#define DIFFDRR_LM_HIP_H

#define DDRR_LM_ABI_VERSION 1
#define DDRR_LM_SUMS 44
#define DDRR_LM_GROUP_RAYS 1024
#define DDRR_LM_STATE_DOUBLES 40
#define DDRR_LM_MAX_POSES 65535

#ifdef __cplusplus
extern "C" {
#endif

int ddrr_lm_abi_version(void);
const char *ddrr_lm_last_error(void);

/* bytes of the partial sums ddrr_lm_normal_sums writes for B poses of N rays (0 for B < 1 or N < 1) */
long ddrr_lm_workspace_bytes(int B, int N);

/* the 44 sums of every pose as per-workgroup partials in `ws`; with jac != NULL also j_n as (B, N, 6)
 * floats.  x1_stride is 0 (one fixed image) or N. */
int ddrr_lm_normal_sums(const float *aux, const float *x1, long x1_stride, const float *source_v,
                        const float *Mw, const float *Ainv, const float *P, const float *rot,
                        const float *xyz, int a0, int a1, int a2, const float *reorient34, int B, int N,
                        float eps, int with_img_path, void *ws, float *jac, void *stream);

/* accept or reject the rendered poses, solve, write the next trial poses: steps 1-4 above.
 * up > 1, 0 < down < 1, 0 < lambda_min <= lambda_max, ncc_eps >= 0, all finite. */
int ddrr_lm_step(const void *ws, void *state, float *rot, float *xyz, int B, int N, double ncc_eps,
                 double up, double down, double lambda_min, double lambda_max, float *ncc_out,
                 void *stream);

#ifdef __cplusplus
}
#endif

#endif
