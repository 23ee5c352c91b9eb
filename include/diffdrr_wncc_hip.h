/*
 * diffdrr_wncc_hip.h -- C ABI of libdiffdrr_wncc_hip.so: the weighted (masked) normalised cross-correlation
 * of image pairs and the two epilogues of a registration step with a per-pixel weight (gfx950).
 *
 * A library of its own, next to libdiffdrr_hip.so (include/diffdrr_hip.h) and the other satellite
 * libraries: they share no symbol, no state and no version number.  Its kernels include the main library's
 * shared headers (csrc/siddon_core.h, raygen_core.h, record_layout.h) and define none of their arithmetic
 * again; what is new is csrc/wncc_core.h.
 *
 * Definition, per pair b.  x1 (fixed) and x2 (moving) of N pixels, weights w >= 0, finite.
 * V = {n : w_n != 0}, Sw = sum_V w.
 *   mu_i = sum_V w x_i / Sw        var_i = sum_V w x_i^2 / Sw - mu_i^2        s_i = sqrt(var_i + eps)
 *   ncc  = (sum_V w x1 x2 / Sw - mu1 mu2) / (s1 s2)
 *   d ncc / d x2[n] = (w_n / Sw) (z1[n] - ncc z2[n]) / s2,   z_i = (x_i - mu_i) / s_i     (x1 symmetrically)
 *  - a pixel with w_n == 0 is selected out of every sum, not multiplied by zero: x1 and x2 may hold NaN or
 *    Inf there, and its gradient is exactly 0;
 *  - Sw <= 0 (nothing left of a pair): ncc = 0, every gradient 0, mu = 0, s = sqrt(eps), Sw reported as 0;
 *  - w == 1 everywhere is the NCC of include/diffdrr_hip.h (ddrr_ncc_forward, ddrr_siddon_ncc_forward);
 *  - c w gives what w gives (bit for bit for c a power of two);
 *  - negative or non-finite weights are the caller's to exclude: nothing checks them on the device;
 *  - the kernels return no gradient with respect to w.
 * stats (B, DDRR_WNCC_STATS) floats per pair: mu1, s1, mu2, s2, ncc, Sw.
 *
 * How it is summed.  The six raw moments (Sw, sum w x1, sum w x2, sum w x1^2, sum w x2^2, sum w x1 x2) are
 * taken in double.  Workgroup g of pair b covers the pixels [g * DDRR_WNCC_GROUP_RAYS, (g + 1) *
 * DDRR_WNCC_GROUP_RAYS) and writes its partial into slot b * G + g of the caller's workspace, G = ceil(N /
 * DDRR_WNCC_GROUP_RAYS); a second small kernel adds a pair's slots in ascending g, finishes the statistics
 * and, where asked, adds the pairs' values in ascending b.  The backward of the fused step does the same with
 * its twelve partial sums of dL/dMw (floats) and goes on to the pose parameters.  A slot is
 * DDRR_WNCC_SLOT_BYTES bytes (six doubles, or twelve floats).  The workspace needs no initialisation and
 * is left in no particular state: every slot a call reads it has written before.  No atomics, no tickets:
 * the results are bitwise reproducible.  There is ONE launch shape -- DDRR_WNCC_GROUP_RAYS pixels per
 * workgroup, four per thread -- whatever the batch: no variant by launch size.
 *
 * ddrr_wncc_siddon_forward forms x2 = L I on the fly from the blocked record `aux` (csrc/record_layout.h,
 * plane 0) of ddrr_siddon_forward_bricks and the rays' lengths `img`, as ddrr_siddon_ncc_forward does.
 * ddrr_wncc_siddon_backward_pose returns (g_rot, g_xyz) of sum_b g_out[b * g_stride] ncc_b: per ray the
 * weighted d ncc / d x2, siddon_backward_ray<REDUCE_SUM> on the record, raygen_ray_adjoint (with the path
 * through the ray's length unless with_img_path == 0), per pose pose_euler_backward -- the chain of
 * ddrr_siddon_ncc_backward_pose with the weight in the per-pixel gradient.  The rays are generated again
 * from Mw, Ainv and P (csrc/raygen_core.h raygen_ray: the same bits as ddrr_pose_raygen_forward wrote).
 *
 * Conventions
 *  - pointers are DEVICE pointers (HIP, gfx950), borrowed for the call only; `ws` is 8-byte aligned and
 *    holds ddrr_wncc_workspace_bytes(B, N) bytes; the library keeps nothing on the device;
 *  - x1 is (B, N) with x1_stride == N or (1, N) with x1_stride == 0; w likewise with w_stride; x2, img and
 *    the gradients are (B, N); g_stride is 1 or 0 (one value for the batch);
 *  - 16-byte loads where N % 4 == 0 and every row pointer is 16-byte aligned, scalar loads otherwise;
 *  - 0 <= B <= DDRR_WNCC_MAX_POSES, N >= 1; B == 0 is a valid no-op (nothing launched, nothing written);
 *  - eps >= 0 and finite (the NCC's for the forwards, the renderer's for ddrr_wncc_siddon_backward_pose);
 *  - a0, a1, a2 in {0: X, 1: Y, 2: Z} with a1 != a0 and a1 != a2 (as ddrr_pose_euler_forward);
 *  - `stream` is a hipStream_t (NULL = default stream); calls are asynchronous and never synchronise
 *    with the host;
 *  - return value: 0 on success, -1 for an argument error (checked before any launch), otherwise a
 *    hipError_t; ddrr_wncc_last_error() describes the last failure.
 */
#ifndef DIFFDRR_WNCC_HIP_H
#define DIFFDRR_WNCC_HIP_H

#define DDRR_WNCC_ABI_VERSION 1
#define DDRR_WNCC_GROUP_RAYS 1024
#define DDRR_WNCC_STATS 6
#define DDRR_WNCC_SLOT_BYTES 48
#define DDRR_WNCC_MAX_POSES 65535

#ifdef __cplusplus
extern "C" {
#endif

int ddrr_wncc_abi_version(void);
const char *ddrr_wncc_last_error(void);

/* bytes of the per-workgroup partials of B pairs of N pixels (0 for B < 1 or N < 1) */
long ddrr_wncc_workspace_bytes(int B, int N);

/* ncc (B) and stats (B, 6) of the pairs (x1, x2) under w */
int ddrr_wncc_forward(const float *x1, long x1_stride, const float *x2, const float *w, long w_stride, int B,
                      int N, float eps, void *ws, float *ncc, float *stats, void *stream);

/* g_x2 and / or g_x1 (B, N; either may be NULL; g_x1 needs x1_stride == N) of sum_b g_out[b * g_stride] ncc_b */
int ddrr_wncc_backward(const float *x1, long x1_stride, const float *x2, const float *w, long w_stride,
                       const float *stats, const float *g_out, int g_stride, int B, int N, float *g_x1,
                       float *g_x2, void *stream);

/* the same with x2 = img * (plane 0 of the blocked record aux); out (B, N) != NULL: the image is written;
 * ncc_sum != NULL: sum_b ncc_b, added in ascending b */
int ddrr_wncc_siddon_forward(const float *aux, const float *img, const float *x1, long x1_stride,
                             const float *w, long w_stride, int B, int N, float eps, void *ws, float *ncc,
                             float *stats, float *out, float *ncc_sum, void *stream);

/* (g_rot, g_xyz) (B, 3) each of sum_b g_out[b * g_stride] ncc_b */
int ddrr_wncc_siddon_backward_pose(const float *aux, const float *x1, long x1_stride, const float *w,
                                   long w_stride, const float *stats, const float *g_out, int g_stride,
                                   const float *source_v, const float *Mw, const float *Ainv, const float *P,
                                   const float *rot, const float *xyz, int a0, int a1, int a2,
                                   const float *reorient34, int B, int N, float eps, int with_img_path,
                                   void *ws, float *g_rot, float *g_xyz, void *stream);

#ifdef __cplusplus
}
#endif

#endif
