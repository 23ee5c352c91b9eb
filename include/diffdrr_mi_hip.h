/*
 * diffdrr_mi_hip.h -- C ABI of libdiffdrr_mi_hip.so: MutualInformation (reference
 * diffdrr/metrics.py:110-139, through kornia's marginal_pdf / joint_pdf) as fused gfx950 kernels.
 *
 * A library of its own, next to libdiffdrr_hip.so (include/diffdrr_hip.h): the two share no
 * symbol, no state and no version number.
 *
 * What is computed, per image pair b (N = H W pixels, K = num_bins bins):
 *   k1[n,k] = exp(-0.5 ((x1[n] - bins[k]) / sigma)^2)           k2 likewise from x2
 *   P1[k]   = mean_n k1[n,k];  p1 = P1 / (sum_k P1 + epsilon)     p2 likewise
 *   J[k,l]  = sum_n k1[n,k] k2[n,l];  pJ = J / (sum_kl J + 1e-10)
 *   H1 = -sum_k p1 log2(p1 + epsilon), H2 likewise, H12 = -sum_kl pJ log2(pJ + epsilon)
 *   out[b]  = H1 + H2 - H12, or 2 (H1 + H2 - H12) / (H1 + H2) when `normalize`.
 * No (N, K) kernel-value tensor exists: the operands of the fp32 MFMAs that form J are evaluated
 * from the images in registers.
 *
 * Conventions
 *  - pointers are DEVICE pointers to fp32 (HIP, gfx950), borrowed for the call only;
 *  - an image argument is (B, H, W) with `stride` floats between pairs: H W, or 0 for ONE image
 *    shared by the batch (an expanded tensor, read in place);
 *  - `bins` (num_bins) and `sigma` (one float) are read on the device: no host synchronisation;
 *  - `workspace` is caller-owned device memory of ddrr_mi_workspace_bytes(B, H, W, num_bins) bytes,
 *    16-byte aligned, that belongs to the call until its work on `stream` is done (contents need
 *    not be initialised).  The library keeps nothing on the device;
 *  - 1 <= num_bins <= 256, H, W >= 1, 0 <= B <= 65535 (B = 0: nothing is launched), epsilon >= 0;
 *  - the results are bitwise reproducible: every sum is taken in a fixed order (no atomics);
 *  - `stream` is a hipStream_t (NULL = default stream); calls are asynchronous;
 *  - return value: 0 on success, -1 for an argument error (checked before any launch), otherwise
 *    a hipError_t; ddrr_mi_last_error() describes the last failure.
 */
#ifndef DIFFDRR_MI_HIP_H
#define DIFFDRR_MI_HIP_H

#define DDRR_MI_ABI_VERSION 1
#define DDRR_MI_MAX_BINS 256

#ifdef __cplusplus
extern "C" {
#endif

int ddrr_mi_abi_version(void);
const char *ddrr_mi_last_error(void);

/* Bytes of `workspace` for one call of ddrr_mi_forward; -1 for invalid sizes. */
long ddrr_mi_workspace_bytes(int B, int H, int W, int num_bins);

/* Floats per pair of the `state` that ddrr_mi_forward leaves for ddrr_mi_backward; -1 for an invalid
 * num_bins. */
long ddrr_mi_state_floats(int num_bins);

/* out (B) = MI(x1[b], x2[b]).  `state` (B * ddrr_mi_state_floats(num_bins) floats) or NULL: when
 * given, the call also leaves there what the gradient needs -- dL/dJ and the two marginal terms. */
int ddrr_mi_forward(const float *x1, long x1_stride, const float *x2, long x2_stride, int B, int H, int W,
                    const float *bins, int num_bins, const float *sigma, float epsilon, int normalize,
                    void *workspace, long workspace_bytes, float *out, float *state, void *stream);

/* grad (B, H, W) = g_out[b] * d out[b] / d x2[b] (which = 1), or d out[b] / d x1[b] (which = 0):
 * the similarity is symmetric, so both are one launch.  x1, x2, bins, sigma: as given to the forward
 * that filled `state`.  g_out: B floats with g_stride = 1, or one float with g_stride = 0 (the gradient
 * of a sum).  grad has B H W floats also when the differentiated image is shared (stride 0). */
int ddrr_mi_backward(const float *x1, long x1_stride, const float *x2, long x2_stride, int B, int H, int W,
                     const float *bins, int num_bins, const float *sigma, const float *state, int which,
                     const float *g_out, int g_stride, float *grad, void *stream);

#ifdef __cplusplus
}
#endif

#endif
