/*
 * diffdrr_wmi_hip.h -- C ABI of libdiffdrr_wmi_hip.so: MutualInformation under per-pixel weights (a mask, a
 * collimator, a confidence map) as fused gfx950 kernels.  The unweighted criterion is include/diffdrr_mi_hip.h.
 *
 * A library of its own, next to libdiffdrr_mi_hip.so: the two share no symbol, no state and no version
 * number.  Both instantiate the kernel bodies of csrc/mi_kernels.h, this one with the weight, at one launch geometry.
 *
 * What is computed, per image pair b (N = H W pixels, K = num_bins bins, w >= 0 and finite -- not looked for):
 *   V = {n: w[n] != 0},  Sw = sum_V w[n]
 *   k1[n,k] = exp(-0.5 ((x1[n] - bins[k]) / sigma)^2)                k2 likewise from x2
 *   P1[k]   = sum_V w[n] k1[n,k] / Sw;  p1 = P1 / (sum_k P1 + epsilon)   p2 likewise
 *   J[k,l]  = sum_V w[n] k1[n,k] k2[n,l];  pJ = J / (sum_kl J + 1e-10)
 *   H1 = -sum_k p1 log2(p1 + epsilon), H2 likewise, H12 = -sum_kl pJ log2(pJ + epsilon)
 *   out[b]  = H1 + H2 - H12, or 2 (H1 + H2 - H12) / (H1 + H2) when `normalize`.
 * A pixel outside V is selected out of every sum, not multiplied by 0: x1 and x2 are not read there (NaN and
 * Inf are safe) and the gradient there is exactly 0.  A pair with Sw = 0 has the value 0 and the gradient 0.
 * With w = 1 everywhere the results are those of include/diffdrr_mi_hip.h bit for bit.
 *
 * Conventions: those of include/diffdrr_mi_hip.h
 *  - pointers are DEVICE pointers to fp32 (HIP, gfx950), borrowed for the call only;
 *  - an image argument is (B, H, W) with `stride` floats between pairs: >= H W, or 0 for ONE image shared by
 *    the batch (an expanded tensor, read in place); the weight `w` likewise with `w_stride`;
 *  - `bins` (num_bins) and `sigma` (one float) are read on the device: no host synchronisation;
 *  - `workspace` is caller-owned device memory of ddrr_wmi_workspace_bytes(B, H, W, num_bins) bytes,
 *    16-byte aligned, that belongs to the call until its work on `stream` is done (contents need
 *    not be initialised).  The library keeps nothing on the device;
 *  - 1 <= num_bins <= 256, H, W >= 1, 0 <= B <= 65535 (B = 0: nothing is launched), epsilon >= 0;
 *  - the results are bitwise reproducible: every sum is taken in a fixed order (no atomics);
 *  - `stream` is a hipStream_t (NULL = default stream); calls are asynchronous;
 *  - return value: 0 on success, -1 for an argument error (checked before any launch), otherwise
 *    a hipError_t; ddrr_wmi_last_error() describes the last failure.
 */
#ifndef DIFFDRR_WMI_HIP_H
#define DIFFDRR_WMI_HIP_H

#define DDRR_WMI_ABI_VERSION 1
#define DDRR_WMI_MAX_BINS 256

#ifdef __cplusplus
extern "C" {
#endif

int ddrr_wmi_abi_version(void);
const char *ddrr_wmi_last_error(void);

/* Bytes of `workspace` for one call of ddrr_wmi_forward; -1 for invalid sizes.  (What ddrr_mi_workspace_bytes
 * returns plus the per-chunk partial sums of the weights: 8 B (chunks + 1) bytes.) */
long ddrr_wmi_workspace_bytes(int B, int H, int W, int num_bins);

/* Floats per pair of the `state` that ddrr_wmi_forward leaves for ddrr_wmi_backward; -1 for an invalid
 * num_bins. */
long ddrr_wmi_state_floats(int num_bins);

/* out (B) = MI(x1[b], x2[b]) under w[b].  `state` (B * ddrr_wmi_state_floats(num_bins) floats) or NULL: when
 * given, the call also leaves there what the gradient needs -- dL/dJ and the two marginal terms (all zero for
 * a pair with Sw = 0).  `weight_sum` (B doubles) or NULL: when given, Sw of every pair. */
int ddrr_wmi_forward(const float *x1, long x1_stride, const float *x2, long x2_stride, const float *w,
                     long w_stride, int B, int H, int W, const float *bins, int num_bins, const float *sigma,
                     float epsilon, int normalize, void *workspace, long workspace_bytes, float *out, float *state,
                     double *weight_sum, void *stream);

/* grad (B, H, W) = g_out[b] * d out[b] / d x2[b] (which = 1), or d out[b] / d x1[b] (which = 0); exactly 0
 * where w == 0.  x1, x2, w, bins, sigma: as given to the forward that filled `state`.  g_out: B floats with
 * g_stride = 1, or one float with g_stride = 0 (the gradient of a sum).  grad has B H W floats also when the
 * differentiated image is shared (stride 0).  No gradient with respect to the weight. */
int ddrr_wmi_backward(const float *x1, long x1_stride, const float *x2, long x2_stride, const float *w,
                      long w_stride, int B, int H, int W, const float *bins, int num_bins, const float *sigma,
                      const float *state, int which, const float *g_out, int g_stride, float *grad, void *stream);

#ifdef __cplusplus
}
#endif

#endif
