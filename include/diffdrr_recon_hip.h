/*
 * diffdrr_recon_hip.h -- C ABI of libdiffdrr_recon_hip.so: what a volume reconstruction iteration
 * does around the renderer (reference notebooks/tutorials/reconstruction.ipynb), as fused gfx950
 * kernels: 3-D total variation with its gradient, and an Adam step of the volume with the
 * projection onto [lower, upper] folded in.
 *
 * A library of its own, next to libdiffdrr_hip.so (include/diffdrr_hip.h) and libdiffdrr_mi_hip.so
 * (include/diffdrr_mi_hip.h): they share no symbol, no state and no version number.
 *
 * Total variation of a (Dx, Dy, Dz) fp32 volume V, z fastest, voxel spacing (sx, sy, sz), with
 * forward differences that are zero past the last plane:
 *   dx[i,j,k] = (V[i+1,j,k] - V[i,j,k]) / sx   if i + 1 < Dx else 0        (dy, dz likewise)
 *   DDRR_RECON_TV_ISOTROPIC:    n = sqrt(dx^2 + dy^2 + dz^2 + eps^2),  TV = sum n,
 *                               px, py, pz = dx / (n sx), dy / (n sy), dz / (n sz)
 *   DDRR_RECON_TV_ANISOTROPIC:  TV = sum |dx| + |dy| + |dz|,
 *                               px, py, pz = sign(dx) / sx, sign(dy) / sy, sign(dz) / sz,  sign(0) = 0
 *   dTV/dV[i,j,k] = -(px + py + pz)[i,j,k] + px[i-1,j,k] + py[i,j-1,k] + pz[i,j,k-1]
 *                   (terms with an index of -1 absent).
 *
 * Conventions
 *  - pointers are DEVICE pointers to fp32 (HIP, gfx950), 4-byte aligned, borrowed for the call only;
 *  - `workspace` is caller-owned device memory of ddrr_recon_tv_workspace_bytes(Dx, Dy, Dz) bytes,
 *    16-byte aligned, that belongs to the call until its work on `stream` is done (contents need
 *    not be initialised).  The library keeps nothing on the device;
 *  - 0 <= Dx, Dy, Dz <= 65535 and Dx Dy Dz <= 2^34; an empty volume or tensor is a valid no-op
 *    (nothing is launched, nothing is written);
 *  - the results are bitwise reproducible: every sum is taken in a fixed order (no atomics);
 *  - `stream` is a hipStream_t (NULL = default stream); calls are asynchronous and never
 *    synchronise with the host: what they need from the device (`scale`, `step`) is read there;
 *  - return value: 0 on success, -1 for an argument error (checked before any launch), otherwise
 *    a hipError_t; ddrr_recon_last_error() describes the last failure.
 */
#ifndef DIFFDRR_RECON_HIP_H
#define DIFFDRR_RECON_HIP_H

#define DDRR_RECON_ABI_VERSION 1
#define DDRR_RECON_TV_ISOTROPIC 0
#define DDRR_RECON_TV_ANISOTROPIC 1
#define DDRR_RECON_MAX_DIM 65535

#ifdef __cplusplus
extern "C" {
#endif

int ddrr_recon_abi_version(void);
const char *ddrr_recon_last_error(void);

/* Bytes of `workspace` for one call of ddrr_recon_tv3d (0 for an empty volume); -1 for invalid sizes. */
long ddrr_recon_tv_workspace_bytes(int Dx, int Dy, int Dz);

/* value[0] = TV(volume), and, in the same pass over the volume, with g = dTV/dV and
 * w = weight * (scale ? scale[0] : 1):
 *   grad == NULL:                   nothing more (weight, scale and accumulate are not used);
 *   grad != NULL, accumulate == 0:  grad  = w g      (every voxel is written);
 *   grad != NULL, accumulate != 0:  grad += w g      (one fused multiply-add per voxel).
 * `scale` is one DEVICE float or NULL (the upstream gradient of an autograd node, read on the
 * device); `weight` a host number.  `value` is the unweighted TV.  `grad` must not overlap `volume`.
 * sx, sy, sz > 0 and finite; eps >= 0 and finite (isotropic only: with eps = 0 the gradient at a
 * voxel whose three differences vanish is 0 / 0, as it is for the formula). */
int ddrr_recon_tv3d(const float *volume, int Dx, int Dy, int Dz, float sx, float sy, float sz, int mode,
                    float eps, float *grad, int accumulate, float weight, const float *scale, void *workspace,
                    long workspace_bytes, float *value, void *stream);

/* One step of torch.optim.Adam (no weight decay, no amsgrad) on n floats, in place, then the projection
 * param = min(max(param, lower), upper) in the same pass (-inf / +inf: no bound; lower <= upper):
 *   t = step[0] + 1;  g = maximize ? -grad : grad
 *   exp_avg += (g - exp_avg)(1 - beta1);  exp_avg_sq = beta2 exp_avg_sq + (1 - beta2) g^2
 *   param -= lr / (1 - beta1^t) * exp_avg / (sqrt(exp_avg_sq) / sqrt(1 - beta2^t) + eps)
 * with the operations in the order of torch's single-tensor implementation (the bias corrections in
 * double, the rest in fp32, rounded where torch's kernels round: bit-identical on the device to
 * torch.optim.Adam's default, multi-tensor flavour).  `step` is ONE DEVICE float, the number of steps taken so far; the call
 * leaves step[0] + 1 there (a second, one-thread launch behind the update: nothing else writes it).
 * 0 <= n <= 2^40; lr, eps >= 0; 0 <= beta1, beta2 < 1.  16-byte accesses where all four tensors are
 * 16-byte aligned. */
int ddrr_recon_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float *step, long n,
                         double lr, double beta1, double beta2, double eps, float lower, float upper, int maximize,
                         void *stream);

#ifdef __cplusplus
}
#endif

#endif
