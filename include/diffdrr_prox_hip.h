/*
 * diffdrr_prox_hip.h -- C ABI of libdiffdrr_prox_hip.so: the proximal operator of the 3-D total variation
 * with a box constraint inside it, by the fast gradient projection of Beck & Teboulle (2009), as fused gfx950
 * kernels.  It is the inner solver of FISTA reconstruction (diffdrr_amd.reconstruction.Fista).
 *
 * A library of its own, next to libdiffdrr_recon_hip.so (include/diffdrr_recon_hip.h: the smoothed TV and the
 * Adam step) and the others: they share no symbol, no state and no version number.
 *
 * Definitions.  b, x: fp32 (Dx, Dy, Dz), z fastest.  A dual field p: fp32 (3, Dx, Dy, Dz), component a along
 * axis a.  Spacing (sx, sy, sz).
 *   D, the forward differences of include/diffdrr_recon_hip.h, zero past the last plane:
 *       (D x)_x[i,j,k] = (x[i+1,j,k] - x[i,j,k]) / sx  if i + 1 < Dx else 0              (y, z likewise)
 *   D^T, its exact adjoint; a dual component on the last plane of its axis never contributes:
 *       (D^T p)[i,j,k] = (u_x[i-1,j,k] - u_x[i,j,k]) / sx + (y, z likewise),
 *       u_x[i,j,k] = p_x[i,j,k] if 0 <= i and i + 1 < Dx else 0
 *   TV(x) = sum |D x|_2 per voxel (DDRR_PROX_TV_ISOTROPIC) or sum |D x|_1 (DDRR_PROX_TV_ANISOTROPIC): the
 *       non-smooth TV, no eps.
 *   P_C(v) = min(max(v, lower), upper);  -inf / +inf: no bound.
 *   prox(b) = argmin_{x in C} 1/2 |x - b|^2 + lambda TV(x), by n = `iterations` steps from the dual start p_0
 *   (what `dual` holds on entry), r_0 = p_0, t_0 = 1, Lip = 4 (1/sx^2 + 1/sy^2 + 1/sz^2):
 *       x       = P_C(b - lambda D^T r_k)
 *       p_{k+1} = Pi(r_k + D x / (Lip lambda))     Pi: isotropic p / max(1, |p|_2) per voxel,
 *                                                      anisotropic clamp(p, -1, 1) per component
 *       t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2;   r_{k+1} = p_{k+1} + ((t_k - 1) / t_{k+1}) (p_{k+1} - p_k)
 *   result: x_out = P_C(b - lambda D^T p_n), and dual = p_n (the warm start of the next call).  The t_k are host
 *   doubles, rounded to float once per launch.  lambda == 0: x_out = P_C(b), no iteration runs, `dual` is left
 *   as given.
 *   With x_prev: the final primal step also writes y_out = x_out + beta (x_out - x_prev) (one fused
 *   multiply-add), FISTA's extrapolation, in the pass that already holds x_out.
 *
 * Kernels.  One inner iteration is two passes.  Each is a (y, z) tile of 16 x 64 voxels marched along x over 32
 * planes, four consecutive z voxels per lane with 16-byte accesses from any dword alignment (Dz is arbitrary),
 * the plane a voxel's neighbours come from staged in LDS with its coordinates clamped to the volume (every read
 * is inside it); differences past the last plane and terms of index -1 are set by selects.
 *   primal:  x = P_C(b - lambda D^T r); r_x of plane i - 1 is carried in registers, r_y of row j - 1 and r_z of
 *            voxel k - 1 come from LDS.  16 B read, 4 B written per voxel.
 *   dual:    p, r <- the update above, in place (pointwise in p and r); x of plane i + 1 is carried in registers,
 *            x of row j + 1 and voxel k + 1 come from LDS.  28 B read, 24 B written per voxel.
 * 72 B per voxel per inner iteration; the final primal pass reads 16 B (20 B with x_prev) and writes 4 B (8 B).
 * `scratch` holds r: 3 Dx Dy Dz floats (ddrr_prox_workspace_bytes), needed when iterations > 0 and lambda > 0;
 * x_out holds the x of every iteration.  No other volume-sized memory, no atomics, no reductions: the results
 * are bitwise reproducible.
 *
 * Conventions: those of include/diffdrr_recon_hip.h
 *  - pointers are DEVICE pointers to fp32 (HIP, gfx950), 4-byte aligned, borrowed for the call only; the library
 *    keeps nothing on the device;
 *  - 0 <= Dx, Dy, Dz <= DDRR_PROX_MAX_DIM and Dx Dy Dz <= 2^34; an empty volume is a valid no-op;
 *  - x_out, y_out, dual and scratch must not overlap b; x_out must not overlap x_prev, dual or scratch;
 *    y_out must not overlap x_out, dual or scratch (y_out may be x_prev itself); scratch must not overlap dual,
 *    nor x_prev either of them;
 *  - `stream` is a hipStream_t (NULL = default stream); the call runs all its launches on it and never
 *    synchronises with the host;
 *  - return value: 0 on success, -1 for an argument error (checked before any launch), otherwise a hipError_t;
 *    ddrr_prox_last_error() describes the last failure.
 */
#ifndef DIFFDRR_PROX_HIP_H
#define DIFFDRR_PROX_HIP_H

#define DDRR_PROX_ABI_VERSION 1
#define DDRR_PROX_TV_ISOTROPIC 0
#define DDRR_PROX_TV_ANISOTROPIC 1
#define DDRR_PROX_MAX_DIM 65535

#ifdef __cplusplus
extern "C" {
#endif

int ddrr_prox_abi_version(void);
const char *ddrr_prox_last_error(void);

/* bytes of `scratch` for a call with these sizes (0 for an empty volume or iterations == 0); -1 (and a message)
 * for invalid sizes */
long ddrr_prox_workspace_bytes(int Dx, int Dy, int Dz, int iterations);

/* x_out = prox(b), dual: p_0 in, p_n out.  x_prev, y_out: both NULL, or both given (beta finite).  scratch may be
 * NULL when ddrr_prox_workspace_bytes(...) is 0 or lambda == 0. */
int ddrr_prox_tv3d(const float *b, int Dx, int Dy, int Dz, float sx, float sy, float sz, int mode, float lambda,
                   int iterations, float lower, float upper, float *dual, float *scratch, long scratch_bytes,
                   float *x_out, const float *x_prev, float beta, float *y_out, void *stream);

#ifdef __cplusplus
}
#endif

#endif
