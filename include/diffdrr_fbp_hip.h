/*
 * diffdrr_fbp_hip.h -- C ABI of libdiffdrr_fbp_hip.so: the two passes of an analytic (FDK) start of a
 * cone-beam reconstruction, as gfx950 kernels: cosine weighting + 1-D filtering of the projections,
 * and voxel-driven backprojection of the filtered projections into the volume.
 *
 * A library of its own, next to libdiffdrr_hip.so (include/diffdrr_hip.h), libdiffdrr_mi_hip.so
 * (include/diffdrr_mi_hip.h) and libdiffdrr_recon_hip.so (include/diffdrr_recon_hip.h): they share no
 * symbol, no state and no version number.
 *
 * Filter.  `images` is (B, H, W), W fastest.  With `axis == 0` the filtered index n, k is the column
 * (within a row; L = W), with `axis == 1` it is the row (within a column; L = H):
 *   out[b, ., n] = scale * sum_k taps[(n - k) + L - 1] * images[b, ., k] * cw[., k]      (k ascending)
 *   cw(r, c) = sdd / sqrt(sdd^2 + (u0 + c du)^2 + (v0 + r dv)^2),   or 1 when cosine_weight == 0
 * `taps` holds 2 L - 1 floats, its centre (lag 0) at index L - 1.  The products are summed in double
 * and rounded once.
 *
 * Backprojection.  `volume` is (Dx, Dy, Dz), z fastest; `views` holds 16 floats per view: a row-major
 * 3 x 4 matrix M_b (12 floats), a weight w_b, 3 unused floats.  For the voxel (i, j, k):
 *   (a, b, U)^T = M_b (i, j, k, 1)^T,   col = a / U,   row = b / U      (pixel centres at integers)
 *   volume[i, j, k] (+)= sum_b w_b * (distance_weight ? 1 / U^2 : 1) * bilinear(images[b], row, col)
 * summed in ascending b.  The bilinear sample takes the four neighbours of (floor(row), floor(col)):
 *   (I[r0, c0] (1 - fc) + I[r0, c0 + 1] fc) (1 - fr) + (I[r0 + 1, c0] (1 - fc) + I[r0 + 1, c0 + 1] fc) fr
 * where a neighbour outside 0 <= r < H, 0 <= c < W counts as zero.  A view with U <= 0 or a non-finite
 * coordinate contributes zero to the voxel.  a, b and U are computed for every voxel on its own, as
 * three fused multiply-adds per component (in double, from the float matrix), never stepped along an
 * axis: the error does not grow with the volume's size.  With accumulate == 0 every voxel is written;
 * otherwise the sum over the views is added to what the voxel holds.
 *
 * Conventions
 *  - pointers are DEVICE pointers to fp32 (HIP, gfx950), 4-byte aligned, borrowed for the call only;
 *    the library keeps nothing on the device;
 *  - filter: 0 <= B, 0 <= H, W <= 4096, B H W <= 2^31; `out` must not overlap `images`;
 *  - backprojection: 0 <= B <= 65535, 0 <= H, W <= 4096, 0 <= Dx, Dy, Dz <= 65535, Dx Dy Dz <= 2^34
 *    (64-bit voxel offsets); `volume` must not overlap `images`;
 *  - empty inputs are valid no-ops: an empty `images` for the filter and an empty volume for the
 *    backprojection launch nothing and write nothing (a backprojection of B = 0 views or of empty
 *    images into a non-empty volume is a sum of nothing: zeros, or the volume unchanged);
 *  - the results are bitwise reproducible: every sum is taken in a fixed order (no atomics);
 *  - `stream` is a hipStream_t (NULL = default stream); calls are asynchronous and never
 *    synchronise with the host;
 *  - return value: 0 on success, -1 for an argument error (checked before any launch), otherwise
 *    a hipError_t; ddrr_fbp_last_error() describes the last failure.
 */
#ifndef DIFFDRR_FBP_HIP_H
#define DIFFDRR_FBP_HIP_H

#define DDRR_FBP_ABI_VERSION 1
#define DDRR_FBP_MAX_IMAGE_DIM 4096
#define DDRR_FBP_MAX_VIEWS 65535
#define DDRR_FBP_MAX_DIM 65535
#define DDRR_FBP_VIEW_FLOATS 16

#ifdef __cplusplus
extern "C" {
#endif

int ddrr_fbp_abi_version(void);
const char *ddrr_fbp_last_error(void);

/* out = scale * (taps convolved along `axis` with images * cw): the definition above.  sdd > 0 and
 * u0, du, v0, dv, sdd, scale finite (u0, du, v0, dv, sdd are read only with cosine_weight != 0). */
int ddrr_fbp_filter(const float *images, int B, int H, int W, int axis, const float *taps, float scale,
                    float u0, float du, float v0, float dv, float sdd, int cosine_weight, float *out,
                    void *stream);

/* volume (+)= the weighted backprojection of images through `views` (B x 16 floats): the definition
 * above. */
int ddrr_fbp_backproject(const float *images, int B, int H, int W, const float *views, int distance_weight,
                         float *volume, int Dx, int Dy, int Dz, int accumulate, void *stream);

#ifdef __cplusplus
}
#endif

#endif
