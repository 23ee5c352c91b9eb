/*
 * diffdrr_bspline_hip.h -- C ABI of libdiffdrr_bspline_hip.so: the cubic B-spline free-form deformation of
 * the volume in front of the renderers (gfx950): W = V o (id + u), u the tensor-product cubic B-spline of a
 * control lattice (Rueckert et al. 1999), and its two adjoints.
 *
 * A library of its own, next to libdiffdrr_warp_hip.so (include/diffdrr_warp_hip.h: the trilinear field) and
 * the five others: they share no symbol, no state and no version number.
 *
 * Definitions.  V: float (Dx, Dy, Dz), contiguous, z fastest.  displacement: float (3, Gx, Gy, Gz),
 * contiguous, 2 <= G_a <= D_a; component a is in voxels of axis a.
 *   Lattice.  As in include/diffdrr_warp_hip.h: voxel x of axis a lies in
 *     cell  c = min(floor(x (G_a - 1) / (D_a - 1)), G_a - 2)   (integer arithmetic: exact), at
 *     frac  t = (x (G_a - 1) - c (D_a - 1)) / (D_a - 1)        (an exact integer, one division).
 *   Field.  Per axis  u = sum_{k = 0..3} B_k(t) coeff[clamp(c - 1 + k, 0, G_a - 1)]  with
 *       B_0 = (1 - t)^3 / 6,  B_1 = (3 t^3 - 6 t^2 + 4) / 6,  B_2 = (-3 t^3 + 3 t^2 + 3 t + 1) / 6,  B_3 = t^3 / 6,
 *     and the field is the tensor product over the three axes: 4 x 4 x 4 coefficients per voxel, formed as the
 *     (x, y) sum of each of the four z nodes (x taps outer, y taps inner, ascending), then the sum in z
 *     (ascending).  Border coefficients are edge-replicated, so the lattice keeps the shape of the trilinear
 *     one.  The spline APPROXIMATES: u at a node is (c[n-1] + 4 c[n] + c[n+1]) / 6 per axis, not c[n].  It is
 *     C^2 inside the lattice; constants are reproduced everywhere, functions linear in the node index in
 *     every cell 1 <= c <= G_a - 3 (not in the two border cells, where a tap is clamped).
 *   Sampling.  Exactly include/diffdrr_warp_hip.h's: u_a clamped to [-(D_a + 2), D_a + 2],
 *     i0 = x_a + floor(u_a), f = u_a - floor(u_a) (p = x + u is never rounded to a float), the 8 corners
 *     with DDRR_BSPLINE_PADDING_ZEROS (corners outside the volume contribute 0) or _BORDER (indices clamped
 *     to [0, D_a - 1]).  A zero lattice gives f = 0 and W == V bit for bit.
 *   Gradients for an upstream gW:
 *       gU[a, n] = sum_x B_n(x) gW[x] d_a V(p(x)),  B_n(x) the product over the axes of the weights of the
 *                  taps of x that land on node n: a clamped tap adds to the border node it was clamped to;
 *                  d_a V(p) as in include/diffdrr_warp_hip.h;
 *       gV = the trilinear scatter of gW: gV[i0 + c] += w_c gW[x].
 *
 * ddrr_bspline_backward_displacement uses no atomics and is bitwise reproducible: the separable adjoint in
 * three gathers of fixed order, through the workspace ws = r1 | r2 (floats):
 *     r1[a, x, y, n] (3, Dx, Dy, Gz) = sum_z w^z_n(z) q_a(x, y, z),   q_a = gW d_a V(p),
 *     r2[a, x, m, n] (3, Dx, Gy, Gz) = sum_y w^y_m(y) r1[a, x, y, n],
 *     gU[a, l, m, n]                 = sum_x w^x_l(x) r2[a, x, m, n],
 *   each sum a chain of  acc = acc + w v  from 0 (a float for r1; a double, rounded once at the end, for r2
 *   and gU, whose chains grow with the axis: tens of thousands of terms at 65535 voxels) over the voxels of the cells max(n - 2, 0) .. min(n + 1, G - 2)
 *   of that axis in ascending voxel order; voxel x of cell c carries the weight of its tap k = n + 1 - c,
 *   folded: in cell 0 the weight of tap 0 is added to tap 1's (w_1 = B_1 + B_0), in cell G - 2 tap 3's to
 *   tap 2's (w_2 = B_2 + B_3).  The first gather walks a row in pieces of DDRR_BSPLINE_CHUNK_VOXELS voxels and
 *   carries the chain from piece to piece through r1 (the first piece that reaches a node stores, later ones
 *   continue), so the pieces do not show in the result.  It depends on the inputs and the shapes only.
 *   ddrr_bspline_workspace_bytes = 4 * 3 * Dx * Gz * (Dy + Gy).
 * ddrr_bspline_backward_volume adds with float atomics (global_atomic_add_f32): its result is NOT bitwise
 * reproducible from launch to launch.
 *
 * Conventions: those of include/diffdrr_warp_hip.h
 *  - pointers are DEVICE pointers (HIP, gfx950), borrowed for the call only; the library keeps nothing on
 *    the device; outputs must not alias inputs;
 *  - 2 <= G_a <= D_a <= DDRR_BSPLINE_MAX_DIM and Dx Dy Dz <= 2^31; anything else is an argument error;
 *  - `stream` is a hipStream_t (NULL = default stream); calls are asynchronous and never synchronise
 *    with the host;
 *  - return value: 0 on success, -1 for an argument error (checked before any launch), otherwise a
 *    hipError_t; ddrr_bspline_last_error() describes the last failure.
 */
#ifndef DIFFDRR_BSPLINE_HIP_H
#define DIFFDRR_BSPLINE_HIP_H

#define DDRR_BSPLINE_ABI_VERSION 1
#define DDRR_BSPLINE_PADDING_ZEROS 0
#define DDRR_BSPLINE_PADDING_BORDER 1
#define DDRR_BSPLINE_MAX_DIM 65535
#define DDRR_BSPLINE_CHUNK_VOXELS 256
#define DDRR_BSPLINE_ROWS 4

#ifdef __cplusplus
extern "C" {
#endif

int ddrr_bspline_abi_version(void);
const char *ddrr_bspline_last_error(void);

/* W (Dx, Dy, Dz) = V o (id + u): one pass over the output */
int ddrr_bspline_forward(const float *V, int Dx, int Dy, int Dz, const float *displacement, int Gx, int Gy,
                         int Gz, int padding, float *W, void *stream);

/* bytes of r1 | r2 of ddrr_bspline_backward_displacement; -1 (and a message) outside the domain above */
long ddrr_bspline_workspace_bytes(int Dx, int Dy, int Dz, int Gx, int Gy, int Gz);

/* gU (3, Gx, Gy, Gz), written (not added to); ws: ws_bytes >= ddrr_bspline_workspace_bytes(...), 4-byte
 * aligned, every byte of the queried size is written before it is read */
int ddrr_bspline_backward_displacement(const float *V, int Dx, int Dy, int Dz, const float *displacement,
                                       int Gx, int Gy, int Gz, int padding, const float *gW, void *ws,
                                       long ws_bytes, float *gU, void *stream);

/* gV (Dx, Dy, Dz), written (cleared, then the scatter): not bitwise reproducible */
int ddrr_bspline_backward_volume(const float *displacement, int Gx, int Gy, int Gz, int Dx, int Dy, int Dz,
                                 int padding, const float *gW, float *gV, void *stream);

#ifdef __cplusplus
}
#endif

#endif
