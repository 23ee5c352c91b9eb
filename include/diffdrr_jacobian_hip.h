/*
 * diffdrr_jacobian_hip.h -- C ABI of libdiffdrr_jacobian_hip.so: the Jacobian determinant of the map
 * x -> x + u(x) of a lattice deformation (gfx950), the count of folded voxels, the volume-preservation penalty
 * on log det (Rohlfing et al. 2003) and the lattice gradient of both.  No entry writes a dense field or a dense
 * derivative, and none uses an atomic: every result is bitwise reproducible.
 *
 * A library of its own, next to libdiffdrr_warp_hip.so (include/diffdrr_warp_hip.h: the trilinear field),
 * libdiffdrr_bspline_hip.so (include/diffdrr_bspline_hip.h: the cubic B-spline) and the others: they share no
 * symbol, no state and no version number.
 *
 * Definitions.  displacement: float (3, Gx, Gy, Gz), contiguous, 2 <= G_a <= D_a; component a is in voxels of
 * axis a, exactly as the warp entries take it.  Cell c and fraction t of voxel x of an axis are those of
 * include/diffdrr_warp_hip.h (integer arithmetic, one division).  With s_b = (G_b - 1) / (D_b - 1):
 *   Field derivative.  J_ab(x) = delta_ab + d u_a / d x_b at every voxel x: the analytic derivative of the
 *     basis in the cell the voxel is assigned to -- the tensor product in which axis b uses derivative weights
 *     times s_b and the other two axes the field's own weights.
 *       DDRR_JACOBIAN_BASIS_LINEAR: derivative weights (-1, +1) on the nodes c, c + 1, the others (1 - t, t).
 *         The derivative is piecewise constant along b; a voxel on a node plane gets its own cell's
 *         derivative (one-sided).
 *       DDRR_JACOBIAN_BASIS_BSPLINE: derivative weights
 *           B'_0 = -(1 - t)^2 / 2,  B'_1 = (3 t^2 - 4 t) / 2,  B'_2 = (-3 t^2 + 2 t + 1) / 2,  B'_3 = t^2 / 2
 *         on the taps clamp(c - 1 + k, 0, G - 1), the others B_k(t) (include/diffdrr_bspline_hip.h); taps are
 *         edge-replicated as in the field.
 *     Formed as the (x, y) sums of each z node the voxel reaches -- nine per node: (w_x w_y, w'_x w_y, w_x w'_y)
 *     times three components, per x tap the y sums and then the x sums, taps ascending, accumulated in double
 *     and rounded to float once -- then the sum in z (ascending, float), times s_b, plus delta_ab.
 *   Determinant.  d(x) = det J(x) by cofactor expansion along the first row, in float:
 *       d = J_00 (J_11 J_22 - J_12 J_21) + J_01 (J_12 J_20 - J_10 J_22) + J_02 (J_10 J_21 - J_11 J_20).
 *     J in millimetres is S J S^-1 for axis-aligned pitches S, so the determinant in voxels is the determinant
 *     in millimetres: no pitch enters.  A zero lattice gives d == 1.0f exactly.
 *   Penalty.  P = (1 / N) sum_x psi(d(x)), N = Dx Dy Dz, with 0 < eps <= 1 and
 *       psi(d) = ln^2 d                                              for d >= eps,
 *       psi(d) = a0 + a1 (d - eps) + a2 (d - eps)^2 / 2              for d <  eps,
 *       a0 = ln^2 eps,  a1 = 2 ln eps / eps,  a2 = 2 (1 - ln eps) / eps^2
 *     (the C^2 continuation of the log term: finite, with a finite gradient, at and below zero).  psi is
 *     evaluated in double from the float d; the sum is of fixed order and in double.
 *   Statistics.  folded = the number of voxels with d <= 0 (int64); range = (min d, max d).
 *   Gradient for an upstream map gradient gD (Dx, Dy, Dz):
 *       gU[a, n] = sum_x sum_b gD(x) cof_ab(x) d J_ab(x) / d U[a, n],   cof the cofactor matrix of J(x);
 *     with gD == NULL it is the penalty's: gD(x) = psi'(d(x)) / N, formed in registers, in float.  A clamped
 *     B-spline tap adds to the border node it was clamped to.
 *
 * Kernels.  A workgroup of 256 threads owns four volume rows (x, y .. y + 3), one wave each, and of each row a
 * chunk of 256 z voxels; a wave collapses x and y once per (row, z node) into LDS (the nine lines above, sized by
 * the most nodes a chunk of the shape reaches), a voxel's J is then 2 (linear) or 4 (B-spline) taps of those lines.
 * Forward: every workgroup reduces its voxels' (psi sum, folded, min, max) in a fixed order -- per wave the tree
 * in which entry i takes entry i + h for h = 32, 16, .. 1, then wave 0 .. 3 ascending -- and writes one 24-byte
 * partial; a second launch of one workgroup folds the partials (thread t the partials t, t + 256, ... ascending,
 * then the same reduction).  ddrr_jacobian_determinant also writes d; ddrr_jacobian_penalty writes nothing per
 * voxel.
 * Backward, B-spline: the separable adjoint in three gathers of fixed order through ws = r1 | r2 (floats),
 * with c_ab = gD cof_ab s_b, w the folded weights and w' the folded derivative weights of an axis
 * (include/diffdrr_bspline_hip.h: chains in ascending voxel order, a clamped tap folded into the border node):
 *     r1[k, a, x, y, n] (3, 3, Dx, Dy, Gz):  k = 0: sum_z w_n c_ax;  k = 1: sum_z w_n c_ay;  k = 2: sum_z w'_n c_az
 *     r2[k, a, x, m, n] (2, 3, Dx, Gy, Gz):  k = 0: sum_y w_m r1[0];  k = 1: sum_y (w'_m r1[1] + w_m r1[2])
 *     gU[a, l, m, n]                       = sum_x (w'_l r2[0] + w_l r2[1])
 *   (float chains for r1, carried from chunk to chunk through r1; double accumulators, rounded once, for r2 and
 *   gU).  Backward, linear: lattice cell by lattice cell in pieces of DDRR_WARP_PIECE_VOXELS voxels with the
 *   fixed-order sums of include/diffdrr_warp_hip.h: 24 floats per (cell, piece), then per node the pieces of
 *   its up to 8 cells in ascending order.
 * ddrr_jacobian_workspace_bytes, one size for the three entries, is the larger of
 *     24 * ceil(Dz / 256) * ceil(Dy / 4) * Dx                           (the forward partials) and
 *     4 * 3 * Dx * Gz * (3 Dy + 2 Gy)                                   (B-spline: r1 | r2), or
 *     4 * 24 * (Gx - 1) (Gy - 1) (Gz - 1) * K                           (linear; K as in ddrr_warp_workspace_bytes).
 *
 * Conventions: those of include/diffdrr_warp_hip.h
 *  - pointers are DEVICE pointers (HIP, gfx950), borrowed for the call only; the library keeps nothing on
 *    the device; outputs must not alias inputs;
 *  - 2 <= G_a <= D_a <= DDRR_JACOBIAN_MAX_DIM and Dx Dy Dz <= 2^31; anything else is an argument error;
 *  - `stream` is a hipStream_t (NULL = default stream); calls are asynchronous and never synchronise
 *    with the host;
 *  - return value: 0 on success, -1 for an argument error (checked before any launch), otherwise a
 *    hipError_t; ddrr_jacobian_last_error() describes the last failure.
 */
#ifndef DIFFDRR_JACOBIAN_HIP_H
#define DIFFDRR_JACOBIAN_HIP_H

#define DDRR_JACOBIAN_ABI_VERSION 1
#define DDRR_JACOBIAN_BASIS_LINEAR 0
#define DDRR_JACOBIAN_BASIS_BSPLINE 1
#define DDRR_JACOBIAN_MAX_DIM 65535
#define DDRR_JACOBIAN_PARTIAL_BYTES 24

#ifdef __cplusplus
extern "C" {
#endif

int ddrr_jacobian_abi_version(void);
const char *ddrr_jacobian_last_error(void);

/* bytes of ws for any of the three entries below; -1 (and a message) outside the domain above */
long ddrr_jacobian_workspace_bytes(int Dx, int Dy, int Dz, int Gx, int Gy, int Gz, int basis);

/* det (Dx, Dy, Dz) = d, folded (one int64) and range (two floats: min d, max d), all written; ws: ws_bytes >=
 * ddrr_jacobian_workspace_bytes(...), 8-byte aligned, written before it is read */
int ddrr_jacobian_determinant(const float *displacement, int Gx, int Gy, int Gz, int Dx, int Dy, int Dz, int basis,
                              float *det, void *ws, long ws_bytes, long *folded, float *range, void *stream);

/* penalty (one double) = P, folded and range as above; nothing per voxel is written */
int ddrr_jacobian_penalty(const float *displacement, int Gx, int Gy, int Gz, int Dx, int Dy, int Dz, int basis,
                          double eps, void *ws, long ws_bytes, double *penalty, long *folded, float *range,
                          void *stream);

/* gU (3, Gx, Gy, Gz), written (not added to): the gradient for gD (Dx, Dy, Dz), or the penalty's (eps) when gD
 * is NULL; eps is checked either way */
int ddrr_jacobian_backward(const float *displacement, int Gx, int Gy, int Gz, int Dx, int Dy, int Dz, int basis,
                           const float *gD, double eps, void *ws, long ws_bytes, float *gU, void *stream);

#ifdef __cplusplus
}
#endif

#endif
