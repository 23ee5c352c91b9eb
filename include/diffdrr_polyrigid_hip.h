/*
 * diffdrr_polyrigid_hip.h -- C ABI of libdiffdrr_polyrigid_hip.so: a polyrigid deformation of the volume in
 * front of the renderers (gfx950): W = V o (id + u), u(x) the displacement of the rigid motion exp(xi(x)),
 * xi the trilinear interpolation of a lattice of twists, and its two adjoints.
 *
 * A library of its own, next to libdiffdrr_hip.so (include/diffdrr_hip.h), libdiffdrr_mi_hip.so,
 * libdiffdrr_recon_hip.so, libdiffdrr_fbp_hip.so, libdiffdrr_lm_hip.so, libdiffdrr_warp_hip.so and
 * libdiffdrr_bspline_hip.so: they share no symbol, no state and no version number.
 *
 * The model.  K bodies, each with a twist theta_k = (omega_k, v_k) (a rotation vector in radians, a
 * translation in mm), and non-negative weights (K, Gx, Gy, Gz) that sum to 1 over k at every lattice node.
 * The twists are blended in the Lie algebra, Xi[c, n] = sum_k weights[k, n] theta[k, c]; that sum stays in
 * front of this library, which never sees K.
 *
 * Definitions.  V: float (Dx, Dy, Dz), contiguous, z fastest.  Xi: float (6, Gx, Gy, Gz), contiguous,
 * 2 <= G_a <= D_a; components 0..2 are omega, 3..5 are v.  Voxel pitch h = (hx, hy, hz) in mm.
 *   Lattice.  Node, cell c and fraction t of a voxel are those of include/diffdrr_warp_hip.h (integer cell, one
 *     division).
 *   Twist.  xi_c(x) = the trilinear interpolation of Xi[c] at x, formed per component as seven linear
 *     interpolations  a + t (b - a): along x of the four node pairs of the cell, along y of the two pairs of
 *     results, along z last.  (A lattice that is constant in a component gives that constant exactly.)
 *   Displacement.  y_a = h_a (x_a - (D_a - 1) / 2)  (mm from the volume's centre),  s = |omega|^2,
 *       u_mm = omega x a + omega x (omega x b) + v,   a = A(s) y + B(s) v,   b = B(s) y + C(s) v
 *            = A omega x y + B omega x (omega x y) + v + B omega x v + C omega x (omega x v)  = exp(xi) y - y,
 *       A = sin(phi) / phi,  B = (1 - cos(phi)) / phi^2,  C = (phi - sin(phi)) / phi^3,  phi = sqrt(s),
 *       u_a = u_mm,a / h_a  (voxels of axis a).   u is formed directly, never as p - x.
 *     A, B, C are functions of s.  For s < DDRR_POLYRIGID_SERIES_BELOW (= 9/4, phi < 1.5) they and their
 *     derivatives in s are the Taylor series in s with DDRR_POLYRIGID_SERIES_TERMS = 8 terms, by Horner's rule:
 *       A = sum_n (-s)^n / (2n + 1)!,   B = sum_n (-s)^n / (2n + 2)!,   C = sum_n (-s)^n / (2n + 3)!
 *     (the first dropped term is below 1e-11 of the sum at the seam; theta = 0 has a finite gradient and no
 *     0 / 0); from there on the closed forms, with  A' = (C - B) / 2,  B' = (A - 2 B) / (2 s),
 *     C' = (B - 3 C) / (2 s).  At the seam phi - sin(phi) = 0.50: nothing cancels, and the two forms agree to
 *     float rounding.
 *   Sampling.  That of include/diffdrr_warp_hip.h: i0 = x + floor(u), f = u - floor(u), u_a clamped to
 *     [-(D_a + 2), D_a + 2] first; eight corners; DDRR_POLYRIGID_PADDING_ZEROS or _BORDER.  Xi = 0 gives u = 0
 *     and W == V exactly.
 *   Precision.  The sample position -- the fractions, the twist at the voxel, y, A, B, C and u -- is formed in
 *     double from the float inputs; floor(u) is taken from the double and only f is rounded to float (an f that
 *     rounds to 1 stays in its voxel, at f = 1).  u is a difference of terms of |omega| |y|, hundreds of mm on a
 *     long axis, and floor(u) decides which forward difference the gradients take.  The interpolation of V, the
 *     adjoint below (on the twist and y rounded to float) and every sum are float.
 *   Gradients for an upstream gW:
 *       gXi[c, n] = sum_x hat_n(x) sum_a gW[x] d_a V(p(x)) d u_a / d xi_c (x),   hat_n the trilinear weight of
 *                   node n at x, d_a V as in include/diffdrr_warp_hip.h (at f = 0 the forward difference);
 *                   with g_a = gW d_a V / h_a:
 *                     d / d v     = g + B g x omega + C (omega (omega . g) - s g)
 *                     d / d omega = a x g + (omega x b) x g + b x (g x omega) + 2 omega (g . n),
 *                     n = omega x (A' y + B' v) + omega x (omega x (B' y + C' v));
 *       gV = the trilinear scatter of gW: gV[i0 + c] += w_c gW[x].
 *
 * ddrr_polyrigid_backward_twists uses no atomics and is bitwise reproducible: the pieces and the order of the
 * sums are those of ddrr_warp_backward_displacement (include/diffdrr_warp_hip.h) -- lattice cell (cx, cy, cz)
 * (linear index (cx (Gy - 1) + cy) (Gz - 1) + cz) is cut into P pieces of DDRR_POLYRIGID_PIECE_VOXELS voxels
 * of its box in z-fastest order, P = ceil(largest cell's voxel count / DDRR_POLYRIGID_PIECE_VOXELS) for every
 * cell.  A workgroup of 256 threads sums one piece -- thread t the voxels t, t + 256, ... of the piece in that
 * order, then per value eight slices of 32 threads in ascending order, then the slices in ascending order --
 * and writes DDRR_POLYRIGID_PIECE_FLOATS = 48 floats, [node (i, j, k) of the cell: 4 i + 2 j + k][component c],
 * to ws[(cell * P + piece) * 48 + .].  A second launch adds, per node and component, the pieces of its up to
 * 8 incident cells in ascending (cell, piece) order.  The result depends on the inputs and the shapes only.
 * ddrr_polyrigid_backward_volume adds with float atomics (global_atomic_add_f32): its result is NOT bitwise
 * reproducible from launch to launch (the order of the adds into a voxel is the hardware's).
 *
 * Stated limitation: the weights live on the lattice, so a body is exactly rigid only over the cells where its
 * weight is 1 at all eight nodes.  A lattice as fine as the volume (G_a = D_a) is allowed.
 *
 * Conventions
 *  - pointers are DEVICE pointers (HIP, gfx950), borrowed for the call only; the library keeps nothing on
 *    the device; outputs must not alias inputs; the pitch is passed by value;
 *  - 2 <= G_a <= D_a <= DDRR_POLYRIGID_MAX_DIM and Dx Dy Dz <= 2^31 (offsets are computed in 64 bits all the
 *    same), h_a > 0 and finite; anything else is an argument error;
 *  - `stream` is a hipStream_t (NULL = default stream); calls are asynchronous and never synchronise
 *    with the host;
 *  - return value: 0 on success, -1 for an argument error (checked before any launch), otherwise a
 *    hipError_t; ddrr_polyrigid_last_error() describes the last failure.
 */
#ifndef DIFFDRR_POLYRIGID_HIP_H
#define DIFFDRR_POLYRIGID_HIP_H

#define DDRR_POLYRIGID_ABI_VERSION 1
#define DDRR_POLYRIGID_PADDING_ZEROS 0
#define DDRR_POLYRIGID_PADDING_BORDER 1
#define DDRR_POLYRIGID_MAX_DIM 65535
#define DDRR_POLYRIGID_PIECE_VOXELS 1024
#define DDRR_POLYRIGID_PIECE_FLOATS 48
#define DDRR_POLYRIGID_SERIES_TERMS 8
/* the seam in s = |omega|^2 as a fraction: the series below NUM / DEN, the closed forms from there on */
#define DDRR_POLYRIGID_SERIES_BELOW_NUM 9
#define DDRR_POLYRIGID_SERIES_BELOW_DEN 4

#ifdef __cplusplus
extern "C" {
#endif

int ddrr_polyrigid_abi_version(void);
const char *ddrr_polyrigid_last_error(void);

/* W (Dx, Dy, Dz) = V o (id + u): one pass over the output; no dense field exists in memory */
int ddrr_polyrigid_forward(const float *V, int Dx, int Dy, int Dz, const float *Xi, int Gx, int Gy, int Gz,
                           float hx, float hy, float hz, int padding, float *W, void *stream);

/* bytes of the per-piece partial sums of ddrr_polyrigid_backward_twists: a function of the shapes only; -1 (and
 * a message) outside the domain above */
long ddrr_polyrigid_workspace_bytes(int Dx, int Dy, int Dz, int Gx, int Gy, int Gz);

/* gXi (6, Gx, Gy, Gz), written (not added to); ws: ws_bytes >= ddrr_polyrigid_workspace_bytes(...), 4-byte
 * aligned, every byte of the queried size is written before it is read */
int ddrr_polyrigid_backward_twists(const float *V, int Dx, int Dy, int Dz, const float *Xi, int Gx, int Gy,
                                   int Gz, float hx, float hy, float hz, int padding, const float *gW, void *ws,
                                   long ws_bytes, float *gXi, void *stream);

/* gV (Dx, Dy, Dz), written (cleared, then the scatter): not bitwise reproducible */
int ddrr_polyrigid_backward_volume(const float *Xi, int Gx, int Gy, int Gz, int Dx, int Dy, int Dz, float hx,
                                   float hy, float hz, int padding, const float *gW, float *gV, void *stream);

#ifdef __cplusplus
}
#endif

#endif
