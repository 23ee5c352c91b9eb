/*
 * diffdrr_warp_hip.h -- C ABI of libdiffdrr_warp_hip.so: a free-form deformation of the volume in front
 * of the renderers (gfx950): W = V o (id + u), u the trilinear interpolation of a control lattice, and its
 * two adjoints.
 *
 * A library of its own, next to libdiffdrr_hip.so (include/diffdrr_hip.h), libdiffdrr_mi_hip.so,
 * libdiffdrr_recon_hip.so, libdiffdrr_fbp_hip.so and libdiffdrr_lm_hip.so: they share no symbol, no state
 * and no version number.
 *
 * Definitions.  V: float (Dx, Dy, Dz), contiguous, z fastest.  displacement: float (3, Gx, Gy, Gz),
 * contiguous, 2 <= G_a <= D_a; component a is in voxels of axis a.
 *   Lattice.  Node i of axis a sits at voxel coordinate i (D_a - 1) / (G_a - 1).  Voxel x of axis a lies in
 *     cell  c = min(floor(x (G_a - 1) / (D_a - 1)), G_a - 2)   (integer arithmetic: exact), at
 *     frac  t = (x (G_a - 1) - c (D_a - 1)) / (D_a - 1)        (an exact integer, one division)
 *     so cell c holds the voxels [ceil(c (D_a - 1) / (G_a - 1)), ceil((c + 1) (D_a - 1) / (G_a - 1))), the
 *     last cell also voxel D_a - 1 (t = 1).
 *   Field.  u_a(x) = sum over the 8 nodes n of the voxel's cell of hat_n(x) displacement[a, n],
 *     hat_n = w_x w_y w_z, w = 1 - t at the cell's lower node and t at its upper one (formed as the
 *     bilinear sum in x, y of each of the two z nodes, then the sum in z).
 *   Sampling.  p_a = x_a + u_a(x), i0 = floor(p), f = p - i0, formed as i0 = x_a + floor(u_a) and
 *     f = u_a - floor(u_a) (the same numbers; p itself is never rounded to a float), with u_a clamped to
 *     [-(D_a + 2), D_a + 2] first (beyond it every corner is outside the volume: no result changes, every
 *     index stays finite);
 *       W[x] = sum over the 8 corners c of w_c V[i0 + c],   w_c the product of (1 - f_a) or f_a per axis.
 *     DDRR_WARP_PADDING_ZEROS: corners outside the volume contribute 0;  _BORDER: their indices are
 *     clamped to [0, D_a - 1].  u = 0 gives f = 0 and W == V exactly.
 *   Gradients for an upstream gW:
 *       gU[a, n] = sum_x hat_n(x) gW[x] d_a V(p(x)),   d_a V(p) the derivative of the sum above in f_a
 *                  (a corner outside the volume: 0 with zeros padding; with border padding both corners
 *                  clamp to one voxel and the derivative vanishes); at f = 0 it is V[i + 1] - V[i];
 *       gV = the trilinear scatter of gW: gV[i0 + c] += w_c gW[x].
 *
 * ddrr_warp_backward_displacement uses no atomics and is bitwise reproducible: lattice cell (cx, cy, cz)
 * (linear index (cx (Gy - 1) + cy) (Gz - 1) + cz) is cut into K pieces of DDRR_WARP_PIECE_VOXELS voxels of
 * its box in z-fastest order, K = ceil(largest cell's voxel count / DDRR_WARP_PIECE_VOXELS) for every cell.
 * A workgroup of 256 threads sums one piece -- thread t the voxels t, t + 256, ... of the piece in that
 * order, then per value eight slices of 32 threads in ascending order, then the slices in ascending order --
 * and writes DDRR_WARP_PIECE_FLOATS = 24 floats, [node (i, j, k) of the cell: 4 i + 2 j + k][component a],
 * to ws[(cell * K + piece) * 24 + .].  A second launch adds, per node and component, the pieces of its up
 * to 8 incident cells in ascending (cell, piece) order.  The result depends on the inputs and the shapes
 * only.
 * ddrr_warp_backward_volume adds with float atomics (global_atomic_add_f32): its result is NOT bitwise
 * reproducible from launch to launch (the order of the adds into a voxel is the hardware's).
 *
 * Conventions
 *  - pointers are DEVICE pointers (HIP, gfx950), borrowed for the call only; the library keeps nothing on
 *    the device; outputs must not alias inputs;
 *  - 2 <= G_a <= D_a <= DDRR_WARP_MAX_DIM and Dx Dy Dz <= 2^31 (offsets are computed in 64 bits all the
 *    same); anything else is an argument error;
 *  - `stream` is a hipStream_t (NULL = default stream); calls are asynchronous and never synchronise
 *    with the host;
 *  - return value: 0 on success, -1 for an argument error (checked before any launch), otherwise a
 *    hipError_t; ddrr_warp_last_error() describes the last failure.
 */
#ifndef DIFFDRR_WARP_HIP_H
#define DIFFDRR_WARP_HIP_H

#define DDRR_WARP_ABI_VERSION 1
#define DDRR_WARP_PADDING_ZEROS 0
#define DDRR_WARP_PADDING_BORDER 1
#define DDRR_WARP_MAX_DIM 65535
#define DDRR_WARP_PIECE_VOXELS 1024
#define DDRR_WARP_PIECE_FLOATS 24

#ifdef __cplusplus
extern "C" {
#endif

int ddrr_warp_abi_version(void);
const char *ddrr_warp_last_error(void);

/* W (Dx, Dy, Dz) = V o (id + u): one pass over the output */
int ddrr_warp_forward(const float *V, int Dx, int Dy, int Dz, const float *displacement, int Gx, int Gy,
                      int Gz, int padding, float *W, void *stream);

/* bytes of the per-piece partial sums of ddrr_warp_backward_displacement; -1 (and a message) outside the
 * domain above */
long ddrr_warp_workspace_bytes(int Dx, int Dy, int Dz, int Gx, int Gy, int Gz);

/* gU (3, Gx, Gy, Gz), written (not added to); ws: ws_bytes >= ddrr_warp_workspace_bytes(...), 4-byte
 * aligned, every byte of the queried size is written before it is read */
int ddrr_warp_backward_displacement(const float *V, int Dx, int Dy, int Dz, const float *displacement,
                                    int Gx, int Gy, int Gz, int padding, const float *gW, void *ws,
                                    long ws_bytes, float *gU, void *stream);

/* gV (Dx, Dy, Dz), written (cleared, then the scatter): not bitwise reproducible */
int ddrr_warp_backward_volume(const float *displacement, int Gx, int Gy, int Gz, int Dx, int Dy, int Dz,
                              int padding, const float *gW, float *gV, void *stream);

#ifdef __cplusplus
}
#endif

#endif
