// prox.hip -- the proximal operator of the 3-D total variation with a box constraint, by fast gradient
// projection, as fused gfx950 kernels: the C ABI of include/diffdrr_prox_hip.h (libdiffdrr_prox_hip.so).
//
// One inner iteration is two passes over the volume, both on the scheme of recon.hip's tv3d_kernel: a workgroup
// owns a (y, z) tile of kTY x kTZ voxels and marches it along x over kXC planes; every lane owns four consecutive
// z voxels (16-byte accesses from any dword alignment); the plane a voxel's y and z neighbours come from is
// staged in LDS, fetched with its coordinates CLAMPED to the volume so that every read is inside it; the x
// neighbour is carried in registers.  Differences past the last plane and terms of index -1 are set by selects.
//   prox_primal_kernel<EPI>  x = P_C(b - lambda D^T r): r_y with the row below the tile and r_z with the column
//       below it in LDS, r_x of plane i - 1 in registers.  EPI: also y = x + beta (x - x_prev).
//   prox_dual_kernel<MODE>   p <- Pi(r + D x / (Lip lambda)), r <- p + c (p - p_old), pointwise in p and r: x
//       with the row and the column above the tile in LDS, x of plane i + 1 in registers.
// The planes are double-buffered in LDS (one barrier per plane) and the next plane's loads are issued before the
// current one is computed.  The arithmetic of a voxel is csrc/prox_core.h's.  No atomics, no reductions.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "prox_core.h"

namespace {

using namespace ddrr_prox;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));  // 16 bytes from any dword address

thread_local char g_err[512] = "";

int fail(int code, const char *what) {
    snprintf(g_err, sizeof(g_err), "%s", what);
    return code;
}

int finish(const char *where) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "%s: %s", where, hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

constexpr int kTZ = 64;       // tile: voxels along z (16 lanes x 4: one 256-byte run per row)
constexpr int kTY = 16;       // tile: rows (4 per wave)
constexpr int kXC = 32;       // planes one workgroup marches through
constexpr int kThreads = 256;
// a staged row: [3] = voxel k0 - 1, [4 .. 67] = the tile's, [68] = voxel k0 + 64 (quads 16-byte aligned)
constexpr int kRowF = 72;
constexpr int kPlaneF = (kTY + 1) * kRowF;  // the tile's rows and one halo row

__device__ __forceinline__ f32x4 load_quad(const float *row, int k, int Dz) {
    if (k + 3 < Dz) return *reinterpret_cast<const f32x4_a4 *>(row + k);
    f32x4 v;  // (the row's last quad and beyond: the last voxel repeated)
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = row[min(k + e, Dz - 1)];
    return v;
}

__device__ __forceinline__ void store_quad(float *row, int k, int Dz, bool row_ok, f32x4 v) {
    if (!row_ok) return;
    if (k + 3 < Dz) {
        *reinterpret_cast<f32x4_a4 *>(row + k) = v;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k + e < Dz) row[k + e] = v[e];
    }
}

// ---------------------------------------------------------------------------------------------- primal
struct PrimalArgs {
    const float *b;
    const float *r;       // (3, Dx, Dy, Dz), or NULL: no dual term (lambda == 0)
    float *x;
    const float *x_prev;  // EPI
    float *y;             // EPI
    long n;               // Dx Dy Dz
    float beta;
    Params q;
};

struct PrimalFetch {
    f32x4 b, rx, ry, rz, ry_halo;
    float rz_halo;
};

__device__ __forceinline__ void fetch(PrimalFetch &f, const PrimalArgs &a, int plane, int j0, int k0, int t) {
    const int r = t >> 4, k = k0 + 4 * (t & 15);
    const long row = ((long)plane * a.q.Dy + min(j0 + r, a.q.Dy - 1)) * a.q.Dz;
    f.b = load_quad(a.b + row, k, a.q.Dz);
    if (!a.r) return;
    f.rx = load_quad(a.r + row, k, a.q.Dz);
    f.ry = load_quad(a.r + a.n + row, k, a.q.Dz);
    f.rz = load_quad(a.r + 2 * a.n + row, k, a.q.Dz);
    if (r == 0)  // row j0 - 1
        f.ry_halo = load_quad(a.r + a.n + ((long)plane * a.q.Dy + max(j0 - 1, 0)) * a.q.Dz, k, a.q.Dz);
    if ((t & 15) == 0) f.rz_halo = a.r[2 * a.n + row + max(k0 - 1, 0)];  // column k0 - 1
}

// rows 0 .. kTY of `ry`: j0 - 1 .. j0 + kTY - 1; rows 0 .. kTY - 1 of `rz`: the tile's, [3] = column k0 - 1
__device__ __forceinline__ void commit(const PrimalFetch &f, float *ry, float *rz, int t) {
    const int r = t >> 4, q = t & 15;
    *reinterpret_cast<f32x4 *>(ry + (r + 1) * kRowF + 4 + 4 * q) = f.ry;
    if (r == 0) *reinterpret_cast<f32x4 *>(ry + 4 + 4 * q) = f.ry_halo;
    if (q == 0) rz[r * kRowF + 3] = f.rz_halo;
    rz[r * kRowF + 4 + 4 * q + 3] = f.rz[3];  // (what the next lane needs of this one)
}

template <bool EPI>
__global__ __launch_bounds__(kThreads) void prox_primal_kernel(const PrimalArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[2][2 * kPlaneF];
    const int t = threadIdx.x, r = t >> 4, q = t & 15;
    const int k0 = blockIdx.x * kTZ, j0 = blockIdx.y * kTY, x0 = blockIdx.z * kXC;
    const int x1 = min(x0 + kXC, a.q.Dx);
    const int j = j0 + r, k = k0 + 4 * q;
    const bool row_ok = j < a.q.Dy, oky = j + 1 < a.q.Dy, dual = a.r != nullptr;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 rx_lo = zero;  // r_x of plane i - 1
    if (dual && x0 > 0) rx_lo = load_quad(a.r + ((long)(x0 - 1) * a.q.Dy + min(j, a.q.Dy - 1)) * a.q.Dz, k, a.q.Dz);
    PrimalFetch f;
    f.rx = f.ry = f.rz = f.ry_halo = zero;
    f.rz_halo = 0.f;
    fetch(f, a, x0, j0, k0, t);
    for (int i = x0; i < x1; ++i) {
        float *ry = lds[i & 1], *rz = ry + kPlaneF;
        if (dual) commit(f, ry, rz, t);
        const PrimalFetch cur = f;
        if (i + 1 < x1) fetch(f, a, i + 1, j0, k0, t);
        __syncthreads();
        const long at = ((long)i * a.q.Dy + j) * a.q.Dz;
        f32x4 xp = zero;
        if (EPI && row_ok) xp = load_quad(a.x_prev + at, k, a.q.Dz);
        f32x4 ry_lo = zero;
        float rz_lo = 0.f;
        if (dual) {
            ry_lo = *reinterpret_cast<const f32x4 *>(ry + r * kRowF + 4 + 4 * q);
            rz_lo = rz[r * kRowF + 3 + 4 * q];
        }
        const bool okx = i + 1 < a.q.Dx;
        const float zl[4] = {rz_lo, cur.rz[0], cur.rz[1], cur.rz[2]};
        f32x4 x, y;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            x[e] = primal(cur.b[e], okx ? cur.rx[e] : 0.f, i > 0 ? rx_lo[e] : 0.f, oky ? cur.ry[e] : 0.f,
                          j > 0 ? ry_lo[e] : 0.f, k + e + 1 < a.q.Dz ? cur.rz[e] : 0.f, k + e > 0 ? zl[e] : 0.f, a.q);
            if (EPI) y[e] = extrapolate(x[e], xp[e], a.beta);
        }
        store_quad(a.x + at, k, a.q.Dz, row_ok, x);
        if (EPI) store_quad(a.y + at, k, a.q.Dz, row_ok, y);
        rx_lo = cur.rx;
    }
}

// ------------------------------------------------------------------------------------------------ dual
struct DualArgs {
    const float *x;
    const float *r_in;  // (3, Dx, Dy, Dz); may be p itself (step 0: r_0 = p_0)
    float *p;           // in place
    float *r_out;       // or NULL: the last step's r is not needed
    long n;
    float c;            // (t_k - 1) / t_{k+1}
    Params q;
};

struct DualFetch {
    f32x4 own, row_halo;
    float col_halo;
};

__device__ __forceinline__ void fetch(DualFetch &f, const DualArgs &a, int plane, int j0, int k0, int t) {
    const int r = t >> 4, k = k0 + 4 * (t & 15);
    const long row = ((long)plane * a.q.Dy + min(j0 + r, a.q.Dy - 1)) * a.q.Dz;
    f.own = load_quad(a.x + row, k, a.q.Dz);
    if (r == 0)  // row j0 + kTY
        f.row_halo = load_quad(a.x + ((long)plane * a.q.Dy + min(j0 + kTY, a.q.Dy - 1)) * a.q.Dz, k, a.q.Dz);
    if ((t & 15) == 0) f.col_halo = a.x[row + min(k0 + kTZ, a.q.Dz - 1)];  // column k0 + kTZ
}

// rows 0 .. kTY of `plane`: j0 .. j0 + kTY; [4 + kTZ] = column k0 + kTZ
__device__ __forceinline__ void commit(const DualFetch &f, float *plane, int t) {
    const int r = t >> 4, q = t & 15;
    *reinterpret_cast<f32x4 *>(plane + r * kRowF + 4 + 4 * q) = f.own;
    if (r == 0) *reinterpret_cast<f32x4 *>(plane + kTY * kRowF + 4 + 4 * q) = f.row_halo;
    if (q == 0) plane[r * kRowF + 4 + kTZ] = f.col_halo;
}

// (the isotropic form takes 132 registers, three waves per SIMD: bounding it to 128 spills four of them)
template <int MODE>
__global__ __launch_bounds__(kThreads) void prox_dual_kernel(const DualArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[2][kPlaneF];
    const int t = threadIdx.x, r = t >> 4, q = t & 15;
    const int k0 = blockIdx.x * kTZ, j0 = blockIdx.y * kTY, x0 = blockIdx.z * kXC;
    const int x1 = min(x0 + kXC, a.q.Dx);
    const int j = j0 + r, k = k0 + 4 * q;
    const bool row_ok = j < a.q.Dy, oky = j + 1 < a.q.Dy;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    DualFetch f;
    f.row_halo = zero;
    f.col_halo = 0.f;
    fetch(f, a, x0, j0, k0, t);
    for (int i = x0; i < x1; ++i) {
        float *plane = lds[i & 1];
        commit(f, plane, t);
        fetch(f, a, min(i + 1, a.q.Dx - 1), j0, k0, t);  // (its own quad is this plane's x neighbour)
        const long row = ((long)i * a.q.Dy + min(j, a.q.Dy - 1)) * a.q.Dz;
        f32x4 pv[3], rv[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) rv[c] = load_quad(a.r_in + c * a.n + row, k, a.q.Dz);
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 3; ++c) pv[c] = load_quad(a.p + c * a.n + row, k, a.q.Dz);
        const f32x4 x = *reinterpret_cast<const f32x4 *>(plane + r * kRowF + 4 + 4 * q);
        const f32x4 x_yp = *reinterpret_cast<const f32x4 *>(plane + (r + 1) * kRowF + 4 + 4 * q);
        const float xz[5] = {x[0], x[1], x[2], x[3], plane[r * kRowF + 8 + 4 * q]};
        const bool okx = i + 1 < a.q.Dx;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float d[3] = {difference(x[e], f.own[e], a.q.isx, okx), difference(x[e], x_yp[e], a.q.isy, oky),
                                difference(xz[e], xz[e + 1], a.q.isz, k + e + 1 < a.q.Dz)};
            float p[3] = {pv[0][e], pv[1][e], pv[2][e]}, rr[3] = {rv[0][e], rv[1][e], rv[2][e]};
            dual_step<MODE>(d, a.q.inv, a.c, p, rr);
#pragma unroll
            for (int c = 0; c < 3; ++c) pv[c][e] = p[c], rv[c][e] = rr[c];
        }
        const long at = ((long)i * a.q.Dy + j) * a.q.Dz;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            store_quad(a.p + c * a.n + at, k, a.q.Dz, row_ok, pv[c]);
            if (a.r_out) store_quad(a.r_out + c * a.n + at, k, a.q.Dz, row_ok, rv[c]);
        }
    }
}

}  // namespace

extern "C" {

int ddrr_prox_abi_version(void) { return DDRR_PROX_ABI_VERSION; }
const char *ddrr_prox_last_error(void) { return g_err; }

long ddrr_prox_workspace_bytes(int Dx, int Dy, int Dz, int iterations) {
    if (const char *what = dims_error(Dx, Dy, Dz)) return fail(-1, what);
    if (iterations < 0) return fail(-1, "iterations must be >= 0");
    return workspace_bytes(Dx, Dy, Dz, iterations);
}

int ddrr_prox_tv3d(const float *b, int Dx, int Dy, int Dz, float sx, float sy, float sz, int mode, float lambda,
                   int iterations, float lower, float upper, float *dual, float *scratch, long scratch_bytes,
                   float *x_out, const float *x_prev, float beta, float *y_out, void *stream) {
    if (const char *what = argument_error(b, Dx, Dy, Dz, sx, sy, sz, mode, lambda, iterations, lower, upper, dual,
                                          scratch, scratch_bytes, x_out, x_prev, beta, y_out))
        return fail(-1, what);
    const long n = (long)Dx * Dy * Dz;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((Dz + kTZ - 1) / kTZ), (unsigned)((Dy + kTY - 1) / kTY), (unsigned)((Dx + kXC - 1) / kXC));
    const dim3 block(kThreads);
    PrimalArgs pa;
    pa.b = b, pa.x = x_out, pa.x_prev = nullptr, pa.y = nullptr, pa.n = n, pa.beta = 0.f;
    pa.q = make_params(Dx, Dy, Dz, sx, sy, sz, lambda, lower, upper);
    DualArgs da;
    da.x = x_out, da.p = dual, da.n = n, da.q = pa.q;
    double t = 1.0;
    for (int k = 0; lambda > 0.f && k < iterations; ++k) {
        pa.r = da.r_in = k == 0 ? dual : scratch;
        hipLaunchKernelGGL(prox_primal_kernel<false>, grid, block, 0, s, pa);
        if (int rc = finish("ddrr_prox_tv3d (primal)")) return rc;
        const double t1 = next_t(t);
        da.c = (float)((t - 1.0) / t1);
        da.r_out = k + 1 < iterations ? scratch : nullptr;
        t = t1;
        if (mode == DDRR_PROX_TV_ISOTROPIC)
            hipLaunchKernelGGL(prox_dual_kernel<DDRR_PROX_TV_ISOTROPIC>, grid, block, 0, s, da);
        else
            hipLaunchKernelGGL(prox_dual_kernel<DDRR_PROX_TV_ANISOTROPIC>, grid, block, 0, s, da);
        if (int rc = finish("ddrr_prox_tv3d (dual)")) return rc;
    }
    pa.r = lambda > 0.f ? dual : nullptr;
    if (x_prev) {
        pa.x_prev = x_prev, pa.y = y_out, pa.beta = beta;
        hipLaunchKernelGGL(prox_primal_kernel<true>, grid, block, 0, s, pa);
    } else {
        hipLaunchKernelGGL(prox_primal_kernel<false>, grid, block, 0, s, pa);
    }
    return finish("ddrr_prox_tv3d (result)");
}

}  // extern "C"
