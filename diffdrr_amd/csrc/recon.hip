// recon.hip -- what a reconstruction iteration does to the volume around the renderer, as fused gfx950
// kernels: the C ABI of include/diffdrr_recon_hip.h (libdiffdrr_recon_hip.so).
//
//   tv3d_kernel<MODE, GRAD>  3-D total variation, value and gradient in ONE pass over the volume.  The
//       stencil of dTV/dV at a voxel lies inside the [-1, +1]^3 box around it: a workgroup owns a (y, z)
//       tile of kTY x kTZ voxels and marches it along x over kXC planes with two planes of the tile (one
//       voxel of halo around them) live in LDS and a third one in flight from memory.  Every lane owns
//       four consecutive z voxels: a wave reads and writes four 256-byte runs with 16-byte accesses
//       from any dword alignment (Dz is arbitrary).  The planes are staged with their coordinates
//       CLAMPED to the volume, so every read is inside it; differences past the last plane and the
//       terms of index -1 are set to zero by selects (not left to x - x: inf - inf is not 0).  What a
//       voxel needs of its lower neighbours (px of plane i - 1, py of row j - 1, pz of voxel k - 1) is
//       carried in registers along x and recomputed from LDS along y and z.  Per-workgroup partial
//       values, in double, go to the workspace ...
//   tv3d_sum_kernel          ... and are summed by one workgroup in a fixed order, in double.
//   adam_kernel<VEC>         torch.optim.Adam's update of a flat tensor + clamp, 16 B read and 12 B
//       written per element; the bias corrections once per workgroup, in double, from the device's
//       step counter, which adam_count_kernel (one thread, behind it on the stream) increments.
// No atomics anywhere: value and gradient are bitwise reproducible.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/diffdrr_recon_hip.h"

namespace {

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

// ------------------------------------------------------------------------------------ total variation
constexpr int kTZ = 64;        // tile: voxels along z (16 lanes x 4: one 256-byte run per row)
constexpr int kTY = 16;        // tile: rows (4 per wave)
constexpr int kXC = 32;        // planes one workgroup marches through (+ 1 to warm up px)
constexpr int kTvThreads = 256;
// a staged row: [3] = voxel k0 - 1, [4 .. 67] = the tile's, [68] = voxel k0 + 64 (quads 16-byte aligned)
constexpr int kRowF = 72;
constexpr int kPlaneF = (kTY + 2) * kRowF;  // rows j0 - 1 .. j0 + kTY
constexpr int kSumThreads = 1024;
constexpr long kMaxVoxels = 1L << 34;

struct TvArgs {
    const float *vol;
    float *grad;
    const float *scale;
    double *partial;
    int Dx, Dy, Dz;
    float isx, isy, isz, eps2, weight;
};

// What one thread fetches of a plane for the tile: its own quad, and for some threads a quad of the two
// halo rows or one voxel of the two halo columns.
struct Staged {
    f32x4 own, ext;
    float halo;
};

__device__ __forceinline__ f32x4 load_quad(const float *__restrict__ row, int k, int Dz) {
    if (k + 3 < Dz) return *reinterpret_cast<const f32x4_a4 *>(row + k);
    f32x4 v;  // (the row's last quad and beyond: the last voxel repeated)
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = row[min(k + e, Dz - 1)];
    return v;
}

__device__ __forceinline__ void fetch(Staged &s, const TvArgs &a, int plane, int j0, int k0, int t) {
    const int r = t >> 4, q = t & 15;
    const long base = (long)plane * a.Dy;
    s.own = load_quad(a.vol + (base + min(j0 + r, a.Dy - 1)) * a.Dz, k0 + 4 * q, a.Dz);
    if (t < 32) {  // rows j0 - 1 and j0 + kTY
        const int j = min(max(r ? j0 + kTY : j0 - 1, 0), a.Dy - 1);
        s.ext = load_quad(a.vol + (base + j) * a.Dz, k0 + 4 * q, a.Dz);
    } else if (t >= 64 && t < 64 + 2 * (kTY + 2)) {  // columns k0 - 1 and k0 + kTZ of all rows
        const int h = t - 64;
        const int j = min(max(j0 - 1 + (h >> 1), 0), a.Dy - 1);
        const int k = min(max((h & 1) ? k0 + kTZ : k0 - 1, 0), a.Dz - 1);
        s.halo = a.vol[(base + j) * a.Dz + k];
    }
}

__device__ __forceinline__ void commit(const Staged &s, float *__restrict__ plane, int t) {
    const int r = t >> 4, q = t & 15;
    *reinterpret_cast<f32x4 *>(plane + (r + 1) * kRowF + 4 + 4 * q) = s.own;
    if (t < 32) {
        *reinterpret_cast<f32x4 *>(plane + (r ? kTY + 1 : 0) * kRowF + 4 + 4 * q) = s.ext;
    } else if (t >= 64 && t < 64 + 2 * (kTY + 2)) {
        const int h = t - 64;
        plane[(h >> 1) * kRowF + ((h & 1) ? 4 + kTZ : 3)] = s.halo;
    }
}

__device__ __forceinline__ float sgn(float d) { return (float)(d > 0.f) - (float)(d < 0.f); }

// 1 / n of a voxel with differences (dx, dy, dz) (isotropic); `n` itself where it is asked for
__device__ __forceinline__ float inv_norm(float dx, float dy, float dz, float eps2, float *n = nullptr) {
    const float n2 = fmaf(dx, dx, fmaf(dy, dy, fmaf(dz, dz, eps2)));
    const float rn = rsqrtf(n2);
    if (n) *n = n2 > 0.f ? n2 * rn : 0.f;
    return rn;
}

// MODE: DDRR_RECON_TV_*.  GRAD: 0 = value only, 1 = grad = w g, 2 = grad += w g.
template <int MODE, int GRAD>
__global__ __launch_bounds__(kTvThreads) void tv3d_kernel(const TvArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[3 * kPlaneF];
    __shared__ double wave_sum[kTvThreads / 64];
    const int t = threadIdx.x, r = t >> 4, q = t & 15;
    const int k0 = blockIdx.x * kTZ, j0 = blockIdx.y * kTY, x0 = blockIdx.z * kXC;
    const int x1 = min(x0 + kXC, a.Dx);
    const int j = j0 + r, k = k0 + 4 * q;
    const bool row_ok = j < a.Dy;
    const float isx = a.isx, isy = a.isy, isz = a.isz, eps2 = a.eps2;
    float w = 0.f;
    if (GRAD) w = a.scale ? a.weight * a.scale[0] : a.weight;
    // (the gradient of plane x0 needs px of plane x0 - 1: one step that computes nothing else)
    const int xs = (GRAD && x0 > 0) ? x0 - 1 : x0;
    Staged s;
    fetch(s, a, xs, j0, k0, t);
    commit(s, lds, t);
    fetch(s, a, min(xs + 1, a.Dx - 1), j0, k0, t);
    commit(s, lds + kPlaneF, t);
    __syncthreads();
    const int o = (r + 1) * kRowF + 4 + 4 * q;
    int c = 0;  // the buffer of plane i; plane i + 1 is in the one behind it, plane i + 2 goes to the third
    f32x4 px_prev = {0.f, 0.f, 0.f, 0.f};
    double acc = 0.0;
    for (int i = xs; i < x1; ++i) {
        const int nb = c == 2 ? 0 : c + 1, sb = nb == 2 ? 0 : nb + 1;
        const bool more = i + 1 < x1, out = i >= x0;
        if (more) fetch(s, a, min(i + 2, a.Dx - 1), j0, k0, t);
        const long at = ((long)i * a.Dy + j) * a.Dz + k;
        const bool whole = row_ok && k + 3 < a.Dz;
        f32x4 old = {0.f, 0.f, 0.f, 0.f};
        if (GRAD == 2 && out && row_ok) {
            if (whole) {
                old = *reinterpret_cast<const f32x4_a4 *>(a.grad + at);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (k + e < a.Dz) old[e] = a.grad[at + e];
            }
        }
        const float *cur = lds + c * kPlaneF, *nxt = lds + nb * kPlaneF;
        const f32x4 c0 = *reinterpret_cast<const f32x4 *>(cur + o);
        const f32x4 n0 = *reinterpret_cast<const f32x4 *>(nxt + o);
        const f32x4 cyp = *reinterpret_cast<const f32x4 *>(cur + o + kRowF);
        const float cz[5] = {c0[0], c0[1], c0[2], c0[3], cur[o + 4]};
        // (a difference past the last plane IS zero, whatever the voxel holds -- inf - inf of the clamped
        // staging would not be)
        const bool okx = i + 1 < a.Dx, oky = j + 1 < a.Dy;
        f32x4 px, py, pz;
        float val = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float dx = okx ? (n0[e] - c0[e]) * isx : 0.f, dy = oky ? (cyp[e] - c0[e]) * isy : 0.f;
            const float dz = k + e + 1 < a.Dz ? (cz[e + 1] - cz[e]) * isz : 0.f;
            float n;
            if (MODE == DDRR_RECON_TV_ISOTROPIC) {
                const float rn = inv_norm(dx, dy, dz, eps2, &n);
                px[e] = dx * rn * isx;
                py[e] = dy * rn * isy;
                pz[e] = dz * rn * isz;
            } else {
                n = fabsf(dx) + fabsf(dy) + fabsf(dz);
                px[e] = sgn(dx) * isx;
                py[e] = sgn(dy) * isy;
                pz[e] = sgn(dz) * isz;
            }
            if (row_ok && k + e < a.Dz) val += n;
        }
        if (out) acc += (double)val;
        if (GRAD && out) {
            // py of row j - 1 and pz of voxel k - 1, from the same two planes
            const f32x4 cym = *reinterpret_cast<const f32x4 *>(cur + o - kRowF);
            const float c_lo = cur[o - 1];
            f32x4 pym;
            float pz_lo;
            if (MODE == DDRR_RECON_TV_ISOTROPIC) {
                const f32x4 nym = *reinterpret_cast<const f32x4 *>(nxt + o - kRowF);
                const float mz[5] = {cym[0], cym[1], cym[2], cym[3], cur[o - kRowF + 4]};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float dy = (c0[e] - cym[e]) * isy;
                    pym[e] = dy * inv_norm(okx ? (nym[e] - cym[e]) * isx : 0.f, dy,
                                           k + e + 1 < a.Dz ? (mz[e + 1] - mz[e]) * isz : 0.f, eps2) * isy;
                }
                const float dz = (c0[0] - c_lo) * isz;
                pz_lo = dz * inv_norm(okx ? (nxt[o - 1] - c_lo) * isx : 0.f,
                                      oky ? (cur[o + kRowF - 1] - c_lo) * isy : 0.f, dz, eps2) * isz;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) pym[e] = sgn(c0[e] - cym[e]) * isy;
                pz_lo = sgn(c0[0] - c_lo) * isz;
            }
            if (j == 0) pym = f32x4{0.f, 0.f, 0.f, 0.f};  // (the terms of index -1 are absent)
            if (k == 0) pz_lo = 0.f;
            const float pzm[4] = {pz_lo, pz[0], pz[1], pz[2]};
            f32x4 res;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float g = (px_prev[e] - px[e]) + (pym[e] - py[e]) + (pzm[e] - pz[e]);
                res[e] = GRAD == 2 ? fmaf(w, g, old[e]) : w * g;
            }
            if (whole) {
                *reinterpret_cast<f32x4_a4 *>(a.grad + at) = res;
            } else if (row_ok) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (k + e < a.Dz) a.grad[at + e] = res[e];
            }
        }
        px_prev = px;
        if (more) commit(s, lds + sb * kPlaneF, t);
        __syncthreads();
        c = nb;
    }
    // the workgroup's value: lanes, then waves, in a fixed order
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
    if ((t & 63) == 0) wave_sum[t >> 6] = acc;
    __syncthreads();
    if (t == 0) {
        const long block = ((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        a.partial[block] = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
    }
}

__global__ __launch_bounds__(kSumThreads) void tv3d_sum_kernel(const double *__restrict__ partial, long n,
                                                               float *__restrict__ value) {
    __shared__ double part[kSumThreads];
    double s = 0.0;
    for (long i = threadIdx.x; i < n; i += kSumThreads) s += partial[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int half = kSumThreads / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) part[threadIdx.x] += part[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) value[0] = (float)part[0];
}

struct TvGrid {
    unsigned gx, gy, gz;
    long blocks;
};

TvGrid tv_grid(int Dx, int Dy, int Dz) {
    TvGrid g;
    g.gx = (unsigned)((Dz + kTZ - 1) / kTZ);
    g.gy = (unsigned)((Dy + kTY - 1) / kTY);
    g.gz = (unsigned)((Dx + kXC - 1) / kXC);
    g.blocks = (long)g.gx * g.gy * g.gz;
    return g;
}

int check_dims(int Dx, int Dy, int Dz) {
    if (Dx < 0 || Dy < 0 || Dz < 0) return fail(-1, "Dx, Dy, Dz must be >= 0");
    if (Dx > DDRR_RECON_MAX_DIM || Dy > DDRR_RECON_MAX_DIM || Dz > DDRR_RECON_MAX_DIM)
        return fail(-1, "Dx, Dy, Dz must be <= 65535");
    if ((long)Dx * Dy * Dz > kMaxVoxels) return fail(-1, "Dx Dy Dz must be <= 2^34");
    return 0;
}

// -------------------------------------------------------------------------------------------- Adam
constexpr int kAdamThreads = 256;
constexpr long kAdamMaxBlocks = 16384;
constexpr long kAdamMaxN = 1L << 40;

struct AdamArgs {
    float *p;
    const float *g;
    float *m, *v;
    const float *step;
    long n;
    double lr, beta1, beta2;
    float w1, b2, w2, eps, lower, upper;  // 1 - beta1, beta2, 1 - beta2 as torch hands them to its fp32 ops
    int maximize;
};

// The roundings of torch's single-tensor Adam on the device, one per line: where torch's kernels fuse a
// multiply into an add (lerp, addcmul, addcdiv) so does this, where they are separate launches (mul_, the
// division by sqrt(bias_correction2), add_(eps)) nothing is fused.  The division is a division, as in the
// multi-tensor flavour torch takes by default on the device (its single-tensor flavour multiplies by the
// float reciprocal of the host scalar: one more rounding).
__device__ __forceinline__ void adam_one(float &p, float g, float &m, float &v, const AdamArgs &a, float step_size,
                                         float bc2_sqrt) {
    g = a.maximize ? -g : g;
    m = fmaf(a.w1, g - m, m);                    // exp_avg.lerp_(grad, 1 - beta1)
    v = fmaf(a.w2, __fmul_rn(g, g), __fmul_rn(v, a.b2));  // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = __fadd_rn(__fdiv_rn(sqrtf(v), bc2_sqrt), a.eps);  // (sqrt / bc2_sqrt).add_(eps)
    p = fmaf(-step_size, __fdiv_rn(m, denom), p);  // param.addcdiv_(exp_avg, denom, value=-step_size)
    p = p < a.lower ? a.lower : p;               // (NaN stays NaN, as torch.clamp leaves it)
    p = p > a.upper ? a.upper : p;
}

template <bool VEC>
__global__ __launch_bounds__(kAdamThreads) void adam_kernel(const AdamArgs a) {
    __shared__ float shared[2];
    if (threadIdx.x == 0) {
        const double t = (double)a.step[0] + 1.0;
        shared[0] = (float)(a.lr / (1.0 - pow(a.beta1, t)));
        shared[1] = (float)sqrt(1.0 - pow(a.beta2, t));
    }
    __syncthreads();
    const float step_size = shared[0], bc2_sqrt = shared[1];
    const long stride = (long)gridDim.x * kAdamThreads;
    const long first = (long)blockIdx.x * kAdamThreads + threadIdx.x;
    if (VEC) {
        const long quads = a.n >> 2;
        for (long i = first; i < quads; i += stride) {
            f32x4 p = reinterpret_cast<const f32x4 *>(a.p)[i];
            const f32x4 g = reinterpret_cast<const f32x4 *>(a.g)[i];
            f32x4 m = reinterpret_cast<const f32x4 *>(a.m)[i];
            f32x4 v = reinterpret_cast<const f32x4 *>(a.v)[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pe = p[e], me = m[e], ve = v[e];
                adam_one(pe, g[e], me, ve, a, step_size, bc2_sqrt);
                p[e] = pe, m[e] = me, v[e] = ve;
            }
            reinterpret_cast<f32x4 *>(a.p)[i] = p;
            reinterpret_cast<f32x4 *>(a.m)[i] = m;
            reinterpret_cast<f32x4 *>(a.v)[i] = v;
        }
        const long i = (quads << 2) + first;  // the last n % 4 elements
        if (i < a.n) adam_one(a.p[i], a.g[i], a.m[i], a.v[i], a, step_size, bc2_sqrt);
    } else {
        for (long i = first; i < a.n; i += stride) adam_one(a.p[i], a.g[i], a.m[i], a.v[i], a, step_size, bc2_sqrt);
    }
}

__global__ void adam_count_kernel(float *step) { step[0] += 1.f; }

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

}  // namespace

extern "C" {

int ddrr_recon_abi_version(void) { return DDRR_RECON_ABI_VERSION; }
const char *ddrr_recon_last_error(void) { return g_err; }

long ddrr_recon_tv_workspace_bytes(int Dx, int Dy, int Dz) {
    if (check_dims(Dx, Dy, Dz)) return -1;
    if (Dx == 0 || Dy == 0 || Dz == 0) return 0;
    return tv_grid(Dx, Dy, Dz).blocks * (long)sizeof(double);
}

int ddrr_recon_tv3d(const float *volume, int Dx, int Dy, int Dz, float sx, float sy, float sz, int mode,
                    float eps, float *grad, int accumulate, float weight, const float *scale, void *workspace,
                    long workspace_bytes, float *value, void *stream) {
    if (!volume) return fail(-1, "null volume pointer");
    if (!workspace) return fail(-1, "null workspace pointer");
    if (!value) return fail(-1, "null value pointer");
    if (int rc = check_dims(Dx, Dy, Dz)) return rc;
    if (!(sx > 0.f && sy > 0.f && sz > 0.f) || !isfinite(sx) || !isfinite(sy) || !isfinite(sz))
        return fail(-1, "sx, sy, sz must be > 0 and finite");
    if (mode != DDRR_RECON_TV_ISOTROPIC && mode != DDRR_RECON_TV_ANISOTROPIC)
        return fail(-1, "mode must be DDRR_RECON_TV_ISOTROPIC or DDRR_RECON_TV_ANISOTROPIC");
    if (!(eps >= 0.f) || !isfinite(eps)) return fail(-1, "eps must be >= 0 and finite");
    if (grad && !isfinite(weight)) return fail(-1, "weight must be finite");
    if (!aligned4(volume) || !aligned4(grad) || !aligned4(scale) || !aligned4(value))
        return fail(-1, "volume, grad, scale and value must be 4-byte aligned");
    if (!aligned16(workspace)) return fail(-1, "workspace must be 16-byte aligned");
    const long voxels = (long)Dx * Dy * Dz;
    if (grad) {
        const uintptr_t v0 = reinterpret_cast<uintptr_t>(volume), g0 = reinterpret_cast<uintptr_t>(grad);
        const uintptr_t bytes = (uintptr_t)voxels * sizeof(float);
        if (v0 < g0 + bytes && g0 < v0 + bytes) return fail(-1, "grad must not overlap volume");
    }
    if (voxels == 0) return 0;
    const TvGrid g = tv_grid(Dx, Dy, Dz);
    if (workspace_bytes < g.blocks * (long)sizeof(double))
        return fail(-1, "workspace_bytes is smaller than ddrr_recon_tv_workspace_bytes()");
    TvArgs a;
    a.vol = volume;
    a.grad = grad;
    a.scale = scale;
    a.partial = static_cast<double *>(workspace);
    a.Dx = Dx, a.Dy = Dy, a.Dz = Dz;
    a.isx = 1.f / sx, a.isy = 1.f / sy, a.isz = 1.f / sz;
    a.eps2 = eps * eps;
    a.weight = weight;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(g.gx, g.gy, g.gz), block(kTvThreads);
    const int form = grad ? (accumulate ? 2 : 1) : 0;
#define DDRR_RECON_TV(MODE_, GRAD_) hipLaunchKernelGGL((tv3d_kernel<MODE_, GRAD_>), grid, block, 0, s, a)
    if (mode == DDRR_RECON_TV_ISOTROPIC) {
        if (form == 0) DDRR_RECON_TV(DDRR_RECON_TV_ISOTROPIC, 0);
        else if (form == 1) DDRR_RECON_TV(DDRR_RECON_TV_ISOTROPIC, 1);
        else DDRR_RECON_TV(DDRR_RECON_TV_ISOTROPIC, 2);
    } else {
        if (form == 0) DDRR_RECON_TV(DDRR_RECON_TV_ANISOTROPIC, 0);
        else if (form == 1) DDRR_RECON_TV(DDRR_RECON_TV_ANISOTROPIC, 1);
        else DDRR_RECON_TV(DDRR_RECON_TV_ANISOTROPIC, 2);
    }
#undef DDRR_RECON_TV
    if (int rc = finish("ddrr_recon_tv3d (tiles)")) return rc;
    hipLaunchKernelGGL(tv3d_sum_kernel, dim3(1), dim3(kSumThreads), 0, s, a.partial, g.blocks, value);
    return finish("ddrr_recon_tv3d (sum)");
}

int ddrr_recon_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float *step, long n,
                         double lr, double beta1, double beta2, double eps, float lower, float upper, int maximize,
                         void *stream) {
    if (!param) return fail(-1, "null param pointer");
    if (!grad) return fail(-1, "null grad pointer");
    if (!exp_avg) return fail(-1, "null exp_avg pointer");
    if (!exp_avg_sq) return fail(-1, "null exp_avg_sq pointer");
    if (!step) return fail(-1, "null step pointer");
    if (n < 0 || n > kAdamMaxN) return fail(-1, "n must be in [0, 2^40]");
    if (!(lr >= 0.0) || !isfinite(lr)) return fail(-1, "lr must be >= 0 and finite");
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return fail(-1, "beta1, beta2 must be in [0, 1)");
    if (!(eps >= 0.0) || !isfinite(eps)) return fail(-1, "eps must be >= 0 and finite");
    if (!(lower <= upper)) return fail(-1, "lower must be <= upper (and neither NaN)");
    if (!aligned4(param) || !aligned4(grad) || !aligned4(exp_avg) || !aligned4(exp_avg_sq) || !aligned4(step))
        return fail(-1, "param, grad, exp_avg, exp_avg_sq and step must be 4-byte aligned");
    if (n == 0) return 0;
    AdamArgs a;
    a.p = param, a.g = grad, a.m = exp_avg, a.v = exp_avg_sq, a.step = step, a.n = n;
    a.lr = lr, a.beta1 = beta1, a.beta2 = beta2;
    a.w1 = (float)(1.0 - beta1), a.b2 = (float)beta2, a.w2 = (float)(1.0 - beta2), a.eps = (float)eps;
    a.lower = lower, a.upper = upper, a.maximize = maximize ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = aligned16(param) && aligned16(grad) && aligned16(exp_avg) && aligned16(exp_avg_sq);
    const long items = vec ? (n + 3) / 4 : n;
    long blocks = (items + kAdamThreads - 1) / kAdamThreads;
    if (blocks > kAdamMaxBlocks) blocks = kAdamMaxBlocks;
    if (vec) hipLaunchKernelGGL(adam_kernel<true>, dim3((unsigned)blocks), dim3(kAdamThreads), 0, s, a);
    else hipLaunchKernelGGL(adam_kernel<false>, dim3((unsigned)blocks), dim3(kAdamThreads), 0, s, a);
    if (int rc = finish("ddrr_recon_adam_step (update)")) return rc;
    hipLaunchKernelGGL(adam_count_kernel, dim3(1), dim3(1), 0, s, step);
    return finish("ddrr_recon_adam_step (count)");
}

}  // extern "C"
