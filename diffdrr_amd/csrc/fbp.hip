// fbp.hip -- the two passes of an FDK start as gfx950 kernels: the C ABI of include/diffdrr_fbp_hip.h
// (libdiffdrr_fbp_hip.so).  The arithmetic is fbp_core.h's; what is here is who computes what.
//
//   filter_kernel<AXIS>   one workgroup per image line (a row, or a column for AXIS 1): the line, cosine
//       weighted, and the 2 L - 1 taps go to LDS once ((3 L - 1) floats, 48 KB at L = 4096); every
//       thread then owns outputs n = t, t + 256, ... and sums its L products in ascending k, in double.
//       A wave reads one line element (a broadcast) and 64 consecutive taps per step: no bank conflict.
//   backproject_kernel    voxel driven: a workgroup owns a (4, 4, 64) tile of voxels -- a wave one x
//       plane of it, a lane four consecutive z voxels of one row -- and walks the views in ascending
//       order with the four sums in registers; the volume is written once, 16 bytes per lane, 256-byte
//       runs per row.  A view's matrix and weight are wave-uniform (scalar loads); the pixels are
//       gathered through L1 / L2: a tile's shadow on the detector is a few pixels wide, and every
//       workgroup is on the same view's image at about the same time.
// No atomics anywhere: the results are bitwise reproducible.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/diffdrr_fbp_hip.h"
#include "fbp_core.h"

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

bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

bool overlap(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a_bytes && b_bytes && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

int check_images(int B, int H, int W) {
    if (B < 0 || H < 0 || W < 0) return fail(-1, "B, H, W must be >= 0");
    if (H > DDRR_FBP_MAX_IMAGE_DIM || W > DDRR_FBP_MAX_IMAGE_DIM) return fail(-1, "H, W must be <= 4096");
    return 0;
}

// ------------------------------------------------------------------------------------------ filter
constexpr int kFilterThreads = 256;
constexpr long kFilterMaxBlocks = 1L << 20;
constexpr long kFilterMaxPixels = 1L << 31;

struct FilterArgs {
    const float *images, *taps;
    float *out;
    long lines;
    int H, W;
    float scale, u0, du, v0, dv, sdd;
    int cosine_weight;
};

// AXIS 0: line = (b, row), elements along the columns.  AXIS 1: line = (b, column), elements along the rows.
template <int AXIS>
__global__ __launch_bounds__(kFilterThreads) void filter_kernel(const FilterArgs a) {
    extern __shared__ float lds[];
    const int L = AXIS == 0 ? a.W : a.H, across = AXIS == 0 ? a.H : a.W;
    float *line = lds, *taps = lds + L;
    const int t = threadIdx.x;
    for (int n = t; n < 2 * L - 1; n += kFilterThreads) taps[n] = a.taps[n];
    for (long id = blockIdx.x; id < a.lines; id += gridDim.x) {
        const long b = id / across;
        const int at = (int)(id - b * across);
        const long first = AXIS == 0 ? (b * a.H + at) * a.W : b * a.H * a.W + at;
        const long step = AXIS == 0 ? 1 : a.W;
        __syncthreads();  // (the line of the last round has been read; the taps are there)
        for (int k = t; k < L; k += kFilterThreads)
            line[k] = fbp::weighted_pixel(a.images[first + k * step], AXIS == 0 ? at : k, AXIS == 0 ? k : at,
                                          a.u0, a.du, a.v0, a.dv, a.sdd, a.cosine_weight);
        __syncthreads();
        for (int n = t; n < L; n += kFilterThreads) a.out[first + n * step] = fbp::convolve(line, taps, L, n, a.scale);
    }
}

// ---------------------------------------------------------------------------------- backprojection
constexpr int kBpThreads = 256;
constexpr int kBpZ = 64, kBpY = 4, kBpX = 4;  // the tile: 16 lanes x 4 voxels along z, 4 rows, 4 planes (waves)
constexpr long kMaxVoxels = 1L << 34;

struct BpArgs {
    const float *images, *views;
    float *volume;
    int B, H, W, Dx, Dy, Dz;
    int distance_weight, accumulate;
};

__global__ __launch_bounds__(kBpThreads) void backproject_kernel(const BpArgs a) {
    const int t = threadIdx.x;
    const int k = blockIdx.x * kBpZ + 4 * (t & 15);
    const int j = blockIdx.y * kBpY + ((t >> 4) & 3);
    const int i = blockIdx.z * kBpX + (t >> 6);
    if (i >= a.Dx || j >= a.Dy || k >= a.Dz) return;
    const int count = min(4, a.Dz - k);
    const long pixels = (long)a.H * a.W;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int b = 0; b < a.B; ++b) {
        const float *__restrict__ view = a.views + (long)b * DDRR_FBP_VIEW_FLOATS;
        const float *__restrict__ img = a.images + b * pixels;
        const fbp::Row p = fbp::row_of(view, i, j);
#pragma unroll
        for (int e = 0; e < 4; ++e)  // (past the row's end: the last voxel again, not stored)
            acc[e] = fbp::accumulate_view(acc[e], img, a.H, a.W, view, p, min(k + e, a.Dz - 1), a.distance_weight);
    }
    float *__restrict__ dst = a.volume + (((long)i * a.Dy + j) * a.Dz + k);
    if (count == 4) {
        f32x4 res = {acc[0], acc[1], acc[2], acc[3]};
        if (a.accumulate) res += *reinterpret_cast<const f32x4_a4 *>(dst);
        *reinterpret_cast<f32x4_a4 *>(dst) = res;
    } else {
#pragma unroll
        for (int e = 0; e < 3; ++e)
            if (e < count) dst[e] = a.accumulate ? dst[e] + acc[e] : acc[e];
    }
}

}  // namespace

extern "C" {

int ddrr_fbp_abi_version(void) { return DDRR_FBP_ABI_VERSION; }
const char *ddrr_fbp_last_error(void) { return g_err; }

int ddrr_fbp_filter(const float *images, int B, int H, int W, int axis, const float *taps, float scale,
                    float u0, float du, float v0, float dv, float sdd, int cosine_weight, float *out,
                    void *stream) {
    if (!images) return fail(-1, "null images pointer");
    if (!taps) return fail(-1, "null taps pointer");
    if (!out) return fail(-1, "null out pointer");
    if (int rc = check_images(B, H, W)) return rc;
    const long n = (long)B * H * W;
    if (n > kFilterMaxPixels) return fail(-1, "B H W must be <= 2^31");
    if (axis != 0 && axis != 1) return fail(-1, "axis must be 0 (along columns) or 1 (along rows)");
    if (!isfinite(scale)) return fail(-1, "scale must be finite");
    if (cosine_weight && !(isfinite(u0) && isfinite(du) && isfinite(v0) && isfinite(dv) && isfinite(sdd) && sdd > 0.f))
        return fail(-1, "u0, du, v0, dv must be finite and sdd > 0 and finite");
    if (!aligned4(images) || !aligned4(taps) || !aligned4(out))
        return fail(-1, "images, taps and out must be 4-byte aligned");
    if (overlap(images, (uint64_t)n * sizeof(float), out, (uint64_t)n * sizeof(float)))
        return fail(-1, "out must not overlap images");
    if (n == 0) return 0;
    FilterArgs a;
    a.images = images, a.taps = taps, a.out = out;
    a.H = H, a.W = W;
    a.lines = (long)B * (axis == 0 ? H : W);
    a.scale = scale, a.u0 = u0, a.du = du, a.v0 = v0, a.dv = dv, a.sdd = sdd;
    a.cosine_weight = cosine_weight ? 1 : 0;
    const int L = axis == 0 ? W : H;
    const size_t lds = (size_t)(3 * L - 1) * sizeof(float);
    const dim3 grid((unsigned)(a.lines < kFilterMaxBlocks ? a.lines : kFilterMaxBlocks)), block(kFilterThreads);
    hipStream_t s = (hipStream_t)stream;
    if (axis == 0) hipLaunchKernelGGL(filter_kernel<0>, grid, block, lds, s, a);
    else hipLaunchKernelGGL(filter_kernel<1>, grid, block, lds, s, a);
    return finish("ddrr_fbp_filter");
}

int ddrr_fbp_backproject(const float *images, int B, int H, int W, const float *views, int distance_weight,
                         float *volume, int Dx, int Dy, int Dz, int accumulate, void *stream) {
    if (!images) return fail(-1, "null images pointer");
    if (!views) return fail(-1, "null views pointer");
    if (!volume) return fail(-1, "null volume pointer");
    if (int rc = check_images(B, H, W)) return rc;
    if (B > DDRR_FBP_MAX_VIEWS) return fail(-1, "B must be <= 65535");
    if (Dx < 0 || Dy < 0 || Dz < 0) return fail(-1, "Dx, Dy, Dz must be >= 0");
    if (Dx > DDRR_FBP_MAX_DIM || Dy > DDRR_FBP_MAX_DIM || Dz > DDRR_FBP_MAX_DIM)
        return fail(-1, "Dx, Dy, Dz must be <= 65535");
    const long voxels = (long)Dx * Dy * Dz;
    if (voxels > kMaxVoxels) return fail(-1, "Dx Dy Dz must be <= 2^34");
    if (!aligned4(images) || !aligned4(views) || !aligned4(volume))
        return fail(-1, "images, views and volume must be 4-byte aligned");
    if (overlap(images, (uint64_t)B * H * W * sizeof(float), volume, (uint64_t)voxels * sizeof(float)))
        return fail(-1, "volume must not overlap images");
    if (voxels == 0) return 0;
    BpArgs a;
    a.images = images, a.views = views, a.volume = volume;
    a.B = (H == 0 || W == 0) ? 0 : B;  // (empty images: a sum of nothing)
    a.H = H, a.W = W, a.Dx = Dx, a.Dy = Dy, a.Dz = Dz;
    a.distance_weight = distance_weight ? 1 : 0, a.accumulate = accumulate ? 1 : 0;
    if (a.B == 0 && a.accumulate) return 0;
    const dim3 grid((unsigned)((Dz + kBpZ - 1) / kBpZ), (unsigned)((Dy + kBpY - 1) / kBpY),
                    (unsigned)((Dx + kBpX - 1) / kBpX)), block(kBpThreads);
    hipLaunchKernelGGL(backproject_kernel, grid, block, 0, (hipStream_t)stream, a);
    return finish("ddrr_fbp_backproject");
}

}  // extern "C"
