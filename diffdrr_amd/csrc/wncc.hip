// wncc.hip -- the weighted (masked) NCC of image pairs and the two epilogues of a registration step with a
// per-pixel weight: the C ABI of include/diffdrr_wncc_hip.h (libdiffdrr_wncc_hip.so).  The arithmetic is
// wncc_core.h's (and through it siddon_core.h's, raygen_core.h's and record_layout.h's); what is here is who
// computes what.
//
//   moments_kernel<RECORD>   one workgroup per (pair, run of 1024 pixels), four pixels per thread: one 16-byte
//       load each of the fixed image, the weight and the moving image -- RECORD: the rays' lengths and plane 0 of
//       the blocked record, whose product is the image (optionally written) -- where the rows allow it, four
//       scalar loads each otherwise; everything a thread reads is requested before its first pixel is summed.
//       Six double moments per thread, wave butterflies, the four waves through LDS in wave order, one partial
//       (six doubles) per workgroup into the caller's workspace.
//   fold_moments_kernel      a thread per (pair, moment) adds the pair's partials in workgroup order; one thread
//       per pair finishes the statistics (wncc_core.h finalize).  With a batch sum wanted the launch is ONE
//       workgroup that walks the pairs 32 at a time and adds their values in pair order.
//   pixel_backward_kernel    the image entries' gradient, one pixel per thread.
//   siddon_backward_kernel   one workgroup per (pose, run of 1024 rays), four rays per thread, all of a thread's
//       loads (five record planes, fixed pixel, weight, detector point) requested before the first ray is worked
//       on, as in siddon_ncc_bwd_pose_kernel; twelve float sums per thread, butterflies, LDS, one partial
//       (twelve floats) per workgroup.
//   fold_pose_kernel         a thread per (pose, matrix entry) adds the partials in workgroup order; one thread
//       per pose runs pose_euler_backward.
// No atomics and no tickets: a fold is a launch of its own, so the partials it reads are complete and visible,
// and the results are bitwise reproducible.  One launch shape whatever the batch (no variant by launch size).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "wncc_core.h"

namespace {

using namespace ddrr_wncc;

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

constexpr int kWaves = kBlock / 64;

__device__ __forceinline__ bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <bool RECORD>
__global__ __launch_bounds__(kBlock) void moments_kernel(
    const float *__restrict__ aux, const float *__restrict__ x2, const float *__restrict__ x1, long x1_stride,
    const float *__restrict__ w, long w_stride, int N, double *__restrict__ ws, float *__restrict__ out) {
    __shared__ double red[kMoments][kWaves];
    const int b = blockIdx.y;
    const float *p1 = x1 + b * x1_stride, *pw = w + b * w_stride, *p2 = x2 + (long)b * N;
    const long r0 = (long)b * N;
    const int n0 = blockIdx.x * kGroupRays, n_end = min(N, n0 + kGroupRays);
    double m[kMoments] = {0., 0., 0., 0., 0., 0.};
    // (plane 0 of rays 4 k .. 4 k + 3 is one aligned 16-byte run of the blocked record, record_layout.h)
    const bool vec = (N & 3) == 0 && aligned16(p1) && aligned16(pw) && aligned16(p2) && (!RECORD || aligned16(aux)) &&
                     (!out || aligned16(out));
    if (vec) {
        const int nq = n0 + 4 * (int)threadIdx.x;
        const bool in = nq < n_end;
        const int n = in ? nq : n0;  // (a quad beyond the run re-reads the first, unused)
        float4 I4 = make_float4(1.f, 1.f, 1.f, 1.f);
        if constexpr (RECORD) I4 = *reinterpret_cast<const float4 *>(aux + ddrr::rec_index(r0 + n, 0));
        const float4 L4 = *reinterpret_cast<const float4 *>(p2 + n);
        const float4 a4 = *reinterpret_cast<const float4 *>(p1 + n);
        const float4 w4 = *reinterpret_cast<const float4 *>(pw + n);
        if (in) {
            float4 c4 = L4;
            if constexpr (RECORD) c4 = make_float4(L4.x * I4.x, L4.y * I4.y, L4.z * I4.z, L4.w * I4.w);
            if (out) *reinterpret_cast<float4 *>(out + r0 + nq) = c4;
            moments_take(m, w4.x, a4.x, c4.x);
            moments_take(m, w4.y, a4.y, c4.y);
            moments_take(m, w4.z, a4.z, c4.z);
            moments_take(m, w4.w, a4.w, c4.w);
        }
    } else {
        float I[kPer], L[kPer], a[kPer], ww[kPer];
        bool in[kPer];
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const int nk = n0 + (int)threadIdx.x + k * kBlock;
            in[k] = nk < n_end;
            const int n = in[k] ? nk : n_end - 1;  // (a pixel beyond the run re-reads the last one, unused)
            I[k] = RECORD ? aux[ddrr::rec_index(r0 + n, 0)] : 1.f;
            L[k] = p2[n];
            a[k] = p1[n];
            ww[k] = pw[n];
        }
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            if (!in[k]) continue;
            const float c = RECORD ? L[k] * I[k] : L[k];  // (= siddon_out_from_record_kernel)
            if (out) out[r0 + n0 + (int)threadIdx.x + k * kBlock] = c;
            moments_take(m, ww[k], a[k], c);
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < kMoments; ++k) {
        double v = m[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) red[k][wave] = v;
    }
    __syncthreads();
    if (threadIdx.x < kMoments) {
        double v = red[threadIdx.x][0];
#pragma unroll
        for (int k = 1; k < kWaves; ++k) v += red[threadIdx.x][k];
        ws[((long)b * gridDim.x + blockIdx.x) * kMoments + threadIdx.x] = v;
    }
}

constexpr int kFoldPairs = kBlock / 8;  // pairs of a pass of fold_moments_kernel: eight threads each, six used

__global__ __launch_bounds__(kBlock) void fold_moments_kernel(const double *__restrict__ ws, int B, int G, float eps,
                                                              float *__restrict__ ncc, float *__restrict__ stats,
                                                              float *__restrict__ ncc_sum) {
    __shared__ double S[kFoldPairs][8];
    __shared__ float vals[kFoldPairs];
    const int p = threadIdx.x >> 3, k = threadIdx.x & 7;
    double total = 0.0;  // (thread 0's, with ncc_sum: the launch is then one workgroup)
    for (int base = blockIdx.x * kFoldPairs; base < B; base += gridDim.x * kFoldPairs) {
        const int b = base + p;
        if (b < B && k < kMoments) {
            const double *q = ws + (long)b * G * kMoments + k;
            double v = q[0];
            for (int g = 1; g < G; ++g) v += q[(long)g * kMoments];
            S[p][k] = v;
        }
        __syncthreads();
        if (b < B && k == 0) {
            float st[kStats];
            finalize(S[p], eps, st);
#pragma unroll
            for (int e = 0; e < kStats; ++e) stats[b * kStats + e] = st[e];
            ncc[b] = st[4];
            vals[p] = st[4];
        }
        __syncthreads();
        if (ncc_sum && threadIdx.x == 0) {
            const int count = min(kFoldPairs, B - base);
            for (int e = 0; e < count; ++e) total += (double)vals[e];
        }
    }
    if (ncc_sum && threadIdx.x == 0 && blockIdx.x == 0) *ncc_sum = (float)total;
}

__global__ __launch_bounds__(kBlock) void pixel_backward_kernel(
    const float *__restrict__ x1, long x1_stride, const float *__restrict__ x2, const float *__restrict__ w,
    long w_stride, const float *__restrict__ stats, const float *__restrict__ g_out, int g_stride, int N,
    float *__restrict__ g_x1, float *__restrict__ g_x2) {
    const int b = blockIdx.y, n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= N) return;
    const float *st = stats + b * kStats;
    const float gn = grad_scale(g_out[b * g_stride], st[5]);
    const float a = x1[b * x1_stride + n], c = x2[(long)b * N + n], wn = w[b * w_stride + n];
    if (g_x2) g_x2[(long)b * N + n] = grad_pixel(gn, wn, a, st[0], st[1], c, st[2], st[3], st[4]);
    if (g_x1) g_x1[(long)b * N + n] = grad_pixel(gn, wn, c, st[2], st[3], a, st[0], st[1], st[4]);
}

__global__ __launch_bounds__(kBlock) void siddon_backward_kernel(
    const float *__restrict__ aux, const float *__restrict__ x1, long x1_stride, const float *__restrict__ w,
    long w_stride, const float *__restrict__ stats, const float *__restrict__ g_out, int g_stride,
    const float *__restrict__ source_v, const float *__restrict__ Mw, const float *__restrict__ Ainv,
    const float *__restrict__ P, int N, float eps, int with_img_path, float *__restrict__ ws) {
    __shared__ float red[kWaves][kGrad];
    const int b = blockIdx.y;
    const float *M = Mw + (long)b * 12;
    const float s[3] = {source_v[b * 3], source_v[b * 3 + 1], source_v[b * 3 + 2]};
    float st[kStats];
#pragma unroll
    for (int e = 0; e < kStats; ++e) st[e] = stats[b * kStats + e];
    const float gn = grad_scale(g_out[b * g_stride], st[5]);
    float acc[kGrad];
#pragma unroll
    for (int k = 0; k < kGrad; ++k) acc[k] = 0.f;
    const int n_end = min(N, (int)(blockIdx.x + 1) * kGroupRays);
    // (a ray's voxel-space target and length are regenerated from the pose's matrix and the detector point by
    // the function that wrote them, raygen_core.h raygen_ray, as in siddon_ncc_bwd_pose_kernel)
    float rec[kPer][ddrr::SIDDON_AUX], x1s[kPer], wts[kPer], Ps[kPer][3];
    bool in[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int n0 = blockIdx.x * kGroupRays + threadIdx.x + k * kBlock;
        in[k] = n0 < n_end;
        const int n = in[k] ? n0 : n_end - 1;  // (a ray beyond the image re-reads the last one with weight 0)
        ddrr::rec_blocked_load(aux, (long)b * N + n, rec[k]);
        x1s[k] = x1[b * x1_stride + n];
        wts[k] = w[b * w_stride + n];
#pragma unroll
        for (int a = 0; a < 3; ++a) Ps[k][a] = P[n * 3 + a];
    }
#pragma unroll
    for (int k = 0; k < kPer; ++k)
        ray_backward(rec[k], s, M, Ainv, Ps[k], wts[k], x1s[k], st, gn, eps, with_img_path, in[k], acc);
#pragma unroll
    for (int k = 0; k < kGrad; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o, 64);
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kGrad; ++k) red[wave][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < kGrad) {
        float v = red[0][threadIdx.x];
#pragma unroll
        for (int k = 1; k < kWaves; ++k) v += red[k][threadIdx.x];
        ws[((long)b * gridDim.x + blockIdx.x) * kGrad + threadIdx.x] = v;
    }
}

constexpr int kFoldPoses = kBlock / 16;  // poses of a workgroup of fold_pose_kernel: sixteen threads each, twelve used

__global__ __launch_bounds__(kBlock) void fold_pose_kernel(const float *__restrict__ ws, const float *__restrict__ rot,
                                                           const float *__restrict__ xyz, int a0, int a1, int a2,
                                                           const float *__restrict__ Ro, int B, int G,
                                                           float *__restrict__ g_rot, float *__restrict__ g_xyz) {
    __shared__ float S[kFoldPoses][16];
    const int p = threadIdx.x >> 4, k = threadIdx.x & 15;
    const int b = blockIdx.x * kFoldPoses + p;
    if (b < B && k < kGrad) {
        const float *q = ws + (long)b * G * kGrad + k;
        float v = q[0];
        for (int g = 1; g < G; ++g) v += q[(long)g * kGrad];
        S[p][k] = v;
    }
    __syncthreads();
    if (b >= B || k != 0) return;
    float g[kGrad], gth[3], gx[3];
#pragma unroll
    for (int e = 0; e < kGrad; ++e) g[e] = S[p][e];
    const float th[3] = {rot[b * 3], rot[b * 3 + 1], rot[b * 3 + 2]};
    const float tr[3] = {xyz[b * 3], xyz[b * 3 + 1], xyz[b * 3 + 2]};
    const int axes[3] = {a0, a1, a2};
    ddrr::pose_euler_backward(th, tr, axes, Ro, g, gth, gx);
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        g_rot[b * 3 + e] = gth[e];
        g_xyz[b * 3 + e] = gx[e];
    }
}

template <bool RECORD>
int forward(const char *where, const float *aux, const float *x2, const float *x1, long x1_stride, const float *w,
            long w_stride, int B, int N, float eps, void *ws, float *ncc, float *stats, float *out, float *ncc_sum,
            void *stream) {
    if ((RECORD && !aux) || !x2 || !x1 || !w || !ws || !ncc || !stats) return fail(-1, "null pointer");
    if (const char *m = check_sizes(B, N)) return fail(-1, m);
    if (const char *m = check_rows(x1_stride, w_stride, N)) return fail(-1, m);
    if (const char *m = check_eps(eps)) return fail(-1, m);
    if (const char *m = check_ws(ws)) return fail(-1, m);
    if (B == 0) return 0;
    const int G = groups_of(N);
    hipLaunchKernelGGL(moments_kernel<RECORD>, dim3(G, B), dim3(kBlock), 0, (hipStream_t)stream, aux, x2, x1,
                       x1_stride, w, w_stride, N, reinterpret_cast<double *>(ws), out);
    if (int rc = finish(where)) return rc;
    const int blocks = ncc_sum ? 1 : (B + kFoldPairs - 1) / kFoldPairs;
    hipLaunchKernelGGL(fold_moments_kernel, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream,
                       reinterpret_cast<const double *>(ws), B, G, eps, ncc, stats, ncc_sum);
    return finish(where);
}

}  // namespace

extern "C" {

int ddrr_wncc_abi_version(void) { return DDRR_WNCC_ABI_VERSION; }
const char *ddrr_wncc_last_error(void) { return g_err; }

long ddrr_wncc_workspace_bytes(int B, int N) {
    return (B < 1 || N < 1) ? 0 : (long)B * groups_of(N) * DDRR_WNCC_SLOT_BYTES;
}

int ddrr_wncc_forward(const float *x1, long x1_stride, const float *x2, const float *w, long w_stride, int B,
                      int N, float eps, void *ws, float *ncc, float *stats, void *stream) {
    return forward<false>("ddrr_wncc_forward", nullptr, x2, x1, x1_stride, w, w_stride, B, N, eps, ws, ncc, stats,
                          nullptr, nullptr, stream);
}

int ddrr_wncc_backward(const float *x1, long x1_stride, const float *x2, const float *w, long w_stride,
                       const float *stats, const float *g_out, int g_stride, int B, int N, float *g_x1,
                       float *g_x2, void *stream) {
    if (!x1 || !x2 || !w || !stats || !g_out) return fail(-1, "null pointer");
    if (const char *m = check_sizes(B, N)) return fail(-1, m);
    if (const char *m = check_rows(x1_stride, w_stride, N)) return fail(-1, m);
    if (const char *m = check_g_stride(g_stride)) return fail(-1, m);
    if (g_x1 && x1_stride == 0) return fail(-1, "a shared x1 gets no gradient here");
    if (B == 0) return 0;
    hipLaunchKernelGGL(pixel_backward_kernel, dim3((N + kBlock - 1) / kBlock, B), dim3(kBlock), 0,
                       (hipStream_t)stream, x1, x1_stride, x2, w, w_stride, stats, g_out, g_stride, N, g_x1, g_x2);
    return finish("ddrr_wncc_backward");
}

int ddrr_wncc_siddon_forward(const float *aux, const float *img, const float *x1, long x1_stride,
                             const float *w, long w_stride, int B, int N, float eps, void *ws, float *ncc,
                             float *stats, float *out, float *ncc_sum, void *stream) {
    return forward<true>("ddrr_wncc_siddon_forward", aux, img, x1, x1_stride, w, w_stride, B, N, eps, ws, ncc,
                         stats, out, ncc_sum, stream);
}

int ddrr_wncc_siddon_backward_pose(const float *aux, const float *x1, long x1_stride, const float *w,
                                   long w_stride, const float *stats, const float *g_out, int g_stride,
                                   const float *source_v, const float *Mw, const float *Ainv, const float *P,
                                   const float *rot, const float *xyz, int a0, int a1, int a2,
                                   const float *reorient34, int B, int N, float eps, int with_img_path,
                                   void *ws, float *g_rot, float *g_xyz, void *stream) {
    if (!aux || !x1 || !w || !stats || !g_out || !source_v || !Mw || !Ainv || !P || !rot || !xyz || !reorient34 ||
        !ws || !g_rot || !g_xyz)
        return fail(-1, "null pointer");
    if (const char *m = check_axes(a0, a1, a2)) return fail(-1, m);
    if (const char *m = check_sizes(B, N)) return fail(-1, m);
    if (const char *m = check_rows(x1_stride, w_stride, N)) return fail(-1, m);
    if (const char *m = check_g_stride(g_stride)) return fail(-1, m);
    if (const char *m = check_eps(eps)) return fail(-1, m);
    if (const char *m = check_ws(ws)) return fail(-1, m);
    if (B == 0) return 0;
    const int G = groups_of(N);
    hipLaunchKernelGGL(siddon_backward_kernel, dim3(G, B), dim3(kBlock), 0, (hipStream_t)stream, aux, x1, x1_stride,
                       w, w_stride, stats, g_out, g_stride, source_v, Mw, Ainv, P, N, eps, with_img_path ? 1 : 0,
                       reinterpret_cast<float *>(ws));
    if (int rc = finish("ddrr_wncc_siddon_backward_pose")) return rc;
    hipLaunchKernelGGL(fold_pose_kernel, dim3((B + kFoldPoses - 1) / kFoldPoses), dim3(kBlock), 0,
                       (hipStream_t)stream, reinterpret_cast<const float *>(ws), rot, xyz, a0, a1, a2, reorient34, B,
                       G, g_rot, g_xyz);
    return finish("ddrr_wncc_siddon_backward_pose");
}

}  // extern "C"
