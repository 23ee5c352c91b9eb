// wmvlm.hip -- the three kernels of a multi-view Levenberg-Marquardt registration step with a pixel weight and a
// detector per view, around the renderer: the C ABI of include/diffdrr_wmvlm_hip.h (libdiffdrr_wmvlm_hip.so).  The
// arithmetic is lm_core.h's, wlm_core.h's, raygen_core.h's, siddon_core.h's and record_layout.h's, with
// wmvlm_core.h's sum over the non-empty views; what is here is who computes what.
// Rendered pose b = s * V + v: start s = b / V owns the parameters; view v = b % V the reorient, the fixed image,
// the weight (w + v * w_stride) and the detector points (P + v * P_stride).
//
//   wmv_raygen_kernel        mvlm.hip's mv_raygen_kernel with the view's detector points: one thread per ray, every
//       workgroup works its pose's matrix out again (three sincos, 30 fma, one lane, into LDS), and all of them
//       together clear what the render behind this launch wants zeroed.
//   wmv_normal_sums_kernel   wlm.hip's wnormal_sums_kernel -- one workgroup per (pose, run of 1024 rays), four rays
//       per thread, everything a thread's rays read requested before the first is worked on, the rows (j, x, f)
//       staged in LDS with the weights in a plane of their own and the constant 1 behind them, the 45 sums taken by
//       one thread per (sum, slice) in double with nothing contracted, vector stores only -- with the fixed image,
//       the weight, the reorient, the detector points and the parameters picked per pose.  The picks are scalar (b
//       is uniform in a workgroup), so a ray costs what it costs there.
//   wmv_step_kernel          one workgroup (one wave) per START: for each view in turn 45 lanes add the pose's
//       partials in index order, lane 0 forms the view's normal equations where the view is not empty and adds them
//       to the start's (31 doubles in LDS, so that they are not held in registers across the views); then lane 0
//       takes the Sw-weighted mean, accepts or rejects, solves and writes the next trial.  Two barriers per view.
// No atomics anywhere: the results are bitwise reproducible.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   wmv_raygen_kernel        34 VGPRs, no scratch, 48 B of LDS
//   wmv_normal_sums_kernel   111 VGPRs, no scratch, 38 848 B of LDS (wlm.hip's wnormal_sums_kernel: 110, none,
//                            38 848: the view's picks cost one register, 4 waves per SIMD either way)
//   wmv_step_kernel          116 VGPRs, no scratch, 616 B of LDS (45 + 31 doubles and padding)
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "wmvlm_core.h"

namespace {

using namespace ddrr_wmvlm;

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

__global__ __launch_bounds__(kBlock) void wmv_raygen_kernel(
    const float *__restrict__ rot, const float *__restrict__ xyz, int a0, int a1, int a2,
    const float *__restrict__ reorient_v, const float *__restrict__ Ainv, const float *__restrict__ P0, long P_stride,
    int V, int N, float *__restrict__ Mw, float *__restrict__ source_v, float *__restrict__ target_v,
    float *__restrict__ img, float *__restrict__ clear, long clear_n, int *__restrict__ counter) {
    __shared__ float Ms[12];
    const int b = blockIdx.y, n = blockIdx.x * kBlock + threadIdx.x;
    const int s = b / V, v = b - s * V;
    const float *P = P0 + v * P_stride;
    // what the render behind this launch has to find zeroed (its record, its brick counter)
    if (clear) {
        const long stride = (long)gridDim.x * gridDim.y * kBlock, n4 = clear_n >> 2;
        float4 *c4 = reinterpret_cast<float4 *>(clear);
        const long first = ((long)blockIdx.y * gridDim.x + blockIdx.x) * kBlock + threadIdx.x;
        for (long i = first; i < n4; i += stride) c4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (first < (clear_n & 3)) clear[(n4 << 2) + first] = 0.f;
    }
    if (counter && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 4) counter[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        const float th[3] = {rot[s * 3], rot[s * 3 + 1], rot[s * 3 + 2]};
        const float t[3] = {xyz[s * 3], xyz[s * 3 + 1], xyz[s * 3 + 2]};
        const int axes[3] = {a0, a1, a2};
        float M[12];
        ddrr::pose_euler_forward(th, t, axes, reorient_v + v * 12, M);
#pragma unroll
        for (int k = 0; k < 12; ++k) Ms[k] = M[k];
        if (blockIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < 12; ++k) Mw[b * 12 + k] = M[k];
            const float sw[3] = {M[3], M[7], M[11]};
            float sv[3];
            ddrr::apply34(Ainv, sw, sv);
            source_v[b * 3 + 0] = sv[0];
            source_v[b * 3 + 1] = sv[1];
            source_v[b * 3 + 2] = sv[2];
        }
    }
    __syncthreads();
    if (n >= N) return;
    float M[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) M[k] = Ms[k];
    const float Pn[3] = {P[n * 3], P[n * 3 + 1], P[n * 3 + 2]};
    const ddrr::RayGenOut o = ddrr::raygen_ray(M, Ainv, Pn);
    const long r = (long)b * N + n;
    target_v[r * 3 + 0] = o.tv[0];
    target_v[r * 3 + 1] = o.tv[1];
    target_v[r * 3 + 2] = o.tv[2];
    img[r] = o.L;
}

__global__ __launch_bounds__(kBlock) void wmv_normal_sums_kernel(
    const float *__restrict__ aux, const float *__restrict__ x1, const float *__restrict__ wt, long w_stride,
    const float *__restrict__ source_v, const float *__restrict__ Mw, const float *__restrict__ Ainv,
    const float *__restrict__ P0, long P_stride, const float *__restrict__ rot, const float *__restrict__ xyz, int a0,
    int a1, int a2, const float *__restrict__ reorient_v, int V, int N, float eps, int with_img_path,
    double *__restrict__ ws, float *__restrict__ jac) {
    __shared__ __attribute__((aligned(16))) float us[kGroupRays * 8];  // (j, x, f) of the workgroup's rays
    __shared__ float wl[kGroupRays + 1];                               // their weights, then the constant 1
    __shared__ float pose[kPoseFloats];
    __shared__ double red[kSlices][kWSums];
    const int b = blockIdx.y;
    const int st = b / V, v = b - st * V;
    const float *M = Mw + (long)b * 12;
    const float *Ro = reorient_v + v * 12;
    const float *f = x1 + (long)v * N;
    const float *wv_ = wt + v * w_stride;
    const float *P = P0 + v * P_stride;
    const float s[3] = {source_v[b * 3], source_v[b * 3 + 1], source_v[b * 3 + 2]};
    const int n_end = min(N, (int)(blockIdx.x + 1) * kGroupRays);
    // (the pose's half of pose_euler_backward by one lane, before its wave requests its rays: as lm.hip)
    if (threadIdx.x == 0) {
        const float th[3] = {rot[st * 3], rot[st * 3 + 1], rot[st * 3 + 2]};
        const float tr[3] = {xyz[st * 3], xyz[st * 3 + 1], xyz[st * 3 + 2]};
        const int axes[3] = {a0, a1, a2};
        ddrr::PoseEulerAdjoint q;
        ddrr::pose_euler_adjoint_setup(th, tr, axes, Ro, q);
#pragma unroll
        for (int e = 0; e < 9; ++e) pose[e] = q.R[e];
#pragma unroll
        for (int e = 0; e < 3; ++e) pose[9 + e] = q.v[e];
#pragma unroll
        for (int e = 0; e < 27; ++e) pose[12 + e] = q.dR[e];
        wl[kGroupRays] = 1.f;
    }
    __builtin_amdgcn_sched_barrier(0);
    float rec[kPer][ddrr::SIDDON_AUX], fs[kPer], wv[kPer], Ps[kPer][3];
    bool in[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int n0 = blockIdx.x * kGroupRays + threadIdx.x + k * kBlock;
        in[k] = n0 < n_end;
        const int n = in[k] ? n0 : n_end - 1;  // (a ray beyond the image re-reads the last one, unused)
        ddrr::rec_blocked_load(aux, (long)b * N + n, rec[k]);
        fs[k] = f[n];
        wv[k] = wv_[n];
#pragma unroll
        for (int a = 0; a < 3; ++a) Ps[k][a] = P[n * 3 + a];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        float j[6], x;
        ray_jacobian(rec[k], s, M, Ainv, Ps[k], eps, with_img_path, pose, Ro, j, x);
        const int local = threadIdx.x + k * kBlock;
        if (in[k]) {
            const bool on = wv[k] != 0.f;  // (selected, not multiplied: the fixed pixel may be NaN under weight 0)
            float4 *dst = reinterpret_cast<float4 *>(us + 8 * local);
            dst[0] = on ? make_float4(j[0], j[1], j[2], j[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
            dst[1] = on ? make_float4(j[4], j[5], x, fs[k]) : make_float4(0.f, 0.f, 0.f, 0.f);
            wl[local] = wv[k];
            if (jac) {
                float *out = jac + ((long)b * N + blockIdx.x * kGroupRays + local) * 6;
#pragma unroll
                for (int p = 0; p < 6; ++p) out[p] = j[p];
            }
        }
    }
    __syncthreads();
    const int count = n_end - (int)blockIdx.x * kGroupRays;
    if (threadIdx.x < kWSums * kSlices)
        red[threadIdx.x / kWSums][threadIdx.x % kWSums] =
            wslice_sum(us, wl, wl + kGroupRays, count, threadIdx.x % kWSums, threadIdx.x / kWSums);
    __syncthreads();
    if (threadIdx.x < kWSums) {
        double t = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kSlices; ++w) t += red[w][threadIdx.x];
        ws[((long)b * gridDim.x + blockIdx.x) * kWSums + threadIdx.x] = t;
    }
}

__global__ __launch_bounds__(64) void wmv_step_kernel(const double *__restrict__ ws, double *__restrict__ state,
                                                      float *__restrict__ rot, float *__restrict__ xyz, int V,
                                                      int groups, double ncc_eps, double up, double down,
                                                      double lambda_min, double lambda_max,
                                                      float *__restrict__ ncc_out, float *__restrict__ ncc_views,
                                                      double *__restrict__ sw_views) {
    __shared__ double S[kWSums];
    __shared__ double acc[kAcc];
    const int s = blockIdx.x;
    if (threadIdx.x == 0) clear_views(acc);
    for (int v = 0; v < V; ++v) {
        const long b = (long)s * V + v;
        if (threadIdx.x < kWSums) {
            const double *p = ws + b * groups * kWSums + threadIdx.x;
            double t = p[0];
            for (int w = 1; w < groups; ++w) t += p[(long)w * kWSums];
            S[threadIdx.x] = t;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double sw_v;
            const double ncc_v = add_wview(S, ncc_eps, acc, sw_v);
            if (ncc_views) ncc_views[b] = (float)ncc_v;
            if (sw_views) sw_views[b] = sw_v;
        }
        __syncthreads();  // (S is overwritten by the next view)
    }
    if (threadIdx.x != 0) return;
    wstep_start(acc, up, down, lambda_min, lambda_max, state + (long)s * kState, rot + s * 3, xyz + s * 3,
                ncc_out + s);
}

}  // namespace

extern "C" {

int ddrr_wmvlm_abi_version(void) { return DDRR_WMVLM_ABI_VERSION; }
const char *ddrr_wmvlm_last_error(void) { return g_err; }

long ddrr_wmvlm_workspace_bytes(int S, int V, int N) {
    return (S < 1 || check_shape(S, V, N)) ? 0 : (long)S * V * groups_of(N) * kWSums * (long)sizeof(double);
}

int ddrr_wmvlm_raygen(const float *rot, const float *xyz, int a0, int a1, int a2, const float *reorient_v,
                      const float *Ainv, const float *P, long P_stride, int S, int V, int N, float *Mw,
                      float *source_v, float *target_v, float *img, float *clear, long clear_floats,
                      void *clear_launch_ws, void *stream) {
    if (const char *bad = check_raygen_args(rot, xyz, a0, a1, a2, reorient_v, Ainv, P, P_stride, S, V, N, Mw, source_v,
                                            target_v, img, clear, clear_floats, clear_launch_ws))
        return fail(-1, bad);
    if (S == 0) return 0;
    hipLaunchKernelGGL(wmv_raygen_kernel, dim3((N + kBlock - 1) / kBlock, S * V), dim3(kBlock), 0,
                       (hipStream_t)stream, rot, xyz, a0, a1, a2, reorient_v, Ainv, P, P_stride, V, N, Mw, source_v,
                       target_v, img, clear_floats > 0 ? clear : nullptr, clear_floats,
                       reinterpret_cast<int *>(clear_launch_ws));
    return finish("ddrr_wmvlm_raygen");
}

int ddrr_wmvlm_normal_sums(const float *aux, const float *x1, const float *w, long w_stride, const float *source_v,
                           const float *Mw, const float *Ainv, const float *P, long P_stride, const float *rot,
                           const float *xyz, int a0, int a1, int a2, const float *reorient_v, int S, int V, int N,
                           float eps, int with_img_path, void *ws, float *jac, void *stream) {
    if (const char *bad = check_sums_args(aux, x1, w, w_stride, source_v, Mw, Ainv, P, P_stride, rot, xyz, a0, a1, a2,
                                          reorient_v, S, V, N, ws))
        return fail(-1, bad);
    if (S == 0) return 0;
    hipLaunchKernelGGL(wmv_normal_sums_kernel, dim3(groups_of(N), S * V), dim3(kBlock), 0, (hipStream_t)stream, aux,
                       x1, w, w_stride, source_v, Mw, Ainv, P, P_stride, rot, xyz, a0, a1, a2, reorient_v, V, N, eps,
                       with_img_path ? 1 : 0, reinterpret_cast<double *>(ws), jac);
    return finish("ddrr_wmvlm_normal_sums");
}

int ddrr_wmvlm_step(const void *ws, void *state, float *rot, float *xyz, int S, int V, int N, double ncc_eps,
                    double up, double down, double lambda_min, double lambda_max, float *ncc_out,
                    float *ncc_views, double *sw_views, void *stream) {
    if (const char *bad = check_step_args(ws, state, rot, xyz, S, V, N, ncc_eps, up, down, lambda_min, lambda_max,
                                          ncc_out, sw_views))
        return fail(-1, bad);
    if (S == 0) return 0;
    hipLaunchKernelGGL(wmv_step_kernel, dim3(S), dim3(64), 0, (hipStream_t)stream,
                       reinterpret_cast<const double *>(ws), reinterpret_cast<double *>(state), rot, xyz, V,
                       groups_of(N), ncc_eps, up, down, lambda_min, lambda_max, ncc_out, ncc_views, sw_views);
    return finish("ddrr_wmvlm_step");
}

}  // extern "C"
