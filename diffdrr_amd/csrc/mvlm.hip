// mvlm.hip -- the three kernels of a multi-view Levenberg-Marquardt registration step around the renderer: the C ABI
// of include/diffdrr_mvlm_hip.h (libdiffdrr_mvlm_hip.so).  The arithmetic is lm_core.h's, raygen_core.h's,
// siddon_core.h's and record_layout.h's, with mvlm_core.h's sum over the views; what is here is who computes what.
// Rendered pose b = s * V + v: start s = b / V owns the parameters, view v = b % V the reorient and the fixed image.
//
//   mv_raygen_kernel        pose_ncc.hip's pose_raygen_fwd_kernel with (rot[s], xyz[s], Ro_v): one thread per ray,
//       every workgroup works its pose's matrix out again (three sincos, 30 fma, one lane, into LDS), and all of
//       them together clear what the render behind this launch wants zeroed.
//   mv_normal_sums_kernel   lm.hip's normal_sums_kernel -- one workgroup per (pose, run of 1024 rays), four rays per
//       thread, everything a thread's rays read requested before the first is worked on, the rows (j, x, f) staged
//       in LDS, the 44 sums taken as the Gram matrix of the staged values by one thread per (sum, slice) in double,
//       vector stores only -- with the fixed image, the reorient and the parameters picked per pose.  The picks
//       are scalar (b is uniform in a workgroup), so a ray costs what it costs there: the same registers, 34 KB LDS.
//   mv_step_kernel          one workgroup (one wave) per START: for each view in turn 44 lanes add the pose's
//       partials in index order, lane 0 forms the view's normal equations and adds them to the start's (28 doubles
//       in LDS, so that they are not held in registers across the views); then lane 0 accepts or rejects, solves
//       and writes the next trial.  Two barriers per view: V is a handful.
// No atomics anywhere: the results are bitwise reproducible.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "mvlm_core.h"

namespace {

using namespace ddrr_mvlm;

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

__global__ __launch_bounds__(kBlock) void mv_raygen_kernel(
    const float *__restrict__ rot, const float *__restrict__ xyz, int a0, int a1, int a2,
    const float *__restrict__ reorient_v, const float *__restrict__ Ainv, const float *__restrict__ P, int V, int N,
    float *__restrict__ Mw, float *__restrict__ source_v, float *__restrict__ target_v, float *__restrict__ img,
    float *__restrict__ clear, long clear_n, int *__restrict__ counter) {
    __shared__ float Ms[12];
    const int b = blockIdx.y, n = blockIdx.x * kBlock + threadIdx.x;
    const int s = b / V, v = b - s * V;
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

__global__ __launch_bounds__(kBlock) void mv_normal_sums_kernel(
    const float *__restrict__ aux, const float *__restrict__ x1, const float *__restrict__ source_v,
    const float *__restrict__ Mw, const float *__restrict__ Ainv, const float *__restrict__ P,
    const float *__restrict__ rot, const float *__restrict__ xyz, int a0, int a1, int a2,
    const float *__restrict__ reorient_v, int V, int N, float eps, int with_img_path, double *__restrict__ ws,
    float *__restrict__ jac) {
    __shared__ __attribute__((aligned(16))) float us[kGroupRays * 8];  // (j, x, f) of the workgroup's rays
    __shared__ float pose[kPoseFloats];
    __shared__ double red[kSlices][kSums];
    const int b = blockIdx.y;
    const int st = b / V, v = b - st * V;
    const float *M = Mw + (long)b * 12;
    const float *Ro = reorient_v + v * 12;
    const float *f = x1 + (long)v * N;
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
    }
    __builtin_amdgcn_sched_barrier(0);
    float rec[kPer][ddrr::SIDDON_AUX], fs[kPer], Ps[kPer][3];
    bool in[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int n0 = blockIdx.x * kGroupRays + threadIdx.x + k * kBlock;
        in[k] = n0 < n_end;
        const int n = in[k] ? n0 : n_end - 1;  // (a ray beyond the image re-reads the last one, unused)
        ddrr::rec_blocked_load(aux, (long)b * N + n, rec[k]);
        fs[k] = f[n];
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
            float4 *dst = reinterpret_cast<float4 *>(us + 8 * local);
            dst[0] = make_float4(j[0], j[1], j[2], j[3]);
            dst[1] = make_float4(j[4], j[5], x, fs[k]);
            if (jac) {
                float *out = jac + ((long)b * N + blockIdx.x * kGroupRays + local) * 6;
#pragma unroll
                for (int p = 0; p < 6; ++p) out[p] = j[p];
            }
        }
    }
    __syncthreads();
    const int count = n_end - (int)blockIdx.x * kGroupRays;
    if (threadIdx.x < kSums * kSlices)
        red[threadIdx.x / kSums][threadIdx.x % kSums] = slice_sum(us, count, threadIdx.x % kSums, threadIdx.x / kSums);
    __syncthreads();
    if (threadIdx.x < kSums) {
        double t = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kSlices; ++w) t += red[w][threadIdx.x];
        ws[((long)b * gridDim.x + blockIdx.x) * kSums + threadIdx.x] = t;
    }
}

__global__ __launch_bounds__(64) void mv_step_kernel(const double *__restrict__ ws, double *__restrict__ state,
                                                     float *__restrict__ rot, float *__restrict__ xyz, int V, int N,
                                                     int groups, double ncc_eps, double up, double down,
                                                     double lambda_min, double lambda_max,
                                                     float *__restrict__ ncc_out, float *__restrict__ ncc_views) {
    __shared__ double S[kSums];
    __shared__ double acc[kAcc];
    const int s = blockIdx.x;
    for (int v = 0; v < V; ++v) {
        const long b = (long)s * V + v;
        if (threadIdx.x < kSums) {
            const double *p = ws + b * groups * kSums + threadIdx.x;
            double t = p[0];
            for (int w = 1; w < groups; ++w) t += p[(long)w * kSums];
            S[threadIdx.x] = t;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const double ncc_v = add_view(S, N, ncc_eps, v, acc);
            if (ncc_views) ncc_views[b] = (float)ncc_v;
        }
        __syncthreads();  // (S is overwritten by the next view)
    }
    if (threadIdx.x != 0) return;
    step_start(acc, V, up, down, lambda_min, lambda_max, state + (long)s * kState, rot + s * 3, xyz + s * 3,
               ncc_out + s);
}

}  // namespace

extern "C" {

int ddrr_mvlm_abi_version(void) { return DDRR_MVLM_ABI_VERSION; }
const char *ddrr_mvlm_last_error(void) { return g_err; }

long ddrr_mvlm_workspace_bytes(int S, int V, int N) {
    return (S < 1 || check_shape(S, V, N)) ? 0 : (long)S * V * groups_of(N) * kSums * (long)sizeof(double);
}

int ddrr_mvlm_raygen(const float *rot, const float *xyz, int a0, int a1, int a2, const float *reorient_v,
                     const float *Ainv, const float *P, int S, int V, int N, float *Mw, float *source_v,
                     float *target_v, float *img, float *clear, long clear_floats, void *clear_launch_ws,
                     void *stream) {
    if (const char *bad = check_raygen_args(rot, xyz, a0, a1, a2, reorient_v, Ainv, P, S, V, N, Mw, source_v, target_v,
                                            img, clear, clear_floats, clear_launch_ws))
        return fail(-1, bad);
    if (S == 0) return 0;
    hipLaunchKernelGGL(mv_raygen_kernel, dim3((N + kBlock - 1) / kBlock, S * V), dim3(kBlock), 0, (hipStream_t)stream,
                       rot, xyz, a0, a1, a2, reorient_v, Ainv, P, V, N, Mw, source_v, target_v, img,
                       clear_floats > 0 ? clear : nullptr, clear_floats, reinterpret_cast<int *>(clear_launch_ws));
    return finish("ddrr_mvlm_raygen");
}

int ddrr_mvlm_normal_sums(const float *aux, const float *x1, const float *source_v, const float *Mw,
                          const float *Ainv, const float *P, const float *rot, const float *xyz, int a0, int a1,
                          int a2, const float *reorient_v, int S, int V, int N, float eps, int with_img_path,
                          void *ws, float *jac, void *stream) {
    if (const char *bad = check_sums_args(aux, x1, source_v, Mw, Ainv, P, rot, xyz, a0, a1, a2, reorient_v, S, V, N, ws))
        return fail(-1, bad);
    if (S == 0) return 0;
    hipLaunchKernelGGL(mv_normal_sums_kernel, dim3(groups_of(N), S * V), dim3(kBlock), 0, (hipStream_t)stream, aux, x1,
                       source_v, Mw, Ainv, P, rot, xyz, a0, a1, a2, reorient_v, V, N, eps, with_img_path ? 1 : 0,
                       reinterpret_cast<double *>(ws), jac);
    return finish("ddrr_mvlm_normal_sums");
}

int ddrr_mvlm_step(const void *ws, void *state, float *rot, float *xyz, int S, int V, int N, double ncc_eps,
                   double up, double down, double lambda_min, double lambda_max, float *ncc_out,
                   float *ncc_views, void *stream) {
    if (const char *bad = check_step_args(ws, state, rot, xyz, S, V, N, ncc_eps, up, down, lambda_min, lambda_max,
                                          ncc_out))
        return fail(-1, bad);
    if (S == 0) return 0;
    hipLaunchKernelGGL(mv_step_kernel, dim3(S), dim3(64), 0, (hipStream_t)stream,
                       reinterpret_cast<const double *>(ws), reinterpret_cast<double *>(state), rot, xyz, V, N,
                       groups_of(N), ncc_eps, up, down, lambda_min, lambda_max, ncc_out, ncc_views);
    return finish("ddrr_mvlm_step");
}

}  // extern "C"
