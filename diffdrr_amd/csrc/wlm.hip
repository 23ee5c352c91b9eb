// wlm.hip -- the two kernels of a Levenberg-Marquardt registration step with a per-pixel weight: the C ABI of
// include/diffdrr_wlm_hip.h (libdiffdrr_wlm_hip.so).  The arithmetic is wlm_core.h's and lm_core.h's (and through
// them siddon_core.h's, raygen_core.h's and record_layout.h's); what is here is who computes what.
//
//   wnormal_sums_kernel  lm.hip's normal_sums_kernel -- one workgroup per (pose, run of 1024 rays), four rays per
//       thread, everything a thread's rays read requested before the first is worked on, the rows (j, x, f) staged
//       in LDS, the sums taken as the Gram matrix of the staged values by one thread per (sum, slice) -- with a
//       ninth value per ray, its weight.  The weight is one more load per ray (4 B next to the 32 B record, the
//       4 B fixed pixel and the 12 B detector point) and goes to a plane of its own in LDS (4 KB beside the 32 KB of
//       rows): a 36-byte row would break the two 16-byte stores of a row and put the rows of consecutive rays at
//       36-byte steps, where the plane keeps ds_write_b128 for the rows and one ds_write_b32 for the weight, and
//       every (sum, slice) thread reads the weight as a broadcast (all 45 threads of a slice read the same ray).
//       225 = 5 x 45 threads take one (sum, slice) each: per product two LDS reads of the row (one a broadcast),
//       one of the weight (a broadcast), two v_mul_f64 and one v_add_f64 where the unweighted kernel has one
//       v_fma_f64 -- the product by the weight rounds on its own (include/diffdrr_wlm_hip.h), so nothing is fused.
//       The constant 1 of u_n is read from LDS at stride 0 (wl[1024]), so the loop has no branch, its three reads are
//       independent and it unrolls by four: 110 registers, no scratch, 38 848 bytes of LDS.
//       A ray of weight 0 stages a row of zeros and weight 0 (its fixed pixel, which may be NaN, is selected out).
//       The per-thread-accumulator form lm.hip's header records as worse stays unbuilt here too.
//   wstep_kernel         one workgroup (one wave) per pose: 45 lanes add the pose's partials in index order,
//       lane 0 forms the normal equations with n = Sw, accepts or rejects, solves and writes the next trial.
// No atomics anywhere: the results are bitwise reproducible.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "wlm_core.h"

namespace {

using namespace ddrr_wlm;

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

int groups_of(int N) { return (N + kGroupRays - 1) / kGroupRays; }

__global__ __launch_bounds__(kBlock) void wnormal_sums_kernel(
    const float *__restrict__ aux, const float *__restrict__ x1, long x1_stride, const float *__restrict__ wt,
    long w_stride, const float *__restrict__ source_v, const float *__restrict__ Mw,
    const float *__restrict__ Ainv, const float *__restrict__ P, const float *__restrict__ rot,
    const float *__restrict__ xyz, int a0, int a1, int a2, const float *__restrict__ Ro, int N, float eps,
    int with_img_path, double *__restrict__ ws, float *__restrict__ jac) {
    __shared__ __attribute__((aligned(16))) float us[kGroupRays * 8];  // (j, x, f) of the workgroup's rays
    __shared__ float wl[kGroupRays + 1];                               // their weights, then the constant 1
    __shared__ float pose[kPoseFloats];
    __shared__ double red[kSlices][kWSums];
    const int b = blockIdx.y;
    const float *M = Mw + (long)b * 12;
    const float s[3] = {source_v[b * 3], source_v[b * 3 + 1], source_v[b * 3 + 2]};
    const int n_end = min(N, (int)(blockIdx.x + 1) * kGroupRays);
    // (the pose's half of pose_euler_backward by one lane, before its wave requests its rays: as lm.hip)
    if (threadIdx.x == 0) {
        const float th[3] = {rot[b * 3], rot[b * 3 + 1], rot[b * 3 + 2]};
        const float tr[3] = {xyz[b * 3], xyz[b * 3 + 1], xyz[b * 3 + 2]};
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
        fs[k] = x1[b * x1_stride + n];
        wv[k] = wt[b * w_stride + n];
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
        double v = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kSlices; ++w) v += red[w][threadIdx.x];
        ws[((long)b * gridDim.x + blockIdx.x) * kWSums + threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(64) void wstep_kernel(const double *__restrict__ ws, double *__restrict__ state,
                                                   float *__restrict__ rot, float *__restrict__ xyz, int groups,
                                                   double ncc_eps, double up, double down, double lambda_min,
                                                   double lambda_max, float *__restrict__ ncc_out) {
    __shared__ double S[kWSums];
    const int b = blockIdx.x;
    if (threadIdx.x < kWSums) {
        const double *p = ws + (long)b * groups * kWSums + threadIdx.x;
        double v = p[0];
        for (int w = 1; w < groups; ++w) v += p[(long)w * kWSums];
        S[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    wstep_pose(S, ncc_eps, up, down, lambda_min, lambda_max, state + (long)b * kState, rot + b * 3, xyz + b * 3,
               ncc_out + b);
}

}  // namespace

extern "C" {

int ddrr_wlm_abi_version(void) { return DDRR_WLM_ABI_VERSION; }
const char *ddrr_wlm_last_error(void) { return g_err; }

long ddrr_wlm_workspace_bytes(int B, int N) {
    return (B < 1 || N < 1) ? 0 : (long)B * groups_of(N) * kWSums * (long)sizeof(double);
}

int ddrr_wlm_normal_sums(const float *aux, const float *x1, long x1_stride, const float *w, long w_stride,
                         const float *source_v, const float *Mw, const float *Ainv, const float *P,
                         const float *rot, const float *xyz, int a0, int a1, int a2, const float *reorient34,
                         int B, int N, float eps, int with_img_path, void *ws, float *jac, void *stream) {
    if (const char *bad = check_sums_args(aux, x1, x1_stride, w, w_stride, source_v, Mw, Ainv, P, rot, xyz, a0, a1,
                                          a2, reorient34, B, N, ws))
        return fail(-1, bad);
    if (B == 0) return 0;
    hipLaunchKernelGGL(wnormal_sums_kernel, dim3(groups_of(N), B), dim3(kBlock), 0, (hipStream_t)stream, aux, x1,
                       x1_stride, w, w_stride, source_v, Mw, Ainv, P, rot, xyz, a0, a1, a2, reorient34, N, eps,
                       with_img_path ? 1 : 0, reinterpret_cast<double *>(ws), jac);
    return finish("ddrr_wlm_normal_sums");
}

int ddrr_wlm_step(const void *ws, void *state, float *rot, float *xyz, int B, int N, double ncc_eps,
                  double up, double down, double lambda_min, double lambda_max, float *ncc_out,
                  void *stream) {
    if (const char *bad = check_step_args(ws, state, rot, xyz, B, N, ncc_eps, up, down, lambda_min, lambda_max,
                                          ncc_out))
        return fail(-1, bad);
    if (B == 0) return 0;
    hipLaunchKernelGGL(wstep_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream,
                       reinterpret_cast<const double *>(ws), reinterpret_cast<double *>(state), rot, xyz,
                       groups_of(N), ncc_eps, up, down, lambda_min, lambda_max, ncc_out);
    return finish("ddrr_wlm_step");
}

}  // extern "C"
