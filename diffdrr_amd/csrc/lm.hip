// lm.hip -- the two kernels of a Levenberg-Marquardt registration step behind the renderer: the C ABI of
// include/diffdrr_lm_hip.h (libdiffdrr_lm_hip.so).  The arithmetic is lm_core.h's (and through it
// siddon_core.h's, raygen_core.h's and record_layout.h's); what is here is who computes what.
//
//   normal_sums_kernel   one workgroup per (pose, run of 1024 rays), four rays per thread.  Everything a
//       thread's rays read -- five record planes, the fixed pixel, the detector point -- is requested before
//       the first is worked on, as in siddon_ncc_bwd_pose_kernel.  A ray is ~150 fma to its Jacobian row
//       (the record's endpoint gradients, the ray generation's adjoint, then pose_euler_backward's map from
//       the matrix gradient to the parameters -- 72 fma on 39 floats of the pose that one lane puts into LDS:
//       the 12 x 6 derivative D of include/diffdrr_lm_hip.h in factored form, and the very operations the
//       existing backward entry performs); the row, x and f (8 floats) go to LDS.  The 44 sums are the Gram matrix of those 1024 x 9
//       values ((j, x, f, 1): all pairs but 1 * 1): 220 threads take one (sum, slice of the rays) each and
//       add their products in double in ray order -- two LDS reads (one a broadcast) and one v_fma_f64 per
//       product --, 44 threads add the five slices and write the workgroup's partial.  Keeping the 44 sums
//       per thread instead (float accumulators over its four rays, then 44 double butterflies through the
//       wave) was tried first: 44 + 36 loaded values + a ray's temporaries came to 166 registers, or 128
//       with 84 bytes of scratch, and the butterflies alone are 528 ds_bpermute per wave.  The staged form
//       takes 105 registers, no scratch, no cross-lane traffic, and rounds nothing before the double sums.
//   step_kernel          one workgroup (one wave) per pose: 44 lanes add the pose's partials in index order,
//       lane 0 forms the normal equations, accepts or rejects, solves and writes the next trial.
// No atomics anywhere: the results are bitwise reproducible.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "lm_core.h"

namespace {

using namespace ddrr_lm;

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

__global__ __launch_bounds__(kBlock) void normal_sums_kernel(
    const float *__restrict__ aux, const float *__restrict__ x1, long x1_stride,
    const float *__restrict__ source_v, const float *__restrict__ Mw, const float *__restrict__ Ainv,
    const float *__restrict__ P, const float *__restrict__ rot, const float *__restrict__ xyz, int a0, int a1,
    int a2, const float *__restrict__ Ro, int N, float eps, int with_img_path, double *__restrict__ ws,
    float *__restrict__ jac) {
    __shared__ __attribute__((aligned(16))) float us[kGroupRays * 8];  // (j, x, f) of the workgroup's rays
    __shared__ float pose[kPoseFloats];
    __shared__ double red[kSlices][kSums];
    const int b = blockIdx.y;
    const float *M = Mw + (long)b * 12;
    const float s[3] = {source_v[b * 3], source_v[b * 3 + 1], source_v[b * 3 + 2]};
    const int n_end = min(N, (int)(blockIdx.x + 1) * kGroupRays);
    // the pose's half of pose_euler_backward (three sincos, six 3 x 3 products) by one lane of the first wave,
    // before that wave requests its rays (its eight 3 x 3 matrices are not to share the registers with 36
    // loaded values); the other three waves have their loads in flight meanwhile
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
        fs[k] = x1[b * x1_stride + n];
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
        double v = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kSlices; ++w) v += red[w][threadIdx.x];
        ws[((long)b * gridDim.x + blockIdx.x) * kSums + threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(64) void step_kernel(const double *__restrict__ ws, double *__restrict__ state,
                                                  float *__restrict__ rot, float *__restrict__ xyz, int N,
                                                  int groups, double ncc_eps, double up, double down,
                                                  double lambda_min, double lambda_max,
                                                  float *__restrict__ ncc_out) {
    __shared__ double S[kSums];
    const int b = blockIdx.x;
    if (threadIdx.x < kSums) {
        const double *p = ws + (long)b * groups * kSums + threadIdx.x;
        double v = p[0];
        for (int w = 1; w < groups; ++w) v += p[(long)w * kSums];
        S[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    step_pose(S, N, ncc_eps, up, down, lambda_min, lambda_max, state + (long)b * kState, rot + b * 3, xyz + b * 3,
              ncc_out + b);
}

}  // namespace

extern "C" {

int ddrr_lm_abi_version(void) { return DDRR_LM_ABI_VERSION; }
const char *ddrr_lm_last_error(void) { return g_err; }

long ddrr_lm_workspace_bytes(int B, int N) {
    return (B < 1 || N < 1) ? 0 : (long)B * groups_of(N) * kSums * (long)sizeof(double);
}

int ddrr_lm_normal_sums(const float *aux, const float *x1, long x1_stride, const float *source_v,
                        const float *Mw, const float *Ainv, const float *P, const float *rot,
                        const float *xyz, int a0, int a1, int a2, const float *reorient34, int B, int N,
                        float eps, int with_img_path, void *ws, float *jac, void *stream) {
    if (!aux || !x1 || !source_v || !Mw || !Ainv || !P || !rot || !xyz || !reorient34 || !ws)
        return fail(-1, "null pointer");
    if (a0 < 0 || a0 > 2 || a1 < 0 || a1 > 2 || a2 < 0 || a2 > 2 || a1 == a0 || a1 == a2)
        return fail(-1, "invalid Euler convention");
    if (B < 0 || N < 1) return fail(-1, "bad batch / image size");
    if (x1_stride != 0 && x1_stride != N) return fail(-1, "x1_stride must be N, or 0 for a shared image");
    if (reinterpret_cast<uintptr_t>(ws) & 7) return fail(-1, "ws must be 8-byte aligned");
    if (B == 0) return 0;
    if (B > DDRR_LM_MAX_POSES) return fail(-1, "at most 65535 poses per call");
    hipLaunchKernelGGL(normal_sums_kernel, dim3(groups_of(N), B), dim3(kBlock), 0, (hipStream_t)stream, aux, x1,
                       x1_stride, source_v, Mw, Ainv, P, rot, xyz, a0, a1, a2, reorient34, N, eps,
                       with_img_path ? 1 : 0, reinterpret_cast<double *>(ws), jac);
    return finish("ddrr_lm_normal_sums");
}

int ddrr_lm_step(const void *ws, void *state, float *rot, float *xyz, int B, int N, double ncc_eps,
                 double up, double down, double lambda_min, double lambda_max, float *ncc_out,
                 void *stream) {
    if (!ws || !state || !rot || !xyz || !ncc_out) return fail(-1, "null pointer");
    if (B < 0 || N < 1) return fail(-1, "bad batch / image size");
    if (!(ncc_eps >= 0.0 && isfinite(ncc_eps))) return fail(-1, "ncc_eps must be >= 0 and finite");
    if (!(up > 1.0 && isfinite(up) && down > 0.0 && down < 1.0))
        return fail(-1, "up must be > 1 and finite, down in (0, 1)");
    if (!(lambda_min > 0.0 && lambda_min <= lambda_max && isfinite(lambda_max)))
        return fail(-1, "0 < lambda_min <= lambda_max, finite, expected");
    if ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(state)) & 7)
        return fail(-1, "ws and state must be 8-byte aligned");
    if (B == 0) return 0;
    if (B > DDRR_LM_MAX_POSES) return fail(-1, "at most 65535 poses per call");
    hipLaunchKernelGGL(step_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream,
                       reinterpret_cast<const double *>(ws), reinterpret_cast<double *>(state), rot, xyz, N,
                       groups_of(N), ncc_eps, up, down, lambda_min, lambda_max, ncc_out);
    return finish("ddrr_lm_step");
}

}  // extern "C"
