// lm.hip -- the two kernels of a Levenberg-Marquardt registration step behind the renderer: the C ABI of
// include/diffdrr_lm_hip.h (libdiffdrr_lm_hip.so).  The arithmetic is lm_core.h's (and through it
// siddon_core.h's, raygen_core.h's and record_layout.h's); who computes what is lm_kernels.h's, written once for
// this library and the three that grew out of it (wlm.hip, mvlm.hip, wmvlm.hip).
//
//   normal_sums_kernel   lm_kernels.h's normal_sums_body on the 44 unweighted sums: rendered pose b owns its
//       parameters and its fixed image (x1 + b * x1_stride); one reorient and one detector for all.
//   step_kernel          one workgroup (one wave) per pose: 44 lanes add the pose's partials in index order,
//       lane 0 forms the normal equations, accepts or rejects, solves and writes the next trial.
// No atomics anywhere: the results are bitwise reproducible.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   normal_sums_kernel   106 VGPRs, no scratch, 34 688 B of LDS
//   step_kernel          126 VGPRs, no scratch, 352 B of LDS
#include <hip/hip_runtime.h>

#include "lm_kernels.h"

namespace {

using namespace ddrr_lm;

int groups_of(int N) { return (N + kGroupRays - 1) / kGroupRays; }

__global__ __launch_bounds__(kBlock) void normal_sums_kernel(
    const float *__restrict__ aux, const float *__restrict__ x1, long x1_stride,
    const float *__restrict__ source_v, const float *__restrict__ Mw, const float *__restrict__ Ainv,
    const float *__restrict__ P, const float *__restrict__ rot, const float *__restrict__ xyz, int a0, int a1,
    int a2, const float *__restrict__ Ro, int N, float eps, int with_img_path, double *__restrict__ ws,
    float *__restrict__ jac) {
    const int b = blockIdx.y;
    normal_sums_body<PlainSums>({b, Ro, x1 + b * x1_stride, nullptr, P}, aux, source_v, Mw, Ainv, rot, xyz, a0, a1, a2,
                                N, eps, with_img_path, ws, jac);
}

__global__ __launch_bounds__(64) void step_kernel(const double *__restrict__ ws, double *__restrict__ state,
                                                  float *__restrict__ rot, float *__restrict__ xyz, int N,
                                                  int groups, double ncc_eps, double up, double down,
                                                  double lambda_min, double lambda_max,
                                                  float *__restrict__ ncc_out) {
    __shared__ double S[kSums];
    const int b = blockIdx.x;
    sum_partials<kSums>(ws, b, groups, S);
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
    if (const char *bad = check_sums_args(aux, x1, x1_stride, source_v, Mw, Ainv, P, rot, xyz, a0, a1, a2, reorient34,
                                          B, N, ws))
        return fail(-1, bad);
    if (B == 0) return 0;
    hipLaunchKernelGGL(normal_sums_kernel, dim3(groups_of(N), B), dim3(kBlock), 0, (hipStream_t)stream, aux, x1,
                       x1_stride, source_v, Mw, Ainv, P, rot, xyz, a0, a1, a2, reorient34, N, eps,
                       with_img_path ? 1 : 0, reinterpret_cast<double *>(ws), jac);
    return finish("ddrr_lm_normal_sums");
}

int ddrr_lm_step(const void *ws, void *state, float *rot, float *xyz, int B, int N, double ncc_eps,
                 double up, double down, double lambda_min, double lambda_max, float *ncc_out,
                 void *stream) {
    if (const char *bad = check_step_args(ws, state, rot, xyz, B, N, ncc_eps, up, down, lambda_min, lambda_max,
                                          ncc_out))
        return fail(-1, bad);
    if (B == 0) return 0;
    hipLaunchKernelGGL(step_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream,
                       reinterpret_cast<const double *>(ws), reinterpret_cast<double *>(state), rot, xyz, N,
                       groups_of(N), ncc_eps, up, down, lambda_min, lambda_max, ncc_out);
    return finish("ddrr_lm_step");
}

}  // extern "C"
