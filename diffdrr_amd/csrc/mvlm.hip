// mvlm.hip -- the three kernels of a multi-view Levenberg-Marquardt registration step around the renderer: the C ABI
// of include/diffdrr_mvlm_hip.h (libdiffdrr_mvlm_hip.so).  The arithmetic is lm_core.h's, raygen_core.h's,
// siddon_core.h's and record_layout.h's, with mvlm_core.h's sum over the views; who computes what is lm_kernels.h's.
// Rendered pose b = s * V + v: start s = b / V owns the parameters, view v = b % V the reorient and the fixed image.
//
//   mv_raygen_kernel        lm_kernels.h's raygen_body with (rot[s], xyz[s], Ro_v) on the one detector.
//   mv_normal_sums_kernel   lm_kernels.h's normal_sums_body on the 44 unweighted sums, with the fixed image, the
//       reorient and the parameters picked per pose.  The picks are scalar (b is uniform in a workgroup), so a ray
//       costs what it costs in lm.hip: the same registers, 34 KB LDS.
//   mv_step_kernel          one workgroup (one wave) per START: for each view in turn 44 lanes add the pose's
//       partials in index order, lane 0 forms the view's normal equations and adds them to the start's (28 doubles
//       in LDS, so that they are not held in registers across the views); then lane 0 accepts or rejects, solves
//       and writes the next trial.  Two barriers per view: V is a handful.
// No atomics anywhere: the results are bitwise reproducible.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   mv_raygen_kernel        34 VGPRs, no scratch, 48 B of LDS
//   mv_normal_sums_kernel   106 VGPRs, no scratch, 34 688 B of LDS
//   mv_step_kernel          124 VGPRs, no scratch, 576 B of LDS (44 + 28 doubles)
#include <hip/hip_runtime.h>

#include "lm_kernels.h"
#include "mvlm_core.h"

namespace {

using namespace ddrr_mvlm;

__global__ __launch_bounds__(kBlock) void mv_raygen_kernel(
    const float *__restrict__ rot, const float *__restrict__ xyz, int a0, int a1, int a2,
    const float *__restrict__ reorient_v, const float *__restrict__ Ainv, const float *__restrict__ P, int V, int N,
    float *__restrict__ Mw, float *__restrict__ source_v, float *__restrict__ target_v, float *__restrict__ img,
    float *__restrict__ clear, long clear_n, int *__restrict__ counter) {
    const int b = blockIdx.y, s = b / V, v = b - s * V;
    raygen_body(rot, xyz, a0, a1, a2, reorient_v + v * 12, Ainv, P, s, N, Mw, source_v, target_v, img, clear, clear_n,
                counter);
}

__global__ __launch_bounds__(kBlock) void mv_normal_sums_kernel(
    const float *__restrict__ aux, const float *__restrict__ x1, const float *__restrict__ source_v,
    const float *__restrict__ Mw, const float *__restrict__ Ainv, const float *__restrict__ P,
    const float *__restrict__ rot, const float *__restrict__ xyz, int a0, int a1, int a2,
    const float *__restrict__ reorient_v, int V, int N, float eps, int with_img_path, double *__restrict__ ws,
    float *__restrict__ jac) {
    const int b = blockIdx.y, st = b / V, v = b - st * V;
    normal_sums_body<PlainSums>({st, reorient_v + v * 12, x1 + (long)v * N, nullptr, P}, aux, source_v, Mw, Ainv, rot,
                                xyz, a0, a1, a2, N, eps, with_img_path, ws, jac);
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
        sum_partials<kSums>(ws, b, groups, S);
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
