// wmvlm.hip -- the three kernels of a multi-view Levenberg-Marquardt registration step with a pixel weight and a
// detector per view, around the renderer: the C ABI of include/diffdrr_wmvlm_hip.h (libdiffdrr_wmvlm_hip.so).  The
// arithmetic is lm_core.h's, wlm_core.h's, raygen_core.h's, siddon_core.h's and record_layout.h's, with
// wmvlm_core.h's sum over the non-empty views; who computes what is lm_kernels.h's.
// Rendered pose b = s * V + v: start s = b / V owns the parameters; view v = b % V the reorient, the fixed image,
// the weight (w + v * w_stride) and the detector points (P + v * P_stride).
//
//   wmv_raygen_kernel        lm_kernels.h's raygen_body with (rot[s], xyz[s], Ro_v) on the view's detector points.
//   wmv_normal_sums_kernel   lm_kernels.h's normal_sums_body on the 45 weighted sums, with the fixed image, the
//       weight, the reorient, the detector points and the parameters picked per pose.  The picks are scalar (b is
//       uniform in a workgroup), so a ray costs what it costs in wlm.hip.
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

#include "lm_kernels.h"
#include "wmvlm_core.h"

namespace {

using namespace ddrr_wmvlm;

__global__ __launch_bounds__(kBlock) void wmv_raygen_kernel(
    const float *__restrict__ rot, const float *__restrict__ xyz, int a0, int a1, int a2,
    const float *__restrict__ reorient_v, const float *__restrict__ Ainv, const float *__restrict__ P0, long P_stride,
    int V, int N, float *__restrict__ Mw, float *__restrict__ source_v, float *__restrict__ target_v,
    float *__restrict__ img, float *__restrict__ clear, long clear_n, int *__restrict__ counter) {
    const int b = blockIdx.y, s = b / V, v = b - s * V;
    raygen_body(rot, xyz, a0, a1, a2, reorient_v + v * 12, Ainv, P0 + v * P_stride, s, N, Mw, source_v, target_v, img,
                clear, clear_n, counter);
}

__global__ __launch_bounds__(kBlock) void wmv_normal_sums_kernel(
    const float *__restrict__ aux, const float *__restrict__ x1, const float *__restrict__ wt, long w_stride,
    const float *__restrict__ source_v, const float *__restrict__ Mw, const float *__restrict__ Ainv,
    const float *__restrict__ P0, long P_stride, const float *__restrict__ rot, const float *__restrict__ xyz, int a0,
    int a1, int a2, const float *__restrict__ reorient_v, int V, int N, float eps, int with_img_path,
    double *__restrict__ ws, float *__restrict__ jac) {
    const int b = blockIdx.y, st = b / V, v = b - st * V;
    normal_sums_body<WeightedSums>({st, reorient_v + v * 12, x1 + (long)v * N, wt + v * w_stride, P0 + v * P_stride},
                                   aux, source_v, Mw, Ainv, rot, xyz, a0, a1, a2, N, eps, with_img_path, ws, jac);
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
        sum_partials<kWSums>(ws, b, groups, S);
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
