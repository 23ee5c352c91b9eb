// mi.hip -- MutualInformation as fused gfx950 kernels: the C ABI of include/diffdrr_mi_hip.h
// (libdiffdrr_mi_hip.so).  The kernels, the workspace layout and the launch geometry are mi_kernels.h's, instantiated
// with kWeighted = false: no weight is read, none is passed.  Here: the __global__ wrappers and the entries.
#include <hip/hip_runtime.h>

#include "../../include/diffdrr_mi_hip.h"
#include "mi_kernels.h"

namespace {

using namespace ddrr_mi;

static_assert(kMaxBins == DDRR_MI_MAX_BINS, "mi_kernels.h and include/diffdrr_mi_hip.h disagree");

__global__ __launch_bounds__(kFwdWaves * 64, 2) void mi_joint_kernel(
        const float *__restrict__ x1, long s1, const float *__restrict__ x2, long s2, int N,
        const float *__restrict__ bins, int K, const float *__restrict__ sigma, int Kp, int nb, int chunks,
        int cp, float *__restrict__ part_J, float *__restrict__ part_P) {
    joint_body<false>(x1, s1, x2, s2, nullptr, 0, N, bins, K, sigma, Kp, nb, chunks, cp, part_J, part_P, nullptr);
}

__global__ __launch_bounds__(256) void mi_reduce_kernel(const float *__restrict__ part_J,
                                                        const float *__restrict__ part_P, int chunks, int Kp,
                                                        double *__restrict__ J, double *__restrict__ P) {
    reduce_body<false>(part_J, part_P, nullptr, chunks, Kp, J, P, nullptr, nullptr);
}

__global__ __launch_bounds__(kEpiThreads) void mi_epilogue_kernel(
        double *__restrict__ J, const double *__restrict__ P, int K, int Kp, int N, float epsilon,
        int normalize, float *__restrict__ out, float *__restrict__ state, long SS) {
    epilogue_body<false>(J, P, nullptr, K, Kp, N, epsilon, normalize, out, state, SS);
}

template <int NS>
__global__ __launch_bounds__(512) void mi_grad_kernel(
        const float *__restrict__ xo, long so, const float *__restrict__ xt, long st, int N,
        const float *__restrict__ bins, int K, const float *__restrict__ sigma, const float *__restrict__ state,
        long SS, int Kp, int transpose, int m_offset, const float *__restrict__ g_out, int g_stride, int tpw,
        float *__restrict__ grad) {
    grad_body<NS, false>(xo, so, xt, st, nullptr, 0, N, bins, K, sigma, state, SS, Kp, transpose, m_offset, g_out,
                         g_stride, tpw, grad);
}

}  // namespace

extern "C" {

int ddrr_mi_abi_version(void) { return DDRR_MI_ABI_VERSION; }
const char *ddrr_mi_last_error(void) { return g_err; }

long ddrr_mi_workspace_bytes(int B, int H, int W, int num_bins) {
    if (check_sizes(B, H, W, num_bins)) return -1;
    if (B == 0) return 0;
    return geom<false>(B, H, W, num_bins).total * (long)sizeof(float);
}

long ddrr_mi_state_floats(int num_bins) {
    if (check_sizes(0, 1, 1, num_bins)) return -1;
    return state_floats(num_bins);
}

int ddrr_mi_forward(const float *x1, long x1_stride, const float *x2, long x2_stride, int B, int H, int W,
                    const float *bins, int num_bins, const float *sigma, float epsilon, int normalize,
                    void *workspace, long workspace_bytes, float *out, float *state, void *stream) {
    if (!x1) return fail(-1, "null x1 pointer");
    if (!x2) return fail(-1, "null x2 pointer");
    if (!bins) return fail(-1, "null bins pointer");
    if (!sigma) return fail(-1, "null sigma pointer");
    if (!workspace) return fail(-1, "null workspace pointer");
    if (!out) return fail(-1, "null out pointer");
    if (int rc = check_sizes(B, H, W, num_bins)) return rc;
    if (int rc = check_strides(x1_stride, x2_stride, 0, H, W)) return rc;
    if (!(epsilon >= 0.0f)) return fail(-1, "epsilon must be >= 0");
    if (B == 0) return 0;
    const Geom g = geom<false>(B, H, W, num_bins);
    if (workspace_bytes < g.total * (long)sizeof(float))
        return fail(-1, "workspace_bytes is smaller than ddrr_mi_workspace_bytes()");
    if ((reinterpret_cast<unsigned long>(workspace) & 15) != 0) return fail(-1, "workspace must be 16-byte aligned");
    float *ws = static_cast<float *>(workspace);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mi_joint_kernel, dim3(g.chunks, g.nb * g.nb, B), dim3(kFwdWaves * 64), 0, s, x1, x1_stride,
                       x2, x2_stride, g.N, bins, num_bins, sigma, g.Kp, g.nb, g.chunks, g.cp, ws + g.part_J,
                       ws + g.part_P);
    if (int rc = finish("ddrr_mi_forward (joint)")) return rc;
    const long E = (long)g.Kp * g.Kp + 2 * g.Kp;
    hipLaunchKernelGGL(mi_reduce_kernel, dim3((unsigned)((E + 255) / 256), B), dim3(256), 0, s, ws + g.part_J,
                       ws + g.part_P, g.chunks, g.Kp, reinterpret_cast<double *>(ws + g.J),
                       reinterpret_cast<double *>(ws + g.P));
    if (int rc = finish("ddrr_mi_forward (reduce)")) return rc;
    hipLaunchKernelGGL(mi_epilogue_kernel, dim3(B), dim3(kEpiThreads), 0, s, reinterpret_cast<double *>(ws + g.J),
                       reinterpret_cast<const double *>(ws + g.P), num_bins, g.Kp,
                       g.N, epsilon, normalize ? 1 : 0, out, state, state_floats(num_bins));
    return finish("ddrr_mi_forward (epilogue)");
}

int ddrr_mi_backward(const float *x1, long x1_stride, const float *x2, long x2_stride, int B, int H, int W,
                     const float *bins, int num_bins, const float *sigma, const float *state, int which,
                     const float *g_out, int g_stride, float *grad, void *stream) {
    if (!x1) return fail(-1, "null x1 pointer");
    if (!x2) return fail(-1, "null x2 pointer");
    if (!bins) return fail(-1, "null bins pointer");
    if (!sigma) return fail(-1, "null sigma pointer");
    if (!state) return fail(-1, "null state pointer");
    if (!g_out) return fail(-1, "null g_out pointer");
    if (!grad) return fail(-1, "null grad pointer");
    if (int rc = check_sizes(B, H, W, num_bins)) return rc;
    if (int rc = check_strides(x1_stride, x2_stride, 0, H, W)) return rc;
    if (which != 0 && which != 1) return fail(-1, "which must be 0 (x1) or 1 (x2)");
    if (g_stride != 0 && g_stride != 1) return fail(-1, "g_stride must be 0 or 1");
    if (B == 0) return 0;
    const GradGeom q = grad_geom(x1, x1_stride, x2, x2_stride, B, H, W, num_bins, which);
    dispatch_ns(num_bins, [&](auto ns) {
        hipLaunchKernelGGL(mi_grad_kernel<decltype(ns)::value>, dim3(q.chunks, B), dim3(64 * q.nbw), 0,
                           (hipStream_t)stream, q.xo, q.so, q.xt, q.st, q.N, bins, num_bins, sigma, state, q.SS, q.Kp,
                           q.transpose, q.m_offset, g_out, g_stride, q.tpw, grad);
    });
    return finish("ddrr_mi_backward");
}

}  // extern "C"
