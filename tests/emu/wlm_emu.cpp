// Host build of csrc/wlm_core.h behind the C ABI of include/diffdrr_wlm_hip.h: the loops of the gfx950 kernels
// (csrc/wlm.hip) over workgroups, rays and slices, one element at a time, the sums in the kernels' order.
// Compiled by tests/wlm_cases.py with g++; no HIP, no GPU.  Pointers are host pointers; `stream` is ignored.
#include <stdio.h>

#include <vector>

#include "../../diffdrr_amd/csrc/wlm_core.h"

namespace {

using namespace ddrr_wlm;

thread_local char g_err[512] = "";

int fail(int code, const char *what) {
    snprintf(g_err, sizeof(g_err), "%s", what);
    return code;
}

int groups_of(int N) { return (N + kGroupRays - 1) / kGroupRays; }

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
                         int B, int N, float eps, int with_img_path, void *ws_raw, float *jac, void *) {
    if (const char *bad = check_sums_args(aux, x1, x1_stride, w, w_stride, source_v, Mw, Ainv, P, rot, xyz, a0, a1,
                                          a2, reorient34, B, N, ws_raw))
        return fail(-1, bad);
    double *ws = reinterpret_cast<double *>(ws_raw);
    const int G = groups_of(N), axes[3] = {a0, a1, a2};
    const float one = 1.f;
    std::vector<float> us((size_t)kGroupRays * 8), wl((size_t)kGroupRays);
    for (int b = 0; b < B; ++b) {
        ddrr::PoseEulerAdjoint q;
        ddrr::pose_euler_adjoint_setup(rot + b * 3, xyz + b * 3, axes, reorient34, q);
        float pose[kPoseFloats];
        for (int e = 0; e < 9; ++e) pose[e] = q.R[e];
        for (int e = 0; e < 3; ++e) pose[9 + e] = q.v[e];
        for (int e = 0; e < 27; ++e) pose[12 + e] = q.dR[e];
        for (int g = 0; g < G; ++g) {
            const int n0 = g * kGroupRays, count = (N < n0 + kGroupRays ? N : n0 + kGroupRays) - n0;
            for (int i = 0; i < count; ++i) {
                const int n = n0 + i;
                float rec[8], j[6], x, *u = us.data() + 8 * i;
                ddrr::rec_blocked_load(aux, (long)b * N + n, rec);
                ray_jacobian(rec, source_v + b * 3, Mw + (long)b * 12, Ainv, P + n * 3, eps, with_img_path, pose,
                             reorient34, j, x);
                const float wn = w[b * w_stride + n];
                const bool on = wn != 0.f;  // (selected, not multiplied)
                for (int p = 0; p < 6; ++p) u[p] = on ? j[p] : 0.f;
                u[6] = on ? x : 0.f;
                u[7] = on ? x1[b * x1_stride + n] : 0.f;
                wl[i] = wn;
                if (jac)
                    for (int p = 0; p < 6; ++p) jac[((long)b * N + n) * 6 + p] = j[p];
            }
            for (int k = 0; k < kWSums; ++k) {
                double v = wslice_sum(us.data(), wl.data(), &one, count, k, 0);
                for (int s = 1; s < kSlices; ++s) v += wslice_sum(us.data(), wl.data(), &one, count, k, s);
                ws[((long)b * G + g) * kWSums + k] = v;
            }
        }
    }
    return 0;
}

int ddrr_wlm_step(const void *ws_raw, void *state, float *rot, float *xyz, int B, int N, double ncc_eps,
                  double up, double down, double lambda_min, double lambda_max, float *ncc_out, void *) {
    if (const char *bad = check_step_args(ws_raw, state, rot, xyz, B, N, ncc_eps, up, down, lambda_min, lambda_max,
                                          ncc_out))
        return fail(-1, bad);
    const double *ws = reinterpret_cast<const double *>(ws_raw);
    const int G = groups_of(N);
    for (int b = 0; b < B; ++b) {
        double S[kWSums];
        for (int k = 0; k < kWSums; ++k) {
            double v = ws[(long)b * G * kWSums + k];
            for (int g = 1; g < G; ++g) v += ws[((long)b * G + g) * kWSums + k];
            S[k] = v;
        }
        wstep_pose(S, ncc_eps, up, down, lambda_min, lambda_max, reinterpret_cast<double *>(state) + (long)b * kState,
                   rot + b * 3, xyz + b * 3, ncc_out + b);
    }
    return 0;
}

}  // extern "C"
