// Host build of csrc/lm_core.h behind the C ABI of include/diffdrr_lm_hip.h: the loops of the gfx950 kernels
// (csrc/lm.hip) over workgroups, rays and slices, one element at a time, the sums in the kernels' order.
// Compiled by tests/lm_cases.py with g++; no HIP, no GPU.  Pointers are host pointers; `stream` is ignored.
#include <stdio.h>

#include <vector>

#include "../../diffdrr_amd/csrc/lm_core.h"

namespace {

using namespace ddrr_lm;

thread_local char g_err[512] = "";

int fail(int code, const char *what) {
    snprintf(g_err, sizeof(g_err), "%s", what);
    return code;
}

int groups_of(int N) { return (N + kGroupRays - 1) / kGroupRays; }

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
                        float eps, int with_img_path, void *ws_raw, float *jac, void *) {
    if (!aux || !x1 || !source_v || !Mw || !Ainv || !P || !rot || !xyz || !reorient34 || !ws_raw)
        return fail(-1, "null pointer");
    if (a0 < 0 || a0 > 2 || a1 < 0 || a1 > 2 || a2 < 0 || a2 > 2 || a1 == a0 || a1 == a2)
        return fail(-1, "invalid Euler convention");
    if (B < 0 || N < 1) return fail(-1, "bad batch / image size");
    if (x1_stride != 0 && x1_stride != N) return fail(-1, "x1_stride must be N, or 0 for a shared image");
    double *ws = reinterpret_cast<double *>(ws_raw);
    const int G = groups_of(N), axes[3] = {a0, a1, a2};
    std::vector<float> us((size_t)kGroupRays * 8);
    for (int b = 0; b < B; ++b) {
        ddrr::PoseEulerAdjoint q;
        ddrr::pose_euler_adjoint_setup(rot + b * 3, xyz + b * 3, axes, reorient34, q);
        float pose[kPoseFloats];
        for (int e = 0; e < 9; ++e) pose[e] = q.R[e];
        for (int e = 0; e < 3; ++e) pose[9 + e] = q.v[e];
        for (int e = 0; e < 27; ++e) pose[12 + e] = q.dR[e];
        for (int w = 0; w < G; ++w) {
            const int n0 = w * kGroupRays, count = (N < n0 + kGroupRays ? N : n0 + kGroupRays) - n0;
            for (int i = 0; i < count; ++i) {
                const int n = n0 + i;
                float rec[8], x, *u = us.data() + 8 * i;
                ddrr::rec_blocked_load(aux, (long)b * N + n, rec);
                ray_jacobian(rec, source_v + b * 3, Mw + (long)b * 12, Ainv, P + n * 3, eps, with_img_path, pose,
                             reorient34, u, x);
                u[6] = x;
                u[7] = x1[b * x1_stride + n];
                if (jac)
                    for (int p = 0; p < 6; ++p) jac[((long)b * N + n) * 6 + p] = u[p];
            }
            for (int k = 0; k < kSums; ++k) {
                double v = slice_sum(us.data(), count, k, 0);
                for (int s = 1; s < kSlices; ++s) v += slice_sum(us.data(), count, k, s);
                ws[((long)b * G + w) * kSums + k] = v;
            }
        }
    }
    return 0;
}

int ddrr_lm_step(const void *ws_raw, void *state, float *rot, float *xyz, int B, int N, double ncc_eps,
                 double up, double down, double lambda_min, double lambda_max, float *ncc_out, void *) {
    if (!ws_raw || !state || !rot || !xyz || !ncc_out) return fail(-1, "null pointer");
    if (B < 0 || N < 1) return fail(-1, "bad batch / image size");
    const double *ws = reinterpret_cast<const double *>(ws_raw);
    const int G = groups_of(N);
    for (int b = 0; b < B; ++b) {
        double S[kSums];
        for (int k = 0; k < kSums; ++k) {
            double v = ws[(long)b * G * kSums + k];
            for (int w = 1; w < G; ++w) v += ws[((long)b * G + w) * kSums + k];
            S[k] = v;
        }
        step_pose(S, N, ncc_eps, up, down, lambda_min, lambda_max, reinterpret_cast<double *>(state) + (long)b * kState,
                  rot + b * 3, xyz + b * 3, ncc_out + b);
    }
    return 0;
}

}  // extern "C"
