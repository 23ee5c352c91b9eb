// Host build of csrc/wmvlm_core.h behind the C ABI of include/diffdrr_wmvlm_hip.h: the loops of the gfx950 kernels
// (csrc/wmvlm.hip) over poses, workgroups, rays and slices, one element at a time, the sums in the kernels' order.
// Compiled by tests/wmvlm_cases.py with g++; no HIP, no GPU.  Pointers are host pointers; `stream` is ignored.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../diffdrr_amd/csrc/wmvlm_core.h"

namespace {

using namespace ddrr_wmvlm;

thread_local char g_err[512] = "";

int fail(int code, const char *what) {
    snprintf(g_err, sizeof(g_err), "%s", what);
    return code;
}

}  // namespace

extern "C" {

int ddrr_wmvlm_abi_version(void) { return DDRR_WMVLM_ABI_VERSION; }
const char *ddrr_wmvlm_last_error(void) { return g_err; }

long ddrr_wmvlm_workspace_bytes(int S, int V, int N) {
    return (S < 1 || check_shape(S, V, N)) ? 0 : (long)S * V * groups_of(N) * kWSums * (long)sizeof(double);
}

int ddrr_wmvlm_raygen(const float *rot, const float *xyz, int a0, int a1, int a2, const float *reorient_v,
                      const float *Ainv, const float *P0, long P_stride, int S, int V, int N, float *Mw,
                      float *source_v, float *target_v, float *img, float *clear, long clear_floats,
                      void *clear_launch_ws, void *) {
    if (const char *bad = check_raygen_args(rot, xyz, a0, a1, a2, reorient_v, Ainv, P0, P_stride, S, V, N, Mw,
                                            source_v, target_v, img, clear, clear_floats, clear_launch_ws))
        return fail(-1, bad);
    if (S == 0) return 0;
    if (clear_floats > 0) memset(clear, 0, (size_t)clear_floats * sizeof(float));
    if (clear_launch_ws) memset(clear_launch_ws, 0, 16);
    const int axes[3] = {a0, a1, a2};
    for (int b = 0; b < S * V; ++b) {
        const int s = b / V, v = b - s * V;
        const float *P = P0 + v * P_stride;
        float *M = Mw + (long)b * 12;
        ddrr::pose_euler_forward(rot + s * 3, xyz + s * 3, axes, reorient_v + v * 12, M);
        const float sw[3] = {M[3], M[7], M[11]};
        ddrr::apply34(Ainv, sw, source_v + b * 3);
        for (int n = 0; n < N; ++n) {
            const ddrr::RayGenOut o = ddrr::raygen_ray(M, Ainv, P + n * 3);
            const long r = (long)b * N + n;
            for (int a = 0; a < 3; ++a) target_v[r * 3 + a] = o.tv[a];
            img[r] = o.L;
        }
    }
    return 0;
}

int ddrr_wmvlm_normal_sums(const float *aux, const float *x1, const float *w, long w_stride, const float *source_v,
                           const float *Mw, const float *Ainv, const float *P0, long P_stride, const float *rot,
                           const float *xyz, int a0, int a1, int a2, const float *reorient_v, int S, int V, int N,
                           float eps, int with_img_path, void *ws_raw, float *jac, void *) {
    if (const char *bad = check_sums_args(aux, x1, w, w_stride, source_v, Mw, Ainv, P0, P_stride, rot, xyz, a0, a1, a2,
                                          reorient_v, S, V, N, ws_raw))
        return fail(-1, bad);
    double *ws = reinterpret_cast<double *>(ws_raw);
    const int G = groups_of(N), axes[3] = {a0, a1, a2};
    const float one = 1.f;
    std::vector<float> us((size_t)kGroupRays * 8), wl((size_t)kGroupRays);
    for (int b = 0; b < S * V; ++b) {
        const int s = b / V, v = b - s * V;
        const float *Ro = reorient_v + v * 12, *f = x1 + (long)v * N, *wv = w + v * w_stride, *P = P0 + v * P_stride;
        ddrr::PoseEulerAdjoint q;
        ddrr::pose_euler_adjoint_setup(rot + s * 3, xyz + s * 3, axes, Ro, q);
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
                ray_jacobian(rec, source_v + b * 3, Mw + (long)b * 12, Ainv, P + n * 3, eps, with_img_path, pose, Ro, j,
                             x);
                const float wn = wv[n];
                const bool on = wn != 0.f;  // (selected, not multiplied)
                for (int p = 0; p < 6; ++p) u[p] = on ? j[p] : 0.f;
                u[6] = on ? x : 0.f;
                u[7] = on ? f[n] : 0.f;
                wl[i] = wn;
                if (jac)
                    for (int p = 0; p < 6; ++p) jac[((long)b * N + n) * 6 + p] = j[p];
            }
            for (int k = 0; k < kWSums; ++k) {
                double t = wslice_sum(us.data(), wl.data(), &one, count, k, 0);
                for (int sl = 1; sl < kSlices; ++sl) t += wslice_sum(us.data(), wl.data(), &one, count, k, sl);
                ws[((long)b * G + g) * kWSums + k] = t;
            }
        }
    }
    return 0;
}

int ddrr_wmvlm_step(const void *ws_raw, void *state, float *rot, float *xyz, int S, int V, int N, double ncc_eps,
                    double up, double down, double lambda_min, double lambda_max, float *ncc_out, float *ncc_views,
                    double *sw_views, void *) {
    if (const char *bad = check_step_args(ws_raw, state, rot, xyz, S, V, N, ncc_eps, up, down, lambda_min, lambda_max,
                                          ncc_out, sw_views))
        return fail(-1, bad);
    const double *ws = reinterpret_cast<const double *>(ws_raw);
    const int G = groups_of(N);
    for (int s = 0; s < S; ++s) {
        double acc[kAcc];
        clear_views(acc);
        for (int v = 0; v < V; ++v) {
            const long b = (long)s * V + v;
            double Sb[kWSums], sw_v;
            for (int k = 0; k < kWSums; ++k) {
                double t = ws[b * G * kWSums + k];
                for (int g = 1; g < G; ++g) t += ws[(b * G + g) * kWSums + k];
                Sb[k] = t;
            }
            const double ncc_v = add_wview(Sb, ncc_eps, acc, sw_v);
            if (ncc_views) ncc_views[b] = (float)ncc_v;
            if (sw_views) sw_views[b] = sw_v;
        }
        wstep_start(acc, up, down, lambda_min, lambda_max, reinterpret_cast<double *>(state) + (long)s * kState,
                    rot + s * 3, xyz + s * 3, ncc_out + s);
    }
    return 0;
}

}  // extern "C"
