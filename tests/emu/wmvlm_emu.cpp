// Host build of csrc/wmvlm_core.h behind the C ABI of include/diffdrr_wmvlm_hip.h: lm_emu_loops.h's loops with the
// picks of csrc/wmvlm.hip's wrappers.  Compiled by tests/wmvlm_cases.py with g++; no HIP, no GPU.  Pointers are host
// pointers; `stream` is ignored.
#include "lm_emu_loops.h"

#include "../../diffdrr_amd/csrc/wmvlm_core.h"

using namespace ddrr_wmvlm;

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
    emu_raygen(rot, xyz, a0, a1, a2, reorient_v, Ainv, [&](int v) { return P0 + v * P_stride; }, S, V, N, Mw, source_v,
               target_v, img, clear, clear_floats, clear_launch_ws);
    return 0;
}

int ddrr_wmvlm_normal_sums(const float *aux, const float *x1, const float *w, long w_stride, const float *source_v,
                           const float *Mw, const float *Ainv, const float *P0, long P_stride, const float *rot,
                           const float *xyz, int a0, int a1, int a2, const float *reorient_v, int S, int V, int N,
                           float eps, int with_img_path, void *ws, float *jac, void *) {
    if (const char *bad = check_sums_args(aux, x1, w, w_stride, source_v, Mw, Ainv, P0, P_stride, rot, xyz, a0, a1, a2,
                                          reorient_v, S, V, N, ws))
        return fail(-1, bad);
    emu_normal_sums<WeightedSums>(
        S * V,
        [&](int b) {
            const int st = b / V, v = b - st * V;
            return PosePicks{st, reorient_v + v * 12, x1 + (long)v * N, w + v * w_stride, P0 + v * P_stride};
        },
        aux, source_v, Mw, Ainv, rot, xyz, a0, a1, a2, N, eps, with_img_path, reinterpret_cast<double *>(ws), jac);
    return 0;
}

int ddrr_wmvlm_step(const void *ws, void *state, float *rot, float *xyz, int S, int V, int N, double ncc_eps,
                    double up, double down, double lambda_min, double lambda_max, float *ncc_out, float *ncc_views,
                    double *sw_views, void *) {
    if (const char *bad = check_step_args(ws, state, rot, xyz, S, V, N, ncc_eps, up, down, lambda_min, lambda_max,
                                          ncc_out, sw_views))
        return fail(-1, bad);
    for (int s = 0; s < S; ++s) {
        double acc[kAcc];
        clear_views(acc);
        for (int v = 0; v < V; ++v) {
            const long b = (long)s * V + v;
            double Sb[kWSums], sw_v;
            emu_sum_partials<kWSums>(reinterpret_cast<const double *>(ws), b, groups_of(N), Sb);
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
