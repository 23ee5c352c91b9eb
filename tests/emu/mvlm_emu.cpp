// Host build of csrc/mvlm_core.h behind the C ABI of include/diffdrr_mvlm_hip.h: lm_emu_loops.h's loops with the
// picks of csrc/mvlm.hip's wrappers.  Compiled by tests/mvlm_cases.py with g++; no HIP, no GPU.  Pointers are host
// pointers; `stream` is ignored.
#include "lm_emu_loops.h"

#include "../../diffdrr_amd/csrc/mvlm_core.h"

using namespace ddrr_mvlm;

extern "C" {

int ddrr_mvlm_abi_version(void) { return DDRR_MVLM_ABI_VERSION; }
const char *ddrr_mvlm_last_error(void) { return g_err; }

long ddrr_mvlm_workspace_bytes(int S, int V, int N) {
    return (S < 1 || check_shape(S, V, N)) ? 0 : (long)S * V * groups_of(N) * kSums * (long)sizeof(double);
}

int ddrr_mvlm_raygen(const float *rot, const float *xyz, int a0, int a1, int a2, const float *reorient_v,
                     const float *Ainv, const float *P, int S, int V, int N, float *Mw, float *source_v,
                     float *target_v, float *img, float *clear, long clear_floats, void *clear_launch_ws, void *) {
    if (const char *bad = check_raygen_args(rot, xyz, a0, a1, a2, reorient_v, Ainv, P, S, V, N, Mw, source_v, target_v,
                                            img, clear, clear_floats, clear_launch_ws))
        return fail(-1, bad);
    if (S == 0) return 0;
    emu_raygen(rot, xyz, a0, a1, a2, reorient_v, Ainv, [&](int) { return P; }, S, V, N, Mw, source_v, target_v, img,
               clear, clear_floats, clear_launch_ws);
    return 0;
}

int ddrr_mvlm_normal_sums(const float *aux, const float *x1, const float *source_v, const float *Mw,
                          const float *Ainv, const float *P, const float *rot, const float *xyz, int a0, int a1,
                          int a2, const float *reorient_v, int S, int V, int N, float eps, int with_img_path,
                          void *ws, float *jac, void *) {
    if (const char *bad = check_sums_args(aux, x1, source_v, Mw, Ainv, P, rot, xyz, a0, a1, a2, reorient_v, S, V, N, ws))
        return fail(-1, bad);
    emu_normal_sums<PlainSums>(
        S * V,
        [&](int b) {
            const int st = b / V, v = b - st * V;
            return PosePicks{st, reorient_v + v * 12, x1 + (long)v * N, nullptr, P};
        },
        aux, source_v, Mw, Ainv, rot, xyz, a0, a1, a2, N, eps, with_img_path, reinterpret_cast<double *>(ws), jac);
    return 0;
}

int ddrr_mvlm_step(const void *ws, void *state, float *rot, float *xyz, int S, int V, int N, double ncc_eps,
                   double up, double down, double lambda_min, double lambda_max, float *ncc_out, float *ncc_views,
                   void *) {
    if (const char *bad = check_step_args(ws, state, rot, xyz, S, V, N, ncc_eps, up, down, lambda_min, lambda_max,
                                          ncc_out))
        return fail(-1, bad);
    for (int s = 0; s < S; ++s) {
        double acc[kAcc];
        for (int v = 0; v < V; ++v) {
            const long b = (long)s * V + v;
            double Sb[kSums];
            emu_sum_partials<kSums>(reinterpret_cast<const double *>(ws), b, groups_of(N), Sb);
            const double ncc_v = add_view(Sb, N, ncc_eps, v, acc);
            if (ncc_views) ncc_views[b] = (float)ncc_v;
        }
        step_start(acc, V, up, down, lambda_min, lambda_max, reinterpret_cast<double *>(state) + (long)s * kState,
                   rot + s * 3, xyz + s * 3, ncc_out + s);
    }
    return 0;
}

}  // extern "C"
