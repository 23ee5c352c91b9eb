// Host build of csrc/wlm_core.h behind the C ABI of include/diffdrr_wlm_hip.h: lm_emu_loops.h's loops with the picks
// of csrc/wlm.hip's wrappers.  Compiled by tests/wlm_cases.py with g++; no HIP, no GPU.  Pointers are host pointers;
// `stream` is ignored.
#include "lm_emu_loops.h"

#include "../../diffdrr_amd/csrc/wlm_core.h"

using namespace ddrr_wlm;

static int groups_of(int N) { return (N + kGroupRays - 1) / kGroupRays; }

extern "C" {

int ddrr_wlm_abi_version(void) { return DDRR_WLM_ABI_VERSION; }
const char *ddrr_wlm_last_error(void) { return g_err; }

long ddrr_wlm_workspace_bytes(int B, int N) {
    return (B < 1 || N < 1) ? 0 : (long)B * groups_of(N) * kWSums * (long)sizeof(double);
}

int ddrr_wlm_normal_sums(const float *aux, const float *x1, long x1_stride, const float *w, long w_stride,
                         const float *source_v, const float *Mw, const float *Ainv, const float *P,
                         const float *rot, const float *xyz, int a0, int a1, int a2, const float *reorient34,
                         int B, int N, float eps, int with_img_path, void *ws, float *jac, void *) {
    if (const char *bad = check_sums_args(aux, x1, x1_stride, w, w_stride, source_v, Mw, Ainv, P, rot, xyz, a0, a1,
                                          a2, reorient34, B, N, ws))
        return fail(-1, bad);
    emu_normal_sums<WeightedSums>(
        B, [&](int b) { return PosePicks{b, reorient34, x1 + b * x1_stride, w + b * w_stride, P}; }, aux, source_v, Mw,
        Ainv, rot, xyz, a0, a1, a2, N, eps, with_img_path, reinterpret_cast<double *>(ws), jac);
    return 0;
}

int ddrr_wlm_step(const void *ws, void *state, float *rot, float *xyz, int B, int N, double ncc_eps,
                  double up, double down, double lambda_min, double lambda_max, float *ncc_out, void *) {
    if (const char *bad = check_step_args(ws, state, rot, xyz, B, N, ncc_eps, up, down, lambda_min, lambda_max,
                                          ncc_out))
        return fail(-1, bad);
    for (int b = 0; b < B; ++b) {
        double S[kWSums];
        emu_sum_partials<kWSums>(reinterpret_cast<const double *>(ws), b, groups_of(N), S);
        wstep_pose(S, ncc_eps, up, down, lambda_min, lambda_max, reinterpret_cast<double *>(state) + (long)b * kState,
                   rot + b * 3, xyz + b * 3, ncc_out + b);
    }
    return 0;
}

}  // extern "C"
