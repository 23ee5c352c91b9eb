// Host build of csrc/wncc_core.h behind the C ABI of include/diffdrr_wncc_hip.h: the loops of the gfx950 kernels
// (csrc/wncc.hip) over workgroups and pixels, one element at a time -- per-workgroup partials into the caller's
// workspace, then the folds in workgroup and in pair order.  Compiled by tests/wncc_cases.py with g++; no HIP, no
// GPU.  Pointers are host pointers; `stream` is ignored.
#include <stdio.h>

#include "../../diffdrr_amd/csrc/wncc_core.h"

namespace {

using namespace ddrr_wncc;

thread_local char g_err[512] = "";

int fail(int code, const char *what) {
    snprintf(g_err, sizeof(g_err), "%s", what);
    return code;
}

int forward(bool record, const float *aux, const float *x2, const float *x1, long x1_stride, const float *w,
            long w_stride, int B, int N, float eps, void *ws_raw, float *ncc, float *stats, float *out,
            float *ncc_sum) {
    if ((record && !aux) || !x2 || !x1 || !w || !ws_raw || !ncc || !stats) return fail(-1, "null pointer");
    if (const char *m = check_sizes(B, N)) return fail(-1, m);
    if (const char *m = check_rows(x1_stride, w_stride, N)) return fail(-1, m);
    if (const char *m = check_eps(eps)) return fail(-1, m);
    if (const char *m = check_ws(ws_raw)) return fail(-1, m);
    double *ws = reinterpret_cast<double *>(ws_raw);
    const int G = groups_of(N);
    for (int b = 0; b < B; ++b)
        for (int g = 0; g < G; ++g) {
            double m[kMoments] = {0., 0., 0., 0., 0., 0.};
            const int n_end = N < (g + 1) * kGroupRays ? N : (g + 1) * kGroupRays;
            for (int n = g * kGroupRays; n < n_end; ++n) {
                const long r = (long)b * N + n;
                const float c = record ? x2[r] * aux[ddrr::rec_index(r, 0)] : x2[r];
                if (out) out[r] = c;
                moments_take(m, w[b * w_stride + n], x1[b * x1_stride + n], c);
            }
            for (int k = 0; k < kMoments; ++k) ws[((long)b * G + g) * kMoments + k] = m[k];
        }
    double total = 0.0;
    for (int b = 0; b < B; ++b) {
        double S[kMoments];
        for (int k = 0; k < kMoments; ++k) {
            S[k] = ws[(long)b * G * kMoments + k];
            for (int g = 1; g < G; ++g) S[k] += ws[((long)b * G + g) * kMoments + k];
        }
        finalize(S, eps, stats + b * kStats);
        ncc[b] = stats[b * kStats + 4];
        total += (double)ncc[b];
    }
    if (ncc_sum) *ncc_sum = (float)total;
    return 0;
}

}  // namespace

extern "C" {

int ddrr_wncc_abi_version(void) { return DDRR_WNCC_ABI_VERSION; }
const char *ddrr_wncc_last_error(void) { return g_err; }

long ddrr_wncc_workspace_bytes(int B, int N) {
    return (B < 1 || N < 1) ? 0 : (long)B * groups_of(N) * DDRR_WNCC_SLOT_BYTES;
}

int ddrr_wncc_forward(const float *x1, long x1_stride, const float *x2, const float *w, long w_stride, int B,
                      int N, float eps, void *ws, float *ncc, float *stats, void *) {
    return forward(false, nullptr, x2, x1, x1_stride, w, w_stride, B, N, eps, ws, ncc, stats, nullptr, nullptr);
}

int ddrr_wncc_backward(const float *x1, long x1_stride, const float *x2, const float *w, long w_stride,
                       const float *stats, const float *g_out, int g_stride, int B, int N, float *g_x1,
                       float *g_x2, void *) {
    if (!x1 || !x2 || !w || !stats || !g_out) return fail(-1, "null pointer");
    if (const char *m = check_sizes(B, N)) return fail(-1, m);
    if (const char *m = check_rows(x1_stride, w_stride, N)) return fail(-1, m);
    if (const char *m = check_g_stride(g_stride)) return fail(-1, m);
    if (g_x1 && x1_stride == 0) return fail(-1, "a shared x1 gets no gradient here");
    for (int b = 0; b < B; ++b) {
        const float *st = stats + b * kStats;
        const float gn = grad_scale(g_out[b * g_stride], st[5]);
        for (int n = 0; n < N; ++n) {
            const float a = x1[b * x1_stride + n], c = x2[(long)b * N + n], wn = w[b * w_stride + n];
            if (g_x2) g_x2[(long)b * N + n] = grad_pixel(gn, wn, a, st[0], st[1], c, st[2], st[3], st[4]);
            if (g_x1) g_x1[(long)b * N + n] = grad_pixel(gn, wn, c, st[2], st[3], a, st[0], st[1], st[4]);
        }
    }
    return 0;
}

int ddrr_wncc_siddon_forward(const float *aux, const float *img, const float *x1, long x1_stride,
                             const float *w, long w_stride, int B, int N, float eps, void *ws, float *ncc,
                             float *stats, float *out, float *ncc_sum, void *) {
    return forward(true, aux, img, x1, x1_stride, w, w_stride, B, N, eps, ws, ncc, stats, out, ncc_sum);
}

int ddrr_wncc_siddon_backward_pose(const float *aux, const float *x1, long x1_stride, const float *w,
                                   long w_stride, const float *stats, const float *g_out, int g_stride,
                                   const float *source_v, const float *Mw, const float *Ainv, const float *P,
                                   const float *rot, const float *xyz, int a0, int a1, int a2,
                                   const float *reorient34, int B, int N, float eps, int with_img_path,
                                   void *ws_raw, float *g_rot, float *g_xyz, void *) {
    if (!aux || !x1 || !w || !stats || !g_out || !source_v || !Mw || !Ainv || !P || !rot || !xyz || !reorient34 ||
        !ws_raw || !g_rot || !g_xyz)
        return fail(-1, "null pointer");
    if (const char *m = check_axes(a0, a1, a2)) return fail(-1, m);
    if (const char *m = check_sizes(B, N)) return fail(-1, m);
    if (const char *m = check_rows(x1_stride, w_stride, N)) return fail(-1, m);
    if (const char *m = check_g_stride(g_stride)) return fail(-1, m);
    if (const char *m = check_eps(eps)) return fail(-1, m);
    if (const char *m = check_ws(ws_raw)) return fail(-1, m);
    float *ws = reinterpret_cast<float *>(ws_raw);
    const int G = groups_of(N), axes[3] = {a0, a1, a2};
    for (int b = 0; b < B; ++b) {
        const float *st = stats + b * kStats;
        const float gn = grad_scale(g_out[b * g_stride], st[5]);
        for (int g = 0; g < G; ++g) {
            float acc[kGrad] = {0.f};
            const int n_end = N < (g + 1) * kGroupRays ? N : (g + 1) * kGroupRays;
            for (int n = g * kGroupRays; n < n_end; ++n) {
                float rec[8];
                ddrr::rec_blocked_load(aux, (long)b * N + n, rec);
                ray_backward(rec, source_v + b * 3, Mw + (long)b * 12, Ainv, P + n * 3, w[b * w_stride + n],
                             x1[b * x1_stride + n], st, gn, eps, with_img_path, true, acc);
            }
            for (int k = 0; k < kGrad; ++k) ws[((long)b * G + g) * kGrad + k] = acc[k];
        }
        float gM[kGrad];
        for (int k = 0; k < kGrad; ++k) {
            gM[k] = ws[(long)b * G * kGrad + k];
            for (int g = 1; g < G; ++g) gM[k] += ws[((long)b * G + g) * kGrad + k];
        }
        ddrr::pose_euler_backward(rot + b * 3, xyz + b * 3, axes, reorient34, gM, g_rot + b * 3, g_xyz + b * 3);
    }
    return 0;
}

}  // extern "C"
