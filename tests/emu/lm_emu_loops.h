// The loops of the gfx950 Levenberg-Marquardt kernels (csrc/lm_kernels.h) over poses, workgroups, rays and slices on
// the host, one element at a time, the sums in the kernels' order: written once for the four host builds
// (lm_emu.cpp, wlm_emu.cpp, mvlm_emu.cpp, wmvlm_emu.cpp), as the kernels are for the four libraries.  The arithmetic
// is the core headers' own; `Sums` is csrc/lm_core.h's PlainSums or csrc/wlm_core.h's WeightedSums, and `picks(b)`
// says what rendered pose b reads, as the __global__ wrappers do.  No HIP, no GPU.
#pragma once

#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../diffdrr_amd/csrc/lm_core.h"

namespace ddrr_lm {

inline thread_local char g_err[512] = "";

inline int fail(int code, const char *what) {
    snprintf(g_err, sizeof(g_err), "%s", what);
    return code;
}

// csrc/lm_kernels.h's PosePicks
struct PosePicks {
    int start;
    const float *Ro, *f, *w, *P;
};

// normal_sums_body for rendered poses 0 .. B - 1
template <class Sums, class Picks>
void emu_normal_sums(int B, Picks picks, const float *aux, const float *source_v, const float *Mw, const float *Ainv,
                     const float *rot, const float *xyz, int a0, int a1, int a2, int N, float eps, int with_img_path,
                     double *ws, float *jac) {
    constexpr int kCount = Sums::kCount;
    const int G = (N + kGroupRays - 1) / kGroupRays, axes[3] = {a0, a1, a2};
    std::vector<float> us((size_t)kGroupRays * 8), wl((size_t)kGroupRays + 1);
    wl[kGroupRays] = 1.f;  // (the constant 1 behind the weights)
    for (int b = 0; b < B; ++b) {
        const PosePicks pk = picks(b);
        ddrr::PoseEulerAdjoint q;
        ddrr::pose_euler_adjoint_setup(rot + pk.start * 3, xyz + pk.start * 3, axes, pk.Ro, q);
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
                ray_jacobian(rec, source_v + b * 3, Mw + (long)b * 12, Ainv, pk.P + n * 3, eps, with_img_path, pose,
                             pk.Ro, j, x);
                bool on = true;
                if constexpr (Sums::kWeighted) {
                    wl[i] = pk.w[n];
                    on = wl[i] != 0.f;  // (selected, not multiplied)
                }
                for (int p = 0; p < 6; ++p) u[p] = on ? j[p] : 0.f;
                u[6] = on ? x : 0.f;
                u[7] = on ? pk.f[n] : 0.f;
                if (jac)
                    for (int p = 0; p < 6; ++p) jac[((long)b * N + n) * 6 + p] = j[p];
            }
            for (int k = 0; k < kCount; ++k) {
                double t = Sums::slice(us.data(), wl.data(), count, k, 0);
                for (int sl = 1; sl < kSlices; ++sl) t += Sums::slice(us.data(), wl.data(), count, k, sl);
                ws[((long)b * G + g) * kCount + k] = t;
            }
        }
    }
}

// raygen_body for the S * V rendered poses: `P_of(v)` is view v's detector points
template <class PointsOf>
void emu_raygen(const float *rot, const float *xyz, int a0, int a1, int a2, const float *reorient_v,
                const float *Ainv, PointsOf P_of, int S, int V, int N, float *Mw, float *source_v, float *target_v,
                float *img, float *clear, long clear_floats, void *clear_launch_ws) {
    if (clear_floats > 0) memset(clear, 0, (size_t)clear_floats * sizeof(float));
    if (clear_launch_ws) memset(clear_launch_ws, 0, 16);
    const int axes[3] = {a0, a1, a2};
    for (int b = 0; b < S * V; ++b) {
        const int s = b / V, v = b - s * V;
        const float *P = P_of(v);
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
}

// sum_partials for rendered pose b
template <int kCount>
void emu_sum_partials(const double *ws, long b, int G, double *S) {
    for (int k = 0; k < kCount; ++k) {
        double t = ws[b * G * kCount + k];
        for (int g = 1; g < G; ++g) t += ws[(b * G + g) * kCount + k];
        S[k] = t;
    }
}

}  // namespace ddrr_lm
