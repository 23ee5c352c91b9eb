// lm_kernels.h -- the structure of the Levenberg-Marquardt kernels, written once for the four libraries (lm.hip,
// wlm.hip, mvlm.hip, wmvlm.hip): who computes what in the normal-sums kernel, the multi-view ray generation, the
// partial-sum loop of the step kernels, and the error buffer of the entries.  The arithmetic is the core headers'
// (lm_core.h and what it includes; the weighted sums come in through the `Sums` of the including library).  A
// library's .hip file holds the __global__ wrappers, which only pick what a rendered pose reads, and the entries.
//
//   normal_sums_body   one workgroup per (pose, run of 1024 rays), four rays per thread.  Everything a thread's rays
//       read -- five record planes, the fixed pixel, the detector point, with `Sums::kWeighted` the weight -- is
//       requested before the first is worked on, as in siddon_ncc_bwd_pose_kernel.  A ray is ~150 fma to its Jacobian
//       row (the record's endpoint gradients, the ray generation's adjoint, then pose_euler_backward's map from the
//       matrix gradient to the parameters -- 72 fma on 39 floats of the pose that one lane puts into LDS: the 12 x 6
//       derivative D of include/diffdrr_lm_hip.h in factored form, and the very operations the existing backward
//       entry performs); the row, x and f (8 floats) go to LDS.  The sums are the Gram matrix of those 1024 x 9 values
//       ((j, x, f, 1): all pairs but 1 * 1): 5 x Sums::kCount threads take one (sum, slice of the rays) each and add
//       their products in double in ray order, Sums::kCount threads add the five slices and write the workgroup's
//       partial.  Keeping the sums per thread instead (float accumulators over its four rays, then 44 double
//       butterflies through the wave) was tried first: 44 + 36 loaded values + a ray's temporaries came to 166
//       registers, or 128 with 84 bytes of scratch, and the butterflies alone are 528 ds_bpermute per wave.  The
//       staged form takes 106 registers, no scratch, no cross-lane traffic, and rounds nothing before the double sums.
//       Unweighted (PlainSums): 44 sums by slice_sum, two LDS reads (one a broadcast) and one v_fma_f64 per product.
//       Weighted (WeightedSums): a ninth value per ray, its weight -- one more load per ray (4 B next to the 32 B
//       record, the 4 B fixed pixel and the 12 B detector point) into a plane of its own in LDS (4 KB beside the 32 KB
//       of rows): a 36-byte row would break the two 16-byte stores of a row and put the rows of consecutive rays at
//       36-byte steps, where the plane keeps ds_write_b128 for the rows and one ds_write_b32 for the weight, and every
//       (sum, slice) thread reads the weight as a broadcast.  45 sums by wslice_sum: two v_mul_f64 and one v_add_f64
//       per product, nothing fused (include/diffdrr_wlm_hip.h); the constant 1 of u_n is read from LDS at stride 0
//       (wl[1024]), so the loop has no branch.  A ray of weight 0 stages a row of zeros and weight 0 (its fixed pixel,
//       which may be NaN, is selected out, not multiplied).
//   raygen_body        pose_ncc.hip's pose_raygen_fwd_kernel with (rot[s], xyz[s], the view's reorient and detector
//       points): one thread per ray, every workgroup works its pose's matrix out again (three sincos, 30 fma, one
//       lane, into LDS), and all of them together clear what the render behind this launch wants zeroed.
//   sum_partials       the first half of a step kernel: kCount lanes add a pose's partials in index order into LDS.
// No atomics anywhere: the results are bitwise reproducible.
#pragma once

#include <hip/hip_runtime.h>

#include <stdio.h>

#include "lm_core.h"

namespace ddrr_lm {

// ------------------------------------------------------------------------------------------------ the entries
// (one buffer per library: each is a shared object of its own)
inline thread_local char g_err[512] = "";

inline int fail(int code, const char *what) {
    snprintf(g_err, sizeof(g_err), "%s", what);
    return code;
}

inline int finish(const char *where) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "%s: %s", where, hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------ the kernels
// What rendered pose blockIdx.y reads beside its own record, matrix and source: the pose (of S) that owns its
// parameters, and its reorient, fixed image, weight (PlainSums: unused) and detector points.  Uniform in a workgroup.
struct PosePicks {
    int start;
    const float *Ro, *f, *w, *P;
};

template <class Sums>
__device__ __forceinline__ void normal_sums_body(const PosePicks pk, const float *__restrict__ aux,
                                                 const float *__restrict__ source_v, const float *__restrict__ Mw,
                                                 const float *__restrict__ Ainv, const float *__restrict__ rot,
                                                 const float *__restrict__ xyz, int a0, int a1, int a2, int N,
                                                 float eps, int with_img_path, double *__restrict__ ws,
                                                 float *__restrict__ jac) {
    constexpr bool kWeighted = Sums::kWeighted;
    constexpr int kCount = Sums::kCount;
    __shared__ __attribute__((aligned(16))) float us[kGroupRays * 8];  // (j, x, f) of the workgroup's rays
    __shared__ float wl[kWeighted ? kGroupRays + 1 : 1];               // their weights, then the constant 1
    __shared__ float pose[kPoseFloats];
    __shared__ double red[kSlices][kCount];
    const int b = blockIdx.y, st = pk.start;
    const float *M = Mw + (long)b * 12;
    const float *Ro = pk.Ro;
    const float s[3] = {source_v[b * 3], source_v[b * 3 + 1], source_v[b * 3 + 2]};
    const int n_end = min(N, (int)(blockIdx.x + 1) * kGroupRays);
    // the pose's half of pose_euler_backward (three sincos, six 3 x 3 products) by one lane of the first wave,
    // before that wave requests its rays (its eight 3 x 3 matrices are not to share the registers with 36
    // loaded values); the other three waves have their loads in flight meanwhile
    if (threadIdx.x == 0) {
        const float th[3] = {rot[st * 3], rot[st * 3 + 1], rot[st * 3 + 2]};
        const float tr[3] = {xyz[st * 3], xyz[st * 3 + 1], xyz[st * 3 + 2]};
        const int axes[3] = {a0, a1, a2};
        ddrr::PoseEulerAdjoint q;
        ddrr::pose_euler_adjoint_setup(th, tr, axes, Ro, q);
#pragma unroll
        for (int e = 0; e < 9; ++e) pose[e] = q.R[e];
#pragma unroll
        for (int e = 0; e < 3; ++e) pose[9 + e] = q.v[e];
#pragma unroll
        for (int e = 0; e < 27; ++e) pose[12 + e] = q.dR[e];
        if constexpr (kWeighted) wl[kGroupRays] = 1.f;
    }
    __builtin_amdgcn_sched_barrier(0);
    float rec[kPer][ddrr::SIDDON_AUX], fs[kPer], wv[kPer], Ps[kPer][3];
    bool in[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int n0 = blockIdx.x * kGroupRays + threadIdx.x + k * kBlock;
        in[k] = n0 < n_end;
        const int n = in[k] ? n0 : n_end - 1;  // (a ray beyond the image re-reads the last one, unused)
        ddrr::rec_blocked_load(aux, (long)b * N + n, rec[k]);
        fs[k] = pk.f[n];
        if constexpr (kWeighted) wv[k] = pk.w[n];
#pragma unroll
        for (int a = 0; a < 3; ++a) Ps[k][a] = pk.P[n * 3 + a];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        float j[6], x;
        ray_jacobian(rec[k], s, M, Ainv, Ps[k], eps, with_img_path, pose, Ro, j, x);
        const int local = threadIdx.x + k * kBlock;
        if (in[k]) {
            float4 *dst = reinterpret_cast<float4 *>(us + 8 * local);
            if constexpr (kWeighted) {
                const bool on = wv[k] != 0.f;  // (selected, not multiplied: the fixed pixel may be NaN under weight 0)
                dst[0] = on ? make_float4(j[0], j[1], j[2], j[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
                dst[1] = on ? make_float4(j[4], j[5], x, fs[k]) : make_float4(0.f, 0.f, 0.f, 0.f);
                wl[local] = wv[k];
            } else {
                dst[0] = make_float4(j[0], j[1], j[2], j[3]);
                dst[1] = make_float4(j[4], j[5], x, fs[k]);
            }
            if (jac) {
                float *out = jac + ((long)b * N + blockIdx.x * kGroupRays + local) * 6;
#pragma unroll
                for (int p = 0; p < 6; ++p) out[p] = j[p];
            }
        }
    }
    __syncthreads();
    const int count = n_end - (int)blockIdx.x * kGroupRays;
    if (threadIdx.x < kCount * kSlices)
        red[threadIdx.x / kCount][threadIdx.x % kCount] =
            Sums::slice(us, wl, count, threadIdx.x % kCount, threadIdx.x / kCount);
    __syncthreads();
    if (threadIdx.x < kCount) {
        double v = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kSlices; ++w) v += red[w][threadIdx.x];
        ws[((long)b * gridDim.x + blockIdx.x) * kCount + threadIdx.x] = v;
    }
}

// rendered pose blockIdx.y: start s with the view's reorient `Ro` and detector points `P`
__device__ __forceinline__ void raygen_body(const float *__restrict__ rot, const float *__restrict__ xyz, int a0,
                                            int a1, int a2, const float *Ro, const float *__restrict__ Ainv,
                                            const float *P, int s, int N, float *__restrict__ Mw,
                                            float *__restrict__ source_v, float *__restrict__ target_v,
                                            float *__restrict__ img, float *__restrict__ clear, long clear_n,
                                            int *__restrict__ counter) {
    __shared__ float Ms[12];
    const int b = blockIdx.y, n = blockIdx.x * kBlock + threadIdx.x;
    // what the render behind this launch has to find zeroed (its record, its brick counter)
    if (clear) {
        const long stride = (long)gridDim.x * gridDim.y * kBlock, n4 = clear_n >> 2;
        float4 *c4 = reinterpret_cast<float4 *>(clear);
        const long first = ((long)blockIdx.y * gridDim.x + blockIdx.x) * kBlock + threadIdx.x;
        for (long i = first; i < n4; i += stride) c4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (first < (clear_n & 3)) clear[(n4 << 2) + first] = 0.f;
    }
    if (counter && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 4) counter[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        const float th[3] = {rot[s * 3], rot[s * 3 + 1], rot[s * 3 + 2]};
        const float t[3] = {xyz[s * 3], xyz[s * 3 + 1], xyz[s * 3 + 2]};
        const int axes[3] = {a0, a1, a2};
        float M[12];
        ddrr::pose_euler_forward(th, t, axes, Ro, M);
#pragma unroll
        for (int k = 0; k < 12; ++k) Ms[k] = M[k];
        if (blockIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < 12; ++k) Mw[b * 12 + k] = M[k];
            const float sw[3] = {M[3], M[7], M[11]};
            float sv[3];
            ddrr::apply34(Ainv, sw, sv);
            source_v[b * 3 + 0] = sv[0];
            source_v[b * 3 + 1] = sv[1];
            source_v[b * 3 + 2] = sv[2];
        }
    }
    __syncthreads();
    if (n >= N) return;
    float M[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) M[k] = Ms[k];
    const float Pn[3] = {P[n * 3], P[n * 3 + 1], P[n * 3 + 2]};
    const ddrr::RayGenOut o = ddrr::raygen_ray(M, Ainv, Pn);
    const long r = (long)b * N + n;
    target_v[r * 3 + 0] = o.tv[0];
    target_v[r * 3 + 1] = o.tv[1];
    target_v[r * 3 + 2] = o.tv[2];
    img[r] = o.L;
}

// S[k] = the sum over the `groups` workgroups of rendered pose b of partial k, in index order, by lane k
template <int kCount>
__device__ __forceinline__ void sum_partials(const double *__restrict__ ws, long b, int groups, double *S) {
    if (threadIdx.x < kCount) {
        const double *p = ws + b * groups * kCount + threadIdx.x;
        double v = p[0];
        for (int w = 1; w < groups; ++w) v += p[(long)w * kCount];
        S[threadIdx.x] = v;
    }
}

}  // namespace ddrr_lm
