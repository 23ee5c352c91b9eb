// mi_kernels.h -- the MutualInformation kernels (reference diffdrr/metrics.py:110-139; kornia marginal_pdf /
// joint_pdf), written once for the two libraries: mi.hip (include/diffdrr_mi_hip.h) instantiates every body with
// kWeighted = false, the library with per-pixel weights (include/diffdrr_wmi_hip.h) with kWeighted = true.  A
// library's .hip file holds the __global__ wrappers, one call of a body each, and the entries.  Every difference
// between the two criteria is a `kWeighted` branch below; the unweighted instantiation carries no weight code.
//
// The reference builds (B, N, K) fp32 kernel-value tensors k1, k2 and forms the joint histogram
// J = k1^T k2 (K x K per pair) with a batched matmul.  Here the matmul runs on the fp32-input MFMA
// (v_mfma_f32_32x32x2_f32: exact f32, a k-ordered fma chain) and every operand is evaluated in
// registers from the two images -- A[i = bin][k = pixel] = k1[pixel, bin] -- so the images are the
// only bytes read.  Launches of one forward:
//   joint_body     grid (pixel chunk, 64x64 J block, pair): 4 waves share one 64 x 64 block of J
//                  (2 x 2 MFMA tiles per wave, each operand evaluated once for two MFMAs) and split
//                  the chunk's pixels; their accumulators are summed in LDS in wave order and
//                  written as that chunk's partial J.  The waves of block row / column 0 also sum
//                  their operands: the partial marginals sum_n k1[n, k], sum_n k2[n, l].
//                  Weighted: the A operand is w[n] k1[n, k], or 0 where w[n] == 0; the B operand stays k2[n, l]
//                  (0 where w[n] == 0: the images are not read there).  Both partial marginals sum w k.  Each chunk
//                  also writes its sum of the weights (in double, in pixel order per wave, then in wave order).  A
//                  k-step (2 pixels) whose weights are both 0 is skipped under a wave-uniform test: it would add
//                  exact zeros.
//   reduce_body    one thread per element of J and of the marginals: the partials summed over the
//                  chunks in chunk order, in double.  Weighted: one more element, the chunks' sums of weights
//                  (Sw per pair).
//   epilogue_body  one workgroup per pair, in double: pdfs, entropies, the value and, if a gradient
//                  will be needed, G = dL/dJ and m = dL/dP / N (the `state`).  Weighted: 1 / Sw for 1 / N; a pair
//                  with Sw == 0 gets the value 0 and an all-zero state.
// The backward is one launch, grad_body: D[n, l] = sum_k k_other[n, k] G[k, l] on the MFMA, with
// one wave per 32 columns of G holding its (K x 32) slab of G in registers (A again evaluated on the
// fly), then at the accumulator positions  -k u / sigma * (m[l] + D[n, l])  summed over l: over the
// lanes by shuffles, over the waves in LDS in wave order.  Weighted: the pixel's result times w[n], once, at the
// end; exact 0.0f where w[n] == 0 (never 0 * NaN).  A 32-pixel tile whose weights are all 0 skips the MFMA loop (the
// test is uniform over the workgroup: every wave looks at the same 32 weights).
// The launch geometry -- Kp, nb, chunks, cp of the forward, NS, waves and tpw of the backward -- does not depend on
// kWeighted, and with w = 1 everywhere every weighted result is the unweighted one bit for bit
// (tests/test_gpu_wmi.py).  Every sum is taken in a fixed order: no atomics, results are bitwise reproducible.
#pragma once

#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdio.h>

#include <type_traits>

namespace ddrr_mi {

typedef float f32x16 __attribute__((ext_vector_type(16)));

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

constexpr int kMaxBins = 256;     // DDRR_MI_MAX_BINS, DDRR_WMI_MAX_BINS
constexpr int kBlk = 64;          // J block of one forward workgroup (2 x 2 tiles of 32 x 32)
constexpr int kFwdWaves = 4;      // waves of a forward workgroup (they split the chunk's pixels)
constexpr int kTargetBlocks = 1024;  // forward workgroups aimed at (256 CUs)
constexpr int kGradTargetBlocks = 256;
constexpr int kInner = 32;        // MFMA k-steps (2 pixels each) summed in one f32 chain
constexpr int kEpiThreads = 1024;
constexpr float kExpScale = -0.72134752044448170f;  // -0.5 log2(e): k = exp2(u^2 * kExpScale)

inline int check_sizes(int B, int H, int W, int K) {
    if (B < 0 || B > 65535) return fail(-1, "B must be in [0, 65535]");
    if (H < 1 || W < 1) return fail(-1, "H and W must be >= 1");
    if ((long)H * W > INT_MAX) return fail(-1, "H W must be < 2^31");
    if (K < 1 || K > kMaxBins) return fail(-1, "num_bins must be in [1, 256]");
    return 0;
}

// (sw: the weight's stride; the unweighted entries pass 0)
inline int check_strides(long s1, long s2, long sw, int H, int W) {
    const long N = (long)H * W;
    if (s1 != 0 && s1 < N) return fail(-1, "x1_stride must be 0 or >= H W");
    if (s2 != 0 && s2 < N) return fail(-1, "x2_stride must be 0 or >= H W");
    if (sw != 0 && sw < N) return fail(-1, "w_stride must be 0 or >= H W");
    return 0;
}

// Where the pieces of the workspace and of the state live (floats), for one call's sizes.
struct Geom {
    int N, Kp, nb, chunks, cp;
    // offsets into the workspace (floats; J, P, Sw and part_W hold doubles), total floats
    long part_J, part_P, J, P, Sw, part_W, total;
};

template <bool kWeighted>
Geom geom(int B, int H, int W, int K) {
    Geom g;
    g.N = H * W;
    g.Kp = (K + kBlk - 1) / kBlk * kBlk;
    g.nb = g.Kp / kBlk;
    const long blocks = (long)B * g.nb * g.nb;
    long chunks = blocks > 0 ? (kTargetBlocks + blocks - 1) / blocks : 1;
    const long max_chunks = (g.N + 255) / 256;  // at least 256 pixels (64 per wave) per chunk
    if (chunks > max_chunks) chunks = max_chunks;
    if (chunks < 1) chunks = 1;
    // pixels per chunk: a multiple of 2 per wave (one MFMA k-step), no empty chunk
    const long per = (g.N + chunks - 1) / chunks;
    g.cp = (int)((per + 2 * kFwdWaves - 1) / (2 * kFwdWaves) * (2 * kFwdWaves));
    g.chunks = (g.N + g.cp - 1) / g.cp;
    const long KK = (long)g.Kp * g.Kp;
    g.part_J = 0;
    g.part_P = g.part_J + (long)B * g.chunks * KK;
    g.J = g.part_P + (long)B * g.chunks * 2 * g.Kp;
    g.P = g.J + 2 * (long)B * KK;
    g.Sw = g.P + 2 * (long)B * 2 * g.Kp;  // (the unweighted workspace ends here; every offset so far is even)
    g.part_W = g.Sw + (kWeighted ? 2 * (long)B : 0);
    g.total = g.part_W + (kWeighted ? 2 * (long)B * g.chunks : 0);
    return g;
}

inline long state_floats(int K) {
    const long Kp = (K + kBlk - 1) / kBlk * kBlk;
    return Kp * Kp + 2 * Kp;  // G (Kp x Kp), m1 (Kp), m2 (Kp)
}

// The backward's launch: grid (chunks, B), 64 * nbw threads, tpw tiles of 32 pixels per workgroup; xo / xt are the
// other and the differentiated image, `transpose` and `m_offset` pick G or G^T and m1 or m2 of the state.
struct GradGeom {
    int N, Kp, tpw, chunks, nbw, transpose, m_offset;
    const float *xo, *xt;
    long so, st, SS;
};

inline GradGeom grad_geom(const float *x1, long s1, const float *x2, long s2, int B, int H, int W, int K, int which) {
    GradGeom q;
    q.N = H * W;
    q.Kp = (K + kBlk - 1) / kBlk * kBlk;
    const int ntiles = (q.N + 31) / 32;
    const long tpw_l = ((long)ntiles * B + kGradTargetBlocks - 1) / kGradTargetBlocks;
    q.tpw = (int)(tpw_l < 1 ? 1 : tpw_l);
    q.chunks = (ntiles + q.tpw - 1) / q.tpw;
    q.nbw = (K + 31) / 32;
    q.xo = which ? x1 : x2, q.xt = which ? x2 : x1;
    q.so = which ? s1 : s2, q.st = which ? s2 : s1;
    q.transpose = which ? 0 : 1, q.m_offset = which ? q.Kp : 0;
    q.SS = state_floats(K);
    return q;
}

// launch(std::integral_constant<int, NS>): NS = the MFMA k-steps (2 bins each) of the grad kernel for K bins
template <class Launch>
void dispatch_ns(int K, Launch &&launch) {
    if (K <= 2) launch(std::integral_constant<int, 1>());
    else if (K <= 8) launch(std::integral_constant<int, 4>());
    else if (K <= 32) launch(std::integral_constant<int, 16>());
    else if (K <= 64) launch(std::integral_constant<int, 32>());
    else if (K <= 128) launch(std::integral_constant<int, 64>());
    else launch(std::integral_constant<int, 128>());
}

// ------------------------------------------------------------------------------------------------ the kernels
__device__ __forceinline__ float kernel_value(float x, float bin, float inv_sigma) {
    const float u = (x - bin) * inv_sigma;
    return __builtin_amdgcn_exp2f(u * u * kExpScale);
}

// ------------------------------------------------------------------------------------------ forward
// (wt, sw, part_W: kWeighted only)
template <bool kWeighted>
__device__ __forceinline__ void joint_body(const float *__restrict__ x1, long s1, const float *__restrict__ x2,
                                           long s2, const float *__restrict__ wt, long sw, int N,
                                           const float *__restrict__ bins, int K, const float *__restrict__ sigma,
                                           int Kp, int nb, int chunks, int cp, float *__restrict__ part_J,
                                           float *__restrict__ part_P, double *__restrict__ part_W) {
    __shared__ float lacc[kFwdWaves - 1][kBlk * kBlk];   // waves 1..3's accumulators
    __shared__ float lmarg[kFwdWaves][2][2][kBlk];       // [wave][P1, P2][lane half][bin]
    __shared__ double lsw[kWeighted ? kFwdWaves : 1][2];  // [wave][lane half]: sums of the weights
    const int c = blockIdx.x, bi = blockIdx.y / nb, bj = blockIdx.y % nb, b = blockIdx.z;
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, h = l >> 5, r = l & 31;
    const float is = 1.0f / sigma[0];
    float brow[2], bcol[2];
    bool vrow[2], vcol[2];
#pragma unroll
    for (int f = 0; f < 2; ++f) {
        const int kr = bi * kBlk + f * 32 + r, kc = bj * kBlk + f * 32 + r;
        vrow[f] = kr < K;
        vcol[f] = kc < K;
        brow[f] = vrow[f] ? bins[kr] : 0.0f;
        bcol[f] = vcol[f] ? bins[kc] : 0.0f;
    }
    const float *a = x1 + b * s1;
    const float *bb = x2 + b * s2;
    const float *wb = kWeighted ? wt + b * sw : nullptr;
    const int quarter = cp / kFwdWaves;
    const int p0 = c * cp + w * quarter;
    const int p1 = min(p0 + quarter, N);
    // two levels of f32 sums: the MFMA accumulates at most kInner k-steps, then the run is added into
    // `acc` (the gradient of MI is a small difference of large terms: it amplifies the rounding of J by
    // ~10^2, and a chain of thousands of f32 adds would show)
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
    float m1[2] = {0.0f, 0.0f}, m2[2] = {0.0f, 0.0f};
    double wsum = 0.0;  // of this lane half's pixels (the 32 lanes of a half hold the same sum)
    for (int s0 = p0; s0 < p1; s0 += 2 * kInner) {
        const int s_end = min(s0 + 2 * kInner, p1);
        f32x16 run[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) run[i][j][e] = 0.0f;
        float r1[2] = {0.0f, 0.0f}, r2[2] = {0.0f, 0.0f};
        for (int s = s0; s < s_end; s += 2) {
            const int n = s + h;
            bool vn = n < s_end;
            float wn = 1.0f;
            if constexpr (kWeighted) {
                wn = vn ? wb[n] : 0.0f;
                vn = wn != 0.0f;           // (in the chunk and in V: the images are read nowhere else)
                if (!__any(vn)) continue;  // both pixels of the k-step are masked: it would add exact zeros
                wsum += (double)wn;
            }
            const float xa = vn ? a[n] : 0.0f, xb = vn ? bb[n] : 0.0f;
            float A[2], Bv[2];
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                const float k1 = kernel_value(xa, brow[f], is);
                A[f] = (vn && vrow[f]) ? (kWeighted ? wn * k1 : k1) : 0.0f;
                Bv[f] = (vn && vcol[f]) ? kernel_value(xb, bcol[f], is) : 0.0f;
                r1[f] += A[f];
                r2[f] += kWeighted ? wn * Bv[f] : Bv[f];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    run[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[i], Bv[j], run[i][j], 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] += run[i][j];
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            m1[f] += r1[f];
            m2[f] += r2[f];
        }
    }
    // C/D map of the 32x32 tiles: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    if (w > 0) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    lacc[w - 1][(i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h) * kBlk + j * 32 + r] = acc[i][j][e];
    }
#pragma unroll
    for (int f = 0; f < 2; ++f) {
        lmarg[w][0][h][f * 32 + r] = m1[f];
        lmarg[w][1][h][f * 32 + r] = m2[f];
    }
    if constexpr (kWeighted)
        if (r == 0) lsw[w][h] = wsum;
    __syncthreads();
    const long KK = (long)Kp * Kp;
    if (w == 0) {
        float *pj = part_J + ((long)b * chunks + c) * KK;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int row = i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h, col = j * 32 + r;
                    float v = acc[i][j][e];
#pragma unroll
                    for (int q = 0; q < kFwdWaves - 1; ++q) v += lacc[q][row * kBlk + col];
                    pj[(long)(bi * kBlk + row) * Kp + bj * kBlk + col] = v;
                }
    } else if (w == 1) {
        // marginals: P1 from the blocks of column 0, P2 from those of row 0 (lane = bin of the block)
        float *pp = part_P + ((long)b * chunks + c) * 2 * Kp;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            if ((q == 0 && bj != 0) || (q == 1 && bi != 0)) continue;
            float v = 0.0f;
#pragma unroll
            for (int ww = 0; ww < kFwdWaves; ++ww) v += lmarg[ww][q][0][l] + lmarg[ww][q][1][l];
            pp[q * Kp + (q == 0 ? bi : bj) * kBlk + l] = v;
        }
    } else if (kWeighted && w == 2 && l == 0 && bi == 0 && bj == 0) {
        double v = 0.0;
#pragma unroll
        for (int ww = 0; ww < kFwdWaves; ++ww) v += lsw[ww][0] + lsw[ww][1];
        part_W[(long)b * chunks + c] = v;
    }
}

// (in double: J and the marginals are what the pdfs -- and through log2 the gradient -- are formed from)
// (part_W, Sw, weight_sum: kWeighted only -- one more element, the pair's sum of weights)
template <bool kWeighted>
__device__ __forceinline__ void reduce_body(const float *__restrict__ part_J, const float *__restrict__ part_P,
                                            const double *__restrict__ part_W, int chunks, int Kp,
                                            double *__restrict__ J, double *__restrict__ P, double *__restrict__ Sw,
                                            double *__restrict__ weight_sum) {
    const int b = blockIdx.y;
    const long KK = (long)Kp * Kp;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= KK + 2 * Kp + (kWeighted ? 1 : 0)) return;
    double v = 0.0;
    if (kWeighted && e == KK + 2 * Kp) {
        for (int c = 0; c < chunks; ++c) v += part_W[(long)b * chunks + c];
        Sw[b] = v;
        if (weight_sum) weight_sum[b] = v;
    } else if (e < KK) {
        const float *src = part_J + (long)b * chunks * KK + e;
        for (int c = 0; c < chunks; ++c) v += src[(long)c * KK];
        J[(long)b * KK + e] = v;
    } else {
        const long e2 = e - KK;
        const float *src = part_P + (long)b * chunks * 2 * Kp + e2;
        for (int c = 0; c < chunks; ++c) v += src[(long)c * 2 * Kp];
        P[(long)b * 2 * Kp + e2] = v;
    }
}

// Sum of three doubles over the workgroup, in a fixed order; every thread gets the sums.
__device__ __forceinline__ void block_sum3(double &a, double &b, double &c, double (*red)[3]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o);
        b += __shfl_xor(b, o);
        c += __shfl_xor(c, o);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[w][0] = a;
        red[w][1] = b;
        red[w][2] = c;
    }
    __syncthreads();
    a = b = c = 0.0;
    for (int q = 0; q < kEpiThreads / 64; ++q) {
        a += red[q][0];
        b += red[q][1];
        c += red[q][2];
    }
    __syncthreads();
}

// One log2 per element: the pass that forms the entropies also forms sum_k dent(p_k) p_k and, when a
// gradient will be needed, leaves dent(pJ) in place of J (the workspace) for the pass that writes G; every
// thread reads back only what it wrote itself.  (Sw: kWeighted only, in place of N)
template <bool kWeighted>
__device__ __forceinline__ void epilogue_body(double *__restrict__ J, const double *__restrict__ P,
                                              const double *__restrict__ Sw, int K, int Kp, int N, float epsilon,
                                              int normalize, float *__restrict__ out, float *__restrict__ state,
                                              long SS) {
    __shared__ double red[kEpiThreads / 64][3];
    const int b = blockIdx.x, t = threadIdx.x;
    const long KK = (long)Kp * Kp;
    if constexpr (kWeighted) {
        if (Sw[b] == 0.0) {  // (uniform over the workgroup) an empty pair: the value 0, no gradient
            if (t == 0) out[b] = 0.0f;
            if (state)
                for (long e = t; e < SS; e += kEpiThreads) state[b * SS + e] = 0.0f;
            return;
        }
    }
    double *Jb = J + b * KK;
    const double *P1 = P + (long)b * 2 * Kp, *P2 = P1 + Kp;
    // (`invN`: 1 / Sw under weights, which is 1 / N when w = 1 everywhere)
    const double eps = epsilon, invN = kWeighted ? 1.0 / Sw[b] : 1.0 / N, inv_ln2 = 1.4426950408889634;
    const int KK_real = K * K;
    double sJ = 0.0, s1 = 0.0, s2 = 0.0;
    for (int e = t; e < KK_real; e += kEpiThreads) sJ += Jb[(long)(e / K) * Kp + e % K];
    for (int k = t; k < K; k += kEpiThreads) {
        s1 += P1[k] * invN;
        s2 += P2[k] * invN;
    }
    block_sum3(sJ, s1, s2, red);
    const double nJ = 1.0 / (sJ + 1e-10), n1 = 1.0 / (s1 + eps), n2 = 1.0 / (s2 + eps);
    // entropies H = -sum p log2(p + eps) and, for the gradient, sum dent(p) p with
    // dent(p) = d(-p log2(p + eps)) / dp = -(log2(p + eps) + p / ((p + eps) ln 2))
    double h1 = 0.0, h2 = 0.0, h12 = 0.0, d1 = 0.0, d2 = 0.0, dJ = 0.0;
    for (int e = t; e < KK_real; e += kEpiThreads) {
        const long i = (long)(e / K) * Kp + e % K;
        const double p = Jb[i] * nJ, lg = log2(p + eps), de = -(lg + p / (p + eps) * inv_ln2);
        h12 -= p * lg;
        dJ += de * p;
        if (state) Jb[i] = de;
    }
    for (int k = t; k < K; k += kEpiThreads) {
        const double p = P1[k] * invN * n1, q = P2[k] * invN * n2;
        const double lp = log2(p + eps), lq = log2(q + eps);
        h1 -= p * lp;
        h2 -= q * lq;
        d1 -= (lp + p / (p + eps) * inv_ln2) * p;
        d2 -= (lq + q / (q + eps) * inv_ln2) * q;
    }
    block_sum3(h1, h2, h12, red);
    block_sum3(d1, d2, dJ, red);
    double mi = h1 + h2 - h12;
    if (normalize) mi = 2.0 * mi / (h1 + h2);
    if (t == 0) out[b] = (float)mi;
    if (!state) return;
    // dL/dH1 = dL/dH2 = a1, dL/dH12 = a12; c = dL/dp = a dent(p); then through p = P / (S + eps):
    // dL/dP_j = (c_j - sum_k c_k p_k) / (S + eps)
    double a1 = 1.0, a12 = -1.0;
    if (normalize) {
        const double d = h1 + h2;
        a1 = 2.0 * h12 / (d * d);
        a12 = -2.0 / d;
    }
    float *G = state + b * SS, *m1 = G + KK, *m2 = m1 + Kp;
    for (int e = t; e < KK_real; e += kEpiThreads) {
        const long i = (long)(e / K) * Kp + e % K;
        G[i] = (float)(a12 * (Jb[i] - dJ) * nJ);
    }
    for (long e = t; e < KK; e += kEpiThreads)  // padding bins: no gradient
        if (e / Kp >= K || e % Kp >= K) G[e] = 0.0f;
    for (int k = t; k < Kp; k += kEpiThreads) {
        double v1 = 0.0, v2 = 0.0;
        if (k < K) {
            const double p = P1[k] * invN * n1, q = P2[k] * invN * n2;
            const double dp = -(log2(p + eps) + p / (p + eps) * inv_ln2), dq = -(log2(q + eps) + q / (q + eps) * inv_ln2);
            v1 = a1 * (dp - d1) * n1 * invN;
            v2 = a1 * (dq - d2) * n2 * invN;
        }
        m1[k] = (float)v1;
        m2[k] = (float)v2;
    }
}

// ----------------------------------------------------------------------------------------- backward
// grad[b, n] = g[b] * sum_l (-k_t[n,l] u_t[n,l] / sigma) (m_t[l] + sum_k k_o[n,k] G_ot[k,l]),
// t = the differentiated image, o = the other one; G_ot = G (t = x2) or G^T (t = x1).
// One wave per 32 columns l (blockDim = 64 * ceil(K / 32)); NS = MFMA k-steps (2 bins each) >= K / 2.
// (wt, sw: kWeighted only)
template <int NS, bool kWeighted>
__device__ __forceinline__ void grad_body(const float *__restrict__ xo, long so, const float *__restrict__ xt,
                                          long st, const float *__restrict__ wt, long sw, int N,
                                          const float *__restrict__ bins, int K, const float *__restrict__ sigma,
                                          const float *__restrict__ state, long SS, int Kp, int transpose,
                                          int m_offset, const float *__restrict__ g_out, int g_stride, int tpw,
                                          float *__restrict__ grad) {
    __shared__ float lbins[2 * NS];
    __shared__ float lred[8][32];
    const int nbw = blockDim.x >> 6, w = threadIdx.x >> 6, l = threadIdx.x & 63, h = l >> 5, r = l & 31;
    const int c = blockIdx.x, b = blockIdx.y;
    for (int k = threadIdx.x; k < 2 * NS; k += blockDim.x) lbins[k] = k < K ? bins[k] : 0.0f;
    const float is = 1.0f / sigma[0];
    const float *G = state + b * SS;
    const float *m = G + (long)Kp * Kp + m_offset;
    const int j = w * 32 + r;
    const bool vj = j < K;
    const float binj = vj ? bins[j] : 0.0f, mj = vj ? m[j] : 0.0f;
    float gb[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int k = 2 * s + h;
        gb[s] = (vj && k < K) ? G[transpose ? (long)j * Kp + k : (long)k * Kp + j] : 0.0f;
    }
    __syncthreads();
    const float g = g_out[g_stride ? b : 0];
    const float *xob = xo + b * so, *xtb = xt + b * st, *wb = kWeighted ? wt + b * sw : nullptr;
    float *gradb = grad + (long)b * N;
    const int ntiles = (N + 31) / 32;
    const int t0 = c * tpw, t1 = min(t0 + tpw, ntiles);
    for (int tile = t0; tile < t1; ++tile) {
        const int n0 = tile * 32;
        const int na = n0 + r;
        bool va = na < N;
        float wa = 1.0f;
        if constexpr (kWeighted) {
            wa = va ? wb[na] : 0.0f;  // (every wave of the workgroup holds the same 32 weights)
            va = wa != 0.0f;
            if (!__any(va)) {         // a tile of masked pixels: exact zeros, no MFMA loop
                if (threadIdx.x < 32 && na < N) gradb[na] = 0.0f;
                continue;
            }
        }
        const float xa = va ? xob[na] : 0.0f;
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
#pragma unroll
        for (int s = 0; s < NS; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(kernel_value(xa, lbins[2 * s + h], is), gb[s], acc, 0, 0, 0);
        float part[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int p = n0 + (e & 3) + 8 * (e >> 2) + 4 * h;
            const float xv = p < N ? xtb[p] : 0.0f;
            const float u = (xv - binj) * is;
            const float kt = __builtin_amdgcn_exp2f(u * u * kExpScale);
            float v = vj ? -kt * u * is * (mj + acc[e]) : 0.0f;
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o);  // (within a 32-lane half)
            part[e] = v;
        }
        if (r == 0) {
#pragma unroll
            for (int e = 0; e < 16; ++e) lred[w][(e & 3) + 8 * (e >> 2) + 4 * h] = part[e];
        }
        __syncthreads();
        if (threadIdx.x < 32) {
            const int p = n0 + threadIdx.x;
            if (p < N) {
                float v = 0.0f;
                for (int q = 0; q < nbw; ++q) v += lred[q][threadIdx.x];
                if constexpr (kWeighted)
                    gradb[p] = va ? g * v * wa : 0.0f;  // (p = na here; x1, x2 may hold NaN under w == 0)
                else
                    gradb[p] = g * v;
            }
        }
        __syncthreads();
    }
}

}  // namespace ddrr_mi
