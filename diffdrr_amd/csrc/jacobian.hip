// jacobian.hip -- the kernels of the Jacobian determinant of a lattice deformation, its statistics, the
// volume-preservation penalty and the lattice gradient of both: the C ABI of include/diffdrr_jacobian_hip.h
// (libdiffdrr_jacobian_hip.so).  The arithmetic is jacobian_core.h's; what is here is who computes what.  No
// kernel forms a 64-tap sum per voxel, none writes a dense field or a dense derivative, none uses an atomic.
//
// A workgroup of 256 threads owns four volume rows (x, y .. y + 3), one wave each, and of each row a chunk of
// 256 z voxels (bspline.hip's scheme).  A wave first collapses x and y for its row: nine lines, (w_x w_y,
// w'_x w_y, w_x w'_y) times three components, one value per z node the chunk reaches, into LDS as floats
// [line][node], sized by the most nodes a chunk of the shape reaches (line_stride: dynamic LDS, so a coarse
// lattice keeps the occupancy its registers allow).  A voxel's J is then 2 (linear) or 4 (B-spline) taps of
// each line: lanes read the same word or consecutive words.
//
//   jacobian_forward_kernel<basis>  lane l takes the run of four z voxels from 4 l of the chunk; with a map it
//       stores d (16 bytes where Dz is a multiple of 4), without one it adds psi(d); either way the workgroup
//       reduces (psi sum, folded, min, max) -- a butterfly over each wave's lanes, then the four waves in
//       order -- and writes one partial.
//   jacobian_fold_kernel            one workgroup: thread t the partials t, t + 256, ... ascending, the same
//       reduction.
//   jacobian_rows_kernel            first gather of the B-spline gradient.  A workgroup of 128 threads walks its
//       two rows chunk by chunk: lane l takes voxels l, l + 64, l + 128, l + 192 and writes their nine c_ab to
//       LDS next to the chunk's folded z weights and derivative weights; lane 4 s + a carries the three chains
//       of component a of the nodes n = s mod 16, continued from chunk to chunk through r1.
//   jacobian_gather_kernel          second and third gather: one thread per output value, lanes along z nodes.
//   jacobian_pieces_kernel, jacobian_nodes_kernel  the linear gradient: warp.hip's (cell, piece) workgroups with
//       the cell's 24 lattice values uniform over the workgroup, then per node the pieces of its cells.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include "jacobian_core.h"

namespace {

using namespace ddrr_jacobian;
using ddrr_warp::kRedStride;
using ddrr_warp::kSlices;
using ddrr_warp::node_sum;
using ddrr_warp::slice_sum;

thread_local char g_err[512] = "";

int fail(int code, const char *what) {
    snprintf(g_err, sizeof(g_err), "%s", what);
    return code;
}

int finish(const char *where) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "%s: %s", where, hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

// the wave's lines for the chunk's span into L; every lane of the wave calls it
template <int BASIS>
__device__ __forceinline__ void fill_lines(const float *__restrict__ disp, const Shape &s, const Taps &tx,
                                           const Taps &ty, Span span, int lane, int stride, float *L) {
    const int tasks = 3 * (span.hi - span.lo + 1);
    for (int v = lane; v < tasks; v += kLanes) fill_task<BASIS>(disp, s, tx, ty, span, v, stride, L);
}

// the workgroup's partial into red[0]: per wave the butterfly over lanes 32, 16, .. 1 apart (lane 0 ends with the
// tree of tree_level over the wave's 64), then wave 0 .. 3 in order; every thread calls it
__device__ __forceinline__ void reduce_workgroup(Partial mine, Partial *red) {
    for (int off = kLanes / 2; off > 0; off >>= 1) {
        Partial other;
        other.sum = __shfl_xor(mine.sum, off);
        other.count = __shfl_xor(mine.count, off);
        other.lo = __shfl_xor(mine.lo, off);
        other.hi = __shfl_xor(mine.hi, off);
        merge(mine, other);
    }
    if (threadIdx.x % kLanes == 0) red[threadIdx.x / kLanes] = mine;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kRows; ++w) merge(red[0], red[w]);
}

template <int BASIS>
__global__ __launch_bounds__(kBlock, 4) void jacobian_forward_kernel(const float *__restrict__ disp, Shape s,
                                                                  float *__restrict__ det, int vec, int penalty,
                                                                  double eps, int stride,
                                                                  Partial *__restrict__ partials) {
    extern __shared__ float lines[];  // [row][line][stride]
    __shared__ Partial red[kRows];
    const int wave = threadIdx.x / kLanes, lane = threadIdx.x % kLanes;
    const int x = blockIdx.z, y = blockIdx.y * kRows + wave, zlo = blockIdx.x * kChunk;
    const int zend = zlo + kChunk < s.D[2] ? zlo + kChunk : s.D[2];
    const bool row = y < s.D[1];
    const Span span = chunk_span<BASIS>(zlo, zend, s.D[2], s.G[2]);
    float *L = lines + wave * kLines * stride;
    if (row)
        fill_lines<BASIS>(disp, s, taps_of<BASIS>(x, s.D[0], s.G[0]), taps_of<BASIS>(y, s.D[1], s.G[1]), span, lane,
                          stride, L);
    __syncthreads();
    Partial mine = no_voxels();
    const int z0 = zlo + 4 * lane;
    if (row && z0 < zend) {
        float sc[3], out[4];
        scales_of(s, sc);
        forward_run<BASIS>(s, L, stride, span.lo, z0, sc, penalty != 0, eps, out, mine);
        if (det) {
            float *dst = det + ((long)x * s.D[1] + y) * s.D[2] + z0;
            if (vec) {
                *reinterpret_cast<float4 *>(dst) = make_float4(out[0], out[1], out[2], out[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (z0 + k < s.D[2]) dst[k] = out[k];
            }
        }
    }
    reduce_workgroup(mine, red);
    if (threadIdx.x == 0) partials[((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = red[0];
}

__global__ __launch_bounds__(kBlock) void jacobian_fold_kernel(const Partial *__restrict__ partials, long groups,
                                                               double inv_n, double *__restrict__ penalty,
                                                               long *__restrict__ folded, float *__restrict__ range) {
    __shared__ Partial red[kRows];
    Partial mine = no_voxels();
    for (long i = threadIdx.x; i < groups; i += kBlock) merge(mine, partials[i]);
    reduce_workgroup(mine, red);
    if (threadIdx.x == 0) {
        if (penalty) *penalty = red[0].sum * inv_n;
        *folded = red[0].count;
        range[0] = red[0].lo;
        range[1] = red[0].hi;
    }
}

__global__ __launch_bounds__(kGradBlock) void jacobian_rows_kernel(const float *__restrict__ disp, Shape s,
                                                                   const float *__restrict__ gD, float eps,
                                                                   float inv_n, int stride, float *r1) {
    extern __shared__ float lines[];  // [row][line][stride]
    __shared__ float cab[kGradRows][kRowFloats];  // the nine c_ab of a chunk's voxels, padded
    __shared__ float wz[4][kPadded], dz[4][kPadded];
    const int wave = threadIdx.x / kLanes, lane = threadIdx.x % kLanes;
    const int x = blockIdx.y, y = blockIdx.x * kGradRows + wave;
    const bool row = y < s.D[1];
    const long at = ((long)x * s.D[1] + y) * s.D[2];
    const int a = lane & 3, slot = lane >> 2;
    const long plane = plane1_floats(s);
    float *mine = r1 + (((long)(a < 3 ? a : 0) * s.D[0] + x) * s.D[1] + y) * s.G[2];  // r1[0, a, x, y, .]
    float sc[3], *L = lines + wave * kLines * stride;
    scales_of(s, sc);
    int done = -1;  // the last node an earlier chunk reached
    for (int zlo = 0; zlo < s.D[2]; zlo += kChunk) {
        const int zend = zlo + kChunk < s.D[2] ? zlo + kChunk : s.D[2];
        const Span span = chunk_span<BSPLINE>(zlo, zend, s.D[2], s.G[2]);
        if (row)  // (the taps are formed per chunk: two sets of double weights are not kept across the loop)
            fill_lines<BSPLINE>(disp, s, taps_of<BSPLINE>(x, s.D[0], s.G[0]), taps_of<BSPLINE>(y, s.D[1], s.G[1]), span,
                                lane, stride, L);
        for (int zi = threadIdx.x; zlo + zi < zend; zi += kGradBlock) {
            float w[4], d[4];
            node_weights(zlo + zi, s.D[2], s.G[2], w, d);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                wz[k][padded(zi)] = w[k];
                dz[k][padded(zi)] = d[k];
            }
        }
        __syncthreads();
        if (row) {
#pragma unroll 1
            for (int zi = lane; zlo + zi < zend; zi += kLanes) {
                float c[9];
                voxel_c<BSPLINE>(s, L, stride, span.lo, zlo + zi, at + zlo + zi, sc, gD, eps, inv_n, c);
#pragma unroll
                for (int e = 0; e < 9; ++e) cab[wave][e * kPadded + padded(zi)] = c[e];
            }
        }
        __syncthreads();
        const int nlo = span.lo < 0 ? 0 : span.lo, nhi = span.hi > s.G[2] - 1 ? s.G[2] - 1 : span.hi;
        if (row && a < 3) {
            for (int n = nlo + ((slot - nlo) & (kSlots - 1)); n <= nhi; n += kSlots) {
                const bool first = n > done;
#pragma unroll 1
                for (int b = 0; b < 3; ++b) {  // c_ax and c_ay with w, c_az with w'
                    float *dst = mine + b * plane + n;
                    *dst = node_chain(cab[wave] + (3 * a + b) * kPadded, b < 2 ? wz[0] : dz[0], s.D[2], s.G[2], n, zlo,
                                      zend, first ? 0.f : *dst);
                }
            }
        }
        done = nhi;
        __syncthreads();
    }
}

// out[o, m, i] = the chain of node m of an axis of D voxels over (srcD, srcW)[o, ., i]; `count` values
__global__ __launch_bounds__(kBlock) void jacobian_gather_kernel(const float *__restrict__ srcD,
                                                                 const float *__restrict__ srcW, int D, int G,
                                                                 long inner, long count, float *__restrict__ out) {
    const long e = (long)blockIdx.x * kBlock + threadIdx.x;
    if (e >= count) return;
    const long om = e / inner, i = e - om * inner, o = om / G, base = o * D * inner + i;
    out[e] = gather_pair(srcD ? srcD + base : nullptr, srcW + base, inner, D, G, (int)(om - o * G));
}

__global__ __launch_bounds__(kBlock, 4) void jacobian_pieces_kernel(const float *__restrict__ disp, Shape s,
                                                                 const float *__restrict__ gD, float eps, float inv_n,
                                                                 unsigned pieces, float *__restrict__ ws) {
    __shared__ float red[kPieceFloats * kRedStride];
    __shared__ float part[kSlices][kPieceFloats];
    const unsigned cell = blockIdx.x / pieces, piece = blockIdx.x - cell * pieces;
    const unsigned gz = (unsigned)(s.G[2] - 1), gy = (unsigned)(s.G[1] - 1);
    const unsigned cxy = cell / gz;
    const int cz = (int)(cell - cxy * gz), cx = (int)(cxy / gy), cy = (int)(cxy - (unsigned)cx * gy);
    float acc[kPieceFloats];
    piece_thread(s, disp, gD, eps, inv_n, cx, cy, cz, piece, threadIdx.x, acc);
#pragma unroll
    for (int e = 0; e < kPieceFloats; ++e) red[e * kRedStride + threadIdx.x] = acc[e];
    __syncthreads();
    if (threadIdx.x < kPieceFloats * kSlices) {
        const int e = threadIdx.x % kPieceFloats, sl = threadIdx.x / kPieceFloats;
        part[sl][e] = slice_sum(red + e * kRedStride, sl);
    }
    __syncthreads();
    if (threadIdx.x < kPieceFloats) {
        float v = part[0][threadIdx.x];
#pragma unroll
        for (int sl = 1; sl < kSlices; ++sl) v += part[sl][threadIdx.x];
        ws[(long)blockIdx.x * kPieceFloats + threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(kBlock) void jacobian_nodes_kernel(const float *__restrict__ ws, Shape s, long pieces,
                                                                float *__restrict__ gU) {
    const long nodes = (long)s.G[0] * s.G[1] * s.G[2];
    const long e = (long)blockIdx.x * kBlock + threadIdx.x;
    if (e >= 3 * nodes) return;
    const int a = (int)(e / nodes);
    const long n = e - a * nodes;
    const long nxy = n / s.G[2];
    const int k = (int)(n - nxy * s.G[2]), i = (int)(nxy / s.G[1]), j = (int)(nxy - (long)i * s.G[1]);
    gU[e] = node_sum(ws, s, pieces, a, i, j, k);
}

// the checks every entry with a workspace shares; 0, or -1 with the message set
int check(const Shape &s, int basis, const void *ws, long ws_bytes) {
    const char *what = argument_error(s, basis);
    if (what) return fail(-1, what);
    const long need = workspace_bytes(s, basis);
    if (need < 0) return fail(-1, "more than 2^31 - 1 (cell, piece) workgroups: the lattice is too fine");
    if (ws_bytes < need) return fail(-1, "ws_bytes is smaller than ddrr_jacobian_workspace_bytes");
    if (reinterpret_cast<uintptr_t>(ws) & 7) return fail(-1, "ws must be 8-byte aligned");
    return 0;
}

int forward(const Shape &s, const float *disp, int basis, float *det, bool penalty, double eps, void *ws,
            double *out, long *folded, float *range, hipStream_t stream) {
    const dim3 grid((unsigned)chunks_of(s), (s.D[1] + kRows - 1) / kRows, s.D[0]);
    const int vec = det && (s.D[2] % 4 == 0) && (reinterpret_cast<uintptr_t>(det) & 15) == 0;
    Partial *partials = reinterpret_cast<Partial *>(ws);
    const int stride = basis == BSPLINE ? line_stride<BSPLINE>(s) : line_stride<LINEAR>(s);
    const size_t lds = (size_t)kRows * kLines * stride * sizeof(float);
    if (basis == BSPLINE)
        hipLaunchKernelGGL(jacobian_forward_kernel<BSPLINE>, grid, dim3(kBlock), lds, stream, disp, s, det, vec,
                           penalty ? 1 : 0, eps, stride, partials);
    else
        hipLaunchKernelGGL(jacobian_forward_kernel<LINEAR>, grid, dim3(kBlock), lds, stream, disp, s, det, vec,
                           penalty ? 1 : 0, eps, stride, partials);
    const double inv_n = 1.0 / ((double)s.D[0] * s.D[1] * s.D[2]);
    hipLaunchKernelGGL(jacobian_fold_kernel, dim3(1), dim3(kBlock), 0, stream, partials, groups_of(s), inv_n, out,
                       folded, range);
    return 0;
}

}  // namespace

extern "C" {

int ddrr_jacobian_abi_version(void) { return DDRR_JACOBIAN_ABI_VERSION; }
const char *ddrr_jacobian_last_error(void) { return g_err; }

long ddrr_jacobian_workspace_bytes(int Dx, int Dy, int Dz, int Gx, int Gy, int Gz, int basis) {
    const Shape s = {{Dx, Dy, Dz}, {Gx, Gy, Gz}};
    const char *what = argument_error(s, basis);
    if (what) return fail(-1, what);
    const long need = workspace_bytes(s, basis);
    if (need < 0) return fail(-1, "more than 2^31 - 1 (cell, piece) workgroups: the lattice is too fine");
    return need;
}

int ddrr_jacobian_determinant(const float *displacement, int Gx, int Gy, int Gz, int Dx, int Dy, int Dz, int basis,
                              float *det, void *ws, long ws_bytes, long *folded, float *range, void *stream) {
    if (!displacement || !det || !ws || !folded || !range) return fail(-1, "null pointer");
    const Shape s = {{Dx, Dy, Dz}, {Gx, Gy, Gz}};
    if (check(s, basis, ws, ws_bytes)) return -1;
    forward(s, displacement, basis, det, false, 1.0, ws, nullptr, folded, range, (hipStream_t)stream);
    return finish("ddrr_jacobian_determinant");
}

int ddrr_jacobian_penalty(const float *displacement, int Gx, int Gy, int Gz, int Dx, int Dy, int Dz, int basis,
                          double eps, void *ws, long ws_bytes, double *penalty, long *folded, float *range,
                          void *stream) {
    if (!displacement || !ws || !penalty || !folded || !range) return fail(-1, "null pointer");
    const Shape s = {{Dx, Dy, Dz}, {Gx, Gy, Gz}};
    if (check(s, basis, ws, ws_bytes)) return -1;
    if (eps_error(eps)) return fail(-1, eps_error(eps));
    forward(s, displacement, basis, nullptr, true, eps, ws, penalty, folded, range, (hipStream_t)stream);
    return finish("ddrr_jacobian_penalty");
}

int ddrr_jacobian_backward(const float *displacement, int Gx, int Gy, int Gz, int Dx, int Dy, int Dz, int basis,
                           const float *gD, double eps, void *ws, long ws_bytes, float *gU, void *stream) {
    if (!displacement || !ws || !gU) return fail(-1, "null pointer");
    const Shape s = {{Dx, Dy, Dz}, {Gx, Gy, Gz}};
    if (check(s, basis, ws, ws_bytes)) return -1;
    if (eps_error(eps)) return fail(-1, eps_error(eps));
    const float inv_n = (float)(1.0 / ((double)Dx * Dy * Dz)), feps = (float)eps;
    const hipStream_t q = (hipStream_t)stream;
    if (basis == BSPLINE) {
        const long p1 = plane1_floats(s), p2 = plane2_floats(s), n3 = 3L * Gx * Gy * Gz;
        float *r1 = reinterpret_cast<float *>(ws), *r2 = r1 + 3 * p1;
        const int stride = line_stride<BSPLINE>(s);
        hipLaunchKernelGGL(jacobian_rows_kernel, dim3((Dy + kGradRows - 1) / kGradRows, Dx), dim3(kGradBlock),
                           (size_t)kGradRows * kLines * stride * sizeof(float), q, displacement, s, gD, feps, inv_n,
                           stride, r1);
        // over y: r2[k, (a, x), m, n] from r1[., (a, x), y, n]; over x: gU[a, l, (m, n)] from r2[., a, x, (m, n)]
        const dim3 g2((unsigned)((p2 + kBlock - 1) / kBlock)), g3((unsigned)((n3 + kBlock - 1) / kBlock));
        hipLaunchKernelGGL(jacobian_gather_kernel, g2, dim3(kBlock), 0, q, (const float *)nullptr, r1, Dy, Gy, (long)Gz,
                           p2, r2);
        hipLaunchKernelGGL(jacobian_gather_kernel, g2, dim3(kBlock), 0, q, r1 + p1, r1 + 2 * p1, Dy, Gy, (long)Gz, p2,
                           r2 + p2);
        hipLaunchKernelGGL(jacobian_gather_kernel, g3, dim3(kBlock), 0, q, r2, r2 + p2, Dx, Gx, (long)Gy * Gz, n3, gU);
    } else {
        const long pieces = pieces_per_cell(s), groups = cells_of(s) * pieces, values = 3L * Gx * Gy * Gz;
        hipLaunchKernelGGL(jacobian_pieces_kernel, dim3((unsigned)groups), dim3(kBlock), 0, q, displacement, s, gD,
                           feps, inv_n, (unsigned)pieces, reinterpret_cast<float *>(ws));
        hipLaunchKernelGGL(jacobian_nodes_kernel, dim3((unsigned)((values + kBlock - 1) / kBlock)), dim3(kBlock), 0, q,
                           reinterpret_cast<const float *>(ws), s, pieces, gU);
    }
    return finish("ddrr_jacobian_backward");
}

}  // extern "C"
