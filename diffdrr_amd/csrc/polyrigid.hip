// polyrigid.hip -- the kernels of a polyrigid deformation of the volume in front of the renderers: the C ABI of
// include/diffdrr_polyrigid_hip.h (libdiffdrr_polyrigid_hip.so).  The arithmetic is polyrigid_core.h's; what is
// here is who computes what.
//
//   forward_kernel       one thread per run of four z voxels of a volume row (x = blockIdx.y).  The twist comes
//       from registers: the thread interpolates its cell's four lattice columns along x and y at the two z nodes
//       of its cell (2 x 24 lattice reads), steps the z cell with the integer remainder (no division per voxel)
//       and re-reads one line when a run crosses a node.  Per output: six interpolations, three 8-term series,
//       three cross products, eight gathered voxels; W leaves as one 16-byte store per thread where Dz is a
//       multiple of 4.  No dense twist or displacement field exists in memory.
//   twist_pieces_kernel  one workgroup per (lattice cell, piece of 1024 of its voxels): thread t takes the
//       voxels t, t + 256, ... of the piece and keeps the cell's 8 nodes x 6 components as 48 sums in registers,
//       then a fixed-order LDS reduction in two passes of 24 values (the warp library's buffer): 192 threads add
//       one (value, slice of 32 threads) each, 24 threads add the 8 slices.
//   twist_nodes_kernel   one thread per (component, node): adds the pieces of the node's up to 8 cells in
//       index order.  No atomics in either: bitwise reproducible.
//   volume_kernel        one thread per voxel, lanes along z: each of the 8 corners is one
//       global_atomic_add_f32 per wave whose addresses follow the lanes' z (contiguous runs wherever the
//       motion is smooth).  Not bitwise reproducible.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include "polyrigid_core.h"

namespace {

using namespace ddrr_polyrigid;

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

// (4 waves per SIMD: the sample position in double fits 128 VGPRs without scratch)
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4, 4))) void forward_kernel(const float *__restrict__ V, Geometry g,
                                                         const float *__restrict__ Xi, int padding,
                                                         float *__restrict__ W, int nq, int vec) {
    const unsigned t = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    if (t >= (unsigned)g.s.D[1] * (unsigned)nq) return;
    const int x = blockIdx.y, y = (int)(t / (unsigned)nq), z0 = 4 * (int)(t - (unsigned)y * (unsigned)nq);
    float out[4];
    forward_run(V, g, Xi, padding, x, y, z0, out);
    float *dst = W + ((long)x * g.s.D[1] + y) * g.s.D[2] + z0;
    if (vec) {
        *reinterpret_cast<float4 *>(dst) = make_float4(out[0], out[1], out[2], out[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (z0 + k < g.s.D[2]) dst[k] = out[k];
    }
}

__global__ __launch_bounds__(kBlock) void twist_pieces_kernel(const float *__restrict__ V, Geometry g,
                                                              const float *__restrict__ Xi, int padding,
                                                              const float *__restrict__ gW, unsigned pieces,
                                                              float *__restrict__ ws) {
    __shared__ float red[kHalfFloats * kRedStride];
    __shared__ float part[kSlices][kHalfFloats];
    const unsigned cell = blockIdx.x / pieces, piece = blockIdx.x - cell * pieces;
    const unsigned gz = (unsigned)(g.s.G[2] - 1), gy = (unsigned)(g.s.G[1] - 1);
    const unsigned cxy = cell / gz;
    const int cz = (int)(cell - cxy * gz), cx = (int)(cxy / gy), cy = (int)(cxy - (unsigned)cx * gy);
    float acc[kPieceFloats];
    piece_thread(V, g, Xi, padding, gW, cx, cy, cz, piece, threadIdx.x, acc);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        // (the second pass may write red at once: the first pass's reads of it ended before its second barrier;
        // its reads of part end before this pass's first barrier)
#pragma unroll
        for (int e = 0; e < kHalfFloats; ++e) red[e * kRedStride + threadIdx.x] = acc[half * kHalfFloats + e];
        __syncthreads();
        if (threadIdx.x < kHalfFloats * kSlices) {
            const int e = threadIdx.x % kHalfFloats, sl = threadIdx.x / kHalfFloats;
            part[sl][e] = slice_sum(red + e * kRedStride, sl);
        }
        __syncthreads();
        if (threadIdx.x < kHalfFloats) {
            float v = part[0][threadIdx.x];
#pragma unroll
            for (int sl = 1; sl < kSlices; ++sl) v += part[sl][threadIdx.x];
            ws[(long)blockIdx.x * kPieceFloats + half * kHalfFloats + threadIdx.x] = v;
        }
    }
}

__global__ __launch_bounds__(kBlock) void twist_nodes_kernel(const float *__restrict__ ws, Shape s, long pieces,
                                                             float *__restrict__ gXi) {
    const long nodes = (long)s.G[0] * s.G[1] * s.G[2];
    const long e = (long)blockIdx.x * kBlock + threadIdx.x;
    if (e >= kTwist * nodes) return;
    const int c = (int)(e / nodes);
    const long n = e - c * nodes;
    const long nxy = n / s.G[2];
    const int k = (int)(n - nxy * s.G[2]), i = (int)(nxy / s.G[1]), j = (int)(nxy - (long)i * s.G[1]);
    gXi[e] = twist_node_sum(ws, s, pieces, c, i, j, k);
}

__global__ __launch_bounds__(kBlock) void volume_kernel(const float *__restrict__ Xi, Geometry g, int padding,
                                                        const float *__restrict__ gW, float *__restrict__ gV) {
    const unsigned t = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    if (t >= (unsigned)g.s.D[1] * (unsigned)g.s.D[2]) return;
    const int x = blockIdx.y, y = (int)(t / (unsigned)g.s.D[2]), z = (int)(t - (unsigned)y * (unsigned)g.s.D[2]);
    const float gw = gW[((long)x * g.s.D[1] + y) * g.s.D[2] + z];
    long o[8];
    float w[8];
    scatter_terms(g, Xi, padding, x, y, z, gw, o, w);
#pragma unroll
    for (int c = 0; c < 8; ++c)
        if (w[c] != 0.f) unsafeAtomicAdd(gV + o[c], w[c]);
}

int check(const Geometry &g, int padding) {
    const char *what = domain_error(g, padding);
    return what ? fail(-1, what) : 0;
}

}  // namespace

extern "C" {

int ddrr_polyrigid_abi_version(void) { return DDRR_POLYRIGID_ABI_VERSION; }
const char *ddrr_polyrigid_last_error(void) { return g_err; }

long ddrr_polyrigid_workspace_bytes(int Dx, int Dy, int Dz, int Gx, int Gy, int Gz) {
    const Geometry g = {{{Dx, Dy, Dz}, {Gx, Gy, Gz}}, {1.f, 1.f, 1.f}};
    if (check(g, DDRR_POLYRIGID_PADDING_ZEROS)) return -1;
    const long groups = cells_of(g.s) * pieces_per_cell(g.s);
    if (groups > 0x7fffffffL) return fail(-1, "more than 2^31 - 1 (cell, piece) workgroups: the lattice is too fine");
    return groups * kPieceFloats * (long)sizeof(float);
}

int ddrr_polyrigid_forward(const float *V, int Dx, int Dy, int Dz, const float *Xi, int Gx, int Gy, int Gz,
                           float hx, float hy, float hz, int padding, float *W, void *stream) {
    if (!V || !Xi || !W) return fail(-1, "null pointer");
    const Geometry g = {{{Dx, Dy, Dz}, {Gx, Gy, Gz}}, {hx, hy, hz}};
    if (check(g, padding)) return -1;
    const int nq = (Dz + 3) / 4;
    const int vec = (Dz % 4 == 0) && (reinterpret_cast<uintptr_t>(W) & 15) == 0;
    const unsigned blocks = ((unsigned)Dy * (unsigned)nq + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(forward_kernel, dim3(blocks, Dx), dim3(kBlock), 0, (hipStream_t)stream, V, g, Xi, padding, W,
                       nq, vec);
    return finish("ddrr_polyrigid_forward");
}

int ddrr_polyrigid_backward_twists(const float *V, int Dx, int Dy, int Dz, const float *Xi, int Gx, int Gy,
                                   int Gz, float hx, float hy, float hz, int padding, const float *gW, void *ws,
                                   long ws_bytes, float *gXi, void *stream) {
    if (!V || !Xi || !gW || !ws || !gXi) return fail(-1, "null pointer");
    const Geometry g = {{{Dx, Dy, Dz}, {Gx, Gy, Gz}}, {hx, hy, hz}};
    if (check(g, padding)) return -1;
    const long need = ddrr_polyrigid_workspace_bytes(Dx, Dy, Dz, Gx, Gy, Gz);
    if (need < 0) return -1;
    if (ws_bytes < need) return fail(-1, "ws_bytes is smaller than ddrr_polyrigid_workspace_bytes");
    if (reinterpret_cast<uintptr_t>(ws) & 3) return fail(-1, "ws must be 4-byte aligned");
    const long pieces = pieces_per_cell(g.s);
    const long groups = cells_of(g.s) * pieces;
    hipLaunchKernelGGL(twist_pieces_kernel, dim3((unsigned)groups), dim3(kBlock), 0, (hipStream_t)stream, V, g, Xi,
                       padding, gW, (unsigned)pieces, reinterpret_cast<float *>(ws));
    const long values = (long)kTwist * Gx * Gy * Gz;
    hipLaunchKernelGGL(twist_nodes_kernel, dim3((unsigned)((values + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       (hipStream_t)stream, reinterpret_cast<const float *>(ws), g.s, pieces, gXi);
    return finish("ddrr_polyrigid_backward_twists");
}

int ddrr_polyrigid_backward_volume(const float *Xi, int Gx, int Gy, int Gz, int Dx, int Dy, int Dz, float hx,
                                   float hy, float hz, int padding, const float *gW, float *gV, void *stream) {
    if (!Xi || !gW || !gV) return fail(-1, "null pointer");
    const Geometry g = {{{Dx, Dy, Dz}, {Gx, Gy, Gz}}, {hx, hy, hz}};
    if (check(g, padding)) return -1;
    const hipError_t e = hipMemsetAsync(gV, 0, (size_t)Dx * Dy * Dz * sizeof(float), (hipStream_t)stream);
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "ddrr_polyrigid_backward_volume: %s", hipGetErrorString(e));
        return (int)e;
    }
    const unsigned blocks = ((unsigned)Dy * (unsigned)Dz + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(volume_kernel, dim3(blocks, Dx), dim3(kBlock), 0, (hipStream_t)stream, Xi, g, padding, gW, gV);
    return finish("ddrr_polyrigid_backward_volume");
}

}  // extern "C"
