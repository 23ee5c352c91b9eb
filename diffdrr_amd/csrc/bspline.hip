// bspline.hip -- the kernels of the cubic B-spline free-form deformation of the volume: the C ABI of
// include/diffdrr_bspline_hip.h (libdiffdrr_bspline_hip.so).  The arithmetic is bspline_core.h's; what is here
// is who computes what.  No kernel forms the 64-tap sum per voxel and none writes a dense field.
//
// A workgroup of 256 threads owns four volume rows (x, y .. y + 3), one wave each, and of each row a chunk of
// 256 z voxels.  A wave first collapses x and y for its row: the row's line, one value per (component, z node
// the chunk reaches), each the 16-term sum of lattice values (L2-resident, 16 reads per value, amortised over
// the chunk), into LDS as [component][node], in double (bspline_core.h says why).  A voxel's field is then
// 4 taps x 3 components of that line.
// Lanes of a wave read one tap of neighbouring voxels: the same word (broadcast) or consecutive words, which
// is conflict-free while a 32-lane group spans fewer than 32 nodes -- a node spacing of 4 voxels or more in
// the forward kernel, any spacing in the others.
//
//   bspline_forward_kernel  lane l takes the run of four z voxels from 4 l of the chunk (eight gathers and
//       one interpolation each) and stores 16 bytes where Dz is a multiple of 4.
//   bspline_rows_kernel     first gather of the lattice gradient.  The workgroup walks its rows chunk by
//       chunk: lane l takes voxels l, l + 64, l + 128, l + 192 of the chunk (gW and the gathers coalesce),
//       writes q = gW dV(p) to LDS next to the chunk's folded z weights; then lane 4 s + a carries the chains
//       of component a of the nodes n = s mod 16 -- always the same lane for a node, so a chain that continues
//       in the next chunk is that lane's own store and load of r1.
//   bspline_gather_kernel   second and third gather: one thread per output value, lanes along z nodes.
//   bspline_volume_kernel   the rows kernel's voxel mapping; each of the 8 corners is one
//       global_atomic_add_f32 per wave.  Not bitwise reproducible.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include "bspline_core.h"

namespace {

using namespace ddrr_bspline;

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

// the wave's row line for the chunk's span into L; every lane of the wave calls it
__device__ __forceinline__ void fill_line(const float *__restrict__ disp, const Shape &s, const Taps &tx,
                                          const Taps &ty, Span span, int lane, double *L) {
    const int count = span.hi - span.lo + 1;
    for (int v = lane; v < 3 * count; v += kLanes) {
        const int a = v / count, j = v - a * count;
        L[a * kLineNodes + j] = line_value(disp, s.G, tx, ty, a, clamp_node(span.lo + j, s.G[2]));
    }
}

__global__ __launch_bounds__(kBlock) void bspline_forward_kernel(const float *__restrict__ V, Shape s,
                                                                 const float *__restrict__ disp, int padding,
                                                                 float *__restrict__ W, int vec) {
    __shared__ double lines[kRows][kLineValues];
    const int wave = threadIdx.x / kLanes, lane = threadIdx.x % kLanes;
    const int x = blockIdx.z, y = blockIdx.y * kRows + wave, zlo = blockIdx.x * kChunk;
    const int zend = zlo + kChunk < s.D[2] ? zlo + kChunk : s.D[2];
    const bool row = y < s.D[1];
    const Span span = chunk_span(zlo, zend, s.D[2], s.G[2]);
    if (row) fill_line(disp, s, taps_of(x, s.D[0], s.G[0]), taps_of(y, s.D[1], s.G[1]), span, lane, lines[wave]);
    __syncthreads();
    const int z0 = zlo + 4 * lane;
    if (!row || z0 >= zend) return;
    float out[4];
    forward_run(V, s, padding, lines[wave], span.lo, x, y, z0, out);
    float *dst = W + ((long)x * s.D[1] + y) * s.D[2] + z0;
    if (vec) {
        *reinterpret_cast<float4 *>(dst) = make_float4(out[0], out[1], out[2], out[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (z0 + k < s.D[2]) dst[k] = out[k];
    }
}

__global__ __launch_bounds__(kBlock) void bspline_rows_kernel(const float *__restrict__ V, Shape s,
                                                              const float *__restrict__ disp, int padding,
                                                              const float *__restrict__ gW, float *r1) {
    __shared__ double lines[kRows][kLineValues];
    __shared__ float q[kRows][3][kPadded];
    __shared__ float wz[4][kPadded];
    const int wave = threadIdx.x / kLanes, lane = threadIdx.x % kLanes;
    const int x = blockIdx.y, y = blockIdx.x * kRows + wave;
    const bool row = y < s.D[1];
    const Taps tx = taps_of(x, s.D[0], s.G[0]), ty = taps_of(row ? y : 0, s.D[1], s.G[1]);
    const long at = ((long)x * s.D[1] + y) * s.D[2];
    const int a = lane & 3, slot = lane >> 2;
    float *mine = r1 + (((long)(a < 3 ? a : 0) * s.D[0] + x) * s.D[1] + y) * s.G[2];  // r1[a, x, y, .]
    int done = -1;  // the last node an earlier chunk reached
    for (int zlo = 0; zlo < s.D[2]; zlo += kChunk) {
        const int zend = zlo + kChunk < s.D[2] ? zlo + kChunk : s.D[2];
        const Span span = chunk_span(zlo, zend, s.D[2], s.G[2]);
        if (row) fill_line(disp, s, tx, ty, span, lane, lines[wave]);
        if (zlo + (int)threadIdx.x < zend) {
            float w[4];
            node_weights(zlo + threadIdx.x, s.D[2], s.G[2], w);
#pragma unroll
            for (int k = 0; k < 4; ++k) wz[k][padded(threadIdx.x)] = w[k];
        }
        __syncthreads();
        if (row) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int zi = lane + kLanes * i, z = zlo + zi;
                if (z < zend) {
                    float qv[3];
                    voxel_q(V, s, padding, lines[wave], span.lo, x, y, z, gW[at + z], qv);
#pragma unroll
                    for (int c = 0; c < 3; ++c) q[wave][c][padded(zi)] = qv[c];
                }
            }
        }
        __syncthreads();
        const int nlo = span.lo < 0 ? 0 : span.lo, nhi = span.hi > s.G[2] - 1 ? s.G[2] - 1 : span.hi;
        if (row && a < 3) {
            for (int n = nlo + ((slot - nlo) & (kSlots - 1)); n <= nhi; n += kSlots) {
                float *dst = mine + n;
                *dst = node_chain(q[wave][a], wz[0], s.D[2], s.G[2], n, zlo, zend, n > done ? 0.f : *dst);
            }
        }
        done = nhi;
        __syncthreads();
    }
}

// out[o, m, i] = the chain of node m of an axis of D voxels over src[o, ., i]; `count` values, `inner` per node
__global__ __launch_bounds__(kBlock) void bspline_gather_kernel(const float *__restrict__ src, int D, int G, long inner,
                                                                long count, float *__restrict__ out) {
    const long e = (long)blockIdx.x * kBlock + threadIdx.x;
    if (e >= count) return;
    const long om = e / inner, i = e - om * inner, o = om / G;
    out[e] = gather_axis(src + o * D * inner + i, inner, D, G, (int)(om - o * G));
}

__global__ __launch_bounds__(kBlock) void bspline_volume_kernel(const float *__restrict__ disp, Shape s, int padding,
                                                                const float *__restrict__ gW, float *__restrict__ gV) {
    __shared__ double lines[kRows][kLineValues];
    const int wave = threadIdx.x / kLanes, lane = threadIdx.x % kLanes;
    const int x = blockIdx.z, y = blockIdx.y * kRows + wave, zlo = blockIdx.x * kChunk;
    const int zend = zlo + kChunk < s.D[2] ? zlo + kChunk : s.D[2];
    const bool row = y < s.D[1];
    const Span span = chunk_span(zlo, zend, s.D[2], s.G[2]);
    if (row) fill_line(disp, s, taps_of(x, s.D[0], s.G[0]), taps_of(y, s.D[1], s.G[1]), span, lane, lines[wave]);
    __syncthreads();
    if (!row) return;
    const long at = ((long)x * s.D[1] + y) * s.D[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int z = zlo + lane + kLanes * i;
        if (z >= zend) break;
        long o[8];
        float w[8];
        scatter_terms(s, padding, lines[wave], span.lo, x, y, z, gW[at + z], o, w);
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if (w[c] != 0.f) unsafeAtomicAdd(gV + o[c], w[c]);
    }
}

int check(const Shape &s, int padding) {
    const char *what = domain_error(s, padding);
    return what ? fail(-1, what) : 0;
}

dim3 chunk_grid(const Shape &s) {
    return dim3((s.D[2] + kChunk - 1) / kChunk, (s.D[1] + kRows - 1) / kRows, s.D[0]);
}

}  // namespace

extern "C" {

int ddrr_bspline_abi_version(void) { return DDRR_BSPLINE_ABI_VERSION; }
const char *ddrr_bspline_last_error(void) { return g_err; }

long ddrr_bspline_workspace_bytes(int Dx, int Dy, int Dz, int Gx, int Gy, int Gz) {
    const Shape s = {{Dx, Dy, Dz}, {Gx, Gy, Gz}};
    if (check(s, DDRR_BSPLINE_PADDING_ZEROS)) return -1;
    return (r1_floats(s) + r2_floats(s)) * (long)sizeof(float);
}

int ddrr_bspline_forward(const float *V, int Dx, int Dy, int Dz, const float *displacement, int Gx, int Gy,
                         int Gz, int padding, float *W, void *stream) {
    if (!V || !displacement || !W) return fail(-1, "null pointer");
    const Shape s = {{Dx, Dy, Dz}, {Gx, Gy, Gz}};
    if (check(s, padding)) return -1;
    const int vec = (Dz % 4 == 0) && (reinterpret_cast<uintptr_t>(W) & 15) == 0;
    hipLaunchKernelGGL(bspline_forward_kernel, chunk_grid(s), dim3(kBlock), 0, (hipStream_t)stream, V, s, displacement,
                       padding, W, vec);
    return finish("ddrr_bspline_forward");
}

int ddrr_bspline_backward_displacement(const float *V, int Dx, int Dy, int Dz, const float *displacement,
                                       int Gx, int Gy, int Gz, int padding, const float *gW, void *ws,
                                       long ws_bytes, float *gU, void *stream) {
    if (!V || !displacement || !gW || !ws || !gU) return fail(-1, "null pointer");
    const Shape s = {{Dx, Dy, Dz}, {Gx, Gy, Gz}};
    if (check(s, padding)) return -1;
    if (ws_bytes < ddrr_bspline_workspace_bytes(Dx, Dy, Dz, Gx, Gy, Gz))
        return fail(-1, "ws_bytes is smaller than ddrr_bspline_workspace_bytes");
    if (reinterpret_cast<uintptr_t>(ws) & 3) return fail(-1, "ws must be 4-byte aligned");
    float *r1 = reinterpret_cast<float *>(ws), *r2 = r1 + r1_floats(s);
    hipLaunchKernelGGL(bspline_rows_kernel, dim3((Dy + kRows - 1) / kRows, Dx), dim3(kBlock), 0, (hipStream_t)stream, V,
                       s, displacement, padding, gW, r1);
    // over y: r2[(a, x), m, n] from r1[(a, x), y, n]; over x: gU[a, l, (m, n)] from r2[a, x, (m, n)]
    const long n2 = r2_floats(s), n3 = 3L * Gx * Gy * Gz;
    hipLaunchKernelGGL(bspline_gather_kernel, dim3((unsigned)((n2 + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       (hipStream_t)stream, r1, Dy, Gy, (long)Gz, n2, r2);
    hipLaunchKernelGGL(bspline_gather_kernel, dim3((unsigned)((n3 + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       (hipStream_t)stream, r2, Dx, Gx, (long)Gy * Gz, n3, gU);
    return finish("ddrr_bspline_backward_displacement");
}

int ddrr_bspline_backward_volume(const float *displacement, int Gx, int Gy, int Gz, int Dx, int Dy, int Dz,
                                 int padding, const float *gW, float *gV, void *stream) {
    if (!displacement || !gW || !gV) return fail(-1, "null pointer");
    const Shape s = {{Dx, Dy, Dz}, {Gx, Gy, Gz}};
    if (check(s, padding)) return -1;
    const hipError_t e = hipMemsetAsync(gV, 0, (size_t)Dx * Dy * Dz * sizeof(float), (hipStream_t)stream);
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "ddrr_bspline_backward_volume: %s", hipGetErrorString(e));
        return (int)e;
    }
    hipLaunchKernelGGL(bspline_volume_kernel, chunk_grid(s), dim3(kBlock), 0, (hipStream_t)stream, displacement, s,
                       padding, gW, gV);
    return finish("ddrr_bspline_backward_volume");
}

}  // extern "C"
