// Host build of csrc/jacobian_core.h behind the C ABI of include/diffdrr_jacobian_hip.h: the loops of the gfx950
// kernels (csrc/jacobian.hip) over workgroups, rows, chunks, lanes and node tasks, one element at a time, the
// sums in the kernels' order.  Compiled by tests/jacobian_cases.py with g++; no HIP, no GPU.  Pointers are host
// pointers; `stream` is ignored.  With -DJACOBIAN_EMU_MAIN it is a program of its own that runs the entries on
// exactly-sized heap buffers (built with -fsanitize=address,undefined: the memory check of the index arithmetic).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../diffdrr_amd/csrc/jacobian_core.h"

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

int check(const Shape &s, int basis, const void *ws, long ws_bytes) {
    const char *what = argument_error(s, basis);
    if (what) return fail(-1, what);
    const long need = workspace_bytes(s, basis);
    if (need < 0) return fail(-1, "more than 2^31 - 1 (cell, piece) workgroups: the lattice is too fine");
    if (ws_bytes < need) return fail(-1, "ws_bytes is smaller than ddrr_jacobian_workspace_bytes");
    if (reinterpret_cast<uintptr_t>(ws) & 7) return fail(-1, "ws must be 8-byte aligned");
    return 0;
}

// a wave's fill_lines: exactly kLines * stride floats on the heap, so that a sanitizer sees an index past the
// wave's part of the LDS array
template <int BASIS>
void fill_lines(const float *disp, const Shape &s, int x, int y, Span span, int stride, std::vector<float> &L) {
    std::vector<float>((size_t)kLines * stride, 0.f).swap(L);
    const Taps tx = taps_of<BASIS>(x, s.D[0], s.G[0]), ty = taps_of<BASIS>(y, s.D[1], s.G[1]);
    for (int v = 0; v < 3 * (span.hi - span.lo + 1); ++v) fill_task<BASIS>(disp, s, tx, ty, span, v, stride, L.data());
}

// reduce_workgroup: the tree over each wave's lanes, then the waves in order
Partial reduce_workgroup(std::vector<Partial> &red) {
    for (int w = 0; w < kRows; ++w)
        for (int half = kLanes / 2; half > 0; half >>= 1)
            for (int i = 0; i < half; ++i) tree_level(red.data() + w * kLanes, half, i);
    Partial r = red[0];
    for (int w = 1; w < kRows; ++w) merge(r, red[(size_t)w * kLanes]);
    return r;
}

template <int BASIS>
void forward_groups(const Shape &s, const float *disp, float *det, bool penalty, double eps, Partial *partials) {
    const int chunks = (int)chunks_of(s), ygroups = (s.D[1] + kRows - 1) / kRows, stride = line_stride<BASIS>(s);
    std::vector<float> L;
    std::vector<Partial> red((size_t)kBlock);
    float sc[3];
    scales_of(s, sc);
    for (int x = 0; x < s.D[0]; ++x)
        for (int gy = 0; gy < ygroups; ++gy)
            for (int gz = 0; gz < chunks; ++gz) {  // one workgroup of the forward kernel
                const int zlo = gz * kChunk, zend = zlo + kChunk < s.D[2] ? zlo + kChunk : s.D[2];
                const Span span = chunk_span<BASIS>(zlo, zend, s.D[2], s.G[2]);
                for (int wave = 0; wave < kRows; ++wave) {
                    const int y = gy * kRows + wave;
                    if (y < s.D[1]) fill_lines<BASIS>(disp, s, x, y, span, stride, L);
                    for (int lane = 0; lane < kLanes; ++lane) {
                        Partial mine = no_voxels();
                        const int z0 = zlo + 4 * lane;
                        if (y < s.D[1] && z0 < zend) {
                            float out[4];
                            forward_run<BASIS>(s, L.data(), stride, span.lo, z0, sc, penalty, eps, out, mine);
                            for (int k = 0; det && k < 4 && z0 + k < s.D[2]; ++k)
                                det[((long)x * s.D[1] + y) * s.D[2] + z0 + k] = out[k];
                        }
                        red[(size_t)wave * kLanes + lane] = mine;
                    }
                }
                partials[((long)x * ygroups + gy) * chunks + gz] = reduce_workgroup(red);
            }
}

// jacobian_fold_kernel
void fold_partials(const Shape &s, const Partial *partials, double *penalty, long *folded, float *range) {
    const long groups = groups_of(s);
    std::vector<Partial> red((size_t)kBlock);
    for (int t = 0; t < kBlock; ++t) {
        Partial mine = no_voxels();
        for (long i = t; i < groups; i += kBlock) merge(mine, partials[i]);
        red[t] = mine;
    }
    const Partial all = reduce_workgroup(red);
    if (penalty) *penalty = all.sum * (1.0 / ((double)s.D[0] * s.D[1] * s.D[2]));
    *folded = all.count;
    range[0] = all.lo;
    range[1] = all.hi;
}

void forward(const Shape &s, const float *disp, int basis, float *det, bool penalty, double eps, void *ws,
             double *out, long *folded, float *range) {
    Partial *partials = reinterpret_cast<Partial *>(ws);
    if (basis == BSPLINE)
        forward_groups<BSPLINE>(s, disp, det, penalty, eps, partials);
    else
        forward_groups<LINEAR>(s, disp, det, penalty, eps, partials);
    fold_partials(s, partials, out, folded, range);
}

// out[o, m, i]: jacobian_gather_kernel
void gather(const float *srcD, const float *srcW, int D, int G, long inner, long count, float *out) {
    for (long e = 0; e < count; ++e) {
        const long om = e / inner, i = e - om * inner, o = om / G, base = o * D * inner + i;
        out[e] = gather_pair(srcD ? srcD + base : nullptr, srcW + base, inner, D, G, (int)(om - o * G));
    }
}

void backward_bspline(const Shape &s, const float *disp, const float *gD, float eps, float inv_n, float *r1,
                      float *gU) {
    const long p1 = plane1_floats(s), p2 = plane2_floats(s);
    float *r2 = r1 + 3 * p1;
    const int stride = line_stride<BSPLINE>(s);
    std::vector<float> L, cab((size_t)kRowFloats), wz((size_t)4 * kPadded), dz((size_t)4 * kPadded);
    float sc[3];
    scales_of(s, sc);
    for (int x = 0; x < s.D[0]; ++x)
        for (int y = 0; y < s.D[1]; ++y) {  // one wave of the rows kernel
            int done = -1;
            for (int zlo = 0; zlo < s.D[2]; zlo += kChunk) {
                const int zend = zlo + kChunk < s.D[2] ? zlo + kChunk : s.D[2];
                const Span span = chunk_span<BSPLINE>(zlo, zend, s.D[2], s.G[2]);
                fill_lines<BSPLINE>(disp, s, x, y, span, stride, L);
                for (int z = zlo; z < zend; ++z) {
                    float w[4], d[4], c[9];
                    node_weights(z, s.D[2], s.G[2], w, d);
                    for (int k = 0; k < 4; ++k) {
                        wz.at((size_t)k * kPadded + padded(z - zlo)) = w[k];
                        dz.at((size_t)k * kPadded + padded(z - zlo)) = d[k];
                    }
                    voxel_c<BSPLINE>(s, L.data(), stride, span.lo, z, ((long)x * s.D[1] + y) * s.D[2] + z, sc, gD, eps,
                                     inv_n, c);
                    for (int e = 0; e < 9; ++e) cab.at((size_t)e * kPadded + padded(z - zlo)) = c[e];
                }
                const int nlo = span.lo < 0 ? 0 : span.lo, nhi = span.hi > s.G[2] - 1 ? s.G[2] - 1 : span.hi;
                for (int a = 0; a < 3; ++a)
                    for (int n = nlo; n <= nhi; ++n)
                        for (int b = 0; b < 3; ++b) {
                            float *dst = r1 + b * p1 + (((long)a * s.D[0] + x) * s.D[1] + y) * s.G[2] + n;
                            *dst = node_chain(cab.data() + (size_t)(3 * a + b) * kPadded, b < 2 ? wz.data() : dz.data(),
                                              s.D[2], s.G[2], n, zlo, zend, n > done ? 0.f : *dst);
                        }
                done = nhi;
            }
        }
    gather(nullptr, r1, s.D[1], s.G[1], s.G[2], p2, r2);
    gather(r1 + p1, r1 + 2 * p1, s.D[1], s.G[1], s.G[2], p2, r2 + p2);
    gather(r2, r2 + p2, s.D[0], s.G[0], (long)s.G[1] * s.G[2], 3L * s.G[0] * s.G[1] * s.G[2], gU);
}

void backward_linear(const Shape &s, const float *disp, const float *gD, float eps, float inv_n, float *ws,
                     float *gU) {
    const long pieces = pieces_per_cell(s);
    std::vector<float> red((size_t)kPieceFloats * kRedStride), part((size_t)kSlices * kPieceFloats);
    for (int cx = 0; cx < s.G[0] - 1; ++cx)
        for (int cy = 0; cy < s.G[1] - 1; ++cy)
            for (int cz = 0; cz < s.G[2] - 1; ++cz)
                for (long piece = 0; piece < pieces; ++piece) {  // one workgroup of the pieces kernel
                    for (int tid = 0; tid < kBlock; ++tid) {
                        float acc[kPieceFloats];
                        piece_thread(s, disp, gD, eps, inv_n, cx, cy, cz, (unsigned)piece, tid, acc);
                        for (int e = 0; e < kPieceFloats; ++e) red.at((size_t)e * kRedStride + tid) = acc[e];
                    }
                    for (int sl = 0; sl < kSlices; ++sl)
                        for (int e = 0; e < kPieceFloats; ++e)
                            part[(size_t)sl * kPieceFloats + e] = slice_sum(red.data() + (size_t)e * kRedStride, sl);
                    const long cell = ((long)cx * (s.G[1] - 1) + cy) * (s.G[2] - 1) + cz;
                    for (int e = 0; e < kPieceFloats; ++e) {
                        float v = part[e];
                        for (int sl = 1; sl < kSlices; ++sl) v += part[(size_t)sl * kPieceFloats + e];
                        ws[(cell * pieces + piece) * kPieceFloats + e] = v;
                    }
                }
    for (int a = 0; a < 3; ++a)
        for (int i = 0; i < s.G[0]; ++i)
            for (int j = 0; j < s.G[1]; ++j)
                for (int k = 0; k < s.G[2]; ++k)
                    gU[(((long)a * s.G[0] + i) * s.G[1] + j) * s.G[2] + k] = node_sum(ws, s, pieces, a, i, j, k);
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
                              float *det, void *ws, long ws_bytes, long *folded, float *range, void *) {
    if (!displacement || !det || !ws || !folded || !range) return fail(-1, "null pointer");
    const Shape s = {{Dx, Dy, Dz}, {Gx, Gy, Gz}};
    if (check(s, basis, ws, ws_bytes)) return -1;
    forward(s, displacement, basis, det, false, 1.0, ws, nullptr, folded, range);
    return 0;
}

int ddrr_jacobian_penalty(const float *displacement, int Gx, int Gy, int Gz, int Dx, int Dy, int Dz, int basis,
                          double eps, void *ws, long ws_bytes, double *penalty, long *folded, float *range, void *) {
    if (!displacement || !ws || !penalty || !folded || !range) return fail(-1, "null pointer");
    const Shape s = {{Dx, Dy, Dz}, {Gx, Gy, Gz}};
    if (check(s, basis, ws, ws_bytes)) return -1;
    if (eps_error(eps)) return fail(-1, eps_error(eps));
    forward(s, displacement, basis, nullptr, true, eps, ws, penalty, folded, range);
    return 0;
}

int ddrr_jacobian_backward(const float *displacement, int Gx, int Gy, int Gz, int Dx, int Dy, int Dz, int basis,
                           const float *gD, double eps, void *ws, long ws_bytes, float *gU, void *) {
    if (!displacement || !ws || !gU) return fail(-1, "null pointer");
    const Shape s = {{Dx, Dy, Dz}, {Gx, Gy, Gz}};
    if (check(s, basis, ws, ws_bytes)) return -1;
    if (eps_error(eps)) return fail(-1, eps_error(eps));
    const float inv_n = (float)(1.0 / ((double)Dx * Dy * Dz)), feps = (float)eps;
    if (basis == BSPLINE)
        backward_bspline(s, displacement, gD, feps, inv_n, reinterpret_cast<float *>(ws), gU);
    else
        backward_linear(s, displacement, gD, feps, inv_n, reinterpret_cast<float *>(ws), gU);
    return 0;
}

}  // extern "C"

#ifdef JACOBIAN_EMU_MAIN
// The memory check: every entry on exactly-sized heap buffers, both bases, with gD and without; a sanitizer build
// reports any access outside them.
namespace {

unsigned g_seed = 12345u;

float uniform() {  // in [0, 1)
    g_seed = g_seed * 1664525u + 1013904223u;
    return (float)(g_seed >> 8) / 16777216.f;
}

int run(int Dx, int Dy, int Dz, int Gx, int Gy, int Gz, float amplitude, int basis) {
    const size_t n = (size_t)Dx * Dy * Dz, m = (size_t)3 * Gx * Gy * Gz;
    std::vector<float> det(n), gD(n), U(m), gU(m), gP(m), range(2), range2(2);
    std::vector<long> folded(1), folded2(1);
    std::vector<double> penalty(1);
    for (float &v : gD) v = uniform();
    for (float &v : U) v = (2.f * uniform() - 1.f) * amplitude;
    const long bytes = ddrr_jacobian_workspace_bytes(Dx, Dy, Dz, Gx, Gy, Gz, basis);
    if (bytes < 0) return 1;
    std::vector<double> ws(((size_t)bytes + 7) / 8);
    int rc = ddrr_jacobian_determinant(U.data(), Gx, Gy, Gz, Dx, Dy, Dz, basis, det.data(), ws.data(), bytes,
                                       folded.data(), range.data(), nullptr);
    rc |= ddrr_jacobian_penalty(U.data(), Gx, Gy, Gz, Dx, Dy, Dz, basis, 0.1, ws.data(), bytes, penalty.data(),
                                folded2.data(), range2.data(), nullptr);
    rc |= ddrr_jacobian_backward(U.data(), Gx, Gy, Gz, Dx, Dy, Dz, basis, gD.data(), 0.1, ws.data(), bytes, gU.data(),
                                 nullptr);
    rc |= ddrr_jacobian_backward(U.data(), Gx, Gy, Gz, Dx, Dy, Dz, basis, nullptr, 0.1, ws.data(), bytes, gP.data(),
                                 nullptr);
    rc |= folded[0] != folded2[0] || range[0] != range2[0] || range[1] != range2[1];
    double sd = 0, su = 0, sp = 0;
    for (float v : det) sd += v;
    for (float v : gU) su += v;
    for (float v : gP) sp += v;
    printf("%dx%dx%d lattice (%d, %d, %d) +-%g basis %d: rc %d, folded %ld of %zu, d in [%g, %g], penalty %.6g, "
           "sums %.6g %.6g %.6g\n", Dx, Dy, Dz, Gx, Gy, Gz, amplitude, basis, rc, folded[0], n, range[0], range[1],
           penalty[0], sd, su, sp);
    return rc;
}

}  // namespace

int main() {
    int rc = 0;
    for (int basis = 0; basis < 2; ++basis) {
        rc |= run(2, 2, 2, 2, 2, 2, 2.5f, basis);
        rc |= run(2, 2, 2, 2, 2, 2, 12.f, basis);
        rc |= run(37, 41, 45, 7, 6, 8, 12.f, basis);
        rc |= run(23, 30, 37, 4, 5, 3, 12.f, basis);
        rc |= run(5, 6, 700, 2, 3, 700, 12.f, basis);  // one node per z voxel: the widest lines a chunk can need
        rc |= run(5, 6, 600, 3, 4, 7, 12.f, basis);    // rows of several chunks: chains that continue
        rc |= run(6, 5, 515, 2, 5, 515, 12.f, basis);
        rc |= run(3, 4, 1024, 3, 2, 33, 12.f, basis);
        rc |= run(2, 3, 65535, 2, 3, 700, 12.f, basis);
        rc |= run(65535, 2, 3, 9, 2, 2, 12.f, basis);
    }
    return rc;
}
#endif
