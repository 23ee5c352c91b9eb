// Host build of csrc/warp_core.h behind the C ABI of include/diffdrr_warp_hip.h: the loops of the gfx950
// kernels (csrc/warp.hip) over threads, pieces and slices, one element at a time, the sums in the kernels'
// order.  Compiled by tests/warp_cases.py with g++; no HIP, no GPU.  Pointers are host pointers; `stream` is
// ignored.  With -DWARP_EMU_MAIN it is a program of its own that runs the entries on cases whose samples
// leave the volume (built with -fsanitize=address,undefined: the memory check of the index arithmetic).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../diffdrr_amd/csrc/warp_core.h"

namespace {

using namespace ddrr_warp;

thread_local char g_err[512] = "";

int fail(int code, const char *what) {
    snprintf(g_err, sizeof(g_err), "%s", what);
    return code;
}

int check(const Shape &s, int padding) {
    const char *what = domain_error(s, padding);
    return what ? fail(-1, what) : 0;
}

}  // namespace

extern "C" {

int ddrr_warp_abi_version(void) { return DDRR_WARP_ABI_VERSION; }
const char *ddrr_warp_last_error(void) { return g_err; }

long ddrr_warp_workspace_bytes(int Dx, int Dy, int Dz, int Gx, int Gy, int Gz) {
    const Shape s = {{Dx, Dy, Dz}, {Gx, Gy, Gz}};
    if (check(s, DDRR_WARP_PADDING_ZEROS)) return -1;
    const long groups = cells_of(s) * pieces_per_cell(s);
    if (groups > 0x7fffffffL) return fail(-1, "more than 2^31 - 1 (cell, piece) workgroups: the lattice is too fine");
    return groups * kPieceFloats * (long)sizeof(float);
}

int ddrr_warp_forward(const float *V, int Dx, int Dy, int Dz, const float *displacement, int Gx, int Gy,
                      int Gz, int padding, float *W, void *) {
    if (!V || !displacement || !W) return fail(-1, "null pointer");
    const Shape s = {{Dx, Dy, Dz}, {Gx, Gy, Gz}};
    if (check(s, padding)) return -1;
    for (int x = 0; x < Dx; ++x)
        for (int y = 0; y < Dy; ++y)
            for (int z0 = 0; z0 < Dz; z0 += 4) {  // one thread of the forward kernel
                float out[4];
                forward_run(V, s, displacement, padding, x, y, z0, out);
                for (int k = 0; k < 4 && z0 + k < Dz; ++k) W[((long)x * Dy + y) * Dz + z0 + k] = out[k];
            }
    return 0;
}

int ddrr_warp_backward_displacement(const float *V, int Dx, int Dy, int Dz, const float *displacement,
                                    int Gx, int Gy, int Gz, int padding, const float *gW, void *ws_raw,
                                    long ws_bytes, float *gU, void *) {
    if (!V || !displacement || !gW || !ws_raw || !gU) return fail(-1, "null pointer");
    const Shape s = {{Dx, Dy, Dz}, {Gx, Gy, Gz}};
    if (check(s, padding)) return -1;
    const long need = ddrr_warp_workspace_bytes(Dx, Dy, Dz, Gx, Gy, Gz);
    if (need < 0) return -1;
    if (ws_bytes < need) return fail(-1, "ws_bytes is smaller than ddrr_warp_workspace_bytes");
    if (reinterpret_cast<uintptr_t>(ws_raw) & 3) return fail(-1, "ws must be 4-byte aligned");
    float *ws = reinterpret_cast<float *>(ws_raw);
    const long pieces = pieces_per_cell(s);
    std::vector<float> red((size_t)kPieceFloats * kRedStride);
    long group = 0;
    for (int cx = 0; cx < Gx - 1; ++cx)
        for (int cy = 0; cy < Gy - 1; ++cy)
            for (int cz = 0; cz < Gz - 1; ++cz)
                for (long piece = 0; piece < pieces; ++piece, ++group) {
                    for (int tid = 0; tid < kBlock; ++tid) {
                        float acc[kPieceFloats];
                        piece_thread(V, s, displacement, padding, gW, cx, cy, cz, (unsigned)piece, tid, acc);
                        for (int e = 0; e < kPieceFloats; ++e) red[(size_t)e * kRedStride + tid] = acc[e];
                    }
                    for (int e = 0; e < kPieceFloats; ++e) {
                        float v = slice_sum(red.data() + (size_t)e * kRedStride, 0);
                        for (int sl = 1; sl < kSlices; ++sl) v += slice_sum(red.data() + (size_t)e * kRedStride, sl);
                        ws[group * kPieceFloats + e] = v;
                    }
                }
    for (int a = 0; a < 3; ++a)
        for (int i = 0; i < Gx; ++i)
            for (int j = 0; j < Gy; ++j)
                for (int k = 0; k < Gz; ++k)
                    gU[(((long)a * Gx + i) * Gy + j) * Gz + k] = node_sum(ws, s, pieces, a, i, j, k);
    return 0;
}

int ddrr_warp_backward_volume(const float *displacement, int Gx, int Gy, int Gz, int Dx, int Dy, int Dz,
                              int padding, const float *gW, float *gV, void *) {
    if (!displacement || !gW || !gV) return fail(-1, "null pointer");
    const Shape s = {{Dx, Dy, Dz}, {Gx, Gy, Gz}};
    if (check(s, padding)) return -1;
    memset(gV, 0, (size_t)Dx * Dy * Dz * sizeof(float));
    for (int x = 0; x < Dx; ++x)
        for (int y = 0; y < Dy; ++y)
            for (int z = 0; z < Dz; ++z) {
                long o[8];
                float w[8];
                scatter_terms(s, displacement, padding, x, y, z, gW[((long)x * Dy + y) * Dz + z], o, w);
                for (int c = 0; c < 8; ++c)
                    if (w[c] != 0.f) gV[o[c]] += w[c];
            }
    return 0;
}

}  // extern "C"

#ifdef WARP_EMU_MAIN
// The memory check: every entry on exactly-sized heap buffers, displacements of +-12 voxels with both
// paddings (most samples leave the volume) and the smallest case; a sanitizer build reports any access
// outside them.
namespace {

unsigned g_seed = 12345u;

float uniform() {  // in [0, 1)
    g_seed = g_seed * 1664525u + 1013904223u;
    return (float)(g_seed >> 8) / 16777216.f;
}

int run(int Dx, int Dy, int Dz, int Gx, int Gy, int Gz, float amplitude, int padding) {
    const size_t n = (size_t)Dx * Dy * Dz, m = (size_t)3 * Gx * Gy * Gz;
    std::vector<float> V(n), gW(n), W(n), gV(n), U(m), gU(m);
    for (float &v : V) v = uniform();
    for (float &v : gW) v = uniform();
    for (float &v : U) v = (2.f * uniform() - 1.f) * amplitude;
    const long bytes = ddrr_warp_workspace_bytes(Dx, Dy, Dz, Gx, Gy, Gz);
    if (bytes < 0) return 1;
    std::vector<float> ws((size_t)bytes / sizeof(float));
    int rc = ddrr_warp_forward(V.data(), Dx, Dy, Dz, U.data(), Gx, Gy, Gz, padding, W.data(), nullptr);
    rc |= ddrr_warp_backward_displacement(V.data(), Dx, Dy, Dz, U.data(), Gx, Gy, Gz, padding, gW.data(), ws.data(),
                                          bytes, gU.data(), nullptr);
    rc |= ddrr_warp_backward_volume(U.data(), Gx, Gy, Gz, Dx, Dy, Dz, padding, gW.data(), gV.data(), nullptr);
    double sw = 0, su = 0, sv = 0;
    for (float v : W) sw += v;
    for (float v : gU) su += v;
    for (float v : gV) sv += v;
    printf("%dx%dx%d lattice (%d, %d, %d) +-%g padding %d: rc %d, sums %.6g %.6g %.6g\n", Dx, Dy, Dz, Gx, Gy, Gz,
           amplitude, padding, rc, sw, su, sv);
    return rc;
}

}  // namespace

int main() {
    int rc = 0;
    for (int padding = 0; padding < 2; ++padding) {
        rc |= run(23, 30, 37, 4, 5, 3, 12.f, padding);
        rc |= run(9, 10, 133, 2, 3, 17, 12.f, padding);
        rc |= run(2, 2, 2, 2, 2, 2, 2.5f, padding);
        rc |= run(2, 2, 2, 2, 2, 2, 12.f, padding);
        // rows of several z chunks, a node per voxel, axes at the 65535 limit (tests/warp_cases.py)
        rc |= run(5, 6, 600, 3, 4, 7, 12.f, padding);
        rc |= run(6, 5, 515, 2, 5, 515, 12.f, padding);
        rc |= run(3, 4, 1024, 3, 2, 33, 12.f, padding);
        rc |= run(65535, 2, 3, 9, 2, 2, 12.f, padding);
        rc |= run(3, 65535, 2, 2, 65535, 2, 12.f, padding);
        rc |= run(2, 3, 65535, 2, 3, 700, 12.f, padding);
    }
    return rc;
}
#endif
