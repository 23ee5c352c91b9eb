// Host build of csrc/polyrigid_core.h behind the C ABI of include/diffdrr_polyrigid_hip.h: the loops of the
// gfx950 kernels (csrc/polyrigid.hip) over threads, pieces and slices, one element at a time, the sums in the
// kernels' order.  Compiled by tests/polyrigid_cases.py with g++; no HIP, no GPU.  Pointers are host pointers;
// `stream` is ignored.  With -DPOLYRIGID_EMU_MAIN it is a program of its own that runs the entries on cases whose
// samples leave the volume (built with -fsanitize=address,undefined: the memory check of the index arithmetic).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../diffdrr_amd/csrc/polyrigid_core.h"

namespace {

using namespace ddrr_polyrigid;

thread_local char g_err[512] = "";

int fail(int code, const char *what) {
    snprintf(g_err, sizeof(g_err), "%s", what);
    return code;
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
                           float hx, float hy, float hz, int padding, float *W, void *) {
    if (!V || !Xi || !W) return fail(-1, "null pointer");
    const Geometry g = {{{Dx, Dy, Dz}, {Gx, Gy, Gz}}, {hx, hy, hz}};
    if (check(g, padding)) return -1;
    for (int x = 0; x < Dx; ++x)
        for (int y = 0; y < Dy; ++y)
            for (int z0 = 0; z0 < Dz; z0 += 4) {  // one thread of the forward kernel
                float out[4];
                forward_run(V, g, Xi, padding, x, y, z0, out);
                for (int k = 0; k < 4 && z0 + k < Dz; ++k) W[((long)x * Dy + y) * Dz + z0 + k] = out[k];
            }
    return 0;
}

int ddrr_polyrigid_backward_twists(const float *V, int Dx, int Dy, int Dz, const float *Xi, int Gx, int Gy,
                                   int Gz, float hx, float hy, float hz, int padding, const float *gW,
                                   void *ws_raw, long ws_bytes, float *gXi, void *) {
    if (!V || !Xi || !gW || !ws_raw || !gXi) return fail(-1, "null pointer");
    const Geometry g = {{{Dx, Dy, Dz}, {Gx, Gy, Gz}}, {hx, hy, hz}};
    if (check(g, padding)) return -1;
    const long need = ddrr_polyrigid_workspace_bytes(Dx, Dy, Dz, Gx, Gy, Gz);
    if (need < 0) return -1;
    if (ws_bytes < need) return fail(-1, "ws_bytes is smaller than ddrr_polyrigid_workspace_bytes");
    if (reinterpret_cast<uintptr_t>(ws_raw) & 3) return fail(-1, "ws must be 4-byte aligned");
    float *ws = reinterpret_cast<float *>(ws_raw);
    const long pieces = pieces_per_cell(g.s);
    std::vector<float> red((size_t)kPieceFloats * kRedStride);  // (both passes of the kernel's reduction)
    long group = 0;
    for (int cx = 0; cx < Gx - 1; ++cx)
        for (int cy = 0; cy < Gy - 1; ++cy)
            for (int cz = 0; cz < Gz - 1; ++cz)
                for (long piece = 0; piece < pieces; ++piece, ++group) {
                    for (int tid = 0; tid < kBlock; ++tid) {
                        float acc[kPieceFloats];
                        piece_thread(V, g, Xi, padding, gW, cx, cy, cz, (unsigned)piece, tid, acc);
                        for (int e = 0; e < kPieceFloats; ++e) red[(size_t)e * kRedStride + tid] = acc[e];
                    }
                    for (int e = 0; e < kPieceFloats; ++e) {
                        float v = slice_sum(red.data() + (size_t)e * kRedStride, 0);
                        for (int sl = 1; sl < kSlices; ++sl) v += slice_sum(red.data() + (size_t)e * kRedStride, sl);
                        ws[group * kPieceFloats + e] = v;
                    }
                }
    for (int c = 0; c < kTwist; ++c)
        for (int i = 0; i < Gx; ++i)
            for (int j = 0; j < Gy; ++j)
                for (int k = 0; k < Gz; ++k)
                    gXi[(((long)c * Gx + i) * Gy + j) * Gz + k] = twist_node_sum(ws, g.s, pieces, c, i, j, k);
    return 0;
}

int ddrr_polyrigid_backward_volume(const float *Xi, int Gx, int Gy, int Gz, int Dx, int Dy, int Dz, float hx,
                                   float hy, float hz, int padding, const float *gW, float *gV, void *) {
    if (!Xi || !gW || !gV) return fail(-1, "null pointer");
    const Geometry g = {{{Dx, Dy, Dz}, {Gx, Gy, Gz}}, {hx, hy, hz}};
    if (check(g, padding)) return -1;
    memset(gV, 0, (size_t)Dx * Dy * Dz * sizeof(float));
    for (int x = 0; x < Dx; ++x)
        for (int y = 0; y < Dy; ++y)
            for (int z = 0; z < Dz; ++z) {
                long o[8];
                float w[8];
                scatter_terms(g, Xi, padding, x, y, z, gW[((long)x * Dy + y) * Dz + z], o, w);
                for (int c = 0; c < 8; ++c)
                    if (w[c] != 0.f) gV[o[c]] += w[c];
            }
    return 0;
}

}  // extern "C"

#ifdef POLYRIGID_EMU_MAIN
// The memory check: every entry on exactly-sized heap buffers, twists of the tests' large amplitude (rotations of
// up to 0.3 rad, translations of up to 6 mm: a third to most of the samples leave the volume) with both paddings
// and the smallest case; a sanitizer build reports any access outside them.
namespace {

unsigned g_seed = 12345u;

float uniform() {  // in [0, 1)
    g_seed = g_seed * 1664525u + 1013904223u;
    return (float)(g_seed >> 8) / 16777216.f;
}

int run(int Dx, int Dy, int Dz, int Gx, int Gy, int Gz, float rotation, float translation, int padding) {
    const size_t n = (size_t)Dx * Dy * Dz, nodes = (size_t)Gx * Gy * Gz, m = 6 * nodes;
    std::vector<float> V(n), gW(n), W(n), gV(n), Xi(m), gXi(m);
    for (float &v : V) v = uniform();
    for (float &v : gW) v = uniform();
    for (size_t i = 0; i < m; ++i) Xi[i] = (2.f * uniform() - 1.f) * (i < 3 * nodes ? rotation : translation);
    const long bytes = ddrr_polyrigid_workspace_bytes(Dx, Dy, Dz, Gx, Gy, Gz);
    if (bytes < 0) return 1;
    std::vector<float> ws((size_t)bytes / sizeof(float));
    const float h[3] = {0.8f, 1.0f, 2.5f};
    int rc = ddrr_polyrigid_forward(V.data(), Dx, Dy, Dz, Xi.data(), Gx, Gy, Gz, h[0], h[1], h[2], padding, W.data(),
                                    nullptr);
    rc |= ddrr_polyrigid_backward_twists(V.data(), Dx, Dy, Dz, Xi.data(), Gx, Gy, Gz, h[0], h[1], h[2], padding,
                                         gW.data(), ws.data(), bytes, gXi.data(), nullptr);
    rc |= ddrr_polyrigid_backward_volume(Xi.data(), Gx, Gy, Gz, Dx, Dy, Dz, h[0], h[1], h[2], padding, gW.data(),
                                         gV.data(), nullptr);
    double sw = 0, su = 0, sv = 0;
    for (float v : W) sw += v;
    for (float v : gXi) su += v;
    for (float v : gV) sv += v;
    printf("%dx%dx%d lattice (%d, %d, %d) rotation +-%g translation +-%g padding %d: rc %d, sums %.6g %.6g %.6g\n", Dx,
           Dy, Dz, Gx, Gy, Gz, rotation, translation, padding, rc, sw, su, sv);
    return rc;
}

}  // namespace

int main() {
    int rc = 0;
    for (int padding = 0; padding < 2; ++padding) {
        rc |= run(23, 30, 37, 4, 5, 3, 0.3f, 6.f, padding);
        rc |= run(9, 10, 133, 2, 3, 17, 0.3f, 6.f, padding);
        rc |= run(40, 36, 130, 3, 3, 5, 0.3f, 6.f, padding);
        rc |= run(2, 2, 2, 2, 2, 2, 0.05f, 1.5f, padding);
        rc |= run(2, 2, 2, 2, 2, 2, 2.f, 600.f, padding);  // (the closed forms; every sample far outside)
        // rows of several z chunks, a node per voxel, axes at the 65535 limit (tests/warp_cases.py)
        rc |= run(5, 6, 600, 3, 4, 7, 0.3f, 6.f, padding);
        rc |= run(6, 5, 515, 2, 5, 515, 0.3f, 6.f, padding);
        rc |= run(3, 4, 1024, 3, 2, 33, 0.3f, 6.f, padding);
        rc |= run(65535, 2, 3, 9, 2, 2, 0.3f, 6.f, padding);
        rc |= run(3, 65535, 2, 2, 65535, 2, 0.3f, 6.f, padding);
        rc |= run(2, 3, 65535, 2, 3, 700, 0.3f, 6.f, padding);
    }
    return rc;
}
#endif
