// Host build of csrc/bspline_core.h behind the C ABI of include/diffdrr_bspline_hip.h: the loops of the gfx950
// kernels (csrc/bspline.hip) over workgroups, rows, chunks, lanes and node tasks, one element at a time, the
// sums in the kernels' order.  Compiled by tests/bspline_cases.py with g++; no HIP, no GPU.  Pointers are host
// pointers; `stream` is ignored.  With -DBSPLINE_EMU_MAIN it is a program of its own that runs the entries on
// cases whose samples leave the volume (built with -fsanitize=address,undefined: the memory check of the index
// arithmetic).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../diffdrr_amd/csrc/bspline_core.h"

namespace {

using namespace ddrr_bspline;

thread_local char g_err[512] = "";

int fail(int code, const char *what) {
    snprintf(g_err, sizeof(g_err), "%s", what);
    return code;
}

int check(const Shape &s, int padding) {
    const char *what = domain_error(s, padding);
    return what ? fail(-1, what) : 0;
}

// a wave's fill_line: exactly kLineValues doubles, so that a sanitizer sees an index past the LDS array
void fill_line(const float *disp, const Shape &s, int x, int y, Span span, std::vector<double> &L) {
    L.assign(kLineValues, 0.0);
    const Taps tx = taps_of(x, s.D[0], s.G[0]), ty = taps_of(y, s.D[1], s.G[1]);
    const int count = span.hi - span.lo + 1;
    for (int v = 0; v < 3 * count; ++v) {
        const int a = v / count, j = v - a * count;
        L.at((size_t)a * kLineNodes + j) = line_value(disp, s.G, tx, ty, a, clamp_node(span.lo + j, s.G[2]));
    }
}

// out[o, m, i]: bspline_gather_kernel
void gather(const float *src, int D, int G, long inner, long count, float *out) {
    for (long e = 0; e < count; ++e) {
        const long om = e / inner, i = e - om * inner, o = om / G;
        out[e] = gather_axis(src + o * D * inner + i, inner, D, G, (int)(om - o * G));
    }
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
                         int Gz, int padding, float *W, void *) {
    if (!V || !displacement || !W) return fail(-1, "null pointer");
    const Shape s = {{Dx, Dy, Dz}, {Gx, Gy, Gz}};
    if (check(s, padding)) return -1;
    std::vector<double> L;
    for (int x = 0; x < Dx; ++x)
        for (int y = 0; y < Dy; ++y)
            for (int zlo = 0; zlo < Dz; zlo += kChunk) {  // one wave of the forward kernel
                const int zend = zlo + kChunk < Dz ? zlo + kChunk : Dz;
                const Span span = chunk_span(zlo, zend, Dz, Gz);
                fill_line(displacement, s, x, y, span, L);
                for (int z0 = zlo; z0 < zend; z0 += 4) {
                    float out[4];
                    forward_run(V, s, padding, L.data(), span.lo, x, y, z0, out);
                    for (int k = 0; k < 4 && z0 + k < Dz; ++k) W[((long)x * Dy + y) * Dz + z0 + k] = out[k];
                }
            }
    return 0;
}

int ddrr_bspline_backward_displacement(const float *V, int Dx, int Dy, int Dz, const float *displacement,
                                       int Gx, int Gy, int Gz, int padding, const float *gW, void *ws_raw,
                                       long ws_bytes, float *gU, void *) {
    if (!V || !displacement || !gW || !ws_raw || !gU) return fail(-1, "null pointer");
    const Shape s = {{Dx, Dy, Dz}, {Gx, Gy, Gz}};
    if (check(s, padding)) return -1;
    if (ws_bytes < ddrr_bspline_workspace_bytes(Dx, Dy, Dz, Gx, Gy, Gz))
        return fail(-1, "ws_bytes is smaller than ddrr_bspline_workspace_bytes");
    if (reinterpret_cast<uintptr_t>(ws_raw) & 3) return fail(-1, "ws must be 4-byte aligned");
    float *r1 = reinterpret_cast<float *>(ws_raw), *r2 = r1 + r1_floats(s);
    std::vector<double> L;
    std::vector<float> q((size_t)3 * kPadded), wz((size_t)4 * kPadded);
    for (int x = 0; x < Dx; ++x)
        for (int y = 0; y < Dy; ++y) {  // one wave of the rows kernel
            int done = -1;
            for (int zlo = 0; zlo < Dz; zlo += kChunk) {
                const int zend = zlo + kChunk < Dz ? zlo + kChunk : Dz;
                const Span span = chunk_span(zlo, zend, Dz, Gz);
                fill_line(displacement, s, x, y, span, L);
                for (int z = zlo; z < zend; ++z) {
                    float w[4], qv[3];
                    node_weights(z, Dz, Gz, w);
                    for (int k = 0; k < 4; ++k) wz[(size_t)k * kPadded + padded(z - zlo)] = w[k];
                    voxel_q(V, s, padding, L.data(), span.lo, x, y, z, gW[((long)x * Dy + y) * Dz + z], qv);
                    for (int a = 0; a < 3; ++a) q[(size_t)a * kPadded + padded(z - zlo)] = qv[a];
                }
                const int nlo = span.lo < 0 ? 0 : span.lo, nhi = span.hi > Gz - 1 ? Gz - 1 : span.hi;
                for (int a = 0; a < 3; ++a)
                    for (int n = nlo; n <= nhi; ++n) {
                        float *dst = r1 + (((long)a * Dx + x) * Dy + y) * Gz + n;
                        *dst = node_chain(q.data() + (size_t)a * kPadded, wz.data(), Dz, Gz, n, zlo, zend,
                                          n > done ? 0.f : *dst);
                    }
                done = nhi;
            }
        }
    gather(r1, Dy, Gy, Gz, r2_floats(s), r2);
    gather(r2, Dx, Gx, (long)Gy * Gz, 3L * Gx * Gy * Gz, gU);
    return 0;
}

int ddrr_bspline_backward_volume(const float *displacement, int Gx, int Gy, int Gz, int Dx, int Dy, int Dz,
                                 int padding, const float *gW, float *gV, void *) {
    if (!displacement || !gW || !gV) return fail(-1, "null pointer");
    const Shape s = {{Dx, Dy, Dz}, {Gx, Gy, Gz}};
    if (check(s, padding)) return -1;
    memset(gV, 0, (size_t)Dx * Dy * Dz * sizeof(float));
    std::vector<double> L;
    for (int x = 0; x < Dx; ++x)
        for (int y = 0; y < Dy; ++y)
            for (int zlo = 0; zlo < Dz; zlo += kChunk) {
                const int zend = zlo + kChunk < Dz ? zlo + kChunk : Dz;
                const Span span = chunk_span(zlo, zend, Dz, Gz);
                fill_line(displacement, s, x, y, span, L);
                for (int z = zlo; z < zend; ++z) {
                    long o[8];
                    float w[8];
                    scatter_terms(s, padding, L.data(), span.lo, x, y, z, gW[((long)x * Dy + y) * Dz + z], o, w);
                    for (int c = 0; c < 8; ++c)
                        if (w[c] != 0.f) gV[o[c]] += w[c];
                }
            }
    return 0;
}

}  // extern "C"

#ifdef BSPLINE_EMU_MAIN
// The memory check: every entry on exactly-sized heap buffers, coefficients of +-24 voxels with both paddings
// (many samples leave the volume), a row of several chunks and the smallest case; a sanitizer build reports
// any access outside them.
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
    const long bytes = ddrr_bspline_workspace_bytes(Dx, Dy, Dz, Gx, Gy, Gz);
    if (bytes < 0) return 1;
    std::vector<float> ws((size_t)bytes / sizeof(float));
    int rc = ddrr_bspline_forward(V.data(), Dx, Dy, Dz, U.data(), Gx, Gy, Gz, padding, W.data(), nullptr);
    rc |= ddrr_bspline_backward_displacement(V.data(), Dx, Dy, Dz, U.data(), Gx, Gy, Gz, padding, gW.data(),
                                             ws.data(), bytes, gU.data(), nullptr);
    rc |= ddrr_bspline_backward_volume(U.data(), Gx, Gy, Gz, Dx, Dy, Dz, padding, gW.data(), gV.data(), nullptr);
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
        rc |= run(23, 30, 37, 4, 5, 3, 24.f, padding);
        rc |= run(37, 41, 45, 7, 6, 8, 24.f, padding);
        rc |= run(5, 6, 700, 2, 3, 700, 24.f, padding);  // one node per z voxel: the widest line a chunk can need
        rc |= run(5, 6, 600, 2, 3, 9, 24.f, padding);    // chains that continue across chunks
        rc |= run(2, 2, 2, 2, 2, 2, 2.5f, padding);
        rc |= run(2, 2, 2, 2, 2, 2, 24.f, padding);
        // rows of several z chunks, a node per voxel, axes at the 65535 limit (tests/warp_cases.py)
        rc |= run(5, 6, 600, 3, 4, 7, 24.f, padding);
        rc |= run(6, 5, 515, 2, 5, 515, 24.f, padding);
        rc |= run(3, 4, 1024, 3, 2, 33, 24.f, padding);
        rc |= run(65535, 2, 3, 9, 2, 2, 24.f, padding);
        rc |= run(3, 65535, 2, 2, 65535, 2, 24.f, padding);
        rc |= run(2, 3, 65535, 2, 3, 700, 24.f, padding);
    }
    return rc;
}
#endif
