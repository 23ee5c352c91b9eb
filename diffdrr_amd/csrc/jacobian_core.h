// jacobian_core.h -- the arithmetic of the Jacobian kernels (jacobian.hip; include/diffdrr_jacobian_hip.h has
// the definitions): the derivative weights of the cubic B-spline, a voxel's taps per basis, the nine (x, y) sums
// of the lattice that make a row's lines at a z node, J from two or four entries of those lines, the determinant
// and the cofactors, psi and psi', the statistics a workgroup reduces, and the chains of the lattice gradient.
// The lines are accumulated in double and kept in float: nothing here takes a floor, so nothing downstream needs
// more than the float they round to, and the double sum costs nothing per voxel (a line serves a whole chunk).
// The lattice geometry is warp_core.h's, the B-spline weights, their folding and the z chains bspline_core.h's:
// both are included, not edited.  Host and device (DDRR_HD): tests/emu/jacobian_emu.cpp compiles the same
// functions for the CPU.
#pragma once

#include <math.h>

#include "../../include/diffdrr_jacobian_hip.h"
#include "bspline_core.h"

namespace ddrr_jacobian {

using ddrr_bspline::clamp_node;
using ddrr_bspline::fold;
using ddrr_bspline::frac_of;
using ddrr_bspline::kBlock;
using ddrr_bspline::kChunk;
using ddrr_bspline::kLanes;
using ddrr_bspline::kLineNodes;
using ddrr_bspline::kPadded;
using ddrr_bspline::kRows;
using ddrr_bspline::kSlots;
using ddrr_bspline::node_chain;
using ddrr_bspline::padded;
using ddrr_bspline::Span;
using ddrr_bspline::weights;
using ddrr_warp::Box;
using ddrr_warp::cell_begin;
using ddrr_warp::cell_box;
using ddrr_warp::cell_of;
using ddrr_warp::cells_of;
using ddrr_warp::frac_in;
using ddrr_warp::kPer;
using ddrr_warp::kPieceFloats;
using ddrr_warp::kPieceVoxels;
using ddrr_warp::pieces_per_cell;
using ddrr_warp::Shape;

constexpr int LINEAR = DDRR_JACOBIAN_BASIS_LINEAR, BSPLINE = DDRR_JACOBIAN_BASIS_BSPLINE;
constexpr int kLines = 9;                          // (w_x w_y, w'_x w_y, w_x w'_y) x three components
// a row's lines in LDS are [3 kind + component][node - lo], `stride` floats apart: line_stride() of the shape
constexpr int kRowFloats = kLines * kPadded;       // a chunk's nine c_ab per voxel of a row in LDS, padded
constexpr int kGradRows = 2, kGradBlock = kGradRows * kLanes;  // rows of a workgroup of the rows kernel (LDS)
static_assert(ddrr_warp::kBlock == kBlock, "one workgroup size");

// the taps of a basis on an axis: their number and the first one's node relative to the cell
template <int BASIS>
struct Basis {
    static constexpr int taps = BASIS == BSPLINE ? 4 : 2, first = BASIS == BSPLINE ? -1 : 0;
};

// the domain of every entry (include/diffdrr_jacobian_hip.h); nullptr, or what is wrong
inline const char *argument_error(const Shape &s, int basis) {
    const char *what = ddrr_warp::domain_error(s, DDRR_WARP_PADDING_ZEROS);
    if (what) return what;
    if (basis != LINEAR && basis != BSPLINE)
        return "basis must be DDRR_JACOBIAN_BASIS_LINEAR or DDRR_JACOBIAN_BASIS_BSPLINE";
    return nullptr;
}

inline const char *eps_error(double eps) { return eps > 0.0 && eps <= 1.0 ? nullptr : "eps must be in (0, 1]"; }

// ------------------------------------------------------------------------------------------------ workspace
// what a workgroup of the forward kernel leaves: psi sum, folded count, min and max of its voxels
struct Partial {
    double sum;
    long count;
    float lo, hi;
};
static_assert(sizeof(Partial) == DDRR_JACOBIAN_PARTIAL_BYTES, "the partials of the workspace formula");

inline long chunks_of(const Shape &s) { return (s.D[2] + kChunk - 1) / kChunk; }
inline long groups_of(const Shape &s) { return chunks_of(s) * ((s.D[1] + kRows - 1) / kRows) * s.D[0]; }
DDRR_HD long plane1_floats(const Shape &s) { return 3L * s.D[0] * s.D[1] * s.G[2]; }  // one k of r1
DDRR_HD long plane2_floats(const Shape &s) { return 3L * s.D[0] * s.G[1] * s.G[2]; }  // one k of r2

// bytes of ws; -1: the linear gradient would need more than 2^31 - 1 workgroups
inline long workspace_bytes(const Shape &s, int basis) {
    const long forward = groups_of(s) * (long)sizeof(Partial);
    long backward;
    if (basis == BSPLINE) {
        backward = (3 * plane1_floats(s) + 2 * plane2_floats(s)) * (long)sizeof(float);
    } else {
        const long groups = cells_of(s) * pieces_per_cell(s);
        if (groups > 0x7fffffffL) return -1;
        backward = groups * kPieceFloats * (long)sizeof(float);
    }
    return forward > backward ? forward : backward;
}

// ------------------------------------------------------------------------------------------------ the basis
template <typename T>
DDRR_HD void derivative_weights(T t, T B[4]) {
    const T s = T(1) - t, half = T(0.5);
    B[0] = -(s * s) * half;
    B[1] = (T(3) * t - T(4)) * t * half;
    B[2] = ((T(-3) * t + T(2)) * t + T(1)) * half;
    B[3] = t * t * half;
}

// weights w and derivative weights d of a fraction, per tap of the basis
template <int BASIS, typename T>
DDRR_HD void tap_weights(T t, T w[4], T d[4]) {
    if (BASIS == BSPLINE) {
        weights(t, w);
        derivative_weights(t, d);
    } else {
        w[0] = T(1) - t, w[1] = t, w[2] = w[3] = T(0);
        d[0] = T(-1), d[1] = T(1), d[2] = d[3] = T(0);
    }
}

// the taps of voxel x of an axis: nodes (clamped) with their weights and derivative weights
struct Taps {
    int n[4];
    double w[4], d[4];
};

template <int BASIS>
DDRR_HD Taps taps_of(int x, int D, int G) {
    const int c = cell_of(x, D, G).c;
    Taps r;
    tap_weights<BASIS>(frac_of(x, c, D, G), r.w, r.d);
#pragma unroll
    for (int k = 0; k < 4; ++k) r.n[k] = clamp_node(c + Basis<BASIS>::first + k, G);
    return r;
}

// component a of the row's three lines at z node k (0 <= k < Gz): per x tap the two y sums (with w_y and with
// w'_y), then the three x sums, taps ascending, in double
template <int BASIS>
DDRR_HD void line_values(const float *disp, const int G[3], const Taps &tx, const Taps &ty, int a, int k,
                         float out[3]) {
    const long plane = (long)G[1] * G[2], all = plane * G[0];
    const float *d = disp + a * all + k;
    double v = 0.0, vx = 0.0, vy = 0.0;
#pragma unroll
    for (int i = 0; i < Basis<BASIS>::taps; ++i) {
        double sy = 0.0, dy = 0.0;  // the y sums of x tap i
#pragma unroll
        for (int j = 0; j < Basis<BASIS>::taps; ++j) {
            const double u = d[tx.n[i] * plane + (long)ty.n[j] * G[2]];
            sy += ty.w[j] * u;
            dy += ty.d[j] * u;
        }
        v += tx.w[i] * sy;
        vx += tx.d[i] * sy;
        vy += tx.w[i] * dy;
    }
    out[0] = (float)v, out[1] = (float)vx, out[2] = (float)vy;
}

// the z nodes (not clamped) the voxels [zlo, zend) of a row reach: entry j of a line is node lo + j
template <int BASIS>
DDRR_HD Span chunk_span(int zlo, int zend, int D, int G) {
    Span r;
    r.lo = cell_of(zlo, D, G).c + Basis<BASIS>::first;
    r.hi = cell_of(zend - 1, D, G).c + Basis<BASIS>::first + Basis<BASIS>::taps - 1;
    return r;
}

// the most z nodes a chunk of a row reaches (<= kLineNodes): what the kernels size a row's lines in LDS by, so
// that a coarse lattice does not pay for the one-node-per-voxel case in occupancy
template <int BASIS>
inline int line_stride(const Shape &s) {
    int m = 0;
    for (int zlo = 0; zlo < s.D[2]; zlo += kChunk) {
        const Span span = chunk_span<BASIS>(zlo, zlo + kChunk < s.D[2] ? zlo + kChunk : s.D[2], s.D[2], s.G[2]);
        m = span.hi - span.lo + 1 > m ? span.hi - span.lo + 1 : m;
    }
    return m;
}

// task v of a wave's fill (0 <= v < 3 count): component a = v / count of the lines at node lo + v % count
template <int BASIS>
DDRR_HD void fill_task(const float *disp, const Shape &s, const Taps &tx, const Taps &ty, Span span, int v, int stride,
                       float *L) {
    const int count = span.hi - span.lo + 1, a = v / count, j = v - a * count;
    float out[3];
    line_values<BASIS>(disp, s.G, tx, ty, a, clamp_node(span.lo + j, s.G[2]), out);
#pragma unroll
    for (int kind = 0; kind < 3; ++kind) L[(3 * kind + a) * stride + j] = out[kind];
}

// s_b = (G_b - 1) / (D_b - 1)
DDRR_HD void scales_of(const Shape &s, float sc[3]) {
#pragma unroll
    for (int b = 0; b < 3; ++b) sc[b] = (float)(s.G[b] - 1) / (float)(s.D[b] - 1);
}

// J (row major, [3 a + b]) of a voxel of z cell c at fraction t from the row's lines
template <int BASIS>
DDRR_HD void jacobian_of(const float *L, int stride, int lo, int c, float t, const float sc[3], float J[9]) {
    float w[4], d[4];
    tap_weights<BASIS>(t, w, d);
    const float *p = L + (c + Basis<BASIS>::first - lo);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float jx = 0.f, jy = 0.f, jz = 0.f;
#pragma unroll
        for (int k = 0; k < Basis<BASIS>::taps; ++k) {
            jz += d[k] * p[a * stride + k];
            jx += w[k] * p[(3 + a) * stride + k];
            jy += w[k] * p[(6 + a) * stride + k];
        }
        J[3 * a + 0] = sc[0] * jx;
        J[3 * a + 1] = sc[1] * jy;
        J[3 * a + 2] = sc[2] * jz;
        J[3 * a + a] += 1.f;
    }
}

// cof_ab = d det / d J_ab
DDRR_HD void cofactors(const float J[9], float C[9]) {
    C[0] = J[4] * J[8] - J[5] * J[7];
    C[1] = J[5] * J[6] - J[3] * J[8];
    C[2] = J[3] * J[7] - J[4] * J[6];
    C[3] = J[2] * J[7] - J[1] * J[8];
    C[4] = J[0] * J[8] - J[2] * J[6];
    C[5] = J[1] * J[6] - J[0] * J[7];
    C[6] = J[1] * J[5] - J[2] * J[4];
    C[7] = J[2] * J[3] - J[0] * J[5];
    C[8] = J[0] * J[4] - J[1] * J[3];
}

// the expansion along the first row
DDRR_HD float determinant(const float J[9]) {
    return J[0] * (J[4] * J[8] - J[5] * J[7]) + J[1] * (J[5] * J[6] - J[3] * J[8]) + J[2] * (J[3] * J[7] - J[4] * J[6]);
}

// ------------------------------------------------------------------------------------------------ the penalty
DDRR_HD double psi(double d, double eps) {
    if (d >= eps) {
        const double l = log(d);
        return l * l;
    }
    const double le = log(eps), x = d - eps;
    return le * le + (2.0 * le / eps) * x + ((1.0 - le) / (eps * eps)) * x * x;
}

// psi' in float: the gradient's upstream factor (its error is relative to itself, like that of c_ab)
DDRR_HD float psi_prime(float d, float eps) {
    if (d >= eps) return 2.f * logf(d) / d;
    const float le = logf(eps);
    return 2.f * le / eps + (2.f * (1.f - le) / (eps * eps)) * (d - eps);
}

// the upstream gradient of a voxel: gD's, or the penalty's own, psi'(d) / N
DDRR_HD float upstream(const float *gD, long at, float d, float eps, float inv_n) {
    return gD ? gD[at] : psi_prime(d, eps) * inv_n;
}

// ------------------------------------------------------------------------------------------------ statistics
DDRR_HD Partial no_voxels() {
    Partial p;
    p.sum = 0.0, p.count = 0, p.lo = INFINITY, p.hi = -INFINITY;
    return p;
}

DDRR_HD void add_voxel(Partial &p, float d, bool penalty, double eps) {
    if (penalty) p.sum += psi((double)d, eps);
    p.count += d <= 0.f ? 1 : 0;
    p.lo = fminf(p.lo, d);
    p.hi = fmaxf(p.hi, d);
}

DDRR_HD void merge(Partial &p, const Partial &q) {
    p.sum += q.sum;
    p.count += q.count;
    p.lo = fminf(p.lo, q.lo);
    p.hi = fmaxf(p.hi, q.hi);
}

// one level of the tree over a wave's kLanes partials: entry i takes entry i + half, for half = kLanes / 2 .. 1
// (the kernel's butterfly leaves the same sum, formed in the same order, in lane 0)
DDRR_HD void tree_level(Partial *red, int half, int i) {
    if (i < half) merge(red[i], red[i + half]);
}

// ------------------------------------------------------------------------------------------------ forward
// d of the run of (up to) four z voxels from z0 of a row, added to the thread's statistics: the forward
// kernel's thread.  The z cell is stepped with frac_in's integer numerator (at most one node per step).
template <int BASIS>
DDRR_HD void forward_run(const Shape &s, const float *L, int stride, int lo, int z0, const float sc[3], bool penalty,
                         double eps, float out[4], Partial &stats) {
    int c = cell_of(z0, s.D[2], s.G[2]).c;
    unsigned r = (unsigned)z0 * (unsigned)(s.G[2] - 1) - (unsigned)c * (unsigned)(s.D[2] - 1);
    const float den = (float)(s.D[2] - 1);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        out[k] = 0.f;
        if (z0 + k < s.D[2]) {
            if (k > 0) {
                r += (unsigned)(s.G[2] - 1);
                if (r >= (unsigned)(s.D[2] - 1) && c < s.G[2] - 2) {  // the run crosses a node
                    r -= (unsigned)(s.D[2] - 1);
                    ++c;
                }
            }
            float J[9];
            jacobian_of<BASIS>(L, stride, lo, c, (float)r / den, sc, J);
            out[k] = determinant(J);
            add_voxel(stats, out[k], penalty, eps);
        }
    }
}

// ------------------------------------------------------------------------------------------------ B-spline gradient
// the nine c_ab = g cof_ab s_b of voxel z of a row, g its upstream gradient
template <int BASIS>
DDRR_HD void voxel_c(const Shape &s, const float *L, int stride, int lo, int z, long at, const float sc[3],
                     const float *gD, float eps, float inv_n, float c[9]) {
    const ddrr_warp::Cell cz = cell_of(z, s.D[2], s.G[2]);
    float J[9];
    jacobian_of<BASIS>(L, stride, lo, cz.c, cz.t, sc, J);
    cofactors(J, c);
    const float g = upstream(gD, at, determinant(J), eps, inv_n);
#pragma unroll
    for (int e = 0; e < 9; ++e) c[e] *= g * sc[e % 3];
}

// the folded weights and derivative weights of voxel x of an axis (the B-spline gradient's)
DDRR_HD void node_weights(int x, int D, int G, float w[4], float d[4]) {
    const ddrr_warp::Cell c = cell_of(x, D, G);
    tap_weights<BSPLINE>(c.t, w, d);
    fold(c.c, G, w);
    fold(c.c, G, d);
}

// the chain of node m of an axis of D voxels and G nodes, x ascending (the second and third gathers):
// acc = (acc + w'_m(x) srcD[x stride]) + w_m(x) srcW[x stride], without the first term where srcD is null; kept
// in double and rounded once, as ddrr_bspline::gather_axis
DDRR_HD float gather_pair(const float *srcD, const float *srcW, long stride, int D, int G, int m) {
    const int c0 = m - 2 < 0 ? 0 : m - 2, c1 = m + 1 > G - 2 ? G - 2 : m + 1;
    double acc = 0.0;
    for (int c = c0; c <= c1; ++c) {
        const int k = m + 1 - c, e = cell_begin(c + 1, D, G);
        for (int x = cell_begin(c, D, G); x < e; ++x) {
            float w[4], d[4];
            tap_weights<BSPLINE>(frac_in(x, c, D, G), w, d);
            fold(c, G, w);
            fold(c, G, d);
            if (srcD) acc += (double)d[k] * (double)srcD[x * stride];
            acc += (double)w[k] * (double)srcW[x * stride];
        }
    }
    return (float)acc;
}

// ------------------------------------------------------------------------------------------------ linear gradient
// J of a voxel at fractions t of the cell whose 8 nodes x 3 components are v[a][4 i + 2 j + k]
DDRR_HD void linear_jacobian(const float v[3][8], const float t[3], const float sc[3], float J[9]) {
    const float wx[2] = {1.f - t[0], t[0]}, wy[2] = {1.f - t[1], t[1]}, wz[2] = {1.f - t[2], t[2]};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float jx = 0.f, jy = 0.f, jz = 0.f;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                jx += wy[p] * wz[q] * (v[a][4 + 2 * p + q] - v[a][2 * p + q]);
                jy += wx[p] * wz[q] * (v[a][4 * p + 2 + q] - v[a][4 * p + q]);
                jz += wx[p] * wy[q] * (v[a][4 * p + 2 * q + 1] - v[a][4 * p + 2 * q]);
            }
        J[3 * a + 0] = sc[0] * jx;
        J[3 * a + 1] = sc[1] * jy;
        J[3 * a + 2] = sc[2] * jz;
        J[3 * a + a] += 1.f;
    }
}

// thread `tid` of piece `piece` of cell (cx, cy, cz): its kPer voxels, in order, into acc[3 node + a] (zeroed
// here), node = 4 i + 2 j + k of the cell (the layout of warp_core.h's pieces)
DDRR_HD void piece_thread(const Shape &s, const float *disp, const float *gD, float eps, float inv_n, int cx, int cy,
                          int cz, unsigned piece, int tid, float acc[kPieceFloats]) {
#pragma unroll
    for (int e = 0; e < kPieceFloats; ++e) acc[e] = 0.f;
    const long plane = (long)s.G[1] * s.G[2], all = plane * s.G[0];
    float v[3][8], sc[3];
    scales_of(s, sc);
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int n = 0; n < 8; ++n)
            v[a][n] = disp[a * all + (cx + (n >> 2)) * plane + (long)(cy + ((n >> 1) & 1)) * s.G[2] + cz + (n & 1)];
    const Box box = cell_box(s, cx, cy, cz);
    const unsigned count = (unsigned)box.n[0] * (unsigned)box.n[1] * (unsigned)box.n[2];  // <= 2^31
#pragma unroll 1
    for (int k = 0; k < kPer; ++k) {
        const unsigned l = piece * (unsigned)kPieceVoxels + (unsigned)(k * kBlock + tid);
        if (l >= count) break;
        const unsigned row = l / (unsigned)box.n[2];
        const int z = box.b[2] + (int)(l - row * (unsigned)box.n[2]);
        const unsigned lx = row / (unsigned)box.n[1];
        const int y = box.b[1] + (int)(row - lx * (unsigned)box.n[1]);
        const int x = box.b[0] + (int)lx;
        const float t[3] = {frac_in(x, cx, s.D[0], s.G[0]), frac_in(y, cy, s.D[1], s.G[1]),
                            frac_in(z, cz, s.D[2], s.G[2])};
        float J[9], c[9];
        linear_jacobian(v, t, sc, J);
        cofactors(J, c);
        const float g = upstream(gD, ((long)x * s.D[1] + y) * s.D[2] + z, determinant(J), eps, inv_n);
#pragma unroll
        for (int e = 0; e < 9; ++e) c[e] *= g * sc[e % 3];
        const float w[3][2] = {{1.f - t[0], t[0]}, {1.f - t[1], t[1]}, {1.f - t[2], t[2]}};
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const float hx = (i ? 1.f : -1.f) * w[1][j] * w[2][q], hy = w[0][i] * (j ? 1.f : -1.f) * w[2][q],
                                hz = w[0][i] * w[1][j] * (q ? 1.f : -1.f);
#pragma unroll
                    for (int a = 0; a < 3; ++a)
                        acc[3 * (4 * i + 2 * j + q) + a] += (c[3 * a] * hx + c[3 * a + 1] * hy) + c[3 * a + 2] * hz;
                }
    }
}

}  // namespace ddrr_jacobian
