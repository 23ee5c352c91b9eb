// polyrigid_core.h -- the arithmetic of the polyrigid deformation kernels (polyrigid.hip;
// include/diffdrr_polyrigid_hip.h has the definitions): the twist from the cell's 8 lattice nodes, A, B, C and
// their derivatives in s, the displacement exp(xi) y - y and its adjoint in xi, and a voxel's share of its cell's
// 48 sums.  The sample position is formed in double (the twist at the voxel, A, B, C, exp(xi) y - y), floor and
// fraction are taken from the double and only the fraction is rounded to float, as bspline_core.h does and for its
// reason: floor(u) decides on which side of a voxel face a sample falls, where the twist gradient jumps, and u is
// a difference of terms of |omega| |y| -- hundreds of mm on a long axis -- that float knows to 1e-5 mm at best.
// Everything after that (the interpolation, the adjoint, every sum) is float.  The lattice geometry, everything about sampling (Axis, axis_of, the corners), the pieces and the
// fixed-order sums are warp_core.h's.  Host and device (DDRR_HD): tests/emu/polyrigid_emu.cpp compiles the same
// functions for the CPU.
#pragma once

#include <math.h>

#include "../../include/diffdrr_polyrigid_hip.h"
#include "warp_core.h"

namespace ddrr_polyrigid {

using ddrr_warp::Axis;
using ddrr_warp::axis_of;
using ddrr_warp::Box;
using ddrr_warp::Cell;
using ddrr_warp::cell_box;
using ddrr_warp::cell_of;
using ddrr_warp::cells_of;
using ddrr_warp::column_weights;
using ddrr_warp::corner_offsets;
using ddrr_warp::corner_weights;
using ddrr_warp::frac_in;
using ddrr_warp::interpolate;
using ddrr_warp::interpolate_gradient;
using ddrr_warp::pieces_per_cell;
using ddrr_warp::Shape;
using ddrr_warp::slice_sum;

constexpr int kBlock = ddrr_warp::kBlock;
constexpr int kPieceVoxels = DDRR_POLYRIGID_PIECE_VOXELS;
constexpr int kPer = kPieceVoxels / kBlock;             // voxels of a thread in a piece
constexpr int kTwist = 6;                               // components of a twist: omega, v
constexpr int kPieceFloats = DDRR_POLYRIGID_PIECE_FLOATS;  // 8 nodes x 6 components
constexpr int kHalfFloats = kPieceFloats / 2;           // what one pass of the LDS reduction holds
constexpr int kSlices = ddrr_warp::kSlices, kSliceLen = ddrr_warp::kSliceLen;
constexpr int kRedStride = ddrr_warp::kRedStride;
constexpr int kTerms = DDRR_POLYRIGID_SERIES_TERMS;
constexpr float kSeriesBelow = (float)DDRR_POLYRIGID_SERIES_BELOW_NUM / (float)DDRR_POLYRIGID_SERIES_BELOW_DEN;
static_assert(kPieceVoxels == ddrr_warp::kPieceVoxels, "the pieces are the warp library's");
static_assert(kPieceFloats == 8 * kTwist && kTerms == 8, "8 nodes x 6 components; the tables below have 8 terms");
static_assert(DDRR_POLYRIGID_PADDING_ZEROS == DDRR_WARP_PADDING_ZEROS &&
                  DDRR_POLYRIGID_PADDING_BORDER == DDRR_WARP_PADDING_BORDER &&
                  DDRR_POLYRIGID_MAX_DIM == DDRR_WARP_MAX_DIM,
              "axis_of and domain_error read the warp library's codes");

struct Geometry {
    Shape s;
    float h[3];  // voxel pitch, mm
};

// the domain of every entry (include/diffdrr_polyrigid_hip.h); nullptr, or what is wrong
inline const char *domain_error(const Geometry &g, int padding) {
    if (padding != DDRR_POLYRIGID_PADDING_ZEROS && padding != DDRR_POLYRIGID_PADDING_BORDER)
        return "padding must be DDRR_POLYRIGID_PADDING_ZEROS or DDRR_POLYRIGID_PADDING_BORDER";
    const char *what = ddrr_warp::domain_error(g.s, padding);
    if (what) return what;
    for (int a = 0; a < 3; ++a)
        if (!(g.h[a] > 0.f) || !(g.h[a] <= 3.4028234e38f)) return "the voxel pitch must be positive and finite (h_a > 0)";
    return nullptr;
}

// ------------------------------------------------------------------------------------------------ the twist
DDRR_HD double lerp(double a, double b, double t) { return a + t * (b - a); }

// frac_in in double: the same exact integer numerator, one division
DDRR_HD double frac_of(int x, int c, int D, int G) {
    return (double)((unsigned)x * (unsigned)(G - 1) - (unsigned)c * (unsigned)(D - 1)) / (double)(D - 1);
}

// the six components on the lattice line (cx + tx, cy + ty, node k): along x, then along y; 24 lattice reads
DDRR_HD void twist_line(const float *Xi, const int G[3], int cx, int cy, double tx, double ty, int k,
                        double L[kTwist]) {
    const long plane = (long)G[1] * G[2], all = plane * G[0];
    const long o = (long)cx * plane + (long)cy * G[2] + k;
#pragma unroll
    for (int c = 0; c < kTwist; ++c) {
        const float *d = Xi + c * all + o;
        L[c] = lerp(lerp(d[0], d[plane], tx), lerp(d[G[2]], d[plane + G[2]], tx), ty);
    }
}

// ------------------------------------------------------------------------------------------------ A, B, C
template <typename T>
struct CoefOf {
    T A, B, C, dA, dB, dC;  // and d / d s
};
using Coef = CoefOf<float>;

constexpr double inverse_factorial(int m) {
    double f = 1.0;
    for (int i = 2; i <= m; ++i) f *= i;
    return 1.0 / f;
}

// sum_n (-s)^n / (2n + First)! and its derivative in s, kTerms terms, by Horner's rule in q = -s:
// v <- c_n + q v, and d <- v + q d is its derivative in q
template <typename T, int First, int N = kTerms - 2>
struct Series {
    static DDRR_HD void step(T s, T &v, T &d) {
        constexpr T c = (T)inverse_factorial(2 * N + First);
        d = v - s * d;
        v = c - s * v;
        Series<T, First, N - 1>::step(s, v, d);
    }
};
template <typename T, int First>
struct Series<T, First, -1> {
    static DDRR_HD void step(T, T &, T &) {}
};

template <int First, typename T>
DDRR_HD void series(T s, T &value, T &slope) {
    constexpr T last = (T)inverse_factorial(2 * (kTerms - 1) + First);
    T v = last, d = T(0);
    Series<T, First>::step(s, v, d);
    value = v;
    slope = -d;
}

DDRR_HD Coef coefficients(float s) {
    Coef k;
    if (s < kSeriesBelow) {
        series<1>(s, k.A, k.dA);
        series<2>(s, k.B, k.dB);
        series<3>(s, k.C, k.dC);
    } else {
        const float phi = sqrtf(s), sn = sinf(phi), cs = cosf(phi);
        k.A = sn / phi;
        k.B = (1.f - cs) / s;
        k.C = (phi - sn) / (s * phi);
        k.dA = 0.5f * (k.C - k.B);
        k.dB = (k.A - 2.f * k.B) / (2.f * s);
        k.dC = (k.B - 3.f * k.C) / (2.f * s);
    }
    return k;
}

// A, B, C alone, in double (the sample position's); the seam is where the float s falls, as in coefficients
DDRR_HD void coefficients(double s, double &A, double &B, double &C) {
    if ((float)s < kSeriesBelow) {
        double slope;
        series<1>(s, A, slope);
        series<2>(s, B, slope);
        series<3>(s, C, slope);
    } else {
        const double phi = sqrt(s), sn = sin(phi);
        A = sn / phi;
        B = (1.0 - cos(phi)) / s;
        C = (phi - sn) / (s * phi);
    }
}

// ------------------------------------------------------------------------------------------------ displacement
template <typename T>
DDRR_HD void cross(const T a[3], const T b[3], T r[3]) {
    r[0] = a[1] * b[2] - a[2] * b[1];
    r[1] = a[2] * b[0] - a[0] * b[2];
    r[2] = a[0] * b[1] - a[1] * b[0];
}

template <typename T>
DDRR_HD T dot(const T a[3], const T b[3]) {
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}

// mm from the volume's centre (exact in double)
DDRR_HD void centred(const Geometry &g, int x, int y, int z, double out[3]) {
    const int xs[3] = {x, y, z};
#pragma unroll
    for (int a = 0; a < 3; ++a) out[a] = (double)g.h[a] * ((double)xs[a] - 0.5 * (double)(g.s.D[a] - 1));
}

// u in voxels of each axis, from the twist xi at the voxel and its position y (mm), in double
DDRR_HD void displacement(const Geometry &g, const double xi[kTwist], const double y[3], double u[3]) {
    const double *w = xi, *v = xi + 3;
    double A, B, C;
    coefficients(dot(w, w), A, B, C);
    double a[3], b[3], wa[3], wb[3], wwb[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        a[i] = A * y[i] + B * v[i];
        b[i] = B * y[i] + C * v[i];
    }
    cross(w, a, wa);
    cross(w, b, wb);
    cross(w, wb, wwb);
#pragma unroll
    for (int i = 0; i < 3; ++i) u[i] = ((wa[i] + wwb[i]) + v[i]) / (double)g.h[i];
}

// one axis of a sample position from the displacement in double: clamped as axis_of clamps, floor taken here and
// kept -- a fraction that rounds to 1 as a float stays in its voxel at f = 1, with that voxel's forward difference
DDRR_HD Axis axis_from(int x, double u, int D, int padding) {
    u = fmin(fmax(u, -(double)(D + 2)), (double)(D + 2));  // (a NaN: below the volume, as in axis_of)
    const double fl = floor(u);
    return ddrr_warp::axis_at(x + (int)fl, (float)(u - fl), D, padding);
}

// out[c] = sum_a gu[a] d u_a / d xi_c, gu the gradient in u (voxels)
DDRR_HD void twist_gradient(const Geometry &geo, const float xi[kTwist], const float y[3], const float gu[3],
                            float out[kTwist]) {
    const float *w = xi, *v = xi + 3;
    const float s = dot(w, w);
    const Coef k = coefficients(s);
    float g[3], a[3], b[3], da[3], db[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        g[i] = gu[i] / geo.h[i];
        a[i] = k.A * y[i] + k.B * v[i];
        b[i] = k.B * y[i] + k.C * v[i];
        da[i] = k.dA * y[i] + k.dB * v[i];
        db[i] = k.dB * y[i] + k.dC * v[i];
    }
    float gw[3], ag[3], wb[3], wbg[3], bgw[3], wda[3], wdb[3], wwdb[3];
    cross(g, w, gw);
    cross(a, g, ag);
    cross(w, b, wb);
    cross(wb, g, wbg);
    cross(b, gw, bgw);
    cross(w, da, wda);
    cross(w, db, wdb);
    cross(w, wdb, wwdb);
    const float wg = dot(w, g);
    float gn = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) gn += g[i] * (wda[i] + wwdb[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        out[i] = (ag[i] + wbg[i]) + bgw[i] + 2.f * w[i] * gn;
        out[3 + i] = g[i] + k.B * gw[i] + k.C * (w[i] * wg - s * g[i]);
    }
}

// ------------------------------------------------------------------------------------------------ sampling
// the sample position's three axes of voxel (x, y, z) from its two lattice lines L0 (node cz), L1 (cz + 1);
// xi and y are left, rounded to float, for the adjoint
DDRR_HD void sample_axes(const Geometry &g, int x, int y, int z, double tz, const double L0[kTwist],
                         const double L1[kTwist], int padding, float xi[kTwist], float pos[3], Axis ax[3]) {
    double xd[kTwist], yd[3], u[3];
#pragma unroll
    for (int c = 0; c < kTwist; ++c) {
        xd[c] = lerp(L0[c], L1[c], tz);
        xi[c] = (float)xd[c];
    }
    centred(g, x, y, z, yd);
    displacement(g, xd, yd, u);
    const int xs[3] = {x, y, z};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        pos[a] = (float)yd[a];
        ax[a] = axis_from(xs[a], u[a], g.s.D[a], padding);
    }
}

// W of one voxel
DDRR_HD float warp_voxel(const float *V, const Geometry &g, int x, int y, int z, double tz, const double L0[kTwist],
                         const double L1[kTwist], int padding) {
    Axis ax[3];
    float xi[kTwist], pos[3];
    sample_axes(g, x, y, z, tz, L0, L1, padding, xi, pos, ax);
    long o[8];
    corner_offsets(g.s.D, ax[0], ax[1], ax[2], o);
    float v[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = V[o[c]];
    return interpolate(v, ax[0], ax[1], ax[2]);
}

// W of the run of (up to) four z voxels from z0 of row (x, y): the forward kernel's thread.  The twist comes from
// two lattice lines kept in registers; the z cell is stepped with frac_in's integer numerator (G - 1 <= D - 1: at
// most one node per step) and one line is re-read when the run crosses a node.  out[k] = 0 beyond the row.
DDRR_HD void forward_run(const float *V, const Geometry &g, const float *Xi, int padding, int x, int y, int z0,
                         float out[4]) {
    const Shape &s = g.s;
    const int cx = cell_of(x, s.D[0], s.G[0]).c, cy = cell_of(y, s.D[1], s.G[1]).c;
    const double tx = frac_of(x, cx, s.D[0], s.G[0]), ty = frac_of(y, cy, s.D[1], s.G[1]);
    double L0[kTwist], L1[kTwist];
    int c = cell_of(z0, s.D[2], s.G[2]).c;
    unsigned r = (unsigned)z0 * (unsigned)(s.G[2] - 1) - (unsigned)c * (unsigned)(s.D[2] - 1);
    twist_line(Xi, s.G, cx, cy, tx, ty, c, L0);
    twist_line(Xi, s.G, cx, cy, tx, ty, c + 1, L1);
    const double den = (double)(s.D[2] - 1);
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = 0.f;
    // (not unrolled: one voxel's double arithmetic at a time keeps the kernel at 4 waves per SIMD without scratch;
    // the result goes to out[k] through selects, so that out stays in registers)
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        const int z = z0 + k;
        if (z < s.D[2]) {
            if (k > 0) {
                r += (unsigned)(s.G[2] - 1);
                if (r >= (unsigned)(s.D[2] - 1) && c < s.G[2] - 2) {  // the run crosses a node
                    r -= (unsigned)(s.D[2] - 1);
                    ++c;
#pragma unroll
                    for (int a = 0; a < kTwist; ++a) L0[a] = L1[a];
                    twist_line(Xi, s.G, cx, cy, tx, ty, c + 1, L1);
                }
            }
            const float w = warp_voxel(V, g, x, y, z, (double)r / den, L0, L1, padding);
#pragma unroll
            for (int e = 0; e < 4; ++e) out[e] = e == k ? w : out[e];
        }
    }
}

// ------------------------------------------------------------------------------------------------ twist gradient
// what voxel (x, y, z) of a cell adds to the cell's 48 sums: acc[6 n + c] += hat_n gW sum_a d_a V(p) d u_a / d xi_c
DDRR_HD void accumulate_voxel(const float *V, const Geometry &g, int x, int y, int z, const float wxy[4], float tz,
                              double tzd, const double L0[kTwist], const double L1[kTwist], int padding, float gw,
                              float acc[kPieceFloats]) {
    Axis ax[3];
    float xi[kTwist], pos[3];
    sample_axes(g, x, y, z, tzd, L0, L1, padding, xi, pos, ax);
    long o[8];
    corner_offsets(g.s.D, ax[0], ax[1], ax[2], o);
    float v[8], gu[3], gxi[kTwist];
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = V[o[c]];
    interpolate_gradient(v, ax[0], ax[1], ax[2], gu);
#pragma unroll
    for (int a = 0; a < 3; ++a) gu[a] *= gw;
    twist_gradient(g, xi, pos, gu, gxi);
    const float wz[2] = {1.f - tz, tz};
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const float hat = wxy[i + 2 * j] * wz[k];
#pragma unroll
                for (int c = 0; c < kTwist; ++c) acc[kTwist * (4 * i + 2 * j + k) + c] += hat * gxi[c];
            }
}

// thread `tid` of piece `piece` of cell (cx, cy, cz): its kPer voxels, in order, into acc (zeroed here)
DDRR_HD void piece_thread(const float *V, const Geometry &g, const float *Xi, int padding, const float *gW, int cx,
                          int cy, int cz, unsigned piece, int tid, float acc[kPieceFloats]) {
#pragma unroll
    for (int e = 0; e < kPieceFloats; ++e) acc[e] = 0.f;
    const Shape &s = g.s;
    const Box box = cell_box(s, cx, cy, cz);
    const unsigned count = (unsigned)box.n[0] * (unsigned)box.n[1] * (unsigned)box.n[2];  // <= 2^31
    for (int k = 0; k < kPer; ++k) {
        const unsigned l = piece * (unsigned)kPieceVoxels + (unsigned)(k * kBlock + tid);
        if (l >= count) break;
        const unsigned row = l / (unsigned)box.n[2];
        const int z = box.b[2] + (int)(l - row * (unsigned)box.n[2]);
        const unsigned lx = row / (unsigned)box.n[1];
        const int y = box.b[1] + (int)(row - lx * (unsigned)box.n[1]);
        const int x = box.b[0] + (int)lx;
        float wxy[4];
        double L0[kTwist], L1[kTwist];
        column_weights(frac_in(x, cx, s.D[0], s.G[0]), frac_in(y, cy, s.D[1], s.G[1]), wxy);
        const double tx = frac_of(x, cx, s.D[0], s.G[0]), ty = frac_of(y, cy, s.D[1], s.G[1]);
        twist_line(Xi, s.G, cx, cy, tx, ty, cz, L0);
        twist_line(Xi, s.G, cx, cy, tx, ty, cz + 1, L1);
        const long at = ((long)x * s.D[1] + y) * s.D[2] + z;
        accumulate_voxel(V, g, x, y, z, wxy, frac_in(z, cz, s.D[2], s.G[2]), frac_of(z, cz, s.D[2], s.G[2]), L0, L1,
                         padding, gW[at], acc);
    }
}

// gXi[c, node (i, j, k)]: the pieces of the node's incident cells, ascending (cell, piece)
DDRR_HD float twist_node_sum(const float *ws, const Shape &s, long pieces, int c, int i, int j, int k) {
    float v = 0.f;
    for (int cx = i - 1; cx <= i; ++cx) {
        if (cx < 0 || cx > s.G[0] - 2) continue;
        for (int cy = j - 1; cy <= j; ++cy) {
            if (cy < 0 || cy > s.G[1] - 2) continue;
            for (int cz = k - 1; cz <= k; ++cz) {
                if (cz < 0 || cz > s.G[2] - 2) continue;
                const long cell = ((long)cx * (s.G[1] - 1) + cy) * (s.G[2] - 1) + cz;
                const int node = 4 * (i - cx) + 2 * (j - cy) + (k - cz);
                const float *p = ws + cell * pieces * kPieceFloats + kTwist * node + c;
                for (long q = 0; q < pieces; ++q) v += p[q * kPieceFloats];
            }
        }
    }
    return v;
}

// ------------------------------------------------------------------------------------------------ volume gradient
// the 8 (offset, weight gW) terms voxel (x, y, z) scatters; a term of weight 0 is skipped by the caller
DDRR_HD void scatter_terms(const Geometry &g, const float *Xi, int padding, int x, int y, int z, float gw, long o[8],
                           float w[8]) {
    const Shape &s = g.s;
    const int cx = cell_of(x, s.D[0], s.G[0]).c, cy = cell_of(y, s.D[1], s.G[1]).c, cz = cell_of(z, s.D[2], s.G[2]).c;
    const double tx = frac_of(x, cx, s.D[0], s.G[0]), ty = frac_of(y, cy, s.D[1], s.G[1]);
    double L0[kTwist], L1[kTwist];
    float xi[kTwist], pos[3];
    twist_line(Xi, s.G, cx, cy, tx, ty, cz, L0);
    twist_line(Xi, s.G, cx, cy, tx, ty, cz + 1, L1);
    Axis ax[3];
    sample_axes(g, x, y, z, frac_of(z, cz, s.D[2], s.G[2]), L0, L1, padding, xi, pos, ax);
    // an axis whose two corners are one voxel (clamped at a face of the volume) scatters their weights as one term:
    // the motions here throw whole regions out of the volume, and with border padding a face voxel would take two,
    // four or eight separately rounded adds from each such sample
#pragma unroll
    for (int a = 0; a < 3; ++a)
        if (ax[a].i0 == ax[a].i1) {
            ax[a].w0 += ax[a].w1;
            ax[a].w1 = 0.f;
        }
    corner_offsets(s.D, ax[0], ax[1], ax[2], o);
    corner_weights(ax[0], ax[1], ax[2], w);
#pragma unroll
    for (int c = 0; c < 8; ++c) w[c] *= gw;
}

}  // namespace ddrr_polyrigid
