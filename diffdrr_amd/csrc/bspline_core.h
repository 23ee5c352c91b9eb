// bspline_core.h -- the arithmetic of the cubic B-spline free-form deformation kernels (bspline.hip;
// include/diffdrr_bspline_hip.h has the definitions): the four weights of a fraction, a voxel's taps, the
// (x, y) sum of the lattice that makes a row's z line, the field from four entries of that line, and the
// fixed-order chains of the lattice gradient.  The field is formed in double: its 64 products of coefficients
// of tens of voxels would, summed in float, leave u an ulp or two of |u| uncertain (1e-6 voxel), and floor(u)
// decides on which side of a voxel face a sample falls -- where the coefficient gradient jumps.  floor and
// fraction are taken from the double and only the fraction is rounded to float.  Everything after that (the
// interpolation, every sum of the gradients) is float, but for the accumulators of the second and third gathers
// (gather_axis).  The lattice geometry and everything about sampling (Axis,
// axis_of, the corners) are warp_core.h's.  Host and device (DDRR_HD): tests/emu/bspline_emu.cpp compiles the
// same functions for the CPU.
#pragma once

#include <math.h>

#include "../../include/diffdrr_bspline_hip.h"
#include "warp_core.h"

namespace ddrr_bspline {

using ddrr_warp::Axis;
using ddrr_warp::axis_of;
using ddrr_warp::Cell;
using ddrr_warp::cell_begin;
using ddrr_warp::cell_of;
using ddrr_warp::corner_offsets;
using ddrr_warp::corner_weights;
using ddrr_warp::frac_in;
using ddrr_warp::interpolate;
using ddrr_warp::interpolate_gradient;

constexpr int kBlock = 256;
constexpr int kRows = DDRR_BSPLINE_ROWS;        // volume rows (x, y .. y + 3) of a workgroup: one wave each
constexpr int kLanes = kBlock / kRows;
constexpr int kChunk = DDRR_BSPLINE_CHUNK_VOXELS;  // z voxels of a row a workgroup holds the line for
constexpr int kLineNodes = kChunk + 4;          // nodes c_lo - 1 .. c_hi + 2 of a chunk (c_hi - c_lo <= kChunk - 1)
constexpr int kLineValues = 3 * kLineNodes;     // a row's line in LDS (doubles): [component][node - lo]
constexpr int kPadded = kChunk + kChunk / 32;   // a chunk's per-voxel values in LDS, one pad per 32
constexpr int kSlots = kLanes / 4;              // node tasks of a wave: lane = 4 slot + component
constexpr long kMaxVoxels = 1L << 31;
static_assert(kLanes == 64 && kChunk == 4 * kLanes, "a wave per row, four voxels per lane");

struct Shape {
    int D[3], G[3];
};

// where voxel i of a chunk sits in a padded LDS array: nodes' voxel ranges start a node spacing apart (16, 32:
// one bank), the pad spreads them over the banks
DDRR_HD int padded(int i) { return i + (i >> 5); }

// the domain of every entry (include/diffdrr_bspline_hip.h); nullptr, or what is wrong
inline const char *domain_error(const Shape &s, int padding) {
    for (int a = 0; a < 3; ++a) {
        if (s.D[a] < 1 || s.G[a] < 0) return "volume and lattice sizes must be positive";
        if (s.D[a] > DDRR_BSPLINE_MAX_DIM) return "at most 65535 voxels per axis (D_a < 2^16)";
        if (s.G[a] < 2) return "the lattice needs at least 2 nodes per axis (G_a >= 2)";
        if (s.G[a] > s.D[a]) return "the lattice may have at most one node per voxel (G_a <= D_a)";
    }
    if ((long)s.D[0] * s.D[1] * s.D[2] > kMaxVoxels) return "at most 2^31 voxels (larger volumes are out of scope)";
    if (padding != DDRR_BSPLINE_PADDING_ZEROS && padding != DDRR_BSPLINE_PADDING_BORDER)
        return "padding must be DDRR_BSPLINE_PADDING_ZEROS or DDRR_BSPLINE_PADDING_BORDER";
    return nullptr;
}

// floats of the two intermediate sums of the lattice gradient
inline long r1_floats(const Shape &s) { return 3L * s.D[0] * s.D[1] * s.G[2]; }
inline long r2_floats(const Shape &s) { return 3L * s.D[0] * s.G[1] * s.G[2]; }

// ------------------------------------------------------------------------------------------------ the basis
template <typename T>
DDRR_HD void weights(T t, T B[4]) {
    const T s = T(1) - t, t2 = t * t, sixth = T(1) / T(6);
    B[0] = s * s * s * sixth;
    B[1] = ((T(3) * t - T(6)) * t2 + T(4)) * sixth;
    B[2] = (((T(-3) * t + T(3)) * t + T(3)) * t + T(1)) * sixth;
    B[3] = t2 * t * sixth;
}

// frac_in in double: the same exact integer numerator, one division
DDRR_HD double frac_of(int x, int c, int D, int G) {
    return (double)((unsigned)x * (unsigned)(G - 1) - (unsigned)c * (unsigned)(D - 1)) / (double)(D - 1);
}

// the weights per NODE of a voxel of cell c: a clamped tap's weight joins the border node's own tap
DDRR_HD void fold(int c, int G, float w[4]) {
    if (c == 0) {
        w[1] += w[0];
        w[0] = 0.f;
    }
    if (c == G - 2) {
        w[2] += w[3];
        w[3] = 0.f;
    }
}

DDRR_HD int clamp_node(int n, int G) { return n < 0 ? 0 : (n > G - 1 ? G - 1 : n); }

// the four taps of voxel x of an axis: nodes (clamped) and weights
struct Taps {
    int n[4];
    double w[4];
};

DDRR_HD Taps taps_of(int x, int D, int G) {
    const int c = cell_of(x, D, G).c;
    Taps r;
    weights(frac_of(x, c, D, G), r.w);
#pragma unroll
    for (int k = 0; k < 4; ++k) r.n[k] = clamp_node(c - 1 + k, G);
    return r;
}

// the folded weights of voxel x of an axis (the lattice gradient's)
DDRR_HD void node_weights(int x, int D, int G, float w[4]) {
    const Cell c = cell_of(x, D, G);
    weights(c.t, w);
    fold(c.c, G, w);
}

// component a of the row's line at z node k (0 <= k < Gz): the 16-term (x, y) sum, x taps outer
DDRR_HD double line_value(const float *disp, const int G[3], const Taps &tx, const Taps &ty, int a, int k) {
    const long plane = (long)G[1] * G[2], all = plane * G[0];
    const float *d = disp + a * all + k;
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += (tx.w[i] * ty.w[j]) * d[tx.n[i] * plane + (long)ty.n[j] * G[2]];
    return acc;
}

// the z nodes (not clamped) the voxels [zlo, zend) of a row reach: entry j of the row's line is node lo + j
struct Span {
    int lo, hi;
};

DDRR_HD Span chunk_span(int zlo, int zend, int D, int G) {
    Span r;
    r.lo = cell_of(zlo, D, G).c - 1;
    r.hi = cell_of(zend - 1, D, G).c + 2;
    return r;
}

// u of a voxel of z cell c from the row's line L ([component][node - lo], kLineNodes apart)
DDRR_HD void field_of(const double *L, int lo, int c, const double w[4], double u[3]) {
    const double *p = L + (c - 1 - lo);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        u[a] = ((w[0] * p[0] + w[1] * p[1]) + w[2] * p[2]) + w[3] * p[3];
        p += kLineNodes;
    }
}

// one axis of a sample position from the field in double: clamped as axis_of clamps, floor taken here, the
// fraction in [0, 1) handed to axis_of as a float (a fraction that rounds to 1 becomes the next voxel at 0)
DDRR_HD Axis axis_from(int x, double u, int D, int padding) {
    u = fmin(fmax(u, -(double)(D + 2)), (double)(D + 2));  // (a NaN: below the volume, as in axis_of)
    const double fl = floor(u);
    return axis_of(x + (int)fl, (float)(u - fl), D, padding);
}

// the sample position's three axes of voxel (x, y, z), z in cell c at fraction t
DDRR_HD void sample_axes(const Shape &s, const double *L, int lo, int x, int y, int z, int c, double t, int padding,
                         Axis ax[3]) {
    double w[4], u[3];
    weights(t, w);
    field_of(L, lo, c, w, u);
    const int xs[3] = {x, y, z};
#pragma unroll
    for (int a = 0; a < 3; ++a) ax[a] = axis_from(xs[a], u[a], s.D[a], padding);
}

// ------------------------------------------------------------------------------------------------ forward
// W of the run of (up to) four z voxels from z0 of row (x, y): the forward kernel's thread.  The z cell is
// stepped with frac_in's integer numerator (at most one node per step).  out[k] = 0 beyond the row.
DDRR_HD void forward_run(const float *V, const Shape &s, int padding, const double *L, int lo, int x, int y, int z0,
                         float out[4]) {
    int c = cell_of(z0, s.D[2], s.G[2]).c;
    unsigned r = (unsigned)z0 * (unsigned)(s.G[2] - 1) - (unsigned)c * (unsigned)(s.D[2] - 1);
    const double den = (double)(s.D[2] - 1);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int z = z0 + k;
        out[k] = 0.f;
        if (z < s.D[2]) {
            if (k > 0) {
                r += (unsigned)(s.G[2] - 1);
                if (r >= (unsigned)(s.D[2] - 1) && c < s.G[2] - 2) {  // the run crosses a node
                    r -= (unsigned)(s.D[2] - 1);
                    ++c;
                }
            }
            Axis ax[3];
            sample_axes(s, L, lo, x, y, z, c, (double)r / den, padding, ax);
            long o[8];
            corner_offsets(s.D, ax[0], ax[1], ax[2], o);
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = V[o[e]];
            out[k] = interpolate(v, ax[0], ax[1], ax[2]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ lattice gradient
// q_a = gW d_a V(p) of voxel (x, y, z)
DDRR_HD void voxel_q(const float *V, const Shape &s, int padding, const double *L, int lo, int x, int y, int z,
                     float gw, float q[3]) {
    const int cz = cell_of(z, s.D[2], s.G[2]).c;
    Axis ax[3];
    sample_axes(s, L, lo, x, y, z, cz, frac_of(z, cz, s.D[2], s.G[2]), padding, ax);
    long o[8];
    corner_offsets(s.D, ax[0], ax[1], ax[2], o);
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = V[o[e]];
    interpolate_gradient(v, ax[0], ax[1], ax[2], q);
#pragma unroll
    for (int a = 0; a < 3; ++a) q[a] *= gw;
}

// the chain of z node n over the voxels [zlo, zend) of a row, continued from acc: q and the folded weights
// wz[tap][.] are the chunk's padded arrays (voxel zlo at 0)
DDRR_HD float node_chain(const float *q, const float *wz, int D, int G, int n, int zlo, int zend, float acc) {
    const int c0 = n - 2 < 0 ? 0 : n - 2, c1 = n + 1 > G - 2 ? G - 2 : n + 1;
    for (int c = c0; c <= c1; ++c) {
        const float *w = wz + (n + 1 - c) * kPadded;
        int b = cell_begin(c, D, G), e = cell_begin(c + 1, D, G);
        b = b < zlo ? zlo : b;
        e = e > zend ? zend : e;
        for (int z = b; z < e; ++z) acc += w[padded(z - zlo)] * q[padded(z - zlo)];
    }
    return acc;
}

// the chain of node m of an axis of D voxels and G nodes over src[x * stride], x ascending (the second and
// third gathers).  The sum is kept in double and rounded once: on an axis of 65535 voxels and few nodes a node's
// chain has tens of thousands of terms, and a float accumulator loses 6e-6 of the gradient's scale there.  The
// order stays fixed; the two gather launches are a few thousand outputs each.
DDRR_HD float gather_axis(const float *src, long stride, int D, int G, int m) {
    const int c0 = m - 2 < 0 ? 0 : m - 2, c1 = m + 1 > G - 2 ? G - 2 : m + 1;
    double acc = 0.0;
    for (int c = c0; c <= c1; ++c) {
        const int k = m + 1 - c, e = cell_begin(c + 1, D, G);
        for (int x = cell_begin(c, D, G); x < e; ++x) {
            float w[4];
            weights(frac_in(x, c, D, G), w);
            fold(c, G, w);
            acc += (double)w[k] * (double)src[x * stride];
        }
    }
    return (float)acc;
}

// ------------------------------------------------------------------------------------------------ volume gradient
// the 8 (offset, weight gW) terms voxel (x, y, z) scatters; a term of weight 0 is skipped by the caller
DDRR_HD void scatter_terms(const Shape &s, int padding, const double *L, int lo, int x, int y, int z, float gw,
                           long o[8], float w[8]) {
    const int cz = cell_of(z, s.D[2], s.G[2]).c;
    Axis ax[3];
    sample_axes(s, L, lo, x, y, z, cz, frac_of(z, cz, s.D[2], s.G[2]), padding, ax);
    corner_offsets(s.D, ax[0], ax[1], ax[2], o);
    corner_weights(ax[0], ax[1], ax[2], w);
#pragma unroll
    for (int c = 0; c < 8; ++c) w[c] *= gw;
}

}  // namespace ddrr_bspline
