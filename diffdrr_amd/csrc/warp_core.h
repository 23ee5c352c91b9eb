// warp_core.h -- the arithmetic of the free-form deformation kernels (warp.hip; include/diffdrr_warp_hip.h
// has the definitions): a voxel's lattice cell and fraction, the field from the cell's 8 nodes, the sample
// position, the 8 corners with their weights and derivatives, and the fixed-order sums of the lattice
// gradient.  Host and device (DDRR_HD): tests/emu/warp_emu.cpp compiles the same functions for the CPU.
#pragma once

#include <math.h>

#include "../../include/diffdrr_warp_hip.h"
#include "ddrr_common.h"

namespace ddrr_warp {

constexpr int kBlock = 256;
constexpr int kPieceVoxels = DDRR_WARP_PIECE_VOXELS;
constexpr int kPer = kPieceVoxels / kBlock;       // voxels of a thread in a piece
constexpr int kPieceFloats = DDRR_WARP_PIECE_FLOATS;  // 8 nodes x 3 components
constexpr int kSlices = 8, kSliceLen = kBlock / kSlices;
constexpr int kRedStride = kBlock + 1;            // a value's row of per-thread sums in LDS, padded
constexpr long kMaxVoxels = 1L << 31;

struct Shape {
    int D[3], G[3];
};

// the domain of every entry (include/diffdrr_warp_hip.h); nullptr, or what is wrong
inline const char *domain_error(const Shape &s, int padding) {
    for (int a = 0; a < 3; ++a) {
        if (s.D[a] < 1 || s.G[a] < 0) return "volume and lattice sizes must be positive";
        if (s.D[a] > DDRR_WARP_MAX_DIM) return "at most 65535 voxels per axis (D_a < 2^16)";
        if (s.G[a] < 2) return "the lattice needs at least 2 nodes per axis (G_a >= 2)";
        if (s.G[a] > s.D[a]) return "the lattice may have at most one node per voxel (G_a <= D_a)";
    }
    if ((long)s.D[0] * s.D[1] * s.D[2] > kMaxVoxels) return "at most 2^31 voxels (larger volumes are out of scope)";
    if (padding != DDRR_WARP_PADDING_ZEROS && padding != DDRR_WARP_PADDING_BORDER)
        return "padding must be DDRR_WARP_PADDING_ZEROS or DDRR_WARP_PADDING_BORDER";
    return nullptr;
}

// ------------------------------------------------------------------------------------------------ lattice
struct Cell {
    int c;
    float t;
};

// fraction of voxel x in cell c: the numerator is an exact integer (x, G <= 65535: below 2^32)
DDRR_HD float frac_in(int x, int c, int D, int G) {
    return (float)((unsigned)x * (unsigned)(G - 1) - (unsigned)c * (unsigned)(D - 1)) / (float)(D - 1);
}

DDRR_HD Cell cell_of(int x, int D, int G) {
    unsigned c = (unsigned)x * (unsigned)(G - 1) / (unsigned)(D - 1);
    if (c > (unsigned)(G - 2)) c = (unsigned)(G - 2);
    Cell r;
    r.c = (int)c;
    r.t = frac_in(x, r.c, D, G);
    return r;
}

// first voxel of cell c; for c == G - 1 the end of the last cell
DDRR_HD int cell_begin(int c, int D, int G) {
    if (c >= G - 1) return D;
    return (int)(((unsigned)c * (unsigned)(D - 1) + (unsigned)(G - 2)) / (unsigned)(G - 1));
}

inline int max_extent(int D, int G) {
    int m = 0;
    for (int c = 0; c < G - 1; ++c) {
        const int n = cell_begin(c + 1, D, G) - cell_begin(c, D, G);
        m = n > m ? n : m;
    }
    return m;
}

// pieces per cell of the lattice gradient (the same for every cell: the largest cell's)
inline long pieces_per_cell(const Shape &s) {
    const long n = (long)max_extent(s.D[0], s.G[0]) * max_extent(s.D[1], s.G[1]) * max_extent(s.D[2], s.G[2]);
    return (n + kPieceVoxels - 1) / kPieceVoxels;
}

inline long cells_of(const Shape &s) { return (long)(s.G[0] - 1) * (s.G[1] - 1) * (s.G[2] - 1); }

// the four (x, y) weights of a cell's columns: (0,0) (1,0) (0,1) (1,1)
DDRR_HD void column_weights(float tx, float ty, float w[4]) {
    w[0] = (1.f - tx) * (1.f - ty);
    w[1] = tx * (1.f - ty);
    w[2] = (1.f - tx) * ty;
    w[3] = tx * ty;
}

DDRR_HD float bilinear(const float w[4], float n00, float n10, float n01, float n11) {
    return w[0] * n00 + w[1] * n10 + w[2] * n01 + w[3] * n11;
}

// the field's three components on the lattice line (cx + tx, cy + ty, node k): 12 lattice reads
DDRR_HD void field_line(const float *disp, const int G[3], int cx, int cy, const float w[4], int k, float B[3]) {
    const long plane = (long)G[1] * G[2], all = plane * G[0];
    const long o = (long)cx * plane + (long)cy * G[2] + k;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float *d = disp + a * all + o;
        B[a] = bilinear(w, d[0], d[plane], d[G[2]], d[plane + G[2]]);
    }
}

DDRR_HD float along_z(float tz, float B0, float B1) { return (1.f - tz) * B0 + tz * B1; }

// ------------------------------------------------------------------------------------------------ sampling
// one axis of a sample position: the two corner indices (clamped into the volume), their weights and the
// weights' derivatives in f (a corner outside the volume: all zero with zeros padding)
struct Axis {
    int i0, i1;
    float w0, w1, d0, d1;
};

// the axis of a sample at voxel i + f, 0 <= f <= 1
DDRR_HD Axis axis_at(int i, float f, int D, int padding) {
    const bool border = padding == DDRR_WARP_PADDING_BORDER;
    const float m0 = (border || (i >= 0 && i < D)) ? 1.f : 0.f;
    const float m1 = (border || (i + 1 >= 0 && i + 1 < D)) ? 1.f : 0.f;
    Axis r;
    r.i0 = i < 0 ? 0 : (i > D - 1 ? D - 1 : i);
    r.i1 = i + 1 < 0 ? 0 : (i + 1 > D - 1 ? D - 1 : i + 1);
    r.w0 = (1.f - f) * m0;
    r.w1 = f * m1;
    r.d0 = -m0;
    r.d1 = m1;
    return r;
}

// p = x + u is never rounded to a float: floor(p) = x + floor(u) and f = u - floor(u) carry the precision of
// u (a few voxels), not of p (up to D), which is what decides on which side of a voxel face a sample falls
DDRR_HD Axis axis_of(int x, float u, int D, int padding) {
    u = fminf(fmaxf(u, -(float)(D + 2)), (float)(D + 2));  // (beyond: outside the volume anyway; a NaN: below it)
    const float fl = floorf(u);
    return axis_at(x + (int)fl, u - fl, D, padding);
}

// the 8 corners' offsets into the volume, [4 i + 2 j + k], in 64 bits; always inside it
DDRR_HD void corner_offsets(const int D[3], const Axis &x, const Axis &y, const Axis &z, long o[8]) {
    const long rx[2] = {(long)x.i0 * D[1], (long)x.i1 * D[1]};
    const int iy[2] = {y.i0, y.i1}, iz[2] = {z.i0, z.i1};
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int k = 0; k < 2; ++k) o[4 * i + 2 * j + k] = (rx[i] + iy[j]) * D[2] + iz[k];
}

DDRR_HD float interpolate(const float v[8], const Axis &x, const Axis &y, const Axis &z) {
    const float c00 = z.w0 * v[0] + z.w1 * v[1], c01 = z.w0 * v[2] + z.w1 * v[3];
    const float c10 = z.w0 * v[4] + z.w1 * v[5], c11 = z.w0 * v[6] + z.w1 * v[7];
    return x.w0 * (y.w0 * c00 + y.w1 * c01) + x.w1 * (y.w0 * c10 + y.w1 * c11);
}

// d W / d p_a, a = 0, 1, 2
DDRR_HD void interpolate_gradient(const float v[8], const Axis &x, const Axis &y, const Axis &z, float g[3]) {
    const float c00 = z.w0 * v[0] + z.w1 * v[1], c01 = z.w0 * v[2] + z.w1 * v[3];
    const float c10 = z.w0 * v[4] + z.w1 * v[5], c11 = z.w0 * v[6] + z.w1 * v[7];
    const float e00 = z.d0 * v[0] + z.d1 * v[1], e01 = z.d0 * v[2] + z.d1 * v[3];
    const float e10 = z.d0 * v[4] + z.d1 * v[5], e11 = z.d0 * v[6] + z.d1 * v[7];
    const float c0 = y.w0 * c00 + y.w1 * c01, c1 = y.w0 * c10 + y.w1 * c11;
    g[0] = x.d0 * c0 + x.d1 * c1;
    g[1] = x.w0 * (y.d0 * c00 + y.d1 * c01) + x.w1 * (y.d0 * c10 + y.d1 * c11);
    g[2] = x.w0 * (y.w0 * e00 + y.w1 * e01) + x.w1 * (y.w0 * e10 + y.w1 * e11);
}

DDRR_HD void corner_weights(const Axis &x, const Axis &y, const Axis &z, float w[8]) {
    const float wx[2] = {x.w0, x.w1}, wy[2] = {y.w0, y.w1}, wz[2] = {z.w0, z.w1};
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int k = 0; k < 2; ++k) w[4 * i + 2 * j + k] = wx[i] * wy[j] * wz[k];
}

// the sample position's three axes of voxel (x, y, z) from its two lattice lines B0 (node cz), B1 (cz + 1)
DDRR_HD void sample_axes(const int D[3], int x, int y, int z, float tz, const float B0[3], const float B1[3],
                         int padding, Axis ax[3]) {
    const int xs[3] = {x, y, z};
#pragma unroll
    for (int a = 0; a < 3; ++a) ax[a] = axis_of(xs[a], along_z(tz, B0[a], B1[a]), D[a], padding);
}

// W of one voxel
DDRR_HD float warp_voxel(const float *V, const int D[3], int x, int y, int z, float tz, const float B0[3],
                         const float B1[3], int padding) {
    Axis ax[3];
    sample_axes(D, x, y, z, tz, B0, B1, padding, ax);
    long o[8];
    corner_offsets(D, ax[0], ax[1], ax[2], o);
    float v[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = V[o[c]];
    return interpolate(v, ax[0], ax[1], ax[2]);
}

// W of the run of (up to) four z voxels from z0 of row (x, y): the forward kernel's thread.  The field comes
// from two lattice lines kept in registers; the z cell is stepped with frac_in's integer numerator (G - 1 <= D - 1:
// at most one node per step) and one line is re-read when the run crosses a node.  out[k] = 0 beyond the row.
DDRR_HD void forward_run(const float *V, const Shape &s, const float *disp, int padding, int x, int y, int z0,
                         float out[4]) {
    const Cell cx = cell_of(x, s.D[0], s.G[0]), cy = cell_of(y, s.D[1], s.G[1]);
    float wxy[4], B0[3], B1[3];
    column_weights(cx.t, cy.t, wxy);
    int c = cell_of(z0, s.D[2], s.G[2]).c;
    unsigned r = (unsigned)z0 * (unsigned)(s.G[2] - 1) - (unsigned)c * (unsigned)(s.D[2] - 1);
    field_line(disp, s.G, cx.c, cy.c, wxy, c, B0);
    field_line(disp, s.G, cx.c, cy.c, wxy, c + 1, B1);
    const float den = (float)(s.D[2] - 1);
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
#pragma unroll
                    for (int a = 0; a < 3; ++a) B0[a] = B1[a];
                    field_line(disp, s.G, cx.c, cy.c, wxy, c + 1, B1);
                }
            }
            out[k] = warp_voxel(V, s.D, x, y, z, (float)r / den, B0, B1, padding);
        }
    }
}

// ------------------------------------------------------------------------------------------------ lattice gradient
// what voxel (x, y, z) of a cell adds to the cell's 24 sums: acc[3 n + a] += hat_n gW d_a V(p)
DDRR_HD void accumulate_voxel(const float *V, const int D[3], int x, int y, int z, const float wxy[4], float tz,
                              const float B0[3], const float B1[3], int padding, float gw, float acc[kPieceFloats]) {
    Axis ax[3];
    sample_axes(D, x, y, z, tz, B0, B1, padding, ax);
    long o[8];
    corner_offsets(D, ax[0], ax[1], ax[2], o);
    float v[8], g[3];
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = V[o[c]];
    interpolate_gradient(v, ax[0], ax[1], ax[2], g);
#pragma unroll
    for (int a = 0; a < 3; ++a) g[a] *= gw;
    const float wz[2] = {1.f - tz, tz};
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const float hat = wxy[i + 2 * j] * wz[k];
#pragma unroll
                for (int a = 0; a < 3; ++a) acc[3 * (4 * i + 2 * j + k) + a] += hat * g[a];
            }
}

// a piece's box: the cell's first voxel and extents
struct Box {
    int b[3], n[3];
};

DDRR_HD Box cell_box(const Shape &s, int cx, int cy, int cz) {
    const int c[3] = {cx, cy, cz};
    Box r;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        r.b[a] = cell_begin(c[a], s.D[a], s.G[a]);
        r.n[a] = cell_begin(c[a] + 1, s.D[a], s.G[a]) - r.b[a];
    }
    return r;
}

// thread `tid` of piece `piece` of cell (cx, cy, cz): its kPer voxels, in order, into acc (zeroed here)
DDRR_HD void piece_thread(const float *V, const Shape &s, const float *disp, int padding, const float *gW,
                          int cx, int cy, int cz, unsigned piece, int tid, float acc[kPieceFloats]) {
#pragma unroll
    for (int e = 0; e < kPieceFloats; ++e) acc[e] = 0.f;
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
        float wxy[4], B0[3], B1[3];
        column_weights(frac_in(x, cx, s.D[0], s.G[0]), frac_in(y, cy, s.D[1], s.G[1]), wxy);
        field_line(disp, s.G, cx, cy, wxy, cz, B0);
        field_line(disp, s.G, cx, cy, wxy, cz + 1, B1);
        const long at = ((long)x * s.D[1] + y) * s.D[2] + z;
        accumulate_voxel(V, s.D, x, y, z, wxy, frac_in(z, cz, s.D[2], s.G[2]), B0, B1, padding, gW[at], acc);
    }
}

// one slice of a value's row of per-thread sums (`row` = kBlock floats), ascending
DDRR_HD float slice_sum(const float *row, int slice) {
    float v = row[slice * kSliceLen];
    for (int i = 1; i < kSliceLen; ++i) v += row[slice * kSliceLen + i];
    return v;
}

// gU[a, node (i, j, k)]: the pieces of the node's incident cells, ascending (cell, piece)
DDRR_HD float node_sum(const float *ws, const Shape &s, long pieces, int a, int i, int j, int k) {
    float v = 0.f;
    for (int cx = i - 1; cx <= i; ++cx) {
        if (cx < 0 || cx > s.G[0] - 2) continue;
        for (int cy = j - 1; cy <= j; ++cy) {
            if (cy < 0 || cy > s.G[1] - 2) continue;
            for (int cz = k - 1; cz <= k; ++cz) {
                if (cz < 0 || cz > s.G[2] - 2) continue;
                const long cell = ((long)cx * (s.G[1] - 1) + cy) * (s.G[2] - 1) + cz;
                const int node = 4 * (i - cx) + 2 * (j - cy) + (k - cz);
                const float *p = ws + cell * pieces * kPieceFloats + 3 * node + a;
                for (long q = 0; q < pieces; ++q) v += p[q * kPieceFloats];
            }
        }
    }
    return v;
}

// ------------------------------------------------------------------------------------------------ volume gradient
// the 8 (offset, weight gW) terms voxel (x, y, z) scatters; a term of weight 0 is skipped by the caller
DDRR_HD void scatter_terms(const Shape &s, const float *disp, int padding, int x, int y, int z, float gw, long o[8],
                           float w[8]) {
    const Cell cx = cell_of(x, s.D[0], s.G[0]), cy = cell_of(y, s.D[1], s.G[1]), cz = cell_of(z, s.D[2], s.G[2]);
    float wxy[4], B0[3], B1[3];
    column_weights(cx.t, cy.t, wxy);
    field_line(disp, s.G, cx.c, cy.c, wxy, cz.c, B0);
    field_line(disp, s.G, cx.c, cy.c, wxy, cz.c + 1, B1);
    Axis ax[3];
    sample_axes(s.D, x, y, z, cz.t, B0, B1, padding, ax);
    corner_offsets(s.D, ax[0], ax[1], ax[2], o);
    corner_weights(ax[0], ax[1], ax[2], w);
#pragma unroll
    for (int c = 0; c < 8; ++c) w[c] *= gw;
}

}  // namespace ddrr_warp
