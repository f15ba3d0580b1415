// What csrc/mesh_cloud.hip and tools/mesh_cloud_host_check.hip share: the statements of the surface cloud's rule.
// Every function switches contraction off for itself, so the kernels and the host program evaluate the same fp32 operations whatever their
// file is compiled with; division and square root are the correctly rounded ones (hipcc's default).  tests/mesh_cloud_ref.py restates
// these statements in NumPy fp32, operation for operation.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define MC_FN __host__ __device__ __forceinline__

namespace psi_mcloud {

constexpr float MAX_SEGMENTS = 8388608.0f;      // 2^23: a longest edge of more segments than this is refused (it implies more than 2^21 cells)
constexpr int MAX_CELLS = 1 << 21;              // cells along an axis: three of them make a 63-bit linear index
constexpr long long MAX_CANDIDATES = 2147483647ll;

enum Flag : unsigned { BAD_INDEX = 1u, NOT_FINITE = 2u, TOO_LONG = 4u };

enum Kind : int { EMPTY = 0, CORNERS = 1, ROWS = 2 };

struct Tri {
    float a[3], b[3], c[3];     // ROWS: rotated so that ab is the longest edge; CORNERS: the caller's order
    float L;                    // |ab|
    int kind;
    int m;                      // ROWS: rows 0 .. m-1 of segments, row m is the point c
};

MC_FN uint32_t float_bits(float f)
{
    union { float f; uint32_t u; } b;
    b.f = f;
    return b.u;
}

MC_FN float bits_float(uint32_t u)
{
    union { float f; uint32_t u; } b;
    b.u = u;
    return b.f;
}

MC_FN float sq3(float x, float y, float z)
{
#pragma clang fp contract(off)
    return (x * x + y * y) + z * z;
}

// h = spacing / 2
MC_FN float half_spacing(float spacing)
{
    return spacing * 0.5f;
}

// The triangle of corners p0, p1, p2 (the caller's order): its kind, its rotation and its row count.  `too_long` is set when the longest
// edge has more than 2^23 segments of h (no count is taken then: kind = EMPTY).
MC_FN Tri tri_setup(const float *p0, const float *p1, const float *p2, float h, bool *too_long)
{
#pragma clang fp contract(off)
    Tri t;
    const float e01 = sq3(p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]);
    const float e12 = sq3(p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]);
    const float e20 = sq3(p0[0] - p2[0], p0[1] - p2[1], p0[2] - p2[2]);
    const bool bc = e12 > e01;                            // a tie keeps the first of ab, bc, ca
    const float e_ab_bc = bc ? e12 : e01;
    const bool ca = e20 > e_ab_bc;
    const float e = ca ? e20 : e_ab_bc;
    float a[3], b[3], c[3];                               // selected by value, so that the corners stay in registers
    _Pragma("unroll") for (int k = 0; k < 3; k++) {
        a[k] = ca ? p2[k] : (bc ? p1[k] : p0[k]);
        b[k] = ca ? p0[k] : (bc ? p2[k] : p1[k]);
        c[k] = ca ? p1[k] : (bc ? p0[k] : p2[k]);
        t.a[k] = a[k];
        t.b[k] = b[k];
        t.c[k] = c[k];
    }
    t.L = sqrtf(e);
    t.kind = EMPTY;
    t.m = 0;
    *too_long = false;
    const float ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
    const float vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
    const float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    const float area2 = sqrtf(sq3(nx, ny, nz));
    if (!(area2 > 0.0f) || !(t.L > 0.0f)) return t;        // zero area: no candidate
    if (t.L < h) {                                        // smaller than h: its three corners, in the caller's order
        _Pragma("unroll") for (int k = 0; k < 3; k++) { t.a[k] = p0[k]; t.b[k] = p1[k]; t.c[k] = p2[k]; }
        t.kind = CORNERS;
        return t;
    }
    if (!(t.L / h <= MAX_SEGMENTS)) { *too_long = true; return t; }
    const float Ht = area2 / t.L;
    const int m = (int)ceilf(Ht / h);                     // Ht <= L, so the quotient is at most 2^23
    t.m = m > 1 ? m : 1;
    t.kind = ROWS;
    return t;
}

MC_FN int rows_of(const Tri &t)
{
    return t.kind == ROWS ? t.m + 1 : (t.kind == CORNERS ? 1 : 0);
}

// s = r / m of row r < m
MC_FN float row_s(const Tri &t, int r)
{
    return (float)r / (float)t.m;
}

// segments of row r < m: k = max(1, ceil(((1 - s) L) / h))
MC_FN int row_segments(const Tri &t, int r, float h)
{
#pragma clang fp contract(off)
    const float s = row_s(t, r);
    const int k = (int)ceilf(((1.0f - s) * t.L) / h);
    return k > 1 ? k : 1;
}

// candidates of row r of the triangle: k + 1, the single point c for row m, the three corners for a CORNERS triangle's only row
MC_FN int row_candidates(const Tri &t, int r, float h)
{
    if (t.kind == CORNERS) return 3;
    return r >= t.m ? 1 : row_segments(t, r, h) + 1;
}

// candidate j of row r
MC_FN void row_point(const Tri &t, int r, int j, float h, float p[3])
{
#pragma clang fp contract(off)
    if (t.kind == CORNERS) {        // corner j, picked with bit masks: the compiler turns selects into a table in scratch memory or LDS
        const uint32_t ma = j == 0 ? ~0u : 0u, mb = j == 1 ? ~0u : 0u, mc = ~(ma | mb);
        _Pragma("unroll") for (int k = 0; k < 3; k++) p[k] = bits_float((float_bits(t.a[k]) & ma) | (float_bits(t.b[k]) & mb) | (float_bits(t.c[k]) & mc));
        return;
    }
    if (r >= t.m) {
        _Pragma("unroll") for (int k = 0; k < 3; k++) p[k] = t.c[k];
        return;
    }
    const float s = row_s(t, r);
    const float u = (float)j / (float)row_segments(t, r, h);
    _Pragma("unroll") for (int k = 0; k < 3; k++) {
        const float P = t.a[k] + s * (t.c[k] - t.a[k]);
        const float Q = t.b[k] + s * (t.c[k] - t.b[k]);
        p[k] = P + u * (Q - P);
    }
}

// o = min - v / 2 of an axis
MC_FN float cell_origin(float vmin, float h)
{
    return vmin - h;
}

// cell = floor((p - o) / v) of an axis, kept within [0, 2^21) (a guard for the packing of the index: the candidates lie within the box of
// the vertices up to a rounding, and a box of more cells is refused)
MC_FN int cell_of(float p, float o, float v)
{
#pragma clang fp contract(off)
    const float c = floorf((p - o) / v);
    return c >= (float)(MAX_CELLS - 1) ? MAX_CELLS - 1 : (c > 0.0f ? (int)c : 0);
}

MC_FN float cell_centre(int cell, float o, float v)
{
#pragma clang fp contract(off)
    return o + ((float)cell + 0.5f) * v;
}

// The 63-bit linear cell index of p and the bits of its squared distance to the cell centre (not negative, so the bits order like the value)
MC_FN void cell_key(const float p[3], const float o[3], float v, int64_t *cell, uint32_t *key)
{
#pragma clang fp contract(off)
    float d[3];
    int64_t lin = 0;
    _Pragma("unroll") for (int k = 0; k < 3; k++) {
        const int c = cell_of(p[k], o[k], v);
        d[k] = p[k] - cell_centre(c, o[k], v);
        lin = (lin << 21) | (int64_t)c;
    }
    *cell = lin;
    *key = float_bits(sq3(d[0], d[1], d[2]));
}

// cells along an axis whose vertices span vmin .. vmax (as a float: the caller compares it with MAX_CELLS)
MC_FN float cells_along(float vmin, float vmax, float h, float v)
{
#pragma clang fp contract(off)
    return floorf((vmax - cell_origin(vmin, h)) / v) + 1.0f;
}

}   // namespace psi_mcloud
