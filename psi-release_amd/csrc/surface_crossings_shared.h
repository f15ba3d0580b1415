// The per-pair statements of the surface-crossing test, shared by csrc/surface_crossings.hip and by the host
// rehearsal tools/surface_crossings_host_check.hip.  Both are compiled with -ffp-contract=off: every product and every sum below is
// rounded once, in the association written here.
//
// Fifteen fp32 values of the triangles P = (p0, p1, p2) and Q = (q0, q1, q2):
//   nP = (p1 - p0) x (p2 - p0), nQ alike; a cross component is a*b - c*d
//   sP[i] = dot(nQ, p_i - q0), sQ[k] = dot(nP, q_k - p0), dot = (x + y) + z
//   D[i][k] = dot((p_{i+1} - p_i) x (q_{k+1} - q_k), q_k - p_i), indices mod 3
// x - y = -(y - x) is exact, so a cross product with its factors swapped and a difference vector turned round negate exactly, and their
// dot product keeps its bits: with the roles of P and Q swapped, sP and sQ change places and D is transposed, bit for bit.  The decision
// of a pair is therefore a function of the two triangles alone.
// Event: edge i of P pierces Q iff sP[i] and sP[i+1] are strictly of opposite sign (two comparisons, no product) and D[i][0], D[i][1],
// D[i][2] are all > 0 or all < 0; the edges of Q against P alike with sQ and the columns of D.  A zero anywhere is no event.
// The closed-box overlap test (geom_boxes_meet) and the bound on the bodies of a batch (GEOM_MAX_B) are csrc/geom_shared.h.
// Also here, on the host only: the Morton order of a mesh's triangles (sc_morton_order), the one statement behind the chunk order of the
// body handle and of the scene handle (csrc/scene_crossings_shared.h), which tests/scene_crossings_ref.py restates.
#pragma once
#include "geom_shared.h"
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#define SC_FN __host__ __device__ __forceinline__

constexpr int SC_CHUNK = 256;           // faces per chunk: one workgroup's lanes, one staged record per lane
constexpr int SC_MAX_F = 1 << 21;       // F < 2^21
constexpr int SC_SELF = 1, SC_BETWEEN = 2, SC_BRUTE = 4;

SC_FN float sc_dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

SC_FN void sc_sub3(const float a[3], const float b[3], float o[3]) { o[0] = a[0] - b[0], o[1] = a[1] - b[1], o[2] = a[2] - b[2]; }

SC_FN void sc_cross3(const float a[3], const float b[3], float o[3])
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// IEEE-rounded division and square root, on the host and on the device: hipcc compiles both correctly rounded
// (-fhip-fp32-correctly-rounded-divide-sqrt, its default, which the build also states).  Not __fsqrt_rn: without OCML's rounded
// operations that intrinsic is the native, approximate square root of this toolchain, which differs from IEEE in the last bit.
SC_FN float sc_div(float a, float b) { return a / b; }

SC_FN float sc_sqrt(float a) { return sqrtf(a); }

SC_FN bool sc_opposite(float a, float b) { return (a > 0.0f && b < 0.0f) || (a < 0.0f && b > 0.0f); }

SC_FN bool sc_same_sign3(float a, float b, float c) { return (a > 0.0f && b > 0.0f && c > 0.0f) || (a < 0.0f && b < 0.0f && c < 0.0f); }

// the exact box of a face: comparisons only
SC_FN void sc_face_box(const float p[3][3], float lo[3], float hi[3])
{
#pragma unroll
    for (int a = 0; a < 3; a++) {
        lo[a] = fminf(fminf(p[0][a], p[1][a]), p[2][a]);
        hi[a] = fmaxf(fmaxf(p[0][a], p[1][a]), p[2][a]);
    }
}

// two faces of one body share a vertex index
SC_FN bool sc_share_vertex(const int a[3], const int b[3])
{
    return a[0] == b[0] || a[0] == b[1] || a[0] == b[2] || a[1] == b[0] || a[1] == b[1] || a[1] == b[2] || a[2] == b[0] || a[2] == b[1] ||
           a[2] == b[2];
}

// the point where the edge (a, b) with plane values (sa, sb) of opposite sign meets the other triangle's plane
SC_FN void sc_edge_point(const float a[3], const float b[3], float sa, float sb, float x[3])
{
    const float t = sc_div(sa, sa - sb);
#pragma unroll
    for (int c = 0; c < 3; c++) x[c] = a[c] + t * (b[c] - a[c]);
}

// The events of a pair so far, and the points of the first two (named members and selects: the points stay in registers)
struct sc_events { int n; float ax, ay, az, bx, by, bz; };

SC_FN void sc_event(const float a[3], const float b[3], float sa, float sb, sc_events *e)
{
    float x[3];
    sc_edge_point(a, b, sa, sb, x);
    const bool first = e->n == 0, second = e->n == 1;
    e->ax = first ? x[0] : e->ax, e->ay = first ? x[1] : e->ay, e->az = first ? x[2] : e->az;
    e->bx = second ? x[0] : e->bx, e->by = second ? x[1] : e->by, e->bz = second ? x[2] : e->bz;
    e->n++;
}

// The number of piercing edges of the pair (0 to 6); *length: the distance of the two piercing points when there are exactly two, else 0.
SC_FN int sc_pair(const float p[3][3], const float q[3][3], float *length)
{
    float u[3], v[3], nP[3], nQ[3], d[3], sP[3], sQ[3], eP[3][3], eQ[3][3], D[3][3];
    sc_sub3(p[1], p[0], u);
    sc_sub3(p[2], p[0], v);
    sc_cross3(u, v, nP);
    sc_sub3(q[1], q[0], u);
    sc_sub3(q[2], q[0], v);
    sc_cross3(u, v, nQ);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        sc_sub3(p[i], q[0], d);
        sP[i] = sc_dot3(nQ[0], nQ[1], nQ[2], d[0], d[1], d[2]);
        sc_sub3(q[i], p[0], d);
        sQ[i] = sc_dot3(nP[0], nP[1], nP[2], d[0], d[1], d[2]);
        sc_sub3(p[(i + 1) % 3], p[i], eP[i]);
        sc_sub3(q[(i + 1) % 3], q[i], eQ[i]);
    }
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            float c[3];
            sc_cross3(eP[i], eQ[k], c);
            sc_sub3(q[k], p[i], d);
            D[i][k] = sc_dot3(c[0], c[1], c[2], d[0], d[1], d[2]);
        }
    sc_events e = {0, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int n = (i + 1) % 3;
        if (sc_opposite(sP[i], sP[n]) && sc_same_sign3(D[i][0], D[i][1], D[i][2])) sc_event(p[i], p[n], sP[i], sP[n], &e);
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int n = (k + 1) % 3;
        if (sc_opposite(sQ[k], sQ[n]) && sc_same_sign3(D[0][k], D[1][k], D[2][k])) sc_event(q[k], q[n], sQ[k], sQ[n], &e);
    }
    *length = 0.0f;
    if (e.n == 2) {
        const float dx = e.bx - e.ax, dy = e.by - e.ay, dz = e.bz - e.az;
        *length = sc_sqrt((dx * dx + dy * dy) + dz * dz);
    }
    return e.n;
}

// The sort key of a pair ((i, s), (j, t)): ascending keys are ascending (i, s, j, t).  The caller guarantees (B * F)^2 < 2^63.
SC_FN long long sc_key(int i, int s, int j, int t, int B, int F) { return (((long long)i * F + s) * B + j) * F + t; }

SC_FN void sc_unkey(long long key, int B, int F, int out[4])
{
    out[3] = (int)(key % F);
    key /= F;
    out[2] = (int)(key % B);
    key /= B;
    out[1] = (int)(key % F);
    out[0] = (int)(key / F);
}

// Morton code of a point quantised to 10 bits per axis
SC_FN uint32_t sc_spread10(uint32_t x)
{
    x &= 0x3ffu;
    x = (x | (x << 16)) & 0x030000ffu;
    x = (x | (x << 8)) & 0x0300f00fu;
    x = (x | (x << 4)) & 0x030c30c3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

// The Morton order of nf < 2^31 triangles f [nf,3] over the vertices v: order[k] = the triangle at position k.  The centroid sums
// ((v0 + v1) + v2 per axis) in fp64, quantised to 10 bits per axis of their own bounding box (0 on an axis without extent), bits
// interleaved x lowest, a stable sort: ties keep triangle order.  Plain C++, no HIP call; the body handle's face order
// (psi_surface_crossings_face_order) and the scene handle's (scn_build).  false, with order untouched, when a sum is not finite.
static inline bool sc_morton_order(const float *v, const int32_t *f, long long nf, int32_t *order)
{
    const size_t n = (size_t)nf;
    std::vector<double> c(n * 3);
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (size_t t = 0; t < n; t++)
        for (int a = 0; a < 3; a++) {
            double s = 0.0;
            for (int k = 0; k < 3; k++) s += (double)v[(size_t)f[t * 3 + k] * 3 + a];
            if (!std::isfinite(s)) return false;
            c[t * 3 + a] = s;
            lo[a] = std::min(lo[a], s);
            hi[a] = std::max(hi[a], s);
        }
    std::vector<uint32_t> code(n);
    for (size_t t = 0; t < n; t++) {
        uint32_t m = 0;
        for (int a = 0; a < 3; a++) {
            const double w = hi[a] - lo[a];
            const uint32_t q = w > 0.0 ? (uint32_t)std::min(1023.0, (c[t * 3 + a] - lo[a]) / w * 1024.0) : 0u;
            m |= sc_spread10(q) << a;
        }
        code[t] = m;
    }
    std::iota(order, order + n, 0);
    std::stable_sort(order, order + n, [&](int32_t a, int32_t b) { return code[a] < code[b]; });
    return true;
}
