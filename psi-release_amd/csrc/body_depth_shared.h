// The per-triple statements of the penetration depth of one body in another, shared by csrc/body_depth.hip and by
// the host rehearsal tools/body_depth_host_check.hip.  A triple (i, j, v) asks how far vertex v of body i is from the surface of body j:
// the nearest of the F current triangles of j by the seven-region closest point of csrc/closest_point_shared.h.  No contraction; the
// division and the square root are IEEE-rounded on the device as on the host, so a NumPy fp32 restatement gives the same bits.
#pragma once
#include "body_overlap_shared.h"
#include <stdint.h>
#include <string.h>

#pragma clang fp contract(off)

#include "closest_point_shared.h"

// IEEE-rounded on the host and on the device: hipcc compiles sqrtf correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt, which the
// build states).  Not __fsqrt_rn, which is this toolchain's native square root and differs from IEEE in the last bit
// (csrc/surface_crossings_shared.h has the same note).
#define BD_SQRT(a) sqrtf(a)

constexpr int BD_CHUNK = BO_CHUNK;      // triples of ONE pair per workgroup, and faces staged per round: the chunk table is body_overlap's
constexpr int BD_SLICE = BO_SLICE;      // consecutive faces one workgroup of the nearest pass visits
constexpr int BD_DEPTH = 0, BD_SQUARED = 1;     // the penalty of the loss: sum of depths (L1) or of squared depths

struct BdRecord { float a[3], ab[3], ac[3]; };  // a = X[f0], ab = X[f1] - a, ac = X[f2] - a, each rounded once

struct BdRow {                                  // what a triple reports of its winner
    int face, region;
    float depth, r[3], bary[3];
};

GEOM_FN unsigned int bd_bits(float x)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __float_as_uint(x);
#else
    unsigned int u;
    memcpy(&u, &x, 4);
    return u;
#endif
}

GEOM_FN BdRecord bd_record(const float *__restrict__ vj, const int32_t *__restrict__ f)
{
    const float *a = vj + (size_t)f[0] * 3, *b = vj + (size_t)f[1] * 3, *c = vj + (size_t)f[2] * 3;
    BdRecord r;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        r.a[k] = a[k];
        r.ab[k] = b[k] - a[k];
        r.ac[k] = c[k] - a[k];
    }
    return r;
}

// key = bits(d2) << 32 | face: the smallest, compared as unsigned, wins.  d2 is a sum of squares, so its sign bit is clear unless it is
// a NaN; infinities and NaNs of either sign have larger bits than every finite d2 and lose to it.
GEOM_FN unsigned long long bd_key(float d2, int face) { return ((unsigned long long)bd_bits(d2) << 32) | (unsigned int)face; }

GEOM_FN float bd_d2(float rx, float ry, float rz) { return (rx * rx + ry * ry) + rz * rz; }

// the key of face t (record rec) for the point p
GEOM_FN unsigned long long bd_test(float ax, float ay, float az, float abx, float aby, float abz, float acx, float acy, float acz, float px,
                                   float py, float pz, int t)
{
    float rx, ry, rz;
    closest_point(abx, aby, abz, acx, acy, acz, px - ax, py - ay, pz - az, rx, ry, rz);
    return bd_key(bd_d2(rx, ry, rz), t);
}

GEOM_FN int bd_slices(int F) { return bo_slices(F); }

// The winner's statement once more, on the same inputs and hence with the same bits, with the barycentric coordinates of c:
//   region 4 (1,0,0)  5 (0,1,0)  6 (0,0,1)  1 (1-v, v, 0)  3 (1-w, 0, w)  2 (0, 1-w, w)  0 ((1-v)-w, v, w)
GEOM_FN BdRow bd_row(const BdRecord &rec, float px, float py, float pz, int face)
{
    BdRow o;
    float v, w;
    o.face = face;
    o.region = closest_point_vw(rec.ab[0], rec.ab[1], rec.ab[2], rec.ac[0], rec.ac[1], rec.ac[2], px - rec.a[0], py - rec.a[1], pz - rec.a[2],
                                o.r[0], o.r[1], o.r[2], v, w);
    o.depth = BD_SQRT(bd_d2(o.r[0], o.r[1], o.r[2]));
    switch (o.region) {
    case 4: o.bary[0] = 1.0f; o.bary[1] = 0.0f; o.bary[2] = 0.0f; break;
    case 5: o.bary[0] = 0.0f; o.bary[1] = 1.0f; o.bary[2] = 0.0f; break;
    case 6: o.bary[0] = 0.0f; o.bary[1] = 0.0f; o.bary[2] = 1.0f; break;
    case 1: o.bary[0] = 1.0f - v; o.bary[1] = v; o.bary[2] = 0.0f; break;
    case 3: o.bary[0] = 1.0f - w; o.bary[1] = 0.0f; o.bary[2] = w; break;
    case 2: o.bary[0] = 0.0f; o.bary[1] = 1.0f - w; o.bary[2] = w; break;
    default: o.bary[0] = (1.0f - v) - w; o.bary[1] = v; o.bary[2] = w; break;
    }
    return o;
}

// The four gradient rows of a triple for the upstream g of body i: u = (g * s) * r with s = 1 / depth (0 at depth 0) for the depth
// penalty and s = 2 for the squared one; row 0 is +u at the vertex, rows 1..3 are -(bary[m] * u) at the winner's corners.
GEOM_FN void bd_grad_rows(float g, int penalty, float depth, const float r[3], const float bary[3], float rows[4][3])
{
    const float s = penalty == BD_SQUARED ? 2.0f : (depth > 0.0f ? MS_DIV(1.0f, depth) : 0.0f);
    const float gs = g * s;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float u = gs * r[a];
        rows[0][a] = u;
#pragma unroll
        for (int m = 0; m < 3; m++) rows[1 + m][a] = -(bary[m] * u);
    }
}
