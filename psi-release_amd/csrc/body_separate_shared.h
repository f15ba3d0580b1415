// The statements of the rigid separation of overlapping bodies, shared by csrc/body_separate.hip and by the host
// rehearsal tools/body_separate_host_check.hip: the pose of a vertex under a body's rigid state, the six wrench terms of a vertex, the Adam
// step of one component and the Cayley update of the quaternion.  No contraction; division and square root are IEEE-rounded on the device
// as on the host, and the only operations are + - * / sqrt and comparisons, so the fp32 NumPy restatement (tests/body_separate_ref.py)
// mirrors this file line for line and gives the same bits.
//
//   state    quat (w, x, y, z), transl, pivot, Adam moments m, s [6] per body, all fp32
//   pose     d = base - pivot, p = pivot + transl, x_k = ((R_k0 d0 + R_k1 d1) + R_k2 d2) + p_k; the identity state returns base itself
//   wrench   a = x - p, c = a x G (a component is a*b - c*d); (G, c) are widened to fp64 by the caller and added in a fixed order
//   step     m = b1 m + (1 - b1) g, s = b2 s + ((1 - b2) g) g, u = (m / c1) / (sqrt(s / c2) + eps); transl -= lr_t u[0:3];
//            delta = -(lr_r u[3:6]); quat <- normalise((1, delta / 2) (x) quat) unless delta is exactly zero
//   scene    a node-centred volume sdf [D][D][D] over the box gmin .. gmax: k = fp32((D - 1) / (gmax - gmin)) formed in fp64, o = gmin;
//            u = (x - o) k, clamp to [0, D - 1], cell and fraction, in = 0 < u < D - 1; the eight corners interpolated along z, y, x with
//            lerp(a, b, w) = a + w (b - a); the grid-unit gradient from the same differences, times k under the mask; a vertex with
//            value < 0 is in the scene: G = (-w_scene) g, loss -value; every other vertex gives exact zeros
#pragma once
#include "geom_shared.h"
#include <stdint.h>

#pragma clang fp contract(off)

constexpr int BS_CHUNK = 256;           // vertices per chunk of the wrench sum, and the lanes of its tree

struct bs3 { float x, y, z; };
struct BsQuat { float w, x, y, z; };
struct BsRot { float r00, r01, r02, r10, r11, r12, r20, r21, r22; };

GEOM_FN bs3 bs_make(float x, float y, float z) { bs3 o; o.x = x, o.y = y, o.z = z; return o; }

// The nine entries of R, with their association
GEOM_FN BsRot bs_rotation(BsQuat q)
{
    BsRot R;
    const float w = q.w, x = q.x, y = q.y, z = q.z;
    R.r00 = 1.0f - 2.0f * (y * y + z * z);
    R.r01 = 2.0f * (x * y - w * z);
    R.r02 = 2.0f * (x * z + w * y);
    R.r10 = 2.0f * (x * y + w * z);
    R.r11 = 1.0f - 2.0f * (x * x + z * z);
    R.r12 = 2.0f * (y * z - w * x);
    R.r20 = 2.0f * (x * z - w * y);
    R.r21 = 2.0f * (y * z + w * x);
    R.r22 = 1.0f - 2.0f * (x * x + y * y);
    return R;
}

// quat == (1, 0, 0, 0) and transl == 0 exactly: such a body is not touched by a rounding
GEOM_FN bool bs_is_identity(BsQuat q, bs3 t)
{
    return q.w == 1.0f && q.x == 0.0f && q.y == 0.0f && q.z == 0.0f && t.x == 0.0f && t.y == 0.0f && t.z == 0.0f;
}

// p = pivot + transl: the point the body turns about, in the world
GEOM_FN bs3 bs_centre(bs3 pivot, bs3 transl) { return bs_make(pivot.x + transl.x, pivot.y + transl.y, pivot.z + transl.z); }

GEOM_FN bs3 bs_pose(bs3 base, BsRot R, bs3 pivot, bs3 p, bool identity)
{
    if (identity) return base;
    const float d0 = base.x - pivot.x, d1 = base.y - pivot.y, d2 = base.z - pivot.z;
    return bs_make(((R.r00 * d0 + R.r01 * d1) + R.r02 * d2) + p.x, ((R.r10 * d0 + R.r11 * d1) + R.r12 * d2) + p.y,
                   ((R.r20 * d0 + R.r21 * d1) + R.r22 * d2) + p.z);
}

// c = (x - p) x G
GEOM_FN bs3 bs_torque(bs3 x, bs3 p, bs3 G)
{
    const float a0 = x.x - p.x, a1 = x.y - p.y, a2 = x.z - p.z;
    return bs_make(a1 * G.z - a2 * G.y, a2 * G.x - a0 * G.z, a0 * G.y - a1 * G.x);
}

// The constants of a step: b1, b2, eps, lr_t, lr_r rounded to fp32 by the caller; c1 = fp32(1 - b1^k), c2 = fp32(1 - b2^k) from fp64
struct BsStep { float b1, b2, c1, c2, eps, lr_t, lr_r; };

// One component of Adam: updates m and s, returns u
GEOM_FN float bs_adam(float &m, float &s, float g, BsStep K)
{
    m = K.b1 * m + (1.0f - K.b1) * g;
    s = K.b2 * s + ((1.0f - K.b2) * g) * g;
    return (m / K.c1) / (sqrtf(s / K.c2) + K.eps);
}

// normalise((1, delta / 2) (x) q): the Cayley map, a rotation by |delta| up to O(|delta|^3) without sine or cosine.  delta == 0: q as it is.
GEOM_FN BsQuat bs_quat_step(BsQuat q, bs3 delta)
{
    if (delta.x == 0.0f && delta.y == 0.0f && delta.z == 0.0f) return q;
    const float hx = delta.x / 2.0f, hy = delta.y / 2.0f, hz = delta.z / 2.0f;
    const float nw = ((q.w - hx * q.x) - hy * q.y) - hz * q.z;
    const float nx = ((q.x + hx * q.w) + hy * q.z) - hz * q.y;
    const float ny = ((q.y - hx * q.z) + hy * q.w) + hz * q.x;
    const float nz = ((q.z + hx * q.y) - hy * q.x) + hz * q.w;
    const float n2 = ((nw * nw + nx * nx) + ny * ny) + nz * nz;
    const float n = sqrtf(n2);
    BsQuat o;
    o.w = nw / n, o.x = nx / n, o.y = ny / n, o.z = nz / n;
    return o;
}

// ---- the scene term: a vertex against the signed distance volume of its scene ----
struct BsSceneBox { float k[3], o[3]; };
struct BsAxis { int i0, i1; float w; bool in; };
struct BsSceneSample { float value; bs3 g; };              // g: d value / d x in the world, an exact zero along a clamped axis

// k = (D - 1) / (max - min) in fp64, rounded once; o = min (node-centred volumes: the first node lies on the box)
GEOM_FN BsSceneBox bs_scene_box(const float *gmin, const float *gmax, int D)
{
    BsSceneBox b;
    for (int a = 0; a < 3; a++) {
        b.k[a] = (float)((double)(D - 1) / ((double)gmax[a] - (double)gmin[a]));
        b.o[a] = gmin[a];
    }
    return b;
}

// u = (x - o) k; the median-of-three clamp written as max then min returns 0 for a NaN, so both indices lie in [0, D - 1] for every input
GEOM_FN BsAxis bs_scene_axis(float x, float o, float k, int D)
{
    const float dm1 = (float)(D - 1);
    const float u = (x - o) * k;
    BsAxis A;
    A.in = u > 0.0f && u < dm1;
    const float uc = fminf(fmaxf(u, 0.0f), dm1);
    const float fl = floorf(uc);
    A.i0 = (int)fl;
    A.w = uc - fl;
    A.i1 = A.i0 + 1 < D - 1 ? A.i0 + 1 : D - 1;
    return A;
}

GEOM_FN float bs_lerp(float a, float b, float w) { return a + w * (b - a); }

// q[dx][dy][dz]: the eight corners of the cell
GEOM_FN BsSceneSample bs_scene_sample(const float (&q)[2][2][2], BsAxis X, BsAxis Y, BsAxis Z, BsSceneBox box)
{
    float dz[2][2], r[2][2];
    for (int dx = 0; dx < 2; dx++)
        for (int dy = 0; dy < 2; dy++) {
            dz[dx][dy] = q[dx][dy][1] - q[dx][dy][0];
            r[dx][dy] = q[dx][dy][0] + Z.w * dz[dx][dy];
        }
    const float r0 = bs_lerp(r[0][0], r[0][1], Y.w), r1 = bs_lerp(r[1][0], r[1][1], Y.w);
    BsSceneSample s;
    s.value = bs_lerp(r0, r1, X.w);
    const float gx = r1 - r0;
    const float gy = bs_lerp(r[0][1] - r[0][0], r[1][1] - r[1][0], X.w);
    const float gz = bs_lerp(bs_lerp(dz[0][0], dz[0][1], Y.w), bs_lerp(dz[1][0], dz[1][1], Y.w), X.w);
    s.g = bs_make(X.in ? gx * box.k[0] : 0.0f, Y.in ? gy * box.k[1] : 0.0f, Z.in ? gz * box.k[2] : 0.0f);
    return s;
}

// The vertex x of a body in scene volume `vol` [D][D][D] (element [ix][iy][iz]): its sample; G = (-w_scene) g when value < 0, else +0
GEOM_FN BsSceneSample bs_scene_vertex(const float *vol, int D, BsSceneBox box, bs3 x, float w_scene, bs3 &G, bool &inside)
{
    const BsAxis X = bs_scene_axis(x.x, box.o[0], box.k[0], D), Y = bs_scene_axis(x.y, box.o[1], box.k[1], D);
    const BsAxis Z = bs_scene_axis(x.z, box.o[2], box.k[2], D);
    float q[2][2][2];
    for (int dx = 0; dx < 2; dx++)
        for (int dy = 0; dy < 2; dy++) {
            const size_t row = ((size_t)(dx ? X.i1 : X.i0) * D + (size_t)(dy ? Y.i1 : Y.i0)) * D;
            q[dx][dy][0] = vol[row + Z.i0], q[dx][dy][1] = vol[row + Z.i1];
        }
    const BsSceneSample s = bs_scene_sample(q, X, Y, Z, box);
    inside = s.value < 0.0f;
    const float nw = -w_scene;
    G = inside ? bs_make(nw * s.g.x, nw * s.g.y, nw * s.g.z) : bs_make(0.0f, 0.0f, 0.0f);
    return s;
}

// scene_id of a body: NULL is scene 0, a value outside [0, S) is clamped
GEOM_FN int bs_scene_of(const int32_t *scene_id, int b, int S)
{
    const int s = scene_id ? scene_id[b] : 0;
    return s < 0 ? 0 : (s > S - 1 ? S - 1 : s);
}
