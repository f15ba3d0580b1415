// The seven-region closest point of a triangle, host and device: one fp32 routine with a bit-level contract (DESIGN.md "Mesh -> SDF
// volume"), shared by csrc/mesh_sdf.hip (the distance volume of a scene mesh) and csrc/body_depth.hip (the penetration depth of one body in
// another).  Every including file is compiled with -ffp-contract=off; the division is IEEE-rounded on the device as on the host.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#define MS_FN __host__ __device__ __forceinline__

#ifdef __HIP_DEVICE_COMPILE__
#define MS_DIV(a, b) __fdiv_rn((a), (b))
#else
#define MS_DIV(a, b) ((a) / (b))
#endif

MS_FN float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// The closest point of the triangle (a, a + ab, a + ac) to p, with ap = p - a: r = p - c and the region c lies on
// (0 face, 1 edge ab, 2 edge bc, 3 edge ca, 4 vertex a, 5 vertex b, 6 vertex c).  The order of the tests is part of the contract.
MS_FN int closest_point(float abx, float aby, float abz, float acx, float acy, float acz, float apx, float apy, float apz, float &rx, float &ry,
                        float &rz)
{
    const float d1 = dot3(abx, aby, abz, apx, apy, apz), d2 = dot3(acx, acy, acz, apx, apy, apz);
    const float bpx = apx - abx, bpy = apy - aby, bpz = apz - abz;
    const float d3 = dot3(abx, aby, abz, bpx, bpy, bpz), d4 = dot3(acx, acy, acz, bpx, bpy, bpz);
    const float cpx = apx - acx, cpy = apy - acy, cpz = apz - acz;
    const float d5 = dot3(abx, aby, abz, cpx, cpy, cpz), d6 = dot3(acx, acy, acz, cpx, cpy, cpz);
    int region;
    float qx, qy, qz;
    if (d1 <= 0.0f && d2 <= 0.0f) {
        region = 4;
        qx = 0.0f; qy = 0.0f; qz = 0.0f;
    } else if (d3 >= 0.0f && d4 <= d3) {
        region = 5;
        qx = abx; qy = aby; qz = abz;
    } else if (d1 * d4 - d3 * d2 <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
        region = 1;
        const float v = MS_DIV(d1, d1 - d3);
        qx = v * abx; qy = v * aby; qz = v * abz;
    } else if (d6 >= 0.0f && d5 <= d6) {
        region = 6;
        qx = acx; qy = acy; qz = acz;
    } else if (d5 * d2 - d1 * d6 <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
        region = 3;
        const float w = MS_DIV(d2, d2 - d6);
        qx = w * acx; qy = w * acy; qz = w * acz;
    } else if (d3 * d6 - d5 * d4 <= 0.0f && d4 - d3 >= 0.0f && d5 - d6 >= 0.0f) {
        region = 2;
        const float w = MS_DIV(d4 - d3, (d4 - d3) + (d5 - d6));
        qx = abx + w * (acx - abx); qy = aby + w * (acy - aby); qz = abz + w * (acz - abz);
    } else {
        region = 0;
        const float va = d3 * d6 - d5 * d4, vb = d5 * d2 - d1 * d6, vc = d1 * d4 - d3 * d2;
        const float denom = MS_DIV(1.0f, (va + vb) + vc);
        const float v = vb * denom, w = vc * denom;
        qx = abx * v + acx * w; qy = aby * v + acy * w; qz = abz * v + acz * w;
    }
    rx = apx - qx; ry = apy - qy; rz = apz - qz;
    return region;
}

// closest_point, statement for statement, which also hands out the quotients and products it forms on the way: v (along ab) and w (along
// ac, or along bc in region 2); 0 where the region forms none.  r and the region have the bits closest_point gives.
MS_FN int closest_point_vw(float abx, float aby, float abz, float acx, float acy, float acz, float apx, float apy, float apz, float &rx,
                           float &ry, float &rz, float &v_out, float &w_out)
{
    const float d1 = dot3(abx, aby, abz, apx, apy, apz), d2 = dot3(acx, acy, acz, apx, apy, apz);
    const float bpx = apx - abx, bpy = apy - aby, bpz = apz - abz;
    const float d3 = dot3(abx, aby, abz, bpx, bpy, bpz), d4 = dot3(acx, acy, acz, bpx, bpy, bpz);
    const float cpx = apx - acx, cpy = apy - acy, cpz = apz - acz;
    const float d5 = dot3(abx, aby, abz, cpx, cpy, cpz), d6 = dot3(acx, acy, acz, cpx, cpy, cpz);
    int region;
    float qx, qy, qz;
    v_out = 0.0f; w_out = 0.0f;
    if (d1 <= 0.0f && d2 <= 0.0f) {
        region = 4;
        qx = 0.0f; qy = 0.0f; qz = 0.0f;
    } else if (d3 >= 0.0f && d4 <= d3) {
        region = 5;
        qx = abx; qy = aby; qz = abz;
    } else if (d1 * d4 - d3 * d2 <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
        region = 1;
        const float v = MS_DIV(d1, d1 - d3);
        qx = v * abx; qy = v * aby; qz = v * abz;
        v_out = v;
    } else if (d6 >= 0.0f && d5 <= d6) {
        region = 6;
        qx = acx; qy = acy; qz = acz;
    } else if (d5 * d2 - d1 * d6 <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
        region = 3;
        const float w = MS_DIV(d2, d2 - d6);
        qx = w * acx; qy = w * acy; qz = w * acz;
        w_out = w;
    } else if (d3 * d6 - d5 * d4 <= 0.0f && d4 - d3 >= 0.0f && d5 - d6 >= 0.0f) {
        region = 2;
        const float w = MS_DIV(d4 - d3, (d4 - d3) + (d5 - d6));
        qx = abx + w * (acx - abx); qy = aby + w * (acy - aby); qz = abz + w * (acz - abz);
        w_out = w;
    } else {
        region = 0;
        const float va = d3 * d6 - d5 * d4, vb = d5 * d2 - d1 * d6, vc = d1 * d4 - d3 * d2;
        const float denom = MS_DIV(1.0f, (va + vb) + vc);
        const float v = vb * denom, w = vc * denom;
        qx = abx * v + acx * w; qy = aby * v + acy * w; qz = abz * v + acz * w;
        v_out = v; w_out = w;
    }
    rx = apx - qx; ry = apy - qy; rz = apz - qz;
    return region;
}
