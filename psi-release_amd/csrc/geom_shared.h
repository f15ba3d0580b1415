// The statements the geometry passes share, host and device: csrc/mesh_winding.hip, csrc/body_overlap.hip and csrc/surface_crossings.hip
// with their *_shared.h headers, and the host rehearsals under tools/ that run the same text on the CPU.  Nothing here needs a device
// compiler's extensions beyond the __host__ __device__ markers.  Contraction is the including file's: the winding-number statements carry a
// tolerance contract (DESIGN.md "Winding-number sign", section 10d), the box tests are comparisons only.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#define GEOM_FN __host__ __device__ __forceinline__

constexpr int GEOM_MAX_B = 46340;       // bodies per batch: B * B < 2^31, one workgroup per ordered pair

GEOM_FN float geom_dot3(float ax, float ay, float az, float bx, float by, float bz) { return ax * bx + ay * by + az * bz; }

// n = (B - A) x (C - A) in fp32 (body against body; the winding number of a scene mesh takes its normal from the host in fp64)
GEOM_FN void geom_normal(const float A[3], const float B[3], const float C[3], float n[3])
{
    const float ux = B[0] - A[0], uy = B[1] - A[1], uz = B[2] - A[2];
    const float vx = C[0] - A[0], vy = C[1] - A[1], vz = C[2] - A[2];
    n[0] = uy * vz - uz * vy;
    n[1] = uz * vx - ux * vz;
    n[2] = ux * vy - uy * vx;
}

// half the solid angle of the triangle (A, B, C) with normal n seen from p, signed; atan2(0, 0) counts as 0
GEOM_FN float geom_half_omega(float Ax, float Ay, float Az, float Bx, float By, float Bz, float Cx, float Cy, float Cz, float nx, float ny, float nz,
                              float px, float py, float pz)
{
    const float ax = Ax - px, ay = Ay - py, az = Az - pz;
    const float bx = Bx - px, by = By - py, bz = Bz - pz;
    const float cx = Cx - px, cy = Cy - py, cz = Cz - pz;
    const float la = sqrtf(geom_dot3(ax, ay, az, ax, ay, az)), lb = sqrtf(geom_dot3(bx, by, bz, bx, by, bz)), lc = sqrtf(geom_dot3(cx, cy, cz, cx, cy, cz));
    const float det = geom_dot3(ax, ay, az, nx, ny, nz);
    const float den = la * lb * lc + geom_dot3(ax, ay, az, bx, by, bz) * lc + geom_dot3(bx, by, bz, cx, cy, cz) * la + geom_dot3(cx, cy, cz, ax, ay, az) * lb;
    return (det == 0.0f && den == 0.0f) ? 0.0f : atan2f(det, den);
}

// p inside the closed box [lo, hi]: comparisons only
GEOM_FN bool geom_in_box(float px, float py, float pz, const float lo[3], const float hi[3])
{
    return px >= lo[0] && px <= hi[0] && py >= lo[1] && py <= hi[1] && pz >= lo[2] && pz <= hi[2];
}

// the closed boxes [alo, ahi] and [blo, bhi] share a point
GEOM_FN bool geom_boxes_meet(const float alo[3], const float ahi[3], const float blo[3], const float bhi[3])
{
    return alo[0] <= bhi[0] && blo[0] <= ahi[0] && alo[1] <= bhi[1] && blo[1] <= ahi[1] && alo[2] <= bhi[2] && blo[2] <= ahi[2];
}
