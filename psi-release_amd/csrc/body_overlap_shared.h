// The per-triple statements of the body-against-body overlap test (DESIGN.md "Body against body"), shared by csrc/body_overlap.hip and by
// the host rehearsal tools/body_overlap_host_check.hip.  Everything that decides membership (box, threshold) is a comparison; the winding
// number is fp32 within a chunk of BO_CHUNK faces and fp64 across the chunks of a slice of BO_SLICE faces and across the slices.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#define BO_FN __host__ __device__ __forceinline__

constexpr int BO_CHUNK = 256;       // consecutive faces summed in fp32: a constant of the contract, not a launch parameter
constexpr int BO_SLICE = 2048;      // consecutive faces whose chunk sums are added in fp64, in order, before the slices are
constexpr int BO_CHUNKS_PER_SLICE = BO_SLICE / BO_CHUNK;

BO_FN float bo_dot3(float ax, float ay, float az, float bx, float by, float bz) { return ax * bx + ay * by + az * bz; }

// n = (B - A) x (C - A) of a body's current vertices, fp32
BO_FN void bo_normal(const float A[3], const float B[3], const float C[3], float n[3])
{
    const float ux = B[0] - A[0], uy = B[1] - A[1], uz = B[2] - A[2];
    const float vx = C[0] - A[0], vy = C[1] - A[1], vz = C[2] - A[2];
    n[0] = uy * vz - uz * vy;
    n[1] = uz * vx - ux * vz;
    n[2] = ux * vy - uy * vx;
}

// half the solid angle of the triangle (A, B, C) seen from p, signed: the statement of csrc/mesh_winding.hip, atan2(0, 0) = 0 included
BO_FN float bo_half_omega(float Ax, float Ay, float Az, float Bx, float By, float Bz, float Cx, float Cy, float Cz, float nx, float ny, float nz,
                          float px, float py, float pz)
{
    const float ax = Ax - px, ay = Ay - py, az = Az - pz;
    const float bx = Bx - px, by = By - py, bz = Bz - pz;
    const float cx = Cx - px, cy = Cy - py, cz = Cz - pz;
    const float la = sqrtf(bo_dot3(ax, ay, az, ax, ay, az)), lb = sqrtf(bo_dot3(bx, by, bz, bx, by, bz)), lc = sqrtf(bo_dot3(cx, cy, cz, cx, cy, cz));
    const float det = bo_dot3(ax, ay, az, nx, ny, nz);
    const float den = la * lb * lc + bo_dot3(ax, ay, az, bx, by, bz) * lc + bo_dot3(bx, by, bz, cx, cy, cz) * la + bo_dot3(cx, cy, cz, ax, ay, az) * lb;
    return (det == 0.0f && den == 0.0f) ? 0.0f : atan2f(det, den);
}

// p inside the closed box [lo, hi]: comparisons only
BO_FN bool bo_in_box(float px, float py, float pz, const float lo[3], const float hi[3])
{
    return px >= lo[0] && px <= hi[0] && py >= lo[1] && py <= hi[1] && pz >= lo[2] && pz <= hi[2];
}

// the closed boxes [alo, ahi] and [blo, bhi] share a point
BO_FN bool bo_boxes_meet(const float alo[3], const float ahi[3], const float blo[3], const float bhi[3])
{
    return alo[0] <= bhi[0] && blo[0] <= ahi[0] && alo[1] <= bhi[1] && blo[1] <= ahi[1] && alo[2] <= bhi[2] && blo[2] <= ahi[2];
}

BO_FN float bo_w_of_sum(double s) { return (float)(s / 6.283185307179586476925286766559); }

BO_FN bool bo_inside(float w) { return w > 0.5f; }

BO_FN int bo_slices(int F) { return (F + BO_SLICE - 1) / BO_SLICE; }
