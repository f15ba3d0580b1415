// Two slices per search workgroup (fit.hip: fwd_scene_kernel<.., SPW = 2>): where the tree walk's stack entries live in the engine's
// kd_stack buffer, and when the shape is used at all.  No dependencies: tools/search_shape_host_check.hip runs these statements on the host.
//
// kd_stack holds a region of 2 rows 4-byte entries per contact query of every body: [B][n][2][rows] — entry i of the child references at
// word i, of the box distances at word rows + i.  The search addresses an entry as (uniform base of the body) + (32-bit offset of the
// query's entry), so a body's regions must stay inside a 32-bit offset.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PSI_SHAPE_HD __host__ __device__
#else
#define PSI_SHAPE_HD
#endif

PSI_SHAPE_HD constexpr size_t psi_search_stack_bytes(int B, int n, int rows) { return (size_t)B * (size_t)n * (size_t)rows * 8; }
PSI_SHAPE_HD constexpr size_t psi_search_stack_body_base(int b, int n, int rows) { return (size_t)b * (size_t)n * (size_t)rows * 8; }      // bytes
PSI_SHAPE_HD constexpr bool psi_search_stack_fits(int n, int rows) { return n > 0 && rows > 0 && (size_t)n * (size_t)rows * 8 < ((size_t)1 << 32); }
// byte offset inside the body's part of entry i of query jq: which = 0 child reference, 1 box distance
PSI_SHAPE_HD constexpr unsigned psi_search_stack_entry(int jq, int rows, int which, int i)
{
    return (unsigned)jq * (unsigned)(8 * rows) + 4u * (unsigned)(which * rows + i);
}

// Workgroups of the shared launch that a CU holds: the register budget allows `cap` (6), LDS what fits of static + dynamic bytes per workgroup.
PSI_SHAPE_HD constexpr int psi_search_wgs_per_cu(size_t lds_cu, size_t lds_static, size_t lds_dynamic, int cap)
{
    return lds_static + lds_dynamic == 0 ? cap : (int)(lds_cu / (lds_static + lds_dynamic)) < cap ? (int)(lds_cu / (lds_static + lds_dynamic)) : cap;
}
// Two slices are used only where they cost no residency: the second wave pair's rotation rows add static LDS, and with a deep tree (a
// large dynamic part) that is the step from six workgroups per CU to five — a regime nobody measured, which keeps the one-slice shape.
// static1 / static2: static LDS of the one- and the two-slice instance (0: unknown -> one slice)
PSI_SHAPE_HD constexpr int psi_search_spw_for(size_t lds_cu, size_t static1, size_t static2, size_t lds_dynamic, int cap)
{
    return static1 && static2 && psi_search_wgs_per_cu(lds_cu, static2, lds_dynamic, cap) >= psi_search_wgs_per_cu(lds_cu, static1, lds_dynamic, cap) ? 2 : 1;
}
