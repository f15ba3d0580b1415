// Surface crossings: the conic distance field of a list of triangle pairs, its aggregates per pair of bodies and the rows of the gradient
// of its loss, for gfx950 (wave64).  The contract is DESIGN.md section 10g; the statements are csrc/crossing_field_shared.h.  This file is
// compiled with -ffp-contract=off and IEEE division and square root.
//
//   pair       (i, s, j, t): face s of body i and face t of body j, in the caller's face indices of a psi_surface_crossings handle; the
//              list is strictly ascending, i <= j; any pair is allowed, not only a crossing one
//   role 0     the three corners of (i, s) evaluated in the record of (j, t): body i intrudes;  role 1 the other way round
//   row        psi [2,3] and energy [2] = (psi0^2 + psi1^2) + psi2^2 per role
//
// Passes: eval (one lane per (pair, role): the pair in one 16-byte read, six corners gathered, the receiver record built once for its three
// evaluations), pairs (one workgroup per body: wave 0 adds the entries of the body's row of pair_energy in fp64, one after the other in the
// order of the caller's stable sort of the entries by cell, which is pair order within a cell) and grad_rows (one lane per (pair, role):
// the forward once more on the same inputs, hence with the same bits, then six [3] rows and six int64 targets).  The rows are reduced by
// the caller's stable sort and psi_segment_sum3 (csrc/body_depth.hip).  No floating-point atomics, no scratch.
#include "crossing_field_shared.h"
#include "surface_crossings_handle.h"
#include "surface_crossings_shared.h"
#include "psi_common.h"
#include "wg_device.h"

namespace psi_cf {

constexpr int WG = WG_LANES;

// The six corners of a (pair, role) whose indices are in range: intruder p0 p1 p2, receiver a b c, and their vertex indices
struct Corners { cf3 p0, p1, p2, a, b, c; int ip0, ip1, ip2, ia, ib, ic; int bi, br; bool ok; };

__device__ __forceinline__ Corners cf_gather(const float *__restrict__ verts, const int32_t *__restrict__ faces, int B, int V, int F,
                                             const int4 *__restrict__ pairs, long long lane)
{
    Corners c;
    const int4 pr = pairs[lane >> 1];                       // (i, s, j, t) in one 16-byte read
    const bool role = lane & 1;
    c.bi = role ? pr.z : pr.x, c.br = role ? pr.x : pr.z;
    const int fi = role ? pr.w : pr.y, fr = role ? pr.y : pr.w;
    c.ok = (unsigned)c.bi < (unsigned)B && (unsigned)c.br < (unsigned)B && (unsigned)fi < (unsigned)F && (unsigned)fr < (unsigned)F;
    if (!c.ok) return c;
    const int32_t *f = faces + (size_t)fi * 3, *q = faces + (size_t)fr * 3;
    c.ip0 = f[0], c.ip1 = f[1], c.ip2 = f[2], c.ia = q[0], c.ib = q[1], c.ic = q[2];
    c.ok = (unsigned)c.ip0 < (unsigned)V && (unsigned)c.ip1 < (unsigned)V && (unsigned)c.ip2 < (unsigned)V && (unsigned)c.ia < (unsigned)V &&
           (unsigned)c.ib < (unsigned)V && (unsigned)c.ic < (unsigned)V;
    if (!c.ok) return c;
    const float *vi = verts + (size_t)c.bi * V * 3, *vr = verts + (size_t)c.br * V * 3;
    c.p0 = cf_load(vi + (size_t)c.ip0 * 3), c.p1 = cf_load(vi + (size_t)c.ip1 * 3), c.p2 = cf_load(vi + (size_t)c.ip2 * 3);
    c.a = cf_load(vr + (size_t)c.ia * 3), c.b = cf_load(vr + (size_t)c.ib * 3), c.c = cf_load(vr + (size_t)c.ic * 3);
    return c;
}

// psi [n,2,3] and energy [n,2]: lane 2k + role writes psi[k,role,:] and energy[k,role]
__global__ __launch_bounds__(WG) void cf_eval_kernel(const float *__restrict__ verts, const int32_t *__restrict__ faces, int B, int V, int F,
                                                     const int4 *__restrict__ pairs, long long n, float sigma, float *__restrict__ psi,
                                                     float *__restrict__ energy)
{
    const long long lane = (long long)blockIdx.x * WG + threadIdx.x;
    if (lane >= 2 * n) return;
    const Corners c = cf_gather(verts, faces, B, V, F, pairs, lane);
    float *out = psi + lane * 3;
    if (!c.ok) {
        out[0] = 0.0f, out[1] = 0.0f, out[2] = 0.0f;
        energy[lane] = 0.0f;
        return;
    }
    energy[lane] = cf_pair_role(c.p0, c.p1, c.p2, c.a, c.b, c.c, cf_consts(sigma), 0.0f, out, nullptr);
}

// rows [12n,3] and targets [12n]: lane 2k + role writes rows 6 lane .. 6 lane + 5 (the intruder's corners, then the receiver's)
__global__ __launch_bounds__(WG) void cf_grad_rows_kernel(const float *__restrict__ verts, const int32_t *__restrict__ faces, int B, int V, int F,
                                                          const int4 *__restrict__ pairs, long long n, float sigma,
                                                          const float *__restrict__ g, long long *__restrict__ targets,
                                                          float *__restrict__ rows)
{
    const long long lane = (long long)blockIdx.x * WG + threadIdx.x;
    if (lane >= 2 * n) return;
    const Corners c = cf_gather(verts, faces, B, V, F, pairs, lane);
    long long *tg = targets + lane * 6;
    float *out = rows + lane * 18;
    if (!c.ok) {
#pragma unroll
        for (int m = 0; m < 6; m++) tg[m] = -1;                 // a target the segment sum ignores
#pragma unroll
        for (int m = 0; m < 18; m++) out[m] = 0.0f;
        return;
    }
    float psi[3];
    cf_pair_role(c.p0, c.p1, c.p2, c.a, c.b, c.c, cf_consts(sigma), g[c.bi], psi, out);
    const long long bi = (long long)c.bi * V, br = (long long)c.br * V;
    tg[0] = bi + c.ip0, tg[1] = bi + c.ip1, tg[2] = bi + c.ip2;
    tg[3] = br + c.ia, tg[4] = br + c.ib, tg[5] = br + c.ic;
}

// The running sums of one row of pair_energy, uniform over the wave that carries them
struct RowSums { double sum, total; int cur; };

// One entry, in order: close the cell when the column changes (lane 0 stores it), then add.  col < 0: not an entry of this row.
__device__ __forceinline__ void cf_row_step(RowSums &s, double v, int col, bool lane0, double *__restrict__ row)
{
    if (col < 0) return;
    if (col != s.cur) {
        if (s.cur >= 0) {
            if (lane0) row[s.cur] = s.sum;
            s.total += s.sum;
        }
        s.cur = col;
        s.sum = 0.0;
    }
    s.sum += v;
}

// lane k's value of a wave, as a wave-uniform value (k is a constant after unrolling)
__device__ __forceinline__ double cf_lane_double(double v, int k)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), k), __builtin_amdgcn_readlane(__double2loint(v), k));
}

// One workgroup per body i, the row i of pair_energy.  The 2n (pair, role) entries were sorted stably by their cell (role 0 of (i, j): cell
// i B + j; role 1: cell j B + i), so the entries of row i are positions row_start[i] .. row_start[i+1] of `cells`, ascending in the column,
// and within a cell in pair order.  256 entries at a time are fetched by the 256 lanes and staged in LDS; wave 0 takes them into
// registers, four per lane, and walks them one after the other in order (v_readlane with constant lane numbers: every value and every
// running sum is uniform over the wave, so the walk has no LDS round trip and no divergent branch): it adds in fp64, closes a cell when
// the column changes and adds the closed cells to the body's loss in column order.  pair_energy is zeroed by the caller; loss is written
// for every body.
__global__ __launch_bounds__(WG) void cf_pairs_kernel(const int4 *__restrict__ pairs, const float *__restrict__ energy,
                                                      const long long *__restrict__ cells, const long long *__restrict__ order,
                                                      const long long *__restrict__ row_start, long long n, int B,
                                                      double *__restrict__ pair_energy, float *__restrict__ loss)
{
    static_assert(WG == 256, "wave 0 takes four staged entries per lane");
    __shared__ double s_v[WG];
    __shared__ int s_col[WG];
    const int i = blockIdx.x, t = threadIdx.x;
    const long long lo = max(row_start[i], 0ll), hi = min(row_start[i + 1], 2 * n);
    double *row = pair_energy + (size_t)i * B;
    RowSums s = {0.0, 0.0, -1};
    for (long long r0 = lo; r0 < hi; r0 += WG) {
        const long long r = r0 + t;
        double v = 0.0;
        int col = -1;
        if (r < hi) {
            const long long e = order[r], cell = cells[r];
            if (e >= 0 && e < 2 * n && cell >= (long long)i * B && cell < (long long)(i + 1) * B) {
                const int4 pr = pairs[e >> 1];
                col = (int)(cell - (long long)i * B);
                v = cf_entry_value(pr.x, pr.z, (int)(e & 1), energy[e & ~1ll], energy[e | 1ll]);
                if (pr.x == pr.z && (e & 1)) col = -1;          // a self pair's role-1 entry: added with its role-0 entry
            }
        }
        s_v[t] = v;
        s_col[t] = col;
        __syncthreads();
        if (t < 64) {
            const double v0 = s_v[t], v1 = s_v[t + 64], v2 = s_v[t + 128], v3 = s_v[t + 192];
            const int c0 = s_col[t], c1 = s_col[t + 64], c2 = s_col[t + 128], c3 = s_col[t + 192];
#pragma unroll
            for (int k = 0; k < 64; k++) cf_row_step(s, cf_lane_double(v0, k), __builtin_amdgcn_readlane(c0, k), t == 0, row);
#pragma unroll
            for (int k = 0; k < 64; k++) cf_row_step(s, cf_lane_double(v1, k), __builtin_amdgcn_readlane(c1, k), t == 0, row);
#pragma unroll
            for (int k = 0; k < 64; k++) cf_row_step(s, cf_lane_double(v2, k), __builtin_amdgcn_readlane(c2, k), t == 0, row);
#pragma unroll
            for (int k = 0; k < 64; k++) cf_row_step(s, cf_lane_double(v3, k), __builtin_amdgcn_readlane(c3, k), t == 0, row);
        }
        __syncthreads();
    }
    if (t == 0) {
        if (s.cur >= 0) {
            row[s.cur] = s.sum;
            s.total += s.sum;
        }
        loss[i] = (float)s.total;
    }
}

}  // namespace psi_cf

#define CF_REQUIRE(h, B, n, sigma)                                                                                  \
    PSI_REQUIRE(B >= 1 && B <= GEOM_MAX_B, "1 <= B <= 46340");                                                      \
    PSI_REQUIRE(n >= 1 && n < (1ll << 27), "1 <= n < 2^27");                                                        \
    PSI_REQUIRE(sigma > 0.0f && sigma <= 0.5f, "0 < sigma <= 0.5")

extern "C" int psi_crossing_field_eval(const psi_surface_crossings *h, const float *d_verts, int B, const int32_t *d_pairs, long long n,
                                       float sigma, float *d_psi, float *d_energy, void *stream)
{
    PSI_REQUIRE(h && d_verts && d_pairs && d_psi && d_energy, "null pointer");
    CF_REQUIRE(h, B, n, sigma);
    PSI_REQUIRE(((uintptr_t)d_pairs & 15) == 0, "d_pairs is 16-byte aligned");
    hipLaunchKernelGGL(psi_cf::cf_eval_kernel, dim3(psi_cdiv(2 * n, psi_cf::WG)), dim3(psi_cf::WG), 0, (hipStream_t)stream, d_verts, h->d_caller,
                       B, h->V, h->F, (const int4 *)d_pairs, n, sigma, d_psi, d_energy);
    PSI_CHECK_LAUNCH("cf_eval_kernel");
    return 0;
}

extern "C" int psi_crossing_field_pairs(const psi_surface_crossings *h, int B, const int32_t *d_pairs, long long n, const float *d_energy,
                                        const int64_t *d_cells_sorted, const int64_t *d_order, const int64_t *d_row_start,
                                        double *d_pair_energy, float *d_loss, void *stream)
{
    PSI_REQUIRE(h && d_pairs && d_energy && d_cells_sorted && d_order && d_row_start && d_pair_energy && d_loss, "null pointer");
    CF_REQUIRE(h, B, n, 0.5f);
    PSI_REQUIRE(((uintptr_t)d_pairs & 15) == 0, "d_pairs is 16-byte aligned");
    hipLaunchKernelGGL(psi_cf::cf_pairs_kernel, dim3(B), dim3(psi_cf::WG), 0, (hipStream_t)stream, (const int4 *)d_pairs, d_energy,
                       (const long long *)d_cells_sorted, (const long long *)d_order, (const long long *)d_row_start, n, B, d_pair_energy,
                       d_loss);
    PSI_CHECK_LAUNCH("cf_pairs_kernel");
    return 0;
}

extern "C" int psi_crossing_field_grad_rows(const psi_surface_crossings *h, const float *d_verts, int B, const int32_t *d_pairs, long long n,
                                            float sigma, const float *d_g, int64_t *d_targets, float *d_rows, void *stream)
{
    PSI_REQUIRE(h && d_verts && d_pairs && d_g && d_targets && d_rows, "null pointer");
    CF_REQUIRE(h, B, n, sigma);
    PSI_REQUIRE(((uintptr_t)d_pairs & 15) == 0, "d_pairs is 16-byte aligned");
    hipLaunchKernelGGL(psi_cf::cf_grad_rows_kernel, dim3(psi_cdiv(2 * n, psi_cf::WG)), dim3(psi_cf::WG), 0, (hipStream_t)stream, d_verts,
                       h->d_caller, B, h->V, h->F, (const int4 *)d_pairs, n, sigma, d_g, (long long *)d_targets, d_rows);
    PSI_CHECK_LAUNCH("cf_grad_rows_kernel");
    return 0;
}
