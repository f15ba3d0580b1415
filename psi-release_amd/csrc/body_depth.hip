// Body against body: how deep a vertex of one body of a batch lies in another body, the aggregates per pair of bodies, and the rows of the
// gradient of the penetration loss, for gfx950 (wave64).  The contract is DESIGN.md section 10f; the per-triple statements are
// csrc/body_depth_shared.h and csrc/closest_point_shared.h.  This file is compiled with -ffp-contract=off and IEEE division and square root.
//
//   triple     (i, j, v), i != j: vertex v of body i against the F current triangles of body j; the list is strictly ascending.  The inside
//              triples of a batch are the candidates of csrc/body_overlap.hip with w > 0.5, but any triple is allowed
//   record     of face t of body j: a = X[f0], ab = X[f1] - a, ac = X[f2] - a, each rounded once
//   winner     the face with the smallest key = bits(d2) << 32 | t, d2 = (r.x*r.x + r.y*r.y) + r.z*r.z of the seven-region closest point:
//              equal d2 goes to the lower face, a non-finite d2 loses to every finite one, the visiting order is free
//   row        face, region, depth = sqrt(d2), r = p - c, and the barycentric coordinates of c
//
// Passes: nearest (the hot pass; grid = 256-triple chunk of ONE pair x 2048-face slice, as bo_wind_kernel: per 256 faces every lane stages
// one record in LDS, then every lane reads every record, identical addresses broadcast; a lane keeps its smallest key in registers and
// writes one key per (slice, triple)), finish (the smallest key over the slices, the winner's statement once more, the row), pairs (one
// workgroup per body i: lane 0 adds the depths of its inside triples in fp64, in triple order), grad_rows (four rows per triple) and the
// general psi_segment_sum3 (the lane that starts a run of equal sorted targets adds the run in order and stores once).  No floating-point
// atomics.
#include "body_depth_shared.h"
#include "psi_common.h"
#include "wg_device.h"

namespace psi_bd {

constexpr int WG = WG_LANES;
static_assert(WG == BD_CHUNK, "one staged record per lane");

struct Chunk { int first, n, i, j; };          // body_overlap's table: first triple, triples, the pair
static_assert(sizeof(Chunk) == 16, "the chunk table is [n_chunks,4] int32");

// keys [n_slices, n] uint64: the smallest key of every triple within a slice of faces.  grid = (chunk, slice).
__global__ __launch_bounds__(WG) void bd_nearest_kernel(const float *__restrict__ verts, const int32_t *__restrict__ faces, int B, int V, int F,
                                                        const int *__restrict__ trip, long long n, const Chunk *__restrict__ chunks,
                                                        unsigned long long *__restrict__ keys)
{
    __shared__ float4 stage[WG * 3];           // 12 KB: 256 records (a.xyz ab.x | ab.yz ac.xy | ac.z - - -)
    const int t = threadIdx.x, slice = blockIdx.y;
    const Chunk ch = chunks[blockIdx.x];
    const long long ci = (long long)ch.first + t;
    if ((unsigned)ch.i >= (unsigned)B || (unsigned)ch.j >= (unsigned)B || ch.first < 0) return;      // the same in every lane
    const int v = t < ch.n && ci < n ? trip[ci * 3 + 2] : -1;
    const bool live = (unsigned)v < (unsigned)V;
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (live) {
        const float *p = verts + ((size_t)ch.i * V + v) * 3;
        px = p[0], py = p[1], pz = p[2];
    }
    const float *vj = verts + (size_t)ch.j * V * 3;
    const int f_end = min(F, (slice + 1) * BD_SLICE);
    unsigned long long best = ~0ull;
    for (int f0 = slice * BD_SLICE; f0 < f_end; f0 += BD_CHUNK) {
        const int nst = min(BD_CHUNK, f_end - f0);
        if (t < nst) {
            const BdRecord r = bd_record(vj, faces + (size_t)(f0 + t) * 3);
            stage[3 * t] = make_float4(r.a[0], r.a[1], r.a[2], r.ab[0]);
            stage[3 * t + 1] = make_float4(r.ab[1], r.ab[2], r.ac[0], r.ac[1]);
            stage[3 * t + 2] = make_float4(r.ac[2], 0.0f, 0.0f, 0.0f);
        }
        __syncthreads();
        if (live) {
            for (int k = 0; k < nst; k++) {
                const float4 r0 = stage[3 * k], r1 = stage[3 * k + 1];
                const float acz = stage[3 * k + 2].x;
                const unsigned long long key = bd_test(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, acz, px, py, pz, f0 + k);
                best = key < best ? key : best;
            }
        }
        __syncthreads();
    }
    if (live) keys[(size_t)slice * n + ci] = best;
}

// One lane per triple: the smallest key over the slices, then the winner's statement once more
__global__ __launch_bounds__(WG) void bd_finish_kernel(const float *__restrict__ verts, const int32_t *__restrict__ faces, int B, int V, int F,
                                                       const int *__restrict__ trip, long long n,
                                                       const unsigned long long *__restrict__ keys, int n_slices, int *__restrict__ face,
                                                       int *__restrict__ region, float *__restrict__ depth, float *__restrict__ r,
                                                       float *__restrict__ bary)
{
    const long long c = (long long)blockIdx.x * WG + threadIdx.x;
    if (c >= n) return;
    unsigned long long best = keys[c];
    for (int k = 1; k < n_slices; k++) {
        const unsigned long long key = keys[(size_t)k * n + c];
        best = key < best ? key : best;
    }
    const int t = (int)min((unsigned int)(best & 0xffffffffull), (unsigned int)(F - 1));      // a face of the handle whatever the workspace holds
    const int i = trip[c * 3], j = trip[c * 3 + 1], v = trip[c * 3 + 2];
    if ((unsigned)i >= (unsigned)B || (unsigned)j >= (unsigned)B || (unsigned)v >= (unsigned)V) return;    // not a triple of this batch
    const float *p = verts + ((size_t)i * V + v) * 3;
    const BdRecord rec = bd_record(verts + (size_t)j * V * 3, faces + (size_t)t * 3);
    const BdRow o = bd_row(rec, p[0], p[1], p[2], t);
    face[c] = o.face;
    region[c] = o.region;
    depth[c] = o.depth;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        r[c * 3 + a] = o.r[a];
        bary[c * 3 + a] = o.bary[a];
    }
}

// One workgroup per body i, whose inside triples are rows row_start[i] .. row_start[i+1] of the ascending list: lane 0 adds their depths and
// squared depths in fp64, one after the other in triple order, per pair (i, j) and, the pair sums in j order, per body; the largest depth
// of a pair and of a vertex by an integer maximum on the bits (depths are >= 0).  max_depth, sum_depth, sum_sq and depth_of are zeroed by
// the caller; loss [2,B] is written for every body.
__global__ __launch_bounds__(WG) void bd_pairs_kernel(const int *__restrict__ trip, const float *__restrict__ depth,
                                                      const long long *__restrict__ row_start, long long n, int B, int V,
                                                      float *__restrict__ max_depth,
                                                      double *__restrict__ sum_depth, double *__restrict__ sum_sq,
                                                      unsigned int *__restrict__ depth_of, float *__restrict__ loss)
{
    __shared__ float s_d[WG];
    __shared__ int s_j[WG];
    const int i = blockIdx.x, t = threadIdx.x;
    const long long lo = max(row_start[i], 0ll), hi = min(row_start[i + 1], n);
    double sum = 0.0, sq = 0.0, total = 0.0, total_sq = 0.0;
    unsigned int mx = 0u;
    int cur = -1;
    for (long long r0 = lo; r0 < hi; r0 += WG) {
        const long long r = r0 + t;
        const bool mine = r < hi;
        const float d = mine ? depth[r] : 0.0f;
        int j = -1;
        if (mine) {
            j = trip[r * 3 + 1];
            const int v = trip[r * 3 + 2];
            if (v >= 0 && v < V) atomicMax(depth_of + (size_t)i * V + v, bd_bits(d));
        }
        s_d[t] = d;
        s_j[t] = j;
        __syncthreads();
        if (t == 0) {
            const int nst = (int)min((long long)WG, hi - r0);
            for (int k = 0; k < nst; k++) {
                const int jj = s_j[k];
                if (jj != cur) {
                    if (cur >= 0 && cur < B) {
                        max_depth[(size_t)i * B + cur] = __uint_as_float(mx);
                        sum_depth[(size_t)i * B + cur] = sum;
                        sum_sq[(size_t)i * B + cur] = sq;
                        total += sum;
                        total_sq += sq;
                    }
                    cur = jj;
                    sum = 0.0, sq = 0.0, mx = 0u;
                }
                const double dd = (double)s_d[k];
                sum += dd;
                sq += dd * dd;
                mx = max(mx, bd_bits(s_d[k]));
            }
        }
        __syncthreads();
    }
    if (t == 0) {
        if (cur >= 0 && cur < B) {
            max_depth[(size_t)i * B + cur] = __uint_as_float(mx);
            sum_depth[(size_t)i * B + cur] = sum;
            sum_sq[(size_t)i * B + cur] = sq;
            total += sum;
            total_sq += sq;
        }
        loss[i] = (float)total;
        loss[B + i] = (float)total_sq;
    }
}

// targets [4n] int64 and rows [4n,3] fp32: triple k writes rows 4k .. 4k+3
__global__ __launch_bounds__(WG) void bd_grad_rows_kernel(const int32_t *__restrict__ faces, int B, int V, int F, const int *__restrict__ trip, long long n,
                                                          const int *__restrict__ face, const float *__restrict__ depth,
                                                          const float *__restrict__ r, const float *__restrict__ bary,
                                                          const float *__restrict__ g, int penalty, long long *__restrict__ targets,
                                                          float *__restrict__ rows)
{
    const long long c = (long long)blockIdx.x * WG + threadIdx.x;
    if (c >= n) return;
    const int i = trip[c * 3], j = trip[c * 3 + 1], v = trip[c * 3 + 2], t = face[c];
    if ((unsigned)i >= (unsigned)B || (unsigned)j >= (unsigned)B || (unsigned)v >= (unsigned)V || (unsigned)t >= (unsigned)F) {
#pragma unroll
        for (int m = 0; m < 4; m++) targets[c * 4 + m] = -1;        // a target the segment sum ignores
        return;
    }
    const int32_t *f = faces + (size_t)t * 3;
    const float rr[3] = {r[c * 3], r[c * 3 + 1], r[c * 3 + 2]}, bb[3] = {bary[c * 3], bary[c * 3 + 1], bary[c * 3 + 2]};
    float out[4][3];
    bd_grad_rows(g[i], penalty, depth[c], rr, bb, out);
    targets[c * 4] = (long long)i * V + v;
#pragma unroll
    for (int m = 0; m < 3; m++) targets[c * 4 + 1 + m] = (long long)j * V + f[m];
#pragma unroll
    for (int m = 0; m < 4; m++)
#pragma unroll
        for (int a = 0; a < 3; a++) rows[(c * 4 + m) * 3 + a] = out[m][a];
}

// out[target] = ((0 + x0) + x1) + ... over the run of equal targets, in fp32, in the order of the sorted list
__global__ __launch_bounds__(WG) void segment_sum3_kernel(const long long *__restrict__ targets, const long long *__restrict__ order,
                                                          const float *__restrict__ rows, long long m, float *__restrict__ out,
                                                          long long n_out)
{
    const long long k = (long long)blockIdx.x * WG + threadIdx.x;
    if (k >= m) return;
    const long long tgt = targets[k];
    if (k > 0 && targets[k - 1] == tgt) return;                 // not the start of a run
    if (tgt < 0 || tgt >= n_out) return;
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
    for (long long q = k; q < m && targets[q] == tgt; q++) {
        const long long from = order ? order[q] : q;
        if (from < 0 || from >= m) continue;
        ax = ax + rows[from * 3];
        ay = ay + rows[from * 3 + 1];
        az = az + rows[from * 3 + 2];
    }
    out[tgt * 3] = ax;
    out[tgt * 3 + 1] = ay;
    out[tgt * 3 + 2] = az;
}

}  // namespace psi_bd

#define BD_REQUIRE_N(h, B, n)                                                                                       \
    PSI_REQUIRE(B >= 1 && B <= GEOM_MAX_B, "1 <= B <= 46340");                                                      \
    PSI_REQUIRE(n >= 1 && n < (1ll << 29), "1 <= n < 2^29")

extern "C" size_t psi_body_depth_workspace_bytes(long long n, int F)
{
    if (n < 1 || n >= (1ll << 29) || F < 1) return 0;
    return (size_t)bd_slices(F) * (size_t)n * sizeof(unsigned long long);
}

extern "C" int psi_body_depth_nearest(const psi_body_overlap *h, const float *d_verts, int B, const int32_t *d_trip, long long n,
                                      const int32_t *d_chunks, long long n_chunks, void *d_workspace, size_t workspace_bytes, void *stream)
{
    PSI_REQUIRE(h && d_verts && d_trip && d_chunks && d_workspace, "null pointer");
    BD_REQUIRE_N(h, B, n);
    PSI_REQUIRE(n_chunks >= 1 && n_chunks <= n, "1 <= n_chunks <= n");
    PSI_REQUIRE(workspace_bytes >= psi_body_depth_workspace_bytes(n, h->F), "workspace too small");
    hipLaunchKernelGGL(psi_bd::bd_nearest_kernel, dim3((unsigned)n_chunks, bd_slices(h->F)), dim3(psi_bd::WG), 0, (hipStream_t)stream, d_verts,
                       h->d_faces, B, h->V, h->F, d_trip, n, (const psi_bd::Chunk *)d_chunks, (unsigned long long *)d_workspace);
    PSI_CHECK_LAUNCH("bd_nearest_kernel");
    return 0;
}

extern "C" int psi_body_depth_finish(const psi_body_overlap *h, const float *d_verts, int B, const int32_t *d_trip, long long n,
                                     const void *d_workspace, size_t workspace_bytes, int32_t *d_face, int32_t *d_region, float *d_depth,
                                     float *d_r, float *d_bary, void *stream)
{
    PSI_REQUIRE(h && d_verts && d_trip && d_workspace && d_face && d_region && d_depth && d_r && d_bary, "null pointer");
    BD_REQUIRE_N(h, B, n);
    PSI_REQUIRE(workspace_bytes >= psi_body_depth_workspace_bytes(n, h->F), "workspace too small");
    hipLaunchKernelGGL(psi_bd::bd_finish_kernel, dim3(psi_cdiv(n, psi_bd::WG)), dim3(psi_bd::WG), 0, (hipStream_t)stream, d_verts, h->d_faces,
                       B, h->V, h->F, d_trip, n, (const unsigned long long *)d_workspace, bd_slices(h->F), d_face, d_region, d_depth, d_r, d_bary);
    PSI_CHECK_LAUNCH("bd_finish_kernel");
    return 0;
}

extern "C" int psi_body_depth_pairs(const psi_body_overlap *h, int B, const int32_t *d_trip, long long n, const float *d_depth,
                                    const int64_t *d_row_start, float *d_max_depth, double *d_sum_depth, double *d_sum_sq, float *d_depth_of,
                                    float *d_loss, void *stream)
{
    PSI_REQUIRE(h && d_trip && d_depth && d_row_start && d_max_depth && d_sum_depth && d_sum_sq && d_depth_of && d_loss, "null pointer");
    BD_REQUIRE_N(h, B, n);
    hipLaunchKernelGGL(psi_bd::bd_pairs_kernel, dim3(B), dim3(psi_bd::WG), 0, (hipStream_t)stream, d_trip, d_depth,
                       (const long long *)d_row_start, n, B, h->V, d_max_depth, d_sum_depth, d_sum_sq, (unsigned int *)d_depth_of, d_loss);
    PSI_CHECK_LAUNCH("bd_pairs_kernel");
    return 0;
}

extern "C" int psi_body_depth_grad_rows(const psi_body_overlap *h, int B, const int32_t *d_trip, long long n, const int32_t *d_face,
                                        const float *d_depth, const float *d_r, const float *d_bary, const float *d_g, int penalty,
                                        int64_t *d_targets, float *d_rows, void *stream)
{
    PSI_REQUIRE(h && d_trip && d_face && d_depth && d_r && d_bary && d_g && d_targets && d_rows, "null pointer");
    BD_REQUIRE_N(h, B, n);
    PSI_REQUIRE(penalty == BD_DEPTH || penalty == BD_SQUARED, "penalty is 0 (depth) or 1 (squared)");
    hipLaunchKernelGGL(psi_bd::bd_grad_rows_kernel, dim3(psi_cdiv(n, psi_bd::WG)), dim3(psi_bd::WG), 0, (hipStream_t)stream, h->d_faces, B, h->V,
                       h->F, d_trip, n, d_face, d_depth, d_r, d_bary, d_g, penalty, (long long *)d_targets, d_rows);
    PSI_CHECK_LAUNCH("bd_grad_rows_kernel");
    return 0;
}

extern "C" int psi_segment_sum3(const int64_t *d_targets_sorted, const int64_t *d_order, const float *d_rows, long long m, float *d_out,
                                long long n_out, void *stream)
{
    PSI_REQUIRE(d_targets_sorted && d_rows && d_out, "null pointer");
    PSI_REQUIRE(m >= 1 && m < (1ll << 31), "1 <= m < 2^31");
    PSI_REQUIRE(n_out >= 1, "n_out >= 1");
    hipLaunchKernelGGL(psi_bd::segment_sum3_kernel, dim3(psi_cdiv(m, psi_bd::WG)), dim3(psi_bd::WG), 0, (hipStream_t)stream,
                       (const long long *)d_targets_sorted, (const long long *)d_order, d_rows, m, d_out, n_out);
    PSI_CHECK_LAUNCH("segment_sum3_kernel");
    return 0;
}
