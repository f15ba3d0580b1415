// psi_mesh_cloud_*: even surface samples of a triangle mesh, about one per `spacing` cell whatever the tessellation.
//
// The rule lives in mesh_cloud_shared.h (candidates row by row across every triangle, then the candidate nearest to the centre of its
// cell); this file spreads it over the device.  Work is spread by rows and by candidates, never by triangles, so a floor of two triangles
// is as many workgroups as a floor of ten thousand:
//
//   mcloud_count_kernel    one WAVE per triangle (grid-stride): the lanes share the rows of the triangle, count its candidates and reduce
//                          them with integer shuffles.  Validates the face indices and the coordinates, takes the box of the referenced
//                          vertices (integer atomicMin / atomicMax on order-preserving bits) and the totals (integer atomicAdd): all
//                          order-independent.  psi_mesh_cloud_count reads the 64-byte state back: the one verdict of the call.
//   mcloud_rows_kernel     one thread per row: its triangle (a binary search in the exclusive scan of the rows per triangle) and its
//                          candidate count.
//   mcloud_emit_kernel     one thread per candidate: its row (a binary search in the exclusive scan of the candidates per row), its
//                          position, its triangle, its 63-bit cell index and the bits of its squared distance to the cell centre.
//   mcloud_winners_kernel  after a stable sort of the cell indices (the caller's): one thread per sorted position; the head of a run of
//                          equal cells walks its run and marks the candidate of the smallest (distance bits, candidate number).
//   mcloud_compact_kernel  one thread per candidate: a marked one goes to the slot the inclusive scan of the marks names.
//
// The scans and the sort between the kernels are the caller's (ops.mesh_cloud uses torch.cumsum and a stable torch.sort).  No loop waits
// for another lane: every trip count is a function of the thread's own data (rows of its triangle, log2 of a table, length of its run).
// No floating-point atomics: the result is bit-identical from run to run.  Compiled with -ffp-contract=off, and the shared statements
// switch contraction off for themselves.
#include "psi_common.h"
#include "mesh_cloud_shared.h"

namespace psi_mcloud {

constexpr int WG = 256;
constexpr int WAVES = WG / PSI_WAVE;
constexpr int COUNT_BLOCKS = 1024;

struct State {                       // written by mcloud_init_kernel, then by the atomics of mcloud_count_kernel
    unsigned long long rows, cands;  // totals over the triangles
    unsigned flags;                  // Flag bits
    unsigned minb[3], maxb[3];       // box of the referenced vertices, order-preserving bits
    unsigned pad[3];
};

// float -> unsigned whose order is the order of the floats (finite values)
__host__ __device__ __forceinline__ unsigned ordered_bits(float f)
{
    union { float f; unsigned u; } b;
    b.f = f;
    return (b.u & 0x80000000u) ? ~b.u : (b.u | 0x80000000u);
}

__host__ __device__ __forceinline__ float ordered_float(unsigned u)
{
    union { float f; unsigned u; } b;
    b.u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    return b.f;
}

__global__ void mcloud_init_kernel(State *st)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        st->rows = 0;
        st->cands = 0;
        st->flags = 0;
        for (int k = 0; k < 3; k++) {
            st->minb[k] = 0xffffffffu;
            st->maxb[k] = 0u;
        }
    }
}

__device__ __forceinline__ bool load_tri(const float *__restrict__ verts, const int32_t *__restrict__ faces, int nv, long t, float p[3][3],
                                         unsigned *flags)
{
    const int i0 = faces[t * 3 + 0], i1 = faces[t * 3 + 1], i2 = faces[t * 3 + 2];
    if (i0 < 0 || i0 >= nv || i1 < 0 || i1 >= nv || i2 < 0 || i2 >= nv) {
        *flags |= BAD_INDEX;
        return false;
    }
    const int idx[3] = {i0, i1, i2};
    bool finite = true;
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            p[c][k] = verts[(size_t)idx[c] * 3 + k];
            finite &= isfinite(p[c][k]);
        }
    if (!finite) *flags |= NOT_FINITE;
    return finite;
}

__global__ __launch_bounds__(WG) void mcloud_count_kernel(const float *__restrict__ verts, const int32_t *__restrict__ faces, int nv, int nf,
                                                          float h, int32_t *__restrict__ tri_rows, State *__restrict__ st)
{
    const int lane = threadIdx.x & (PSI_WAVE - 1);
    const long wave = (long)blockIdx.x * WAVES + threadIdx.x / PSI_WAVE;
    const long nwaves = (long)gridDim.x * WAVES;
    unsigned long long rows = 0, cands = 0;       // wave-uniform after the reduction of each triangle
    unsigned flags = 0, minb[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, maxb[3] = {0u, 0u, 0u};
    for (long t = wave; t < nf; t += nwaves) {    // the same triangle in every lane of the wave
        float p[3][3];
        int nr = 0;
        if (load_tri(verts, faces, nv, t, p, &flags)) {
#pragma unroll
            for (int c = 0; c < 3; c++)
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const unsigned ob = ordered_bits(p[c][k]);
                    minb[k] = ob < minb[k] ? ob : minb[k];
                    maxb[k] = ob > maxb[k] ? ob : maxb[k];
                }
            bool too_long;
            const Tri tr = tri_setup(p[0], p[1], p[2], h, &too_long);
            if (too_long) flags |= TOO_LONG;
            nr = rows_of(tr);
            unsigned long long n = 0;
            for (int r = lane; r < nr; r += PSI_WAVE) n += (unsigned long long)row_candidates(tr, r, h);
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) n += __shfl_xor(n, off);
            rows += (unsigned long long)nr;
            cands += n;
        }
        if (lane == 0) tri_rows[t] = nr;
    }
    if (lane != 0) return;
    if (rows) atomicAdd(&st->rows, rows);
    if (cands) atomicAdd(&st->cands, cands);
    if (flags) atomicOr(&st->flags, flags);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (minb[k] != 0xffffffffu) atomicMin(&st->minb[k], minb[k]);
        if (maxb[k] != 0u) atomicMax(&st->maxb[k], maxb[k]);
    }
}

// the last index i of [0, n) with off[i] <= x (off ascending, off[0] = 0 <= x): at most 64 steps
__device__ __forceinline__ long last_not_above(const int64_t *__restrict__ off, long n, int64_t x)
{
    long lo = 0, hi = n - 1;
    while (lo < hi) {
        const long mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ Tri checked_tri(const float *__restrict__ verts, const int32_t *__restrict__ faces, int nv, long t, float h)
{
    float p[3][3];          // the count pass has accepted every index of this mesh: the clamp only guards the address
#pragma unroll
    for (int c = 0; c < 3; c++) {
        int i = faces[t * 3 + c];
        i = i < 0 ? 0 : (i >= nv ? nv - 1 : i);
#pragma unroll
        for (int k = 0; k < 3; k++) p[c][k] = verts[(size_t)i * 3 + k];
    }
    bool too_long;
    return tri_setup(p[0], p[1], p[2], h, &too_long);
}

__global__ __launch_bounds__(WG) void mcloud_rows_kernel(const float *__restrict__ verts, const int32_t *__restrict__ faces, int nv, int nf, float h,
                                                         const int64_t *__restrict__ tri_row_off, long n_rows, int32_t *__restrict__ row_tri,
                                                         int32_t *__restrict__ row_cnt)
{
    const long g = (long)blockIdx.x * WG + threadIdx.x;
    if (g >= n_rows) return;
    const long t = last_not_above(tri_row_off, nf, g);
    const Tri tr = checked_tri(verts, faces, nv, t, h);
    const int r = (int)(g - tri_row_off[t]);
    row_tri[g] = (int32_t)t;
    row_cnt[g] = r < rows_of(tr) ? row_candidates(tr, r, h) : 0;      // r < rows by construction of the scan; the guard is for the table
}

struct Origin {
    float o[3];
};

__global__ __launch_bounds__(WG) void mcloud_emit_kernel(const float *__restrict__ verts, const int32_t *__restrict__ faces, int nv, int nf, float h, float v,
                                                         Origin org, const int64_t *__restrict__ tri_row_off,
                                                         const int32_t *__restrict__ row_tri, const int64_t *__restrict__ row_off, long n_rows,
                                                         long n_cands, float *__restrict__ pos, int32_t *__restrict__ tri,
                                                         int64_t *__restrict__ cell, uint32_t *__restrict__ key)
{
    const long q = (long)blockIdx.x * WG + threadIdx.x;
    if (q >= n_cands) return;
    const long g = last_not_above(row_off, n_rows, q);
    long t = row_tri[g];
    t = t < 0 ? 0 : (t >= nf ? nf - 1 : t);      // row_tri is the table of the rows pass: the clamp only guards the address
    const Tri tr = checked_tri(verts, faces, nv, t, h);
    const int r = (int)(g - tri_row_off[t]);
    int j = (int)(q - row_off[g]);
    const int nj = row_candidates(tr, r, h);
    j = j < nj ? j : nj - 1;              // cannot bind when row_off is the scan of the rows pass (a guard, not a rule)
    float p[3];
    row_point(tr, r, j, h, p);
    int64_t c;
    uint32_t k;
    cell_key(p, org.o, v, &c, &k);
    pos[q * 3 + 0] = p[0];
    pos[q * 3 + 1] = p[1];
    pos[q * 3 + 2] = p[2];
    tri[q] = (int32_t)t;
    cell[q] = c;
    key[q] = k;
}

__global__ __launch_bounds__(WG) void mcloud_winners_kernel(const int64_t *__restrict__ cell_sorted, const int64_t *__restrict__ perm,
                                                            const uint32_t *__restrict__ key, long n, int32_t *__restrict__ keep)
{
    const long i = (long)blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const int64_t c = cell_sorted[i];
    if (i > 0 && cell_sorted[i - 1] == c) return;       // not the head of its run
    int64_t best = perm[i];
    if (best < 0 || best >= n) return;                  // not a permutation: nothing is marked
    uint32_t bk = key[best];
    for (long j = i + 1; j < n && cell_sorted[j] == c; j++) {
        const int64_t cand = perm[j];
        if (cand < 0 || cand >= n) continue;
        const uint32_t k = key[cand];
        if (k < bk || (k == bk && cand < best)) {       // the sort is stable, so `cand < best` never decides; it makes the rule explicit
            bk = k;
            best = cand;
        }
    }
    keep[best] = 1;
}

__global__ __launch_bounds__(WG) void mcloud_compact_kernel(const float *__restrict__ pos, const int32_t *__restrict__ tri,
                                                            const int32_t *__restrict__ keep, const int64_t *__restrict__ keep_scan, long n,
                                                            long n_out, float *__restrict__ points, int32_t *__restrict__ out_tri)
{
    const long q = (long)blockIdx.x * WG + threadIdx.x;
    if (q >= n || !keep[q]) return;
    const int64_t o = keep_scan[q] - 1;                 // inclusive scan of the marks
    if (o < 0 || o >= n_out) return;
    points[o * 3 + 0] = pos[q * 3 + 0];
    points[o * 3 + 1] = pos[q * 3 + 1];
    points[o * 3 + 2] = pos[q * 3 + 2];
    out_tri[o] = tri[q];
}

static int check_spacing(float spacing)
{
    PSI_REQUIRE(std::isfinite(spacing) && spacing > 0.0f && half_spacing(spacing) > 0.0f, "spacing must be a positive finite fp32 number");
    return 0;
}

static int grid_for(long n, unsigned *blocks)
{
    const long b = (n + WG - 1) / WG;
    PSI_REQUIRE(b >= 1 && b < (1l << 31), "1 <= workgroups < 2^31");
    *blocks = (unsigned)b;
    return 0;
}

}   // namespace psi_mcloud

extern "C" int psi_mesh_cloud_count(const float *d_verts, const int32_t *d_faces, int nv, int nf, float spacing, int32_t *d_tri_rows,
                                    float origin[3], long long *n_rows, long long *n_cands, void *stream)
{
    using namespace psi_mcloud;
    PSI_REQUIRE(d_verts && d_faces && d_tri_rows && origin && n_rows && n_cands, "null pointer");
    *n_rows = 0;
    *n_cands = 0;
    if (int rc = check_spacing(spacing)) return rc;
    PSI_REQUIRE(nf >= 1 && nv >= 1, "nf >= 1 and nv >= 1");
    hipStream_t st = (hipStream_t)stream;
    State *d_state = (State *)psi_scratch(sizeof(State), st);
    if (!d_state) {
        psi_set_error("psi_mesh_cloud_count: no workspace");
        return PSI_ENOMEM;
    }
    const float h = half_spacing(spacing);
    hipLaunchKernelGGL(mcloud_init_kernel, dim3(1), dim3(PSI_WAVE), 0, st, d_state);
    PSI_CHECK_LAUNCH("mcloud_init_kernel");
    const int blocks = std::min(COUNT_BLOCKS, psi_cdiv(nf, WAVES));
    hipLaunchKernelGGL(mcloud_count_kernel, dim3(blocks), dim3(WG), 0, st, d_verts, d_faces, nv, nf, h, d_tri_rows, d_state);
    PSI_CHECK_LAUNCH("mcloud_count_kernel");
    State hs;
    PSI_CHECK_HIP(hipMemcpyAsync(&hs, d_state, sizeof(State), hipMemcpyDeviceToHost, st));
    PSI_CHECK_HIP(hipStreamSynchronize(st));
    PSI_REQUIRE(!(hs.flags & BAD_INDEX), "a face index lies outside [0, nv)");
    PSI_REQUIRE(!(hs.flags & NOT_FINITE), "a vertex coordinate of a triangle is not finite");
    PSI_REQUIRE(!(hs.flags & TOO_LONG), "an edge spans more than 2^21 cells");
    for (int k = 0; k < 3; k++) {
        const float lo = ordered_float(hs.minb[k]), hi = ordered_float(hs.maxb[k]);
        PSI_REQUIRE(cells_along(lo, hi, h, spacing) <= (float)MAX_CELLS, "more than 2^21 cells along an axis");
        origin[k] = cell_origin(lo, h);
        PSI_REQUIRE(std::isfinite(origin[k]), "the origin of the cells is not finite");
    }
    *n_rows = (long long)hs.rows;
    *n_cands = (long long)hs.cands;
    PSI_REQUIRE(hs.cands >= 1, "no triangle with area");
    if (hs.cands > (unsigned long long)MAX_CANDIDATES) {
        psi_set_error("invalid argument: %llu candidates at spacing %g exceed 2^31 - 1", hs.cands, (double)spacing);
        return PSI_EINVAL;
    }
    return 0;
}

extern "C" int psi_mesh_cloud_rows(const float *d_verts, const int32_t *d_faces, int nv, int nf, float spacing, const int64_t *d_tri_row_off,
                                   long long n_rows, int32_t *d_row_tri, int32_t *d_row_cnt, void *stream)
{
    using namespace psi_mcloud;
    PSI_REQUIRE(d_verts && d_faces && d_tri_row_off && d_row_tri && d_row_cnt, "null pointer");
    if (int rc = check_spacing(spacing)) return rc;
    PSI_REQUIRE(nv >= 1 && nf >= 1 && n_rows >= 1 && n_rows <= MAX_CANDIDATES, "nv, nf >= 1 and 1 <= n_rows < 2^31");
    unsigned blocks;
    if (int rc = grid_for(n_rows, &blocks)) return rc;
    hipLaunchKernelGGL(mcloud_rows_kernel, dim3(blocks), dim3(WG), 0, (hipStream_t)stream, d_verts, d_faces, nv, nf, half_spacing(spacing),
                       d_tri_row_off, (long)n_rows, d_row_tri, d_row_cnt);
    PSI_CHECK_LAUNCH("mcloud_rows_kernel");
    return 0;
}

extern "C" int psi_mesh_cloud_emit(const float *d_verts, const int32_t *d_faces, int nv, int nf, float spacing, const float origin[3],
                                   const int64_t *d_tri_row_off, const int32_t *d_row_tri, const int64_t *d_row_off, long long n_rows,
                                   long long n_cands, float *d_pos, int32_t *d_tri, int64_t *d_cell, uint32_t *d_key, void *stream)
{
    using namespace psi_mcloud;
    PSI_REQUIRE(d_verts && d_faces && origin && d_tri_row_off && d_row_tri && d_row_off && d_pos && d_tri && d_cell && d_key, "null pointer");
    if (int rc = check_spacing(spacing)) return rc;
    PSI_REQUIRE(nv >= 1 && nf >= 1, "nv, nf >= 1");
    PSI_REQUIRE(n_rows >= 1 && n_cands >= n_rows && n_cands <= MAX_CANDIDATES, "1 <= n_rows <= n_cands < 2^31");
    Origin org;
    for (int k = 0; k < 3; k++) {
        PSI_REQUIRE(std::isfinite(origin[k]), "the origin of the cells is not finite");
        org.o[k] = origin[k];
    }
    unsigned blocks;
    if (int rc = grid_for(n_cands, &blocks)) return rc;
    hipLaunchKernelGGL(mcloud_emit_kernel, dim3(blocks), dim3(WG), 0, (hipStream_t)stream, d_verts, d_faces, nv, nf, half_spacing(spacing), spacing, org,
                       d_tri_row_off, d_row_tri, d_row_off, (long)n_rows, (long)n_cands, d_pos, d_tri, d_cell, d_key);
    PSI_CHECK_LAUNCH("mcloud_emit_kernel");
    return 0;
}

extern "C" int psi_mesh_cloud_winners(const int64_t *d_cell_sorted, const int64_t *d_perm, const uint32_t *d_key, long long n, int32_t *d_keep,
                                      void *stream)
{
    using namespace psi_mcloud;
    PSI_REQUIRE(d_cell_sorted && d_perm && d_key && d_keep, "null pointer");
    PSI_REQUIRE(n >= 1 && n <= MAX_CANDIDATES, "1 <= n < 2^31");
    unsigned blocks;
    if (int rc = grid_for(n, &blocks)) return rc;
    PSI_CHECK_HIP(hipMemsetAsync(d_keep, 0, (size_t)n * sizeof(int32_t), (hipStream_t)stream));
    hipLaunchKernelGGL(mcloud_winners_kernel, dim3(blocks), dim3(WG), 0, (hipStream_t)stream, d_cell_sorted, d_perm, d_key, (long)n, d_keep);
    PSI_CHECK_LAUNCH("mcloud_winners_kernel");
    return 0;
}

extern "C" int psi_mesh_cloud_compact(const float *d_pos, const int32_t *d_tri, const int32_t *d_keep, const int64_t *d_keep_scan, long long n,
                                      long long n_out, float *d_points, int32_t *d_out_tri, void *stream)
{
    using namespace psi_mcloud;
    PSI_REQUIRE(d_pos && d_tri && d_keep && d_keep_scan && d_points && d_out_tri, "null pointer");
    PSI_REQUIRE(n >= 1 && n <= MAX_CANDIDATES && n_out >= 1 && n_out <= n, "1 <= n_out <= n < 2^31");
    unsigned blocks;
    if (int rc = grid_for(n, &blocks)) return rc;
    hipLaunchKernelGGL(mcloud_compact_kernel, dim3(blocks), dim3(WG), 0, (hipStream_t)stream, d_pos, d_tri, d_keep, d_keep_scan, (long)n,
                       (long)n_out, d_points, d_out_tri);
    PSI_CHECK_LAUNCH("mcloud_compact_kernel");
    return 0;
}
