// Body against body: which vertices of one body of a batch lie inside another body of the batch, for gfx950 (wave64).  The contract is
// DESIGN.md "Body against body"; the per-triple statements are csrc/body_overlap_shared.h and csrc/geom_shared.h (boxes, normal, half_omega),
// the workgroup sum, box and the ordered emit pass (wg_emit, which the crossing searches use too) csrc/wg_device.h.
//
//   box        of body j: the exact min / max of its V vertices per axis
//   candidate  an ordered triple (i, j, v), i != j, group[i] == group[j], vertex v of body i inside the closed box of j; ascending (i, j, v)
//   w          (sum over the F triangles of body j, in face order, of half_omega(A, B, C, n; p)) / 2 pi, n = (B - A) x (C - A) in fp32 from the
//              body's current vertices: about 1 inside an outward-wound surface, about 0 outside
//   sum        fp32 within a chunk of 256 consecutive faces; the chunk sums added in fp64, in order, within a slice of 2048 consecutive faces;
//              the slice sums added in fp64 in slice order.  No floating-point atomics
//   decision   vertex v of body i is inside j iff w > 0.5
//
// Passes: boxes (one workgroup per body), count (one workgroup per ordered pair; a pair whose boxes do not meet costs one comparison), emit
// (the triples and the table of 256-candidate chunks, offsets from the caller's scans), wind (grid = candidate chunk x face slice: a chunk's
// candidates belong to ONE pair, so all lanes stage the same body j; per 256 faces every lane builds one triangle record in LDS, then every
// lane reads every record: identical addresses broadcast), decide (the slice sums in order, w, integer atomics into counts and the bit mask).
#include "body_overlap_shared.h"
#include "blob.h"
#include "wg_device.h"
#include <limits.h>

namespace psi_bo {

constexpr int WG = WG_LANES;
static_assert(WG == BO_CHUNK, "one staged record per lane");

struct Chunk { int first, n, i, j; };          // 256-candidate chunk: first candidate, candidates, the pair
static_assert(sizeof(Chunk) == 16, "the chunk table is [n_chunks,4] int32");

// boxes [B,6] = min xyz, max xyz; *bad = the smallest body index with a non-finite coordinate (INT_MAX: none)
__global__ __launch_bounds__(WG) void bo_box_kernel(const float *__restrict__ verts, int V, float *__restrict__ boxes, int *__restrict__ bad)
{
    wg_body_box(verts, V, boxes, bad);
}

// Is (i, j) a pair that is compared, and do its boxes meet?  Loads box j into lo / hi.
__device__ __forceinline__ bool pair_live(const float *__restrict__ boxes, const int *__restrict__ group, int i, int j, float lo[3], float hi[3])
{
    if (i == j) return false;
    if (group && group[i] != group[j]) return false;
    float ilo[3], ihi[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        ilo[a] = boxes[(size_t)i * 6 + a];
        ihi[a] = boxes[(size_t)i * 6 + 3 + a];
        lo[a] = boxes[(size_t)j * 6 + a];
        hi[a] = boxes[(size_t)j * 6 + 3 + a];
    }
    return geom_boxes_meet(ilo, ihi, lo, hi);
}

// pair_count [B,B]: the vertices of body i inside the closed box of body j (0 for a pair that is not compared); every entry is written
__global__ __launch_bounds__(WG) void bo_count_kernel(const float *__restrict__ verts, const float *__restrict__ boxes, const int *__restrict__ group,
                                                      int B, int V, int *__restrict__ pair_count)
{
    __shared__ int s_w[WG / 64];
    const int i = blockIdx.x / B, j = blockIdx.x % B, t = threadIdx.x;
    float lo[3], hi[3];
    if (!pair_live(boxes, group, i, j, lo, hi)) {           // the same in every lane
        if (t == 0) pair_count[blockIdx.x] = 0;
        return;
    }
    const float *v = verts + (size_t)i * V * 3;
    int n = 0;
    for (int k = t; k < V; k += WG) n += geom_in_box(v[(size_t)k * 3], v[(size_t)k * 3 + 1], v[(size_t)k * 3 + 2], lo, hi) ? 1 : 0;
    n = wg_sum(n, s_w);
    if (t == 0) pair_count[blockIdx.x] = n;
}

// cand [n_cand,3] = (i, j, v) ascending; chunks [n_chunks] of up to 256 candidates of one pair.  cand_off / chunk_off [B,B] int64: the
// exclusive scans of pair_count and of ceil(pair_count / 256).
__global__ __launch_bounds__(WG) void bo_emit_kernel(const float *__restrict__ verts, const float *__restrict__ boxes, const int *__restrict__ group,
                                                     int B, int V, const int *__restrict__ pair_count, const long long *__restrict__ cand_off,
                                                     const long long *__restrict__ chunk_off, long long n_cand, long long n_chunks,
                                                     int *__restrict__ cand, Chunk *__restrict__ chunks)
{
    __shared__ int s_wcnt[WG / 64];
    const int pc = pair_count[blockIdx.x];
    if (pc == 0) return;
    const int i = blockIdx.x / B, j = blockIdx.x % B, t = threadIdx.x;
    float lo[3], hi[3];
    if (!pair_live(boxes, group, i, j, lo, hi)) return;
    const long long off = cand_off[blockIdx.x], coff = chunk_off[blockIdx.x];
    for (int c = t; c * BO_CHUNK < pc; c += WG)
        if (coff + c < n_chunks) chunks[coff + c] = Chunk{(int)(off + (long long)c * BO_CHUNK), min(BO_CHUNK, pc - c * BO_CHUNK), i, j};
    const float *v = verts + (size_t)i * V * 3;
    wg_emit(V, pc, off, n_cand, s_wcnt, [&](int k) { return geom_in_box(v[(size_t)k * 3], v[(size_t)k * 3 + 1], v[(size_t)k * 3 + 2], lo, hi); },
            [&](long long pos, int k) {                     // vertex k at its place among the pair's candidates
                cand[pos * 3] = i;
                cand[pos * 3 + 1] = j;
                cand[pos * 3 + 2] = k;
            });
}

// part [n_slices, n_cand] fp64: the slice sums of every candidate.  grid = (chunk, slice).
__global__ __launch_bounds__(WG) void bo_wind_kernel(const float *__restrict__ verts, const int32_t *__restrict__ faces, int V, int F,
                                                     const int *__restrict__ cand, long long n_cand, const Chunk *__restrict__ chunks,
                                                     double *__restrict__ part)
{
    __shared__ float4 stage[WG * 3];           // 12 KB: 256 triangle records (A, B, C, n)
    const int t = threadIdx.x, slice = blockIdx.y;
    const Chunk ch = chunks[blockIdx.x];
    const bool live = t < ch.n;
    const long long ci = (long long)ch.first + t;
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (live) {
        const float *p = verts + ((size_t)ch.i * V + cand[ci * 3 + 2]) * 3;
        px = p[0], py = p[1], pz = p[2];
    }
    const float *vj = verts + (size_t)ch.j * V * 3;
    const int f_end = min(F, (slice + 1) * BO_SLICE);
    double acc = 0.0;
    for (int f0 = slice * BO_SLICE; f0 < f_end; f0 += BO_CHUNK) {
        const int nst = min(BO_CHUNK, f_end - f0);
        if (t < nst) {
            const int32_t *f = faces + (size_t)(f0 + t) * 3;
            const float *a = vj + (size_t)f[0] * 3, *b = vj + (size_t)f[1] * 3, *c = vj + (size_t)f[2] * 3;
            const float A[3] = {a[0], a[1], a[2]}, Bv[3] = {b[0], b[1], b[2]}, C[3] = {c[0], c[1], c[2]};
            float n[3];
            geom_normal(A, Bv, C, n);
            stage[3 * t] = make_float4(A[0], A[1], A[2], Bv[0]);
            stage[3 * t + 1] = make_float4(Bv[1], Bv[2], C[0], C[1]);
            stage[3 * t + 2] = make_float4(C[2], n[0], n[1], n[2]);
        }
        __syncthreads();
        if (live) {
            float s = 0.0f;
            for (int k = 0; k < nst; k++) {
                const float4 r0 = stage[3 * k], r1 = stage[3 * k + 1], r2 = stage[3 * k + 2];
                s += geom_half_omega(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, px, py, pz);
            }
            acc += (double)s;
        }
        __syncthreads();
    }
    if (live) part[(size_t)slice * n_cand + ci] = acc;
}

// w [n_cand]; counts [B,B] and mask [B, ceil(V / 32)] (both zeroed by the caller) by integer atomics, which commute
__global__ __launch_bounds__(WG) void bo_decide_kernel(const int *__restrict__ cand, long long n_cand, const double *__restrict__ part, int n_slices,
                                                       int B, int mask_words, float *__restrict__ w, int *__restrict__ counts,
                                                       unsigned int *__restrict__ mask)
{
    const long long c = (long long)blockIdx.x * WG + threadIdx.x;
    if (c >= n_cand) return;
    double s = 0.0;
    for (int k = 0; k < n_slices; k++) s += part[(size_t)k * n_cand + c];
    const float wv = bo_w_of_sum(s);
    w[c] = wv;
    if (bo_inside(wv)) {
        const int i = cand[c * 3], j = cand[c * 3 + 1], v = cand[c * 3 + 2];
        atomicAdd(counts + (size_t)i * B + j, 1);
        atomicOr(mask + (size_t)i * mask_words + (v >> 5), 1u << (v & 31));
    }
}

}  // namespace psi_bo

extern "C" int psi_body_overlap_create(psi_body_overlap **out, const int32_t *h_faces, int V, int F)
{
    PSI_REQUIRE(out && h_faces, "null pointer");
    PSI_REQUIRE(V >= 1 && F >= 1, "V >= 1 and F >= 1");
    PSI_REQUIRE((long long)F * 3 < (1ll << 31), "F * 3 < 2^31");
    int rc = psi_check_faces(h_faces, V, F);
    if (rc) return rc;
    psi_body_overlap *h = new psi_body_overlap{nullptr, nullptr, V, F};
    PsiBlob T;
    T.upload(h->d_faces, h_faces, (size_t)F * 3 * sizeof(int32_t));
    if (int e = psi_blob_realise(T, &h->blob, "psi_body_overlap_create")) {
        delete h;
        return e;
    }
    *out = h;
    return 0;
}

extern "C" void psi_body_overlap_destroy(psi_body_overlap *h)
{
    if (!h) return;
    (void)hipFree(h->blob);
    delete h;
}

extern "C" int psi_body_overlap_info(const psi_body_overlap *h, int32_t info[2])
{
    PSI_REQUIRE(h && info, "null pointer");
    info[0] = h->V;
    info[1] = h->F;
    return 0;
}

extern "C" size_t psi_body_overlap_workspace_bytes(long long n_cand, int F)
{
    if (n_cand < 1 || n_cand >= (1ll << 31) || F < 1) return 0;
    return (size_t)bo_slices(F) * (size_t)n_cand * sizeof(double);
}

extern "C" int psi_body_overlap_boxes(const psi_body_overlap *h, const float *d_verts, int B, float *d_boxes, int32_t *d_bad, void *stream)
{
    PSI_REQUIRE(h && d_verts && d_boxes && d_bad, "null pointer");
    PSI_REQUIRE(B >= 1 && B <= GEOM_MAX_B, "1 <= B <= 46340");
    hipStream_t st = (hipStream_t)stream;
    PSI_CHECK_HIP(psi_reset_bad_flag(d_bad, st));
    hipLaunchKernelGGL(psi_bo::bo_box_kernel, dim3(B), dim3(psi_bo::WG), 0, st, d_verts, h->V, d_boxes, d_bad);
    PSI_CHECK_LAUNCH("bo_box_kernel");
    return 0;
}

extern "C" int psi_body_overlap_count(const psi_body_overlap *h, const float *d_verts, const int32_t *d_group, int B, const float *d_boxes,
                                      int32_t *d_pair_count, void *stream)
{
    PSI_REQUIRE(h && d_verts && d_boxes && d_pair_count, "null pointer");
    PSI_REQUIRE(B >= 1 && B <= GEOM_MAX_B, "1 <= B <= 46340");
    hipLaunchKernelGGL(psi_bo::bo_count_kernel, dim3(B * B), dim3(psi_bo::WG), 0, (hipStream_t)stream, d_verts, d_boxes, d_group, B, h->V,
                       d_pair_count);
    PSI_CHECK_LAUNCH("bo_count_kernel");
    return 0;
}

extern "C" int psi_body_overlap_emit(const psi_body_overlap *h, const float *d_verts, const int32_t *d_group, int B, const float *d_boxes,
                                     const int32_t *d_pair_count, const int64_t *d_cand_off, const int64_t *d_chunk_off, long long n_cand,
                                     long long n_chunks, int32_t *d_cand, int32_t *d_chunks, void *stream)
{
    PSI_REQUIRE(h && d_verts && d_boxes && d_pair_count && d_cand_off && d_chunk_off && d_cand && d_chunks, "null pointer");
    PSI_REQUIRE(B >= 1 && B <= GEOM_MAX_B, "1 <= B <= 46340");
    PSI_REQUIRE(n_cand >= 1 && n_cand < (1ll << 31), "1 <= n_cand < 2^31");
    PSI_REQUIRE(n_chunks >= 1 && n_chunks <= n_cand, "1 <= n_chunks <= n_cand");
    hipLaunchKernelGGL(psi_bo::bo_emit_kernel, dim3(B * B), dim3(psi_bo::WG), 0, (hipStream_t)stream, d_verts, d_boxes, d_group, B, h->V,
                       d_pair_count, (const long long *)d_cand_off, (const long long *)d_chunk_off, n_cand, n_chunks, d_cand,
                       (psi_bo::Chunk *)d_chunks);
    PSI_CHECK_LAUNCH("bo_emit_kernel");
    return 0;
}

extern "C" int psi_body_overlap_wind(const psi_body_overlap *h, const float *d_verts, int B, const int32_t *d_cand, long long n_cand,
                                     const int32_t *d_chunks, long long n_chunks, void *d_workspace, size_t workspace_bytes, void *stream)
{
    PSI_REQUIRE(h && d_verts && d_cand && d_chunks && d_workspace, "null pointer");
    PSI_REQUIRE(B >= 1 && B <= GEOM_MAX_B, "1 <= B <= 46340");
    PSI_REQUIRE(n_cand >= 1 && n_cand < (1ll << 31), "1 <= n_cand < 2^31");
    PSI_REQUIRE(n_chunks >= 1 && n_chunks <= n_cand, "1 <= n_chunks <= n_cand");
    PSI_REQUIRE(workspace_bytes >= psi_body_overlap_workspace_bytes(n_cand, h->F), "workspace too small");
    hipLaunchKernelGGL(psi_bo::bo_wind_kernel, dim3((unsigned)n_chunks, bo_slices(h->F)), dim3(psi_bo::WG), 0, (hipStream_t)stream, d_verts,
                       h->d_faces, h->V, h->F, d_cand, n_cand, (const psi_bo::Chunk *)d_chunks, (double *)d_workspace);
    PSI_CHECK_LAUNCH("bo_wind_kernel");
    return 0;
}

extern "C" int psi_body_overlap_decide(const psi_body_overlap *h, int B, const int32_t *d_cand, long long n_cand, const void *d_workspace,
                                       size_t workspace_bytes, float *d_w, int32_t *d_counts, uint32_t *d_mask, void *stream)
{
    PSI_REQUIRE(h && d_cand && d_workspace && d_w && d_counts && d_mask, "null pointer");
    PSI_REQUIRE(B >= 1 && B <= GEOM_MAX_B, "1 <= B <= 46340");
    PSI_REQUIRE(n_cand >= 1 && n_cand < (1ll << 31), "1 <= n_cand < 2^31");
    PSI_REQUIRE(workspace_bytes >= psi_body_overlap_workspace_bytes(n_cand, h->F), "workspace too small");
    hipLaunchKernelGGL(psi_bo::bo_decide_kernel, dim3(psi_cdiv(n_cand, psi_bo::WG)), dim3(psi_bo::WG), 0, (hipStream_t)stream, d_cand, n_cand,
                       (const double *)d_workspace, bo_slices(h->F), B, (h->V + 31) / 32, d_w, d_counts, d_mask);
    PSI_CHECK_LAUNCH("bo_decide_kernel");
    return 0;
}
