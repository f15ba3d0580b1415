// Surface crossings: which pairs of triangles of the posed body surfaces of a batch properly intersect, for gfx950 (wave64).  The contract is
// DESIGN.md section 10e; the per-pair statements and the Morton order of the faces are csrc/surface_crossings_shared.h, the closed-box test
// csrc/geom_shared.h, the workgroup sum, box and the two passes of a count-or-emit job csrc/wg_device.h, the argument rules of the
// count-or-emit entry points and the launch of a test kernel's two forms, as in the scene search, csrc/crossings_common.h.  Compiled with
// -ffp-contract=off.
//
//   candidate  an unordered pair of faces ((i, s), (j, t)), (i, s) < (j, t): bodies i < j of one group (between), or two faces s < t of one
//              body that share no vertex index and whose parts are not skipped (self); and the closed face boxes meet
//   decision   the pair crosses iff at least one edge of one triangle pierces the other (sc_pair); events == 2 is the regular case
//
// The handle keeps the faces in chunks of 256, in face order or along a Morton curve of a representative pose; results are reported in the
// caller's face indices.  Passes: boxes (chunk boxes, body boxes, the non-finite flag), tile_count / tile_emit (a job is a pair of bodies
// i <= j, a tile a pair of chunks of a job whose boxes meet; offsets from the caller's scan), test (the hot pass: one workgroup per tile;
// every lane keeps one triangle of chunk ca in registers, the 256 records of chunk cb are staged in LDS and read by all lanes at the same
// address, which broadcasts; once to count the crossing pairs of a tile, once to emit key, events and length), finish (after the caller's
// sort of the keys: pairs, counts, face mask and irregular count by integer atomics) and contour (one workgroup per job adds the lengths
// of its pairs in fp64, sequentially in pair order).  No floating-point atomics.
#include "surface_crossings_shared.h"
#include "crossings_common.h"
#include "surface_crossings_handle.h"
#include "blob.h"
#include <limits.h>

namespace psi_sc {

constexpr int WG = WG_LANES;
static_assert(WG == SC_CHUNK, "one staged record per lane");

struct Tile { int i, j, ca, cb; };
static_assert(sizeof(Tile) == 16, "the tile table is [n_tiles,4] int32");

__device__ __forceinline__ void load_triangle(const float *__restrict__ v, const int32_t *__restrict__ f, int id[3], float p[3][3])
{
#pragma unroll
    for (int k = 0; k < 3; k++) {
        id[k] = f[k];
#pragma unroll
        for (int a = 0; a < 3; a++) p[k][a] = v[(size_t)id[k] * 3 + a];
    }
}

// chunk_boxes [B, n_chunks, 6] = min xyz, max xyz of the faces of a chunk; grid = (chunk, body)
__global__ __launch_bounds__(WG) void sc_chunk_box_kernel(const float *__restrict__ verts, const int32_t *__restrict__ faces, int V, int F,
                                                          float *__restrict__ chunk_boxes)
{
    __shared__ float s_lo[WG / 64][3], s_hi[WG / 64][3];
    const int c = blockIdx.x, b = blockIdx.y, pos = c * SC_CHUNK + threadIdx.x;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (pos < F) {
        int id[3];
        float p[3][3];
        load_triangle(verts + (size_t)b * V * 3, faces + (size_t)pos * 3, id, p);
        sc_face_box(p, lo, hi);
    }
    wg_box(lo, hi, s_lo, s_hi, chunk_boxes + ((size_t)b * gridDim.x + c) * 6);
}

// body_boxes [B,6] over the V vertices of a body (a superset of its chunk boxes); *bad = the smallest body index with a non-finite
// coordinate.  One workgroup per body.
__global__ __launch_bounds__(WG) void sc_body_box_kernel(const float *__restrict__ verts, int V, float *__restrict__ body_boxes, int *__restrict__ bad)
{
    wg_body_box(verts, V, body_boxes, bad);
}

// Is (i, j) a job: admitted by the flags and the groups, and (unless brute) with meeting body boxes?
__device__ __forceinline__ bool job_live(const float *__restrict__ body_boxes, const int *__restrict__ group, int flags, int i, int j)
{
    if (i > j) return false;
    if (i == j ? !(flags & SC_SELF) : !(flags & SC_BETWEEN)) return false;
    if (i != j && group && group[i] != group[j]) return false;
    if (flags & SC_BRUTE) return true;
    return geom_boxes_meet(body_boxes + (size_t)i * 6, body_boxes + (size_t)i * 6 + 3, body_boxes + (size_t)j * 6, body_boxes + (size_t)j * 6 + 3);
}

__device__ __forceinline__ bool tile_live(const float *__restrict__ chunk_boxes, int nC, int flags, int i, int j, int ca, int cb)
{
    if (i == j && ca > cb) return false;
    if (flags & SC_BRUTE) return true;
    const float *a = chunk_boxes + ((size_t)i * nC + ca) * 6, *b = chunk_boxes + ((size_t)j * nC + cb) * 6;
    return geom_boxes_meet(a, a + 3, b, b + 3);
}

// job_tiles [B,B]: the tiles of job (i, j); every entry is written.  With tiles != null (the emit pass) the tiles are written from
// job_off[i,j] on, in ascending (ca, cb) order.
__global__ __launch_bounds__(WG) void sc_tile_kernel(const float *__restrict__ chunk_boxes, const float *__restrict__ body_boxes,
                                                     const int *__restrict__ group, int B, int nC, int flags, int *__restrict__ job_tiles,
                                                     const long long *__restrict__ job_off, long long n_tiles, Tile *__restrict__ tiles)
{
    __shared__ int s_w[WG / 64];
    const int i = blockIdx.x / B, j = blockIdx.x % B, t = threadIdx.x;
    if (!job_live(body_boxes, group, flags, i, j)) {        // the same in every lane
        if (!tiles && t == 0) job_tiles[blockIdx.x] = 0;
        return;
    }
    const auto live = [&](int k) { return tile_live(chunk_boxes, nC, flags, i, j, k / nC, k % nC); };
    if (!tiles) {
        const int n = wg_count(nC * nC, s_w, live);
        if (t == 0) job_tiles[blockIdx.x] = n;
        return;
    }
    const int want = job_tiles[blockIdx.x];
    if (want == 0) return;
    wg_emit(nC * nC, want, job_off[blockIdx.x], n_tiles, s_w, live, [&](long long pos, int k) { tiles[pos] = Tile{i, j, k / nC, k % nC}; });
}

// The hot pass.  EMIT = false: tile_hits[tile] = the crossing pairs of the tile.  EMIT = true: key, events and length of every crossing
// pair, at tile_off[tile] + a slot taken from an LDS counter (the order within a tile is free: the keys are unique and sorted afterwards).
template <bool EMIT>
__global__ __launch_bounds__(WG) void sc_test_kernel(const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                     const int32_t *__restrict__ orig, const int32_t *__restrict__ part,
                                                     const uint8_t *__restrict__ skip, int P, int B, int V, int F,
                                                     const Tile *__restrict__ tiles, int *__restrict__ tile_hits,
                                                     const long long *__restrict__ tile_off, long long n_pairs, long long *__restrict__ keys,
                                                     int *__restrict__ events, float *__restrict__ length)
{
    // 20 KB: per staged face lo.xyz hi.x | hi.yz id0 id1 | id2 part p0.xy | p0.z p1.xyz | p2.xyz orig
    __shared__ float4 stage[WG * 5];
    __shared__ int s_w[WG / 64];
    __shared__ int s_slot;
    const int t = threadIdx.x;
    const Tile tl = tiles[blockIdx.x];
    const bool self = tl.i == tl.j, diagonal = self && tl.ca == tl.cb;
    const int nst = min(SC_CHUNK, F - tl.cb * SC_CHUNK);
    if (EMIT && t == 0) s_slot = 0;
    if (t < nst) {
        const int pos = tl.cb * SC_CHUNK + t;
        int id[3];
        float q[3][3], lo[3], hi[3];
        load_triangle(verts + (size_t)tl.j * V * 3, faces + (size_t)pos * 3, id, q);
        sc_face_box(q, lo, hi);
        stage[5 * t] = make_float4(lo[0], lo[1], lo[2], hi[0]);
        stage[5 * t + 1] = make_float4(hi[1], hi[2], __int_as_float(id[0]), __int_as_float(id[1]));
        stage[5 * t + 2] = make_float4(__int_as_float(id[2]), __int_as_float(part ? part[pos] : 0), q[0][0], q[0][1]);
        stage[5 * t + 3] = make_float4(q[0][2], q[1][0], q[1][1], q[1][2]);
        stage[5 * t + 4] = make_float4(q[2][0], q[2][1], q[2][2], __int_as_float(orig[pos]));
    }
    const int apos = tl.ca * SC_CHUNK + t;
    const bool live = apos < F;
    int aid[3] = {0, 0, 0}, apart = 0, aorig = 0;
    float p[3][3] = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}}, alo[3], ahi[3];
    if (live) {
        load_triangle(verts + (size_t)tl.i * V * 3, faces + (size_t)apos * 3, aid, p);
        apart = part ? part[apos] : 0;
        aorig = orig[apos];
    }
    sc_face_box(p, alo, ahi);
    const long long off = EMIT ? tile_off[blockIdx.x] : 0;
    const int want = EMIT ? tile_hits[blockIdx.x] : 0;
    __syncthreads();
    int hits = 0;
    if (live) {
        const int k0 = diagonal ? t + 1 : 0;    // on a diagonal tile every unordered pair of positions once
        for (int k = k0; k < nst; k++) {
            const float4 r0 = stage[5 * k], r1 = stage[5 * k + 1];
            const float blo[3] = {r0.x, r0.y, r0.z}, bhi[3] = {r0.w, r1.x, r1.y};
            if (!geom_boxes_meet(alo, ahi, blo, bhi)) continue;
            const float4 r2 = stage[5 * k + 2];
            if (self) {
                const int bid[3] = {__float_as_int(r1.z), __float_as_int(r1.w), __float_as_int(r2.x)};
                if (sc_share_vertex(aid, bid)) continue;
                if (skip && skip[(size_t)apart * P + __float_as_int(r2.y)]) continue;
            }
            const float4 r3 = stage[5 * k + 3], r4 = stage[5 * k + 4];
            const float q[3][3] = {{r2.z, r2.w, r3.x}, {r3.y, r3.z, r3.w}, {r4.x, r4.y, r4.z}};
            float len;
            const int ev = sc_pair(p, q, &len);
            if (ev == 0) continue;
            hits++;
            if (EMIT) {
                const int slot = atomicAdd(&s_slot, 1);
                const long long at = off + slot;
                if (slot < want && at < n_pairs) {
                    const int borig = __float_as_int(r4.w);
                    const int s = self ? min(aorig, borig) : aorig, u = self ? max(aorig, borig) : borig;
                    keys[at] = sc_key(tl.i, s, tl.j, u, B, F);
                    events[at] = ev;
                    length[at] = len;
                }
            }
        }
    }
    if (!EMIT) {
        hits = wg_sum(hits, s_w);
        if (t == 0) tile_hits[blockIdx.x] = hits;
    }
}

// One lane per pair of the sorted list: the row, and integer atomics (which commute) into counts, the face mask and the irregular count
__global__ __launch_bounds__(WG) void sc_finish_kernel(const long long *__restrict__ keys, const long long *__restrict__ order,
                                                       const int *__restrict__ ev_in, const float *__restrict__ len_in, long long n, int B, int F,
                                                       int mask_words, int *__restrict__ pairs, int *__restrict__ ev_out,
                                                       float *__restrict__ len_out, int *__restrict__ counts, unsigned int *__restrict__ mask,
                                                       int *__restrict__ irregular)
{
    const long long c = (long long)blockIdx.x * WG + threadIdx.x;
    if (c >= n) return;
    int r[4];
    sc_unkey(keys[c], B, F, r);
    const long long from = order[c];
    const int ev = ev_in[from];
#pragma unroll
    for (int a = 0; a < 4; a++) pairs[c * 4 + a] = r[a];
    ev_out[c] = ev;
    len_out[c] = len_in[from];
    atomicAdd(counts + (size_t)r[0] * B + r[2], 1);
    if (r[0] != r[2]) atomicAdd(counts + (size_t)r[2] * B + r[0], 1);
    atomicOr(mask + (size_t)r[0] * mask_words + (r[1] >> 5), 1u << (r[1] & 31));
    atomicOr(mask + (size_t)r[2] * mask_words + (r[3] >> 5), 1u << (r[3] & 31));
    if (ev != 2) atomicAdd(irregular, 1);
}

// contour [B,B] fp64: one workgroup per job (i, j), i <= j, with pairs.  The pairs of body i are rows row_start[i] .. row_start[i+1] of the
// sorted list; the lanes find those of body j, lane 0 adds their lengths one after the other in row order.
__global__ __launch_bounds__(WG) void sc_contour_kernel(const int *__restrict__ pairs, const float *__restrict__ length,
                                                        const long long *__restrict__ row_start, const int *__restrict__ counts, int B,
                                                        double *__restrict__ contour)
{
    __shared__ float s_len[WG];
    __shared__ unsigned long long s_mask[WG / 64];
    const int i = blockIdx.x / B, j = blockIdx.x % B, t = threadIdx.x;
    if (i > j || counts[blockIdx.x] == 0) return;
    const long long lo = row_start[i], hi = row_start[i + 1];
    double acc = 0.0;
    for (long long r0 = lo; r0 < hi; r0 += WG) {
        const long long r = r0 + t;
        const bool mine = r < hi && pairs[r * 4 + 2] == j;
        s_len[t] = mine ? length[r] : 0.0f;
        const unsigned long long m = __ballot(mine);
        if ((t & 63) == 0) s_mask[t >> 6] = m;
        __syncthreads();
        if (t == 0)
            for (int w = 0; w < WG / 64; w++)
                for (unsigned long long mm = s_mask[w]; mm; mm &= mm - 1) acc += (double)s_len[w * 64 + __ffsll((long long)mm) - 1];
        __syncthreads();
    }
    if (t == 0) {
        contour[(size_t)i * B + j] = acc;
        contour[(size_t)j * B + i] = acc;
    }
}

}  // namespace psi_sc

extern "C" int psi_surface_crossings_face_order(const int32_t *h_faces, int V, int F, const float *h_order_verts, int32_t *h_order)
{
    PSI_REQUIRE(h_faces && h_order, "null pointer");
    PSI_REQUIRE(V >= 1 && F >= 1 && F < SC_MAX_F, "V >= 1 and 1 <= F < 2^21");
    const int rc = psi_check_faces(h_faces, V, F);
    if (rc) return rc;
    if (!h_order_verts) {
        for (int f = 0; f < F; f++) h_order[f] = f;
        return 0;
    }
    PSI_REQUIRE(sc_morton_order(h_order_verts, h_faces, F, h_order), "order_verts is finite");
    return 0;
}

extern "C" int psi_surface_crossings_create(psi_surface_crossings **out, const int32_t *h_faces, int V, int F, const float *h_order_verts,
                                            const int32_t *h_face_part, const uint8_t *h_part_skip, int P)
{
    PSI_REQUIRE(out && h_faces, "null pointer");
    PSI_REQUIRE((h_face_part == nullptr) == (h_part_skip == nullptr), "face_part and part_skip come together");
    PSI_REQUIRE(h_face_part ? (P >= 1 && P <= 32768) : P == 0, "1 <= P <= 32768 with parts, P = 0 without");
    PSI_REQUIRE(F >= 1, "F >= 1");
    std::vector<int32_t> order((size_t)F);
    const int rc = psi_surface_crossings_face_order(h_faces, V, F, h_order_verts, order.data());
    if (rc) return rc;
    std::vector<int32_t> faces((size_t)F * 3), part;
    for (int k = 0; k < F; k++)
        for (int a = 0; a < 3; a++) faces[(size_t)k * 3 + a] = h_faces[(size_t)order[k] * 3 + a];
    if (h_face_part) {
        part.resize((size_t)F);
        for (int k = 0; k < F; k++) {
            const int32_t pt = h_face_part[order[k]];
            if (pt < 0 || pt >= P) {
                psi_set_error("invalid argument: face %d has part %d outside [0, %d)", (int)order[k], (int)pt, P);
                return PSI_EINVAL;
            }
            part[k] = pt;
        }
        for (int a = 0; a < P; a++)
            for (int b = 0; b < P; b++)
                PSI_REQUIRE((h_part_skip[(size_t)a * P + b] != 0) == (h_part_skip[(size_t)b * P + a] != 0), "part_skip is symmetric");
    }
    psi_surface_crossings *h = new psi_surface_crossings{nullptr, nullptr, nullptr, nullptr, nullptr, V, F, P, nullptr};
    PsiBlob T;
    T.upload(h->d_faces, faces.data(), faces.size() * sizeof(int32_t));
    T.upload(h->d_orig, order.data(), order.size() * sizeof(int32_t));
    T.upload(h->d_part, part.data(), part.size() * sizeof(int32_t)).or_null();
    T.upload(h->d_skip, h_part_skip, (size_t)P * P).or_null();
    T.upload(h->d_caller, h_faces, (size_t)F * 3 * sizeof(int32_t));
    if (int e = psi_blob_realise(T, &h->blob, "psi_surface_crossings_create")) {
        delete h;
        return e;
    }
    *out = h;
    return 0;
}

extern "C" void psi_surface_crossings_destroy(psi_surface_crossings *h)
{
    if (!h) return;
    (void)hipFree(h->blob);
    delete h;
}

extern "C" int psi_surface_crossings_info(const psi_surface_crossings *h, int32_t info[4])
{
    PSI_REQUIRE(h && info, "null pointer");
    info[0] = h->V;
    info[1] = h->F;
    info[2] = (h->F + SC_CHUNK - 1) / SC_CHUNK;
    info[3] = h->P;
    return 0;
}

#define SC_REQUIRE_B(h, B)                                                                                          \
    PSI_REQUIRE(B >= 1 && B <= GEOM_MAX_B, "1 <= B <= 46340");                                                      \
    PSI_REQUIRE((double)B * h->F * (double)B * h->F < 9.2e18, "(B * F)^2 < 2^63: the pair key is one int64")

extern "C" int psi_surface_crossings_boxes(const psi_surface_crossings *h, const float *d_verts, int B, float *d_chunk_boxes,
                                           float *d_body_boxes, int32_t *d_bad, void *stream)
{
    PSI_REQUIRE(h && d_verts && d_chunk_boxes && d_body_boxes && d_bad, "null pointer");
    SC_REQUIRE_B(h, B);
    hipStream_t st = (hipStream_t)stream;
    const int nC = (h->F + SC_CHUNK - 1) / SC_CHUNK;
    PSI_CHECK_HIP(psi_reset_bad_flag(d_bad, st));
    hipLaunchKernelGGL(psi_sc::sc_chunk_box_kernel, dim3(nC, B), dim3(psi_sc::WG), 0, st, d_verts, h->d_faces, h->V, h->F, d_chunk_boxes);
    PSI_CHECK_LAUNCH("sc_chunk_box_kernel");
    hipLaunchKernelGGL(psi_sc::sc_body_box_kernel, dim3(B), dim3(psi_sc::WG), 0, st, d_verts, h->V, d_body_boxes, d_bad);
    PSI_CHECK_LAUNCH("sc_body_box_kernel");
    return 0;
}

extern "C" int psi_surface_crossings_tiles(const psi_surface_crossings *h, const int32_t *d_group, int B, int flags, const float *d_chunk_boxes,
                                           const float *d_body_boxes, int32_t *d_job_tiles, const int64_t *d_job_off, long long n_tiles,
                                           int32_t *d_tiles, void *stream)
{
    PSI_REQUIRE(h && d_chunk_boxes && d_body_boxes && d_job_tiles, "null pointer");
    SC_REQUIRE_TILE_PASS(d_job_off, n_tiles, d_tiles);
    PSI_REQUIRE(flags >= 0 && flags < 8, "flags");
    SC_REQUIRE_B(h, B);
    hipLaunchKernelGGL(psi_sc::sc_tile_kernel, dim3(B * B), dim3(psi_sc::WG), 0, (hipStream_t)stream, d_chunk_boxes, d_body_boxes, d_group, B,
                       (h->F + SC_CHUNK - 1) / SC_CHUNK, flags, d_job_tiles, (const long long *)d_job_off, n_tiles, (psi_sc::Tile *)d_tiles);
    PSI_CHECK_LAUNCH("sc_tile_kernel");
    return 0;
}

extern "C" int psi_surface_crossings_test(const psi_surface_crossings *h, const float *d_verts, int B, const int32_t *d_tiles, long long n_tiles,
                                          int32_t *d_tile_hits, const int64_t *d_tile_off, long long n_pairs, int64_t *d_keys,
                                          int32_t *d_events, float *d_length, void *stream)
{
    PSI_REQUIRE(h && d_verts && d_tiles && d_tile_hits, "null pointer");
    SC_REQUIRE_TEST_PASS(n_tiles, SC_REQUIRE_B(h, B), d_tile_off, n_pairs, d_keys, d_events, d_length);
    SC_LAUNCH_TEST(psi_sc::sc_test_kernel, n_tiles, stream, d_keys, d_verts, h->d_faces, h->d_orig, h->d_part, h->d_skip, h->P, B, h->V, h->F,
                   (const psi_sc::Tile *)d_tiles, d_tile_hits, (const long long *)d_tile_off, n_pairs, (long long *)d_keys, d_events, d_length);
    PSI_CHECK_LAUNCH("sc_test_kernel");
    return 0;
}

extern "C" int psi_surface_crossings_finish(const psi_surface_crossings *h, int B, const int64_t *d_keys_sorted, const int64_t *d_order,
                                            const int32_t *d_events_in, const float *d_length_in, long long n_pairs, const int64_t *d_row_start,
                                            int32_t *d_pairs, int32_t *d_events, float *d_length, int32_t *d_counts, double *d_contour,
                                            uint32_t *d_face_mask, int32_t *d_irregular, void *stream)
{
    PSI_REQUIRE(h && d_keys_sorted && d_order && d_events_in && d_length_in && d_row_start && d_pairs && d_events && d_length && d_counts &&
                    d_contour && d_face_mask && d_irregular, "null pointer");
    PSI_REQUIRE(n_pairs >= 1 && n_pairs < (1ll << 31), "1 <= n_pairs < 2^31");
    SC_REQUIRE_B(h, B);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(psi_sc::sc_finish_kernel, dim3(psi_cdiv(n_pairs, psi_sc::WG)), dim3(psi_sc::WG), 0, st, (const long long *)d_keys_sorted,
                       (const long long *)d_order, d_events_in, d_length_in, n_pairs, B, h->F, (h->F + 31) / 32, d_pairs, d_events, d_length,
                       d_counts, d_face_mask, d_irregular);
    PSI_CHECK_LAUNCH("sc_finish_kernel");
    hipLaunchKernelGGL(psi_sc::sc_contour_kernel, dim3(B * B), dim3(psi_sc::WG), 0, st, d_pairs, d_length, (const long long *)d_row_start, d_counts,
                       B, d_contour);
    PSI_CHECK_LAUNCH("sc_contour_kernel");
    return 0;
}
