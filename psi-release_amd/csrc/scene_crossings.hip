// Scene crossings: which triangles of the posed body surfaces of a batch properly intersect which triangles of a static scene mesh, for
// gfx950 (wave64).  The contract is DESIGN.md section 10i; the per-pair statements and the Morton order are csrc/surface_crossings_shared.h,
// the key and the host half of create csrc/scene_crossings_shared.h, the closed-box test csrc/geom_shared.h, the workgroup sum and the two
// passes of a count-or-emit job csrc/wg_device.h, the argument rules of the count-or-emit entry points and the launch of a test kernel's
// two forms, as in the body search, csrc/crossings_common.h.  This file is compiled with -ffp-contract=off.
//
//   candidate  a body face (i, s) and a scene triangle t whose closed exact face boxes meet
//   decision   sc_pair(P = body face, Q = scene triangle): the pair crosses iff at least one edge of one pierces the other
//
// The scene handle keeps the triangles along a Morton curve of their centroids in chunks of 256, with the box of every chunk and of the
// scene; the bodies come with the chunks and boxes of a psi_surface_crossings handle (psi_surface_crossings_boxes).  Passes: tiles (a job
// is a body chunk (i, c), a tile a job and a scene chunk k whose boxes meet; counted, then written from the caller's scan in ascending
// k), test (the hot pass: one workgroup per tile; every lane keeps one body face in registers, the records of the scene chunk are staged
// in LDS with their boxes and read by all lanes at the same address, which broadcasts; once to count, once to emit key, events and
// length), finish (after the caller's sort of the keys: the rows, and counts, the two bit masks and the irregular count by integer
// atomics, which commute) and contour (one workgroup per body adds the lengths of its rows in fp64, one after the other in row order).
// No floating-point atomics.
#include "scene_crossings_shared.h"
#include "crossings_common.h"
#include "surface_crossings_handle.h"
#include "blob.h"

struct psi_scene_crossings {
    char *blob;                // records | chunk boxes
    float4 *d_recs;            // [nf, SCN_REC_ROWS] in chunk order
    float *d_chunk_boxes;      // [nK, 6]
    int nv, nf, nK;
    float box[6];              // the scene's box
};

namespace psi_scn {

constexpr int WG = WG_LANES;
static_assert(WG == SC_CHUNK, "one staged record per lane");

struct Tile { int i, c, k, zero; };
static_assert(sizeof(Tile) == 16, "the tile table is [n_tiles,4] int32");
struct Box6 { float v[6]; };

// job_tiles [B, nCb]: the tiles of job (i, c) = (blockIdx.y, blockIdx.x); every entry is written.  With tiles != null (the emit pass)
// the tiles are written from job_off[job] on, in ascending k.
__global__ __launch_bounds__(WG) void scn_tile_kernel(const float *__restrict__ body_chunk_boxes, const float *__restrict__ body_boxes,
                                                      const float *__restrict__ scene_chunk_boxes, Box6 scene, int nCb, int nK, int brute,
                                                      int *__restrict__ job_tiles, const long long *__restrict__ job_off, long long n_tiles,
                                                      Tile *__restrict__ tiles)
{
    __shared__ int s_w[WG / 64];
    const int c = blockIdx.x, i = blockIdx.y, t = threadIdx.x;
    const size_t job = (size_t)i * nCb + c;
    const float *bb = body_boxes + (size_t)i * 6, *cb = body_chunk_boxes + job * 6;
    // the same in every lane: a body outside the scene's box costs one comparison
    const bool live = brute || (geom_boxes_meet(bb, bb + 3, scene.v, scene.v + 3) && geom_boxes_meet(cb, cb + 3, scene.v, scene.v + 3));
    if (!live) {
        if (!tiles && t == 0) job_tiles[job] = 0;
        return;
    }
    const auto meets = [&](int k) {
        return brute || geom_boxes_meet(cb, cb + 3, scene_chunk_boxes + (size_t)k * 6, scene_chunk_boxes + (size_t)k * 6 + 3);
    };
    if (!tiles) {
        const int n = wg_count(nK, s_w, meets);
        if (t == 0) job_tiles[job] = n;
        return;
    }
    const int want = job_tiles[job];
    if (want == 0) return;
    wg_emit(nK, want, job_off[job], n_tiles, s_w, meets, [&](long long pos, int k) { tiles[pos] = Tile{i, c, k, 0}; });
}

// The hot pass.  EMIT = false: tile_hits[tile] = the crossing pairs of the tile.  EMIT = true: key, events and length of every crossing
// pair, at tile_off[tile] + a slot taken from an LDS counter (the order within a tile is free: the keys are unique and sorted afterwards).
template <bool EMIT>
__global__ __launch_bounds__(WG) void scn_test_kernel(const float4 *__restrict__ recs, int nf, int nK, const float *__restrict__ verts,
                                                      const int32_t *__restrict__ faces, const int32_t *__restrict__ orig, int B, int V, int F,
                                                      const Tile *__restrict__ tiles, int *__restrict__ tile_hits,
                                                      const long long *__restrict__ tile_off, long long n_pairs, long long *__restrict__ keys,
                                                      int *__restrict__ events, float *__restrict__ length)
{
    // 16 KB: per staged triangle lo.xyz hi.x | hi.yz q0.xy | q0.z q1.xyz | q2.xyz caller's index
    __shared__ float4 stage[WG * 4];
    __shared__ int s_w[WG / 64];
    __shared__ int s_slot;
    const int t = threadIdx.x;
    const Tile tl = tiles[blockIdx.x];
    const int nCb = (F + SC_CHUNK - 1) / SC_CHUNK;
    if (tl.i < 0 || tl.i >= B || tl.c < 0 || tl.c >= nCb || tl.k < 0 || tl.k >= nK) {     // not a tile of this batch (the same in every lane)
        if (!EMIT && t == 0) tile_hits[blockIdx.x] = 0;
        return;
    }
    const int nst = min(SC_CHUNK, nf - tl.k * SC_CHUNK);
    if (EMIT && t == 0) s_slot = 0;
    if (t < nst) {          // rows past the end of a partial scene chunk are neither read nor staged
        const float4 *r = recs + ((size_t)tl.k * SC_CHUNK + t) * SCN_REC_ROWS;
        const float4 a = r[0], b = r[1], c = r[2];
        const float q[3][3] = {{a.x, a.y, a.z}, {a.w, b.x, b.y}, {b.z, b.w, c.x}};
        float lo[3], hi[3];
        sc_face_box(q, lo, hi);
        stage[4 * t] = make_float4(lo[0], lo[1], lo[2], hi[0]);
        stage[4 * t + 1] = make_float4(hi[1], hi[2], q[0][0], q[0][1]);
        stage[4 * t + 2] = make_float4(q[0][2], q[1][0], q[1][1], q[1][2]);
        stage[4 * t + 3] = make_float4(q[2][0], q[2][1], q[2][2], c.y);
    }
    const int apos = tl.c * SC_CHUNK + t;
    const bool live = apos < F;         // lanes past the end of a partial body chunk take no part
    int aorig = 0;
    float p[3][3] = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}}, alo[3], ahi[3];
    if (live) {
        const float *v = verts + (size_t)tl.i * V * 3;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int id = faces[(size_t)apos * 3 + k];
#pragma unroll
            for (int a = 0; a < 3; a++) p[k][a] = v[(size_t)id * 3 + a];
        }
        aorig = orig[apos];
    }
    sc_face_box(p, alo, ahi);
    const long long off = EMIT ? tile_off[blockIdx.x] : 0;
    const int want = EMIT ? tile_hits[blockIdx.x] : 0;
    __syncthreads();
    int hits = 0;
    if (live) {
        for (int k = 0; k < nst; k++) {
            const float4 r0 = stage[4 * k], r1 = stage[4 * k + 1];
            const float blo[3] = {r0.x, r0.y, r0.z}, bhi[3] = {r0.w, r1.x, r1.y};
            if (!geom_boxes_meet(alo, ahi, blo, bhi)) continue;
            const float4 r2 = stage[4 * k + 2], r3 = stage[4 * k + 3];
            const float q[3][3] = {{r1.z, r1.w, r2.x}, {r2.y, r2.z, r2.w}, {r3.x, r3.y, r3.z}};
            float len;
            const int ev = sc_pair(p, q, &len);
            if (ev == 0) continue;
            hits++;
            if (EMIT) {
                const int slot = atomicAdd(&s_slot, 1);
                const long long at = off + slot;
                if (slot < want && at >= 0 && at < n_pairs) {
                    keys[at] = scn_key(tl.i, aorig, __float_as_int(r3.w), F, nf);
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

// One lane per row of the sorted list: the row, and integer atomics (which commute) into counts, the two bit masks and the irregular count
__global__ __launch_bounds__(WG) void scn_finish_kernel(const long long *__restrict__ keys, const long long *__restrict__ order,
                                                        const int *__restrict__ ev_in, const float *__restrict__ len_in, long long n, int B, int F,
                                                        int nf, int face_words, int *__restrict__ pairs, int *__restrict__ ev_out,
                                                        float *__restrict__ len_out, int *__restrict__ counts,
                                                        unsigned int *__restrict__ face_mask, unsigned int *__restrict__ tri_mask,
                                                        int *__restrict__ irregular)
{
    const long long c = (long long)blockIdx.x * WG + threadIdx.x;
    if (c >= n) return;
    int r[3];
    scn_unkey(keys[c], F, nf, r);
    const long long from = order[c];
    const bool ok = from >= 0 && from < n && r[0] >= 0 && r[0] < B;        // a key of this batch (r[1] < F and r[2] < nf by the modulus)
    const int ev = ok ? ev_in[from] : 0;
#pragma unroll
    for (int a = 0; a < 3; a++) pairs[c * 3 + a] = r[a];
    ev_out[c] = ev;
    len_out[c] = ok ? len_in[from] : 0.0f;
    if (!ok) return;
    atomicAdd(counts + r[0], 1);
    atomicOr(face_mask + (size_t)r[0] * face_words + (r[1] >> 5), 1u << (r[1] & 31));
    atomicOr(tri_mask + (r[2] >> 5), 1u << (r[2] & 31));
    if (ev != 2) atomicAdd(irregular, 1);
}

// contour [B] fp64: one workgroup per body; its rows are row_start[i] .. row_start[i+1] of the sorted list; the lanes fetch 256 lengths,
// lane 0 adds them one after the other in row order.
__global__ __launch_bounds__(WG) void scn_contour_kernel(const float *__restrict__ length, const long long *__restrict__ row_start, long long n,
                                                         double *__restrict__ contour)
{
    __shared__ float s_len[WG];
    const int i = blockIdx.x, t = threadIdx.x;
    const long long lo = max(row_start[i], 0ll), hi = min(row_start[i + 1], n);
    if (hi <= lo) return;                                   // the same in every lane
    double acc = 0.0;
    for (long long r0 = lo; r0 < hi; r0 += WG) {
        const long long r = r0 + t;
        s_len[t] = r < hi ? length[r] : 0.0f;
        __syncthreads();
        if (t == 0) {
            const int m = (int)min((long long)WG, hi - r0);
            for (int k = 0; k < m; k++) acc += (double)s_len[k];
        }
        __syncthreads();
    }
    if (t == 0) contour[i] = acc;
}

}  // namespace psi_scn

extern "C" int psi_scene_crossings_create(psi_scene_crossings **out, const float *h_verts, int nv, const int32_t *h_faces, int nf)
{
    PSI_REQUIRE(out && h_verts && h_faces, "null pointer");
    PSI_REQUIRE(nv >= 1 && nf >= 1, "nv >= 1 and 1 <= nf < 2^31");
    ScnBuilt hb;
    long long bad = -1;
    const int rc = scn_build(h_verts, nv, h_faces, nf, &hb, &bad);
    if (rc == SCN_BAD_INDEX) psi_set_error("invalid argument: scene triangle %lld refers to a vertex outside [0, %d)", bad, nv);
    if (rc == SCN_NOT_FINITE) psi_set_error("invalid argument: scene triangle %lld refers to a non-finite vertex", bad);
    if (rc == SCN_NO_FACES) psi_set_error("invalid argument: 1 <= nf < 2^31");
    if (rc) return PSI_EINVAL;
    psi_scene_crossings *h = new psi_scene_crossings{nullptr, nullptr, nullptr, nv, nf, (nf + SC_CHUNK - 1) / SC_CHUNK, {0, 0, 0, 0, 0, 0}};
    for (int a = 0; a < 6; a++) h->box[a] = hb.box[a];
    PsiBlob T;
    T.upload(h->d_recs, hb.recs.data(), hb.recs.size() * sizeof(float));
    T.upload(h->d_chunk_boxes, hb.chunk_boxes.data(), hb.chunk_boxes.size() * sizeof(float));
    if (int e = psi_blob_realise(T, &h->blob, "psi_scene_crossings_create")) {
        delete h;
        return e == (int)hipErrorOutOfMemory ? PSI_ENOMEM : e;
    }
    *out = h;
    return 0;
}

extern "C" void psi_scene_crossings_destroy(psi_scene_crossings *h)
{
    if (!h) return;
    (void)hipFree(h->blob);
    delete h;
}

extern "C" int psi_scene_crossings_info(const psi_scene_crossings *h, int32_t info[4])
{
    PSI_REQUIRE(h && info, "null pointer");
    info[0] = h->nv;
    info[1] = h->nf;
    info[2] = h->nK;
    info[3] = 0;
    return 0;
}

#define SCN_REQUIRE_B(h, B, F)                                                                          \
    PSI_REQUIRE(B >= 1 && B <= GEOM_MAX_B, "1 <= B <= 46340");                                          \
    PSI_REQUIRE(F >= 1 && F < SC_MAX_F, "1 <= F < 2^21");                                               \
    PSI_REQUIRE(scn_key_fits(B, F, h->nf), "B * F * nf < 2^63: the pair key is one int64")

extern "C" int psi_scene_crossings_tiles(const psi_scene_crossings *h, const psi_surface_crossings *body, int B, int brute,
                                         const float *d_chunk_boxes, const float *d_body_boxes, int32_t *d_job_tiles, const int64_t *d_job_off,
                                         long long n_tiles, int32_t *d_tiles, void *stream)
{
    PSI_REQUIRE(h && body && d_chunk_boxes && d_body_boxes && d_job_tiles, "null pointer");
    SC_REQUIRE_TILE_PASS(d_job_off, n_tiles, d_tiles);
    PSI_REQUIRE(brute == 0 || brute == 1, "brute is 0 or 1");
    SCN_REQUIRE_B(h, B, body->F);
    psi_scn::Box6 scene;
    for (int a = 0; a < 6; a++) scene.v[a] = h->box[a];
    const int nCb = (body->F + SC_CHUNK - 1) / SC_CHUNK;
    hipLaunchKernelGGL(psi_scn::scn_tile_kernel, dim3(nCb, B), dim3(psi_scn::WG), 0, (hipStream_t)stream, d_chunk_boxes, d_body_boxes,
                       h->d_chunk_boxes, scene, nCb, h->nK, brute, d_job_tiles, (const long long *)d_job_off, n_tiles, (psi_scn::Tile *)d_tiles);
    PSI_CHECK_LAUNCH("scn_tile_kernel");
    return 0;
}

extern "C" int psi_scene_crossings_test(const psi_scene_crossings *h, const psi_surface_crossings *body, const float *d_verts, int B,
                                        const int32_t *d_tiles, long long n_tiles, int32_t *d_tile_hits, const int64_t *d_tile_off,
                                        long long n_pairs, int64_t *d_keys, int32_t *d_events, float *d_length, void *stream)
{
    PSI_REQUIRE(h && body && d_verts && d_tiles && d_tile_hits, "null pointer");
    SC_REQUIRE_TEST_PASS(n_tiles, SCN_REQUIRE_B(h, B, body->F), d_tile_off, n_pairs, d_keys, d_events, d_length);
    SC_LAUNCH_TEST(psi_scn::scn_test_kernel, n_tiles, stream, d_keys, h->d_recs, h->nf, h->nK, d_verts, body->d_faces, body->d_orig, B, body->V,
                   body->F, (const psi_scn::Tile *)d_tiles, d_tile_hits, (const long long *)d_tile_off, n_pairs, (long long *)d_keys, d_events,
                   d_length);
    PSI_CHECK_LAUNCH("scn_test_kernel");
    return 0;
}

extern "C" int psi_scene_crossings_finish(const psi_scene_crossings *h, const psi_surface_crossings *body, int B, const int64_t *d_keys_sorted,
                                          const int64_t *d_order, const int32_t *d_events_in, const float *d_length_in, long long n_pairs,
                                          const int64_t *d_row_start, int32_t *d_pairs, int32_t *d_events, float *d_length, int32_t *d_counts,
                                          double *d_contour, uint32_t *d_face_mask, uint32_t *d_tri_mask, int32_t *d_irregular, void *stream)
{
    PSI_REQUIRE(h && body && d_keys_sorted && d_order && d_events_in && d_length_in && d_row_start && d_pairs && d_events && d_length && d_counts &&
                    d_contour && d_face_mask && d_tri_mask && d_irregular, "null pointer");
    PSI_REQUIRE(n_pairs >= 1 && n_pairs < (1ll << 31), "1 <= n_pairs < 2^31");
    SCN_REQUIRE_B(h, B, body->F);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(psi_scn::scn_finish_kernel, dim3(psi_cdiv(n_pairs, psi_scn::WG)), dim3(psi_scn::WG), 0, st, (const long long *)d_keys_sorted,
                       (const long long *)d_order, d_events_in, d_length_in, n_pairs, B, body->F, h->nf, (body->F + 31) / 32, d_pairs, d_events,
                       d_length, d_counts, d_face_mask, d_tri_mask, d_irregular);
    PSI_CHECK_LAUNCH("scn_finish_kernel");
    hipLaunchKernelGGL(psi_scn::scn_contour_kernel, dim3(B), dim3(psi_scn::WG), 0, st, d_length, (const long long *)d_row_start, n_pairs, d_contour);
    PSI_CHECK_LAUNCH("scn_contour_kernel");
    return 0;
}
