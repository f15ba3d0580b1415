// Result images for gfx950 (wave64): generated bodies drawn into the snapshots of their scene, shaded, with the pixels of every body that
// the scene hides counted — what the reference captures from an open3d window (utils/utils_show_test_results.py, img_%06d_cam1.png /
// _cam2.png).  The bodies go through the snapshot rasteriser's own statements (raster_device.h; this file is compiled with
// -ffp-contract=off), so the arithmetic contract of raster.hip holds here word for word; DESIGN.md "Result images" states the rest:
//   normal     of a vertex: the sum, in ascending face index, of the unnormalised (v1 - v0) x (v2 - v0) of its faces (world frame)
//   draw       a (body, view) pair with a colour; the index of a piece is d * F + face, the key (bits of z) << 32 | index as in raster.hip
//   owner      the body owns a pixel iff a body piece covers it and the scene has no hit there or z_body < z_scene (fp32 compare)
//   shade      s = 0.3 + (0.7*|N_z|) / sqrtf((N_x^2 + N_y^2) + N_z^2), 0.3 when the length is 0 or not finite; N is the interpolated
//              camera-space vertex normal (l0*(n0*iz0) + l1*(n1*iz1)) + l2*(n2*iz2) of a body, the flat normal of a scene triangle
//   channel    (unsigned char)rintf(255 * min(max(c, 0), 1)) of colour * s
//
// Launches of one psi_raster_bodies_render call:
//   rb_check_draws   one lane per draw: body and view indices in range
//   per pass of at most draws_per_pass draws (the piece records of a pass are what the workspace holds):
//     rb_setup       one lane per (draw, face): pieces -> records, tile boxes, per-(view, tile) counts
//     rs_scan, rs_view_base, the one host read of the pass (the views' pair counts; the first pass also brings rb_check_draws' verdict),
//     rs_fill        the binning pass both rasterisers share (raster_bins.h: rs_bin_pass); a row of rs_fill is a draw, the bin entry the
//                    piece slot within the pass, in the bins of the draw's view
//     rb_tile        one workgroup per (view, tile): raster.hip's LDS z-buffer over the bin, min-combined into the body key image by a plain
//                    load / min / store (one workgroup owns a tile within a pass, and the passes are stream-ordered)
//   rb_compose       one lane per pixel: owner, shading (the winning triangle set up again with three attributes), colours, counts
// No floating-point atomics; integer atomics only for the bin counts and the per-draw pixel counts.
#include "raster_bins.h"
#include "blob.h"
#include <algorithm>
#include <vector>

struct psi_raster_bodies {
    int *faces;        // [F][3]    device
    int *voff;         // [V + 1]   CSR: the faces of vertex v are vface[voff[v] .. voff[v + 1]), ascending
    int *vface;        // [3 F]
    int V, F;
    RsGrownBins bins_extra;  // as psi_raster_mesh's, for a pass
    char *blob;        // the one allocation behind faces, voff and vface
};

namespace {

constexpr int MAX_PASS_DRAWS = 65535;    // a pass's draws are a grid dimension

// (v1 - v0) x (v2 - v0) of face f of one body, each component two products and one subtraction
RS_FN void face_cross(const float *__restrict__ bv, const int *__restrict__ faces, int f, float c[3])
{
    const float *p0 = bv + (size_t)faces[(size_t)f * 3 + 0] * 3, *p1 = bv + (size_t)faces[(size_t)f * 3 + 1] * 3,
                *p2 = bv + (size_t)faces[(size_t)f * 3 + 2] * 3;
    const float ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
    const float bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
    c[0] = ay * bz - az * by;
    c[1] = az * bx - ax * bz;
    c[2] = ax * by - ay * bx;
}

// the unnormalised normal of vertex v: its faces' cross products summed left to right in list order; (0,0,0) without a face
RS_FN void vertex_normal(const float *__restrict__ bv, const psi_raster_bodies &tp, int v, float n[3])
{
    n[0] = n[1] = n[2] = 0.0f;
    for (int e = tp.voff[v]; e < tp.voff[v + 1]; e++) {
        float c[3];
        face_cross(bv, tp.faces, tp.vface[e], c);
        n[0] = n[0] + c[0];
        n[1] = n[1] + c[1];
        n[2] = n[2] + c[2];
    }
}

RS_FN float shade(float nx, float ny, float nz)
{
    const float len = RS_SQRT((nx * nx + ny * ny) + nz * nz);
    if (!(len > 0.0f) || !(len < INFINITY)) return 0.3f;
    return 0.3f + RS_DIV(0.7f * fabsf(nz), len);
}

RS_FN unsigned char channel(float c) { return (unsigned char)rintf(255.f * fminf(fmaxf(c, 0.f), 1.f)); }

struct Scene {                       // what the compose step reads of the scene; tri == nullptr: no scene
    psi_raster_mesh mesh;
    const float *vrgb, *depth;
    const int *tri;
};

struct Draws {
    const int *body, *view;
    const float *rgb;
    const float *bverts;             // [B][V][3]
};

struct PixelOut {
    unsigned char rgb[3];
    float depth, bdepth;
    int draw, bid;
    bool visible;                    // a body piece covers the pixel (draw_of >= 0) and beats the scene
    int draw_of;                     // the draw of the nearest body piece, -1 without one
};

// one pixel of the result images from its body key and the scene's snapshot
RS_FN PixelOut compose_pixel(const Scene &sc, const psi_raster_bodies &tp, const Draws &dr, const View &vw, float near_, int px, int py, size_t o,
                             unsigned long long key, const float bg[3])
{
    PixelOut out;
    const bool has_body = key != ~0ull;
    const unsigned zbits = (unsigned)(key >> 32);
    const float zb = __builtin_bit_cast(float, zbits);
    const int gid = (int)(unsigned)(key & 0xffffffffu);
    const int d = has_body ? gid / tp.F : -1;
    const int st = sc.tri ? sc.tri[o] : -1;
    const bool scene = st >= 0 && st < sc.mesh.nf;
    const float zs = scene ? sc.depth[o] : 0.0f;
    const bool body_owns = has_body && (!scene || zb < zs);
    out.bdepth = has_body ? zb : 0.0f;
    out.bid = has_body ? gid : -1;
    out.draw_of = d;
    out.visible = body_owns;
    out.draw = body_owns ? d : -1;
    out.depth = body_owns ? zb : zs;
    float col[3] = {bg[0], bg[1], bg[2]};
    if (body_owns) {
        const int face = gid - d * tp.F;
        const float *bv = dr.bverts + (size_t)dr.body[d] * tp.V * 3;
        CamVertT<3> v[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int i = tp.faces[(size_t)face * 3 + k];
            v[k] = to_camera<3>(vw, bv + (size_t)i * 3);
            float n[3];
            vertex_normal(bv, tp, i, n);
#pragma unroll
            for (int c = 0; c < 3; c++) v[k].a[c] = (vw.m[4 * c + 0] * n[0] + vw.m[4 * c + 1] * n[1]) + vw.m[4 * c + 2] * n[2];
        }
        float N[3], z;
        attributes_at<3>(vw, near_, v[0], v[1], v[2], px, py, zbits, N, &z);
        const float s = shade(N[0], N[1], N[2]);
#pragma unroll
        for (int c = 0; c < 3; c++) col[c] = dr.rgb[(size_t)d * 3 + c] * s;
    } else if (scene) {
        CamVertT<3> v[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int i = sc.mesh.faces[(size_t)st * 3 + k];
            v[k] = to_camera<3>(vw, sc.mesh.verts + (size_t)i * 3);
#pragma unroll
            for (int c = 0; c < 3; c++) v[k].a[c] = sc.vrgb ? sc.vrgb[(size_t)i * 3 + c] : 0.8f;
        }
        const float ax = v[1].x - v[0].x, ay = v[1].y - v[0].y, az = v[1].z - v[0].z;
        const float bx = v[2].x - v[0].x, by = v[2].y - v[0].y, bz = v[2].z - v[0].z;
        const float s = shade(ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx);
        float base[3] = {0.8f, 0.8f, 0.8f};
        if (sc.vrgb) {
            float num[3], z;
            attributes_at<3>(vw, near_, v[0], v[1], v[2], px, py, __builtin_bit_cast(unsigned, zs), num, &z);
#pragma unroll
            for (int c = 0; c < 3; c++) base[c] = z * num[c];
        }
#pragma unroll
        for (int c = 0; c < 3; c++) col[c] = base[c] * s;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) out.rgb[c] = channel(col[c]);
    return out;
}

// stage (a) for face f of draw d: the pieces' records and tile boxes (NOBOX: nothing to draw); the number of pieces the guard dropped
RS_FN int setup_body_face(const psi_raster_bodies &tp, const float *__restrict__ bv, const View &vw, float near_, int W, int H, int d, int f,
                          PieceRec r[2], unsigned box[2])
{
    CamVertT<1> v[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        v[k] = to_camera<1>(vw, bv + (size_t)tp.faces[(size_t)f * 3 + k] * 3);
        v[k].a[0] = 0.0f;
    }
    PieceT<1> pc[2];
    int dropped = 0;
    const int n = setup_triangle(vw, near_, v[0], v[1], v[2], pc, &dropped);
#pragma unroll
    for (int k = 0; k < 2; k++) box[k] = k < n ? piece_record(pc[k], d * tp.F + f, W, H, r[k]) : NOBOX;
    return dropped;
}

__global__ __launch_bounds__(256) void rb_normals_kernel(psi_raster_bodies tp, const float *__restrict__ bverts, long total, float *__restrict__ normals)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;          // (body, vertex)
    if (i >= total) return;
    const long b = i / tp.V;
    float n[3];
    vertex_normal(bverts + (size_t)b * tp.V * 3, tp, (int)(i - b * tp.V), n);
    normals[i * 3 + 0] = n[0];
    normals[i * 3 + 1] = n[1];
    normals[i * 3 + 2] = n[2];
}

__global__ __launch_bounds__(256) void rb_check_draws_kernel(const int *__restrict__ draw_body, const int *__restrict__ draw_view, int M, int B, int n_views,
                                                             int *__restrict__ bad)
{
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d < M && (draw_body[d] < 0 || draw_body[d] >= B || draw_view[d] < 0 || draw_view[d] >= n_views)) atomicOr(bad, 1);
}

// piece slot of (draw d0 + j, piece k, face f) of a pass: (j * 2 + k) * F + f.  A draw whose body or view is out of range writes empty
// slots: the host learns of it from rb_check_draws with the first pass's counts and refuses the call.
__global__ __launch_bounds__(256) void rb_setup_kernel(psi_raster_bodies tp, Draws dr, int d0, int B, int n_views, const float *__restrict__ w2c,
                                                       const float *__restrict__ intr, int W, int H, float near_, int tiles_x, int ntiles,
                                                       PieceRec *__restrict__ recs, unsigned *__restrict__ pbox, int *__restrict__ tcount,
                                                       int *__restrict__ stats)
{
    const int j = blockIdx.y, d = d0 + j;
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= tp.F) return;
    const int body = dr.body[d], view = dr.view[d];
    PieceRec r[2];
    unsigned box[2] = {NOBOX, NOBOX};
    if (body >= 0 && body < B && view >= 0 && view < n_views) {
        const int dropped = setup_body_face(tp, dr.bverts + (size_t)body * tp.V * 3, load_view(w2c, intr, view), near_, W, H, d, f, r, box);
        if (dropped) atomicAdd(&stats[view * 2 + 1], dropped);
    }
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const size_t slot = ((size_t)j * 2 + k) * tp.F + f;
        if (box[k] != NOBOX) {
            recs[slot] = r[k];
            count_box_tiles(box[k], view, tiles_x, ntiles, tcount);
        }
        pbox[slot] = box[k];
    }
}

__global__ __launch_bounds__(WG) void rb_tile_kernel(int W, int H, int tiles_x, int ntiles, const PieceRec *__restrict__ recs, const int *__restrict__ tcount,
                                                     const int *__restrict__ toff, const long long *__restrict__ vbase, const int *__restrict__ bins,
                                                     const int *__restrict__ pstats, int *__restrict__ stats, unsigned long long *__restrict__ keyimg)
{
    const int view = blockIdx.y, tile = blockIdx.x, t = threadIdx.x;
    if (tile == 0 && t == 0) stats[view * 2 + 0] += pstats[view * 2 + 0];          // the call's pairs: the passes' summed (one writer, stream order)
    const int n = tcount[(size_t)view * ntiles + tile];
    if (n == 0) return;                                       // the whole workgroup: nothing of this pass touches the tile
    const int tpx = (tile % tiles_x) * TILE, tpy = (tile / tiles_x) * TILE;
    __shared__ unsigned long long zbuf[WG];
    __shared__ PieceRec big[WG];
    __shared__ int nbig;
    const int *__restrict__ bin = bins + vbase[view] + toff[(size_t)view * ntiles + tile];
    const int px = tpx + (t & (TILE - 1)), py = tpy + t / TILE;
    const bool live = px < W && py < H;
    const unsigned long long key = tile_nearest_key(recs, bin, n, W, H, tpx, tpy, px, py, live, zbuf, big, &nbig);
    if (!live) return;
    const size_t o = ((size_t)view * H + py) * W + px;
    keyimg[o] = key_min(keyimg[o], key);
}

__global__ __launch_bounds__(256) void rb_compose_kernel(Scene sc, psi_raster_bodies tp, Draws dr, const float *__restrict__ w2c, const float *__restrict__ intr,
                                                         int W, int H, float near_, const unsigned long long *__restrict__ keyimg, float bg0, float bg1,
                                                         float bg2, unsigned char *__restrict__ rgb, float *__restrict__ depth, int *__restrict__ draw,
                                                         float *__restrict__ bdepth, int *__restrict__ bid, int *__restrict__ counts)
{
    const int view = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    const bool live = p < W * H;
    int dd = -1;
    bool vis = false;
    if (live) {
        const size_t o = (size_t)view * W * H + p;
        const float bg[3] = {bg0, bg1, bg2};
        const PixelOut px = compose_pixel(sc, tp, dr, load_view(w2c, intr, view), near_, p % W, p / W, o, keyimg[o], bg);
        rgb[o * 3 + 0] = px.rgb[0];
        rgb[o * 3 + 1] = px.rgb[1];
        rgb[o * 3 + 2] = px.rgb[2];
        depth[o] = px.depth;
        draw[o] = px.draw;
        bdepth[o] = px.bdepth;
        bid[o] = px.bid;
        dd = px.draw_of;
        vis = px.visible;
    }
    // counts[d] = {covered, visible}: one integer atomic per (wave, draw) rather than per pixel; every lane of the wave arrives here
    unsigned long long todo = __ballot(dd >= 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int dl = __shfl(dd, leader);
        const unsigned long long same = __ballot(dd == dl), seen = __ballot(dd == dl && vis);
        if ((int)(threadIdx.x & 63) == leader) {
            atomicAdd(&counts[dl * 2 + 0], __popcll(same));
            if (seen) atomicAdd(&counts[dl * 2 + 1], __popcll(seen));
        }
        todo &= ~same;
    }
}

struct Layout : BinLayout {
    size_t o_pstats, o_bad, o_keys;
    int dpp;
};

// dpp * F < 2^30: a pass's 2 * dpp * F piece slots are ints in the bins
bool layout(int F, int draws_per_pass, int n_views, int W, int H, Layout &L)
{
    if (F <= 0 || draws_per_pass <= 0 || n_views <= 0 || n_views > 65535 || W <= 0 || H <= 0 || W > 4096 || H > 4096) return false;
    L.dpp = std::min(draws_per_pass, MAX_PASS_DRAWS);
    if ((long long)L.dpp * F >= (1LL << 30)) return false;
    L.begin((size_t)L.dpp * 2 * F, n_views, W, H);
    L.o_pstats = L.take((size_t)n_views * 8);
    L.o_bad = L.take(4);
    L.o_keys = L.take((size_t)n_views * W * H * 8);
    L.place_bins();
    return true;
}

// the CSR of a topology: the faces of vertex v are vface[voff[v] .. voff[v + 1]), ascending; false when an index lies outside [0, V)
bool vertex_face_lists(const std::vector<int> &faces, int V, int F, std::vector<int> &voff, std::vector<int> &vface)
{
    voff.assign((size_t)V + 1, 0);
    vface.resize((size_t)F * 3);
    for (int i : faces) {
        if (i < 0 || i >= V) return false;
        voff[(size_t)i + 1]++;
    }
    for (int v = 0; v < V; v++) voff[(size_t)v + 1] += voff[v];
    std::vector<int> cur(voff.begin(), voff.end() - 1);
    for (int f = 0; f < F; f++)                              // faces in ascending order, so every vertex's list ascends
        for (int k = 0; k < 3; k++) vface[(size_t)cur[faces[(size_t)f * 3 + k]]++] = f;
    return true;
}

}  // namespace

extern "C" int psi_raster_bodies_create(psi_raster_bodies **out, const int32_t *d_faces, int V, int F)
{
    PSI_REQUIRE(out && d_faces, "null pointer");
    PSI_REQUIRE(V >= 1 && F >= 1 && (long)F * 3 < (1L << 31), "V >= 1, 1 <= 3 F < 2^31");
    std::vector<int> hf((size_t)F * 3);
    // a one-off between two device synchronisations, like psi_raster_mesh_create: the faces may have been produced on any stream
    PSI_CHECK_HIP(hipDeviceSynchronize());
    PSI_CHECK_HIP(hipMemcpy(hf.data(), d_faces, hf.size() * 4, hipMemcpyDeviceToHost));
    std::vector<int> voff, vface;
    if (!vertex_face_lists(hf, V, F, voff, vface)) {
        psi_set_error("psi_raster_bodies_create: a face index lies outside [0, V)");
        return PSI_EINVAL;
    }
    psi_raster_bodies *b = new psi_raster_bodies();
    b->V = V;
    b->F = F;
    PsiBlob T;
    T.upload(b->faces, hf.data(), (size_t)F * 12);
    T.upload(b->voff, voff.data(), ((size_t)V + 1) * 4);
    T.upload(b->vface, vface.data(), (size_t)F * 12);
    if (int rc = psi_blob_realise(T, &b->blob, "psi_raster_bodies_create")) {
        delete b;
        return rc;
    }
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        psi_set_error("psi_raster_bodies_create failed: %s", hipGetErrorString(e));
        psi_raster_bodies_destroy(b);
        return (int)e;
    }
    *out = b;
    return 0;
}

extern "C" void psi_raster_bodies_destroy(psi_raster_bodies *b)
{
    if (!b) return;
    (void)hipFree(b->blob);
    rs_free_grown_bins(b->bins_extra);
    delete b;
}

extern "C" int psi_raster_bodies_normals(psi_raster_bodies *b, const float *d_bverts, int B, float *d_normals, void *stream)
{
    PSI_REQUIRE(b && d_normals && B >= 0 && (d_bverts || B == 0), "null pointer or B < 0");
    const long total = (long)B * b->V;
    PSI_REQUIRE(total < (1L << 31) * 256, "B * V too large for one launch");
    if (total == 0) return 0;
    hipLaunchKernelGGL(rb_normals_kernel, dim3(psi_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, *b, d_bverts, total, d_normals);
    PSI_CHECK_LAUNCH("rb_normals_kernel");
    return 0;
}

extern "C" size_t psi_raster_bodies_workspace_bytes(int F, int draws_per_pass, int n_views, int W, int H)
{
    Layout L;
    return layout(F, draws_per_pass, n_views, W, H, L) ? L.bytes : 0;
}

extern "C" int psi_raster_bodies_render(psi_raster_mesh *scene, const float *d_vrgb, psi_raster_bodies *b, const float *d_bverts, int B,
                                        const int32_t *d_draw_body, const int32_t *d_draw_view, const float *d_draw_rgb, int M, const float *d_w2c,
                                        const float *d_intr, int n_views, int W, int H, float near_, const float *d_sdepth, const int32_t *d_stri,
                                        float bg_r, float bg_g, float bg_b, int draws_per_pass, uint8_t *d_rgb, float *d_depth, int32_t *d_draw,
                                        float *d_bdepth, int32_t *d_bid, int32_t *d_counts, int32_t *d_stats, void *d_workspace, void *stream)
{
    PSI_REQUIRE(b && d_w2c && d_intr && d_rgb && d_depth && d_draw && d_bdepth && d_bid && d_stats, "null pointer");
    PSI_REQUIRE(M >= 0 && B >= 0, "M >= 0, B >= 0");
    PSI_REQUIRE(M == 0 || (d_bverts && d_draw_body && d_draw_view && d_draw_rgb && d_counts), "null pointer with M > 0");
    PSI_REQUIRE((long long)M * b->F < (1LL << 31), "M * F < 2^31 (the piece index is 31 bits of the key)");
    PSI_REQUIRE(!d_sdepth == !d_stri && (!d_stri || scene) && (!d_vrgb || scene), "the scene's depth and tri images come together, with its mesh");
    PSI_REQUIRE(n_views >= 1 && n_views <= 65535, "1 <= n_views <= 65535");
    PSI_REQUIRE(W >= 1 && H >= 1 && W <= 4096 && H <= 4096, "image sizes 1..4096");
    PSI_REQUIRE(near_ > 0.0f, "near > 0");
    Layout L;
    PSI_REQUIRE(layout(b->F, draws_per_pass, n_views, W, H, L), "draws_per_pass >= 1 and draws_per_pass * F < 2^30");
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)d_workspace;
    if (!ws) {
        ws = (char *)psi_scratch(L.bytes, st);
        if (!ws) return PSI_ENOMEM;
    }
    const BinRegions R(L, ws);
    int *pstats = (int *)(ws + L.o_pstats), *d_bad = (int *)(ws + L.o_bad);
    unsigned long long *keys = (unsigned long long *)(ws + L.o_keys);
    const Draws dr = {d_draw_body, d_draw_view, d_draw_rgb, d_bverts};

    PSI_CHECK_HIP(hipMemsetAsync(keys, 0xff, (size_t)n_views * W * H * 8, st));
    PSI_CHECK_HIP(hipMemsetAsync(d_stats, 0, (size_t)n_views * 8, st));
    if (M > 0) {
        PSI_CHECK_HIP(hipMemsetAsync(d_counts, 0, (size_t)M * 8, st));
        PSI_CHECK_HIP(hipMemsetAsync(d_bad, 0, 4, st));
        hipLaunchKernelGGL(rb_check_draws_kernel, dim3(psi_cdiv(M, 256)), dim3(256), 0, st, d_draw_body, d_draw_view, M, B, n_views, d_bad);
        PSI_CHECK_LAUNCH("rb_check_draws_kernel");
    }
    for (int d0 = 0; d0 < M; d0 += L.dpp) {
        const int nd = std::min(L.dpp, M - d0);
        PSI_CHECK_HIP(hipMemsetAsync(R.tcount, 0, L.count_bytes(), st));
        hipLaunchKernelGGL(rb_setup_kernel, dim3(psi_cdiv(b->F, 256), nd), dim3(256), 0, st, *b, dr, d0, B, n_views, d_w2c, d_intr, W, H, near_, L.tiles_x,
                           L.ntiles, R.recs, R.pbox, R.tcount, d_stats);
        PSI_CHECK_LAUNCH("rb_setup_kernel");
        int *pass_bins = nullptr;
        if (int rc = rs_bin_pass("psi_raster_bodies_render", L, R, b->bins_extra, n_views, pstats, d0 == 0 ? d_bad : nullptr,
                                 "a draw's body lies outside [0, B) or its view outside [0, n_views)", nd, 2 * b->F, d_draw_view, d0, st, &pass_bins))
            return rc;
        hipLaunchKernelGGL(rb_tile_kernel, dim3(L.ntiles, n_views), dim3(WG), 0, st, W, H, L.tiles_x, L.ntiles, R.recs, R.tcount, R.toff, R.vbase, pass_bins,
                           pstats, d_stats, keys);
        PSI_CHECK_LAUNCH("rb_tile_kernel");
    }
    Scene sc;
    sc.mesh = scene ? *scene : psi_raster_mesh();
    sc.vrgb = d_vrgb;
    sc.depth = d_sdepth;
    sc.tri = d_stri;
    hipLaunchKernelGGL(rb_compose_kernel, dim3(psi_cdiv((long)W * H, 256), n_views), dim3(256), 0, st, sc, *b, dr, d_w2c, d_intr, W, H, near_, keys, bg_r, bg_g,
                       bg_b, d_rgb, d_depth, d_draw, d_bdepth, d_bid, d_counts);
    PSI_CHECK_LAUNCH("rb_compose_kernel");
    return 0;
}
