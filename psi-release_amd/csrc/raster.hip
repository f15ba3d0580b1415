// Depth / triangle-id / label snapshots of a triangle mesh for gfx950 (wave64): a tile-binned rasteriser that replaces the OpenGL window
// of the reference's snapshot tool (utils/utils_prox_snapshots_virtualcam.py: capture_depth_float_buffer / capture_screen_float_buffer).
//
// Arithmetic contract (include/psi_hip.h, DESIGN.md "Snapshot rasteriser"; this file is compiled with -ffp-contract=off):
//   camera space   xc = ((m00*X + m01*Y) + m02*Z) + m03   (fp32, this association; yc, zc alike)
//   near clip      vertex inside <=> zc >= near; a new vertex from the inside vertex a towards the outside vertex b:
//                  t = (near - za) / (zb - za),  p = a + t*(b - a)  (x, y, z and the label), so two triangles that share an edge get the
//                  identical point; a triangle becomes 0, 1 or 2 pieces, which keep its index
//   projection     u = (fx*xc)/zc + cx,  U = (int)rintf(u*256)   (8 sub-pixel bits, round half to even; IEEE division); v / V alike
//   guard          a piece with |U| or |V| above 2^28 is not drawn (counted); integer area 0 is dropped; area < 0 is re-wound
//   coverage       sample (256*px + 128, 256*py + 128), int64 edge functions, top-left rule: exact, so a sample on a shared edge belongs
//                  to exactly one of the two pieces
//   depth          li = (float)ei / (float)area,  1/z = (l0*(1/z0) + l1*(1/z1)) + l2*(1/z2),  z = 1 / (1/z)
//   visibility     key = (bits of z) << 32 | triangle index, the pixel keeps the minimum key: independent of the order of the pieces
//   label          seg = z * ((l0*(lab0/z0) + l1*(lab1/z1)) + l2*(lab2/z2))
//
// Launches of one psi_raster_render call (all views at once; the view is a grid dimension):
//   rs_setup    one lane per (view, triangle): pieces -> 48-byte records, their tile boxes, per-tile counts (integer atomics)
//   rs_scan, rs_view_base, the one host read of the call (the views' pair counts), rs_fill: the binning pass both rasterisers share
//               (raster_bins.h: rs_bin_pass); a row of rs_fill is a view, the bin entry the piece slot within the view
//   rs_tile     one workgroup per (view, 16x16 tile): the z-buffer of the tile as 256 64-bit keys in LDS; the bin is streamed in chunks
//               of 256 pieces, one record per lane, read once.  A piece whose box covers few pixels of the tile is rasterised by its own
//               lane (LDS atomic minimum); the others are put in an LDS list and rasterised by the whole workgroup, one lane per pixel.
//               Then the resolve: depth and id from the key; the label by setting the winning triangle up again (same arithmetic, so
//               the same pieces) and interpolating the piece that covers the pixel.
// No floating-point atomics and no global atomics on the pixel path.
#include "raster_bins.h"
#include "blob.h"

namespace {

typedef CamVertT<1> CamVert;   // the one attribute of a snapshot vertex is its label

RS_FN void load_triangle(const psi_raster_mesh &mesh, const View &vw, int tri, CamVert &v0, CamVert &v1, CamVert &v2)
{
    const int a = mesh.faces[(size_t)tri * 3 + 0], b = mesh.faces[(size_t)tri * 3 + 1], c = mesh.faces[(size_t)tri * 3 + 2];
    v0 = to_camera<1>(vw, mesh.verts + (size_t)a * 3);
    v1 = to_camera<1>(vw, mesh.verts + (size_t)b * 3);
    v2 = to_camera<1>(vw, mesh.verts + (size_t)c * 3);
    v0.a[0] = mesh.vlabel ? mesh.vlabel[a] : 0.0f;
    v1.a[0] = mesh.vlabel ? mesh.vlabel[b] : 0.0f;
    v2.a[0] = mesh.vlabel ? mesh.vlabel[c] : 0.0f;
}

// the label of pixel (px, py), won by triangle tri at depth bits zbits: seg = z * ((l0*(lab0/z0) + l1*(lab1/z1)) + l2*(lab2/z2))
RS_FN float label_at(const psi_raster_mesh &mesh, const View &vw, float near_, int tri, int px, int py, unsigned zbits)
{
    CamVert v0, v1, v2;
    load_triangle(mesh, vw, tri, v0, v1, v2);
    float num, z;
    return attributes_at<1>(vw, near_, v0, v1, v2, px, py, zbits, &num, &z) ? z * num : 0.0f;
}

// piece slot of (triangle t, piece k) of a view: k * nf + t, so the rarely used second slots lie together
__global__ __launch_bounds__(256) void rs_setup_kernel(psi_raster_mesh mesh, const float *__restrict__ w2c, const float *__restrict__ intr, int W, int H,
                                                       float near_, int tiles_x, int ntiles, PieceRec *__restrict__ recs,
                                                       unsigned *__restrict__ pbox, int *__restrict__ tcount, int *__restrict__ stats)
{
    const int view = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= mesh.nf) return;
    const View vw = load_view(w2c, intr, view);
    CamVert v0, v1, v2;
    load_triangle(mesh, vw, t, v0, v1, v2);
    PieceT<1> pc[2];
    int dropped = 0;
    const int n = setup_triangle(vw, near_, v0, v1, v2, pc, &dropped);
    if (dropped) atomicAdd(&stats[view * 2 + 1], dropped);
    const size_t vslot = (size_t)view * 2 * mesh.nf;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const size_t slot = vslot + (size_t)k * mesh.nf + t;
        PieceRec r;
        const unsigned box = k < n ? piece_record(pc[k], t, W, H, r) : NOBOX;
        if (box != NOBOX) {
            recs[slot] = r;
            count_box_tiles(box, view, tiles_x, ntiles, tcount);
        }
        pbox[slot] = box;
    }
}

__global__ __launch_bounds__(WG) void rs_tile_kernel(psi_raster_mesh mesh, const float *__restrict__ w2c, const float *__restrict__ intr, int W, int H,
                                                     float near_, int tiles_x, int ntiles, const PieceRec *__restrict__ recs,
                                                     const int *__restrict__ tcount, const int *__restrict__ toff, const long long *__restrict__ vbase,
                                                     const int *__restrict__ bins, float *__restrict__ depth, int *__restrict__ tri_out,
                                                     float *__restrict__ seg)
{
    const int view = blockIdx.y, tile = blockIdx.x, t = threadIdx.x;
    const int tpx = (tile % tiles_x) * TILE, tpy = (tile / tiles_x) * TILE;        // the tile's first pixel
    __shared__ unsigned long long zbuf[WG];
    __shared__ PieceRec big[WG];
    __shared__ int nbig;
    const int n = tcount[(size_t)view * ntiles + tile];
    const int *__restrict__ bin = bins + vbase[view] + toff[(size_t)view * ntiles + tile];
    const PieceRec *__restrict__ vrecs = recs + (size_t)view * 2 * mesh.nf;
    const int px = tpx + (t & (TILE - 1)), py = tpy + t / TILE;                      // this lane's pixel in the one-lane-per-pixel phase
    const bool live = px < W && py < H;
    const unsigned long long key = tile_nearest_key(vrecs, bin, n, W, H, tpx, tpy, px, py, live, zbuf, big, &nbig);
    if (!live) return;
    const size_t o = ((size_t)view * H + py) * W + px;
    if (key == ~0ull) {
        depth[o] = 0.0f;
        tri_out[o] = -1;
        if (seg) seg[o] = 0.0f;
        return;
    }
    const float z = __uint_as_float((unsigned)(key >> 32));
    const int tri = (int)(unsigned)(key & 0xffffffffu);
    depth[o] = z;
    tri_out[o] = tri;
    if (!seg) return;
    seg[o] = label_at(mesh, load_view(w2c, intr, view), near_, tri, px, py, (unsigned)(key >> 32));
}

__global__ __launch_bounds__(256) void rs_check_faces_kernel(const int *__restrict__ faces, long n, int nv, int *__restrict__ bad)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n && (faces[i] < 0 || faces[i] >= nv)) atomicOr(bad, 1);
}

BinLayout layout(int nf, int n_views, int W, int H)
{
    BinLayout L;
    L.begin((size_t)n_views * 2 * nf, n_views, W, H);
    L.place_bins();
    return L;
}

}  // namespace

extern "C" int psi_raster_mesh_create(psi_raster_mesh **out, const float *d_verts, const int32_t *d_faces, const float *d_vlabel, int nv, int nf)
{
    PSI_REQUIRE(out && d_verts && d_faces, "null pointer");
    PSI_REQUIRE(nv >= 1 && nf >= 1 && (long)nf * 2 < (1L << 30), "nv >= 1, 1 <= nf < 2^29");
    // a one-off between two device synchronisations: the inputs may have been produced on any stream
    PSI_CHECK_HIP(hipDeviceSynchronize());
    psi_raster_mesh *m = new psi_raster_mesh();
    m->nv = nv;
    m->nf = nf;
    int *d_bad = nullptr;
    int bad = 0;
    // room for the labels and the flag word whether or not labels are given
    PsiBlob T;
    T.copy(m->verts, d_verts, (size_t)nv * 12);
    T.copy(m->faces, d_faces, (size_t)nf * 12);
    T.copy(m->vlabel, d_vlabel, d_vlabel ? (size_t)nv * 4 : 0, (size_t)nv * 4).or_null();
    T.zero(d_bad, 4);
    if (int rc = psi_blob_realise(T, &m->blob, "psi_raster_mesh_create")) {
        delete m;
        return rc;
    }
    hipLaunchKernelGGL(rs_check_faces_kernel, dim3(psi_cdiv((long)nf * 3, 256)), dim3(256), 0, 0, m->faces, (long)nf * 3, nv, d_bad);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(&bad, d_bad, 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess || bad) {
        if (bad) psi_set_error("psi_raster_mesh_create: a face index lies outside [0, nv)");
        else psi_set_error("psi_raster_mesh_create failed: %s", hipGetErrorString(e));
        psi_raster_mesh_destroy(m);
        return bad ? PSI_EINVAL : (int)e;
    }
    *out = m;
    return 0;
}

extern "C" void psi_raster_mesh_destroy(psi_raster_mesh *m)
{
    if (!m) return;
    (void)hipFree(m->blob);
    rs_free_grown_bins(m->bins_extra);
    delete m;
}

extern "C" size_t psi_raster_workspace_bytes(int nf, int n_views, int W, int H)
{
    if (nf <= 0 || n_views <= 0 || W <= 0 || H <= 0) return 0;
    return layout(nf, n_views, W, H).bytes;
}

extern "C" int psi_raster_render(psi_raster_mesh *m, const float *d_w2c, const float *d_intr, int n_views, int W, int H, float near_,
                                 float *d_depth, int32_t *d_tri, float *d_seg, int32_t *d_stats, void *d_workspace, void *stream)
{
    PSI_REQUIRE(m && d_w2c && d_intr && d_depth && d_tri && d_stats, "null pointer");
    PSI_REQUIRE(n_views >= 1 && n_views <= 65535, "1 <= n_views <= 65535");
    PSI_REQUIRE(W >= 1 && H >= 1 && W <= 4096 && H <= 4096, "image sizes 1..4096");
    PSI_REQUIRE(near_ > 0.0f, "near > 0");
    hipStream_t st = (hipStream_t)stream;
    const BinLayout L = layout(m->nf, n_views, W, H);
    char *ws = (char *)d_workspace;
    if (!ws) {
        ws = (char *)psi_scratch(L.bytes, st);
        if (!ws) return PSI_ENOMEM;
    }
    const BinRegions R(L, ws);

    PSI_CHECK_HIP(hipMemsetAsync(R.tcount, 0, L.count_bytes(), st));
    PSI_CHECK_HIP(hipMemsetAsync(d_stats, 0, (size_t)n_views * 8, st));
    hipLaunchKernelGGL(rs_setup_kernel, dim3(psi_cdiv(m->nf, 256), n_views), dim3(256), 0, st, *m, d_w2c, d_intr, W, H, near_, L.tiles_x, L.ntiles,
                       R.recs, R.pbox, R.tcount, d_stats);
    PSI_CHECK_LAUNCH("rs_setup_kernel");
    int *bins = nullptr;
    if (int rc = rs_bin_pass("psi_raster_render", L, R, m->bins_extra, n_views, d_stats, nullptr, nullptr, n_views, 2 * m->nf, nullptr, 0, st, &bins))
        return rc;
    hipLaunchKernelGGL(rs_tile_kernel, dim3(L.ntiles, n_views), dim3(WG), 0, st, *m, d_w2c, d_intr, W, H, near_, L.tiles_x, L.ntiles, R.recs, R.tcount,
                       R.toff, R.vbase, bins, d_depth, d_tri, d_seg);
    PSI_CHECK_LAUNCH("rs_tile_kernel");
    return 0;
}
