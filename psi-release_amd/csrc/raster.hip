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
//   rs_scan     one workgroup per view: exclusive prefix sum of the view's tile counts, the view's number of (tile, piece) pairs
//   rs_fill     one lane per (view, piece slot): piece ids into the bins (integer atomics; the order inside a bin is free)
//   rs_tile     one workgroup per (view, 16x16 tile): the z-buffer of the tile as 256 64-bit keys in LDS; the bin is streamed in chunks
//               of 256 pieces, one record per lane, read once.  A piece whose box covers few pixels of the tile is rasterised by its own
//               lane (LDS atomic minimum); the others are put in an LDS list and rasterised by the whole workgroup, one lane per pixel.
//               Then the resolve: depth and id from the key; the label by setting the winning triangle up again (same arithmetic, so
//               the same pieces) and interpolating the piece that covers the pixel.
// No floating-point atomics and no global atomics on the pixel path.
#include "psi_common.h"
#include <math.h>
#include <vector>

#pragma clang fp contract(off)

struct psi_raster_mesh {
    float *verts;      // [nv][3]   owned copies
    int *faces;        // [nf][3]
    float *vlabel;     // [nv] or nullptr
    int nv, nf;
    void *bins_extra;  // grown on demand when a call's (tile, piece) pairs exceed what its workspace holds
    size_t bins_extra_bytes;
};

namespace {

constexpr int TILE = 16;             // pixels per tile edge
constexpr int WG = TILE * TILE;      // lanes per tile workgroup = pieces per chunk of the bin stream
constexpr int SMALL_BOX = 8;         // a piece whose box covers at most this many pixels of the tile is rasterised by its own lane
constexpr int SUB = 256;             // sub-pixel steps per pixel
constexpr float GUARD = 268435456.f; // 2^28
constexpr unsigned NOBOX = 0x000000ffu;  // tx0 = 255 with tx1 = 0: no piece has tx0 > tx1, so no packed tile box equals it

// the arithmetic helpers are host + device functions: a serial host program can run the very same statements (plain '/' is the IEEE
// division on the host; on the device __fdiv_rn asks for it whatever the build's division mode)
#define RS_FN __host__ __device__ __forceinline__
#ifdef __HIP_DEVICE_COMPILE__
#define RS_DIV(a, b) __fdiv_rn((a), (b))
#else
#define RS_DIV(a, b) ((a) / (b))
#endif

struct __attribute__((aligned(16))) PieceRec {   // 48 bytes = 3 x 16
    int U0, V0, U1, V1;
    int U2, V2, tri, pad0;
    float iz0, iz1, iz2, pad1;
};
static_assert(sizeof(PieceRec) == 48, "setup records are 16-byte multiples");

struct CamVert {
    float x, y, z, l;
};

struct Piece {
    int U[3], V[3];
    float iz[3], lab[3];
};

struct View {
    float m[12];
    float fx, fy, cx, cy;
};

RS_FN View load_view(const float *__restrict__ w2c, const float *__restrict__ intr, int view)
{
    View vw;
#pragma unroll
    for (int i = 0; i < 12; i++) vw.m[i] = w2c[(size_t)view * 12 + i];
    vw.fx = intr[view * 4 + 0];
    vw.fy = intr[view * 4 + 1];
    vw.cx = intr[view * 4 + 2];
    vw.cy = intr[view * 4 + 3];
    return vw;
}

RS_FN CamVert to_camera(const View &vw, const float *__restrict__ p, float label)
{
    const float X = p[0], Y = p[1], Z = p[2];
    CamVert c;
    c.x = ((vw.m[0] * X + vw.m[1] * Y) + vw.m[2] * Z) + vw.m[3];
    c.y = ((vw.m[4] * X + vw.m[5] * Y) + vw.m[6] * Z) + vw.m[7];
    c.z = ((vw.m[8] * X + vw.m[9] * Y) + vw.m[10] * Z) + vw.m[11];
    c.l = label;
    return c;
}

// the point of edge a -> b on z = near, always from the inside vertex a
RS_FN CamVert clip_point(const CamVert &a, const CamVert &b, float near_)
{
    const float t = RS_DIV(near_ - a.z, b.z - a.z);
    CamVert p;
    p.x = a.x + t * (b.x - a.x);
    p.y = a.y + t * (b.y - a.y);
    p.z = a.z + t * (b.z - a.z);
    p.l = a.l + t * (b.l - a.l);
    return p;
}

struct Snapped {
    int U, V;
    float iz, l;
    bool ok;
};

RS_FN Snapped project(const View &vw, const CamVert &c)
{
    const float u = RS_DIV(vw.fx * c.x, c.z) + vw.cx;
    const float v = RS_DIV(vw.fy * c.y, c.z) + vw.cy;
    const float ru = rintf(u * (float)SUB), rv = rintf(v * (float)SUB);
    Snapped s;
    s.ok = fabsf(ru) <= GUARD && fabsf(rv) <= GUARD;       // false for NaN / inf too
    s.U = s.ok ? (int)ru : 0;
    s.V = s.ok ? (int)rv : 0;
    s.iz = RS_DIV(1.0f, c.z);
    s.l = c.l;
    return s;
}

RS_FN long long edge_fn(int ax, int ay, int bx, int by, int px, int py)
{
    return (long long)(bx - ax) * (long long)(py - ay) - (long long)(by - ay) * (long long)(px - ax);
}

// one piece from three snapped vertices: false when it is not drawn (guard: counted in *dropped; zero area: not counted)
RS_FN bool make_piece(const Snapped &a, const Snapped &b, const Snapped &c, Piece &out, int *dropped)
{
    if (!(a.ok && b.ok && c.ok)) {
        *dropped += 1;
        return false;
    }
    const long long area = edge_fn(a.U, a.V, b.U, b.V, c.U, c.V);
    if (area == 0) return false;
    const bool flip = area < 0;                            // both windings are drawn: re-wind to positive area
    const Snapped &p1 = flip ? c : b, &p2 = flip ? b : c;
    out.U[0] = a.U; out.V[0] = a.V; out.iz[0] = a.iz; out.lab[0] = a.l;
    out.U[1] = p1.U; out.V[1] = p1.V; out.iz[1] = p1.iz; out.lab[1] = p1.l;
    out.U[2] = p2.U; out.V[2] = p2.V; out.iz[2] = p2.iz; out.lab[2] = p2.l;
    return true;
}

// stage (a) for one (view, triangle): number of drawn pieces (0..2) in out[]
RS_FN int setup_triangle(const View &vw, float near_, const CamVert &v0, const CamVert &v1, const CamVert &v2, Piece out[2],
                                              int *dropped)
{
    const bool i0 = v0.z >= near_, i1 = v1.z >= near_, i2 = v2.z >= near_;
    const int nin = (int)i0 + (int)i1 + (int)i2;
    if (nin == 0) return 0;
    int n = 0;
    if (nin == 3) {
        n += make_piece(project(vw, v0), project(vw, v1), project(vw, v2), out[n], dropped) ? 1 : 0;
    } else if (nin == 1) {
        // a inside, b and c (the next two in cyclic order) outside: (a, ab, ac)
        const CamVert &a = i0 ? v0 : (i1 ? v1 : v2), &b = i0 ? v1 : (i1 ? v2 : v0), &c = i0 ? v2 : (i1 ? v0 : v1);
        n += make_piece(project(vw, a), project(vw, clip_point(a, b, near_)), project(vw, clip_point(a, c, near_)), out[n], dropped) ? 1 : 0;
    } else {
        // c outside, a and b (the next two in cyclic order) inside: the quad (a, b, bc, ac) as (a, b, bc) and (a, bc, ac)
        const CamVert &c = !i0 ? v0 : (!i1 ? v1 : v2), &a = !i0 ? v1 : (!i1 ? v2 : v0), &b = !i0 ? v2 : (!i1 ? v0 : v1);
        const Snapped sa = project(vw, a), sb = project(vw, b), sbc = project(vw, clip_point(b, c, near_)),
                      sac = project(vw, clip_point(a, c, near_));
        n += make_piece(sa, sb, sbc, out[n], dropped) ? 1 : 0;
        n += make_piece(sa, sbc, sac, out[n], dropped) ? 1 : 0;
    }
    return n;
}

RS_FN int imin2(int a, int b) { return a < b ? a : b; }
RS_FN int imax2(int a, int b) { return a > b ? a : b; }
RS_FN int imin3(int a, int b, int c) { return imin2(a, imin2(b, c)); }
RS_FN int imax3(int a, int b, int c) { return imax2(a, imax2(b, c)); }

// pixels whose sample can lie in the box of the snapped vertices, clipped to the image: false when there are none
RS_FN bool pixel_box(int U0, int V0, int U1, int V1, int U2, int V2, int W, int H, int &x0, int &y0, int &x1, int &y1)
{
    x0 = imax2(0, (imin3(U0, U1, U2) - SUB / 2 + SUB - 1) >> 8);
    x1 = imin2(W - 1, (imax3(U0, U1, U2) - SUB / 2) >> 8);
    y0 = imax2(0, (imin3(V0, V1, V2) - SUB / 2 + SUB - 1) >> 8);
    y1 = imin2(H - 1, (imax3(V0, V1, V2) - SUB / 2) >> 8);
    return x0 <= x1 && y0 <= y1;
}

// top-left rule for an edge a -> b of a positive-area piece: a sample ON the edge is inside for exactly one of the two directions
RS_FN bool edge_owns_tie(int ax, int ay, int bx, int by)
{
    const int dx = bx - ax, dy = by - ay;
    return dy > 0 || (dy == 0 && dx < 0);
}

// coverage of pixel (px, py) by a positive-area piece; the three edge values (e0 opposite vertex 0, ...) when covered
RS_FN bool cover(int U0, int V0, int U1, int V1, int U2, int V2, int px, int py, long long &e0, long long &e1, long long &e2)
{
    const int sx = px * SUB + SUB / 2, sy = py * SUB + SUB / 2;
    e0 = edge_fn(U1, V1, U2, V2, sx, sy);
    e1 = edge_fn(U2, V2, U0, V0, sx, sy);
    e2 = edge_fn(U0, V0, U1, V1, sx, sy);
    if ((e0 | e1 | e2) < 0) return false;
    return (e0 > 0 || edge_owns_tie(U1, V1, U2, V2)) && (e1 > 0 || edge_owns_tie(U2, V2, U0, V0)) && (e2 > 0 || edge_owns_tie(U0, V0, U1, V1));
}

RS_FN void barycentric(long long e0, long long e1, long long e2, float &l0, float &l1, float &l2)
{
    const float area = (float)(e0 + e1 + e2);
    l0 = RS_DIV((float)e0, area);
    l1 = RS_DIV((float)e1, area);
    l2 = RS_DIV((float)e2, area);
}

RS_FN bool pixel_key(const PieceRec &r, int px, int py, unsigned long long &key)
{
    long long e0, e1, e2;
    if (!cover(r.U0, r.V0, r.U1, r.V1, r.U2, r.V2, px, py, e0, e1, e2)) return false;
    float l0, l1, l2;
    barycentric(e0, e1, e2, l0, l1, l2);
    const float invz = (l0 * r.iz0 + l1 * r.iz1) + l2 * r.iz2;
    const float z = RS_DIV(1.0f, invz);
    key = ((unsigned long long)__builtin_bit_cast(unsigned, z) << 32) | (unsigned)r.tri;
    return true;
}

RS_FN unsigned pack_box(int tx0, int ty0, int tx1, int ty1)
{
    return (unsigned)tx0 | ((unsigned)ty0 << 8) | ((unsigned)tx1 << 16) | ((unsigned)ty1 << 24);
}

RS_FN void load_triangle(const psi_raster_mesh &mesh, const View &vw, int tri, CamVert &v0, CamVert &v1, CamVert &v2)
{
    const int a = mesh.faces[(size_t)tri * 3 + 0], b = mesh.faces[(size_t)tri * 3 + 1], c = mesh.faces[(size_t)tri * 3 + 2];
    v0 = to_camera(vw, mesh.verts + (size_t)a * 3, mesh.vlabel ? mesh.vlabel[a] : 0.0f);
    v1 = to_camera(vw, mesh.verts + (size_t)b * 3, mesh.vlabel ? mesh.vlabel[b] : 0.0f);
    v2 = to_camera(vw, mesh.verts + (size_t)c * 3, mesh.vlabel ? mesh.vlabel[c] : 0.0f);
}

// the label of pixel (px, py), won by triangle tri at depth bits zbits: the triangle set up again (the same statements on the same inputs,
// hence the same pieces), interpolated on the piece that covers the pixel
RS_FN float label_at(const psi_raster_mesh &mesh, const View &vw, float near_, int tri, int px, int py, unsigned zbits)
{
    CamVert v0, v1, v2;
    load_triangle(mesh, vw, tri, v0, v1, v2);
    Piece pc[2];
    int dropped = 0;
    const int np = setup_triangle(vw, near_, v0, v1, v2, pc, &dropped);
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        long long e0, e1, e2;
        if (k < np && cover(pc[k].U[0], pc[k].V[0], pc[k].U[1], pc[k].V[1], pc[k].U[2], pc[k].V[2], px, py, e0, e1, e2)) {
            float l0, l1, l2;
            barycentric(e0, e1, e2, l0, l1, l2);
            const float invz = (l0 * pc[k].iz[0] + l1 * pc[k].iz[1]) + l2 * pc[k].iz[2];
            const float zk = RS_DIV(1.0f, invz);
            const float num = (l0 * (pc[k].lab[0] * pc[k].iz[0]) + l1 * (pc[k].lab[1] * pc[k].iz[1])) + l2 * (pc[k].lab[2] * pc[k].iz[2]);
            if (__builtin_bit_cast(unsigned, zk) == zbits) s = zk * num;
        }
    }
    return s;
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
    Piece pc[2];
    int dropped = 0;
    const int n = setup_triangle(vw, near_, v0, v1, v2, pc, &dropped);
    if (dropped) atomicAdd(&stats[view * 2 + 1], dropped);
    const size_t vslot = (size_t)view * 2 * mesh.nf;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const size_t slot = vslot + (size_t)k * mesh.nf + t;
        unsigned box = NOBOX;
        int x0, y0, x1, y1;
        if (k < n && pixel_box(pc[k].U[0], pc[k].V[0], pc[k].U[1], pc[k].V[1], pc[k].U[2], pc[k].V[2], W, H, x0, y0, x1, y1)) {
            PieceRec r;
            r.U0 = pc[k].U[0]; r.V0 = pc[k].V[0]; r.U1 = pc[k].U[1]; r.V1 = pc[k].V[1];
            r.U2 = pc[k].U[2]; r.V2 = pc[k].V[2]; r.tri = t; r.pad0 = 0;
            r.iz0 = pc[k].iz[0]; r.iz1 = pc[k].iz[1]; r.iz2 = pc[k].iz[2]; r.pad1 = 0.0f;
            recs[slot] = r;
            const int tx0 = x0 / TILE, tx1 = x1 / TILE, ty0 = y0 / TILE, ty1 = y1 / TILE;
            box = pack_box(tx0, ty0, tx1, ty1);
            for (int ty = ty0; ty <= ty1; ty++)
                for (int tx = tx0; tx <= tx1; tx++) atomicAdd(&tcount[(size_t)view * ntiles + ty * tiles_x + tx], 1);
        }
        pbox[slot] = box;
    }
}

// exclusive prefix sum of one view's tile counts (one workgroup per view, chunks of 256 in tile order)
__global__ __launch_bounds__(256) void rs_scan_kernel(const int *__restrict__ tcount, int ntiles, int *__restrict__ toff, int *__restrict__ stats)
{
    const int view = blockIdx.x, t = threadIdx.x;
    __shared__ long long part[256];
    __shared__ long long carry;                              // 64-bit: a view whose pairs exceed an int is reported, not wrapped
    if (t == 0) carry = 0;
    __syncthreads();
    for (int c0 = 0; c0 < ntiles; c0 += 256) {
        const int i = c0 + t;
        const int v = i < ntiles ? tcount[(size_t)view * ntiles + i] : 0;
        part[t] = v;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {                  // inclusive Hillis-Steele scan of the chunk
            const long long add = t >= o ? part[t - o] : 0;
            __syncthreads();
            part[t] += add;
            __syncthreads();
        }
        if (i < ntiles) toff[(size_t)view * ntiles + i] = (int)(carry + part[t] - v);   // meaningless past 2^31, where the call is refused
        __syncthreads();
        if (t == 255) carry += part[255];
        __syncthreads();
    }
    if (t == 0) stats[view * 2 + 0] = carry > 0x7fffffffLL ? -1 : (int)carry;          // -1: the host refuses the call before any bin is filled
}

// first bin entry of every view: the views' pair counts summed in view order
__global__ __launch_bounds__(64) void rs_view_base_kernel(const int *__restrict__ stats, int n_views, long long *__restrict__ vbase)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    long long a = 0;
    for (int v = 0; v < n_views; v++) {
        vbase[v] = a;
        a += stats[v * 2 + 0];
    }
}

__global__ __launch_bounds__(256) void rs_fill_kernel(int nf, int tiles_x, int ntiles, const unsigned *__restrict__ pbox, const int *__restrict__ toff,
                                                      const long long *__restrict__ vbase, int *__restrict__ tcursor, int *__restrict__ bins)
{
    const int view = blockIdx.y;
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= 2 * nf) return;
    const unsigned box = pbox[(size_t)view * 2 * nf + s];
    if (box == NOBOX) return;
    const int tx0 = box & 255, ty0 = (box >> 8) & 255, tx1 = (box >> 16) & 255, ty1 = box >> 24;
    int *base = bins + vbase[view];
    for (int ty = ty0; ty <= ty1; ty++)
        for (int tx = tx0; tx <= tx1; tx++) {
            const size_t tile = (size_t)view * ntiles + ty * tiles_x + tx;
            const int pos = atomicAdd(&tcursor[tile], 1);
            base[toff[tile] + pos] = s;
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
    zbuf[t] = ~0ull;
    const int n = tcount[(size_t)view * ntiles + tile];
    const int *__restrict__ bin = bins + vbase[view] + toff[(size_t)view * ntiles + tile];
    const PieceRec *__restrict__ vrecs = recs + (size_t)view * 2 * mesh.nf;
    const int px = tpx + (t & (TILE - 1)), py = tpy + t / TILE;                      // this lane's pixel in the one-lane-per-pixel phase
    const bool live = px < W && py < H;
    unsigned long long mine = ~0ull;
    for (int c0 = 0; c0 < n; c0 += WG) {
        if (t == 0) nbig = 0;
        __syncthreads();
        if (c0 + t < n) {
            const PieceRec r = vrecs[bin[c0 + t]];
            int x0, y0, x1, y1;
            pixel_box(r.U0, r.V0, r.U1, r.V1, r.U2, r.V2, W, H, x0, y0, x1, y1);
            x0 = max(x0, tpx); y0 = max(y0, tpy);
            x1 = min(x1, tpx + TILE - 1); y1 = min(y1, tpy + TILE - 1);
            if ((x1 - x0 + 1) * (y1 - y0 + 1) <= SMALL_BOX) {
                for (int y = y0; y <= y1; y++)
                    for (int x = x0; x <= x1; x++) {
                        unsigned long long key;
                        if (pixel_key(r, x, y, key)) atomicMin(&zbuf[(y - tpy) * TILE + (x - tpx)], key);
                    }
            } else {
                big[atomicAdd(&nbig, 1)] = r;
            }
        }
        __syncthreads();
        const int nb = nbig;
        if (live)
            for (int k = 0; k < nb; k++) {
                unsigned long long key;
                if (pixel_key(big[k], px, py, key)) mine = key < mine ? key : mine;
            }
        __syncthreads();                                     // big / nbig are rewritten by the next chunk
    }
    __syncthreads();
    if (!live) return;
    const unsigned long long lds_key = zbuf[t];
    const unsigned long long key = lds_key < mine ? lds_key : mine;
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

struct Layout {
    size_t o_recs, o_pbox, o_tcount, o_toff, o_tcursor, o_vbase, o_bins, bytes;
    size_t pair_cap;
    int tiles_x, tiles_y, ntiles;
};

Layout layout(int nf, int n_views, int W, int H)
{
    Layout L;
    L.tiles_x = psi_cdiv(W, TILE);
    L.tiles_y = psi_cdiv(H, TILE);
    L.ntiles = L.tiles_x * L.tiles_y;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; };
    const size_t slots = (size_t)n_views * 2 * nf, vt = (size_t)n_views * L.ntiles;
    L.o_recs = take(slots * sizeof(PieceRec));
    L.o_pbox = take(slots * 4);
    L.o_tcount = take(vt * 4);           // tcount and tcursor are adjacent: one memset clears both
    L.o_tcursor = take(vt * 4);
    L.o_toff = take(vt * 4);
    L.o_vbase = take((size_t)n_views * 8);
    // room for the bins: every piece in one tile, plus 64 pieces in every tile (large triangles cover many tiles); a call that needs more
    // takes the bins from a buffer the mesh object owns
    L.pair_cap = (size_t)n_views * ((size_t)2 * nf + (size_t)64 * L.ntiles);
    L.o_bins = take(L.pair_cap * 4);
    L.bytes = o;
    return L;
}

}  // namespace

extern "C" int psi_raster_mesh_create(psi_raster_mesh **out, const float *d_verts, const int32_t *d_faces, const float *d_vlabel, int nv, int nf)
{
    PSI_REQUIRE(out && d_verts && d_faces, "null pointer");
    PSI_REQUIRE(nv >= 1 && nf >= 1 && (long)nf * 2 < (1L << 30), "nv >= 1, 1 <= nf < 2^29");
    psi_raster_mesh *m = new psi_raster_mesh();
    m->nv = nv;
    m->nf = nf;
    const size_t bv = ((size_t)nv * 12 + 255) & ~(size_t)255, bf = ((size_t)nf * 12 + 255) & ~(size_t)255, bl = ((size_t)nv * 4 + 255) & ~(size_t)255;
    char *blob = nullptr;
    int bad = 0;
    // a one-off between two device synchronisations: the inputs may have been produced on any stream
    hipError_t e = hipMalloc((void **)&blob, bv + bf + bl + 256);
    if (e != hipSuccess) {
        psi_set_error("psi_raster_mesh_create: hipMalloc failed: %s", hipGetErrorString(e));
        delete m;
        return (int)e;
    }
    m->verts = (float *)blob;
    m->faces = (int *)(blob + bv);
    m->vlabel = d_vlabel ? (float *)(blob + bv + bf) : nullptr;
    int *d_bad = (int *)(blob + bv + bf + bl);
    e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(m->verts, d_verts, (size_t)nv * 12, hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipMemcpy(m->faces, d_faces, (size_t)nf * 12, hipMemcpyDeviceToDevice);
    if (e == hipSuccess && d_vlabel) e = hipMemcpy(m->vlabel, d_vlabel, (size_t)nv * 4, hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipMemset(d_bad, 0, 4);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(rs_check_faces_kernel, dim3(psi_cdiv((long)nf * 3, 256)), dim3(256), 0, 0, m->faces, (long)nf * 3, nv, d_bad);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(&bad, d_bad, 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess || bad) {
        if (bad) psi_set_error("psi_raster_mesh_create: a face index lies outside [0, nv)");
        else psi_set_error("psi_raster_mesh_create failed: %s", hipGetErrorString(e));
        (void)hipFree(blob);
        delete m;
        return bad ? PSI_EINVAL : (int)e;
    }
    *out = m;
    return 0;
}

extern "C" void psi_raster_mesh_destroy(psi_raster_mesh *m)
{
    if (!m) return;
    (void)hipFree(m->verts);             // the blob's first member
    if (m->bins_extra) (void)hipFree(m->bins_extra);
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
    const Layout L = layout(m->nf, n_views, W, H);
    char *ws = (char *)d_workspace;
    if (!ws) {
        ws = (char *)psi_scratch(L.bytes, st);
        if (!ws) return PSI_ENOMEM;
    }
    PieceRec *recs = (PieceRec *)(ws + L.o_recs);
    unsigned *pbox = (unsigned *)(ws + L.o_pbox);
    int *tcount = (int *)(ws + L.o_tcount), *tcursor = (int *)(ws + L.o_tcursor), *toff = (int *)(ws + L.o_toff);
    long long *vbase = (long long *)(ws + L.o_vbase);
    int *bins = (int *)(ws + L.o_bins);

    PSI_CHECK_HIP(hipMemsetAsync(tcount, 0, L.o_toff - L.o_tcount, st));
    PSI_CHECK_HIP(hipMemsetAsync(d_stats, 0, (size_t)n_views * 8, st));
    hipLaunchKernelGGL(rs_setup_kernel, dim3(psi_cdiv(m->nf, 256), n_views), dim3(256), 0, st, *m, d_w2c, d_intr, W, H, near_, L.tiles_x, L.ntiles,
                       recs, pbox, tcount, d_stats);
    PSI_CHECK_LAUNCH("rs_setup_kernel");
    hipLaunchKernelGGL(rs_scan_kernel, dim3(n_views), dim3(256), 0, st, tcount, L.ntiles, toff, d_stats);
    PSI_CHECK_LAUNCH("rs_scan_kernel");
    hipLaunchKernelGGL(rs_view_base_kernel, dim3(1), dim3(64), 0, st, d_stats, n_views, vbase);
    PSI_CHECK_LAUNCH("rs_view_base_kernel");
    // the bins are sized from the counts: the one host read of the call
    std::vector<int> h_stats((size_t)n_views * 2);
    PSI_CHECK_HIP(hipMemcpyAsync(h_stats.data(), d_stats, (size_t)n_views * 8, hipMemcpyDeviceToHost, st));
    PSI_CHECK_HIP(hipStreamSynchronize(st));
    size_t pairs = 0;
    for (int v = 0; v < n_views; v++) {
        PSI_REQUIRE(h_stats[(size_t)v * 2] >= 0, "a view's (tile, piece) pairs exceed 2^31");
        pairs += (size_t)h_stats[(size_t)v * 2];
    }
    if (pairs > L.pair_cap) {
        if (m->bins_extra_bytes < pairs * 4) {
            if (m->bins_extra) (void)hipFree(m->bins_extra);  // one call at a time per mesh (psi_hip.h) and this call's stream is idle: nothing reads the old buffer
            m->bins_extra = nullptr;
            m->bins_extra_bytes = 0;
            const size_t want = pairs * 4 + pairs;
            hipError_t e = hipMalloc(&m->bins_extra, want);
            if (e != hipSuccess) {
                psi_set_error("psi_raster_render: hipMalloc of %zu bytes for the bins failed: %s", want, hipGetErrorString(e));
                return PSI_ENOMEM;
            }
            m->bins_extra_bytes = want;
        }
        bins = (int *)m->bins_extra;
    }
    hipLaunchKernelGGL(rs_fill_kernel, dim3(psi_cdiv(2L * m->nf, 256), n_views), dim3(256), 0, st, m->nf, L.tiles_x, L.ntiles, pbox, toff, vbase, tcursor,
                       bins);
    PSI_CHECK_LAUNCH("rs_fill_kernel");
    hipLaunchKernelGGL(rs_tile_kernel, dim3(L.ntiles, n_views), dim3(WG), 0, st, *m, d_w2c, d_intr, W, H, near_, L.tiles_x, L.ntiles, recs, tcount, toff,
                       vbase, bins, d_depth, d_tri, d_seg);
    PSI_CHECK_LAUNCH("rs_tile_kernel");
    return 0;
}
