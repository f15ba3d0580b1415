// The statements of the snapshot rasteriser's contract (DESIGN.md "Snapshot rasteriser") as host + device functions, shared by
// raster.hip (scene snapshots) and raster_bodies.hip (bodies composited into them): a serial host program can run the very same
// statements (tools/result_images_host_check.hip).  Include it only from files compiled with -ffp-contract=off.
//
// A vertex carries NA attributes that are interpolated along with it (the near clip's a + t*(b - a), then perspective-correct over the
// piece): the label of the snapshots (NA = 1), a normal or a colour of the result images (NA = 3).
#pragma once
#include "psi_common.h"
#include <math.h>

#pragma clang fp contract(off)

// Bins that a handle owns: grown on demand (raster_bins.h: rs_bin_pass) when the (tile, piece) pairs of a call or pass exceed what its
// workspace holds, kept for the next one, freed with the handle.
struct RsGrownBins {
    void *ptr;
    size_t bytes;
};

static inline void rs_free_grown_bins(RsGrownBins &g)
{
    if (g.ptr) (void)hipFree(g.ptr);
    g.ptr = nullptr;
    g.bytes = 0;
}

struct psi_raster_mesh {
    float *verts;      // [nv][3]   owned copies
    int *faces;        // [nf][3]
    float *vlabel;     // [nv] or nullptr
    int nv, nf;
    RsGrownBins bins_extra;  // for a call whose (tile, piece) pairs exceed its workspace's bins
    char *blob;        // the one allocation behind verts, faces and vlabel
};

namespace {

constexpr int TILE = 16;             // pixels per tile edge
constexpr int WG = TILE * TILE;      // lanes per tile workgroup = pieces per chunk of the bin stream
constexpr int SMALL_BOX = 8;         // a piece whose box covers at most this many pixels of the tile is rasterised by its own lane
constexpr int SUB = 256;             // sub-pixel steps per pixel
constexpr float GUARD = 268435456.f; // 2^28
constexpr unsigned NOBOX = 0x000000ffu;  // tx0 = 255 with tx1 = 0: no piece has tx0 > tx1, so no packed tile box equals it

// plain '/' and sqrtf are the IEEE operations on the host; on the device __fdiv_rn / __fsqrt_rn ask for them whatever the build's mode
#define RS_FN __host__ __device__ __forceinline__
#ifdef __HIP_DEVICE_COMPILE__
#define RS_DIV(a, b) __fdiv_rn((a), (b))
#define RS_SQRT(a) __fsqrt_rn(a)
#else
#define RS_DIV(a, b) ((a) / (b))
#define RS_SQRT(a) sqrtf(a)
#endif

struct __attribute__((aligned(16))) PieceRec {   // 48 bytes = 3 x 16
    int U0, V0, U1, V1;
    int U2, V2, tri, pad0;
    float iz0, iz1, iz2, pad1;
};
static_assert(sizeof(PieceRec) == 48, "setup records are 16-byte multiples");

template <int NA>
struct CamVertT {
    float x, y, z, a[NA];
};

template <int NA>
struct PieceT {
    int U[3], V[3];
    float iz[3], a[3][NA];
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

// position into camera space; the attributes are the caller's
template <int NA>
RS_FN CamVertT<NA> to_camera(const View &vw, const float *__restrict__ p)
{
    const float X = p[0], Y = p[1], Z = p[2];
    CamVertT<NA> c;
    c.x = ((vw.m[0] * X + vw.m[1] * Y) + vw.m[2] * Z) + vw.m[3];
    c.y = ((vw.m[4] * X + vw.m[5] * Y) + vw.m[6] * Z) + vw.m[7];
    c.z = ((vw.m[8] * X + vw.m[9] * Y) + vw.m[10] * Z) + vw.m[11];
    return c;
}

// the point of edge a -> b on z = near, always from the inside vertex a
template <int NA>
RS_FN CamVertT<NA> clip_point(const CamVertT<NA> &a, const CamVertT<NA> &b, float near_)
{
    const float t = RS_DIV(near_ - a.z, b.z - a.z);
    CamVertT<NA> p;
    p.x = a.x + t * (b.x - a.x);
    p.y = a.y + t * (b.y - a.y);
    p.z = a.z + t * (b.z - a.z);
#pragma unroll
    for (int i = 0; i < NA; i++) p.a[i] = a.a[i] + t * (b.a[i] - a.a[i]);
    return p;
}

template <int NA>
struct SnappedT {
    int U, V;
    float iz, a[NA];
    bool ok;
};

template <int NA>
RS_FN SnappedT<NA> project(const View &vw, const CamVertT<NA> &c)
{
    const float u = RS_DIV(vw.fx * c.x, c.z) + vw.cx;
    const float v = RS_DIV(vw.fy * c.y, c.z) + vw.cy;
    const float ru = rintf(u * (float)SUB), rv = rintf(v * (float)SUB);
    SnappedT<NA> s;
    s.ok = fabsf(ru) <= GUARD && fabsf(rv) <= GUARD;       // false for NaN / inf too
    s.U = s.ok ? (int)ru : 0;
    s.V = s.ok ? (int)rv : 0;
    s.iz = RS_DIV(1.0f, c.z);
#pragma unroll
    for (int i = 0; i < NA; i++) s.a[i] = c.a[i];
    return s;
}

RS_FN long long edge_fn(int ax, int ay, int bx, int by, int px, int py)
{
    return (long long)(bx - ax) * (long long)(py - ay) - (long long)(by - ay) * (long long)(px - ax);
}

// one piece from three snapped vertices: false when it is not drawn (guard: counted in *dropped; zero area: not counted)
template <int NA>
RS_FN bool make_piece(const SnappedT<NA> &a, const SnappedT<NA> &b, const SnappedT<NA> &c, PieceT<NA> &out, int *dropped)
{
    if (!(a.ok && b.ok && c.ok)) {
        *dropped += 1;
        return false;
    }
    const long long area = edge_fn(a.U, a.V, b.U, b.V, c.U, c.V);
    if (area == 0) return false;
    const bool flip = area < 0;                            // both windings are drawn: re-wind to positive area
    const SnappedT<NA> &p1 = flip ? c : b, &p2 = flip ? b : c;
    out.U[0] = a.U; out.V[0] = a.V; out.iz[0] = a.iz;
    out.U[1] = p1.U; out.V[1] = p1.V; out.iz[1] = p1.iz;
    out.U[2] = p2.U; out.V[2] = p2.V; out.iz[2] = p2.iz;
#pragma unroll
    for (int i = 0; i < NA; i++) {
        out.a[0][i] = a.a[i];
        out.a[1][i] = p1.a[i];
        out.a[2][i] = p2.a[i];
    }
    return true;
}

// stage (a) for one (view, triangle): number of drawn pieces (0..2) in out[]
template <int NA>
RS_FN int setup_triangle(const View &vw, float near_, const CamVertT<NA> &v0, const CamVertT<NA> &v1, const CamVertT<NA> &v2, PieceT<NA> out[2],
                         int *dropped)
{
    typedef CamVertT<NA> CV;
    const bool i0 = v0.z >= near_, i1 = v1.z >= near_, i2 = v2.z >= near_;
    const int nin = (int)i0 + (int)i1 + (int)i2;
    if (nin == 0) return 0;
    int n = 0;
    if (nin == 3) {
        n += make_piece(project(vw, v0), project(vw, v1), project(vw, v2), out[n], dropped) ? 1 : 0;
    } else if (nin == 1) {
        // a inside, b and c (the next two in cyclic order) outside: (a, ab, ac)
        const CV &a = i0 ? v0 : (i1 ? v1 : v2), &b = i0 ? v1 : (i1 ? v2 : v0), &c = i0 ? v2 : (i1 ? v0 : v1);
        n += make_piece(project(vw, a), project(vw, clip_point(a, b, near_)), project(vw, clip_point(a, c, near_)), out[n], dropped) ? 1 : 0;
    } else {
        // c outside, a and b (the next two in cyclic order) inside: the quad (a, b, bc, ac) as (a, b, bc) and (a, bc, ac)
        const CV &c = !i0 ? v0 : (!i1 ? v1 : v2), &a = !i0 ? v1 : (!i1 ? v2 : v0), &b = !i0 ? v2 : (!i1 ? v0 : v1);
        const SnappedT<NA> sa = project(vw, a), sb = project(vw, b), sbc = project(vw, clip_point(b, c, near_)),
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

// the record of a drawn piece and its packed tile box; NOBOX when no pixel's sample can lie in its box
template <int NA>
RS_FN unsigned piece_record(const PieceT<NA> &pc, int index, int W, int H, PieceRec &r)
{
    int x0, y0, x1, y1;
    if (!pixel_box(pc.U[0], pc.V[0], pc.U[1], pc.V[1], pc.U[2], pc.V[2], W, H, x0, y0, x1, y1)) return NOBOX;
    r.U0 = pc.U[0]; r.V0 = pc.V[0]; r.U1 = pc.U[1]; r.V1 = pc.V[1];
    r.U2 = pc.U[2]; r.V2 = pc.V[2]; r.tri = index; r.pad0 = 0;
    r.iz0 = pc.iz[0]; r.iz1 = pc.iz[1]; r.iz2 = pc.iz[2]; r.pad1 = 0.0f;
    return pack_box(x0 / TILE, y0 / TILE, x1 / TILE, y1 / TILE);
}

// The attributes of pixel (px, py), won at depth bits zbits by the triangle (v0, v1, v2): the triangle set up again (the same statements on
// the same inputs, hence the same pieces) and interpolated on the piece that covers the pixel:
//   num[i] = (l0*(a0[i]*iz0) + l1*(a1[i]*iz1)) + l2*(a2[i]*iz2),  *z = the piece's depth there;  false (num = 0) when no piece matches
template <int NA>
RS_FN bool attributes_at(const View &vw, float near_, const CamVertT<NA> &v0, const CamVertT<NA> &v1, const CamVertT<NA> &v2, int px, int py,
                         unsigned zbits, float num[NA], float *z)
{
    PieceT<NA> pc[2];
    int dropped = 0;
    const int np = setup_triangle(vw, near_, v0, v1, v2, pc, &dropped);
    bool found = false;
#pragma unroll
    for (int i = 0; i < NA; i++) num[i] = 0.0f;
    *z = 0.0f;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        long long e0, e1, e2;
        if (k < np && cover(pc[k].U[0], pc[k].V[0], pc[k].U[1], pc[k].V[1], pc[k].U[2], pc[k].V[2], px, py, e0, e1, e2)) {
            float l0, l1, l2;
            barycentric(e0, e1, e2, l0, l1, l2);
            const float invz = (l0 * pc[k].iz[0] + l1 * pc[k].iz[1]) + l2 * pc[k].iz[2];
            const float zk = RS_DIV(1.0f, invz);
            if (__builtin_bit_cast(unsigned, zk) == zbits) {
                found = true;
                *z = zk;
#pragma unroll
                for (int i = 0; i < NA; i++)
                    num[i] = (l0 * (pc[k].a[0][i] * pc[k].iz[0]) + l1 * (pc[k].a[1][i] * pc[k].iz[1])) + l2 * (pc[k].a[2][i] * pc[k].iz[2]);
            }
        }
    }
    return found;
}

// the z-buffer entry of a key image: nearest depth first, then the lower index
RS_FN unsigned long long key_min(unsigned long long a, unsigned long long b) { return a < b ? a : b; }

// One tile's nearest key per pixel over a bin of piece records (rs_tile_kernel's scheme): the bin is streamed in chunks of WG pieces, one
// record per lane, read once.  A piece whose box covers at most SMALL_BOX pixels of the tile is rasterised by its own lane (LDS atomic
// minimum); the others are put in an LDS list and rasterised by the whole workgroup, one lane per pixel.  Called by all WG lanes of the
// workgroup; returns the key of this lane's pixel (px, py) (~0 when nothing covers it or the pixel lies outside the image).
__device__ __forceinline__ unsigned long long tile_nearest_key(const PieceRec *__restrict__ recs, const int *__restrict__ bin, int n, int W, int H,
                                                               int tpx, int tpy, int px, int py, bool live, unsigned long long *zbuf, PieceRec *big,
                                                               int *nbig)
{
    const int t = threadIdx.x;
    zbuf[t] = ~0ull;
    unsigned long long mine = ~0ull;
    for (int c0 = 0; c0 < n; c0 += WG) {
        if (t == 0) *nbig = 0;
        __syncthreads();
        if (c0 + t < n) {
            const PieceRec r = recs[bin[c0 + t]];
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
                big[atomicAdd(nbig, 1)] = r;
            }
        }
        __syncthreads();
        const int nb = *nbig;
        if (live)
            for (int k = 0; k < nb; k++) {
                unsigned long long key;
                if (pixel_key(big[k], px, py, key)) mine = key_min(key, mine);
            }
        __syncthreads();                                     // big / nbig are rewritten by the next chunk
    }
    __syncthreads();
    return key_min(zbuf[t], mine);
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
}  // namespace
