// Signed distance volume of a triangle mesh for gfx950 (wave64): the {scene}_sdf.npy that the fitting loop and the plausibility table sample,
// computed from the scene mesh instead of downloaded.  The reference has no code for this; the contract is DESIGN.md "Mesh -> SDF volume".
//
// Arithmetic contract (this file is compiled with -ffp-contract=off):
//   node           p[a] = gmin[a] + (float)i_a * ((gmax[a] - gmin[a]) / (float)(D - 1))      (the sampler's align_corners = True positions)
//   closest point  one fp32 routine on the 48-byte record (a, ab = b - a, ac = c - a): seven Voronoi regions in a fixed order of tests,
//                  q = the closest point relative to a, r = (p - a) - q = p - c, d2 = (r.x*r.x + r.y*r.y) + r.z*r.z
//   minimum        key = bits(d2) << 32 | kept-triangle index; a node keeps the smallest key, so the visiting order is free and equal
//                  d2 goes to the lower index
//   value          sqrt(d2) of the winner, negated when (r.x*n.x + r.y*n.y) + r.z*n.z < 0 with n the angle-weighted pseudonormal of the
//                  feature (face, edge or vertex) of the winner that c lies on; a dot product of exactly 0 gives the positive sign
// Welding, the dropping of zero-area triangles and the pseudonormals are computed once, in fp64, on the host (psi_mesh_sdf_create), together
// with the cell grid: the bins depend on the mesh alone, so they are filled there and their order is the same in every run.
//
// One kernel per psi_mesh_sdf_compute call:
//   msdf_brick  one 256-lane workgroup per 8x8x8 brick of nodes, two nodes per lane.  mode 0: the cells of the grid are visited in shells
//               of growing Chebyshev distance from the cells the brick's box lies in; 256 cells at a time, one per lane, a cell is kept when
//               it is not empty and a lower bound of its distance to the brick's box does not exceed the largest current best distance of
//               the brick's nodes (one LDS reduction per 256 cells); the records of the kept cells are staged through LDS 256 at a time and
//               every lane tests every staged record.  The search ends at the first shell whose lower bound exceeds that distance; the
//               shell loop is bounded by the extent of the cell grid.  mode 1: every record is streamed through the same routine.
// No floating-point atomics, no communication between workgroups, no spinning: the volume is bit-identical from run to run, and pruning
// changes no bit (the bounds carry an explicit slack, below).
#include "mesh_sdf_shared.h"
#include "blob.h"
#include <string.h>
#include <algorithm>
#include <vector>

#pragma clang fp contract(off)

#include "closest_point_shared.h"      // MS_DIV, dot3, closest_point: the routine csrc/body_depth.hip shares

namespace {

constexpr int BRICK = 8;             // nodes per brick edge
constexpr int WG = 256;              // lanes per workgroup = records per staged chunk = cells per batch
constexpr int MAX_CELLS_AXIS = 128;  // cells per axis of the grid, at most
constexpr float REL_SLACK = 1e-4f;   // of the largest coordinate magnitude: ~100 x the fp32 error of a distance or of a cell boundary
constexpr float REL_GROW = 1.0001f;  // on the largest best distance, against the rounding of the squares that are compared

struct __attribute__((aligned(16))) TriRec {   // 48 bytes = 3 x 16: what the scan reads
    float a[3], ab[3], ac[3];
    int idx;                                   // the triangle's index among the kept ones (= its own position in the array)
    int pad[2];
};
static_assert(sizeof(TriRec) == 48, "scan records are 16-byte multiples");

struct __attribute__((aligned(16))) NrmRec {   // 96 bytes: only the winner of a node is read
    float n[7][3];                             // 0 face, 1 edge ab, 2 edge bc, 3 edge ca, 4 vertex a, 5 vertex b, 6 vertex c
    float pad[3];
};
static_assert(sizeof(NrmRec) == 96, "normal records are 16-byte multiples");

struct CellGrid {
    float bmin[3], h[3], invh[3];
    int n[3];
};

struct NodeGrid {
    float gmin[3], step[3];
    int D;
    float slack;
};

#ifdef __HIP_DEVICE_COMPILE__
#define MS_SQRT(a) __fsqrt_rn(a)
#else
#define MS_SQRT(a) sqrtf(a)
#endif

MS_FN float node_pos(const NodeGrid &g, int axis, int i) { return psi_mesh_node_pos(g.gmin[axis], g.step[axis], i); }

// the cell of the grid a coordinate lies in (clamped): monotone in x, which is all that binning and search need from it
MS_FN int cell_of(const CellGrid &g, int axis, float x)
{
    float u = (x - g.bmin[axis]) * g.invh[axis];
    u = fminf(fmaxf(u, 0.0f), (float)(g.n[axis] - 1));
    return (int)u;
}

struct Box {
    int x0, y0, z0, nx, ny, nz;
    MS_FN int count() const { return nx * ny * nz; }
};

MS_FN Box make_box(int x0, int x1, int y0, int y1, int z0, int z1, bool present)
{
    Box b;
    b.x0 = x0; b.y0 = y0; b.z0 = z0;
    b.nx = present ? x1 - x0 + 1 : 0;
    b.ny = y1 - y0 + 1;
    b.nz = z1 - z0 + 1;
    return b;
}

// The brick's search state: its box of node positions and the range of cells that box lies in.
struct Brick {
    float lo[3], hi[3];
    int c0[3], c1[3];
};

MS_FN Brick make_brick(const NodeGrid &ng, const CellGrid &cg, int bx, int by, int bz)
{
    const int first[3] = {bx, by, bz};
    Brick br;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const int last = (first[a] + BRICK < ng.D ? first[a] + BRICK : ng.D) - 1;
        br.lo[a] = node_pos(ng, a, first[a]);
        br.hi[a] = node_pos(ng, a, last);
        br.c0[a] = cell_of(cg, a, br.lo[a]);
        br.c1[a] = cell_of(cg, a, br.hi[a]);
    }
    return br;
}

// the last shell that has a cell: the largest index distance from the brick's cells to a border of the grid
MS_FN int last_shell(const CellGrid &cg, const Brick &br)
{
    int s = 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        s = s > br.c0[a] ? s : br.c0[a];
        s = s > cg.n[a] - 1 - br.c1[a] ? s : cg.n[a] - 1 - br.c1[a];
    }
    return s;
}

// Shell s = the cells at Chebyshev index distance s from the brick's cells, as up to six disjoint boxes clipped to the grid: the two x
// slabs over the shell's whole y and z range, the two y slabs over the x range between them, the two z slabs over what is left.  Shell 0
// is the brick's own cells.  Every cell of the grid lies in exactly one box of exactly one shell.  (Six named members, not an array: the
// lane-dependent choice among them must stay a chain of selects on registers.)
struct Shell {
    Box b0, b1, b2, b3, b4, b5;
    MS_FN int count() const { return b0.count() + b1.count() + b2.count() + b3.count() + b4.count() + b5.count(); }
};

MS_FN Shell shell_boxes(const CellGrid &cg, const Brick &br, int s)
{
    Shell sh;
    if (s == 0) {
        sh.b0 = make_box(br.c0[0], br.c1[0], br.c0[1], br.c1[1], br.c0[2], br.c1[2], true);
        sh.b1 = sh.b2 = sh.b3 = sh.b4 = sh.b5 = make_box(0, 0, 0, 0, 0, 0, false);
        return sh;
    }
    const int q = s - 1;
    const int x0 = br.c0[0], x1 = br.c1[0], y0 = br.c0[1], y1 = br.c1[1], z0 = br.c0[2], z1 = br.c1[2];
    const int NX = cg.n[0], NY = cg.n[1], NZ = cg.n[2];
    auto lo = [](int c, int d) { return c - d > 0 ? c - d : 0; };
    auto hi = [](int c, int d, int n) { return c + d < n - 1 ? c + d : n - 1; };
    sh.b0 = make_box(x0 - s, x0 - s, lo(y0, s), hi(y1, s, NY), lo(z0, s), hi(z1, s, NZ), x0 - s >= 0);
    sh.b1 = make_box(x1 + s, x1 + s, lo(y0, s), hi(y1, s, NY), lo(z0, s), hi(z1, s, NZ), x1 + s <= NX - 1);
    sh.b2 = make_box(lo(x0, q), hi(x1, q, NX), y0 - s, y0 - s, lo(z0, s), hi(z1, s, NZ), y0 - s >= 0);
    sh.b3 = make_box(lo(x0, q), hi(x1, q, NX), y1 + s, y1 + s, lo(z0, s), hi(z1, s, NZ), y1 + s <= NY - 1);
    sh.b4 = make_box(lo(x0, q), hi(x1, q, NX), lo(y0, q), hi(y1, q, NY), z0 - s, z0 - s, z0 - s >= 0);
    sh.b5 = make_box(lo(x0, q), hi(x1, q, NX), lo(y0, q), hi(y1, q, NY), z1 + s, z1 + s, z1 + s <= NZ - 1);
    return sh;
}

// cell number i of a shell (i below its count)
MS_FN void shell_cell(const Shell &sh, int i, int &cx, int &cy, int &cz)
{
    int rem = i;
    cx = cy = cz = 0;
#define MS_TRY_BOX(B)                                   \
    {                                                   \
        const int c = (B).count();                      \
        if (rem >= 0 && rem < c) {                      \
            cx = (B).x0 + rem / ((B).ny * (B).nz);      \
            cy = (B).y0 + (rem / (B).nz) % (B).ny;      \
            cz = (B).z0 + rem % (B).nz;                 \
        }                                               \
        rem -= c;                                       \
    }
    MS_TRY_BOX(sh.b0)
    MS_TRY_BOX(sh.b1)
    MS_TRY_BOX(sh.b2)
    MS_TRY_BOX(sh.b3)
    MS_TRY_BOX(sh.b4)
    MS_TRY_BOX(sh.b5)
#undef MS_TRY_BOX
}

// Lower bound of the distance from the brick's box to any cell of shell s >= 1.  Those cells lie outside the index box of the shells before
// them, so the bound is the distance of the brick's box to the nearest face of that index box which has cells beyond it (+inf: none has).
MS_FN float shell_bound(const CellGrid &cg, const Brick &br, int s)
{
    float lb = INFINITY;
    const int q = s - 1;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        if (br.c0[a] - q > 0) lb = fminf(lb, br.lo[a] - (cg.bmin[a] + (float)(br.c0[a] - q) * cg.h[a]));
        if (br.c1[a] + q < cg.n[a] - 1) lb = fminf(lb, (cg.bmin[a] + (float)(br.c1[a] + s) * cg.h[a]) - br.hi[a]);
    }
    return lb;
}

// squared distance between the brick's box and the nominal extent of a cell, [bmin + i h, bmin + (i + 1) h] per axis
MS_FN float cell_gap2(const CellGrid &cg, const Brick &br, int cx, int cy, int cz)
{
    const int c[3] = {cx, cy, cz};
    float g[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float cl = cg.bmin[a] + (float)c[a] * cg.h[a], ch = cg.bmin[a] + (float)(c[a] + 1) * cg.h[a];
        g[a] = fmaxf(fmaxf(cl - br.hi[a], br.lo[a] - ch), 0.0f);
    }
    return dot3(g[0], g[1], g[2], g[0], g[1], g[2]);
}

// Pruning threshold from the largest best d2 of the brick's nodes.  A cell is skipped, and the search ended, when a squared lower bound
// exceeds it.  The slack (REL_SLACK of the largest coordinate magnitude, about a hundred times the fp32 error of a computed distance or of a
// cell boundary) and the growth factor make the test conservative: a skipped triangle's COMPUTED d2 is above every node's best, so pruning
// changes no bit.  +inf and NaN ("nothing found yet") never compare below anything.
MS_FN float prune_threshold2(float best_d2_max, float slack)
{
    const float thr = MS_SQRT(best_d2_max) * REL_GROW + slack;
    return thr * thr;
}

MS_FN bool pruned(float bound2, float thr2) { return bound2 > thr2; }

// the value of a node from its winner: the closest point again (the same statements on the same inputs), its region, the sign from that
// feature's normal
MS_FN float signed_value(const TriRec &r, const NrmRec &nr, unsigned d2_bits, float px, float py, float pz)
{
    float rx, ry, rz;
    const int region = closest_point(r.ab[0], r.ab[1], r.ab[2], r.ac[0], r.ac[1], r.ac[2], px - r.a[0], py - r.a[1], pz - r.a[2], rx, ry, rz);
    const float *n = nr.n[region];
    const float side = dot3(rx, ry, rz, n[0], n[1], n[2]);
    float d2;
    memcpy(&d2, &d2_bits, 4);
    const float d = MS_SQRT(d2);
    return side < 0.0f ? -d : d;
}

MS_FN unsigned long long key_of(float d2, int idx)
{
    unsigned bits;
    memcpy(&bits, &d2, 4);
    return ((unsigned long long)bits << 32) | (unsigned)idx;
}

template <bool COUNT>
__global__ __launch_bounds__(WG) void msdf_brick_kernel(const TriRec *__restrict__ recs, const NrmRec *__restrict__ nrm, int nk, CellGrid cg,
                                                        const int *__restrict__ cell_start, const int *__restrict__ bins, NodeGrid ng, int mode,
                                                        float *__restrict__ out, unsigned long long *__restrict__ pairs)
{
    __shared__ float4 stage[WG * 3];            // 12 KB: one chunk of records
    __shared__ int s_off[WG], s_start[WG];      // the batch's kept cells: first position in the batch's record list, first bin entry
    __shared__ int s_wsum[WG / 64];
    __shared__ unsigned s_red[WG / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int D = ng.D;
    const int bx = blockIdx.z * BRICK, by = blockIdx.y * BRICK, bz = blockIdx.x * BRICK;     // z runs fastest in the volume
    const int ix0 = bx + (t >> 6), ix1 = ix0 + 4, iy = by + ((t >> 3) & 7), iz = bz + (t & 7);
    const bool live0 = ix0 < D && iy < D && iz < D, live1 = ix1 < D && iy < D && iz < D;
    const float py = node_pos(ng, 1, iy), pz = node_pos(ng, 2, iz);
    const float px0 = node_pos(ng, 0, ix0), px1 = node_pos(ng, 0, ix1);
    unsigned long long best0 = ~0ull, best1 = ~0ull;
    unsigned long long npairs = 0;
    const int nlive = min(BRICK, D - bx) * min(BRICK, D - by) * min(BRICK, D - bz);

    // every lane against the nst records in the stage
    auto test_staged = [&](int nst) {
        for (int k = 0; k < nst; k++) {
            const float4 r0 = stage[3 * k], r1 = stage[3 * k + 1], r2 = stage[3 * k + 2];
            const int idx = __float_as_int(r2.y);
            const float apy = py - r0.y, apz = pz - r0.z;
            float rx, ry, rz;
            closest_point(r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, px0 - r0.x, apy, apz, rx, ry, rz);
            const unsigned long long k0 = key_of(dot3(rx, ry, rz, rx, ry, rz), idx);
            best0 = k0 < best0 ? k0 : best0;
            closest_point(r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, px1 - r0.x, apy, apz, rx, ry, rz);
            const unsigned long long k1 = key_of(dot3(rx, ry, rz, rx, ry, rz), idx);
            best1 = k1 < best1 ? k1 : best1;
        }
        if (COUNT) npairs += (unsigned long long)nst * nlive;
    };
    auto stage_record = [&](int tri) {
        const float4 *src = reinterpret_cast<const float4 *>(recs + tri);
        stage[3 * t] = src[0];
        stage[3 * t + 1] = src[1];
        stage[3 * t + 2] = src[2];
    };

    if (mode == 1) {
        for (int c0 = 0; c0 < nk; c0 += WG) {
            if (c0 + t < nk) stage_record(c0 + t);
            __syncthreads();
            test_staged(min(WG, nk - c0));
            __syncthreads();
        }
    } else {
        const Brick br = make_brick(ng, cg, bx, by, bz);
        const int smax = last_shell(cg, br);
        float thr2 = INFINITY;
        for (int s = 0; s <= smax; s++) {
            if (s > 0) {
                const float lb = shell_bound(cg, br, s);
                if (lb > 0.0f && pruned(lb * lb, thr2)) break;
            }
            const Shell sh = shell_boxes(cg, br, s);
            const int ncell = sh.count();
            for (int base = 0; base < ncell; base += WG) {
                int cnt = 0, start = 0;
                if (base + t < ncell) {
                    int cx, cy, cz;
                    shell_cell(sh, base + t, cx, cy, cz);
                    const int cell = (cx * cg.n[1] + cy) * cg.n[2] + cz;
                    const int st = cell_start[cell], c = cell_start[cell + 1] - st;
                    if (c > 0 && !pruned(cell_gap2(cg, br, cx, cy, cz), thr2)) {
                        cnt = c;
                        start = st;
                    }
                }
                // exclusive scan of the 256 counts: the batch's records as one list
                int incl = cnt;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int up = __shfl_up(incl, o, 64);
                    if (lane >= o) incl += up;
                }
                if (lane == 63) s_wsum[wave] = incl;
                __syncthreads();
                int woff = 0, total = 0;
#pragma unroll
                for (int w = 0; w < WG / 64; w++) {
                    const int v = s_wsum[w];
                    woff += w < wave ? v : 0;
                    total += v;
                }
                s_off[t] = woff + incl - cnt;
                s_start[t] = start;
                __syncthreads();
                for (int c0 = 0; c0 < total; c0 += WG) {
                    const int pos = c0 + t;
                    if (pos < total) {
                        int j = 0;                       // the last cell whose first position is <= pos: it has a record there
#pragma unroll
                        for (int st = WG / 2; st > 0; st >>= 1)
                            if (s_off[j + st] <= pos) j += st;
                        stage_record(bins[s_start[j] + (pos - s_off[j])]);
                    }
                    __syncthreads();
                    test_staged(min(WG, total - c0));
                    __syncthreads();
                }
                if (total > 0) {
                    // the largest best d2 among the brick's nodes: non-negative floats order like their bits
                    unsigned m = max(live0 ? (unsigned)(best0 >> 32) : 0u, live1 ? (unsigned)(best1 >> 32) : 0u);
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
                    if (lane == 0) s_red[wave] = m;
                    __syncthreads();
                    m = max(max(s_red[0], s_red[1]), max(s_red[2], s_red[3]));
                    thr2 = prune_threshold2(__uint_as_float(m), ng.slack);
                }
            }
        }
    }
    if (COUNT && t == 0) atomicAdd(pairs, npairs);
    if (!out) return;                                       // the counting call may ask for the count alone

#pragma unroll
    for (int k = 0; k < 2; k++) {
        const bool live = k ? live1 : live0;
        if (!live) continue;
        const unsigned long long key = k ? best1 : best0;
        const int ix = k ? ix1 : ix0;
        const float px = k ? px1 : px0;
        const int tri = (int)(unsigned)(key & 0xffffffffu);
        if (tri < 0 || tri >= nk) {                         // no record was tested: cannot happen with nk >= 1, and must not index the records
            out[((size_t)ix * D + iy) * D + iz] = INFINITY;
            continue;
        }
        out[((size_t)ix * D + iy) * D + iz] = signed_value(recs[tri], nrm[tri], (unsigned)(key >> 32), px, py, pz);
    }
}

// ---- host side of psi_mesh_sdf_create: welding, degenerate triangles, pseudonormals (fp64), the cell grid and its bins ----

struct V3 {
    double x, y, z;
};
inline V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline double dotd(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline double norm(V3 a) { return sqrt(dotd(a, a)); }
inline void add_scaled(V3 &acc, V3 n, double s) { acc.x += s * n.x; acc.y += s * n.y; acc.z += s * n.z; }
inline void store_unit(float *dst, V3 n)
{
    const double l = norm(n);
    dst[0] = l > 0 ? (float)(n.x / l) : 0.0f;
    dst[1] = l > 0 ? (float)(n.y / l) : 0.0f;
    dst[2] = l > 0 ? (float)(n.z / l) : 0.0f;
}

struct PosKey {
    uint32_t b[3];
    int v;
    bool operator<(const PosKey &o) const
    {
        if (b[0] != o.b[0]) return b[0] < o.b[0];
        if (b[1] != o.b[1]) return b[1] < o.b[1];
        if (b[2] != o.b[2]) return b[2] < o.b[2];
        return v < o.v;
    }
    bool same(const PosKey &o) const { return b[0] == o.b[0] && b[1] == o.b[1] && b[2] == o.b[2]; }
};

struct EdgeUse {
    uint64_t key;      // the welded ids of the edge, low id first
    int tri, slot;     // kept triangle and which of its edges (0 ab, 1 bc, 2 ca)
    bool operator<(const EdgeUse &o) const { return key != o.key ? key < o.key : (tri != o.tri ? tri < o.tri : slot < o.slot); }
};

// everything psi_mesh_sdf_create uploads, built on the host from the vertex and face arrays
struct HostMesh {
    std::vector<TriRec> recs;
    std::vector<NrmRec> nrm;
    std::vector<int> cell_start, bins;
    std::vector<float> kept;   // [nk][3][3]: the vertices A, B, C of the kept triangles (what the winding number is summed over)
    CellGrid cg;
    int32_t info[4];
    float scale;       // the largest coordinate magnitude of the kept triangles
};

int build_host_mesh(const std::vector<float> &hv, const std::vector<int32_t> &hf, int nv, int nf, HostMesh &hm)
{
    for (size_t i = 0; i < hv.size(); i++) PSI_REQUIRE(std::isfinite(hv[i]), "a vertex coordinate is not finite");
    for (size_t i = 0; i < hf.size(); i++) PSI_REQUIRE(hf[i] >= 0 && hf[i] < nv, "a face index lies outside [0, nv)");

    // weld: vertices with bit-identical positions (-0.0 counted as +0.0) get the id of the first of them
    std::vector<PosKey> keys((size_t)nv);
    for (int v = 0; v < nv; v++) {
        for (int a = 0; a < 3; a++) {
            const float x = hv[(size_t)v * 3 + a] == 0.0f ? 0.0f : hv[(size_t)v * 3 + a];
            memcpy(&keys[v].b[a], &x, 4);
        }
        keys[v].v = v;
    }
    std::sort(keys.begin(), keys.end());
    std::vector<int> wid((size_t)nv);
    int n_welded = 0;
    for (size_t i = 0; i < keys.size(); i++) {
        const bool first = i == 0 || !keys[i].same(keys[i - 1]);
        n_welded += first ? 1 : 0;
        wid[keys[i].v] = first ? keys[i].v : wid[keys[i - 1].v];
    }
    auto P = [&](int v) { return V3{(double)hv[(size_t)v * 3], (double)hv[(size_t)v * 3 + 1], (double)hv[(size_t)v * 3 + 2]}; };

    // kept triangles, their unit normals and corner angles
    std::vector<int> kv;              // [nk][3] welded ids
    std::vector<V3> fn;               // unit face normals
    std::vector<V3> vacc((size_t)nv, V3{0, 0, 0});
    int dropped = 0;
    for (int f = 0; f < nf; f++) {
        const int a = wid[hf[(size_t)f * 3]], b = wid[hf[(size_t)f * 3 + 1]], c = wid[hf[(size_t)f * 3 + 2]];
        const V3 pa = P(a), pb = P(b), pc = P(c);
        const V3 N = cross(sub(pb, pa), sub(pc, pa));
        if (a == b || b == c || c == a || (N.x == 0 && N.y == 0 && N.z == 0)) {
            dropped++;
            continue;
        }
        const double l = norm(N);
        const V3 n{N.x / l, N.y / l, N.z / l};
        const int ids[3] = {a, b, c};
        const V3 pts[3] = {pa, pb, pc};
        for (int k = 0; k < 3; k++) {
            const V3 u = sub(pts[(k + 1) % 3], pts[k]), w = sub(pts[(k + 2) % 3], pts[k]);
            add_scaled(vacc[ids[k]], n, atan2(norm(cross(u, w)), dotd(u, w)));
        }
        kv.push_back(a); kv.push_back(b); kv.push_back(c);
        fn.push_back(n);
    }
    const int nk = (int)fn.size();
    PSI_REQUIRE(nk >= 1, "no triangle of non-zero area is left");

    // edges: the normals of all triangles that share the welded pair, summed in triangle order
    std::vector<EdgeUse> eu((size_t)nk * 3);
    for (int t = 0; t < nk; t++)
        for (int k = 0; k < 3; k++) {
            const uint32_t u = (uint32_t)kv[(size_t)t * 3 + k], w = (uint32_t)kv[(size_t)t * 3 + (k + 1) % 3];
            eu[(size_t)t * 3 + k] = EdgeUse{((uint64_t)std::min(u, w) << 32) | std::max(u, w), t, k};
        }
    std::sort(eu.begin(), eu.end());
    std::vector<NrmRec> hn((size_t)nk);
    int open_edges = 0;
    for (size_t i = 0; i < eu.size();) {
        size_t j = i;
        V3 acc{0, 0, 0};
        while (j < eu.size() && eu[j].key == eu[i].key) {
            add_scaled(acc, fn[eu[j].tri], 1.0);
            j++;
        }
        open_edges += (j - i) != 2 ? 1 : 0;
        for (size_t k = i; k < j; k++) store_unit(hn[eu[k].tri].n[1 + eu[k].slot], acc);
        i = j;
    }
    std::vector<TriRec> hr((size_t)nk);
    hm.kept.resize((size_t)nk * 9);
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int t = 0; t < nk; t++) {
        TriRec &r = hr[t];
        const int a = kv[(size_t)t * 3], b = kv[(size_t)t * 3 + 1], c = kv[(size_t)t * 3 + 2];
        for (int k = 0; k < 3; k++) {
            r.a[k] = hv[(size_t)a * 3 + k];
            r.ab[k] = hv[(size_t)b * 3 + k] - r.a[k];          // fp32, rounded once: the statement the contract names
            r.ac[k] = hv[(size_t)c * 3 + k] - r.a[k];
            hm.kept[(size_t)t * 9 + k] = hv[(size_t)a * 3 + k];
            hm.kept[(size_t)t * 9 + 3 + k] = hv[(size_t)b * 3 + k];
            hm.kept[(size_t)t * 9 + 6 + k] = hv[(size_t)c * 3 + k];
            lo[k] = fminf(lo[k], fminf(r.a[k], fminf(hv[(size_t)b * 3 + k], hv[(size_t)c * 3 + k])));
            hi[k] = fmaxf(hi[k], fmaxf(r.a[k], fmaxf(hv[(size_t)b * 3 + k], hv[(size_t)c * 3 + k])));
        }
        r.idx = t;
        r.pad[0] = r.pad[1] = 0;
        store_unit(hn[t].n[0], fn[t]);
        store_unit(hn[t].n[4], vacc[a]);
        store_unit(hn[t].n[5], vacc[b]);
        store_unit(hn[t].n[6], vacc[c]);
        hn[t].pad[0] = hn[t].pad[1] = hn[t].pad[2] = 0.0f;
    }

    // the cell grid over the box of the kept triangles: cubic cells, nk / 8 of them in the cube of the longest extent.  For a surface of
    // evenly sized triangles in a room-shaped box that makes a cell edge of two to three triangle edges: the mean occupied cell holds on
    // the order of ten triangles, and a triangle lies in about two cells (every copy is tested again, so smaller cells cost tests)
    hm.info[0] = nk; hm.info[1] = dropped; hm.info[2] = n_welded; hm.info[3] = open_edges;
    float ext_max = 0.0f, scale = 0.0f;
    for (int k = 0; k < 3; k++) {
        ext_max = fmaxf(ext_max, hi[k] - lo[k]);
        scale = fmaxf(scale, fmaxf(fabsf(lo[k]), fabsf(hi[k])));
    }
    hm.scale = scale;
    const double target = std::min(std::max(nk / 8.0, 1.0), 2097152.0);
    const float edge = ext_max / (float)cbrt(target);
    for (int k = 0; k < 3; k++) {
        const float ext = hi[k] - lo[k];
        int n = edge > 0.0f ? (int)ceilf(ext / edge) : 1;
        n = std::min(std::max(n, 1), MAX_CELLS_AXIS);
        hm.cg.bmin[k] = lo[k];
        hm.cg.n[k] = n;
        hm.cg.h[k] = ext / (float)n;
        hm.cg.invh[k] = ext > 0.0f ? (float)n / ext : 0.0f;
    }
    const CellGrid &cg = hm.cg;
    const size_t ncell = (size_t)cg.n[0] * cg.n[1] * cg.n[2];
    std::vector<int> &start = hm.cell_start;
    start.assign(ncell + 1, 0);
    std::vector<int> range((size_t)nk * 6);
    size_t entries = 0;
    for (int t = 0; t < nk; t++) {
        const int ids[3] = {kv[(size_t)t * 3], kv[(size_t)t * 3 + 1], kv[(size_t)t * 3 + 2]};
        for (int k = 0; k < 3; k++) {
            const float x0 = hv[(size_t)ids[0] * 3 + k], x1 = hv[(size_t)ids[1] * 3 + k], x2 = hv[(size_t)ids[2] * 3 + k];
            range[(size_t)t * 6 + k] = cell_of(cg, k, fminf(x0, fminf(x1, x2)));
            range[(size_t)t * 6 + 3 + k] = cell_of(cg, k, fmaxf(x0, fmaxf(x1, x2)));
        }
        const int *r = &range[(size_t)t * 6];
        entries += (size_t)(r[3] - r[0] + 1) * (r[4] - r[1] + 1) * (r[5] - r[2] + 1);
        for (int x = r[0]; x <= r[3]; x++)
            for (int y = r[1]; y <= r[4]; y++)
                for (int z = r[2]; z <= r[5]; z++) start[((size_t)x * cg.n[1] + y) * cg.n[2] + z + 1]++;
    }
    if (entries >= (size_t)1 << 30) {
        psi_set_error("psi_mesh_sdf_create: %zu (cell, triangle) pairs exceed 2^30", entries);
        return PSI_EINVAL;
    }
    for (size_t c = 0; c < ncell; c++) start[c + 1] += start[c];
    std::vector<int> &hb = hm.bins;
    hb.assign(std::max(entries, (size_t)1), 0);
    std::vector<int> cursor(start.begin(), start.end() - 1);
    for (int t = 0; t < nk; t++) {
        const int *r = &range[(size_t)t * 6];
        for (int x = r[0]; x <= r[3]; x++)
            for (int y = r[1]; y <= r[4]; y++)
                for (int z = r[2]; z <= r[5]; z++) hb[cursor[((size_t)x * cg.n[1] + y) * cg.n[2] + z]++] = t;
    }

    hm.recs.swap(hr);
    hm.nrm.swap(hn);
    return 0;
}

}  // namespace

struct psi_mesh_sdf {
    char *blob;        // records | normals | cell starts | bins
    TriRec *recs;
    NrmRec *nrm;
    int *cell_start, *bins;
    int nk;
    int32_t info[4];
    CellGrid cg;
    float scale;
    std::vector<float> kept;   // host copy of the kept triangles, for csrc/mesh_winding.hip
    psi_mesh_aux aux;          // what it builds from them at first use
};

const float *psi_mesh_sdf_kept_tris(const psi_mesh_sdf *m, int *nk)
{
    *nk = m->nk;
    return m->kept.data();
}

psi_mesh_aux *psi_mesh_sdf_aux(psi_mesh_sdf *m) { return &m->aux; }

extern "C" int psi_mesh_sdf_create(psi_mesh_sdf **out, const float *d_verts, const int32_t *d_faces, int nv, int nf)
{
    PSI_REQUIRE(out && d_verts && d_faces, "null pointer");
    PSI_REQUIRE(nv >= 1 && nf >= 1 && nf < (1 << 28), "nv >= 1, 1 <= nf < 2^28");
    std::vector<float> hv((size_t)nv * 3);
    std::vector<int32_t> hf((size_t)nf * 3);
    // a one-off between two device synchronisations: the inputs may have been produced on any stream
    PSI_CHECK_HIP(hipDeviceSynchronize());
    PSI_CHECK_HIP(hipMemcpy(hv.data(), d_verts, hv.size() * 4, hipMemcpyDeviceToHost));
    PSI_CHECK_HIP(hipMemcpy(hf.data(), d_faces, hf.size() * 4, hipMemcpyDeviceToHost));
    HostMesh hm;
    const int rc = build_host_mesh(hv, hf, nv, nf, hm);
    if (rc != 0) return rc;
    const std::vector<TriRec> &hr = hm.recs;
    const std::vector<NrmRec> &hn = hm.nrm;
    const std::vector<int> &start = hm.cell_start, &hb = hm.bins;
    const int nk = (int)hr.size();
    const size_t ncell = start.size() - 1;
    psi_mesh_sdf *m = new psi_mesh_sdf();
    m->nk = nk;
    m->cg = hm.cg;
    m->scale = hm.scale;
    m->kept.swap(hm.kept);
    m->aux = psi_mesh_aux{nullptr, nullptr};
    for (int k = 0; k < 4; k++) m->info[k] = hm.info[k];
    PsiBlob T;
    T.upload(m->recs, hr.data(), (size_t)nk * sizeof(TriRec));
    T.upload(m->nrm, hn.data(), (size_t)nk * sizeof(NrmRec));
    T.upload(m->cell_start, start.data(), (ncell + 1) * 4);
    T.upload(m->bins, hb.data(), hb.size() * 4);
    if (int rc = psi_blob_realise(T, &m->blob, "psi_mesh_sdf_create")) {
        delete m;
        return rc == (int)hipErrorOutOfMemory ? PSI_ENOMEM : rc;
    }
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        psi_set_error("psi_mesh_sdf_create failed: %s", hipGetErrorString(e));
        psi_mesh_sdf_destroy(m);
        return (int)e;
    }
    *out = m;
    return 0;
}

extern "C" void psi_mesh_sdf_destroy(psi_mesh_sdf *m)
{
    if (!m) return;
    if (m->aux.p && m->aux.destroy) m->aux.destroy(m->aux.p);
    (void)hipFree(m->blob);
    delete m;
}

extern "C" int psi_mesh_sdf_info(const psi_mesh_sdf *m, int32_t info[4])
{
    PSI_REQUIRE(m && info, "null pointer");
    for (int k = 0; k < 4; k++) info[k] = m->info[k];
    return 0;
}

static int mesh_sdf_launch(psi_mesh_sdf *m, const float gmin[3], const float gmax[3], int D, int mode, float *d_out, unsigned long long *d_pairs,
                           void *stream)
{
    PSI_REQUIRE(m && gmin && gmax && (d_out || d_pairs), "null pointer");
    PSI_REQUIRE(mode == 0 || mode == 1, "mode is 0 (pruned search) or 1 (every node against every triangle)");
    NodeGrid ng;
    const int rc = psi_mesh_node_steps(gmin, gmax, D, ng.step);
    if (rc != 0) return rc;
    float scale = m->scale;
    for (int k = 0; k < 3; k++) {
        ng.gmin[k] = gmin[k];
        scale = fmaxf(scale, fmaxf(fabsf(gmin[k]), fabsf(gmax[k])));
    }
    ng.D = D;
    ng.slack = REL_SLACK * scale;
    const int nb = psi_cdiv(D, BRICK);
    hipStream_t st = (hipStream_t)stream;
    if (d_pairs) {
        PSI_CHECK_HIP(hipMemsetAsync(d_pairs, 0, 8, st));
        hipLaunchKernelGGL(msdf_brick_kernel<true>, dim3(nb, nb, nb), dim3(WG), 0, st, m->recs, m->nrm, m->nk, m->cg, m->cell_start, m->bins, ng, mode,
                           d_out, d_pairs);
    } else {
        hipLaunchKernelGGL(msdf_brick_kernel<false>, dim3(nb, nb, nb), dim3(WG), 0, st, m->recs, m->nrm, m->nk, m->cg, m->cell_start, m->bins, ng, mode,
                           d_out, (unsigned long long *)nullptr);
    }
    PSI_CHECK_LAUNCH("msdf_brick_kernel");
    return 0;
}

extern "C" int psi_mesh_sdf_compute(psi_mesh_sdf *m, const float gmin[3], const float gmax[3], int D, int mode, float *d_out, void *stream)
{
    PSI_REQUIRE(d_out, "null pointer");
    return mesh_sdf_launch(m, gmin, gmax, D, mode, d_out, nullptr, stream);
}

extern "C" int psi_mesh_sdf_count_pairs(psi_mesh_sdf *m, const float gmin[3], const float gmax[3], int D, int mode, unsigned long long *d_pairs,
                                        void *stream)
{
    PSI_REQUIRE(d_pairs, "null pointer");
    return mesh_sdf_launch(m, gmin, gmax, D, mode, nullptr, d_pairs, stream);
}
