// Generalised winding number of a triangle mesh on the nodes of a volume, for gfx950 (wave64): the robust sign of the mesh -> SDF volume
// for open, touching and interpenetrating scene meshes (Jacobson et al. 2013).  The contract is DESIGN.md "Winding-number sign".
//
//   node      the positions of csrc/mesh_sdf.hip (psi_mesh_node_pos: the same bits)
//   pair      with a = A - p, b = B - p, c = C - p and n = (B - A) x (C - A) (fp64 on the host, stored as fp32; a . n = a . (b x c)):
//             w = atan2(a . n, |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|) = half the solid angle; atan2(0, 0) counts as 0
//             (geom_half_omega in csrc/geom_shared.h)
//   dipole    a far cluster (area-vector sum N, area-weighted centroid c) adds N . (c - p) / (2 |c - p|^3) in the same unit
//   f         -(1 / 2 pi) * the sum: 1 in the free space of a closed room whose triangles face free space, 0 in furniture and outside
//   sum       fp32 within a staged chunk of 256 records, the chunk sums added in fp64, in a fixed order: kept order in the exact arm
//             (beta = 0); cluster order, then the order within the cluster, in the pruned arm.  No floating-point atomics.
//   far       per 8 x 8 x 8 brick: the distance from c to the brick's box of nodes exceeds beta * r (mwind_far, not contracted, so that the
//             host runs of the same statement decide alike)
//
// One kernel per call: one 256-lane workgroup per brick, two nodes per lane.  The clusters are visited 256 at a time, one per lane; a scan
// of their record counts (1 for a far cluster, its triangles for a near one) makes the batch one list of records, staged through LDS 256 at
// a time; every lane reads every staged record (identical addresses broadcast).  Every loop is bounded by the cluster or triangle count.
#include "geom_shared.h"
#include "mesh_sdf_shared.h"
#include <string.h>
#include <algorithm>
#include <map>
#include <vector>

namespace psi_mwind {

constexpr int BRICK = 8;        // nodes per brick edge
constexpr int WG = 256;         // lanes per workgroup = records per staged chunk = clusters per batch
constexpr int MIN_CLUSTER = 8, MAX_CLUSTER = 256;

struct __attribute__((aligned(16))) WRec {     // 48 bytes: a triangle (A, B, C, n) or, staged only, a dipole (c, N, zeros)
    float a[3], b[3], c[3], n[3];
};
static_assert(sizeof(WRec) == 48, "records are 16-byte multiples");

struct __attribute__((aligned(16))) CRec {     // 32 bytes per cluster
    float c[3], r;                             // area-weighted centroid, largest vertex distance from it
    float n[3];                                // sum of the area vectors (B - A) x (C - A) / 2
    int pad;
};
static_assert(sizeof(CRec) == 32, "cluster records are 16-byte multiples");

struct Nodes {
    float gmin[3], step[3];
    int D;
};

// the dipole of a far cluster in the same unit: N . d / (2 |d|^3), d = c - p (never 0: the cluster is farther than beta * r > 0)
MS_FN float half_dipole(float cx, float cy, float cz, float Nx, float Ny, float Nz, float px, float py, float pz)
{
    const float dx = cx - px, dy = cy - py, dz = cz - pz;
    const float d2 = geom_dot3(dx, dy, dz, dx, dy, dz);
    return 0.5f * geom_dot3(Nx, Ny, Nz, dx, dy, dz) / (d2 * sqrtf(d2));
}

// Is the cluster far for the brick whose nodes span [lo, hi]?  Squares are compared; every operation is rounded on its own.
MS_FN bool mwind_far(const float c[3], float r, const float lo[3], const float hi[3], float beta)
{
#pragma clang fp contract(off)
    const float gx = fmaxf(fmaxf(lo[0] - c[0], c[0] - hi[0]), 0.0f);
    const float gy = fmaxf(fmaxf(lo[1] - c[1], c[1] - hi[1]), 0.0f);
    const float gz = fmaxf(fmaxf(lo[2] - c[2], c[2] - hi[2]), 0.0f);
    const float d2 = (gx * gx + gy * gy) + gz * gz;
    const float t = beta * r;
    return d2 > t * t;
}

// the brick's box of node positions
MS_FN void brick_box(const Nodes &ng, int bx, int by, int bz, float lo[3], float hi[3])
{
    const int first[3] = {bx, by, bz};
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const int last = (first[a] + BRICK < ng.D ? first[a] + BRICK : ng.D) - 1;
        lo[a] = psi_mesh_node_pos(ng.gmin[a], ng.step[a], first[a]);
        hi[a] = psi_mesh_node_pos(ng.gmin[a], ng.step[a], last);
    }
}

MS_FN float f_of_sum(double s) { return (float)(-s / 6.283185307179586476925286766559); }

// recs: the triangles in kept order (beta == 0) or in cluster order (beta > 0: cluster j holds recs[j * cluster ...], the last may be
// partial).  counts (COUNT): [0] += (node, triangle) tests, [1] += (node, dipole) tests, live nodes only.
template <bool COUNT>
__global__ __launch_bounds__(WG) void mwind_brick_kernel(const WRec *__restrict__ recs, int nk, const CRec *__restrict__ clus, int nc, int cluster,
                                                         float beta, Nodes ng, float *__restrict__ out, unsigned long long *__restrict__ counts)
{
    __shared__ float4 stage[WG * 3];           // 12 KB: one chunk of records
    __shared__ int s_kind[WG];                 // 1 = the staged record is a dipole
    __shared__ int s_off[WG], s_src[WG];       // the batch's clusters: first position in the batch's record list; first triangle, or ~cluster
    __shared__ int s_wsum[WG / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int D = ng.D;
    const int bx = blockIdx.z * BRICK, by = blockIdx.y * BRICK, bz = blockIdx.x * BRICK;     // z runs fastest in the volume
    const int ix0 = bx + (t >> 6), ix1 = ix0 + 4, iy = by + ((t >> 3) & 7), iz = bz + (t & 7);
    const bool live0 = ix0 < D && iy < D && iz < D, live1 = ix1 < D && iy < D && iz < D;
    const float py = psi_mesh_node_pos(ng.gmin[1], ng.step[1], iy), pz = psi_mesh_node_pos(ng.gmin[2], ng.step[2], iz);
    const float px0 = psi_mesh_node_pos(ng.gmin[0], ng.step[0], ix0), px1 = psi_mesh_node_pos(ng.gmin[0], ng.step[0], ix1);
    const unsigned long long nlive = (unsigned long long)(min(BRICK, D - bx) * min(BRICK, D - by) * min(BRICK, D - bz));
    double acc0 = 0.0, acc1 = 0.0;
    unsigned long long n_tri = 0, n_dip = 0;   // this lane's share of the brick's records

    // every lane against the nst records in the stage: fp32 within the chunk, fp64 across chunks
    auto test_staged = [&](int nst) {
        float s0 = 0.0f, s1 = 0.0f;
        for (int k = 0; k < nst; k++) {
            const float4 r0 = stage[3 * k], r1 = stage[3 * k + 1], r2 = stage[3 * k + 2];
            if (__builtin_amdgcn_readfirstlane(s_kind[k])) {
                s0 += half_dipole(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, px0, py, pz);
                s1 += half_dipole(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, px1, py, pz);
            } else {
                s0 += geom_half_omega(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, px0, py, pz);
                s1 += geom_half_omega(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, px1, py, pz);
            }
        }
        acc0 += (double)s0;
        acc1 += (double)s1;
    };
    auto stage_triangle = [&](int tri) {
        const float4 *src = reinterpret_cast<const float4 *>(recs + tri);
        stage[3 * t] = src[0];
        stage[3 * t + 1] = src[1];
        stage[3 * t + 2] = src[2];
        s_kind[t] = 0;
    };

    if (beta == 0.0f) {
        for (int c0 = 0; c0 < nk; c0 += WG) {
            if (c0 + t < nk) stage_triangle(c0 + t);
            __syncthreads();
            test_staged(min(WG, nk - c0));
            __syncthreads();
        }
        if (COUNT && t == 0) n_tri = (unsigned long long)nk;
    } else {
        float lo[3], hi[3];
        brick_box(ng, bx, by, bz, lo, hi);
        for (int base = 0; base < nc; base += WG) {
            int cnt = 0, src = 0;
            if (base + t < nc) {
                const int j = base + t;
                const float4 q = reinterpret_cast<const float4 *>(clus + j)[0];
                const float c[3] = {q.x, q.y, q.z};
                const bool far = mwind_far(c, q.w, lo, hi, beta);
                cnt = far ? 1 : min(cluster, nk - j * cluster);
                src = far ? ~j : j * cluster;
                if (COUNT) {
                    n_dip += far ? 1 : 0;
                    n_tri += far ? 0 : cnt;
                }
            }
            // exclusive scan of the 256 counts: the batch's records as one list, in cluster order
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
            // lanes past the last cluster get the list's end: their (empty) range is never chosen below
            s_off[t] = woff + incl - cnt;
            s_src[t] = src;
            __syncthreads();
            for (int c0 = 0; c0 < total; c0 += WG) {
                const int pos = c0 + t;
                if (pos < total) {
                    int j = 0;                           // the last cluster whose first position is <= pos: it has a record there
#pragma unroll
                    for (int st = WG / 2; st > 0; st >>= 1)
                        if (s_off[j + st] <= pos) j += st;
                    const int s = s_src[j];
                    if (s < 0) {
                        const float4 *cr = reinterpret_cast<const float4 *>(clus + ~s);
                        const float4 q0 = cr[0], q1 = cr[1];
                        stage[3 * t] = make_float4(q0.x, q0.y, q0.z, q1.x);
                        stage[3 * t + 1] = make_float4(q1.y, q1.z, 0.0f, 0.0f);
                        stage[3 * t + 2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                        s_kind[t] = 1;
                    } else {
                        stage_triangle(s + (pos - s_off[j]));
                    }
                }
                __syncthreads();
                test_staged(min(WG, total - c0));
                __syncthreads();
            }
        }
    }
    if (COUNT) {
        if (n_tri) atomicAdd(counts, n_tri * nlive);
        if (n_dip) atomicAdd(counts + 1, n_dip * nlive);
    }
    if (!out) return;                                    // the counting call may ask for the counts alone
    if (live0) out[((size_t)ix0 * D + iy) * D + iz] = f_of_sum(acc0);
    if (live1) out[((size_t)ix1 * D + iy) * D + iz] = f_of_sum(acc1);
}

__global__ __launch_bounds__(WG) void mwind_apply_sign_kernel(const float *__restrict__ f, float level, float *__restrict__ vol, long long n)
{
    const long long i = (long long)blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const float d = fabsf(vol[i]);
    vol[i] = f[i] < level ? -d : d;
}

// ---- host side: the records in kept order, and the clusters of one `cluster` value (fp64, stored as fp32) ----

inline void fill_record(const float *tri, WRec &r)
{
    double e1[3], e2[3];
    for (int k = 0; k < 3; k++) {
        r.a[k] = tri[k];
        r.b[k] = tri[3 + k];
        r.c[k] = tri[6 + k];
        e1[k] = (double)tri[3 + k] - (double)tri[k];
        e2[k] = (double)tri[6 + k] - (double)tri[k];
    }
    r.n[0] = (float)(e1[1] * e2[2] - e1[2] * e2[1]);
    r.n[1] = (float)(e1[2] * e2[0] - e1[0] * e2[2]);
    r.n[2] = (float)(e1[0] * e2[1] - e1[1] * e2[0]);
}

inline void kept_records(const float *kept, int nk, std::vector<WRec> &recs)
{
    recs.resize((size_t)nk);
    for (int t = 0; t < nk; t++) fill_record(kept + (size_t)t * 9, recs[t]);
}

// Morton code of a centroid: 10 bits per axis over the box of all centroids, x above y above z in every triple of bits
inline uint32_t morton_code(const double cen[3], const double lo[3], const double ext[3])
{
    uint32_t code = 0;
    for (int a = 0; a < 3; a++) {
        int q = 0;
        if (ext[a] > 0.0) {
            q = (int)floor((cen[a] - lo[a]) / ext[a] * 1024.0);
            q = q > 1023 ? 1023 : q;
        }
        for (int i = 0; i < 10; i++) code |= (uint32_t)((q >> i) & 1) << (3 * i + 2 - a);
    }
    return code;
}

// The kept triangles sorted by the Morton code of their centroids ((A + B) + C) / 3 (equal codes in kept order), cut into consecutive
// clusters of `cluster`; per cluster N = the sum of the area vectors, c = the area-weighted mean of the centroids, r = the largest vertex
// distance from c, each summed in the cluster's order.
inline void build_clusters(const float *kept, int nk, int cluster, std::vector<WRec> &recs, std::vector<CRec> &clus)
{
    std::vector<double> cen((size_t)nk * 3);
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, ext[3];
    for (int t = 0; t < nk; t++)
        for (int k = 0; k < 3; k++) {
            const float *v = kept + (size_t)t * 9;
            const double x = (((double)v[k] + (double)v[3 + k]) + (double)v[6 + k]) / 3.0;
            cen[(size_t)t * 3 + k] = x;
            lo[k] = std::min(lo[k], x);
            hi[k] = std::max(hi[k], x);
        }
    for (int k = 0; k < 3; k++) ext[k] = hi[k] - lo[k];
    std::vector<std::pair<uint32_t, int>> order((size_t)nk);
    for (int t = 0; t < nk; t++) order[t] = {morton_code(&cen[(size_t)t * 3], lo, ext), t};
    std::sort(order.begin(), order.end());
    recs.resize((size_t)nk);
    const int nc = (nk + cluster - 1) / cluster;
    clus.resize((size_t)nc);
    for (int j = 0; j < nc; j++) {
        const int t0 = j * cluster, t1 = std::min(nk, t0 + cluster);
        double N[3] = {0, 0, 0}, wc[3] = {0, 0, 0}, wsum = 0.0;
        for (int i = t0; i < t1; i++) {
            const int t = order[i].second;
            const float *v = kept + (size_t)t * 9;
            fill_record(v, recs[i]);
            double e1[3], e2[3], n[3];
            for (int k = 0; k < 3; k++) {
                e1[k] = (double)v[3 + k] - (double)v[k];
                e2[k] = (double)v[6 + k] - (double)v[k];
            }
            n[0] = 0.5 * (e1[1] * e2[2] - e1[2] * e2[1]);
            n[1] = 0.5 * (e1[2] * e2[0] - e1[0] * e2[2]);
            n[2] = 0.5 * (e1[0] * e2[1] - e1[1] * e2[0]);
            const double area = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
            for (int k = 0; k < 3; k++) {
                N[k] += n[k];
                wc[k] += area * cen[(size_t)t * 3 + k];
            }
            wsum += area;
        }
        double c[3], r2 = 0.0;
        for (int k = 0; k < 3; k++) c[k] = wc[k] / wsum;
        for (int i = t0; i < t1; i++) {
            const float *v = kept + (size_t)order[i].second * 9;
            for (int p = 0; p < 3; p++) {
                const double dx = (double)v[3 * p] - c[0], dy = (double)v[3 * p + 1] - c[1], dz = (double)v[3 * p + 2] - c[2];
                r2 = std::max(r2, (dx * dx + dy * dy) + dz * dz);
            }
        }
        CRec &cr = clus[j];
        for (int k = 0; k < 3; k++) {
            cr.c[k] = (float)c[k];
            cr.n[k] = (float)N[k];
        }
        cr.r = (float)sqrt(r2);
        cr.pad = 0;
    }
}

struct ClusterSet {
    WRec *recs;
    CRec *clus;
    int nc;
};

// what a handle caches for the winding number: the records in kept order (exact arm), and one ClusterSet per `cluster` value used
struct Cache {
    WRec *kept = nullptr;
    std::map<int, ClusterSet> sets;
};

void destroy_cache(void *p)
{
    Cache *c = (Cache *)p;
    if (c->kept) (void)hipFree(c->kept);
    for (auto &kv : c->sets) {
        (void)hipFree(kv.second.recs);
        (void)hipFree(kv.second.clus);
    }
    delete c;
}

template <class T>
int upload(const std::vector<T> &h, T **d)
{
    return psi_upload(d, h.data(), h.size(), "psi_mesh_winding");
}

int launch(psi_mesh_sdf *m, const float gmin[3], const float gmax[3], int D, float beta, int cluster, float *d_f, unsigned long long *d_counts,
           void *stream)
{
    PSI_REQUIRE(m && gmin && gmax && (d_f || d_counts), "null pointer");
    Nodes ng;
    int rc = psi_mesh_node_steps(gmin, gmax, D, ng.step);
    if (rc != 0) return rc;
    PSI_REQUIRE(std::isfinite(beta) && beta >= 0.0f, "beta is finite and not negative");
    PSI_REQUIRE(cluster >= MIN_CLUSTER && cluster <= MAX_CLUSTER, "8 <= cluster <= 256");
    for (int k = 0; k < 3; k++) ng.gmin[k] = gmin[k];
    ng.D = D;

    // first use of this arm (of this cluster size): built on the host, uploaded between two device synchronisations, as create does
    psi_mesh_aux *aux = psi_mesh_sdf_aux(m);
    if (!aux->p) {
        aux->p = new Cache();
        aux->destroy = destroy_cache;
    }
    Cache *cache = (Cache *)aux->p;
    int nk = 0;
    const float *kept = psi_mesh_sdf_kept_tris(m, &nk);
    const WRec *recs = nullptr;
    const CRec *clus = nullptr;
    int nc = 0;
    if (beta == 0.0f) {
        if (!cache->kept) {
            std::vector<WRec> h;
            kept_records(kept, nk, h);
            PSI_CHECK_HIP(hipDeviceSynchronize());
            rc = upload(h, &cache->kept);
            if (rc != 0) return rc;
            PSI_CHECK_HIP(hipDeviceSynchronize());
        }
        recs = cache->kept;
    } else {
        auto it = cache->sets.find(cluster);
        if (it == cache->sets.end()) {
            std::vector<WRec> hr;
            std::vector<CRec> hc;
            build_clusters(kept, nk, cluster, hr, hc);
            ClusterSet cs{nullptr, nullptr, (int)hc.size()};
            PSI_CHECK_HIP(hipDeviceSynchronize());
            rc = upload(hr, &cs.recs);
            if (rc != 0) return rc;
            rc = upload(hc, &cs.clus);
            if (rc != 0) {
                (void)hipFree(cs.recs);
                return rc;
            }
            PSI_CHECK_HIP(hipDeviceSynchronize());
            it = cache->sets.emplace(cluster, cs).first;
        }
        recs = it->second.recs;
        clus = it->second.clus;
        nc = it->second.nc;
    }

    const int nb = psi_cdiv(D, BRICK);
    hipStream_t st = (hipStream_t)stream;
    if (d_counts) {
        PSI_CHECK_HIP(hipMemsetAsync(d_counts, 0, 16, st));
        hipLaunchKernelGGL(mwind_brick_kernel<true>, dim3(nb, nb, nb), dim3(WG), 0, st, recs, nk, clus, nc, cluster, beta, ng, d_f, d_counts);
    } else {
        hipLaunchKernelGGL(mwind_brick_kernel<false>, dim3(nb, nb, nb), dim3(WG), 0, st, recs, nk, clus, nc, cluster, beta, ng, d_f,
                           (unsigned long long *)nullptr);
    }
    PSI_CHECK_LAUNCH("mwind_brick_kernel");
    return 0;
}

}  // namespace psi_mwind

extern "C" int psi_mesh_winding_compute(psi_mesh_sdf *m, const float gmin[3], const float gmax[3], int D, float beta, int cluster, float *d_f,
                                        void *stream)
{
    PSI_REQUIRE(d_f, "null pointer");
    return psi_mwind::launch(m, gmin, gmax, D, beta, cluster, d_f, nullptr, stream);
}

extern "C" int psi_mesh_winding_count(psi_mesh_sdf *m, const float gmin[3], const float gmax[3], int D, float beta, int cluster,
                                      unsigned long long *d_counts, void *stream)
{
    PSI_REQUIRE(d_counts, "null pointer");
    return psi_mwind::launch(m, gmin, gmax, D, beta, cluster, nullptr, d_counts, stream);
}

extern "C" int psi_mesh_sdf_apply_sign(const float *d_f, float level, float *d_vol, long long n, void *stream)
{
    PSI_REQUIRE(d_f && d_vol, "null pointer");
    PSI_REQUIRE(n >= 1 && n <= (1ll << 31) * psi_mwind::WG, "1 <= n <= 2^39");
    PSI_REQUIRE(!std::isnan(level), "level is a number");
    hipLaunchKernelGGL(psi_mwind::mwind_apply_sign_kernel, dim3((unsigned)((n + psi_mwind::WG - 1) / psi_mwind::WG)), dim3(psi_mwind::WG), 0,
                       (hipStream_t)stream, d_f, level, d_vol, n);
    PSI_CHECK_LAUNCH("mwind_apply_sign_kernel");
    return 0;
}
