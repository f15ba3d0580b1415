// psi_flood_fill, psi_mesh_orient_votes: the two device steps of scene_sdf.orient_faces.
//
//   flood_seed_kernel   one thread per seed node: an open seed node inside the grid becomes free.
//   flood_brick_kernel  one WAVE per 8 x 8 x 8 brick of nodes.  The brick and its one-node apron are 10 x 10 rows along z of 10 bits each
//                       in LDS; lane (x, y) owns the row of its 8 nodes.  The brick is flooded to convergence locally (a row spreads
//                       along z with shifts, across rows through the four neighbouring words), the nodes it gained are written, and the
//                       launch's word is raised (integer atomicOr) when the brick gained a node.  psi_flood_fill launches it until a
//                       launch raises nothing; it reads the words of 8 launches back at a time.
//   orient_votes_kernel one lane per sample: the unit normal of the sample's triangle, the two probes p +- delta n, their nearest nodes,
//                       and an integer atomicAdd per free probe (one per wave when the whole wave samples one triangle).
//
// A launch is a function of the state the launch before it left, whatever the order of its workgroups, so not only the set but also the
// number of launches is the same from run to run.  A byte of d_free is 0 (not free), 1 (free) or, between two launches, the stamp
// 2 + (k & 1) of the launch k that gained the node.  Launch k reads a neighbour's node as free when its byte is 1 or carries the stamp of
// launch k - 1, never its own stamp; each brick rewrites the stamps of launch k - 1 among its own nodes to 1 (a neighbour reads either
// value as free).  A launch that gains nothing therefore leaves only 0 and 1 behind.  No floating-point atomics; the trip counts of the
// local loops depend on the brick's own bits alone (at most one trip per node of the brick), and no lane waits for another workgroup.
// Compiled with -ffp-contract=off: the votes are the statements of section 10c, operation by operation.
#include "psi_common.h"

namespace psi_orient {

constexpr int BRICK = 8;
constexpr int SIDE = BRICK + 2;                  // with the apron
constexpr int ROWS = SIDE * SIDE;
constexpr unsigned OWN = 0x1feu;                 // bits 1 .. 8 of a row: the brick's own nodes; bits 0 and 9 are the apron along z
constexpr int BATCH = 8;                         // launches between two reads of the words
constexpr int VOTE_WG = 256;

__global__ void flood_seed_kernel(const uint8_t *__restrict__ open, int Dx, int Dy, int Dz, const int32_t *__restrict__ seeds, int n,
                                  uint8_t *__restrict__ free_)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int x = seeds[i * 3 + 0], y = seeds[i * 3 + 1], z = seeds[i * 3 + 2];
    if (x < 0 || x >= Dx || y < 0 || y >= Dy || z < 0 || z >= Dz) return;
    const size_t at = ((size_t)x * Dy + y) * Dz + z;
    if (open[at]) free_[at] = 1;                 // several seeds on one node store the same byte
}

__global__ __launch_bounds__(PSI_WAVE) void flood_brick_kernel(const uint8_t *__restrict__ open, int Dx, int Dy, int Dz, int nby, int nbz,
                                                               uint8_t *free_, unsigned stamp, unsigned *__restrict__ changed)
{
    __shared__ unsigned s_open[ROWS], s_free[ROWS], s_norm[ROWS];
    const int lane = threadIdx.x;
    const long brick = blockIdx.x;
    const int bz = (int)(brick % nbz), by = (int)((brick / nbz) % nby), bx = (int)(brick / ((long)nbz * nby));
    const int x0 = bx * BRICK - 1, y0 = by * BRICK - 1, z0 = bz * BRICK - 1;      // the apron's corner

    // the free bits first: a brick without a free node in reach has nothing to do and never reads the mask
    unsigned any = 0;
    for (int r = lane; r < ROWS; r += PSI_WAVE) {
        const int ax = r / SIDE, ay = r % SIDE, gx = x0 + ax, gy = y0 + ay;
        const bool own_row = ax >= 1 && ax <= BRICK && ay >= 1 && ay <= BRICK;
        unsigned f = 0, nm = 0;
        if (gx >= 0 && gx < Dx && gy >= 0 && gy < Dy) {
            const uint8_t *row = free_ + ((size_t)gx * Dy + gy) * Dz;
            for (int i = 0; i < SIDE; i++) {
                const int gz = z0 + i;
                if (gz < 0 || gz >= Dz) continue;
                const unsigned b = row[gz];
                const bool own = own_row && i >= 1 && i <= BRICK;
                if (own ? b != 0u : (b != 0u && b != stamp)) f |= 1u << i;
                if (own && b >= 2u) nm |= 1u << i;
            }
        }
        s_free[r] = f;
        s_norm[r] = nm;
        any |= f | nm;
    }
    if (!__syncthreads_or((int)(any != 0u))) return;

    for (int r = lane; r < ROWS; r += PSI_WAVE) {
        const int ax = r / SIDE, ay = r % SIDE, gx = x0 + ax, gy = y0 + ay;
        unsigned o = 0;
        if (gx >= 0 && gx < Dx && gy >= 0 && gy < Dy) {
            const uint8_t *row = open + ((size_t)gx * Dy + gy) * Dz;
            for (int i = 0; i < SIDE; i++) {
                const int gz = z0 + i;
                if (gz >= 0 && gz < Dz && row[gz]) o |= 1u << i;
            }
        }
        s_open[r] = o;
        s_free[r] &= o;                          // a free node is an open node
    }
    __syncthreads();

    const int r = (lane / BRICK + 1) * SIDE + (lane % BRICK + 1);                 // the lane's own row
    const unsigned o = s_open[r] & OWN, f0 = s_free[r];
    unsigned f = f0;
    for (;;) {
        const unsigned nb = s_free[r - SIDE] | s_free[r + SIDE] | s_free[r - 1] | s_free[r + 1];
        unsigned g = f | (nb & o);
        for (;;) {                               // along z: at most 8 trips
            const unsigned g2 = g | (((g << 1) | (g >> 1)) & o);
            if (g2 == g) break;
            g = g2;
        }
        const int grew = g != f;
        __syncthreads();                         // every lane has read its neighbours' words
        f = g;
        s_free[r] = f;
        if (!__syncthreads_or(grew)) break;      // every trip but the last gains a node: at most 513 trips
    }

    const unsigned gained = f & ~f0 & OWN, nm = s_norm[r] & ~gained;
    const int gx = x0 + lane / BRICK + 1, gy = y0 + lane % BRICK + 1;
    if ((gained | nm) != 0u) {                   // then the row lies inside the grid, and so does every node of these bits (they are open)
        uint8_t *row = free_ + ((size_t)gx * Dy + gy) * Dz;
        for (int i = 1; i <= BRICK; i++) {
            const int gz = z0 + i;
            if (gz >= Dz) break;
            if (gained >> i & 1u) row[gz] = (uint8_t)stamp;
            else if (nm >> i & 1u) row[gz] = 1;
        }
    }
    if (__syncthreads_or((int)(gained != 0u)) && lane == 0) atomicOr(changed, 1u);
}

struct VoteArgs {
    float gmin[3], step[3];
    float last;                                  // (float)(D - 1)
    float delta;
    int D, nv, nf;
};

// 1 iff the node nearest to q lies inside the grid and is free
__device__ __forceinline__ int probe_free(const float q[3], const VoteArgs &a, const uint8_t *__restrict__ free_)
{
    int idx[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float r = rintf((q[k] - a.gmin[k]) / a.step[k]);
        if (!(r >= 0.0f && r <= a.last)) return 0;                                // also a NaN
        idx[k] = (int)r;
    }
    return free_[((size_t)idx[0] * a.D + idx[1]) * a.D + idx[2]] != 0;
}

__global__ __launch_bounds__(VOTE_WG) void orient_votes_kernel(const float *__restrict__ points, const int32_t *__restrict__ tri, long n,
                                                               const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                               const uint8_t *__restrict__ free_, VoteArgs a, int32_t *__restrict__ votes)
{
    const long i = (long)blockIdx.x * VOTE_WG + threadIdx.x;
    int t = -1, front = 0, back = 0;
    if (i < n) {
        t = tri[i];
        if (t < 0 || t >= a.nf) t = -1;
    }
    if (t >= 0) {
        const int i0 = faces[(size_t)t * 3 + 0], i1 = faces[(size_t)t * 3 + 1], i2 = faces[(size_t)t * 3 + 2];
        if (i0 < 0 || i0 >= a.nv || i1 < 0 || i1 >= a.nv || i2 < 0 || i2 >= a.nv) {
            t = -1;
        } else {
            float u[3], v[3], p[3];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const float ak = verts[(size_t)i0 * 3 + k];
                u[k] = verts[(size_t)i1 * 3 + k] - ak;
                v[k] = verts[(size_t)i2 * 3 + k] - ak;
                p[k] = points[(size_t)i * 3 + k];
            }
            const float c[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
            const float len = sqrtf((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
            if (len > 0.0f) {                    // a triangle without area (or with a non-finite corner) casts no vote
                float qf[3], qb[3];
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const float d = a.delta * (c[k] / len);
                    qf[k] = p[k] + d;
                    qb[k] = p[k] - d;
                }
                front = probe_free(qf, a, free_);
                back = probe_free(qb, a, free_);
            }
        }
    }
    // the cloud lists its points triangle by triangle, so most waves sample one triangle: one atomic per wave and side
    const int t0 = __shfl(t, 0);
    if (__all(t == t0)) {
        const int nfr = __popcll(__ballot(front)), nbk = __popcll(__ballot(back));
        if ((threadIdx.x & (PSI_WAVE - 1)) == 0 && t0 >= 0) {
            if (nfr) atomicAdd(&votes[(size_t)t0 * 2 + 0], nfr);
            if (nbk) atomicAdd(&votes[(size_t)t0 * 2 + 1], nbk);
        }
    } else if (t >= 0) {
        if (front) atomicAdd(&votes[(size_t)t * 2 + 0], 1);
        if (back) atomicAdd(&votes[(size_t)t * 2 + 1], 1);
    }
}

}  // namespace psi_orient

using namespace psi_orient;

extern "C" int psi_flood_fill(const uint8_t *d_open, int Dx, int Dy, int Dz, const int32_t *d_seed_nodes, int n, uint8_t *d_free, int *h_rounds,
                              void *stream)
{
    PSI_REQUIRE(d_open && d_seed_nodes && d_free && d_open != d_free, "null pointer");
    PSI_REQUIRE(Dx >= 2 && Dx <= 1024 && Dy >= 2 && Dy <= 1024 && Dz >= 2 && Dz <= 1024, "every edge lies in 2 .. 1024");
    PSI_REQUIRE(n >= 1, "at least one seed node");
    hipStream_t st = (hipStream_t)stream;
    const size_t nodes = (size_t)Dx * Dy * Dz;
    const int nbx = psi_cdiv(Dx, BRICK), nby = psi_cdiv(Dy, BRICK), nbz = psi_cdiv(Dz, BRICK);
    const long bricks = (long)nbx * nby * nbz;                                    // at most 128^3
    unsigned *d_words = (unsigned *)psi_scratch(BATCH * sizeof(unsigned), st);
    if (!d_words) return PSI_EINVAL;
    PSI_CHECK_HIP(hipMemsetAsync(d_free, 0, nodes, st));
    hipLaunchKernelGGL(flood_seed_kernel, dim3(psi_cdiv(n, 256)), dim3(256), 0, st, d_open, Dx, Dy, Dz, d_seed_nodes, n, d_free);
    PSI_CHECK_LAUNCH("flood_seed_kernel");
    // every launch but the last gains a node, so nodes + 1 launches always suffice; the bound only keeps a broken device from looping
    long launches = 0;
    for (;;) {
        unsigned h_words[BATCH];
        PSI_CHECK_HIP(hipMemsetAsync(d_words, 0, sizeof(h_words), st));
        for (int k = 0; k < BATCH; k++, launches++) {
            hipLaunchKernelGGL(flood_brick_kernel, dim3((unsigned)bricks), dim3(PSI_WAVE), 0, st, d_open, Dx, Dy, Dz, nby, nbz, d_free,
                               2u + (unsigned)(launches & 1), d_words + k);
            PSI_CHECK_LAUNCH("flood_brick_kernel");
        }
        PSI_CHECK_HIP(hipMemcpyAsync(h_words, d_words, sizeof(h_words), hipMemcpyDeviceToHost, st));
        PSI_CHECK_HIP(hipStreamSynchronize(st));
        for (int k = 0; k < BATCH; k++)
            if (!h_words[k]) {                   // launch k gained nothing: the launches after it did not either
                if (h_rounds) *h_rounds = (int)(launches - BATCH + k + 1);
                return 0;
            }
        if (launches > (long)nodes + BATCH) {
            psi_set_error("psi_flood_fill: no fixed point after %ld launches", launches);
            return PSI_EINVAL;
        }
    }
}

extern "C" int psi_mesh_orient_votes(const float *d_points, const int32_t *d_tri, long long n, const float *d_verts, int nv, const int32_t *d_faces,
                                     int nf, const uint8_t *d_free, const float gmin[3], const float gmax[3], int D, float delta,
                                     int32_t *d_votes, void *stream)
{
    PSI_REQUIRE(d_points && d_tri && d_verts && d_faces && d_free && d_votes && gmin && gmax, "null pointer");
    PSI_REQUIRE(n >= 0 && n < (1LL << 31) && nv >= 1 && nf >= 1, "0 <= n < 2^31, nv >= 1, nf >= 1");
    PSI_REQUIRE(D >= 2 && D <= 1024, "2 <= D <= 1024");
    PSI_REQUIRE(delta > 0.0f && delta < INFINITY, "delta is positive and finite");
    VoteArgs a;
    for (int k = 0; k < 3; k++) {
        PSI_REQUIRE(gmin[k] - gmin[k] == 0.0f && gmax[k] - gmax[k] == 0.0f && gmax[k] > gmin[k], "finite bounds with gmax > gmin");
        a.gmin[k] = gmin[k];
        a.step[k] = (gmax[k] - gmin[k]) / (float)(D - 1);                         // the spacing of psi_mesh_sdf_compute's nodes
        PSI_REQUIRE(a.step[k] > 0.0f, "a node spacing that is positive in fp32");
    }
    a.last = (float)(D - 1);
    a.delta = delta;
    a.D = D;
    a.nv = nv;
    a.nf = nf;
    hipStream_t st = (hipStream_t)stream;
    PSI_CHECK_HIP(hipMemsetAsync(d_votes, 0, (size_t)nf * 2 * sizeof(int32_t), st));
    if (n == 0) return 0;
    hipLaunchKernelGGL(orient_votes_kernel, dim3(psi_cdiv(n, VOTE_WG)), dim3(VOTE_WG), 0, st, d_points, d_tri, (long)n, d_verts, d_faces, d_free,
                       a, d_votes);
    PSI_CHECK_LAUNCH("orient_votes_kernel");
    return 0;
}
