// Body against body: the rigid state of every body applied to its vertices, dL/dverts reduced to a force and a torque per body, and the
// optimiser step, for gfx950 (wave64).  The contract is DESIGN.md section 10h; the statements are csrc/body_separate_shared.h.  This file is
// compiled with -ffp-contract=off and IEEE division and square root.
//
// Kernels: pose (one lane per vertex; the body is blockIdx.y, so the ten state scalars and the nine entries of R are uniform over the wave:
// scalar loads, scalar registers), wrench (one workgroup per (body, chunk of 256 consecutive vertices): six fp64 terms per lane, the fixed
// tree s[l] += s[l + stride], stride = 128 .. 1 — the strides 128 and 64 through LDS, 32 .. 1 by lane shifts within wave 0, which adds the
// same pairs), step (eight lanes per body, six of them at work: lane c adds the chunk sums of component c in chunk order in fp64, rounds
// once, takes the Adam step of its component; lane 0 of the body then moves transl and the quaternion) and scene (the grid and the tree of
// wrench: one lane per vertex samples the body's scene volume and forms its own G; nothing per vertex is stored).  The sums use no
// floating-point atomics and do not depend on the shape of the grid.  No scratch.
#include "body_separate_shared.h"
#include "psi_common.h"
#include "wg_device.h"

namespace psi_bs {

constexpr int WG = WG_LANES;
static_assert(WG == BS_CHUNK, "one lane per vertex of a chunk");
constexpr int STEP_LANES = 64, STEP_PER_BODY = 8;

__device__ __forceinline__ bs3 bs_load(const float *__restrict__ p) { return bs_make(p[0], p[1], p[2]); }

__global__ __launch_bounds__(WG) void bs_pose_kernel(const float *__restrict__ base, const float *__restrict__ quat,
                                                     const float *__restrict__ transl, const float *__restrict__ pivot, int V,
                                                     float *__restrict__ verts)
{
    const int b = blockIdx.y;                                   // uniform: what follows up to `v` is scalar work
    BsQuat q;
    q.w = quat[4 * b], q.x = quat[4 * b + 1], q.y = quat[4 * b + 2], q.z = quat[4 * b + 3];
    const bs3 t = bs_load(transl + 3 * b), c = bs_load(pivot + 3 * b);
    const BsRot R = bs_rotation(q);
    const bs3 p = bs_centre(c, t);
    const bool same = bs_is_identity(q, t);
    const int v = blockIdx.x * WG + threadIdx.x;
    if (v >= V) return;
    const size_t at = ((size_t)b * V + v) * 3;
    const bs3 x = bs_pose(bs_load(base + at), R, c, p, same);
    verts[at] = x.x, verts[at + 1] = x.y, verts[at + 2] = x.z;
}

// The tree s[l] += s[l + stride], stride = 128 .. 1, of N values per lane over the 256 lanes of a workgroup: the strides 128 and 64 through
// LDS, 32 .. 1 by lane shifts within wave 0.  Every lane of the workgroup calls it; it returns false for the lanes past wave 0, and lane 0
// holds the sums.
template <int N>
__device__ __forceinline__ bool bs_tree(double (&a)[N], double (&s)[N][WG], int t)
{
    if (t >= 64) {
#pragma unroll
        for (int k = 0; k < N; k++) s[k][t] = a[k];
    }
    __syncthreads();
    if (t < 128) {                                              // stride 128
#pragma unroll
        for (int k = 0; k < N; k++) a[k] = a[k] + s[k][t + 128];
    }
    if (t >= 64 && t < 128) {                                   // its own slot, which stride 128 did not read
#pragma unroll
        for (int k = 0; k < N; k++) s[k][t] = a[k];
    }
    __syncthreads();
    if (t >= 64) return false;
#pragma unroll
    for (int k = 0; k < N; k++) {
        a[k] = a[k] + s[k][t + 64];                             // stride 64
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a[k] = a[k] + __shfl_down(a[k], o, 64);       // strides 32 .. 1: lane l takes lane l + o
    }
    return true;
}

// chunks [B, nchunk, 6] fp64: (F, T) of the vertices 256 k .. 256 k + 255 of body b; lanes past V hold +0
__global__ __launch_bounds__(WG) void bs_wrench_kernel(const float *__restrict__ verts, const float *__restrict__ G, const float *__restrict__ p,
                                                       int V, double *__restrict__ chunks)
{
    __shared__ double s[6][WG];
    const int b = blockIdx.y, t = threadIdx.x;
    const int v = blockIdx.x * WG + t;
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (v < V) {
        const size_t at = ((size_t)b * V + v) * 3;
        const bs3 g = bs_load(G + at);
        const bs3 c = bs_torque(bs_load(verts + at), bs_load(p + 3 * b), g);
        a[0] = (double)g.x, a[1] = (double)g.y, a[2] = (double)g.z, a[3] = (double)c.x, a[4] = (double)c.y, a[5] = (double)c.z;
    }
    if (!bs_tree<6>(a, s, t)) return;
    if (t == 0) {
        double *out = chunks + ((size_t)b * gridDim.x + blockIdx.x) * 6;
#pragma unroll
        for (int k = 0; k < 6; k++) out[k] = a[k];
    }
}

// The scene term (bs_scene_vertex): one lane per vertex gathers the eight corners of its cell in the body's scene volume; a vertex with
// value < 0 contributes G = (-w_scene) g, c = a x G and -value, every other lane +0.  Per chunk: the six sums, the fp64 sum of -value and
// the count (carried through the tree as a double: an integer <= 256 is exact).  The body, hence the scene, its box and p, is uniform over
// the workgroup.  sdf_out [B,V] and G_out [B,V,3] are written only when given.
__global__ __launch_bounds__(WG) void bs_scene_kernel(const float *__restrict__ verts, const float *__restrict__ p, const float *__restrict__ sdf,
                                                      const float *__restrict__ gmin, const float *__restrict__ gmax,
                                                      const int32_t *__restrict__ scene_id, int V, int D, int S, float w_scene,
                                                      double *__restrict__ chunks, int32_t *__restrict__ count, double *__restrict__ loss,
                                                      float *__restrict__ sdf_out, float *__restrict__ G_out)
{
    __shared__ double s[8][WG];
    const int b = blockIdx.y, t = threadIdx.x;
    const int sc = bs_scene_of(scene_id, b, S);
    const BsSceneBox box = bs_scene_box(gmin + 3 * sc, gmax + 3 * sc, D);
    const int v = blockIdx.x * WG + t;
    double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (v < V) {
        const size_t at = ((size_t)b * V + v) * 3;
        const bs3 x = bs_load(verts + at);
        bs3 g;
        bool inside;
        const BsSceneSample sm = bs_scene_vertex(sdf + (size_t)sc * D * D * D, D, box, x, w_scene, g, inside);
        if (inside) {
            const bs3 c = bs_torque(x, bs_load(p + 3 * b), g);
            a[0] = (double)g.x, a[1] = (double)g.y, a[2] = (double)g.z, a[3] = (double)c.x, a[4] = (double)c.y, a[5] = (double)c.z;
            a[6] = (double)(-sm.value), a[7] = 1.0;
        }
        if (sdf_out) sdf_out[(size_t)b * V + v] = sm.value;
        if (G_out) G_out[at] = g.x, G_out[at + 1] = g.y, G_out[at + 2] = g.z;
    }
    if (!bs_tree<8>(a, s, t)) return;
    if (t == 0) {
        const size_t ch = (size_t)b * gridDim.x + blockIdx.x;
#pragma unroll
        for (int k = 0; k < 6; k++) chunks[ch * 6 + k] = a[k];
        loss[ch] = a[6];
        count[ch] = (int32_t)a[7];
    }
}

// Lane (body, c) = (tid / 8, tid % 8).  chunks != null: g6[body, c] = (float) (((0 + chunk 0) + chunk 1) + ...) is computed and stored;
// otherwise it is read.  update == 0 stops there (the second stage of the wrench on its own).
__global__ __launch_bounds__(STEP_LANES) void bs_step_kernel(const double *__restrict__ chunks, int nchunk, float *__restrict__ g6,
                                                             float *__restrict__ quat, float *__restrict__ transl, float *__restrict__ m,
                                                             float *__restrict__ s, const int32_t *__restrict__ fixed, int B, int update,
                                                             BsStep K)
{
    const int tid = blockIdx.x * STEP_LANES + threadIdx.x;
    const int b = tid / STEP_PER_BODY, c = tid % STEP_PER_BODY;
    const bool live = b < B && c < 6;
    float g = 0.0f;
    if (live) {
        if (chunks) {
            double acc = 0.0;
            const double *row = chunks + (size_t)b * nchunk * 6 + c;
            for (int k = 0; k < nchunk; k++) acc = acc + row[(size_t)k * 6];
            g = (float)acc;
            g6[b * 6 + c] = g;
        } else {
            g = g6[b * 6 + c];
        }
    }
    if (!update) return;
    float u = 0.0f;
    if (live) {
        if (fixed && fixed[b] != 0) g = 0.0f;
        float mm = m[b * 6 + c], ss = s[b * 6 + c];
        u = bs_adam(mm, ss, g, K);
        m[b * 6 + c] = mm, s[b * 6 + c] = ss;
    }
    const int first = (threadIdx.x / STEP_PER_BODY) * STEP_PER_BODY;     // every lane of the wave takes part in the six reads
    const float u0 = __shfl(u, first, 64), u1 = __shfl(u, first + 1, 64), u2 = __shfl(u, first + 2, 64);
    const float u3 = __shfl(u, first + 3, 64), u4 = __shfl(u, first + 4, 64), u5 = __shfl(u, first + 5, 64);
    if (b < B && c == 0) {
        float *t = transl + 3 * b, *qq = quat + 4 * b;
        t[0] = t[0] - K.lr_t * u0, t[1] = t[1] - K.lr_t * u1, t[2] = t[2] - K.lr_t * u2;
        BsQuat q;
        q.w = qq[0], q.x = qq[1], q.y = qq[2], q.z = qq[3];
        q = bs_quat_step(q, bs_make(-(K.lr_r * u3), -(K.lr_r * u4), -(K.lr_r * u5)));
        qq[0] = q.w, qq[1] = q.x, qq[2] = q.y, qq[3] = q.z;
    }
}

}  // namespace psi_bs

#define BS_REQUIRE(B, V)                                                                                            \
    PSI_REQUIRE(B >= 1 && B <= GEOM_MAX_B, "1 <= B <= 46340");                                                      \
    PSI_REQUIRE(V >= 1 && V <= (1 << 24), "1 <= V <= 2^24")

extern "C" int psi_body_separate_pose(const float *d_base, const float *d_quat, const float *d_transl, const float *d_pivot, int B, int V,
                                      float *d_verts, void *stream)
{
    PSI_REQUIRE(d_base && d_quat && d_transl && d_pivot && d_verts, "null pointer");
    BS_REQUIRE(B, V);
    hipLaunchKernelGGL(psi_bs::bs_pose_kernel, dim3(psi_cdiv(V, psi_bs::WG), B), dim3(psi_bs::WG), 0, (hipStream_t)stream, d_base, d_quat,
                       d_transl, d_pivot, V, d_verts);
    PSI_CHECK_LAUNCH("bs_pose_kernel");
    return 0;
}

static int bs_launch_step(const double *d_chunks, int nchunk, float *d_g6, float *d_quat, float *d_transl, float *d_m, float *d_s,
                          const int32_t *d_fixed, int B, int update, BsStep K, hipStream_t st)
{
    hipLaunchKernelGGL(psi_bs::bs_step_kernel, dim3(psi_cdiv((long)B * psi_bs::STEP_PER_BODY, psi_bs::STEP_LANES)), dim3(psi_bs::STEP_LANES), 0,
                       st, d_chunks, nchunk, d_g6, d_quat, d_transl, d_m, d_s, d_fixed, B, update, K);
    PSI_CHECK_LAUNCH("bs_step_kernel");
    return 0;
}

extern "C" int psi_body_separate_wrench(const float *d_verts, const float *d_G, const float *d_p, int B, int V, double *d_chunks, float *d_g6,
                                        void *stream)
{
    PSI_REQUIRE(d_verts && d_G && d_p && d_chunks, "null pointer");
    BS_REQUIRE(B, V);
    const int nchunk = psi_cdiv(V, BS_CHUNK);
    hipLaunchKernelGGL(psi_bs::bs_wrench_kernel, dim3(nchunk, B), dim3(psi_bs::WG), 0, (hipStream_t)stream, d_verts, d_G, d_p, V, d_chunks);
    PSI_CHECK_LAUNCH("bs_wrench_kernel");
    if (!d_g6) return 0;
    return bs_launch_step(d_chunks, nchunk, d_g6, nullptr, nullptr, nullptr, nullptr, nullptr, B, 0, BsStep{}, (hipStream_t)stream);
}

extern "C" int psi_body_separate_scene(const float *d_verts, const float *d_p, const float *d_sdf, const float *d_gmin, const float *d_gmax,
                                       const int32_t *d_scene_id, int B, int V, int D, int S, float w_scene, double *d_chunks,
                                       int32_t *d_count, double *d_loss, float *d_sdf_out, float *d_G_out, void *stream)
{
    PSI_REQUIRE(d_verts && d_p && d_sdf && d_gmin && d_gmax && d_chunks && d_count && d_loss, "null pointer");
    BS_REQUIRE(B, V);
    PSI_REQUIRE(D >= 2 && S >= 1, "D >= 2, S >= 1");
    PSI_REQUIRE(w_scene >= 0.0f && w_scene < INFINITY, "w_scene >= 0, finite");
    hipLaunchKernelGGL(psi_bs::bs_scene_kernel, dim3(psi_cdiv(V, psi_bs::WG), B), dim3(psi_bs::WG), 0, (hipStream_t)stream, d_verts, d_p, d_sdf,
                       d_gmin, d_gmax, d_scene_id, V, D, S, w_scene, d_chunks, d_count, d_loss, d_sdf_out, d_G_out);
    PSI_CHECK_LAUNCH("bs_scene_kernel");
    return 0;
}

extern "C" int psi_body_separate_step(const double *d_chunks, int nchunk, float *d_g6, float *d_quat, float *d_transl, float *d_m, float *d_s,
                                      const int32_t *d_fixed, int B, float b1, float b2, float c1, float c2, float eps, float lr_t, float lr_r,
                                      void *stream)
{
    PSI_REQUIRE(d_g6 && d_quat && d_transl && d_m && d_s, "null pointer");
    PSI_REQUIRE(B >= 1 && B <= GEOM_MAX_B, "1 <= B <= 46340");
    PSI_REQUIRE(d_chunks ? (nchunk >= 1 && nchunk <= (1 << 16)) : nchunk == 0, "1 <= nchunk <= 2^16 with d_chunks, 0 without");
    PSI_REQUIRE(b1 >= 0.0f && b1 < 1.0f && b2 >= 0.0f && b2 < 1.0f, "0 <= beta < 1");
    PSI_REQUIRE(c1 > 0.0f && c1 <= 1.0f && c2 > 0.0f && c2 <= 1.0f, "0 < bias correction <= 1");
    PSI_REQUIRE(eps >= 0.0f && eps < INFINITY && lr_t > 0.0f && lr_t < INFINITY && lr_r > 0.0f && lr_r < INFINITY, "eps >= 0, lr > 0, finite");
    BsStep K;
    K.b1 = b1, K.b2 = b2, K.c1 = c1, K.c2 = c2, K.eps = eps, K.lr_t = lr_t, K.lr_r = lr_r;
    return bs_launch_step(d_chunks, nchunk, d_g6, d_quat, d_transl, d_m, d_s, d_fixed, B, 1, K, (hipStream_t)stream);
}
