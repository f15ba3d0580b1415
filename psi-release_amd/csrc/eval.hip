// Physical-plausibility evaluation for gfx950: per body the two integers the reference derives from a full vertex set,
//   n_neg = #(sdf < 0), n_pos = #(sdf > 0)                                  utils/utils_eval_collision_habitat.py:126-139
// without storing a vertex, an SDF value or a gradient.  The operator sequence (psi_lbs_forward -> psi_sdf_sample_forward -> two
// reductions) writes 10475 x 3 floats per body, reads them back and writes 10475 values for two counters; here the sign test rides
// on the skinning kernel as its epilogue (lbs_device.h: psi_skin_fwd_body), the way the fitting engine's SdfPenEpilogue does.
//   pose_fwd, blend_fwd   the stages of psi_lbs_forward (lbs.hip: psi_lbs_pose_blend_forward)
//   skin_fwd<SdfCountEpilogue>   NB = 1, grid (Vpad / 256, B) — the launch shape of psi_lbs_forward's skinning kernel, so a vertex goes
//                         through the same instruction sequence; the sample is psi_trilinear on the caller's plain [S,D,D,D] volume, the
//                         function sdf_sample_kernel calls.
// Counters are integers added with one atomicAdd per workgroup, body and counter: order-independent, so run-to-run identical.
#include "psi_internal.h"
#include "lbs_device.h"
#include "sdf_device.h"

namespace {

struct SdfCountEpilogue {
    const float *sdf, *gmin, *gmax;
    const int *scene_id;          // [B] or nullptr (scene 0); values are clamped to [0, S)
    int *counts;                  // [B][2] = { #(sdf < 0), #(sdf > 0) }, zeroed before the launch
    int D, S, align_corners;
    bool neg, pos;
    __device__ __forceinline__ void backward(int, int, unsigned, const psi_f2 (&)[6], const float *) {}
    __device__ __forceinline__ void store(float *, size_t, int, int, unsigned, float, float, float) const {}
    __device__ __forceinline__ void vertex(int, int b, int, float x, float y, float z, bool live)
    {
        neg = pos = false;
        if (!live) return;
        // b is uniform over the workgroup: one scalar load, not one per lane
        const int s = scene_id ? min(max(__builtin_amdgcn_readfirstlane(scene_id[b]), 0), S - 1) : 0;
        const float val = psi_trilinear(sdf + (size_t)s * D * D * D, gmin + s * 3, gmax + s * 3, x, y, z, D, align_corners, nullptr);
        neg = val < 0.0f;
        pos = val > 0.0f;
    }
    __device__ __forceinline__ void finish(int, int b, int, int)
    {
        __shared__ int red[PSI_SKIN_BLK / 64][2];
        const int wn = (int)__builtin_popcountll(__builtin_amdgcn_ballot_w64(neg));
        const int wp = (int)__builtin_popcountll(__builtin_amdgcn_ballot_w64(pos));
        if ((threadIdx.x & 63) == 0) {
            red[threadIdx.x >> 6][0] = wn;
            red[threadIdx.x >> 6][1] = wp;
        }
        __syncthreads();
        if (threadIdx.x < 2) {
            int a = 0;
#pragma unroll
            for (int w = 0; w < PSI_SKIN_BLK / 64; w++) a += red[w][threadIdx.x];
            if (a) atomicAdd(counts + (size_t)b * 2 + threadIdx.x, a);
        }
    }
};

}  // namespace

extern "C" int psi_lbs_sdf_counts(const psi_lbs_model *model, const float *betas, const float *pose, const float *transl,
                                  const float *cam_ext, int B, const float *sdf, const int32_t *scene_id, const float *gmin,
                                  const float *gmax, int D, int S, int align_corners, int32_t *counts, float *ws, void *stream)
{
    PSI_REQUIRE(model && betas && pose && ws, "null pointer");
    PSI_REQUIRE(counts && sdf && gmin && gmax, "null pointer");
    PSI_REQUIRE(B >= 1 && B <= 16384, "batch size out of range");
    PSI_REQUIRE(S >= 1 && D >= 2, "grid dim must be >= 2 and at least one scene");
    hipStream_t st = (hipStream_t)stream;
    PSI_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)B * 2 * sizeof(int32_t), st));
    int rc = psi_lbs_pose_blend_forward(model, betas, pose, transl, B, ws, st);
    if (rc) return rc;
    PsiLbsView lv;
    rc = psi_lbs_view(model, B, ws, &lv);
    if (rc) return rc;
    SdfCountEpilogue epi = {sdf, gmin, gmax, scene_id, counts, D, S, align_corners, false, false};
    hipLaunchKernelGGL(psi_skin_fwd_kernel<SdfCountEpilogue>, dim3(lv.m.Vpad / PSI_SKIN_BLK, B), dim3(PSI_SKIN_BLK), 0, st, lv.m, lv.A,
                       lv.v_posed, transl, cam_ext, B, (float *)nullptr, epi);
    PSI_CHECK_LAUNCH("skin_fwd_kernel<SdfCountEpilogue>");
    psi_mark("skin_count_kernel", st);
    return 0;
}
