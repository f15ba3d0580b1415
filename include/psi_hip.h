/*
 * psi_hip.h — C ABI of libpsi_hip.so, the MI355X (gfx950) implementation of PSI's
 * generation-and-fitting hot path.  Plain pointers and sizes only; every pointer is DEVICE memory
 * unless the name starts with h_.  `stream` is a hipStream_t passed as void* (NULL = default stream).
 *
 * Each entry point names the reference interface it replaces (paths relative to the
 * yz-cnsdqz/PSI-release checkout).  How a maintainer binds these from the reference's Python is
 * shown in INTEGRATION.md; this build's own binding is psi-release_amd/hip.py (ctypes).
 *
 * Error convention: every function returns 0 on success, otherwise a hipError_t value (or a
 * negative PSI_E* code for argument errors); psi_last_error() returns a static message.  The
 * reference's pybind functions returned 1/0 and printed (chamfer.cu:145-151); callers ignored it.
 * No entry point synchronises the host; all work is enqueued on `stream`.
 */
#ifndef PSI_HIP_H
#define PSI_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSI_EINVAL (-22)
#define PSI_ETIMEOUT (-110)   /* psi_stream_wait: the stream was still busy at the bound */
#define PSI_ENOMEM (-12)

const char *psi_last_error(void);
int psi_version(void);
/* Device facts for the bench roofline: CU count, wave size, clock (kHz), 1 if the device is gfx950. */
int psi_device_info(int *cu_count, int *wave_size, int *clock_khz, int *is_gfx950);

/* ---------------------------------------------------------------------------------------------
 * Chamfer nearest neighbour — replaces the `chamfer` CUDA extension
 *   chamfer.forward (xyz1, xyz2, dist1, dist2, idx1, idx2)            chamfer_cuda.cpp:17-19,30-31
 *     -> chamfer_cuda_forward / NmDistanceKernel x2                  chamfer.cu:12-154
 *   chamfer.backward(xyz1, xyz2, gradxyz1, gradxyz2, graddist1, graddist2, idx1, idx2)
 *                                                                     chamfer_cuda.cpp:22-27,32
 *     -> chamfer_cuda_backward / NmDistanceGradKernel x2             chamfer.cu:155-196
 * xyz1 [B,n,3], xyz2 [B,m,3] contiguous fp32; dist1 [B,n], dist2 [B,m] fp32; idx1, idx2 int32.
 * dist = min_k (x2-x1)^2+(y2-y1)^2+(z2-z1)^2 evaluated in fp32 left-to-right without FMA
 * contraction; idx = lowest k attaining it (first-minimum rule of chamfer.cu:46,126).
 * dist2/idx2 may both be NULL: PSI discards that direction (fitting_proxe.py:136) and it is skipped.
 * `workspace` (device, >= psi_chamfer_workspace_bytes) holds per-slice partial minima; NULL lets the
 * library use an internal buffer owned by (device, stream) that grows on demand — calls on different
 * streams never share it; growth is refused (PSI_ENOMEM) while the stream is being captured into a
 * hipGraph, so captured callers pass their own workspace.
 * ------------------------------------------------------------------------------------------- */
/* Arithmetic mode of the distance expression this library was built with: 0 = three products and two sums, each rounded
 * (the CUDA source as written, nvcc --fmad=false) — libpsi_hip.so; 1 = mul, fma, fma (nvcc's default --fmad=true contraction
 * of chamfer.cu:32-35) — libpsi_hip_fma.so, selected by PSI_CHAMFER_FMA=1.  Indices can differ between the two only where two
 * targets are within an ulp of the same distance. */
int psi_chamfer_arith_mode(void);
size_t psi_chamfer_workspace_bytes(int B, int n, int m);
int psi_chamfer_forward(const float *xyz1, const float *xyz2, int B, int n, int m,
                        float *dist1, int32_t *idx1, float *dist2, int32_t *idx2,
                        void *workspace, void *stream);
/* Frees the library's internal scratch buffer of `stream` on the current device (all != 0: of every stream of every device).  The
 * buffers behind `workspace = NULL` are per (device, stream) and otherwise live as long as the process; call this before destroying a
 * stream that was used with workspace = NULL. */
int psi_scratch_release(void *stream, int all);
/* Accumulates (+=) into gradxyz1 [B,n,3] / gradxyz2 [B,m,3] exactly like the reference, which is
 * handed zero-filled buffers (dist_chamfer.py:40-45).  gradxyz2 may be NULL (scene needs no grad);
 * graddist2/idx2 may be NULL (then direction 2 contributes nothing). */
int psi_chamfer_backward(const float *xyz1, const float *xyz2, float *gradxyz1, float *gradxyz2,
                         const float *graddist1, const float *graddist2,
                         const int32_t *idx1, const int32_t *idx2, int B, int n, int m, void *stream);

/* Exact NN index over a STATIC target cloud (one scene's vertices, fitting_proxe.py:93-96 loads them once per
 * FittingOP).  psi_nn_index_query returns exactly what psi_chamfer_forward returns for direction 1 against that
 * cloud (bit-identical dist1 / idx1, same first-minimum rule) at a fraction of the pair evaluations: a kd-tree
 * prunes only targets that provably cannot attain or tie the minimum.  h_points: HOST [m,3]. */
typedef struct psi_nn_index psi_nn_index;
int psi_nn_index_create(psi_nn_index **out, const float *h_points, int m);
void psi_nn_index_destroy(psi_nn_index *index);
/* hint (device int32 [B,n], nullable): warm start — on entry the target index that won for each query last time
 * (-1 = none), on exit this call's idx1.  It only seeds the search bound with a real candidate; results are unchanged. */
int psi_nn_index_query(const psi_nn_index *index, const float *xyz1, int B, int n, float *dist1, int32_t *idx1,
                       int32_t *hint, void *stream);

/* A set of scene indices queried in ONE launch with a per-body scene slot: body b is searched in indices[slot[b]]
 * (slot: device int32 [B], values in [0,S)).  This is the training-time pattern — every body of a batch brings its own
 * PROX scene (train_s1.py:159-169 gathers scene_verts [B,m,3] from batch_gen_hdf5.py:222-257 and calls chamfer.forward);
 * dist1/idx1 are bit-identical to psi_chamfer_forward on that gathered [B,m,3] tensor.  The set borrows the indices,
 * which must outlive it. */
typedef struct psi_nn_index_set psi_nn_index_set;
int psi_nn_index_set_create(psi_nn_index_set **out, const psi_nn_index *const *indices, int S);
void psi_nn_index_set_destroy(psi_nn_index_set *set);
int psi_nn_index_set_query(const psi_nn_index_set *set, const int32_t *slot, const float *xyz1, int B, int n,
                           float *dist1, int32_t *idx1, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Trilinear SDF lookup with analytic gradient — replaces
 *   F.grid_sample(sdf[B,1,D,D,D], norm_verts[:,:,[2,1,0]].view(-1,V,1,1,3), padding_mode='border')
 *                                    fitting_proxe.py:144-151, train_s1.py:183-190, train_s2.py:182-189
 * including the normalisation (v-min)/(max-min)*2-1 of fitting_proxe.py:147.
 * sdf [S,D,D,D] fp32, element [s][ix][iy][iz] (C order, fitting_proxe.py:85) — ONE volume per scene,
 * scene_id [B] int32 selects it per batch row (NULL = scene 0); the reference replicates the volume
 * B times (fitting_proxe.py:90).  gmin,gmax [S,3]; verts [B,V,3]; out_sdf [B,V];
 * out_grad [B,V,3] = d sdf / d vert (NULL to skip).  align_corners: 1 = torch 1.2.0 (pinned)
 * semantics, 0 = torch>=1.3 default.
 * psi_sdf_sample_backward: grad_verts[b,v,:] += grad_sdf[b,v] * out_grad[b,v,:].
 * ------------------------------------------------------------------------------------------- */
int psi_sdf_sample_forward(const float *sdf, const int32_t *scene_id, const float *gmin, const float *gmax,
                           const float *verts, int B, int V, int D, int S, int align_corners,
                           float *out_sdf, float *out_grad, void *stream);
int psi_sdf_sample_backward(const float *grad_sdf, const float *out_grad, int B, int V,
                            float *grad_verts, void *stream);
/* Penetration statistics of fitting_proxe.py:155-158 without the .item() host sync:
 * stats[0] = sum_{sdf<0} |sdf|, stats[1] = count(sdf<0) (as float, exact below 2^24), over n values.
 * stats must be zeroed by the caller (the result is ADDED to it; per-block partial sums combined in block order: no atomics,
 * run-to-run bit-identical). */
int psi_sdf_penetration_stats(const float *sdf_vals, long n, float *stats, void *stream);

/* ---------------------------------------------------------------------------------------------
 * SMPL-X linear blend skinning — replaces the body-model call
 *   smplx.create(path, model_type='smplx', ..., batch_size=B)(return_verts=True, body_pose=..., ...)
 *                                                       fitting_proxe.py:55-69,125-128; train_s1.py:66-81,150-153
 * whose arithmetic is lbs() (human_body_prior/body_model/lbs.py:34-118 == smplx 0.1.13 lbs), plus
 * `vertices + transl` and, when cam_ext is given, GeometryTransformer.verts_transform (cvae.py:141-149).
 * psi_lbs_create takes HOST arrays laid out as the SMPL-X loader leaves them:
 *   v_template [V,3]; shapedirs [V,3,NB] (betas | expression); posedirs [P,3V], P=(J-1)*9
 *   (i.e. reshape(posedirs,[-1,P]).T); J_regressor [J,V]; weights [V,J]; parents [J] (-1 for the root).
 * Forward inputs (device): betas [B,NB] (shape | expression), pose [B,J*3] axis-angle of ALL joints
 * (after hand PCA and pose_mean), transl [B,3] or NULL, cam_ext [B,4,4] row-major or NULL.
 * Outputs: verts [B,V,3]; joints [B,J,3] or NULL (posed joints + transl, no camera transform).
 * ws: psi_lbs_workspace_floats(model,B) floats of device scratch; forward saves what backward needs
 * there, so the same ws must be passed to the matching psi_lbs_backward.
 * Backward: grad_verts [B,V,3] -> grad_betas [B,NB], grad_pose [B,J*3], grad_transl [B,3] (each
 * nullable, each OVERWRITTEN).  Joints are not differentiated (PSI reads .vertices only).
 * Arithmetic: fp32 throughout; the blend-shape product v_template + [betas | R - I] . dirs (lbs.py:81,94-99) is formed on the fp16
 * matrix pipe as three split products of two fp16 parts per operand (22 mantissa bits, exact power-of-two scales, fp32 accumulation):
 * 2^-22 relative per product, the accuracy class of an fp32 product chain (tests/test_lbs_gpu.py holds it to fp64 with the margin an
 * fp32 evaluation needs).  |betas| beyond 4094 saturate (the feature rows' fixed scale).  The backward product g_feat = g_vposed . dirs^T
 * is formed the same way, each body's gradient rows scaled by that body's own largest entry (psi_lbs_backward: a row-maximum pass; the
 * fitting engine below: recorded per body by the kernels that write the rows), so that a body's accuracy and bits do not depend on the
 * other bodies of the batch — a body with Inf / NaN gradient entries gets non-finite gradients itself and leaves the others unchanged.
 * ------------------------------------------------------------------------------------------- */
typedef struct psi_lbs_model psi_lbs_model;
int psi_lbs_create(psi_lbs_model **out, const float *h_v_template, const float *h_shapedirs,
                   const float *h_posedirs, const float *h_J_regressor, const float *h_weights,
                   const int32_t *h_parents, int V, int J, int NB);
void psi_lbs_destroy(psi_lbs_model *model);
size_t psi_lbs_workspace_floats(const psi_lbs_model *model, int B);
int psi_lbs_forward(const psi_lbs_model *model, const float *betas, const float *pose, const float *transl,
                    const float *cam_ext, int B, float *verts, float *joints, float *ws, void *stream);
int psi_lbs_backward(const psi_lbs_model *model, const float *grad_verts, const float *betas, const float *pose,
                     const float *cam_ext, int B, float *ws, float *grad_betas, float *grad_pose,
                     float *grad_transl, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Fused fitting engine — replaces the loop body of FittingOP.fitting / cal_loss
 *   for ii in range(num_iter): optimizer.zero_grad(); cal_loss(...); loss.backward(); optimizer.step()
 *                                                                      fitting_proxe.py:101-162,177-189
 * (fitting_habitat.py:103-208 is the same with contact_const = 1.0 and a pre-multiplied camera).
 * One iteration = ~16 stream-ordered HIP kernels, no autograd, no host sync; psi_fit_iterate replays it
 * as a hipGraph.  State (device, owned by the engine): x = xhr_rec [B,75] (transl 3 | 6D rot 6 | betas 10 |
 * VPoser latent 32 | hand PCA 12+12), Adam moments and step count (fitting_proxe.py:73-74: the optimizer
 * persists across files unless reset).
 * psi_fit_create: h_* are HOST arrays.  VPoser decoder weights in nn.Linear layout [out,in]
 * (bodyprior_dec_fc1 [512,32], _fc2 [512,512], _out [126,512], vposer_smpl.py:83-89); hand PCA components
 * [num_pca_comps,45] each; pose_mean [165]; contact vertex ids [n_contact] in the order
 * GeometryTransformer.get_contact_id returns them (cvae.py:99-115).  d_scene_verts [m,3] and d_sdf [D,D,D]
 * are DEVICE arrays owned by the caller and must outlive the engine (one copy per scene, shared by the batch).
 * Data parallel: world_size > 1 scales the loss normalisers by the global batch B*world_size; the caller
 * runs psi_fit_forward(stats) -> all-reduce(sum) of stats[0..5] -> psi_fit_backward_step(stats) per iteration
 * (stats = [sum|xhr-x|, sum z^2, sum s/(s+c), sum|sdf<0|, count(sdf<0), 0], a caller-owned device buffer).
 * ------------------------------------------------------------------------------------------- */
typedef struct psi_fit_engine psi_fit_engine;
typedef struct psi_fit_config {
    int B, n_contact, m_scene, D, align_corners, world_size, num_pca_comps, max_history;
    int nn_mode;   /* 0 = brute-force Chamfer kernel, 1 = exact kd-tree index built from the scene cloud at create */
    float w_rec, w_vposer, w_contact, w_collision, contact_const;
    float lr, beta1, beta2, eps;
    int independent_bodies;   /* != 0: the B bodies are B INDEPENDENT problems — every loss is normalised per body (rec / 75, prior / 32,
                                 contact / n_contact, penetration / that body's own count), so one engine run over B bodies equals B runs of
                                 the reference's loop at batch size 1 (one generated-body file each, fitting_proxe.py:252-263).  world_size 1. */
    int concurrent_engines;   /* how many engines the caller keeps in flight on this GPU at the same time (other streams; 0 or 1 = this one
                                 alone).  The per-body head / tail kernels spread a body over up to 8 workgroups so that a lone engine with
                                 few bodies still covers the chip; engines that share the chip are told not to (B x engines x width <= 256). */
    double lr_d, beta1_d, beta2_d;   /* the Adam hyper-parameters as DOUBLES, the way torch.optim.Adam (fitting_proxe.py:73-74) holds them: it forms
                                 1 - beta and the bias corrections 1 - beta^t in double precision before rounding to fp32 (1 - 0.999 -> 0.001f;
                                 1.0f - 0.999f would be 0.00099998713f).  0 = use the fp32 fields above. */
} psi_fit_config;
int psi_fit_create(psi_fit_engine **out, const psi_lbs_model *lbs, const psi_fit_config *cfg,
                   const float *h_w1, const float *h_b1, const float *h_w2, const float *h_b2,
                   const float *h_w3, const float *h_b3, const float *h_lh_comp, const float *h_rh_comp,
                   const float *h_pose_mean, const int32_t *h_contact_ids,
                   const float *d_scene_verts, const float *d_sdf, const float *h_gmin, const float *h_gmax);
void psi_fit_destroy(psi_fit_engine *engine);
/* Several scenes in one engine: body b of a run is fitted in scene slot[b].  Every scene-aware operator of this ABI takes a scene table
 * and a per-body scene index (psi_sdf_sample_forward, psi_nn_index_set_query, psi_lbs_sdf_counts); this is the fitting engine's form.
 * psi_fit_create_scenes is psi_fit_create with S scenes instead of one (cfg->m_scene and cfg->D are ignored; m and D may differ from
 * scene to scene).  Per scene the engine builds its own exact NN index (as psi_nn_index_create) and its own re-ordered copy of the
 * volume, which costs 8 x the volume per scene: 537 MB at 256^3, 3.8 GB for seven such rooms (PSI_ENOMEM when the allocation fails).
 * PSI_EINVAL: S < 1 or a null scene pointer; cfg->nn_mode != 1 (no brute-force search over several scenes); a D the re-ordered copy
 * cannot hold (D % 4 != 0, D > 480: this engine has no plain-volume fallback); cfg->world_size > 1 (data-parallel runs over several
 * scenes are not supported).  The scene slots are an engine-owned device buffer, all 0 after create; captured graphs stay valid when
 * they change.  psi_fit_set_scene_slots copies d_slot [B] (device int32; values outside [0,S) are clamped, the rule of
 * psi_lbs_sdf_counts) on `stream` — never inside a stream capture — and resets the nearest-neighbour warm-start hints, which index one
 * scene's cloud; the slots persist across psi_fit_set_problem.  On a psi_fit_create engine (one scene) the call only resets the hints. */
typedef struct psi_fit_scene {
    const float *d_verts;   /* DEVICE [m,3], caller-owned, must outlive the engine */
    const float *d_sdf;     /* DEVICE [D,D,D], element [ix][iy][iz], caller-owned  */
    int m, D;
    float gmin[3], gmax[3];
} psi_fit_scene;
int psi_fit_create_scenes(psi_fit_engine **out, const psi_lbs_model *lbs, const psi_fit_config *cfg,
                          const float *h_w1, const float *h_b1, const float *h_w2, const float *h_b2,
                          const float *h_w3, const float *h_b3, const float *h_lh_comp, const float *h_rh_comp,
                          const float *h_pose_mean, const int32_t *h_contact_ids,
                          const psi_fit_scene *h_scenes, int S);
int psi_fit_set_scene_slots(psi_fit_engine *engine, const int32_t *d_slot, void *stream);
int psi_fit_scene_count(const psi_fit_engine *engine);   /* 1 for psi_fit_create engines */
/* xhr = target body vectors [B,75]; x_init = starting parameters (NULL: start at xhr, fitting_proxe.py:175);
 * cam_ext [B,4,4]; reset_optimizer != 0 zeroes the Adam state and step count. */
int psi_fit_set_problem(psi_fit_engine *engine, const float *d_xhr, const float *d_x_init, const float *d_cam_ext,
                        int reset_optimizer, void *stream);
/* use_graph != 0: each half is captured once into its own hipGraph (stats pointer baked in) and replayed. */
int psi_fit_forward(psi_fit_engine *engine, float *d_stats, int use_graph, void *stream);
int psi_fit_backward_step(psi_fit_engine *engine, const float *d_stats, int use_graph, void *stream);
/* n_iter full iterations on one GPU; use_graph != 0 captures the iteration once (stream must not be the NULL stream)
 * and replays it with hipGraphLaunch — a 20-iteration graph for every full twenty, a 10-iteration graph for a remaining ten, a
 * single-iteration graph for the rest
 * (the iteration keeps no host-side state, so the result does not depend on how n_iter is split into calls). */
int psi_fit_iterate(psi_fit_engine *engine, int n_iter, int use_graph, void *stream);
/* Copies x [B,75] and the first n_hist rows of the loss-history RING [max_history,4] (row = (adam_step-1) % max_history) =
 * (l_rec, l_vposer, l_contact, l_collision as printed by fitting_proxe.py:184-186) to device buffers;
 * h_step (host, nullable) receives the Adam step count and forces a stream sync; with h_step the call also checks the engine's error
 * word and returns non-zero if one of the in-kernel cluster exchanges of the per-body kernels gave up waiting (results invalid). */
int psi_fit_read(psi_fit_engine *engine, float *d_x_out, float *d_history_out, int n_hist, int *h_step, void *stream);
/* The four loss values recorded by Adam step `adam_step` (1-based; the row (adam_step-1) % max_history of the ring) -> d_out4
 * (device, 4 floats): what the reference prints per iteration (fitting_proxe.py:184-186) without copying the whole ring.
 * The caller must not ask for a step more than max_history steps in the past (the ring has wrapped). */
int psi_fit_read_losses(psi_fit_engine *engine, int adam_step, float *d_out4, void *stream);
/* Differentiable body decode of the CVAE training losses: x75 [B,75] = [transl | 6D global rot | betas 10 | VPoser latent 32 |
 * hand PCA 12+12] -> camera-frame vertices [B,V,3].  One call replaces the reference's chain
 *   convert_to_3D_rot (cvae.py:117-139) -> body_params_encapsulate_batch (cvae.py:221-251) -> vposer.decode(..., 'aa')
 *   (vposer_smpl.py:156-167) -> body_mesh_model(...) (train_s1.py:143-150) -> verts_transform (cvae.py:141-149),
 * train_s1.py:136-157, with the engine's own head / LBS kernels (B = the engine's batch size).  The forward leaves its
 * activations in the engine; psi_fit_decode_backward must follow it (before the next forward) and returns dL/dx75.
 * The engine's fitting state (x, Adam moments) is overwritten: use a dedicated engine. */
int psi_fit_decode_forward(psi_fit_engine *engine, const float *d_x75, const float *d_cam_ext, float *d_verts, void *stream);
int psi_fit_decode_backward(psi_fit_engine *engine, const float *d_grad_verts, float *d_grad_x75, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Data-parallel fitting with the collective issued from C (RCCL over xGMI; one process per GPU).
 * The reference has no multi-GPU code (cluster_mpi/htcondor_submission.sub:15 submits independent processes); what is sharded
 * here is the batch of FittingOP.fitting (fitting_proxe.py:167-195): rank r owns its rows of xhr_rec and their Adam state, the
 * loss normalisers of fitting_proxe.py:105-110,139,155-158 run over the GLOBAL batch through one 6-float all-reduce per iteration.
 * A communicator is created once per process: rank 0 calls psi_dp_unique_id and hands the 128 bytes to every rank (any side channel:
 * torch.distributed's store, MPI, a file), then every rank calls psi_dp_comm_create with its rank — a collective call, made with the
 * rank's GPU current.  psi_fit_iterate_dp runs n_iter iterations of [forward kernels + the joint-side backward contraction, which leaves
 * the rank's LOCAL loss sums in stats; ncclAllReduce(stats[0..5]); the reduction that applies the global penetration count + the tail] on
 * `stream`; with use_graph != 0 as 10-iteration hipGraphs that CONTAIN the RCCL kernel (no host code between iterations).  The engine
 * must have been created with world_size == the communicator's size.  d_stats (device, >= 8 floats, nullable = engine-owned) is the
 * buffer the all-reduce runs in place on.
 * ------------------------------------------------------------------------------------------- */
#define PSI_DP_ID_BYTES 128
typedef struct psi_dp_comm psi_dp_comm;
int psi_dp_unique_id(char *h_id128);
int psi_dp_comm_create(psi_dp_comm **out, const char *h_id128, int rank, int world);
void psi_dp_comm_destroy(psi_dp_comm *comm);
int psi_dp_comm_info(const psi_dp_comm *comm, int *rank, int *world, int *rccl_version);
/* In-place sum over the ranks of d_buf[0..n) on `stream` (the collective psi_fit_iterate_dp issues; exported for tests and for the
 * training path's scalar reductions). */
int psi_dp_allreduce_sum(psi_dp_comm *comm, float *d_buf, int n, void *stream);
int psi_fit_iterate_dp(psi_fit_engine *engine, psi_dp_comm *comm, int n_iter, int use_graph, float *d_stats, void *stream);
/* How this engine's data-parallel iterations have been launched so far: 0 = none yet, 1 = captured hipGraphs (the collective inside),
 * 2 = eager launches from C (capturing the collective was refused once; results are the same). */
int psi_fit_dp_mode(const psi_fit_engine *engine);
/* Where this engine runs the kinematic chain of the pose stage (the G / A transforms): 1 = as a role of blend_fwd's launch, beside its
 * stream and off the iteration's critical path (cluster head kernels, B <= 64, a free compute unit for every links workgroup), 0 = in
 * the head kernel (also with PSI_FIT_CHAIN_IN_HEAD=1 in the environment at creation).  The results are the same bit for bit. */
int psi_fit_chain_mode(const psi_fit_engine *engine);
/* Host-side wait for everything enqueued on `stream` with a bound (hipStreamQuery polls): 0 = done, PSI_ETIMEOUT = still busy after
 * timeout_ms — the watchdog of the data-parallel loop (a collective that cannot complete becomes an error, not a hang). */
int psi_stream_wait(void *stream, int timeout_ms);

/* Per-kernel timing of one fitting iteration with HIP events on the launch stream (an event is recorded right after
 * every kernel launch of the sequence psi_fit_iterate runs; ungraphed), averaged over n_rep iterations.  Advances the
 * optimisation by n_rep steps.  h_names: [max_stages][name_stride] chars, h_ms: [max_stages] milliseconds. */
int psi_fit_profile(psi_fit_engine *engine, int n_rep, char *h_names, int name_stride, float *h_ms, int max_stages,
                    int *h_n_stages, void *stream);
/* Test/diagnostic copy of an engine-owned device buffer by name ("verts" [B,V,3], "pose" [B,165],
 * "g_pose", "g_rot" [B,55,9], "stats" [8], "adam_m"/"adam_v" [B,75]; the backward's intermediates "gA" [B,64,16], "gfeat" [B,Kpad],
 * "g_transl" [B,3], "gl" / "g_vp" / "v_posed" [B,Npad], the pose stage's "R" / "G" [B,55,12], "A" [B,55,12] + 16 zero rows of 12 and "feat"
 * [ceil(B/32) 32, Kpad] (fp16 pairs in blend_fwd's operand order), and — engines whose per-vertex backward runs inside the scene launch — the
 * contact class of rows "glc" / "gvpc" / "vpc" [B,3 ncp] in slot order (ncp = n_contact rounded up to 256), "spb" [B] (independent
 * bodies: each body's penetration factor -w_collision / N_b), and "penmask" [B][Vpad/64] 64-bit words = 2 floats' worth of bits
 * each, Vpad = V rounded up to 256: bit v % 64 of word v / 64 is set when vertex v of the body had sdf < 0 in the last forward, i.e. when
 * its rows of "gl" / "g_vp" may be non-zero; "gtc_part" [B, nfp, 4]: the translation gradient's contact part per 64-query slice, nfp =
 * ceil(n_contact / 64)) — and, on every engine, the contact term's slices "fpart" [B, nfp] and the search's warm-start hints "nn_hint"
 * (int32 bits; at least [B, n_contact], -1 = none) — into d_out (device).  n_floats above a buffer's size, or an unknown name: PSI_EINVAL. */
int psi_fit_copy_buffer(psi_fit_engine *engine, const char *name, float *d_out, long n_floats, void *stream);

/* The shape of the search role of the engine's shared scene launch: lanes per contact query (2 or 4), slices of 64 contact queries per
 * search workgroup (1 or 2) and the number of search workgroups of a launch, B * ceil(ceil(n_contact / 64) / slices).  All 0 on an engine
 * that runs the search as a launch of its own.  Two slices are chosen with 2 lanes unless PSI_FIT_SEARCH_SPW=1 was set when the engine was
 * created, or the scene's tree is so deep that the shape would lower the number of workgroups a compute unit holds. */
int psi_fit_search_shape(const psi_fit_engine *engine, int *lanes, int *slices, int *workgroups);

/* ---------------------------------------------------------------------------------------------
 * Dense layers of the CVAEs on the matrix cores — replaces nn.Linear (+ LeakyReLU, + skip connection) of
 *   ResBlock                 net_layers.py:28-43  (fc1 -> LeakyReLU -> fc2 -> LeakyReLU -> + x0)
 *   scene feature `fc`       cvae.py:436-440, net_layers.py:66,164  (8192 -> 256, 32768 -> 256)
 *   linear_in / mu_enc / logvar_enc / linear_latent / linear_out, torso_linear, pose_linear, mean/log_var_linear, decode.*
 *                            cvae.py:441-452,474-492; net_layers.py:67-86,165-184
 * y[M,N] = act(x[M,K] W[N,K]^T + bias[N]) (+ residual[M,N]);  W is the nn.Linear weight ([out,in], fp32 master copy).
 * Arithmetic: x and W are rounded to bf16 (RNE) as they are loaded, products accumulate in fp32 on v_mfma_f32_32x32x16_bf16,
 * y is fp32 — the precision of the reference trained under bf16 autocast with an fp32 output.  x: fp32 [M,K], or bf16 [M,K]
 * when x_is_bf16 != 0 (the NHWC bf16 conv feature map flattened).  K % 16 == 0 (forward) and N % 16 == 0 (backward).
 * act: 0 none, 1 LeakyReLU(slope).  act_out (nullable, [M,N]) receives act(...) BEFORE the residual is added: the backward
 * needs its sign.  ws: psi_linear_workspace_floats(M,N,K) floats (0 for small layers; split-K partials for large weights).
 * Backward: gy [M,N] = dL/dy; act_out as saved by the forward (NULL when act == 0); outputs gx [M,K] (dtype of x; nullable),
 * gW [N,K] fp32 and gbias [N] fp32 (nullable), all OVERWRITTEN.  The residual's gradient is gy itself (caller adds it).
 * ws of the backward: psi_linear_backward_workspace_floats(M,N,K) floats (0 for small layers; partial dX of the n-slices otherwise;
 * may be NULL when gx is NULL).  Partials of either direction are summed in slice order: deterministic.
 * ------------------------------------------------------------------------------------------- */
size_t psi_linear_workspace_floats(int M, int N, int K);
int psi_linear_forward(const void *x, int x_is_bf16, const float *W, const float *bias, const float *residual, int M, int N, int K,
                       int act, float slope, float *y, float *act_out, float *ws, void *stream);
/* psi_linear_forward3: the same layer at the fp32 model's precision (cvae.py:474-492 as shipped, no autocast) — three-term split products
 * (see psi_conv2d_forward) — and for ANY K and N (the 3-, 72-, 75-wide layers included; rows that are not 16-byte aligned are gathered
 * element by element).  Same arguments, same workspace. */
int psi_linear_forward3(const void *x, int x_is_bf16, const float *W, const float *bias, const float *residual, int M, int N, int K,
                        int act, float slope, float *y, float *act_out, float *ws, void *stream);
size_t psi_linear_backward_workspace_floats(int M, int N, int K);
/* psi_linear_backward3: the backward of psi_linear_forward3 — dX = G W and dW = G^T X (+ gbias) with three-term split operands, fp32 x, ANY N
 * and K; arguments and workspace as psi_linear_backward. */
int psi_linear_backward3(const float *gy, const float *act_out, const float *x, const float *W, int M, int N, int K, float slope, float *gx,
                         float *gW, float *gbias, float *ws, void *stream);
int psi_linear_backward(const float *gy, const float *act_out, const void *x, int x_is_bf16, const float *W, int M, int N, int K,
                        float slope, void *gx, float *gW, float *gbias, float *ws, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Batch normalisation of the scene trunk with its ReLU and skip connection fused in — replaces, inside the BasicBlocks and the stem of
 * the ResNet-18 prefix the reference builds (cvae.py:427-435; torchvision resnet18 children[1:6] = bn1, relu, maxpool, layer1, layer2),
 *   out = relu(bn1(conv1(x)))          out = relu(bn2(conv2(out)) + identity)          identity = downsample_bn(downsample_conv(x))
 * in TRAINING mode (train_s1.py / train_s2.py call model_h.train(): batch statistics, running statistics updated with `momentum`,
 * unbiased running variance, num_batches_tracked += 1 — nn.BatchNorm2d semantics).
 * x, residual (nullable), y: bf16 feature maps [M, C] with the channel fastest (M = N*H*W: an NHWC / torch channels_last tensor),
 * C % 8 == 0, C <= 256.  y = act(gamma * (x - mean) * invstd + beta (+ residual)), act = ReLU when relu != 0.  save_mean / save_invstd
 * [C] fp32 are kept for the backward.  running_mean / running_var / num_batches_tracked (int64) may be NULL.
 * The batch statistics are fp32 sums of x - x[0][c] and of its square, combined in double (mean = x[0][c] + S/M, var = Q/M - (S/M)^2): the
 * error of the variance is a few fp32 roundings of the variance itself (tests: 64 * 2^-24 * (var + eps)) whatever the ratio of a channel's
 * mean to its standard deviation, and a constant channel has variance 0 exactly.
 * Backward: dy [M,C] bf16 = dL/dy -> dx [M,C] bf16, dresidual [M,C] bf16 (nullable: the gradient of the skip input = dy masked by the
 * ReLU), dgamma / dbeta [C] fp32 (OVERWRITTEN).  y is the forward output (needed only when relu != 0, for the mask).
 * ws: psi_bn_workspace_floats(M, C) floats of device scratch per call (per-block partial sums; deterministic summation order).
 * ------------------------------------------------------------------------------------------- */
size_t psi_bn_workspace_floats(long M, int C);
int psi_bn_forward(const void *x, const void *residual, const float *gamma, const float *beta, float *running_mean,
                   float *running_var, long long *num_batches_tracked, long M, int C, int relu, float momentum, float eps,
                   void *y, float *save_mean, float *save_invstd, float *ws, void *stream);
int psi_bn_backward(const void *dy, const void *x, const void *y, const float *gamma, const float *save_mean,
                    const float *save_invstd, long M, int C, int relu, void *dx, void *dresidual, float *dgamma, float *dbeta,
                    float *ws, void *stream);

/* ---------------------------------------------------------------------------------------------
 * 3x3 convolution, stride 1, padding 1 (nn.Conv2d(C, C', 3, 1, 1)) of the scene trunk on the bf16 matrix cores — replaces the library
 * convolution for layer1 / layer2 of the ResNet-18 prefix (cvae.py:427-435) and the 128 -> 128 head convolution (net_layers.py:160-164),
 * forward and input gradient (the input gradient is the same convolution of dY with the weight rotated by 180 degrees and its channel
 * axes swapped: psi_conv3x3_rotate_weight).  x [N,H,W,Cin] bf16 (NHWC), w [Cout][3][3][Cin] bf16 (a channels_last Conv2d weight),
 * bias [Cout] fp32 or NULL, y [N,H,W,Cout] bf16; fp32 accumulation.  Covered shapes (psi_conv3x3_supported != 0):
 * Cin = 64 with Cout % 64 == 0, H % 8 == 0, W % 32 == 0;  Cin = 128 with Cout % 128 == 0, H % 8 == 0, W % 16 == 0.
 * ------------------------------------------------------------------------------------------- */
int psi_conv3x3_supported(int Cin, int Cout, int H, int W);
int psi_conv3x3_forward(const void *x, const void *w, const float *bias, int N, int H, int W, int Cin, int Cout, void *y, void *stream);
/* Weight gradient of the same convolution: gw [Cout][3][3][Cin] fp32 (OVERWRITTEN) = sum over all pixels of dY (x) X per filter tap; covered
 * when the image width is 16 or 32, H % (128 / W) == 0 and both channel counts are multiples of 64.  ws: psi_conv3x3_wrw_workspace_floats()
 * floats (per-split partial results, summed in a fixed order: deterministic, unlike the library's atomic split-K kernels). */
size_t psi_conv3x3_wrw_workspace_floats(int N, int H, int W, int Cin, int Cout);
int psi_conv3x3_weight_grad(const void *x, const void *dy, int N, int H, int W, int Cin, int Cout, float *gw, float *ws, void *stream);
/* w [Cout][3][3][Cin] -> wt [Cin][3][3][Cout] with wt[ci][kh][kw][co] = w[co][2-kh][2-kw][ci]:  dX = psi_conv3x3_forward(dY, wt) */
int psi_conv3x3_rotate_weight(const void *w, int Cin, int Cout, void *wt, void *stream);
/* fp32 master weight w32 [Cout][3][3][Cin] (the channels_last memory of an nn.Conv2d weight) -> bf16 in both layouts in one launch:
 * wb [Cout][3][3][Cin] (rounded to nearest even, what autocast's cast produces) and, when wt != NULL, wt = the rotated layout above. */
int psi_conv3x3_prepare_weight(const float *w32, int Cin, int Cout, void *wb, void *wt, void *stream);

/* MaxPool2d(kernel_size=3, stride=2, padding=1) of the trunk's stem (torchvision resnet18 children[3]; cvae.py:431-435) on an NHWC bf16 map
 * x [N,H,W,C] -> y [N,OH,OW,C], OH = (H - 1) / 2 + 1; idx [N,OH,OW,C] uint8 = position kh * 3 + kw of the maximum inside its window (first
 * maximum in scan order, like at::max_pool2d_with_indices).  Backward: dx [N,H,W,C] bf16 (OVERWRITTEN) gathers dy through idx. */
int psi_maxpool3x3s2_forward(const void *x, int N, int H, int W, int C, void *y, void *idx, void *stream);
int psi_maxpool3x3s2_backward(const void *dy, const void *idx, int N, int H, int W, int C, void *dx, void *stream);

/* ---- the scene encoders at the REFERENCE'S PRECISION (fp32 model: cvae.py:427-455; torchvision resnet18 children[1:6]; the head
 * convolutions cvae.py:436, net_layers.py:64,162) on hand-written kernels — replaces nn.Conv2d / nn.BatchNorm2d / nn.MaxPool2d of an fp32
 * HumanCVAES1 / S2 (F.conv2d -> MIOpen, at::batch_norm, at::max_pool2d) on the GPU.
 * psi_conv2d_forward: ANY 2-D convolution of that trunk (7x7 / stride 2 stem, stride-1 and stride-2 3x3, 1x1 / stride 2 downsample, 3x3 heads)
 *   as ONE implicit-GEMM kernel (csrc/conv_gemm.hip).  x [N,H,W,Cin] NHWC, fp32 or bf16 (x_bf16); w [Cout,KH,KW,Cin] FP32 (the memory of a
 *   channels_last Conv2d weight: the master weight is read directly, no prepared copy); bias [Cout] fp32 or NULL; y [N,OH,OW,Cout] NHWC fp32 or
 *   bf16 (y_bf16), OH = (H + 2 pad - KH) / stride + 1.  nterm = 3: every product is a three-term bf16 split (hi*hi + hi*lo + lo*hi) with
 *   fp32 accumulation — 0.6-3.2e-5 of the reference's recorded fp32 forward passes (tests/golden/cvae.npz; bound of the tests 2e-4);
 *   nterm = 1: operands rounded to bf16 (the bf16 mode of the trunk: the convolutions psi_conv3x3_forward does not cover).
 *   psi_conv2d_supported: Cout % 32 == 0 and (Cin % 16 == 0, or Cin * KH * KW <= 4096: element-gather paths; the 2 -> 64 channel 7x7 stride-2
 *   stem is routed to its own kernels, csrc/conv_stem.hip).
 * psi_bn_forward_t / psi_bn_backward_t / psi_maxpool3x3s2_forward_t / _backward_t: the operators above on maps of either element type
 *   (map_f32 != 0: fp32 NHWC maps), psi_bn_forward_t also in the INFERENCE form (eval_mode != 0: y = gamma (x - running_mean) /
 *   sqrt(running_var + eps) + beta, nothing updated, save_mean / save_invstd may be NULL) — the generation drivers run the encoders in
 *   .eval() (test_habitat_s2.py:155-170).  idx == NULL in psi_maxpool3x3s2_forward_t: no window positions are kept (inference). */
int psi_conv2d_supported(int Cin, int Cout, int KH, int KW, int stride, int pad);
int psi_conv2d_forward(const void *x, int x_bf16, const float *w, const float *bias, int N, int H, int W, int Cin, int Cout, int KH, int KW,
                       int stride, int pad, void *y, int y_bf16, int nterm, void *stream);
/* psi_conv2d_input_grad: dX of the same convolution — dy [N,OH,OW,Cout] -> dx [N,H,W,Cin] (OVERWRITTEN); wt = the weight re-laid out as
 *   [Cin][KH][KW][Cout] fp32 (torch: weight.permute(1,2,3,0).contiguous()); the forward kernel in its transposed-gather form, any stride
 *   (Cin % 32 == 0; Cout % 64 == 0 or Cout * KH * KW <= 4096).  psi_conv2d_weight_grad: gw [Cout,KH,KW,Cin] fp32 (OVERWRITTEN) = sum over pixels of dy x im2col(x); the
 *   pixel range is split over workgroups, partial tiles summed in slice order (deterministic); ws: psi_conv2d_wgrad_workspace_floats floats.
 *   Both replace aten::convolution_backward (MIOpen igemm_bwd / igemm_wrw) for the trunk's convolutions; nterm as in the forward. */
int psi_conv2d_input_grad(const void *dy, int dy_bf16, const float *wt, int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                          void *dx, int dx_bf16, int nterm, void *stream);
/* Prepared weights: psi_conv2d_prepare_weight rounds / splits the fp32 master weight ONCE per layer and step into bf16 parts (hi parts, for
 *   nterm = 3 followed by the lo parts; Cout*KH*KW*Cin elements each) in the forward layout `wf` [Cout][KH][KW][Cin] and / or the input
 *   gradient's layout `wt` [Cin][KH][KW][Cout] (either may be NULL) — instead of a re-layout copy for the backward and a re-split of every
 *   64 x 64 weight tile in every workgroup of both kernels.  psi_conv2d_forward_p / psi_conv2d_input_grad_p take those buffers in place of
 *   the fp32 weight (same results, bit for bit); psi_conv2d_prepared_ok: the layers they cover (Cin % 16 == 0: all but the stem). */
int psi_conv2d_prepared_ok(int Cin, int Cout, int KH, int KW, int stride, int pad);
int psi_conv2d_prepare_weight(const float *w, int Cout, int KH, int KW, int Cin, int nterm, void *wf, void *wt, void *stream);
int psi_conv2d_forward_p(const void *x, int x_bf16, const void *wf, const float *bias, int N, int H, int W, int Cin, int Cout, int KH, int KW,
                         int stride, int pad, void *y, int y_bf16, int nterm, void *stream);
int psi_conv2d_input_grad_p(const void *dy, int dy_bf16, const void *wt, int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                            void *dx, int dx_bf16, int nterm, void *stream);
size_t psi_conv2d_wgrad_workspace_floats(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad);
int psi_conv2d_weight_grad(const void *x, int x_bf16, const void *dy, int dy_bf16, int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                           int pad, float *gw, float *ws, int nterm, void *stream);
/* psi_adam_step: ONE Adam step over all `count` fp32 parameter tensors of a model (train_s1.py:229 / train_s2.py:295-296:
 *   optim.Adam(model_h.parameters(), lr) stepped once per batch) — replaces torch.optim.Adam's multi-tensor launches (_foreach_add on the
 *   step counters + 4 x multi_tensor_apply for HumanCVAES2's 122 tensors) by one or two hand-written launches (80 tensors each; addresses in
 *   the kernel arguments, so a hipGraph captures them by value).  p / g / m / v: HOST arrays of `count` device pointers (parameter,
 *   gradient, exp_avg, exp_avg_sq), n: element counts; step: device fp32 scalar = steps taken so far, shared by all tensors, incremented
 *   by the last workgroup to finish; ticket: device uint32, zero before the first call.  Arithmetic: the operation order of PyTorch's fused
 *   Adam (moments in double, rounded to fp32 once); weight_decay is the L2 form (grad += wd * p), no amsgrad / maximize. */
int psi_adam_step(void *const *p, const void *const *g, void *const *m, void *const *v, const long *n, int count, float *step, unsigned *ticket,
                  double lr, double beta1, double beta2, double eps, double weight_decay, void *stream);
int psi_bn_forward_t(const void *x, int map_f32, const void *residual, const float *gamma, const float *beta, float *running_mean,
                     float *running_var, long long *num_batches_tracked, long M, int C, int relu, float momentum, float eps, void *y,
                     float *save_mean, float *save_invstd, float *ws, int eval_mode, void *stream);
/* psi_bn_backward_t: y may be NULL for a ReLU layer WITHOUT a skip connection when beta is given — the mask "y > 0" is then recomputed from x
 *   (y = relu(fma(x, gamma * invstd, beta - mean * gamma * invstd)), rounded as the forward stored it): both backward passes read one map less. */
int psi_bn_backward_t(const void *dy, int map_f32, const void *x, const void *y, const float *gamma, const float *beta, const float *save_mean,
                      const float *save_invstd, long M, int C, int relu, void *dx, void *dresidual, float *dgamma, float *dbeta, float *ws,
                      void *stream);
int psi_maxpool3x3s2_forward_t(const void *x, int map_f32, int N, int H, int W, int C, void *y, void *idx, void *stream);
int psi_maxpool3x3s2_backward_t(const void *dy, int map_f32, const void *idx, int N, int H, int W, int C, void *dx, void *stream);

/* ---- body-vector glue of a CVAE training step (train_s1.py:95-133 / train_s2.py:102-139 cal_loss) ------------------------------
 * psi_cvae_target: out75[b] = convert_to_6D_rot(normalize_global_T(xh72[b], cam_int[b], max_d[b]))   (cvae.py:176-199 + 118-127, the
 *   torchgeometry 0.1.2 angle_axis_to_rotation_matrix with its first-order branch at theta^2 <= 1e-6): [B,72] -> [B,75].
 * psi_cvae_losses_forward: xh_rec75 = recover_global_T(rec75, cam_int, max_d) (cvae.py:153-172; only the translation changes) and
 *   losses5 = { w_rec (0.5 L1(rec[:, :3], target[:, :3]) + 0.5 L1(xh_rec[:, :3], xh[:, :3])),  w_rec L1(rec[:, 3:], target[:, 3:]),
 *               KL of latent 0, KL of latent 1 (fca^2 w_kl 0.5 mean(exp(logvar) + mu^2 - 1 - logvar); 0 when mu == NULL),
 *               w_vposer mean(xh_rec[:, 19:51]^2) }                                            (train_s2.py:122-139)
 *   fca: the KL annealing factor, read from fca_dev (a device float, so that a captured step can change it) when that is not NULL.
 * psi_cvae_losses_backward: gradients of  sum_k g_losses5[k] * losses5[k]  +  <g_xh_rec75, xh_rec75>  (g_xh_rec75 may be NULL) with
 *   respect to rec75, mu, logvar (all OVERWRITTEN).  All tensors fp32, contiguous, device memory. */
size_t psi_cvae_losses_workspace_floats(void);      /* ws of psi_cvae_losses_forward */
int psi_cvae_target(const float *xh72, const float *cam_int, const float *max_d, int B, float *out75, void *stream);
int psi_cvae_losses_forward(const float *rec75, const float *target75, const float *xh72, const float *cam_int, const float *max_d,
                            const float *mu0, const float *logvar0, int nz0, const float *mu1, const float *logvar1, int nz1, int B,
                            float w_rec, float w_kl, float w_vposer, float fca, const float *fca_dev, float *ws, float *xh_rec75,
                            float *losses5, void *stream);
int psi_cvae_losses_backward(const float *rec75, const float *target75, const float *xh72, const float *cam_int, const float *max_d,
                             const float *mu0, const float *logvar0, int nz0, const float *mu1, const float *logvar1, int nz1, int B,
                             float w_rec, float w_kl, float w_vposer, float fca, const float *fca_dev, const float *xh_rec75,
                             const float *g_losses5, const float *g_xh_rec75, float *g_rec75, float *g_mu0, float *g_logvar0,
                             float *g_mu1, float *g_logvar1, void *stream);

/* ---- tail of the two scene losses of a training step (train_s1.py:156-204 / train_s2.py:159-202) ----------------------------------
 * forward : losses2[0] = gate w_contact mean(s / (s + 1)), s = sqrt(dist + 1e-4) over the n_contact = B * n_c body->scene distances;
 *           losses2[1] = gate w_collision * (mean |sdf| over the negative ones of the n_sdf = B * V values, 0 if there is none);
 *           stats2 = { sum |sdf| over sdf < 0, their count } (input of the backward).  ws: psi_scene_losses_workspace_floats() floats.
 * backward: g_verts [B,V,3] (OVERWRITTEN) = d(g_losses2[0] losses2[0] + g_losses2[1] losses2[1]) / d body vertices, given xyz1 [B,n_c,3] =
 *           the contact vertices that were queried (rows vid [n_c] of the body), their nearest scene points verts_table[slot[b]][idx[b,j]]
 *           (verts_table [S,m,3], chamfer.cu:155-174) and sdf_grad [B,V,3] = d sdf / d vertex (psi_sdf_sample_forward's out_grad).
 *           chain: psi_contact_slot_chain(vid) — the slots of a vertex that is listed more than once (cvae.py:99-115 keeps duplicates) are
 *           chained in slot order and added by one thread: no atomics, run-to-run bit-identical. */
size_t psi_scene_losses_workspace_floats(void);
int psi_scene_losses_forward(const float *dist, long n_contact, const float *sdf_vals, long n_sdf, float w_contact, float w_collision,
                             float gate, float *ws, float *losses2, float *stats2, void *stream);
int psi_scene_losses_backward(const float *g_losses2, const float *stats2, const float *dist, const float *xyz1, const int32_t *idx,
                              const int32_t *slot, const float *verts_table, long m, const int32_t *vid, const float *sdf_vals,
                              const float *sdf_grad, int B, int V, int n_c, float w_contact, float w_collision, float gate,
                              const int32_t *chain, float *g_verts, void *stream);
/* chain [2 * n_c] of a contact-id list vid [n_c] (device): chain[j] = the next slot > j that lists the same vertex as slot j (-1: none),
 * chain[n_c + j] = 1 when no earlier slot lists it.  A constant of the list: build it once, pass it to every backward. */
int psi_contact_slot_chain(const int32_t *vid, int n_c, int32_t *chain, void *stream);

/* ---- evaluation: physical plausibility (utils/utils_eval_collision_habitat.py:91-175) ---------------------------------------------
 * counts[b] = { #(sdf < 0), #(sdf > 0) } over the V vertices of body b, sampled in sdf[scene_id[b]] — the two integers
 * utils_eval_collision_habitat.py:126-139 derives per body from smplx(...).vertices and F.grid_sample.  Inputs as psi_lbs_forward (betas, pose,
 * transl, cam_ext, ws of psi_lbs_workspace_floats(model, B)) and as psi_sdf_sample_forward (sdf [S,D,D,D], scene_id [B] or NULL, gmin / gmax
 * [S,3], align_corners; a scene_id outside [0,S) is clamped).  counts: device int32 [B,2], OVERWRITTEN.  No vertex, SDF value or gradient is
 * written to memory: the sign test is the epilogue of the skinning kernel.  A vertex goes through the arithmetic of psi_lbs_forward and
 * psi_sdf_sample_forward; the counters are integers, so the result is run-to-run identical. */
int psi_lbs_sdf_counts(const psi_lbs_model *model, const float *betas, const float *pose, const float *transl,
                       const float *cam_ext, int B, const float *sdf, const int32_t *scene_id, const float *gmin,
                       const float *gmax, int D, int S, int align_corners, int32_t *counts, float *ws, void *stream);

/* ---- evaluation: diversity (utils/utils_eval_diversity.py:93-104) -------------------------------------------------------------------
 * scipy.cluster.vq.kmeans(obs, k) in its own protocol, all R restarts in one launch per stage: per restart
 *   prev = +inf; repeat { code, dist = vq(obs, book) (first minimum wins); avg = mean(dist) (EUCLIDEAN, not squared); book = centroids of the
 *   members, codes without members REMOVED, order of the others kept; diff = |prev - avg|; prev = avg } until not (diff > thresh)
 * result: the book after the last update and the avg of the last vq.  Squared distances sum_f (x_f - c_f)^2 in fp32, features in index
 * order; centroid sums, counts and avg in fp64 / integers, combined in a fixed order: bit-identical from run to run and independent of how
 * the iterations are split into calls.
 * obs [N,d] fp32 (device, borrowed: must outlive the object); guess [R,k,d] fp32 (device, copied): R initial codebooks.
 * d <= 128, k <= 64, R <= 64, N >= k; otherwise PSI_EINVAL. */
typedef struct psi_kmeans psi_kmeans;
int psi_kmeans_create(psi_kmeans **out, const float *obs, int N, int d, const float *guess, int k, int R, float thresh);
void psi_kmeans_destroy(psi_kmeans *km);
/* Enqueue n_iter Lloyd iterations of every restart that has not converged; converged restarts are left untouched.  No host sync. */
int psi_kmeans_iterate(psi_kmeans *km, int n_iter, void *stream);
/* book [R,k,d] (first k_eff[r] rows of restart r valid), k_eff [R] int32, avg_dist [R] fp64, iters [R] int32: device outputs, each
 * nullable.  h_converged (host, nullable): number of converged restarts; passing it synchronises the stream (like psi_fit_read). */
int psi_kmeans_read(psi_kmeans *km, float *book, int32_t *k_eff, double *avg_dist, int32_t *iters, int *h_converged, void *stream);
/* scipy.cluster.vq.vq: code[i] = lowest index of the nearest row of book [k,d], dist[i] = its Euclidean distance (nullable). */
int psi_vq(const float *obs, int N, int d, const float *book, int k, int32_t *code, float *dist, void *stream);

/* ---- scene snapshots: depth / triangle id / label images of a triangle mesh (utils/utils_prox_snapshots_virtualcam.py:342-378, 502-541) ----
 * A tile-binned rasteriser with exact integer coverage; every view of a call is rendered by the same launches.  Arithmetic (fp32, not
 * contracted; DESIGN.md "Snapshot rasteriser" has the full statement):
 *   camera space  xc = ((m00*X + m01*Y) + m02*Z) + m03 (yc, zc alike) with the view's world-to-camera rows m; the camera looks along +z,
 *                 x right, y down
 *   near clip     a vertex is inside when zc >= near_z; a triangle crossing the plane becomes one or two pieces; a new vertex is computed
 *                 from the inside vertex a towards the outside vertex b: t = (near_z - za)/(zb - za), p = a + t*(b - a)
 *   projection    u = (fx*xc)/zc + cx, U = (int)rintf(u*256) (IEEE division, round half to even), v / V alike; a piece with |U| or |V| above
 *                 2^28 is not drawn and is counted; pieces of integer area 0 are dropped; both windings are drawn
 *   coverage      sample (256*px + 128, 256*py + 128), int64 edge functions, top-left rule
 *   depth         li = (float)ei/(float)area, 1/z = (l0/z0 + l1/z1) + l2/z2; the pixel keeps the minimum of (bits of z) << 32 | triangle
 *                 index, so the images do not depend on the order of the work and equal depths go to the lower index
 * No floating-point atomics: the three images are bit-identical from run to run, for any batching of the views.
 *
 * psi_raster_mesh_create copies verts [nv,3] fp32, faces [nf,3] int32 and vlabel [nv] fp32 (NULL: all labels 0) from device memory and
 * checks every face index (PSI_EINVAL outside [0, nv)); it synchronises the device, like psi_kmeans_create. */
typedef struct psi_raster_mesh psi_raster_mesh;
int psi_raster_mesh_create(psi_raster_mesh **out, const float *d_verts, const int32_t *d_faces, const float *d_vlabel, int nv, int nf);
void psi_raster_mesh_destroy(psi_raster_mesh *mesh);
/* Host function: bytes of the workspace of one psi_raster_render call (piece records, tile counts, bins). */
size_t psi_raster_workspace_bytes(int nf, int n_views, int W, int H);
/* d_w2c [n_views,3,4] fp32 world-to-camera rows; d_intr [n_views,4] fp32 = fx, fy, cx, cy; W, H <= 4096; near_z > 0.
 * Outputs (device, overwritten): d_depth [n_views,H,W] fp32, z of the winner or 0.0f where nothing was hit; d_tri [n_views,H,W] int32, the
 * triangle index or -1; d_seg [n_views,H,W] fp32 or NULL, z * ((l0*lab0/z0 + l1*lab1/z1) + l2*lab2/z2), the perspective-correct vertex
 * label, or 0; d_stats [n_views,2] int32 = { (tile, piece) pairs binned, pieces not drawn because of the 2^28 guard }.
 * d_workspace: psi_raster_workspace_bytes(nf, n_views, W, H) bytes, or NULL for the library's per-stream scratch.  The bins are sized from
 * the counts, which the host reads: the call synchronises the stream once, after the binning counts (it cannot be captured into a graph);
 * a call whose pairs exceed the workspace's bin space takes the bins from a buffer that the mesh object owns and grows.  Because of that
 * buffer a mesh object is rendered by ONE call at a time: calls on the same mesh from several threads or streams must be serialised by the
 * caller (different mesh objects are independent).  A view with 2^31 or more pairs is refused (PSI_EINVAL). */
int psi_raster_render(psi_raster_mesh *mesh, const float *d_w2c, const float *d_intr, int n_views, int W, int H, float near_z,
                      float *d_depth, int32_t *d_tri, float *d_seg, int32_t *d_stats, void *d_workspace, void *stream);

/* ---- result images: bodies drawn into the snapshots of their scene (utils/utils_show_test_results.py, img_%06d_cam1.png / _cam2.png) ----
 * The bodies are B meshes [B,V,3] of one topology (faces [F,3]) made on the device.  A draw is a (body, view) pair with its own colour;
 * any number of draws may share a view, a body may appear in several views, a view may have none.  Body triangles go through the
 * statements of the snapshot rasteriser above, word for word; the index of a piece is d * F + face.  The rest of the contract (fp32, not
 * contracted, IEEE division and square root; DESIGN.md "Result images"):
 *   normal    of a vertex: the unnormalised world-frame (v1 - v0) x (v2 - v0) of its faces (each component two products and one
 *             subtraction), summed left to right in ascending face index; (0,0,0) for a vertex of no face
 *   owner     the body owns a pixel iff a body piece covers it and the scene has no hit there or z_body < z_scene; equal depths go to the scene
 *   shade     s = 0.3 + (0.7*|N_z|)/sqrtf((N_x*N_x + N_y*N_y) + N_z*N_z), s = 0.3 when the length is 0 or not finite
 *   body      N = (l0*(n0*iz0) + l1*(n1*iz1)) + l2*(n2*iz2) per component, n the camera-space vertex normal ((m00*nx + m01*ny) + m02*nz, ...),
 *             interpolated like the label, near clip included; colour = draw_rgb[d] * s
 *   scene     N = the flat normal (v1 - v0) x (v2 - v0) of the parent triangle's camera-space vertices; base colour = the label formula per
 *             channel of the vertex colours, 0.8 without them; colour = base * s
 *   channel   (unsigned char)rintf(255.f * fminf(fmaxf(c, 0.f), 1.f)); background pixels carry the caller's colour
 * No floating-point atomics: every output is bit-identical from run to run, for any batching of the views and any draws_per_pass.
 *
 * psi_raster_bodies_create reads faces [F,3] int32 from device memory, checks every index (PSI_EINVAL outside [0, V)) and builds the
 * per-vertex face lists on the host; it synchronises the device. */
typedef struct psi_raster_bodies psi_raster_bodies;
int psi_raster_bodies_create(psi_raster_bodies **out, const int32_t *d_faces, int V, int F);
void psi_raster_bodies_destroy(psi_raster_bodies *bodies);
/* d_bverts [B,V,3] fp32 -> d_normals [B,V,3] fp32, one lane per (body, vertex); one kernel on `stream`, no host sync. */
int psi_raster_bodies_normals(psi_raster_bodies *bodies, const float *d_bverts, int B, float *d_normals, void *stream);
/* Host function: bytes of the workspace of one psi_raster_bodies_render call whose passes hold at most draws_per_pass draws (their piece
 * records, 2 * draws_per_pass * F * 52 bytes), plus the tile counts, the bins and the 64-bit body key image.  0 for arguments the render
 * call refuses, draws_per_pass * F >= 2^30 among them. */
size_t psi_raster_bodies_workspace_bytes(int F, int draws_per_pass, int n_views, int W, int H);
/* scene, d_sdepth, d_stri: the scene's mesh object and the depth / tri images [n_views,H,W] of a psi_raster_render of the same views and
 * near_z; all NULL for no scene.  d_vrgb [nv,3] fp32 vertex colours in [0,1] or NULL.  d_bverts [B,V,3]; d_draw_body, d_draw_view [M] int32,
 * d_draw_rgb [M,3] fp32; M * F < 2^31; M = 0 composes the scene alone.  Views as psi_raster_render.  A draw whose body lies outside [0, B)
 * or whose view lies outside [0, n_views) is found on the device and refused (PSI_EINVAL) before anything is drawn.
 * Outputs (device, overwritten): d_rgb [n_views,H,W,3] uint8; d_depth the owner's z or 0; d_draw the draw index where a body owns the pixel,
 * else -1; d_bdepth / d_bid the nearest body piece alone, z and d * F + face, or 0 / -1; d_counts [M,2] int32 = { pixels whose nearest body
 * piece belongs to draw d, those of them that also beat the scene }; d_stats [n_views,2] as psi_raster_render, over the bodies' pieces.
 * d_workspace: psi_raster_bodies_workspace_bytes(F, draws_per_pass, n_views, W, H) bytes, or NULL for the library's per-stream scratch.
 * The call loops over the passes itself and synchronises the stream once per pass, after the binning counts; bins beyond the workspace's
 * come from a buffer the bodies object owns, so a bodies object is rendered by ONE call at a time, like a mesh object. */
int psi_raster_bodies_render(psi_raster_mesh *scene, const float *d_vrgb, psi_raster_bodies *bodies, const float *d_bverts, int B,
                             const int32_t *d_draw_body, const int32_t *d_draw_view, const float *d_draw_rgb, int M, const float *d_w2c,
                             const float *d_intr, int n_views, int W, int H, float near_z, const float *d_sdepth, const int32_t *d_stri,
                             float bg_r, float bg_g, float bg_b, int draws_per_pass, uint8_t *d_rgb, float *d_depth, int32_t *d_draw,
                             float *d_bdepth, int32_t *d_bid, int32_t *d_counts, int32_t *d_stats, void *d_workspace, void *stream);

/* ---- mesh -> signed distance volume: the {scene}_sdf.npy of a scene from its triangle mesh (the reference ships the volumes as downloads) ----
 * Contract (fp32, not contracted; DESIGN.md "Mesh -> SDF volume" has the full statement):
 *   node       (ix, iy, iz) lies at gmin[a] + (float)i_a * ((gmax[a] - gmin[a]) / (float)(D - 1)): the sampler's align_corners = True positions
 *   magnitude  sqrtf of the minimum over the kept triangles of d2 = |p - c|^2, c the closest point of the triangle from one fixed
 *              seven-region routine on the record (a, b - a, c - a); the minimum is taken over bits(d2) << 32 | triangle index, so it does
 *              not depend on the visiting order and equal d2 goes to the lower index
 *   sign       that of (p - c) . n, n the angle-weighted pseudonormal of the face, edge or vertex of the winning triangle that c lies on;
 *              exactly 0 counts as positive.  Triangles face free space: free space is positive, solid negative
 *   topology   vertices with bit-identical positions are welded (-0.0 equals +0.0); triangles with two equal welded vertices or an fp64
 *              cross product of exactly 0 are dropped; pseudonormals in fp64 on the host, stored as fp32; an edge with one triangle uses
 *              that triangle's normal
 * No floating-point atomics: the volume is bit-identical from run to run, and mode 0 and mode 1 give the same bits.
 *
 * psi_mesh_sdf_create reads verts [nv,3] fp32 and faces [nf,3] int32 from device memory, does the topology on the host and uploads the scan
 * records, the normals and the cell grid; it synchronises the device and launches no kernel.  PSI_EINVAL: a face index outside [0, nv), a
 * non-finite vertex coordinate, no triangle left. */
typedef struct psi_mesh_sdf psi_mesh_sdf;
int psi_mesh_sdf_create(psi_mesh_sdf **out, const float *d_verts, const int32_t *d_faces, int nv, int nf);
void psi_mesh_sdf_destroy(psi_mesh_sdf *m);
/* info[0] kept triangles, [1] dropped degenerate triangles, [2] welded vertices (distinct positions among the nv), [3] edges not shared by
 * exactly two triangles */
int psi_mesh_sdf_info(const psi_mesh_sdf *m, int32_t info[4]);
/* gmin, gmax: host pointers.  d_out: device [D,D,D] fp32, element [ix][iy][iz].  mode 0 = pruned search, 1 = every node against every
 * triangle.  PSI_EINVAL when D < 2 or D > 1024, when gmax[a] <= gmin[a], when a bound is not finite.  One kernel on `stream`, no host sync. */
int psi_mesh_sdf_compute(psi_mesh_sdf *m, const float gmin[3], const float gmax[3], int D, int mode, float *d_out, void *stream);
/* The same search in a build of the kernel that also counts the (node, triangle) tests it executes: *d_pairs (device, 64-bit) receives the
 * count.  For measurements (tools/time_mesh_sdf.py); psi_mesh_sdf_compute carries no counter. */
int psi_mesh_sdf_count_pairs(psi_mesh_sdf *m, const float gmin[3], const float gmax[3], int D, int mode, unsigned long long *d_pairs,
                             void *stream);

/* ---- generalised winding number of the same mesh: the sign of the volume for open, touching and interpenetrating meshes ----
 * Contract (DESIGN.md "Winding-number sign"): with a = A - p, b = B - p, c = C - p of a kept triangle,
 *   Omega = 2 atan2(a . (b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|), atan2(0, 0) = 0, and f(p) = -(1 / 4 pi) sum Omega:
 * 1 in the free space of a closed room whose triangles face free space, 0 inside furniture and outside the room.  A node is solid iff
 * f < level (0.5 for a room, -0.5 for objects standing in open space).  The sum is fp32 within a chunk of 256 records and fp64 across
 * chunks, in a fixed order (kept order when beta = 0; cluster order, then the order within the cluster, otherwise): bit-identical from run
 * to run, no floating-point atomics; unlike the distance it may change in the last bits under a permutation of the faces.
 * beta > 0: the kept triangles, sorted by the Morton code of their centroids, are cut into clusters of `cluster` triangles; a cluster whose
 * area-weighted centroid c lies farther than beta * r (r = its largest vertex distance from c) from the box of an 8 x 8 x 8 brick of nodes
 * contributes -N . (c - p) / (4 pi |c - p|^3) to the f of that brick's nodes (N = the sum of its area vectors), a nearer one its
 * triangles.  The records of beta = 0 and the clusters of each `cluster` value are built on the host and uploaded at first use (that call
 * synchronises the device) and cached on the handle; every later call is one kernel on `stream` with no host synchronisation.
 * d_f: device [D,D,D] fp32, element [ix][iy][iz], the node positions of psi_mesh_sdf_compute.  PSI_EINVAL: the cases of
 * psi_mesh_sdf_compute, beta < 0 or not finite, cluster outside 8 .. 256. */
int psi_mesh_winding_compute(psi_mesh_sdf *m, const float gmin[3], const float gmax[3], int D, float beta, int cluster, float *d_f, void *stream);
/* The counting build of the same kernel: d_counts[0] receives the (node, triangle) tests, d_counts[1] the (node, dipole) tests, over
 * the D^3 nodes. */
int psi_mesh_winding_count(psi_mesh_sdf *m, const float gmin[3], const float gmax[3], int D, float beta, int cluster,
                           unsigned long long *d_counts /*[2]*/, void *stream);
/* d_vol[i] = d_f[i] < level ? -|d_vol[i]| : |d_vol[i]| for i < n: one elementwise kernel on `stream`. */
int psi_mesh_sdf_apply_sign(const float *d_f, float level, float *d_vol, long long n, void *stream);

/* ---- training records: the CVAE's input images of n rendered views, both modalities, in one call ----
 * Replaces, per view, two calls of data_preprocessing (utils/utils_prox_snapshots_virtualcam.py:266-330, batch_gen_hdf5.py:398-439) and the
 * window test of is_body_occluded (:342-378).  Contract, fp32, not contracted:
 *   clip, maximum  c = min(x, clip); the view's maximum of c is exact (integer atomicMax on the bits of non-negative floats; NaN pixels are
 *                  left out of it and flag the view)
 *   scale          v = (2 c) / max - 1
 *   resize         F.interpolate(mode='bilinear', align_corners=False): scale = float(in) / out, src = max(fma(scale, dst + 0.5, -0.5), 0),
 *                  i0 = int(src), i1 = min(i0 + 1, in - 1), l1 = src - i0, l0 = 1 - l1, out = l0y (l0x a + l1x b) + l1y (l0x c + l1x d)
 *   placement      H >= W: the image becomes th x (int(W (th / H)) / 2 * 2), centred in the columns; H < W the symmetric case; 0 elsewhere
 *   window         usable = sum / count > z, the sum of the UNCLIPPED depth over [x0,x1) x [y0,y1) (cut to the image) in fp64, row-major,
 *                  one adder; an empty window is not usable; without windows usable = 1
 *   degenerate     a view whose depth or seg maximum is not > 0, or that holds a NaN: usable = 0 and both canvases all 0
 * d_depth, d_seg [n,H,W] fp32, values >= 0 (a negative value counts as 0 in the maximum); they are only read.  d_windows [n,4] int32 =
 * x0, y0, x1, y1 and d_target_z [n] fp32 come together or are both NULL.  Outputs: canvases [n,1,th,tw] fp32, d_max_d / d_seg_max [n] fp32
 * (the clipped maxima), d_usable [n] int32.  Every output of a view is bit-identical whatever other views the call holds, and from run to
 * run: no floating-point atomics.  d_workspace: psi_snapshot_canvas_workspace_bytes(n) bytes (the call zeroes it), or NULL for the
 * library's per-stream scratch.  One memset and two kernels on `stream`, no host synchronisation.
 * PSI_EINVAL: n, H or W < 1, H * W >= 2^31, th or tw odd or < 2, a clip <= 0, a resized image that is empty or wider than the canvas. */
size_t psi_snapshot_canvas_workspace_bytes(int n_views);
int psi_snapshot_canvas(const float *d_depth, const float *d_seg, int n_views, int H, int W, int th, int tw, float clip_depth, float clip_seg,
                        const int32_t *d_windows, const float *d_target_z, float *d_depth_canvas, float *d_seg_canvas, float *d_max_d,
                        float *d_seg_max, int32_t *d_usable, void *d_workspace, void *stream);

/* ---- scene contact cloud: even surface samples of a mesh, about one per `spacing` cell whatever the tessellation ----
 * Contract (csrc/mesh_cloud_shared.h holds the statements), fp32, not contracted, IEEE division and square root.
 * With h = spacing / 2, for every triangle of d_faces in the caller's numbering:
 *   candidates  none for a triangle whose |ab x ac| is 0; the three corners for one whose longest edge is shorter than h; otherwise the
 *               corners are rotated so that ab is the longest edge (a tie takes the first of ab, bc, ca), L = |ab|, Ht = |ab x ac| / L,
 *               m = max(1, ceil(Ht / h)); row r < m lies at s = r / m between P = a + s (c - a) and Q = b + s (c - b) and holds
 *               P + (j / k)(Q - P), j = 0 .. k, with k = max(1, ceil(((1 - s) L) / h)); row m is the point c.  Candidates are numbered
 *               triangle by triangle, row by row, j ascending
 *   selection   o = (minimum over the vertices the faces refer to) - h per axis, cell = floor((p - o) / spacing), centre =
 *               o + (cell + 0.5) spacing; of the candidates of a cell the one with the smallest squared distance to the centre is kept,
 *               on a tie the smallest candidate number; the output is the kept candidates in ascending candidate number
 * Every surface point lies within 2.3 spacing of an output point and no cell holds two.  No floating-point atomics: bit-identical from run
 * to run.  The five calls are the passes of one computation; the scans and the sort between them are the caller's (ops.mesh_cloud):
 *   count    d_verts [nv,3] fp32, d_faces [nf,3] int32 (device).  Writes d_tri_rows [nf] int32 (rows per triangle), then reads the verdict
 *            back (it synchronises `stream`) and fills the host values origin[3], *n_rows and *n_cands.  PSI_EINVAL, with nothing but
 *            d_tri_rows written: spacing not finite or <= 0; nf < 1; a face index outside [0, nv); a non-finite coordinate of a
 *            referenced vertex; no triangle with area; more than 2^21 cells along an axis; more than 2^31 - 1 candidates (*n_cands then
 *            holds the count)
 *   rows     d_tri_row_off [nf] int64 = exclusive scan of d_tri_rows.  Writes d_row_tri, d_row_cnt [n_rows] int32: the triangle and the
 *            candidate count of every row
 *   emit     d_row_off [n_rows] int64 = exclusive scan of d_row_cnt.  Writes d_pos [n_cands,3] fp32, d_tri [n_cands] int32, d_cell
 *            [n_cands] int64 (the linear cell index, 21 bits per axis) and d_key [n_cands] uint32 (the bits of the squared distance)
 *   winners  d_cell_sorted, d_perm [n] int64 = a STABLE ascending sort of d_cell and its permutation.  Writes d_keep [n] int32: 1 for the
 *            kept candidate of every cell, 0 elsewhere
 *   compact  d_keep_scan [n] int64 = inclusive scan of d_keep, n_out its last element.  Writes d_points [n_out,3] fp32, d_out_tri [n_out]
 * rows, emit, winners and compact are one kernel each on `stream` (winners after one memset) with no host synchronisation. */
int psi_mesh_cloud_count(const float *d_verts, const int32_t *d_faces, int nv, int nf, float spacing, int32_t *d_tri_rows, float origin[3],
                         long long *n_rows, long long *n_cands, void *stream);
int psi_mesh_cloud_rows(const float *d_verts, const int32_t *d_faces, int nv, int nf, float spacing, const int64_t *d_tri_row_off,
                        long long n_rows, int32_t *d_row_tri, int32_t *d_row_cnt, void *stream);
int psi_mesh_cloud_emit(const float *d_verts, const int32_t *d_faces, int nv, int nf, float spacing, const float origin[3],
                        const int64_t *d_tri_row_off, const int32_t *d_row_tri, const int64_t *d_row_off, long long n_rows, long long n_cands,
                        float *d_pos, int32_t *d_tri, int64_t *d_cell, uint32_t *d_key, void *stream);
int psi_mesh_cloud_winners(const int64_t *d_cell_sorted, const int64_t *d_perm, const uint32_t *d_key, long long n, int32_t *d_keep,
                           void *stream);
int psi_mesh_cloud_compact(const float *d_pos, const int32_t *d_tri, const int32_t *d_keep, const int64_t *d_keep_scan, long long n,
                           long long n_out, float *d_points, int32_t *d_out_tri, void *stream);

/* ---- orienting a scene mesh towards free space: the two device steps of scene_sdf.orient_faces ----
 * psi_flood_fill: d_free (device, u8 [Dx,Dy,Dz], element [ix][iy][iz], overwritten) becomes 1 at the nodes of d_open (same shape, non-zero =
 * open, only read) that are 6-connected through open nodes to one of the n seed nodes d_seed_nodes [n,3] int32 (ix, iy, iz), 0 elsewhere.  A
 * seed node outside the grid or on a node that is not open contributes nothing.  One wave owns an 8 x 8 x 8 brick of nodes, keeps it and a
 * one-node apron as bits in LDS, floods it to convergence locally, writes the nodes it gained and raises the launch's word (integer
 * atomicOr) when it gained one.  The call launches the kernel until a launch raises nothing, reads the words of 8 launches back at a time
 * (it synchronises `stream` once per 8 launches) and stores in *h_rounds (host, may be NULL) the number of launches up to and including the
 * first that gained nothing.  A launch reads what the launch before it left, never what another workgroup of the same launch writes: the
 * set and *h_rounds are the same from run to run.  The words come from the library's per-stream scratch.
 * PSI_EINVAL: an edge outside 2 .. 1024, n < 1, d_open == d_free.
 *
 * psi_mesh_orient_votes: for sample i < n (d_points [n,3] fp32 on triangle d_tri[i] of d_faces [nf,3] int32 over d_verts [nv,3] fp32), in
 * fp32, not contracted, IEEE division and square root: u = b - a, v = c - a, cr = u x v (each component one product minus the other),
 * len = sqrtf((cr.x cr.x + cr.y cr.y) + cr.z cr.z); a sample whose len is not > 0 casts no vote; q = p +- delta * (cr / len) per axis;
 * the node of q is rintf((q - gmin) / step) per axis, step = (gmax - gmin) / (float)(D - 1), the nodes of psi_mesh_sdf_compute; a probe
 * whose node lies outside [0, D - 1] on an axis is not free.  d_votes [nf,2] int32 (zeroed by the call) counts per triangle the samples
 * whose front probe (+) and whose back probe (-) hit a free node of d_free (u8 [D,D,D]), by integer atomicAdd.  One lane per sample; a
 * sample whose triangle lies outside [0, nf) or whose triangle refers to a vertex outside [0, nv) casts no vote.  One memset and one kernel
 * on `stream`, no host synchronisation.  PSI_EINVAL: D outside 2 .. 1024, bounds as psi_mesh_sdf_compute, delta not positive and finite,
 * n outside 0 .. 2^31 - 1. */
int psi_flood_fill(const uint8_t *d_open, int Dx, int Dy, int Dz, const int32_t *d_seed_nodes, int n, uint8_t *d_free, int *h_rounds, void *stream);
int psi_mesh_orient_votes(const float *d_points, const int32_t *d_tri, long long n, const float *d_verts, int nv, const int32_t *d_faces, int nf,
                          const uint8_t *d_free, const float gmin[3], const float gmax[3], int D, float delta, int32_t *d_votes, void *stream);

/* ---- body against body: which vertices of one body of a batch lie inside another body of the batch ----
 * Contract (csrc/body_overlap_shared.h holds the statements).  d_verts [B,V,3] fp32, world frame; the faces [F,3] int32 of the handle are
 * shared by all bodies and wound outwards; d_group [B] int32 or NULL (all bodies in one group):
 *   box        of body j: the exact min / max of its V vertices per axis
 *   candidate  an ordered triple (i, j, v) with i != j, group[i] == group[j] and vertex v of body i inside the closed box of j (comparisons
 *              only); a vertex outside the box is outside the body.  The list is in ascending (i, j, v) order
 *   w          (sum over the F triangles of body j, in face order, of atan2(a . n, |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|)) / 2 pi with
 *              a = A - p, b = B - p, c = C - p and n = (B - A) x (C - A) in fp32 from the body's current vertices; atan2(0, 0) = 0: the
 *              statement of psi_mesh_winding_compute, about 1 inside and about 0 outside
 *   sum        fp32 within a chunk of 256 consecutive faces; the chunk sums added in fp64, in order, within a slice of 2048 consecutive
 *              faces; the slice sums added in fp64 in slice order.  256 and 2048 are constants of the contract, not launch parameters
 *   decision   vertex v of body i is inside j iff w > 0.5
 * No floating-point atomics: every output is bit-identical from run to run, and the w of a triple has the same bits whatever else the
 * batch holds.  The passes of one computation; the scans between them are the caller's (ops.body_overlap):
 *   create   h_faces: HOST [F,3] int32, copied to the device.  PSI_EINVAL: F < 1, V < 1, a face index outside [0, V)
 *   boxes    writes d_boxes [B,6] fp32 (min xyz, max xyz) and *d_bad (device int32): the smallest index of a body with a non-finite
 *            coordinate, a value >= B when there is none
 *   count    writes d_pair_count [B,B] int32: the vertices of i in the closed box of j; 0 on the diagonal, across groups and where the
 *            boxes do not meet (such a pair costs one comparison)
 *   emit     d_cand_off, d_chunk_off [B,B] int64 = the exclusive scans of d_pair_count and of ceil(d_pair_count / 256); n_cand, n_chunks
 *            their totals.  Writes d_cand [n_cand,3] int32 = (i, j, v) and d_chunks [n_chunks,4] int32 = (first candidate, candidates,
 *            i, j): up to 256 candidates of ONE pair
 *   wind     the hot pass, grid = (chunk, slice): writes the fp64 slice sums of every candidate into d_workspace
 *            (psi_body_overlap_workspace_bytes(n_cand, F) = ceil(F / 2048) * n_cand * 8 bytes; 0 for n_cand outside [1, 2^31))
 *   decide   writes d_w [n_cand] fp32 and adds into d_counts [B,B] int32 and d_mask [B, ceil(V / 32)] uint32 (bit v % 32 of word v / 32:
 *            vertex v is inside another body), which the CALLER has zeroed, by integer atomics
 * Each pass is one kernel on `stream` (boxes after one memset) with no host synchronisation; none launches an empty grid: with n_cand = 0
 * the caller stops after count.  PSI_EINVAL: a null pointer (d_group excepted), B < 1 or B > 46340, n_cand outside [1, 2^31), n_chunks
 * outside [1, n_cand], a workspace smaller than the query's value. */
typedef struct psi_body_overlap psi_body_overlap;
int psi_body_overlap_create(psi_body_overlap **out, const int32_t *h_faces, int V, int F);
void psi_body_overlap_destroy(psi_body_overlap *h);
/* info[0] = V, info[1] = F */
int psi_body_overlap_info(const psi_body_overlap *h, int32_t info[2]);
size_t psi_body_overlap_workspace_bytes(long long n_cand, int F);
int psi_body_overlap_boxes(const psi_body_overlap *h, const float *d_verts, int B, float *d_boxes, int32_t *d_bad, void *stream);
int psi_body_overlap_count(const psi_body_overlap *h, const float *d_verts, const int32_t *d_group, int B, const float *d_boxes,
                           int32_t *d_pair_count, void *stream);
int psi_body_overlap_emit(const psi_body_overlap *h, const float *d_verts, const int32_t *d_group, int B, const float *d_boxes,
                          const int32_t *d_pair_count, const int64_t *d_cand_off, const int64_t *d_chunk_off, long long n_cand,
                          long long n_chunks, int32_t *d_cand, int32_t *d_chunks, void *stream);
int psi_body_overlap_wind(const psi_body_overlap *h, const float *d_verts, int B, const int32_t *d_cand, long long n_cand,
                          const int32_t *d_chunks, long long n_chunks, void *d_workspace, size_t workspace_bytes, void *stream);
int psi_body_overlap_decide(const psi_body_overlap *h, int B, const int32_t *d_cand, long long n_cand, const void *d_workspace,
                            size_t workspace_bytes, float *d_w, int32_t *d_counts, uint32_t *d_mask, void *stream);

/* ---- body against body: penetration depth, its aggregates and the gradient rows of the penetration loss ----
 * Contract (csrc/body_depth_shared.h and csrc/closest_point_shared.h hold the statements; no contraction, IEEE division and square root:
 * an fp32 NumPy restatement gives the same bits).  h: a psi_body_overlap handle (its faces); d_verts [B,V,3] fp32; d_trip [n,3] int32 =
 * (i, j, v), strictly ascending, i != j, every index in range: vertex v of body i against body j.  Any triple is allowed; the inside triples
 * of a batch are the candidates of psi_body_overlap_* with w > 0.5, in their order.
 *   record     of face t of body j: a = X[f0], ab = X[f1] - a, ac = X[f2] - a, each rounded once, from the current vertices
 *   test       ap = p - a; the seven-region closest point of psi_mesh_sdf (same routine, same order of tests) gives r = p - c and the
 *              region (0 face, 1 edge ab, 2 edge bc, 3 edge ca, 4 5 6 vertex a b c); d2 = (r.x*r.x + r.y*r.y) + r.z*r.z
 *   winner     the face with the smallest key = bits(d2) << 32 | t, compared as unsigned: equal d2 goes to the lower face, a non-finite d2
 *              (a collinear face can give one) loses to every finite one; the visiting order is free
 *   row        face, region, depth = sqrt(d2), r [3], bary [3] = the barycentric coordinates of c, from the quotients v, w the routine
 *              forms: region 4 (1,0,0), 5 (0,1,0), 6 (0,0,1), 1 (1-v,v,0), 3 (1-w,0,w), 2 (0,1-w,w), 0 ((1-v)-w,v,w)
 *   aggregates over the inside triples, in triple order: max_depth [B,B] fp32 (integer maximum of the bits), sum_depth and sum_sq [B,B]
 *              fp64 (sum += (double)depth; sum_sq += (double)depth * (double)depth, one triple after the other), depth_of [B,V] fp32 (the
 *              largest depth of a vertex over all j), loss [2,B] fp32: loss[0,i] = (float) sum_j sum_depth[i,j], loss[1,i] the same of
 *              sum_sq, the pair sums added in fp64 in j order
 *   gradient   of sum_i g[i] loss[p,i], exact where the winner is unique: s = (depth > 0 ? 1 / depth : 0) for penalty 0 (depth), s = 2
 *              for penalty 1 (squared); u = (g[i] * s) * r; triple k gives rows 4k .. 4k+3: (i V + v, +u) and (j V + f_m, -(bary[m] * u)),
 *              m = 0, 1, 2.  The caller sorts the targets stably; psi_segment_sum3 adds every run in sorted order in fp32
 * No floating-point atomics: every output is bit-identical from run to run, and the row of a triple does not depend on the rest of the
 * batch.  The passes (each one kernel on `stream`, no host synchronisation, none launches an empty grid: with n = 0 the caller stops):
 *   nearest    the hot pass, grid = (256-triple chunk of ONE pair, 2048-face slice).  d_chunks [n_chunks,4] int32 = (first triple,
 *              triples, i, j) as psi_body_overlap_emit writes it, rebuilt by the caller for its list.  Writes one uint64 key per (slice,
 *              triple) into d_workspace (psi_body_depth_workspace_bytes(n, F) = ceil(F / 2048) * n * 8 bytes; 0 for n outside [1, 2^29))
 *   finish     the smallest key over the slices, the winner's statement once more (the same inputs, the same bits); writes d_face,
 *              d_region [n] int32, d_depth [n], d_r and d_bary [n,3] fp32
 *   pairs      one workgroup per body; d_row_start [B+1] int64 = the first triple of every body i.  Writes d_loss [2,B] and the non-zero
 *              entries of d_max_depth, d_sum_depth, d_sum_sq [B,B] and d_depth_of [B,V], all four ZEROED BY THE CALLER
 *   grad_rows  d_g [B] fp32; writes d_targets [4n] int64 and d_rows [4n,3] fp32
 *   psi_segment_sum3  general: d_targets_sorted [m] int64 ascending, d_order [m] int64 (row d_order[k] belongs to sorted position k) or NULL
 *              (the rows are in sorted order), d_rows [m,3] fp32.  The lane that starts a run of equal targets adds the run in order,
 *              ((0 + x0) + x1) + ..., and stores d_out[target] once; d_out [n_out,3] is ZEROED BY THE CALLER, targets outside [0, n_out)
 *              are ignored
 * PSI_EINVAL: a null pointer (d_order excepted), B < 1 or B > 46340, n outside [1, 2^29), n_chunks outside [1, n], a workspace smaller than
 * the query's value, a penalty other than 0 or 1, m outside [1, 2^31), n_out < 1. */
size_t psi_body_depth_workspace_bytes(long long n, int F);
int psi_body_depth_nearest(const psi_body_overlap *h, const float *d_verts, int B, const int32_t *d_trip, long long n, const int32_t *d_chunks,
                           long long n_chunks, void *d_workspace, size_t workspace_bytes, void *stream);
int psi_body_depth_finish(const psi_body_overlap *h, const float *d_verts, int B, const int32_t *d_trip, long long n, const void *d_workspace,
                          size_t workspace_bytes, int32_t *d_face, int32_t *d_region, float *d_depth, float *d_r, float *d_bary, void *stream);
int psi_body_depth_pairs(const psi_body_overlap *h, int B, const int32_t *d_trip, long long n, const float *d_depth, const int64_t *d_row_start,
                         float *d_max_depth, double *d_sum_depth, double *d_sum_sq, float *d_depth_of, float *d_loss, void *stream);
int psi_body_depth_grad_rows(const psi_body_overlap *h, int B, const int32_t *d_trip, long long n, const int32_t *d_face, const float *d_depth,
                             const float *d_r, const float *d_bary, const float *d_g, int penalty, int64_t *d_targets, float *d_rows,
                             void *stream);
int psi_segment_sum3(const int64_t *d_targets_sorted, const int64_t *d_order, const float *d_rows, long long m, float *d_out, long long n_out,
                     void *stream);

/* ---- Surface crossings: which pairs of triangles of the posed body surfaces of a batch properly intersect (csrc/surface_crossings.hip) ----
 * Contract (csrc/surface_crossings_shared.h holds the statements).  d_verts [B,V,3] fp32, world frame; the faces
 * [F,3] int32 of the handle are shared by all bodies; d_group [B] int32 or NULL; flags = 1 (self pairs) | 2 (between bodies) | 4 (brute:
 * no body-box and no chunk-box culling):
 *   face box   the exact min / max of the face's three vertices
 *   candidate  an unordered pair of faces ((i,s),(j,t)), (i,s) < (j,t): between: i < j and group[i] == group[j]; self: i == j, s < t, no
 *              shared vertex index and part_skip[face_part[s], face_part[t]] == 0; and the two closed face boxes meet
 *   predicate  fifteen fp32 values with fixed association (no contraction): the plane values sP, sQ and the edge values D[3][3]; edge i of
 *              P pierces Q iff sP[i], sP[i+1] are strictly of opposite sign and D[i][0..2] are all > 0 or all < 0; Q against P alike.  The
 *              values keep their bits when P and Q swap roles
 *   decision   the pair crosses iff events >= 1 (events = piercing edges, 0 to 6); events == 2 is regular, and only then is length the
 *              distance of the two piercing points x = a + t (b - a), t = s_a / (s_a - s_b) (division and square root IEEE-rounded)
 * No floating-point atomics: every output is bit-identical from run to run and the row of a pair does not depend on the rest of the batch,
 * on the groups or on the chunk order.  The passes of one computation; the scans and the sort between them are the caller's
 * (ops.surface_crossings):
 *   face_order  HOST: h_order [F] = the caller's face index at every position of the chunk order: 0..F-1 without h_order_verts, else
 *               sorted along a Morton curve (10 bits per axis) of the face centroids of h_order_verts [V,3], ties in face order
 *   create      h_faces HOST [F,3]; h_order_verts HOST [V,3] or NULL; h_face_part HOST [F] int32 and h_part_skip HOST [P,P] uint8
 *               (symmetric) or both NULL with P = 0.  PSI_EINVAL: F < 1, F >= 2^21, V < 1, a face index outside [0,V), a part outside [0,P)
 *   info        info[0..3] = V, F, chunks = ceil(F / 256), P
 *   boxes       d_chunk_boxes [B,chunks,6] and d_body_boxes [B,6] fp32 (min xyz, max xyz), *d_bad (device int32): the smallest index of a
 *               body with a non-finite coordinate, a value >= B when there is none
 *   tiles       a job is (i,j), i <= j, admitted by flags and groups, whose body boxes meet; a tile is (i, j, ca, cb), ca <= cb when i == j,
 *               whose chunk boxes meet.  Count pass (d_job_off = d_tiles = NULL, n_tiles = 0): writes d_job_tiles [B,B] int32.  Emit pass:
 *               d_job_off [B,B] int64 = the exclusive scan of d_job_tiles, n_tiles its total; writes d_tiles [n_tiles,4] int32
 *   test        the hot pass, one workgroup per tile.  Count pass (d_tile_off = d_keys = d_events = d_length = NULL, n_pairs = 0): writes
 *               d_tile_hits [n_tiles] int32.  Emit pass: d_tile_off [n_tiles] int64 = its exclusive scan, n_pairs its total; writes
 *               d_keys [n_pairs] int64 = ((i F + s) B + j) F + t, d_events, d_length, in no particular order
 *   finish      d_keys_sorted ascending, d_order [n_pairs] int64 = where each came from, d_row_start [B+1] int64 = the first sorted row
 *               of every body i.  Writes d_pairs [n_pairs,4] = (i,s,j,t), d_events, d_length; adds into d_counts [B,B] int32 (symmetric),
 *               d_face_mask [B, ceil(F/32)] uint32 and *d_irregular (events != 2) by integer atomics, and writes into d_contour [B,B] fp64
 *               the lengths of the pairs of (i,j) added sequentially in pair order, mirrored: all four ZEROED BY THE CALLER
 * No pass launches an empty grid: with n_tiles = 0 or n_pairs = 0 the caller stops.  PSI_EINVAL: a null pointer (optional ones excepted),
 * B < 1 or B > 46340, (B F)^2 >= 2^63 (the key is one int64), n_tiles or n_pairs outside [1, 2^31). */
typedef struct psi_surface_crossings psi_surface_crossings;
int psi_surface_crossings_face_order(const int32_t *h_faces, int V, int F, const float *h_order_verts, int32_t *h_order);
int psi_surface_crossings_create(psi_surface_crossings **out, const int32_t *h_faces, int V, int F, const float *h_order_verts,
                                 const int32_t *h_face_part, const uint8_t *h_part_skip, int P);
void psi_surface_crossings_destroy(psi_surface_crossings *h);
int psi_surface_crossings_info(const psi_surface_crossings *h, int32_t info[4]);
int psi_surface_crossings_boxes(const psi_surface_crossings *h, const float *d_verts, int B, float *d_chunk_boxes, float *d_body_boxes,
                                int32_t *d_bad, void *stream);
int psi_surface_crossings_tiles(const psi_surface_crossings *h, const int32_t *d_group, int B, int flags, const float *d_chunk_boxes,
                                const float *d_body_boxes, int32_t *d_job_tiles, const int64_t *d_job_off, long long n_tiles,
                                int32_t *d_tiles, void *stream);
int psi_surface_crossings_test(const psi_surface_crossings *h, const float *d_verts, int B, const int32_t *d_tiles, long long n_tiles,
                               int32_t *d_tile_hits, const int64_t *d_tile_off, long long n_pairs, int64_t *d_keys, int32_t *d_events,
                               float *d_length, void *stream);
int psi_surface_crossings_finish(const psi_surface_crossings *h, int B, const int64_t *d_keys_sorted, const int64_t *d_order,
                                 const int32_t *d_events_in, const float *d_length_in, long long n_pairs, const int64_t *d_row_start,
                                 int32_t *d_pairs, int32_t *d_events, float *d_length, int32_t *d_counts, double *d_contour,
                                 uint32_t *d_face_mask, int32_t *d_irregular, void *stream);

/* ---- Surface crossings: the conic distance field of a list of triangle pairs, its loss and the rows of its gradient (csrc/crossing_field.hip) ----
 * Contract (csrc/crossing_field_shared.h holds the statements and their association).  d_verts [B,V,3] fp32; h a
 * psi_surface_crossings handle; d_pairs [n,4] int32 (i, s, j, t) in the caller's face indices, strictly ascending, i <= j, 16-byte aligned;
 * 0 < sigma <= 0.5.  The field is the conic distance field of Tzionas et al. 2016, zero outside the cone; no compatibility with any other
 * implementation is claimed.
 *   record      of the receiver (a,b,c): N = (b-a) x (c-a), n = N / sqrt(N.N), the circumcentre o and the circumradius r
 *   evaluation  of p: h = n.(p-o), rho = |(p-o) - h n|; gate 1: h < sigma; Phi = rho / (r (1 - h/sigma)); gate 2: Phi < 1; Psi = (1 - Phi) Y(h),
 *               Y = (1 - h) - sigma for h <= -sigma, else (c0 - c1 h) - (c2 h) h.  Both gates are positive comparisons: a NaN or an infinity
 *               anywhere (a collinear receiver) gives Psi = 0 and zero gradient rows
 *   role        0: the corners of (i,s) in the record of (j,t); 1: the other way round.  energy = (Psi0^2 + Psi1^2) + Psi2^2
 *   eval        writes d_psi [n,2,3] and d_energy [n,2]
 *   pairs       d_cells_sorted [2n] int64 ascending and d_order [2n] int64: the caller's STABLE sort of the entries e = 2 k + role by their
 *               cell (role 0: i B + j; role 1: j B + i); d_row_start [B+1] int64 = the first sorted position of every row of cells.  Writes
 *               into d_pair_energy [B,B] fp64 (ZEROED BY THE CALLER; not symmetric) the entries of a cell added one after the other in pair
 *               order, a self pair as (double) e0 + (double) e1 at its role-0 entry, and d_loss [B] = (float) sum_j E[i,j] in j order
 *   grad_rows   the forward once more, then per (pair, role) six rows d_rows [12 n,3] and targets d_targets [12 n] int64 = body V + vertex:
 *               the intruder's corners, then the receiver's; role 0 scaled by d_g[i], role 1 by d_g[j]; -1 targets for a pair out of range.
 *               The caller sorts the targets stably and reduces with psi_segment_sum3
 * No floating-point atomics; every index read from a caller's table is range-checked; no pass launches an empty grid (n = 0: the caller
 * stops).  PSI_EINVAL: a null pointer, B < 1 or B > 46340, n outside [1, 2^27), sigma outside (0, 0.5], a misaligned d_pairs. */
int psi_crossing_field_eval(const psi_surface_crossings *h, const float *d_verts, int B, const int32_t *d_pairs, long long n, float sigma,
                            float *d_psi, float *d_energy, void *stream);
int psi_crossing_field_pairs(const psi_surface_crossings *h, int B, const int32_t *d_pairs, long long n, const float *d_energy,
                             const int64_t *d_cells_sorted, const int64_t *d_order, const int64_t *d_row_start, double *d_pair_energy,
                             float *d_loss, void *stream);
int psi_crossing_field_grad_rows(const psi_surface_crossings *h, const float *d_verts, int B, const int32_t *d_pairs, long long n,
                                 float sigma, const float *d_g, int64_t *d_targets, float *d_rows, void *stream);

/* ---- Body against body: move overlapping bodies apart rigidly (csrc/body_separate.hip) ----
 * Contract (csrc/body_separate_shared.h holds the statements and their association).  Every body of a batch has a
 * rigid state, all fp32: d_quat [B,4] (w, x, y, z), d_transl [B,3], d_pivot [B,3], and the Adam moments d_m, d_s [B,6].
 *   pose     d_verts [B,V,3] = R(quat) (d_base - pivot) + (pivot + transl), x_k = ((R_k0 d0 + R_k1 d1) + R_k2 d2) + p_k; a body whose state is
 *            exactly quat = (1,0,0,0), transl = 0 gets the bits of d_base
 *   wrench   d_G [B,V,3] = dL/dverts, d_p [B,3] = pivot + transl.  Per vertex a = x - p, c = a x G in fp32; (G, c) widened to fp64 and added
 *            over every chunk of 256 consecutive vertices by the tree s[l] += s[l + stride], stride = 128 .. 1 (lanes past V hold +0):
 *            d_chunks [B, ceil(V / 256), 6] fp64.  With d_g6 != NULL a second launch adds the chunks of a body in chunk order in fp64 and
 *            rounds once: d_g6 [B,6] fp32 = (force, torque about p)
 *   step     step k of Adam on g6 (zero for a body with d_fixed[b] != 0; d_fixed [B] int32 or NULL), in place: m = b1 m + (1 - b1) g,
 *            s = b2 s + ((1 - b2) g) g, u = (m / c1) / (sqrt(s / c2) + eps), transl -= lr_t u[0:3], delta = -(lr_r u[3:6]),
 *            quat <- normalise((1, delta / 2) (x) quat) unless delta is exactly zero.  c1 = (float)(1 - b1^k) and c2 = (float)(1 - b2^k)
 *            come from the caller, computed in fp64.  With d_chunks != NULL (nchunk = ceil(V / 256)) the launch first adds the chunks as
 *            wrench's second stage does and stores d_g6; with d_chunks == NULL, nchunk == 0 it reads d_g6
 * Each pass is one kernel on `stream` (wrench with d_g6: two), no host synchronisation, no floating-point atomics: the sums do not depend
 * on the grid and every output is bit-identical from run to run and to the fp32 NumPy restatement.  None launches an empty grid.
 * PSI_EINVAL: a null pointer, B < 1 or B > 46340, V < 1 or V > 2^24, a beta outside [0, 1), a bias correction outside (0, 1], a negative or
 * non-finite eps, a non-positive or non-finite learning rate, nchunk that does not go with d_chunks. */
int psi_body_separate_pose(const float *d_base, const float *d_quat, const float *d_transl, const float *d_pivot, int B, int V, float *d_verts,
                           void *stream);
int psi_body_separate_wrench(const float *d_verts, const float *d_G, const float *d_p, int B, int V, double *d_chunks, float *d_g6,
                             void *stream);
int psi_body_separate_step(const double *d_chunks, int nchunk, float *d_g6, float *d_quat, float *d_transl, float *d_m, float *d_s,
                           const int32_t *d_fixed, int B, float b1, float b2, float c1, float c2, float eps, float lr_t, float lr_r,
                           void *stream);
/* The scene term of the separation: the bodies d_verts [B,V,3] against signed distance volumes.  The scene table has the form of
 * psi_sdf_sample_forward with align_corners = 1: d_sdf [S,D,D,D] fp32, element [ix][iy][iz]; d_gmin, d_gmax [S,3] (device); d_scene_id [B]
 * int32 or NULL (scene 0; a value outside [0,S) is clamped).  Per axis k = (float)((D - 1) / ((double)gmax - gmin)), u = (x - gmin) k,
 * clamped to [0, D - 1]; the eight corners of the cell are interpolated along z, then y, then x with lerp(a, b, w) = a + w (b - a); the
 * gradient comes from the same differences, times k, and is an exact zero along an axis whose u is not strictly inside (0, D - 1)
 * (csrc/body_separate_shared.h has every statement).  A vertex with value < 0 is in the scene: G = (-w_scene) g and -value its loss;
 * every other vertex contributes exact zeros.  Outputs per chunk of 256 consecutive vertices, by the tree of wrench: d_chunks
 * [B, ceil(V / 256), 6] fp64 = the sums of (G, (x - p) x G) with d_p [B,3] = pivot + transl, d_count [B, ceil(V / 256)] int32 = the
 * vertices in the scene, d_loss [B, ceil(V / 256)] fp64 = the sum of -value.  d_sdf_out [B,V] and d_G_out [B,V,3] (fp32) receive the value
 * and G of every vertex when not NULL.  One kernel on `stream`, no host synchronisation, no floating-point atomics; bit-identical from
 * run to run and to the fp32 NumPy restatement.  PSI_EINVAL: a null pointer (but d_scene_id, d_sdf_out, d_G_out), B or V outside the
 * limits above, D < 2, S < 1, a negative or non-finite w_scene. */
int psi_body_separate_scene(const float *d_verts, const float *d_p, const float *d_sdf, const float *d_gmin, const float *d_gmax,
                            const int32_t *d_scene_id, int B, int V, int D, int S, float w_scene, double *d_chunks, int32_t *d_count,
                            double *d_loss, float *d_sdf_out, float *d_G_out, void *stream);

/* ---- Scene crossings: which body triangles of a batch properly intersect which triangles of a static scene mesh (csrc/scene_crossings.hip) ----
 * Contract (the per-pair statements are csrc/surface_crossings_shared.h, the key and the host half of create
 * csrc/scene_crossings_shared.h).  The scene: h_verts HOST [nv,3] fp32 and h_faces HOST [nf,3] int32, fixed for the life of the handle;
 * degenerate triangles are kept.  The bodies: d_verts [B,V,3] fp32, world frame, with the topology of the psi_surface_crossings handle
 * `body`.
 *   candidate  a body face (i, s) and a scene triangle t whose closed exact face boxes meet
 *   decision   sc_pair(P = body face, Q = scene triangle), both in the caller's corner order: crosses iff events >= 1; length as in
 *              psi_surface_crossings_*
 *   create     HOST work only, no kernel: the triangles sorted along a Morton curve (10 bits per axis) of their centroid sums (fp64) over
 *              the box of those sums, ties to the lower index; chunks of 256 positions; the exact box of every chunk and of the scene by
 *              comparisons; uploaded per position: the nine coordinates and the caller's index
 *   info       info[4] = nv, nf, scene chunks, 0
 *   tiles      a job is a body chunk (i, c), a tile (i, c, k) a job and a scene chunk whose boxes meet (brute = 1: every (i, c, k)); a
 *              body or body chunk whose box misses the scene's box has none.  d_chunk_boxes [B, body chunks, 6] and d_body_boxes [B,6]
 *              are what psi_surface_crossings_boxes wrote for `body`.  Called twice: with d_job_off = d_tiles = NULL, n_tiles = 0 it
 *              writes d_job_tiles [B, body chunks]; with d_job_off (the caller's exclusive scan of d_job_tiles, int64) it writes d_tiles
 *              [n_tiles,4] int32 (i, c, k, 0), the tiles of a job in ascending k
 *   test       one workgroup per tile.  With d_keys = NULL (and d_tile_off, d_events, d_length NULL, n_pairs = 0) it writes d_tile_hits
 *              [n_tiles]; with d_tile_off (the exclusive scan, int64) it writes the key (i F + s) nf + t (s, t: the caller's indices),
 *              events and length of every crossing pair from d_tile_off[tile] on, in any order within the tile
 *   finish     d_keys_sorted and d_order: the caller's sort of d_keys; d_row_start [B+1] int64: the first row of every body.  Writes
 *              d_pairs [n,3] int32 (i, s, t), d_events [n], d_length [n]; adds into d_counts [B] int32, ors into d_face_mask
 *              [B, ceil(F / 32)] and d_tri_mask [ceil(nf / 32)] (bit k of word k >> 5 at position k & 31), counts d_irregular (events
 *              != 2), and writes d_contour [B] fp64 of the bodies with rows: their lengths added one after the other in row order.  The
 *              five ZEROED BY THE CALLER
 * No floating-point atomics: every output is bit-identical from run to run, and the rows of a body depend neither on the rest of the batch
 * nor on the order of the body faces or of the scene triangles.  No pass launches an empty grid: with n_tiles = 0 or n_pairs = 0 the
 * caller stops.  PSI_EINVAL: a null pointer; create: nv < 1, nf < 1, a face index outside [0, nv), a non-finite referenced vertex; B < 1
 * or B > 46340; B F nf >= 2^63 (the key is one int64); n_tiles or n_pairs outside [1, 2^31). */
typedef struct psi_scene_crossings psi_scene_crossings;
int psi_scene_crossings_create(psi_scene_crossings **out, const float *h_verts, int nv, const int32_t *h_faces, int nf);
void psi_scene_crossings_destroy(psi_scene_crossings *h);
int psi_scene_crossings_info(const psi_scene_crossings *h, int32_t info[4]);
int psi_scene_crossings_tiles(const psi_scene_crossings *h, const psi_surface_crossings *body, int B, int brute, const float *d_chunk_boxes,
                              const float *d_body_boxes, int32_t *d_job_tiles, const int64_t *d_job_off, long long n_tiles, int32_t *d_tiles,
                              void *stream);
int psi_scene_crossings_test(const psi_scene_crossings *h, const psi_surface_crossings *body, const float *d_verts, int B,
                             const int32_t *d_tiles, long long n_tiles, int32_t *d_tile_hits, const int64_t *d_tile_off, long long n_pairs,
                             int64_t *d_keys, int32_t *d_events, float *d_length, void *stream);
int psi_scene_crossings_finish(const psi_scene_crossings *h, const psi_surface_crossings *body, int B, const int64_t *d_keys_sorted,
                               const int64_t *d_order, const int32_t *d_events_in, const float *d_length_in, long long n_pairs,
                               const int64_t *d_row_start, int32_t *d_pairs, int32_t *d_events, float *d_length, int32_t *d_counts,
                               double *d_contour, uint32_t *d_face_mask, uint32_t *d_tri_mask, int32_t *d_irregular, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PSI_HIP_H */
