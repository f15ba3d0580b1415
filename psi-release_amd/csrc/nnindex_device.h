// Device side of the exact NN index (nnindex.hip): node / tree descriptors, the 64-bit (distance, index) key and the search body.
// In a header because two translation units instantiate the search: nnindex.hip (the operator entry points) and fit.hip (the fused
// fitting engine runs it inside the same launch as the skinning + SDF kernel, with a query source that skins the contact vertex itself).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "psi_common.h"
#include "search_sum_order.h"
#include "search_shape.h"

#ifndef PSI_SSTOP
#define PSI_SSTOP(k)
#endif
#ifdef PSI_HEAD_STOPS
// dev: per workgroup {queries that took the tree walk, most node + leaf visits of one query, visits summed, grid points evaluated (max)}
__device__ int psi_kd_stat[4 * 8192];
__device__ int psi_kd_reason[8];        // dev: why a warm query took the tree walk — 0 too many candidates, 1 too many surviving columns, 2 tie flag, 3 no warm candidate
__device__ unsigned long long psi_kd_mark[4 * 8192];   // wall clock (10 ns) of thread 0 at four points of the search body
#define PSI_KD_STAT(what) what
#define PSI_KD_MARK(k) do { __builtin_amdgcn_sched_barrier(0); if (threadIdx.x == 0 && blockIdx.x < 8192 && psi_dbg_sstop >= 9) psi_kd_mark[4 * blockIdx.x + (k)] = wall_clock64(); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define PSI_KD_STAT(what)
#define PSI_KD_MARK(k)
#endif

namespace psikd {

constexpr int LEAF = 8;             // points per leaf; leaves are PADDED to exactly 8 records (copies of the last point)
constexpr int WIDE = 8;             // children per internal node == lanes per query
constexpr int MAXSTACK = 72;        // <= 7 pushes per level; 9 levels of fan-out 8 cover 2^24 points
constexpr int QBLK = 256;           // threads per workgroup
#ifndef PSI_KD_LPQ
#define PSI_KD_LPQ 4
#endif
// Lanes per query: a template parameter LPQ of the search (8: one child box / leaf point per lane; 4: two; 2: four).  Measured at
// B*n_c = 65536, the search as a launch of its own: 4 lanes 28.8 us cold / 23.2 warm, 8 lanes 31.4 / 22.5; the fused iteration is 1.3 us
// faster with 4 than with 8.  LPQ_OPS is the width of the stand-alone operators (kd_query_kernel: a cold tree walk wants the wider group)
// unless the index was created under PSI_NN_SEARCH_LANES=2; the fused fitting engine chooses its own (fit.hip: fit_decide).
constexpr int LPQ_OPS = PSI_KD_LPQ;
static_assert(LPQ_OPS == 4 || LPQ_OPS == 8, "PSI_KD_LPQ: 4 or 8 (2 lanes are chosen at run time)");
constexpr int kd_cpl(int lpq) { return WIDE / lpq; }                        // children (leaf points) per lane
// Queries per workgroup.  With 2 lanes they are the SAME 64 as with 4 — the partial sums of a workgroup are one slice of 64 queries
// whatever the width (search_sum_order.h) — so only waves 0 and 1 of the 256 threads carry queries and the other two retire at once.
constexpr int kd_qpb(int lpq) { return psi_sum_slice_queries(lpq); }
constexpr int kd_threads(int lpq) { return kd_qpb(lpq) * lpq; }              // threads of the workgroup that take part in the search
static_assert(kd_qpb(4) == QBLK / 4 && kd_qpb(8) == QBLK / 8 && kd_qpb(2) == 64 && kd_threads(2) == 128, "workgroup shapes");
constexpr int EMPTY = (int)0x80000000;

// 8-wide node (256 bytes): per child its exact AABB and its reference, 32 bytes each, so lane c of a query's 8-lane group
// reads child c with two 16-byte loads and the group reads the 256-byte record contiguously.
// Child reference: >= 0 internal node index;  < 0 leaf number L encoded -(L) - 1 (records pts[8L .. 8L+7]);  EMPTY = none
// (its box is [+inf, -inf], i.e. infinitely far).
struct KdChild {
    float mn[3], mx[3];
    int ref;
    int pad;
};
struct KdNode {
    KdChild c[WIDE];
};
static_assert(sizeof(KdNode) == 256, "node record is 256 bytes");

struct KdDev {
    const KdNode *nodes;
    const float4 *pts;              // leaf-ordered, 8 records per leaf: {x,y,z,bitcast(orig index)}
    const float4 *opts;             // original order {x,y,z,bitcast(index)}: warm-start lookups
    int root;                       // child-reference of the root (a leaf when m <= LEAF)
    int m;
    int rows;                       // traversal stack rows this tree needs: 7 pushes per level + slack
    // Uniform grid over the same cloud, for WARM queries (ball_query below): cell (cx,cy,cz) holds gpts[cell_start[i] .. cell_start[i+1]),
    // i = (cx * gn[1] + cy) * gn[2] + cz — the cells of a z-run are one contiguous point range.  cell_start == nullptr: no grid.
    const int *cell_start;          // [gn0*gn1*gn2 + 1]
    const float4 *gpts;             // cell-ordered PAIR records {x0,x1,y0,y1} {z0,z1,bitcast(i0),bitcast(i1)}; NaN records past the end
    float gorg[3], ginv;            // cell of a point: clamp(floor((p - gorg) * ginv), 0, gn - 1), evaluated in fp32 exactly like this
    int gn[3];
};

constexpr int GRID_COLS_PER_LANE = 3;       // (x,y) cell columns of the ball a lane scans per pass over the list of surviving columns ...
#ifndef PSI_KD_GRID_COLS_2LANE
#define PSI_KD_GRID_COLS_2LANE 3
#endif
// (... as the template parameter RPL of the search.  With 2 lanes per query 3 runs make a pass 6 columns, and a ball of 7-12 surviving
// columns takes a second pass — two more dependent rounds; 6 runs keep the pass at 12 columns and measured SLOWER, 0.0901 ms per iteration
// against 0.0857 with 3 and 0.0884 with 4 lanes: profiles/search_width_ab.txt)
constexpr int kd_rpl(int lpq) { return lpq == 2 ? PSI_KD_GRID_COLS_2LANE : GRID_COLS_PER_LANE; }
#ifndef PSI_KD_GRID_LIST_MAX
#define PSI_KD_GRID_LIST_MAX 48
#endif
constexpr int GRID_LIST_MAX = PSI_KD_GRID_LIST_MAX;   // ... which holds at most this many (more: the tree walk) ...
#ifndef PSI_KD_GRID_PAIRS
#define PSI_KD_GRID_PAIRS 4
#endif
constexpr int GRID_PAIRS = PSI_KD_GRID_PAIRS;   // pair records a lane requests per round of its scan (nnindex.hip pads the list for the overshoot)
#ifndef PSI_KD_GRID_MAX_CAND
#define PSI_KD_GRID_MAX_CAND 64
#endif
constexpr int GRID_MAX_CAND = PSI_KD_GRID_MAX_CAND;           // ... out of at most this many columns in the ball's bounding rectangle

// lane permutations inside an 8-lane group as DPP modifiers (no LDS traffic)
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false)); }
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false); }
constexpr int DPP_XOR1 = 0xB1;          // quad_perm [1,0,3,2]
constexpr int DPP_XOR2 = 0x4E;          // quad_perm [2,3,0,1]
constexpr int DPP_HALF_MIRROR = 0x141;  // row_half_mirror: lane i <-> 7 - i inside each 8 lanes

// (d, i) packed into one 64-bit key: d >= +0 always (a sum of squares), so its IEEE-754 bit pattern orders like an
// unsigned integer and  key = bits(d) << 32 | i  orders lexicographically by (d, i) — the lowest-index-among-minima
// rule is a single unsigned 64-bit minimum, with no branches.
typedef unsigned long long kd_key;
__device__ __forceinline__ kd_key kd_pack(float d, int i) { return ((kd_key)(unsigned)__float_as_int(d) << 32) | (unsigned)i; }
__device__ __forceinline__ float kd_key_d(kd_key k) { return __int_as_float((int)(k >> 32)); }
__device__ __forceinline__ int kd_key_i(kd_key k) { return (int)(unsigned)k; }

// minimum of the key over the LPQ (2, 4 or 8) lanes of a group, result in every lane
template <int LPQ>
__device__ __forceinline__ kd_key group_min(kd_key k)
{
#define PSI_STEP(CTRL)                                                                              \
    {                                                                                               \
        kd_key k2 = ((kd_key)(unsigned)dpp_i<CTRL>((int)(k >> 32)) << 32) | (unsigned)dpp_i<CTRL>((int)(unsigned)k); \
        k = k2 < k ? k2 : k;                                                                        \
    }
    static_assert(LPQ == 2 || LPQ == 4 || LPQ == 8, "lanes per query");
    PSI_STEP(DPP_XOR1)
    if (LPQ >= 4) PSI_STEP(DPP_XOR2)
    if (LPQ == 8) PSI_STEP(DPP_HALF_MIRROR)
#undef PSI_STEP
    return k;
}

// CONTACT: fused contact-loss epilogue, identical to nn_resolve_kernel<true> in chamfer.hip
// MULTI: body b is searched in tab[slot[b]] (a set of scenes, one launch) instead of the single tree T0
//
// Why a lane group per query: a batch has only B*n_c = 65536 queries.  One lane per query is 1024 waves — one per SIMD, no
// latency hiding at all — each running ~8000 dependent instructions (measured: 15 cycles per instruction, 41-57 us).
// With the child boxes / leaf points of a visit spread over the group's lanes the per-wave instruction stream shrinks several
// fold in the box and leaf arithmetic, there are 4096-8192 waves to overlap the dependent node loads, and a wave diverges
// over 16 (8) queries, not 64.
//   That was written when every query walked the tree.  Since the grid scan a warm query is a seed, a ball set-up, a column list and a few
// rounds of pair records, and most of what a search wave issues is UNIFORM over a query's lanes (the query source, the seed, the ball set-up,
// the contact epilogue): only the column enumeration, the z-run scan and the rare tree walk split over the group.  So the width is a template
// parameter (LPQ), and the fused fitting engine runs its warm searches with TWO lanes per query — 32 queries per wave, 64 per workgroup in two
// waves (fit.hip: fit_decide; profiles/search_width_ab.txt) — while a stand-alone, cold search keeps the wider group (LPQ_OPS).
// Query source: where a query point comes from.  KdQueryFromMemory reads row qidx[j] (or j) of a [rows,3] table per body; the fused
// fitting engine substitutes a source that SKINS the contact vertex on the spot (fit.hip), so the search does not have to wait for
// the skinning kernel.  Three phases, so that a source's loads travel in as few DEPENDENT rounds as possible (a round trip under the load
// of the fused launch is ~2 us, and a search workgroup's life is a chain of them): issue(b, j, active) = loads that depend on nothing but the
// query's slot, fetch(b) = loads that need issue()'s results (called after the caller has ALSO issued its own first loads), prepare(b)
// = once per workgroup with all threads present (it may use LDS and barriers), point() = the query point.
struct KdQueryFromMemory {
    const float *xyz1;
    const int *qidx;
    long qstride;
    __device__ __forceinline__ void issue(int, int, bool) {}
    __device__ __forceinline__ void fetch(int) {}
    __device__ __forceinline__ void prepare(int) {}
    __device__ __forceinline__ void point(int b, int j, int, float &qx, float &qy, float &qz) const
    {
        const size_t qrow = qidx ? (size_t)qidx[j] : (size_t)j;
        const float *qp = xyz1 + (size_t)b * qstride + qrow * 3;
        qx = qp[0]; qy = qp[1]; qz = qp[2];
    }
    // CONTACT searches: contact_post(o, g) sees the gradient of the query's contact term in lane 0 of its group, contact_finish(b, bx, nbx)
    // runs once per workgroup with all threads present — a source that produced the query point itself can carry that gradient further back
    // on the spot (fit.hip: ContactSkinSrc); a source that read the point from memory has nothing to add
    __device__ __forceinline__ void contact_post(size_t, float, float, float) {}
    __device__ __forceinline__ void contact_finish(int, int, int) {}
};

// sum of the per-group contact terms over the workgroup -> *out: the halving tree and the slots of search_sum_order.h, i.e. the same
// association for every LPQ that shares the slice (2 and 4)
// SPW = 2 (two slices per workgroup, search_sum_order.h): every wave pair reduces its own slice into its own four slots, and the first thread of
// each pair writes its slice's value to ITS `out`
// (pr: the caller's pair, uniform over its waves)
template <int LPQ, int SPW = 1>
__device__ __forceinline__ void kd_block_fsum(float fval, float *__restrict__ out, int pr = 0)
{
    __shared__ float wsum[SPW * psi_sum_parts(LPQ)];
    const int tid = threadIdx.x;
    float v = fval;
#pragma unroll
    for (int o2 = psi_sum_part_lanes(LPQ) / 2; o2 > 0; o2 >>= 1) v += __shfl_down(v, o2, 64);
#pragma unroll
    for (int p = 0; p < psi_sum_parts_per_wave(LPQ); p++)
        if ((tid & 63) == psi_sum_first_lane(LPQ, p)) wsum[(int)(SPW == 2 ? psi_sum_wg_slot(LPQ, SPW, tid >> 6, p) : psi_sum_slot(LPQ, tid >> 6, p))] = v;
    __syncthreads();
    if (tid == pr * psi_sum_wg_pair_threads(LPQ)) {
        float t = 0.0f;
#pragma unroll
        for (int w = 0; w < psi_sum_parts(LPQ); w++) t += wsum[pr * psi_sum_parts(LPQ) + w];
        *out = t;
    }
}

// The traversal stack of the tree walk.  SPW == 1: the query's LDS rows (plain accesses).  SPW == 2: the query's region of an engine-owned
// buffer in global memory (the LDS rows hold the grid scan's column list only).  Entries are written by one lane of the query's group and read
// by all of them, so with global memory the pushes are completed (release) before the next pop is requested, and a pop's values are
// acquired, at workgroup scope: the lanes of a group are lanes of one wave, whose vector memory operations issue in order.
template <int SPW, class T>
__device__ __forceinline__ T kd_stack_ld(const T *p)
{
    if constexpr (SPW == 2) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else return *p;
}
template <int SPW, class T>
__device__ __forceinline__ void kd_stack_st(T *p, T v)
{
    if constexpr (SPW == 2) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else *p = v;
}
template <int SPW>
__device__ __forceinline__ void kd_stack_pushed() { if constexpr (SPW == 2) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); }
template <int SPW>
__device__ __forceinline__ void kd_stack_popped() { if constexpr (SPW == 2) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); }

// The warm-start candidate of a query: last iteration's winner (hint[o], -1 = none) and its coordinates.  Two dependent loads that need
// nothing but the query's slot, as two calls: callers issue the first together with their own first loads and the second together with
// their own dependent loads, and compute the query point while it is in flight.
__device__ __forceinline__ int kd_warm_hint(const int *__restrict__ hint, bool active, size_t o) { return (active && hint) ? hint[o] : -1; }
__device__ __forceinline__ int kd_warm_candidate(const KdDev &T, int h, float4 &hp)
{
    hp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (h < 0 || h >= T.m) return -1;
    hp = T.opts[h];
    return h;
}

// entry (obase + jq) * K + k of a per-query table of 4-byte items, K items per query: uniform base + one 32-bit lane offset
template <class T>
__device__ __forceinline__ T &kd_slot(T *tab, size_t obase, int jq, int K, int k)
{
    return *(T *)((char *)(tab + obase * K + k) + (unsigned)jq * (unsigned)(4 * K));
}

// One round of the search: the workgroup's QPB lane groups answer one query each.  (qx,qy,qz): the group's query (the same values in
// all LPQ lanes of the group), active: the group has a query, o: its output slot (dist / idx / hint / gq index).  Returns the contact
// term s / (s + c) of the query in lane 0 of its group (0 elsewhere) when CONTACT.  No barriers inside: groups are independent.
// o == obase + jq, obase uniform over the workgroup: with two lanes per query the outputs are addressed as (uniform base) + (32-bit lane
// offset), so that no 64-bit lane address waits in registers across the search (kd_slot).
// SPW = 2: the workgroup carries 128 queries; stk_n is the query's [rows] column list in LDS and the walk's stack lives in gstk (kd_stack_*)
template <int LPQ, int RPL, bool CONTACT, int SPW, class QSrc>
__device__ __forceinline__ float kd_query_round(const KdDev &T, QSrc &qsrc, float qx, float qy, float qz, bool active, size_t o, float *__restrict__ dist,
                                                int *__restrict__ idx, float cconst, float gscale, float *__restrict__ gq, int *__restrict__ hint,
                                                int rows, int *smem_i, int h, const float4 &hp, size_t obase, int jq, int *__restrict__ gstk)
{
#pragma clang fp contract(off)    // the distance expression (PSI_SQ3) must not be re-contracted in translation units built with contraction on
    constexpr int CPL = kd_cpl(LPQ);
    const int tid = threadIdx.x;
    const int c = tid & (LPQ - 1);                            // my first child / leaf slot (the others: c + LPQ, ...)
    const int g = tid / LPQ;                                  // query group inside the workgroup
    int *stk_n = smem_i + (size_t)g * rows * (SPW == 2 ? 1 : 2);      // [rows] child references (SPW == 2: the column list only)
    float *stk_d = (float *)(stk_n + rows);                   // [rows] box distances
    kd_key bestk = kd_pack(INFINITY, 0x7fffffff);
    float best = INFINITY;                                    // == kd_key_d(bestk)
    if (h >= 0) {
        // warm start: the target that won for this query last time (fetched by the caller, kd_warm_candidate, BEFORE it produced the query
        // point, so the two dependent loads overlap that work) is evaluated first — an ordinary candidate, so the result is unchanged;
        // a good initial `best` prunes almost every sibling on the way down
        float x2 = hp.x - qx, y2 = hp.y - qy, z2 = hp.z - qz;
        best = PSI_SQ3(x2, y2, z2);
        bestk = kd_pack(best, h);
    }
    int sp = 0;
    int cur = T.root;
    float curd = 0.0f;
    bool have = active;
    PSI_KD_STAT(int nvis = 0; int ngp = 0;)
#ifndef PSI_KD_SEED_CELLS
#define PSI_KD_SEED_CELLS 1.5f
#endif
    if (have && T.cell_start && !(best * T.ginv * T.ginv <= PSI_KD_SEED_CELLS * PSI_KD_SEED_CELLS)) {
        // A FAR (or missing) warm candidate — the first iterations of a fitting loop move a body by a tenth of a metre per step, so last
        // iteration's winner is several cells away and its ball holds hundreds of points (the 30-round scans behind the launch's stragglers,
        // profiles/r06_timeline_fwd_scene.txt) — is first replaced by ANY point near the query: the two points of the pair record in the
        // middle of the query's own cell column, z cells [cz - 1, cz + 1] (two dependent loads: the range, one record).  Ordinary candidates,
        // evaluated with the same expression and compared by the (d, index) key: the result is unchanged, the ball shrinks to about a cell.
        // An empty neighbourhood changes nothing (a query with no candidate at all keeps best = +inf and walks the tree as before).
        // Uniform over the lanes of a group (they hold the same query).
        const float fx = fminf(fmaxf(floorf((qx - T.gorg[0]) * T.ginv), 0.0f), (float)(T.gn[0] - 1));
        const float fy = fminf(fmaxf(floorf((qy - T.gorg[1]) * T.ginv), 0.0f), (float)(T.gn[1] - 1));
        const float fz = fminf(fmaxf(floorf((qz - T.gorg[2]) * T.ginv), 0.0f), (float)(T.gn[2] - 1));
        const int cz0 = max((int)fz - 1, 0), cz1 = min((int)fz + 1, T.gn[2] - 1);
        const unsigned cbase = (unsigned)((int)fx * T.gn[1] + (int)fy) * (unsigned)T.gn[2];
        const int p0 = T.cell_start[cbase + cz0], p1 = T.cell_start[cbase + cz1 + 1];
        if (p1 > p0) {
            const float4 *rp = (const float4 *)((const char *)T.gpts + ((unsigned)((p0 + p1) >> 2) << 5));
            const float4 a = rp[0], b = rp[1];                  // {x0,x1,y0,y1} {z0,z1,i0,i1}; a NaN record past the end compares false
            const float xa = a.x - qx, ya = a.z - qy, za = b.x - qz, xb = a.y - qx, yb = a.w - qy, zb = b.y - qz;
            const float da = PSI_SQ3(xa, ya, za), db = PSI_SQ3(xb, yb, zb);
            const kd_key ka = kd_pack(da, __float_as_int(b.z)), kb = kd_pack(db, __float_as_int(b.w));
            if (da == da && ka < bestk) bestk = ka;
            if (db == db && kb < bestk) bestk = kb;
            best = kd_key_d(bestk);
        }
    }
    // Warm query (a candidate from the previous iteration is known): the winner can only lie in the ball of radius sqrt(best) around
    // the query, so instead of walking the tree — ~8 DEPENDENT node / leaf loads — every point of the grid cells that ball touches is
    // evaluated: two dependent rounds of independent loads (cell ranges, then points).
    //   Which cells: in cell units u = (p - org) * ginv the cell of a point is clamp(floor(u)) per axis, the query sits at uq and the
    // ball has radius ru (inflated by 1e-4 relative + 0.01 cell: far above the rounding of u, of the distance expression and of the
    // square roots below).  Column (cx, cy) can hold a point of the ball only if its (x,y) rectangle — the unit square at (cx, cy)
    // (no point has u outside [0, gn]: nnindex.hip puts the origin at the cloud's minimum) — is within ru of uq; if it is, the ball reaches
    // hz = sqrt(ru^2 - dxy^2) along z in that column, i.e. cells floor(uz - hz) .. floor(uz + hz).  The lanes of the group enumerate
    // the columns of the ball's bounding rectangle, the surviving ones are numbered with a ballot and handed out round-robin through
    // the group's (idle) stack rows, so every lane scans at most RPL z-runs per pass, each one contiguous point range.
    //   Exact for the same reason the tree is: every point with computed d <= best lies in a scanned cell, every scanned point is
    // evaluated with the identical distance expression, and the lowest index among minima wins — inside a lane by scan order (a
    // strictly smaller distance replaces; an EQUAL one raises the tie flag, and a group with a flagged lane re-does the query with
    // the tree walk and its (d, index) keys), across lanes and against the warm candidate by the key.  A ball with too many columns
    // (a body far from the scene) takes the tree walk as well.  All decisions are uniform over the lanes of a group.
    const int gshift = (tid & 63) & ~(LPQ - 1);               // bit position of my group inside the wave's ballot
    if (have && T.cell_start && best < INFINITY) {
        const float ru = __builtin_amdgcn_sqrtf(best) * T.ginv * 1.0001f + 0.01f;          // (1 ulp: inside the slack)
        const float uq[3] = {(qx - T.gorg[0]) * T.ginv, (qy - T.gorg[1]) * T.ginv, (qz - T.gorg[2]) * T.ginv};
        const float topx = (float)(T.gn[0] - 1), topy = (float)(T.gn[1] - 1), topz = (float)(T.gn[2] - 1);
        // A query OUTSIDE the grid's box by (ox, oy, oz) cells: every point of the cloud is at least that far from it along those axes, so
        // the ball reaches only rx = sqrt(ru^2 - oy^2 - oz^2) along x inside the box (ry alike) — the bounding rectangle of a body part
        // that hangs out of the scene is the small cap where its ball touches the box, not the square around the whole ball (those queries
        // used to fall to the tree walk and were the launch's tail: 12-25 dependent node visits each).
        const float ru2 = ru * ru;
        const float ox = fmaxf(fmaxf(-uq[0], uq[0] - topx - 1.0f), 0.0f), oy = fmaxf(fmaxf(-uq[1], uq[1] - topy - 1.0f), 0.0f),
                    oz = fmaxf(fmaxf(-uq[2], uq[2] - topz - 1.0f), 0.0f);
        const float oz2 = oz * oz;
        const float rx = __builtin_amdgcn_sqrtf(fmaxf(ru2 - oy * oy - oz2, 0.0f)), ry = __builtin_amdgcn_sqrtf(fmaxf(ru2 - ox * ox - oz2, 0.0f));
        // clamped as floats: a far query must not overflow the conversion
        const float flx = fminf(fmaxf(floorf(uq[0] - rx), 0.0f), topx), fhx = fminf(fmaxf(floorf(uq[0] + rx), 0.0f), topx);
        const float fly = fminf(fmaxf(floorf(uq[1] - ry), 0.0f), topy), fhy = fminf(fmaxf(floorf(uq[1] + ry), 0.0f), topy);
        const float fny = fhy - fly + 1.0f, fncand = (fhx - flx + 1.0f) * fny;
        if (fncand <= (float)GRID_MAX_CAND) {
            const int ncand = (int)fncand;
            const float rny = __builtin_amdgcn_rcpf(fny);
            const int list_max = min(GRID_LIST_MAX, SPW == 2 ? rows : 2 * rows);  // the list lives in the group's stack rows
            int nsurv = 0;
            for (int c0 = 0; c0 < ncand; c0 += LPQ) {          // (uniform over the group)
                const float fcol = (float)(c0 + c);
                const float fcx = floorf((fcol + 0.5f) * rny);   // column index / ny: the quotient's fraction is >= 0.5 / ny, far from rounding
                const float cxf = flx + fcx, cyf = fly + (fcol - fcx * fny);
                // distance from uq to the column's unit square, per axis (the grid's origin is the cloud's exact minimum and its last cell ends at
                // or beyond the maximum, nnindex.hip: no point lies outside [0, gn], so the edge cells are ordinary unit cells)
                const float dx = fmaxf(fmaxf(cxf - uq[0], uq[0] - cxf - 1.0f), 0.0f), dy = fmaxf(fmaxf(cyf - uq[1], uq[1] - cyf - 1.0f), 0.0f);
                const float h2 = ru2 - dx * dx - dy * dy;
                const bool ok = c0 + c < ncand && h2 >= oz2;         // (h2 = what is left for z; the box itself is oz away)
                const float hz = __builtin_amdgcn_sqrtf(fmaxf(h2, 0.0f));
                const int zlo = (int)fminf(fmaxf(floorf(uq[2] - hz), 0.0f), topz), zhi = (int)fminf(fmaxf(floorf(uq[2] + hz), 0.0f), topz);
                const unsigned gm = (unsigned)(__ballot(ok) >> gshift) & ((1u << LPQ) - 1u);
                const int pos = nsurv + __popc(gm & ((1u << c) - 1u));
                if (ok && pos < list_max) stk_n[pos] = (((int)cxf * T.gn[1] + (int)cyf) << 14) | (zlo << 7) | zhi;
                nsurv += __popc(gm);
            }
            if (nsurv <= list_max && nsurv > 0) {
              typedef float v2f __attribute__((ext_vector_type(2)));
              const v2f qxx = {qx, qx}, qyy = {qy, qy}, qzz = {qz, qz};
              float bd = INFINITY;
              int bi = 0x7fffffff;
              bool tie = false;
              // RPL z-runs per lane at a time; a ball with more columns than that (a body part outside the scene's box touches
              // it in a wide, one-cell-deep cap) takes further passes over the list — each two dependent rounds, against the 12-25 of its tree walk
              for (int s0 = 0; s0 < nsurv; s0 += RPL * LPQ) {
                // my z-runs, as ranges of PAIR records: first pair, rounds of GRID_PAIRS pairs
                int ps[RPL], nr[RPL];
                int cs[RPL], ce[RPL];
                const char *csb = (const char *)T.cell_start;
#pragma unroll
                for (int u = 0; u < RPL; u++) {     // all ranges requested together; a slot past the list re-reads entry 0
                    const int e = stk_n[s0 + c + u * LPQ < nsurv ? s0 + c + u * LPQ : 0];
                    const unsigned base = (unsigned)(e >> 14) * (unsigned)T.gn[2];
                    cs[u] = *(const int *)(csb + ((base + ((unsigned)e >> 7 & 127u)) << 2));
                    ce[u] = *(const int *)(csb + ((base + ((unsigned)e & 127u) + 1u) << 2));
                }
                int rounds = 0;
                PSI_KD_MARK(1);
#pragma unroll
                for (int u = 0; u < RPL; u++) {
                    ps[u] = cs[u] >> 1;
                    nr[u] = (ce[u] > cs[u] && s0 + c + u * LPQ < nsurv) ? (((ce[u] + 1) >> 1) - ps[u] + GRID_PAIRS - 1) / GRID_PAIRS : 0;
                    rounds += nr[u];
                }
                // one loop over the rounds of all my runs: round t reads pairs GRID_PAIRS t + off(t) .., off = the run's first pair minus
                // GRID_PAIRS times the rounds before it
                static_assert(RPL >= 2, "the round -> pair mapping below takes at least two runs");
                int upto[RPL - 1], off[RPL];                   // upto[u]: rounds of runs 0 .. u; run u covers rounds [upto[u - 1], upto[u])
                upto[0] = nr[0];
                off[0] = ps[0];
#pragma unroll
                for (int u = 1; u < RPL; u++) {
                    off[u] = ps[u] - GRID_PAIRS * upto[u - 1];
                    if (u < RPL - 1) upto[u] = upto[u - 1] + nr[u];
                }
                for (int t = 0; t < rounds; t++) {
                    PSI_KD_STAT(ngp += 1;)
                    int offt = off[RPL - 1];
#pragma unroll
                    for (int u = RPL - 2; u >= 0; u--) offt = t < upto[u] ? off[u] : offt;
                    const int pr = GRID_PAIRS * t + offt;
                    const float4 *rp = (const float4 *)((const char *)T.gpts + ((unsigned)pr << 5));
                    float4 a[GRID_PAIRS], b[GRID_PAIRS];
#pragma unroll
                    for (int k = 0; k < GRID_PAIRS; k++) { a[k] = rp[2 * k]; b[k] = rp[2 * k + 1]; }
#pragma unroll
                    for (int k = 0; k < GRID_PAIRS; k++) {
                        const v2f x2 = (v2f){a[k].x, a[k].y} - qxx, y2 = (v2f){a[k].z, a[k].w} - qyy, z2 = (v2f){b[k].x, b[k].y} - qzz;
#ifdef PSI_CHAMFER_FMA
                        // PSI_SQ3 on two points in the fma mode (mul, fma, fma — v_pk_mul / v_pk_fma): the same rounding as the warm
                        // candidate above, the tree leaves below and chamfer.hip, which the exactness argument relies on
                        const v2f d = __builtin_elementwise_fma(z2, z2, __builtin_elementwise_fma(y2, y2, x2 * x2));
#else
                        const v2f d = x2 * x2 + y2 * y2 + z2 * z2;     // PSI_SQ3 on two points (contraction is off in this function)
#endif
                        const int i2[2] = {__float_as_int(b[k].z), __float_as_int(b[k].w)};
#pragma unroll
                        for (int e = 0; e < 2; e++) {
                            const bool lt = d[e] < bd;
                            tie = tie || d[e] == bd;
                            bi = lt ? i2[e] : bi;
                            bd = lt ? d[e] : bd;
                        }
                    }
                }
              }
                kd_key k = group_min<LPQ>(kd_pack(bd, bi));
                PSI_KD_MARK(2);
                bestk = k < bestk ? k : bestk;
                best = kd_key_d(bestk);
                have = ((__ballot(tie) >> gshift) & ((1ull << LPQ) - 1ull)) != 0;     // done, unless a lane met two points at equal distance
                PSI_KD_STAT(if (have && c == 0 && psi_dbg_sstop == 10) atomicAdd(psi_kd_reason + 2, 1);)
            } else { PSI_KD_STAT(if (c == 0 && psi_dbg_sstop == 10) { atomicAdd(psi_kd_reason + 1, 1); atomicMax(psi_kd_reason + 5, nsurv); }) }
        } else { PSI_KD_STAT(if (c == 0 && psi_dbg_sstop == 10) { atomicAdd(psi_kd_reason + 0, 1); atomicMax(psi_kd_reason + 4, (int)fminf(fncand, 1e6f)); }) }
    } else { PSI_KD_STAT(if (have && c == 0 && psi_dbg_sstop == 10) atomicAdd(psi_kd_reason + 3, 1);) }
    // the walk's stack, entry i: the query's LDS rows, or (SPW == 2) the query's 8 rows bytes of gstk as uniform base + 32-bit lane offset
    // (search_shape.h; obase = b * n)
    char *const gbase = SPW == 2 ? (char *)gstk + obase * (size_t)rows * 8 : nullptr;
    auto ref_at = [&](int i) -> int * {
        if constexpr (SPW == 2) return (int *)(gbase + psi_search_stack_entry(jq, rows, 0, i));
        else return stk_n + i;
    };
    auto dist_at = [&](int i) -> float * {
        if constexpr (SPW == 2) return (float *)(gbase + psi_search_stack_entry(jq, rows, 1, i));
        else return stk_d + i;
    };
    while (true) {
        while (!have && sp > 0) {                             // pop until something survives the current bound (group-uniform)
            --sp;
            cur = kd_stack_ld<SPW>(ref_at(sp));
            curd = kd_stack_ld<SPW>(dist_at(sp));
            kd_stack_popped<SPW>();
            have = !(curd * 0.999999f > best);
        }
        if (!have) break;
        PSI_KD_STAT(nvis += 1;)
        if (cur >= 0) {
            float dc[CPL];
            int ref[CPL];
            kd_key km = ~0ull;
#pragma unroll
            for (int u = 0; u < CPL; u++) {
                const float4 *cp = (const float4 *)(T.nodes + cur) + 2 * (c + u * LPQ);
                const float4 lo = cp[0], hi = cp[1];          // {mnx,mny,mnz,mxx} {mxy,mxz,ref,-}
                float dx = fmaxf(fmaxf(lo.x - qx, qx - lo.w), 0.0f);
                float dy = fmaxf(fmaxf(lo.y - qy, qy - hi.x), 0.0f);
                float dz = fmaxf(fmaxf(lo.z - qz, qz - hi.y), 0.0f);
                dc[u] = dx * dx + dy * dy + dz * dz;          // +inf for EMPTY children
                ref[u] = __float_as_int(hi.z);
                const kd_key k = kd_pack(dc[u], c + u * LPQ);
                km = k < km ? k : km;
                // two lanes per query: the lane's four child boxes in two rounds of two — all eight registers quads at once are what put the
                // fused launch (fit.hip) over its register budget, and the walk is the rare path there
                if (CPL > 2 && u == CPL / 2 - 1) __builtin_amdgcn_sched_barrier(0);
            }
            km = group_min<LPQ>(km);
            const float dmin = kd_key_d(km);
            const int cmin = kd_key_i(km);
            // push the other children that can still matter; descend into the nearest without a stack round trip
#pragma unroll
            for (int u = 0; u < CPL; u++) {
                const bool push = (c + u * LPQ) != cmin && dc[u] * 0.999999f <= best;
                const unsigned gm = (unsigned)(__ballot(push) >> gshift) & ((1u << LPQ) - 1u);
                if (push) {
                    const int pos = sp + __popc(gm & ((1u << c) - 1u));
                    kd_stack_st<SPW>(ref_at(pos), ref[u]);
                    kd_stack_st<SPW>(dist_at(pos), dc[u]);
                }
                sp += __popc(gm);
            }
            kd_stack_pushed<SPW>();
            int rsel = ref[0];
#pragma unroll
            for (int u = 1; u < CPL; u++) rsel = (cmin / LPQ == u) ? ref[u] : rsel;
            cur = __shfl(rsel, (tid & 63 & ~(LPQ - 1)) | (cmin & (LPQ - 1)), 64);
            curd = dmin;
            have = dmin < INFINITY && !(dmin * 0.999999f > best);
        }
        if (have && cur < 0) {                                // leaf — possibly the one just stepped into
            kd_key k = ~0ull;
#pragma unroll
            for (int u = 0; u < CPL; u++) {
                const float4 p = T.pts[(size_t)(-cur - 1) * LEAF + c + u * LPQ];
                float x2 = p.x - qx, y2 = p.y - qy, z2 = p.z - qz;
                const float d = PSI_SQ3(x2, y2, z2);
                const kd_key ku = kd_pack(d, __float_as_int(p.w));
                k = ku < k ? ku : k;
            }
            k = group_min<LPQ>(k);
            bestk = k < bestk ? k : bestk;
            best = kd_key_d(bestk);
            have = false;
        }
    }
    PSI_KD_STAT(if (blockIdx.x < 8192 && psi_dbg_sstop == 10) {
        int *st_ = psi_kd_stat + 4 * blockIdx.x;
        if (c == 0 && nvis > 0) { atomicAdd(st_ + 0, 1); atomicAdd(st_ + 2, nvis); }
        atomicMax(st_ + 1, nvis);
        atomicMax(st_ + 3, ngp);
    })
    float fval = 0.0f;
    PSI_KD_MARK(3);
    if (active && c == 0) {
        const int besti = kd_key_i(bestk);
        if constexpr (LPQ == 2) {
            if (dist) kd_slot(dist, obase, jq, 1, 0) = best;
            if (idx) kd_slot(idx, obase, jq, 1, 0) = besti;
            if (hint) kd_slot(hint, obase, jq, 1, 0) = besti;
        } else {
            if (dist) dist[o] = best;
            if (idx) idx[o] = besti;
            if (hint) hint[o] = besti;
        }
        if (CONTACT) {
            float4 w = hp;                                    // the winner's coordinates (same values the scan used): the warm candidate's
            if (besti != h) w = T.opts[besti];                // are here already — a load only when the winner changed since the last call
            float sq = sqrtf(best + 1e-4f);
            float den = sq + cconst;
            fval = sq / den;
            float gg = gscale * (cconst / (2.0f * sq * den * den)) * 2.0f;
            const float gx = gg * (qx - w.x), gy = gg * (qy - w.y), gz = gg * (qz - w.z);
            if (LPQ == 2 && gq) {
                kd_slot(gq, obase, jq, 3, 0) = gx;
                kd_slot(gq, obase, jq, 3, 1) = gy;
                kd_slot(gq, obase, jq, 3, 2) = gz;
            } else if (gq) {
                gq[o * 3 + 0] = gx;
                gq[o * 3 + 1] = gy;
                gq[o * 3 + 2] = gz;
            }
            qsrc.contact_post(o, gx, gy, gz);
        }
    }
    return fval;
}

// body of the search for workgroup (bx, b) of an (nbx, B) grid; smem_i: kd_qpb(LPQ) * rows * 8 bytes of LDS for the traversal stacks
// (launched with QBLK threads for every LPQ; the threads beyond kd_threads(LPQ) — waves 2 and 3 with 2 lanes per query — leave before the
// source's first load: the workgroup's barriers count the waves that are left)
// SPW = 2 (LPQ = 2 only): all four waves carry queries — waves 0-1 slice 2 bx, waves 2-3 slice 2 bx + 1 of body b, nbx counting SLICES; the
// second pair of a body's last workgroup leaves behind the source's workgroup phase when the slice count is odd.  smem_i then holds
// kd_qpb(LPQ) * rows * 8 bytes for 128 queries (the column lists), gstk the walk's stacks: B * n * rows * 8 bytes.
template <int LPQ, bool CONTACT, bool MULTI, int SPW, class QSrc>
__device__ __forceinline__ void kd_query_body(KdDev T0, QSrc qsrc, int n, float *__restrict__ dist, int *__restrict__ idx, float cconst,
                                              float gscale, float *__restrict__ gq, float *__restrict__ fpart, int *__restrict__ hint,
                                              int rows, const KdDev *__restrict__ tab, const int *__restrict__ slot, int bx, int b, int nbx,
                                              int *smem_i, int *__restrict__ gstk = nullptr)
{
    static_assert(SPW == 1 || (SPW == 2 && 2 * kd_threads(LPQ) == QBLK), "two slices per workgroup: two wave pairs of 64 queries");
    constexpr int QPB = SPW * kd_qpb(LPQ);
    const int tid = threadIdx.x;
    if (SPW == 1 && kd_threads(LPQ) < QBLK && tid >= kd_threads(LPQ)) return;
    // my pair (uniform over a wave: a scalar) and my slice of the body (== bx when SPW == 1)
    const int pr = SPW == 2 ? __builtin_amdgcn_readfirstlane(psi_sum_wg_pair(LPQ, SPW, tid)) : 0;
    const int sl = psi_sum_wg_slice(SPW, bx, pr);
    const int c = tid & (LPQ - 1), g = tid / LPQ;
    const KdDev T = MULTI ? tab[slot[b]] : T0;
    const int j = bx * QPB + g;
    const bool active = j < n;
    const size_t o = (size_t)b * n + (active ? j : 0);
    float qx = 0, qy = 0, qz = 0;
    float4 hp;
    // round 1: everything that depends on the slot only (the source's own loads, last iteration's winner); round 2: what those name (the
    // winner's coordinates, the source's second-level loads) — then the workgroup phase and the arithmetic
    qsrc.issue(b, active ? j : 0, active);
    const size_t obase = (size_t)b * n;
    const int jq = active ? j : 0;
    const int h0 = LPQ == 2 ? ((active && hint) ? kd_slot(hint, obase, jq, 1, 0) : -1) : kd_warm_hint(hint, active, o);
    qsrc.fetch(b);
    const int h = kd_warm_candidate(T, h0, hp);
    qsrc.prepare(b);
    if (SPW == 2 && sl >= nbx) return;                           // odd slice count: no second slice (the barriers from here on count the live waves)
    qsrc.point(b, active ? j : 0, c, qx, qy, qz);                // every lane of the group ends up with the same point
    PSI_SSTOP(4);                                                // (dev: differential timing — the query source alone)
    PSI_KD_MARK(0);
    const float fval = kd_query_round<LPQ, kd_rpl(LPQ), CONTACT, SPW>(T, qsrc, qx, qy, qz, active, o, dist, idx, cconst, gscale, gq, hint, rows, smem_i, h, hp, obase, jq, gstk);
    if (CONTACT) {
        kd_block_fsum<LPQ, SPW>(fval, fpart + (size_t)b * nbx + sl, pr);
        qsrc.contact_finish(b, sl, nbx);
    }
}

static inline size_t kd_lds_bytes(int lpq, int rows) { return (size_t)kd_qpb(lpq) * rows * 8; }

}  // namespace psikd

struct psi_nn_index;
psikd::KdDev psi_nn_index_dev(const psi_nn_index *ix);          // nnindex.hip
// psi_nn_index_contact (psi_internal.h) over a set of scenes: body b is searched in tab[slot[b]] (both device), rows = the set's largest stack
int psi_nn_index_contact_set(const psikd::KdDev *tab, const int *slot, int rows, const float *verts, long vstride, const int *vid, int B, int n,
                             float cconst, float gscale, float *gq, float *fpart, int *hint, hipStream_t st);
