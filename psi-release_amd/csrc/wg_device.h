// Workgroup helpers of the geometry passes (csrc/body_overlap.hip, csrc/surface_crossings.hip, csrc/scene_crossings.hip), device only: a
// workgroup is WG_LANES = 256 lanes, four waves of 64 (gfx950).  Every helper must be reached by all 256 lanes: each contains a barrier.
// The sum, the box, the ordered rank, and on top of them the two passes of a count-or-emit job (wg_count, wg_emit).
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>

constexpr int WG_LANES = 256;
constexpr int WG_WAVES = WG_LANES / 64;

// The sum of v over the workgroup, in every lane.  s_w: WG_WAVES ints of LDS.
__device__ __forceinline__ int wg_sum(int v, int *s_w)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int t = threadIdx.x;
    __syncthreads();                           // s_w may still be read from an earlier call
    if ((t & 63) == 0) s_w[t >> 6] = v;
    __syncthreads();                           // the four wave sums are published
    return s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// min / max of lo / hi over the workgroup; lanes 0..2 write the six values (min xyz, max xyz) to out.  s_lo, s_hi: [WG_WAVES][3] floats of
// LDS, not reused by the caller without a barrier of its own.
__device__ __forceinline__ void wg_box(float lo[3], float hi[3], float (*s_lo)[3], float (*s_hi)[3], float *__restrict__ out)
{
    const int t = threadIdx.x;
#pragma unroll
    for (int a = 0; a < 3; a++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], o, 64));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o, 64));
        }
        if ((t & 63) == 0) {
            s_lo[t >> 6][a] = lo[a];
            s_hi[t >> 6][a] = hi[a];
        }
    }
    __syncthreads();                           // the four wave boxes are published
    if (t < 3) {
        out[t] = fminf(fminf(s_lo[0][t], s_lo[1][t]), fminf(s_lo[2][t], s_lo[3][t]));
        out[3 + t] = fmaxf(fmaxf(s_hi[0][t], s_hi[1][t]), fmaxf(s_hi[2][t], s_hi[3][t]));
    }
}

// Ordered compaction, one round of 256 items: the place of this lane's item among all items with `in` set, those of earlier rounds
// (*done of them) first, then the lanes below this one; *done grows by the round's total.  A lane without `in` gets the place its item
// would have had.  s_w: WG_WAVES ints of LDS.  The helper's barrier publishes the wave counts; the caller ends every round with a
// __syncthreads() of its own, after which s_w may be written again.
__device__ __forceinline__ int wg_rank(bool in, int *s_w, int *done)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(in);
    if (lane == 0) s_w[wave] = __popcll(m);
    __syncthreads();                           // the four wave counts are published
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < WG_WAVES; w++) {
        const int c = s_w[w];
        before += w < wave ? c : 0;
        total += c;
    }
    const int idx = *done + before + __popcll(m & ((1ull << lane) - 1ull));
    *done += total;
    return idx;
}

// The count pass of a count-or-emit job over the items 0 .. total-1 of one workgroup: how many have live(k) set, in every lane.
template <class Live>
__device__ __forceinline__ int wg_count(int total, int *s_w, Live live)
{
    int n = 0;
    for (int k = threadIdx.x; k < total; k += WG_LANES) n += live(k) ? 1 : 0;
    return wg_sum(n, s_w);
}

// The emit pass of the same job: rounds of 256 items; write(pos, k) for every live item k, pos = off + its place among the live items in
// ascending k.  want: the count pass's result for this job, limit: the rows of the output table; a place beyond either, or a pos outside
// [0, limit), is not written (the caller's scan is not trusted).
template <class Live, class Write>
__device__ __forceinline__ void wg_emit(int total, int want, long long off, long long limit, int *s_w, Live live, Write write)
{
    int done = 0;                              // live items of the rounds before this one
    for (int k0 = 0; k0 < total; k0 += WG_LANES) {
        const int k = k0 + threadIdx.x;
        const bool in = k < total && live(k);
        const int idx = wg_rank(in, s_w, &done);
        const long long pos = off + idx;
        if (in && idx < want && pos >= 0 && pos < limit) write(pos, k);
        __syncthreads();                       // s_w is read by every wave before the next round writes it
    }
}

// The box of body b = blockIdx.x over its V vertices, box [6] = min xyz, max xyz (exact: comparisons only), and the non-finite flag: *bad
// = the smallest body index with a non-finite coordinate.  The host sets *bad above every body index first (psi_reset_bad_flag in
// psi_common.h).  One workgroup per body.
__device__ __forceinline__ void wg_body_box(const float *__restrict__ verts, int V, float *__restrict__ boxes, int *__restrict__ bad)
{
    __shared__ float s_lo[WG_WAVES][3], s_hi[WG_WAVES][3];
    __shared__ int s_w[WG_WAVES];
    const int b = blockIdx.x, t = threadIdx.x;
    const float *v = verts + (size_t)b * V * 3;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int nonfinite = 0;
    for (int k = t; k < V; k += WG_LANES) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const float x = v[(size_t)k * 3 + a];
            nonfinite |= !isfinite(x);
            lo[a] = fminf(lo[a], x);
            hi[a] = fmaxf(hi[a], x);
        }
    }
    wg_box(lo, hi, s_lo, s_hi, boxes + (size_t)b * 6);
    const int any_bad = wg_sum(nonfinite, s_w);
    if (t == 0 && any_bad) atomicMin(bad, b);
}
