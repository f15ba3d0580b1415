// Where the partial sums of the NN search's contact terms live, for every width of a query's lane group (nnindex_device.h: 2, 4 or 8
// lanes hold one query; lane 0 of a group carries the query's term, the group's other lanes +0).
//
// What is fixed, whatever the width: a SLICE is the 64 queries  64 bx .. 64 bx + 63  of one body (fpart[b][bx], gtc_part[(b nbx + bx) 4 + c]
// — fit_reduce_kernel and the statistics add the slices of a body in slice order), and a slice's value is
//      ((0 + P0) + P1) + P2) + P3,          P_p = the PART of queries 16 p .. 16 p + 15 of the slice
// where a part is the sum of its 16 terms over a binary tree, every term having met a +0 first (so a -0 term counts as +0).  With 4 lanes
// per query a part is one wave and the tree is the wave's reduction; with 2 lanes a wave holds TWO parts, in lanes 0-31 and 32-63, and the
// same tree runs inside each half with no step across lane 32.  (8 lanes: a development build, 8 queries per wave and 32 per slice.)
//   The two reductions of a search workgroup use two trees, and both are written in terms of the functions below:
//     kd_block_fsum (nnindex_device.h)    halving tree: v[l] += v[l + d] for d = psi_sum_part_lanes / 2 .. 1 — the steps down to the
//                                         group's width add terms 8, 4, 2, 1 queries apart, the steps below it add the +0 of the idle lanes;
//     ContactSkinSrc::contact_finish      pair tree: v[l] += v[l ^ d] for d = 1 .. psi_sum_part_lanes / 2 — the steps below the group's
//     (fit.hip)                           width add the +0s, the others pair neighbours 1, 2, 4, 8 queries apart.
//   In both the part's value ends in ONE lane of its psi_sum_part_lanes lanes, and part p of wave w is slot psi_sum_slot(lpq, w, p) of the
//   workgroup's four.  No dependencies: tools/search_sum_order_host_check.hip runs these statements on the host.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PSI_SUM_HD __host__ __device__
#else
#define PSI_SUM_HD
#endif

PSI_SUM_HD constexpr int psi_sum_part_queries(int lpq) { return lpq == 8 ? 8 : 16; }                 // terms of one part
PSI_SUM_HD constexpr int psi_sum_part_lanes(int lpq) { return psi_sum_part_queries(lpq) * lpq; }     // lanes that hold them: 32 (2 lanes per query) or 64
PSI_SUM_HD constexpr int psi_sum_parts_per_wave(int lpq) { return 64 / psi_sum_part_lanes(lpq); }    // 2 or 1
PSI_SUM_HD constexpr int psi_sum_parts(int lpq) { return 4; }                                        // parts per workgroup == slots of its LDS table
PSI_SUM_HD constexpr int psi_sum_slice_queries(int lpq) { return psi_sum_parts(lpq) * psi_sum_part_queries(lpq); }      // 64 (8 lanes: 32)
PSI_SUM_HD constexpr int psi_sum_waves(int lpq) { return psi_sum_parts(lpq) / psi_sum_parts_per_wave(lpq); }            // waves that carry queries: 2 or 4
// slot of part p (0 .. parts_per_wave - 1) of wave w: the parts in query order
PSI_SUM_HD constexpr unsigned psi_sum_slot(int lpq, unsigned w, int p) { return w * (unsigned)psi_sum_parts_per_wave(lpq) + (unsigned)p; }
// halving tree: the lane of part p in which the part's sum ends (its first)
PSI_SUM_HD constexpr int psi_sum_first_lane(int lpq, int p) { return p * psi_sum_part_lanes(lpq); }
// pair tree: the lane of part p in which the part's sum ends (its last)
PSI_SUM_HD constexpr int psi_sum_last_lane(int lpq, int p) { return (p + 1) * psi_sum_part_lanes(lpq) - 1; }
// TWO SLICES PER WORKGROUP (spw = 2; 2 lanes per query): the workgroup's four waves are two PAIRS, pair r = waves 2r, 2r + 1 carries slice
// 2 bx + r of the body with exactly the lanes, trees and slot order above, in a slot table of its own: slots 4r .. 4r + 3.  A body with an odd
// number of slices gives the second pair of its last workgroup no slice.  spw = 1: one pair (all waves), pair 0.
PSI_SUM_HD constexpr int psi_sum_wg_pair_threads(int lpq) { return psi_sum_waves(lpq) * 64; }                             // threads that carry one slice
PSI_SUM_HD constexpr int psi_sum_wg_pair(int lpq, int spw, int tid) { return spw == 2 ? tid / psi_sum_wg_pair_threads(lpq) : 0; }
PSI_SUM_HD constexpr int psi_sum_wg_slice(int spw, int bx, int pair) { return spw * bx + pair; }
// slot of part p of wave w (of the workgroup) in the workgroup's spw * psi_sum_parts slots
PSI_SUM_HD constexpr unsigned psi_sum_wg_slot(int lpq, int spw, unsigned w, int p)
{
    return spw == 2 ? (w / (unsigned)psi_sum_waves(lpq)) * (unsigned)psi_sum_parts(lpq) + psi_sum_slot(lpq, w % (unsigned)psi_sum_waves(lpq), p)
                    : psi_sum_slot(lpq, w, p);
}
// the slice's value from the workgroup's slots, in slot order from +0
PSI_SUM_HD inline float psi_sum_slots(const float *slot, int stride, int lpq)
{
    float t = 0.0f;
    for (int s = 0; s < psi_sum_parts(lpq); s++) t += slot[s * stride];
    return t;
}
