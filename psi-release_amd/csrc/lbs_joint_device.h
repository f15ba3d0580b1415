// Device bodies of the joint-side half of the LBS backward — skin_bwd_A (gA = W^T (g_local (x) [v_posed; 1]), a contraction over
// vertices) and blend_bwd (g_feat = g_vposed dirs^T, a contraction over columns with the blend-shape matrix streamed again) — as
// functions of their OPERANDS, so that two kernels can share them: bwd_joint_kernel (lbs.hip: the operator's own backward, the model's
// vertices) and the fused fitting engine's fit_bwd_joint_kernel (fit.hip), which runs the same bodies over two classes of "vertices"
// in one grid: the model's 10475 (carrying the UNSCALED penetration gradient) and the engine's n_c contact slots (carrying the contact
// gradient) — everything behind dL/dverts is linear in it (lbs.py:108-116 backward), so the two parts travel side by side as extra
// slices of the same split contractions and meet, with the 1 / N of the penetration term (fitting_proxe.py:155-158), in the reduction.
#pragma once
#include "lbs_device.h"
#include "pen_steps.h"
#include "ska_plan.h"

#ifndef PSI_SKA_MARK
#define PSI_SKA_MARK(k)
#endif

// ------------------------------------------------------------------------------------------------
// skinning backward, joint part (MFMA): gA[b][j][r*4+s] = sum_v W[v][j] * g_local[b][v][r] * [v_posed;1][s]
// ------------------------------------------------------------------------------------------------
// One workgroup = one 256-vertex slice x NBODY bodies; it is ONE product  D[64 joints][12 NBODY] = W^T[64][256] P[256][12 NBODY]  with
// P[v][12 bb + 4 r + s] = g_local[bb][v][r] [v_posed[bb][v]; 1][s]: the 12 (r, s) entries of consecutive bodies are packed side by side, so
// the 16-wide MFMA tiles carry no padding (a tile per body carried four zero columns: a quarter of the instructions).  Wave w owns joint
// tile w (joints 16 w .. 16 w + 15) for the WHOLE slice and all column tiles: nothing to reduce across waves — the previous form split
// the slice's vertices over the waves and met in LDS behind two barriers per body, which behind the blend_bwd stream's MFMA bursts (the
// two share the launch and each SIMD) cost 2.5 us per body (workgroup timeline: operands staged at 5.6 us, end at 22 — later than the
// stream itself, profiles/r04_timeline_bwd_joint.txt).
//   A operand: lane (li, lk) supplies joint 16 w + li, vertex 64 lk + st in step st: 64 consecutive floats of its weight row, a quad
// (16 B) per four steps, each used for every column tile.  B operand: the same vertex, column 16 nt + li: a product of two LDS values; the
// staged operands are kept component-major ([body][component][vertex], 64-vertex runs padded by 4) so that the four steps of a quad
// are ONE 16-byte LDS read each for g_local and v_posed.
constexpr int SKA_NBODY = 8;
constexpr int SKA_ROW = 256 + 16;          // floats per staged (body, component) row: vertex v sits at v + 4 (v / 64)
constexpr int SKA_MAXT = (12 * SKA_NBODY + 15) / 16;
constexpr int SKA_SMEM_F4 = SKA_NBODY * 2 * 3 * SKA_ROW / 4;      // LDS of one skin_bwd_A workgroup, in 16-byte units

// operands of ONE 256-vertex slice
struct PsiSkaSlice {
    const float *wtt;          // the slice's four wave tiles of the tiled weights: [4][PSI_JP][64]
    const float *gl, *vp;      // g_local / posed vertices of the slice's 256 vertices (768 floats), body b at + b * row_stride
    size_t row_stride;
    float *part;               // [B][PSI_JP][16]: this slice's partial joint-transform gradients
};

// index of the k-th set bit of m (k < popcount(m))
__device__ __forceinline__ int psi_nth_bit(unsigned m, int k)
{
    for (int i = 0; i < k; i++) m &= m - 1u;
    return __builtin_ctz(m);
}

// NT: column tiles of the workgroup, (12 nb + 15) / 16 for its nb bodies — a compile-time count keeps the 16 quads straight-line code with
// all weight quads in registers (the spare columns of the last tile repeat the last column)
// live: bit i set = body b0 + i is one of the workgroup's bodies (uniform; at most SKA_NBODY bits).  The set bodies' 12 columns each are
// packed side by side in the order of their bits — a column is its own sum over the vertices, whichever columns share its tile
// (tests/test_bwd_joint_schedule_gpu.py) — so a workgroup that leaves bodies out (fit.hip: their rows are zero) runs fewer tiles
template <int NT>
__device__ __forceinline__ void skin_bwd_A_body(const PsiSkaSlice &o, int b0, unsigned live, psi_f4 *smem)
{
    typedef psi_f4 f4;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int nb = __builtin_popcount(live);
    const int ncol = 12 * nb;
    // my weight row: joint 16 w + li, vertices 64 lk .. 64 lk + 63 of the slice — all 16 quads requested now (behind the stream's traffic
    // a load takes ~2 us: requested two quads ahead of their use, they made every quad wait, 1 us per quad)
    f4 wa[16];
    {
        // from the wave-tiled copy ([Vpad/64][64 joints][64 vertices]: the same 256 contiguous bytes per lane)
        const f4 *wr = (const f4 *)(o.wtt + ((size_t)lk * PSI_JP + (w * 16 + li)) * 64);
#pragma unroll
        for (int q = 0; q < 16; q++) wa[q] = wr[q];
    }
    // ALL bodies' operands of this slice are requested up front, coalesced (768 consecutive floats of g_local and of v_posed per body: one
    // 16-byte load each for threads 0..191), and parked in LDS component-major
    float *sG = (float *)smem;                                  // [SKA_NBODY][3][SKA_ROW]
    float *sP = sG + SKA_NBODY * 3 * SKA_ROW;                   // [SKA_NBODY][3][SKA_ROW]
    {
        f4 og[SKA_NBODY], op[SKA_NBODY];
        const int t4 = threadIdx.x;
        unsigned rest = live;
#pragma unroll
        for (int bb = 0; bb < SKA_NBODY; bb++) {
            if (bb < nb && t4 < 192) {
                const size_t row = (size_t)(b0 + __builtin_ctz(rest)) * o.row_stride;
                og[bb] = *(const f4 *)(o.gl + row + t4 * 4);
                op[bb] = *(const f4 *)(o.vp + row + t4 * 4);
            }
            rest &= rest - 1u;
        }
#pragma unroll
        for (int bb = 0; bb < SKA_NBODY; bb++)
            if (bb < nb && t4 < 192) {
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int i = t4 * 4 + e, v = i / 3, comp = i - 3 * v;
                    const int pos = (bb * 3 + comp) * SKA_ROW + v + 4 * (v >> 6);
                    sG[pos] = og[bb][e];
                    sP[pos] = op[bb][e];
                }
            }
    }
    __syncthreads();
    PSI_SKA_MARK(0);
    // my columns: tile nt -> column 16 nt + li = 12 bb + 4 r + s
    int goff[NT], poff[NT];                                     // float offsets of my (body, r) / (body, s) rows + my 64-vertex run; poff < 0: s == 3
    f4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++) {
        const int c = min(16 * nt + li, ncol - 1);             // (columns past the last body repeat the last one; they are not stored)
        const int bb = c / 12, rs = c - 12 * bb, r = rs >> 2, sx = rs & 3;
        goff[nt] = (bb * 3 + r) * SKA_ROW + lk * 68;
        poff[nt] = sx < 3 ? (bb * 3 + sx) * SKA_ROW + lk * 68 : -1;
        acc[nt] = (f4){0, 0, 0, 0};
    }
    // (requesting quad q + 1's LDS operands before quad q's MFMAs — a denser MFMA stream of this wave — measured SLOWER, 23.1 against 21.8 us:
    // the stream wave on the same SIMD then waits longer for the pipe, and the launch ends when the later of the two kinds does)
#pragma unroll
    for (int q = 0; q < 16; q++) {
        f4 bop[NT];
#pragma unroll
        for (int nt = 0; nt < NT; nt++) {
            const f4 g4 = *(const f4 *)(sG + goff[nt] + 4 * q);
            const f4 p4 = *(const f4 *)(sP + max(poff[nt], 0) + 4 * q);
            bop[nt] = poff[nt] >= 0 ? g4 * p4 : g4;
        }
#pragma unroll
        for (int e = 0; e < 4; e++)
#pragma unroll
            for (int nt = 0; nt < NT; nt++) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[q][e], bop[nt][e], acc[nt], 0, 0, 0);
        if (q == 0) PSI_SKA_MARK(1);
        __builtin_amdgcn_sched_barrier(0);                      // (the scheduler otherwise hoists every quad's LDS reads to the top and spills)
    }
    // D[row = 4 lk + e -> joint 16 w + 4 lk + e][col = li -> column 16 nt + li]
#pragma unroll
    for (int nt = 0; nt < NT; nt++) {
        const int c = 16 * nt + li;
        if (c < ncol) {
            const int bb = c / 12, rs = c - 12 * bb;
            float *po = o.part + (((size_t)(b0 + psi_nth_bit(live, bb))) * PSI_JP + w * 16 + lk * 4) * 16 + rs;
#pragma unroll
            for (int e = 0; e < 4; e++) po[e * 16] = acc[nt][e];
        }
    }
}

// the same, column-tile count chosen at run time (12 columns per set bit of `live`, at least one)
__device__ __forceinline__ void skin_bwd_A_dispatch_live(const PsiSkaSlice &o, int b0, unsigned live, psi_f4 *smem)
{
    switch ((12 * __builtin_popcount(live) + 15) >> 4) {
    case 1: skin_bwd_A_body<1>(o, b0, live, smem); break;
    case 2: skin_bwd_A_body<2>(o, b0, live, smem); break;
    case 3: skin_bwd_A_body<3>(o, b0, live, smem); break;
    case 4: skin_bwd_A_body<4>(o, b0, live, smem); break;
    case 5: skin_bwd_A_body<5>(o, b0, live, smem); break;
    default: skin_bwd_A_body<SKA_MAXT>(o, b0, live, smem); break;
    }
}
// all of the workgroup's bodies b0 .. min(b0 + nbody, B) - 1
__device__ __forceinline__ void skin_bwd_A_dispatch(const PsiSkaSlice &o, int B, int b0, int nbody, psi_f4 *smem)
{
    skin_bwd_A_dispatch_live(o, b0, (1u << min(nbody, B - b0)) - 1u, smem);
}

// ---- rows that a penetration mask proves zero (the fused fitting engine, fit.hip: FitDev::penmask [B][pm_words], bit = vertex with sdf < 0;
// every other vertex's rows of g_local / g_vposed are exact zeros).  A body whose mask words of the slice are clear contributes sums of
// products with a zero factor to accumulators that start at +0: the workgroup stores the +0 itself and runs the contraction over the
// other bodies only (none: no weights, no operands, no MFMAs).  Once a fit is under way a slice that is live at all is live in one or two
// bodies: one or two column tiles where all of the workgroup's bodies are six, and such a workgroup is what the launch then waits for.
// Each wave looks for itself (the same words, nobody writes them in this launch: the same answer in every wave, no barrier).
// -> bit i set = body b0 + i has a set bit in the slice's four words
__device__ __forceinline__ unsigned psi_pen_slice_live(const unsigned long long *penmask, int pm_words, int slice, int B, int b0, int nbody)
{
    static_assert(4 * SKA_NBODY <= 64, "one lane per (body, word)");
    const int lane = threadIdx.x & 63, nb = min(nbody, B - b0);
    unsigned long long any = 0ull;
    if (lane < 4 * nb) any = penmask[(size_t)(b0 + (lane >> 2)) * pm_words + 4 * slice + (lane & 3)];
    unsigned long long x = __builtin_amdgcn_ballot_w64(any != 0ull);
    x |= x >> 1;
    x |= x >> 2;                                                // bit 4 i: any of body i's four words
    unsigned live = 0u;
#pragma unroll
    for (int i = 0; i < SKA_NBODY; i++) live |= (unsigned)((x >> (4 * i)) & 1ull) << i;
    return live;
}
// +0 in exactly the elements skin_bwd_A_body would store for the bodies b0 + i, i a set bit of `dead`: 64 joints x the 12 (r, s) entries each
__device__ __forceinline__ void skin_bwd_A_zero(const PsiSkaSlice &o, int b0, unsigned dead)
{
    for (; dead != 0u; dead &= dead - 1u) {
        float *pb = o.part + (size_t)(b0 + __builtin_ctz(dead)) * PSI_JP * 16;
        for (int r = threadIdx.x; r < 64 * 12; r += blockDim.x) {
            const int j = r / 12, rs = r - 12 * j;
            pb[j * 16 + rs] = 0.0f;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// blend backward (MFMA): g_feat[b][k] = sum_n g_vp[b][n] dirs[k][n]
// Rounds 3-6 ran this product on the fp32 MFMA (v_mfma_f32_16x16x4_f32 over a 16-column-tiled fp32 copy of the matrix; workgroup = 4 waves
// sharing a 64-row k group and an n-slice, wave w taking n-steps w, w + 4, ..., LDS reduce).  What was learnt on that form and still holds for
// the one below: ONE step of operands in flight per wave serves the launch best WHERE LIVE skin_bwd_A WAVES SHARE THE SIMDs' MATRIX PIPE
// (the operator's own backward, the dense iterations of a fit: 22.0 us at 1 step, 22.6 / 23.9 / 25.1 at 2 / 3 / 4), and the step loop as
// straight-line code with a register ring does not pay (profiles/r06_ab_bwd_joint_pipeline.txt).  Hence PF is a parameter: the fitting
// engine's contact class, which in a sparse iteration is what the launch waits for, keeps two steps in flight (-1.7 us; four measured the
// same, two in the model class gained nothing sparse and lost 0.2-0.5 us dense: profiles/bwd_joint_chains_ab.txt).
// The product on the fp16 matrix pipe at fp32-class accuracy (round 6; what lbs.hip's blend_fwd_h_kernel does for the forward product):
// the fp32 MFMA runs at 1/16 of the fp16 rate, and the stream workgroups' 608 fp32 MFMAs per SIMD were what this launch waited for beside its
// skin_bwd_A waves (with a quarter of them: 25.3 -> 21.2 us, profiles/r06_ab_blend_fp16x3.txt).  The matrix arrives as TWO fp16 parts per
// entry (hi = fp16(x), lo = fp16((x - hi) 2^11), x = value * a power of two: 22 mantissa bits in the same 4 bytes) in MFMA operand order
//   dirs_bh [n-step of 16][Kpad/32 k-tiles][part][n half][32 k][8 n]        (a wave's load of one part of one (step, k-tile) is 1 KB contiguous);
// the gradient rows stay fp32 in memory and are split by the wave that loads them, with the scale 2^s that puts the largest entry of THAT
// BODY's rows into [2^13, 2^14) — fp16 cannot overflow, entries down to 1e-9 of the body's largest keep 22 bits, smaller ones an absolute
// error below 1e-12 of it.  The B operand's column is the body, and the lane that supplies column li also holds output column li, so the
// scale and its inverse are per-lane values, one per body tile: a body's accuracy does not depend on the other bodies of the batch, and a
// body with an Inf entry (scale clamped to 2^-100) or one a trillion times larger than the rest leaves their products bit for bit as they
// were (the first form of this product took one scale per call, and such a body underflowed every other body's rows to zero in fp16).  The
// body's largest entry arrives as the bit patterns of its slots ([B][gv_slots], integer maxima of the producers: exact, order-independent),
// combined here.  A product is hi*hi + (hi*lo + lo*hi) 2^-11 in two fp32 accumulators: 3 MFMAs of 32 cycles per 32 x 32 x 16 block
// instead of 16.
// Workgroup = 4 waves sharing a 64-row k group (two 32-row k-tiles) and an n-slice; wave w takes n-steps w, w + 4, ...; LDS reduce.
// ------------------------------------------------------------------------------------------------
typedef _Float16 psi_h8 __attribute__((ext_vector_type(8)));
typedef float psi_f16v __attribute__((ext_vector_type(16)));
typedef unsigned int psi_u4 __attribute__((ext_vector_type(4)));
struct PsiBlendBwdColsH {
    const float *dirs_bh;      // the class's columns, two fp16 parts per entry (layout above)
    const float *g_vp;         // [B][row_stride] fp32
    size_t row_stride;
    int Kpad, total_steps;
    const unsigned *gvbits;    // [B][gv_slots] bit patterns of maxima of |row entry|: the largest of a body's slots is the largest entry of its rows
    int gv_slots;              // slots per body (>= 1)
    float dsc_inv;             // 1 / matrix scale (the rows' own scale 2^s is applied per body)
    // != nullptr: [B][pm_words] bit v % 64 of word v / 64 clear = the three columns of vertex v are exact zeros in that body's row (fit.hip:
    // FitDev::penmask).  A step whose vertices are clear in every body of the workgroup is not loaded and not multiplied: it would add
    // products with a zero factor.  nullptr: every step is walked
    const unsigned long long *penmask;
    int pm_words;
};
constexpr int PSI_BWH_PM_WORDS = 16;      // mask words per body a stream workgroup looks at (a slice of up to ~170 steps; a longer one is walked whole)
// scale for rows whose largest |entry| has the bit pattern `bits` (0: nothing stored this iteration)
__device__ __forceinline__ float psi_fp16_row_scale(unsigned bits)
{
    int E = (int)((bits >> 23) & 0xffu);                 // largest entry in [2^(E-127), 2^(E-126))
    if (bits == 0u) E = 140;                             // (any scale: every entry is zero)
    int se = 267 - E;                                    // biased exponent of 2^(13 - (E - 127))
    se = se < 27 ? 27 : (se > 227 ? 227 : se);           // |exponent| <= 100: the reciprocal stays a normal number
    return __uint_as_float((unsigned)se << 23);
}
template <int MTB>
constexpr int psi_blend_bwd_h_smem_f4() { return 4 * 2 * MTB * 4 * 64; }

// PF: steps of operands a wave keeps in flight (below)
template <int MTB, int PF>
__device__ __forceinline__ void blend_bwd_h_body(const PsiBlendBwdColsH &o, int B, int s_begin, int s_end, float *__restrict__ part, int kgroup,
                                                 int bgroup, psi_f4 *smem)
{
    typedef psi_f4 f4;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int li = lane & 31, kh = lane >> 5;
    const int KT = o.Kpad / 32;
    const int k0 = kgroup * 64;
    const int b0 = bgroup * 32 * MTB;
    s_end = min(s_end, o.total_steps);
    psi_f16v acc[2][MTB][2];                             // [k-tile][body tile][hi*hi | hi*lo + lo*hi]
#pragma unroll
    for (int kt = 0; kt < 2; kt++)
#pragma unroll
        for (int t = 0; t < MTB; t++)
#pragma unroll
            for (int c = 0; c < 2; c++)
#pragma unroll
                for (int i = 0; i < 16; i++) acc[kt][t][c][i] = 0.0f;
    const float *grow[MTB];
#pragma unroll
    for (int t = 0; t < MTB; t++) grow[t] = o.g_vp + (size_t)min(b0 + t * 32 + li, B - 1) * o.row_stride + 8 * kh;
    const char *dbase = (const char *)o.dirs_bh + ((size_t)(2 * kgroup) * 2) * 1024 + (size_t)(kh * 32 + li) * 16;
    // the mask words of my columns, lane = body, wave w the words w, w + 4, ...: requested together with the scales' slots below
    __shared__ unsigned long long s_pm[PSI_BWH_PM_WORDS];
    static_assert(32 * MTB <= 64, "the mask words are loaded one body per lane: a body group is at most one wave wide");
    int pw0 = 0, pnw = 0;
    bool use_pm = o.penmask != nullptr && s_begin < s_end;       // (uniform over the workgroup)
    if (use_pm) {
        psi_pen_step_words(s_begin, s_end, pw0, pnw);
        pnw = max(min(pnw, o.pm_words - pw0), 0);                // (steps past the last word are padding columns: clear)
        use_pm = pnw <= PSI_BWH_PM_WORDS;
    }
    unsigned long long mw[PSI_BWH_PM_WORDS / 4];
    if (use_pm) {
        const int nb = min(32 * MTB, B - b0);
#pragma unroll
        for (int k = 0; k < PSI_BWH_PM_WORDS / 4; k++)
            mw[k] = (4 * k + w < pnw && lane < nb) ? o.penmask[(size_t)(b0 + lane) * o.pm_words + pw0 + 4 * k + w] : 0ull;
    }
    // the scale of body tile t's column li (body b0 + 32 t + li) and the inverse of both scales for the same output column: lanes li and
    // li + 32 hold the same body and split its slots between them
    float gsc[MTB], us[MTB];
#pragma unroll
    for (int t = 0; t < MTB; t++) {
        const unsigned *sl = o.gvbits + (size_t)min(b0 + t * 32 + li, B - 1) * o.gv_slots;
        // (a lane's up to eight slots requested together instead of one after the other: no gain, profiles/bwd_joint_chains_ab.txt)
        unsigned cbits = 0u;
        for (int p = kh; p < o.gv_slots; p += 2) cbits = max(cbits, sl[p]);
        cbits = max(cbits, (unsigned)__shfl_xor((int)cbits, 32, 64));
        gsc[t] = psi_fp16_row_scale(cbits);
        us[t] = o.dsc_inv / gsc[t];
    }
    // PF steps' operands (PF x (4 + 2 MTB) 16-byte loads per lane) are requested before the first of them is split and multiplied, in
    // the order of the steps: the depth changes no sum.  A last group with fewer than PF live steps requests its first step again for the
    // missing ones (has[p] false: loaded, not multiplied)
    static_assert(PF >= 1 && PF <= 4, "8 steps in flight spill (256 VGPRs and scratch); 4 do at MTB = 2");
    if (use_pm) {
        // OR over the bodies (almost always nothing to OR: one ballot), one word per wave and round -> LDS -> every wave
#pragma unroll
        for (int k = 0; k < PSI_BWH_PM_WORDS / 4; k++) {
            unsigned long long r = mw[k];
            if (__builtin_amdgcn_ballot_w64(r != 0ull) != 0ull) {
#pragma unroll
                for (int o2 = 32; o2 > 0; o2 >>= 1) r |= __shfl_xor(r, o2, 64);
            }
            if (lane == 0 && 4 * k + w < pnw) s_pm[4 * k + w] = r;
        }
        __syncthreads();
    }
    // my steps s_begin + w + 4 i, i < n_i, 64 at a time: lane i decides step i, the wave walks the set bits in increasing order
    const int n_i = s_end - s_begin > w ? (s_end - s_begin - w + 3) >> 2 : 0;
    for (int i0 = 0; i0 < n_i; i0 += 64) {
        bool mine = i0 + lane < n_i;
        if (use_pm && mine) mine = psi_pen_step_live(s_pm, pw0, pnw, s_begin + w + 4 * (i0 + lane));
        unsigned long long todo = __builtin_amdgcn_ballot_w64(mine);
        while (todo != 0ull) {
            psi_u4 d[PF][2][2];
            f4 g[PF][MTB][2];
            bool has[PF];
#pragma unroll
            for (int p = 0; p < PF; p++) {
                has[p] = todo != 0ull;
                const int st = s_begin + w + 4 * (i0 + (has[p] ? (int)__builtin_ctzll(todo) : 0));
                todo &= todo - 1ull;
#pragma unroll
                for (int kt = 0; kt < 2; kt++)
#pragma unroll
                    for (int q = 0; q < 2; q++) d[p][kt][q] = *(const psi_u4 *)(dbase + ((size_t)st * KT * 2 + (size_t)(kt * 2 + q)) * 1024);
#pragma unroll
                for (int t = 0; t < MTB; t++) {
                    g[p][t][0] = *(const f4 *)(grow[t] + (size_t)st * 16);
                    g[p][t][1] = *(const f4 *)(grow[t] + (size_t)st * 16 + 4);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int p = 0; p < PF; p++) {
                if (has[p]) {
#pragma unroll
                    for (int t = 0; t < MTB; t++) {
                        psi_h8 gh, gl;
#pragma unroll
                        for (int e = 0; e < 8; e++) {
                            const float x = g[p][t][e >> 2][e & 3] * gsc[t];
                            const _Float16 hi = (_Float16)x;
                            gh[e] = hi;
                            gl[e] = (_Float16)((x - (float)hi) * 2048.0f);
                        }
#pragma unroll
                        for (int kt = 0; kt < 2; kt++) {
                            const psi_h8 dh = __builtin_bit_cast(psi_h8, d[p][kt][0]), dl = __builtin_bit_cast(psi_h8, d[p][kt][1]);
                            acc[kt][t][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(dh, gh, acc[kt][t][0], 0, 0, 0);
                            acc[kt][t][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(dh, gl, acc[kt][t][1], 0, 0, 0);
                            acc[kt][t][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(dl, gh, acc[kt][t][1], 0, 0, 0);
                        }
                    }
                }
            }
        }
    }
    // D[row = 8 q + 4 kh + e -> k][col = li -> body]: the two accumulators combined, the four waves' sums through LDS, wave w finishes quad q = w
    f4 (*red)[2][MTB][4][64] = (f4 (*)[2][MTB][4][64])smem;      // [wave][k-tile][body tile][row quad][lane]
#pragma unroll
    for (int kt = 0; kt < 2; kt++)
#pragma unroll
        for (int t = 0; t < MTB; t++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float us2 = us[t] * (1.0f / 2048.0f);
                f4 v;
#pragma unroll
                for (int e = 0; e < 4; e++) v[e] = __builtin_fmaf(acc[kt][t][1][4 * q + e], us2, acc[kt][t][0][4 * q + e] * us[t]);
                red[w][kt][t][q][lane] = v;
            }
    __syncthreads();
#pragma unroll
    for (int kt = 0; kt < 2; kt++)
#pragma unroll
        for (int t = 0; t < MTB; t++) {
            const f4 ov = red[0][kt][t][w][lane] + red[1][kt][t][w][lane] + red[2][kt][t][w][lane] + red[3][kt][t][w][lane];
            const int b = b0 + t * 32 + li;
            if (b < B) *(f4 *)(part + (size_t)b * o.Kpad + k0 + kt * 32 + 8 * w + 4 * kh) = ov;
        }
}

// Placement of the stream workgroups: workgroup `bid` runs on XCD bid % 8 (observed dispatch order) and every XCD has its own L2, so the
// k-groups that share an n-slice — and therefore read the same g_vposed columns — are placed on ONE XCD: that slice of g_vposed is
// fetched from memory once and served to the other k-groups from L2 (it used to be fetched by all 8 XCDs).
__device__ __forceinline__ void psi_blend_bwd_place(int bid, int kgroups, int nslices, int &kg, int &slice, int &bg)
{
    if ((nslices & 7) == 0) {
        const int xcd = bid & 7, idx = bid >> 3, spx = nslices >> 3;
        kg = idx % kgroups;
        const int t = idx / kgroups;
        slice = xcd + 8 * (t % spx);
        bg = t / spx;
    } else {
        kg = bid % kgroups;
        const int rest = bid / kgroups;
        slice = rest % nslices;
        bg = rest / nslices;
    }
}
