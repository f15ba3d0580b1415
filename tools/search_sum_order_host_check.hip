// Host check of csrc/search_sum_order.h: the partial sums of a search workgroup's contact terms for 2 and 4 lanes per query, formed with
// the very functions the kernels call (kd_block_fsum in nnindex_device.h, ContactSkinSrc::contact_finish in fit.hip), against the
// association of the 4-lane code written out term by term.  No GPU needed:
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -Xarch_host -fsanitize=address,undefined tools/search_sum_order_host_check.hip -o search_sum_order_host_check
//   search_sum_order_host_check
//
// For every n_c in 1 .. 300 and both widths, random terms (among them -0, denormals, values 10^12 apart, and all -0): a grid of
// cdiv(n_c, 64) workgroups is walked lane by lane the way the kernels place queries on lanes, each wave reduces by the halving tree
// (v[l] += v[l + d], the __shfl_down semantics: a lane whose partner lies beyond the wave adds itself) and by the pair tree (v[l] += v[l ^ d]),
// the parts go to their slots, the slots are added in order.  Every slice below cdiv(n_c, 64) must be written exactly once, none beyond it
// (the output is a heap array of exactly that many floats: the sanitizer sees a write outside), and its bits must equal the reference's.
// With 2 lanes per query the grid is walked a second time with two slices per workgroup (the wave pairs and slot tables of the header).
// Exit status 1 at the first difference.  It does not cover the kernels' own shuffles and barriers: those need the GPU tests.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../psi-release_amd/csrc/search_sum_order.h"

static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
static unsigned long long rng()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}
static unsigned bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
static float from_bits(unsigned u) { float f; memcpy(&f, &u, 4); return f; }

// kind 0: contact terms as the search produces them, s / (s + c) in [0, 1); 1: signed values over 24 binades (1e-6 .. 1e6: 10^12 apart)
// mixed with -0, +0 and denormals; 2: every term -0
static float term(int kind)
{
    const unsigned long long r = rng();
    if (kind == 2) return -0.0f;
    if (kind == 0) return (float)(r >> 40) * (1.0f / 16777216.0f);
    switch ((r >> 8) & 15) {
    case 0: return -0.0f;
    case 1: return 0.0f;
    case 2: return from_bits((unsigned)(r >> 41));                        // a denormal (23 random mantissa bits)
    case 3: return -from_bits((unsigned)(r >> 41));
    default: {
        const float mag = ldexpf(1.0f + (float)((r >> 40) & 0xffff) / 65536.0f, (int)((r >> 16) % 41) - 20);     // 2^-20 .. 2^20
        return (r & 1) ? -mag : mag;
    }
    }
}

// ---- the reference: the association of the 4-lane code, term by term ---------------------------------------------------------------
// kd_block_fsum with 4 lanes per query: the wave's 16 terms sit 4 lanes apart; shfl_down by 32, 16, 8, 4 halves them, by 2 and 1 adds the +0
// of the idle lanes; the four waves are added in order from +0
static float ref_halving(const float *q, int n, int bx)
{
    volatile float t = 0.0f;
    for (int w = 0; w < 4; w++) {
        float a[16];
        for (int i = 0; i < 16; i++) a[i] = 64 * bx + 16 * w + i < n ? q[64 * bx + 16 * w + i] : 0.0f;
        for (int d = 8; d > 0; d >>= 1)
            for (int i = 0; i < d; i++) a[i] = a[i] + a[i + d];
        volatile float p = a[0];
        p = p + 0.0f;
        p = p + 0.0f;
        t = t + p;
    }
    return t;
}
// contact_finish with 4 lanes per query (psi_wave_sum): xor 1 and xor 2 add the idle lanes' +0, then neighbours 1, 2, 4, 8 queries apart
static float ref_pairs(const float *q, int n, int bx)
{
    volatile float t = 0.0f;
    for (int w = 0; w < 4; w++) {
        float a[16];
        for (int i = 0; i < 16; i++) {
            volatile float v = 64 * bx + 16 * w + i < n ? q[64 * bx + 16 * w + i] : 0.0f;
            v = v + 0.0f;
            v = v + 0.0f;
            a[i] = v;
        }
        for (int d = 1; d < 16; d <<= 1)
            for (int i = 0; i < 16; i += 2 * d) a[i] = a[i] + a[i + d];
        t = t + a[0];
    }
    return t;
}

// ---- the kernels' form: lanes, trees and slots through search_sum_order.h -----------------------------------------------------------
struct Out {
    float *v;
    int *writes;
    int n;
};
// spw: slices per workgroup (1; or 2 with 2 lanes per query: wave pair r of workgroup bx carries slice 2 bx + r in slots 4 r .. 4 r + 3, and
// the second pair of the last workgroup has no slice when the slice count is odd)
static int run_grid(int lpq, const float *q, int n, bool pairs, Out &out, int spw = 1)
{
    const int slice_q = psi_sum_slice_queries(lpq), nslices = (n + slice_q - 1) / slice_q, nbx = (nslices + spw - 1) / spw;
    for (int bx = 0; bx < nbx; bx++) {
        float slot[8];
        int slot_writes[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int w = 0; w < spw * psi_sum_waves(lpq); w++) {
            const int pair = psi_sum_wg_pair(lpq, spw, 64 * w);
            if (psi_sum_wg_slice(spw, bx, pair) >= nslices) continue;     // (the pair retires behind the source's workgroup phase)
            float v[64];
            for (int l = 0; l < 64; l++) {
                const int tid = 64 * w + l, g = tid / lpq, c = tid % lpq, j = bx * spw * slice_q + g;
                v[l] = (c == 0 && j < n) ? q[j] : 0.0f;
            }
            const int pl = psi_sum_part_lanes(lpq);
            if (!pairs) {
                for (int d = pl / 2; d > 0; d >>= 1) {
                    float nv[64];
                    for (int l = 0; l < 64; l++) nv[l] = v[l] + (l + d < 64 ? v[l + d] : v[l]);
                    memcpy(v, nv, sizeof(v));
                }
            } else {
                for (int d = 1; d < pl; d <<= 1) {
                    float nv[64];
                    for (int l = 0; l < 64; l++) nv[l] = v[l] + v[l ^ d];
                    memcpy(v, nv, sizeof(v));
                }
            }
            for (int p = 0; p < psi_sum_parts_per_wave(lpq); p++) {
                const int s = spw == 2 ? psi_sum_wg_slot(lpq, spw, w, p) : psi_sum_slot(lpq, w, p);
                if (s < pair * psi_sum_parts(lpq) || s >= (pair + 1) * psi_sum_parts(lpq)) { printf("lpq %d: slot %d of wave %d part %d\n", lpq, s, w, p); return 1; }
                slot[s] = v[pairs ? psi_sum_last_lane(lpq, p) : psi_sum_first_lane(lpq, p)];
                slot_writes[s]++;
            }
        }
        for (int pair = 0; pair < spw; pair++) {
            const int sl = psi_sum_wg_slice(spw, bx, pair);
            if (sl >= nslices) {
                for (int s = 0; s < psi_sum_parts(lpq); s++)
                    if (slot_writes[pair * psi_sum_parts(lpq) + s]) { printf("lpq %d: a pair without a slice wrote slot %d\n", lpq, s); return 1; }
                continue;
            }
            for (int s = 0; s < psi_sum_parts(lpq); s++)
                if (slot_writes[pair * psi_sum_parts(lpq) + s] != 1) { printf("lpq %d: slot %d written %d times\n", lpq, s, slot_writes[pair * psi_sum_parts(lpq) + s]); return 1; }
            out.v[sl] = psi_sum_slots(slot + pair * psi_sum_parts(lpq), 1, lpq);       // (a write beyond the heap array: the sanitizer's)
            out.writes[sl]++;
        }
    }
    return 0;
}

static long checked = 0;

static int check(int n, int kind)
{
    std::vector<float> q(n);
    for (auto &x : q) x = term(kind);
    const int nfp = (n + 63) / 64;
    for (int lpq = 2; lpq <= 4; lpq += 2) {
        if (psi_sum_slice_queries(lpq) != 64 || psi_sum_parts(lpq) * psi_sum_part_queries(lpq) != 64 ||
            psi_sum_waves(lpq) * 64 != 64 * lpq) {
            printf("lpq %d: slice of %d queries, %d waves\n", lpq, psi_sum_slice_queries(lpq), psi_sum_waves(lpq));
            return 1;
        }
        for (int shape = 0; shape < 2 * (lpq == 2 ? 2 : 1); shape++) {      // both trees; with 2 lanes also two slices per workgroup
            const int pairs = shape & 1, spw = 1 + (shape >> 1);
            Out out = {(float *)malloc(sizeof(float) * nfp), (int *)calloc(nfp, sizeof(int)), nfp};
            int bad = run_grid(lpq, q.data(), n, pairs != 0, out, spw);
            for (int bx = 0; bx < nfp && !bad; bx++) {
                const float want = pairs ? ref_pairs(q.data(), n, bx) : ref_halving(q.data(), n, bx);
                checked++;
                if (out.writes[bx] != 1) {
                    printf("n_c %d lpq %d spw %d: slice %d written %d times\n", n, lpq, spw, bx, out.writes[bx]);
                    bad = 1;
                } else if (bits(out.v[bx]) != bits(want)) {
                    printf("n_c %d lpq %d %s tree kind %d: slice %d = %08x, the 4-lane association gives %08x\n", n, lpq, pairs ? "pair" : "halving", kind, bx,
                           bits(out.v[bx]), bits(want));
                    bad = 1;
                }
            }
            free(out.v);
            free(out.writes);
            if (bad) return 1;
        }
    }
    return 0;
}

int main()
{
    for (int n = 1; n <= 300; n++)
        for (int kind = 0; kind < 3; kind++)
            for (int rep = 0; rep < (kind == 2 ? 1 : 4); rep++)
                if (check(n, kind)) return 1;
    printf("search_sum_order: %ld slices of n_c = 1 .. 300 equal the 4-lane association bit for bit at 2 and 4 lanes per query, each written exactly once\n", checked);
    printf("search_sum_order: among them the two-slice workgroups of the 2-lane search (slots 4 r .. 4 r + 3 of wave pair r), odd slice counts included\n");
    return 0;
}
