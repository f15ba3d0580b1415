// The launch plans of fit_bwd_joint_kernel (fit.hip), as functions without dependencies that both the host code and the kernel go through,
// so they cannot disagree; tools/fit_plan_host_check.hip walks every workgroup and every slice of every plan on the host.
//   * psi_ska_plan / psi_ska_map: the skin_bwd_A workgroups — how many bodies a workgroup of each row class takes, and which (slice, body
//     group) workgroup `bid` is.  The launcher (fit_plan_make) calls the first, the kernel the second.
//   * psi_stream_split: the stream (blend_bwd) workgroups — how the column slices are divided between the two row classes and how many
//     16-column steps a slice of each class holds.  fit_decide calls it at psi_fit_create; the kernel reads the four numbers from FitDev
//     and gives slice i of a class the steps [i * sp, (i + 1) * sp), clipped to the class's step count.
//
// skin_bwd_A.
// A workgroup is one 256-vertex slice x nbody bodies = ceil(12 nbody / 16) column tiles of the fp32 MFMA, 64 instructions per tile and wave.
// The two classes differ: the model's 41 slices are almost all skipped once the fit is under way (penetration mask), the contact slots'
// few slices never are, and their workgroups are then what the launch waits for.  So
//   * a first count nb0 is the smallest that gives at most PSI_SKA_WG_MAX workgroups over both classes — about one per CU beside its
//     stream workgroup (AT MOST one: two on a CU and the launch waits for those; fit_plan_make);
//   * the model class takes the LARGEST count with nb0's number of column tiles: the same instructions per wave, fewer workgroups
//     (B = 32: 7 -> 8 bodies, 96 columns are exactly 6 tiles, 41 x 4 = 164 workgroups instead of 205);
//   * the contact class takes the SMALLEST count that keeps the total at or below what nb0 gave for both classes (so the launch never
//     grows), again raised to the largest count with the same number of tiles (B = 32: 4 bodies, 3 tiles, 8 x 8 = 64 workgroups, 228 in
//     all — 3 bodies are 3 tiles as well, in 88 workgroups).
// An override (PSI_SKA_NBODY=n) is n bodies in both classes.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PSI_SKA_HD __host__ __device__
#else
#define PSI_SKA_HD
#endif

constexpr int PSI_SKA_WG_MAX = 256;

struct PsiSkaPlan {
    int nsv, nsv_c;               // 256-vertex slices of the model / of the contact slots
    int nb_m, nb_c;               // bodies per workgroup of each class
    int n_c, n_ska;               // workgroups of the contact class (they come first in the grid); of both classes
};

PSI_SKA_HD inline int psi_ska_cdiv(int a, int b) { return (a + b - 1) / b; }
PSI_SKA_HD inline int psi_ska_tiles(int nbody) { return (12 * nbody + 15) >> 4; }
// the largest count <= limit with nbody's number of column tiles
PSI_SKA_HD inline int psi_ska_fill_tiles(int nbody, int limit)
{
    while (nbody < limit && psi_ska_tiles(nbody + 1) == psi_ska_tiles(nbody)) nbody++;
    return nbody;
}

// B >= 1 bodies, nsv >= 1 model slices, nsv_c >= 0 contact slices, limit = SKA_NBODY, override_ = 0 or 1 .. limit
PSI_SKA_HD inline PsiSkaPlan psi_ska_plan(int B, int nsv, int nsv_c, int limit, int override_)
{
    PsiSkaPlan p;
    p.nsv = nsv;
    p.nsv_c = nsv_c;
    if (override_ >= 1 && override_ <= limit) {
        p.nb_m = p.nb_c = override_;
    } else {
        const int nsl = nsv + nsv_c;
        int nb0 = (int)(((long)B * nsl + PSI_SKA_WG_MAX - 1) / PSI_SKA_WG_MAX);
        if (nb0 < 1) nb0 = 1;
        while (nb0 < limit && (long)nsl * psi_ska_cdiv(B, nb0) > PSI_SKA_WG_MAX) nb0++;
        if (nb0 > limit) nb0 = limit;
        const long room = (long)nsl * psi_ska_cdiv(B, nb0);
        p.nb_m = psi_ska_fill_tiles(nb0, limit);
        const long n_m = (long)nsv * psi_ska_cdiv(B, p.nb_m);
        int nb_c = 1;
        while (nb_c < nb0 && n_m + (long)nsv_c * psi_ska_cdiv(B, nb_c) > room) nb_c++;
        p.nb_c = psi_ska_fill_tiles(nb_c, limit);
    }
    p.n_c = nsv_c * psi_ska_cdiv(B, p.nb_c);
    p.n_ska = p.n_c + nsv * psi_ska_cdiv(B, p.nb_m);
    return p;
}

// workgroup bid < n_ska -> slice sl of the nsv + nsv_c (model slices first, as gA_part is laid out), first body b0, bodies per workgroup
// of its class (the last group of a class may hold fewer: min(nbody, B - b0)).  The contact class's workgroups are the first of the
// grid: they are never skipped.
PSI_SKA_HD inline void psi_ska_map(const PsiSkaPlan &p, int bid, int &sl, int &b0, int &nbody)
{
    if (bid < p.n_c) {
        sl = p.nsv + bid % p.nsv_c;
        b0 = (bid / p.nsv_c) * p.nb_c;
        nbody = p.nb_c;
    } else {
        const int i = bid - p.n_c;
        sl = i % p.nsv;
        b0 = (i / p.nsv) * p.nb_m;
        nbody = p.nb_m;
    }
}

// ---- the stream workgroups' column slices.  SM >= 1 / SC >= 0 steps of 16 columns of the model / the contact class, nsn >= 1 slices for
// both.  The slices are split between the two classes so that the LONGEST slice is as short as possible (a proportional split left a
// 512-slot contact set with one 96-step slice beside 64-step ones: bwd_joint 42 us instead of 28); ties go to the smaller contact count.
// nsn_c == 0 (nsn == 1: no slice to spare): the contact class cannot be streamed, the engine runs without the fused backward.
struct PsiStreamSplit {
    int nsn_m, nsn_c;             // column slices of the model / of the contact slots
    int spm, spc;                 // steps per slice of each class (spc == 0 without contact slices)
};

PSI_SKA_HD inline PsiStreamSplit psi_stream_split(int SM, int SC, int nsn)
{
    PsiStreamSplit s;
    s.nsn_c = 0;
    for (int c = 1, best = 0x7fffffff; c < nsn; c++) {
        const int lm = psi_ska_cdiv(SM, nsn - c), lc = psi_ska_cdiv(SC, c), longest = lm > lc ? lm : lc;
        if (longest < best) { best = longest; s.nsn_c = c; }
    }
    s.nsn_m = nsn - s.nsn_c;
    s.spm = psi_ska_cdiv(SM, s.nsn_m);
    s.spc = s.nsn_c ? psi_ska_cdiv(SC, s.nsn_c) : 0;
    return s;
}
