// Host check of csrc/ska_plan.h: bodies per skin_bwd_A workgroup of fit_bwd_joint_kernel per row class, and the bid -> (slice, body group)
// map, with the very functions the launcher (fit_plan_make) and the kernel call.  No GPU needed:
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -Xarch_host -fsanitize=address,undefined tools/fit_plan_host_check.hip -o fit_plan_host_check
//   fit_plan_host_check
//
// For every B in 1 .. 128, n_c in {1, 16, 64, 256, 257, 1024, 2048, 4096}, V in {1100, 10475} and every PSI_SKA_NBODY override 0 .. 8 it
// walks every workgroup of the plan through the map and checks that each (slice, body) is covered exactly once (the coverage table is a
// heap array of exactly (nsv + nsv_c) x B entries: a slice or body outside it is a sanitizer error), that no workgroup holds more than
// SKA_NBODY bodies, that an override is obeyed, and that the plan never has more workgroups than the single-count rule it replaced gives
// for the same input; at the production shape (B = 32, V = 10475, n_c = 2048: 256 stream workgroups and the statistics workgroup) the
// grid is at most 512, one occupancy round.
// The stream workgroups' column slices (psi_stream_split) for the same V and n_c, with 64, 32 (the SMPL-X-shaped model), 21, 2 slices and
// one: every 16-column step of the model class and of the contact class lies in exactly one slice's [slice * sp, (slice + 1) * sp) clipped
// to the class's step count — the arithmetic of fit_bwd_joint_kernel — the two classes' slices are exactly the nsn the partial table is
// sized for, and the longest slice is the minimum over all splits by brute force (ties: the fewest contact slices); at the production
// shape 384 contact steps in 6 slices of 64.  With arguments `V n_c ...` it only prints the split of those shapes (Kpad = 512).
// Exit status 1 at the first failure.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../psi-release_amd/csrc/ska_plan.h"

constexpr int LIMIT = 8;          // SKA_NBODY (lbs_joint_device.h)

static int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// the rule before the classes had counts of their own: one nbody for both
static int single_count_n_ska(int B, int nsl, int override_)
{
    int nbody = cdiv((long)B * nsl, 256);
    if (nbody < 1) nbody = 1;
    while (nbody < LIMIT && (long)nsl * cdiv(B, nbody) > 256) nbody++;
    if (nbody > LIMIT) nbody = LIMIT;
    if (override_) nbody = override_;
    return nsl * cdiv(B, nbody);
}

static long plans = 0, workgroups = 0;

static int check(int B, int V, int n_c, int override_)
{
    const int nsv = cdiv(V, 256), nsv_c = cdiv(n_c, 256), nsl = nsv + nsv_c;
    const PsiSkaPlan p = psi_ska_plan(B, nsv, nsv_c, LIMIT, override_);
    plans++;
#define FAIL(...) do { printf("B %d V %d n_c %d override %d: ", B, V, n_c, override_); printf(__VA_ARGS__); printf("\n"); return 1; } while (0)
    if (p.nb_m < 1 || p.nb_m > LIMIT || p.nb_c < 1 || p.nb_c > LIMIT) FAIL("bodies per workgroup %d / %d", p.nb_m, p.nb_c);
    if (override_ && (p.nb_m != override_ || p.nb_c != override_)) FAIL("override not obeyed: %d / %d", p.nb_m, p.nb_c);
    if (p.n_ska != nsv * cdiv(B, p.nb_m) + nsv_c * cdiv(B, p.nb_c)) FAIL("n_ska %d", p.n_ska);
    const int before = single_count_n_ska(B, nsl, override_);
    if (p.n_ska > before) FAIL("n_ska %d, the single-count rule gives %d", p.n_ska, before);
    int *cover = (int *)calloc((size_t)nsl * B, sizeof(int));
    int rc = 0;
    for (int bid = 0; bid < p.n_ska && !rc; bid++) {
        int sl = -1, b0 = -1, nbody = -1;
        psi_ska_map(p, bid, sl, b0, nbody);
        workgroups++;
        if (sl < 0 || sl >= nsl || b0 < 0 || b0 >= B || nbody != (sl < nsv ? p.nb_m : p.nb_c)) {
            printf("B %d V %d n_c %d override %d: workgroup %d -> slice %d, first body %d, %d bodies\n", B, V, n_c, override_, bid, sl, b0, nbody);
            rc = 1;
            break;
        }
        const int nb = nbody < B - b0 ? nbody : B - b0;
        for (int bb = 0; bb < nb; bb++) cover[(size_t)sl * B + b0 + bb]++;
    }
    for (int i = 0; i < nsl * B && !rc; i++)
        if (cover[i] != 1) {
            printf("B %d V %d n_c %d override %d: slice %d body %d covered %d times\n", B, V, n_c, override_, i / B, i % B, cover[i]);
            rc = 1;
        }
    free(cover);
    if (rc) return 1;
    if (B == 32 && V == 10475 && n_c == 2048 && !override_) {
        const int grid = p.n_ska + 256 + 1;
        printf("B 32, V 10475, n_c 2048: %d + %d skin_bwd_A workgroups of %d / %d bodies (model / contact), grid %d\n", p.n_ska - p.n_c, p.n_c, p.nb_m,
               p.nb_c, grid);
        if (grid > 512 || p.n_ska > 256) FAIL("more than one occupancy round");
    }
#undef FAIL
    return 0;
}

static long splits = 0, steps = 0;

// every step of a class of S steps in exactly one slice's [slice * sp, (slice + 1) * sp) clipped to S (blend_bwd_h_body's own clipping); the
// table is a heap array of exactly S entries
static int check_class(const char *cls, int V, int n_c, int nsn, int S, int nslices, int sp)
{
    int *cover = (int *)calloc((size_t)(S > 0 ? S : 1), sizeof(int));
    int rc = 0;
    for (int slice = 0; slice < nslices; slice++) {
        const int lo = slice * sp, hi = (slice + 1) * sp < S ? (slice + 1) * sp : S;
        for (int s = lo; s < hi; s++) cover[s]++;
    }
    for (int s = 0; s < S && !rc; s++) {
        steps++;
        if (cover[s] != 1) {
            printf("V %d n_c %d nsn %d: %s step %d in %d slices\n", V, n_c, nsn, cls, s, cover[s]);
            rc = 1;
        }
    }
    free(cover);
    return rc;
}

// the stream workgroups' column slices (psi_stream_split) as fit_bwd_joint_kernel applies them: slice < nsn_m is the model's slice with
// steps of spm, slice - nsn_m the contact class's with steps of spc, nsn_m + nsn_c slices in all.  kpad: the model's padded feature count,
// which decides the number of slices as the workspace layout of lbs.hip does
static int check_split(int V, int n_c, int kpad)
{
    const int SM = 3 * cdiv(V, 256) * 256 / 16, SC = 3 * cdiv(n_c, 256) * 256 / 16;
    int nsn = 256 / (kpad / 64) > 0 ? 256 / (kpad / 64) : 1;
    if (nsn > SM) nsn = SM;
    const PsiStreamSplit s = psi_stream_split(SM, SC, nsn);
    splits++;
#define FAIL(...) do { printf("V %d n_c %d nsn %d: ", V, n_c, nsn); printf(__VA_ARGS__); printf("\n"); return 1; } while (0)
    if (s.nsn_m < 1 || s.nsn_c < 0 || s.nsn_m + s.nsn_c != nsn) FAIL("%d + %d slices", s.nsn_m, s.nsn_c);
    if (s.spm != cdiv(SM, s.nsn_m) || s.spc != (s.nsn_c ? cdiv(SC, s.nsn_c) : 0)) FAIL("steps per slice %d / %d", s.spm, s.spc);
    if (check_class("model", V, n_c, nsn, SM, s.nsn_m, s.spm)) return 1;
    if (s.nsn_c && check_class("contact", V, n_c, nsn, SC, s.nsn_c, s.spc)) return 1;
    // the longest slice is the shortest any split gives; among equals, the fewest contact slices
    int best = 0x7fffffff, best_c = 0;
    for (int c = 1; c < nsn; c++) {
        const int longest = cdiv(SM, nsn - c) > cdiv(SC, c) ? cdiv(SM, nsn - c) : cdiv(SC, c);
        if (longest < best) { best = longest; best_c = c; }
    }
    if (nsn > 1) {
        const int longest = s.spm > s.spc ? s.spm : s.spc;
        if (longest != best || s.nsn_c != best_c) FAIL("%d contact slices, longest %d; brute force: %d, longest %d", s.nsn_c, longest, best_c, best);
    } else if (s.nsn_c) FAIL("a contact slice out of one");
    if (V == 10475 && n_c == 2048 && kpad == 512) {
        printf("V 10475, n_c 2048: %d contact steps, %d slices of %d; %d model steps, %d slices of %d\n", SC, s.nsn_c, s.spc, SM, s.nsn_m, s.spm);
        if (SC != 384 || s.nsn_c != 6 || s.spc != 64) FAIL("not the production table");
    }
#undef FAIL
    return 0;
}

// argv: V n_c pairs — print the stream split of each shape of the SMPL-X-shaped model (Kpad = 512) and leave
int main(int argc, char **argv)
{
    if (argc > 1) {
        for (int i = 1; i + 1 < argc; i += 2) {
            const int V = atoi(argv[i]), n_c = atoi(argv[i + 1]);
            const int SM = 3 * cdiv(V, 256) * 256 / 16, SC = 3 * cdiv(n_c, 256) * 256 / 16;
            const PsiStreamSplit s = psi_stream_split(SM, SC, 32 < SM ? 32 : SM);
            printf("split V %d n_c %d: nsn_m %d nsn_c %d spm %d spc %d SM %d SC %d\n", V, n_c, s.nsn_m, s.nsn_c, s.spm, s.spc, SM, SC);
        }
        return 0;
    }
    const int ncs[] = {1, 16, 64, 256, 257, 1024, 2048, 4096}, Vs[] = {1100, 10475}, kpads[] = {256, 512, 768, 8192, 16384};
    for (int V : Vs)
        for (int n_c : ncs)
            for (int B = 1; B <= 128; B++)
                for (int ov = 0; ov <= LIMIT; ov++)
                    if (check(B, V, n_c, ov)) return 1;
    printf("fit plan: %ld plans, %ld workgroups: every (slice, body) covered exactly once\n", plans, workgroups);
    for (int V : Vs)
        for (int n_c : ncs)
            for (int kpad : kpads)                               // 64, 32 (SMPL-X), 21, 2 slices and 1
                if (check_split(V, n_c, kpad)) return 1;
    printf("stream split: %ld splits, %ld steps: every step in exactly one slice, the longest slice minimal\n", splits, steps);
    return 0;
}
