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
// grid is at most 512, one occupancy round.  Exit status 1 at the first failure.
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

int main()
{
    const int ncs[] = {1, 16, 64, 256, 257, 1024, 2048, 4096}, Vs[] = {1100, 10475};
    for (int V : Vs)
        for (int n_c : ncs)
            for (int B = 1; B <= 128; B++)
                for (int ov = 0; ov <= LIMIT; ov++)
                    if (check(B, V, n_c, ov)) return 1;
    printf("fit plan: %ld plans, %ld workgroups: every (slice, body) covered exactly once\n", plans, workgroups);
    return 0;
}
