// Host check of csrc/chain_plan.h: when the kinematic chain of the pose stage rides in blend_fwd's launch (the links role of
// blend_fwd_h_kernel), and which wave takes which body, with the very functions fit_decide (fit.hip) and the kernel (lbs.hip) call.
// No GPU needed:
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -Xarch_host -fsanitize=address,undefined tools/chain_plan_host_check.hip -o chain_plan_host_check
//   chain_plan_host_check
//
// For every B in 1 .. 130, device CU counts 256, 64 and 32, stream workgroup counts 246 (the SMPL-X-shaped model) and 8, the head cluster
// width the engine picks for B (8, 4, 2, 1) and width 1, and blend_fwd's own grid rows for B (1 up to 64 bodies, then ceil(B / 64)) as well
// as a forced second row:
//   * "off" whenever the head runs without clusters or the grid has more than one row;
//   * when "on": at most 8 links workgroups, at most CUs - stream workgroups of them, bodies_per_wave = ceil(B / 32), and every body is
//     the turn of exactly one (workgroup, wave, turn) — the coverage table is a heap array of exactly B entries, so a body outside it is a
//     sanitizer error — with no wave starting a body outside the batch that another wave does not own;
//   * when "off" for any other reason, that reason holds (the role would need more than 8 workgroups, or more than the free CUs).
// Exit status 1 at the first failure.
#include <stdio.h>
#include <stdlib.h>
#include "../psi-release_amd/csrc/chain_plan.h"

static long plans = 0, on = 0, turns = 0;

static int engine_hc(int B) { return B <= 32 ? 8 : B <= 64 ? 4 : B <= 128 ? 2 : 1; }      // fit_decide, one engine

static int check(int B, int hc, int n_stream, int grid_y, int cus)
{
#define FAIL(...) do { printf("B %d hc %d stream %d rows %d CUs %d: ", B, hc, n_stream, grid_y, cus); printf(__VA_ARGS__); printf("\n"); return 1; } while (0)
    const PsiChainPlan p = psi_chain_plan(B, hc, n_stream, grid_y, cus);
    plans++;
    const int bpw = (B + 31) / 32, need = (B + 4 * bpw - 1) / (4 * bpw);
    if (p.n_links_wg == 0) {
        if (hc > 1 && grid_y == 1 && need <= 8 && need <= cus - n_stream) FAIL("off without a reason (%d workgroups would do)", need);
        return 0;
    }
    on++;
    if (hc <= 1) FAIL("on without head clusters");
    if (grid_y != 1) FAIL("on with %d grid rows", grid_y);
    if (p.n_links_wg < 0 || p.n_links_wg > PSI_CHAIN_WG_MAX || p.n_links_wg > 8) FAIL("%d links workgroups", p.n_links_wg);
    if (p.n_links_wg > cus - n_stream) FAIL("%d links workgroups, %d free CUs", p.n_links_wg, cus - n_stream);
    if (p.bodies_per_wave != bpw) FAIL("%d bodies per wave", p.bodies_per_wave);
    int *cover = (int *)calloc((size_t)B, sizeof(int));
    int rc = 0;
    for (int g = 0; g < p.n_links_wg && !rc; g++)
        for (int w = 0; w < PSI_CHAIN_WAVES && !rc; w++) {
            const int b0 = psi_chain_first_body(p, g, w);
            if (b0 < 0) { printf("workgroup %d wave %d: first body %d\n", g, w, b0); rc = 1; break; }
            for (int b = b0; b < b0 + p.bodies_per_wave && b < B; b++) {        // the kernel's loop
                cover[b]++;
                turns++;
            }
        }
    for (int b = 0; b < B && !rc; b++)
        if (cover[b] != 1) { printf("body %d covered %d times\n", b, cover[b]); rc = 1; }
    free(cover);
    if (rc) FAIL("coverage");
    return 0;
#undef FAIL
}

int main()
{
    const int cus[3] = {256, 64, 32}, streams[2] = {246, 8};
    for (int B = 1; B <= 130; B++)
        for (int ci = 0; ci < 3; ci++)
            for (int si = 0; si < 2; si++) {
                const int rows = B > 32 ? (B + 63) / 64 : 1;
                const int hcs[2] = {engine_hc(B), 1}, gys[2] = {rows, rows + 1};
                for (int hi = 0; hi < 2; hi++)
                    for (int gi = 0; gi < 2; gi++) {
                        if (check(B, hcs[hi], streams[si], gys[gi], cus[ci])) return 1;
                        const PsiChainPlan p = psi_chain_plan(B, hcs[hi], streams[si], gys[gi], cus[ci]);
                        if ((hcs[hi] == 1 || gys[gi] > 1) && p.n_links_wg != 0) {
                            printf("B %d: on with hc %d, %d rows\n", B, hcs[hi], gys[gi]);
                            return 1;
                        }
                    }
            }
    // the shapes the engine's tests and the benchmark run: 246 stream workgroups on 256 CUs
    const int Bs[8] = {1, 3, 4, 5, 32, 33, 64, 65};
    for (int i = 0; i < 8; i++) {
        const int B = Bs[i];
        const PsiChainPlan p = psi_chain_plan(B, engine_hc(B), 246, B > 32 ? (B + 63) / 64 : 1, 256);
        printf("plan B %d: links workgroups %d, bodies per wave %d\n", B, p.n_links_wg, p.bodies_per_wave);
    }
    printf("%ld plans, %ld on, %ld turns: every body covered exactly once, off without clusters and with more than one grid row\n", plans, on, turns);
    return 0;
}
