// Host check of csrc/search_shape.h: the layout of the tree walk's stacks in the engine's kd_stack buffer (two slices per search workgroup)
// and the rule that decides between one and two slices.  No GPU needed:
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -Xarch_host -fsanitize=address,undefined tools/search_shape_host_check.hip -o search_shape_host_check
//   search_shape_host_check
//
// Layout: for a few (B, n, rows) a heap buffer of exactly psi_search_stack_bytes is written the way the search addresses it — the body's
// base plus the 32-bit offset of entry i of query jq, for both tables — every word exactly once (a write outside is the sanitizer's, a word
// written twice or never is counted).  Bound: psi_search_stack_fits refuses exactly the shapes whose body part reaches 2^32 bytes, and the
// largest offset of a shape it accepts does not wrap.  Rule: with the static LDS of the shipped instances (5608 / 7872 bytes) on a
// 163840-byte CU two slices are chosen up to rows = 37 and one from rows = 38 on, where the second pair's rows would cost the sixth workgroup;
// unknown sizes choose one.  Exit status 1 at the first failure.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../psi-release_amd/csrc/search_shape.h"

#define FAIL(...) do { printf(__VA_ARGS__); printf("\n"); return 1; } while (0)

static int layout(int B, int n, int rows)
{
    if (!psi_search_stack_fits(n, rows)) FAIL("B %d n %d rows %d refused", B, n, rows);
    const size_t bytes = psi_search_stack_bytes(B, n, rows);
    if (bytes != (size_t)B * n * rows * 8) FAIL("size of B %d n %d rows %d", B, n, rows);
    char *buf = (char *)malloc(bytes);
    memset(buf, 0, bytes);
    for (int b = 0; b < B; b++)
        for (int jq = 0; jq < n; jq++)
            for (int which = 0; which < 2; which++)
                for (int i = 0; i < rows; i++) {
                    int *w = (int *)(buf + psi_search_stack_body_base(b, n, rows) + psi_search_stack_entry(jq, rows, which, i));
                    *w += 1;
                }
    size_t bad = 0;
    for (size_t k = 0; k < bytes / 4; k++) bad += ((int *)buf)[k] != 1;
    free(buf);
    if (bad) FAIL("B %d n %d rows %d: %zu words not written exactly once", B, n, rows, bad);
    return 0;
}

int main()
{
    const int shapes[][3] = {{1, 1, 9}, {3, 64, 16}, {2, 130, 23}, {32, 2048, 37}, {5, 300, 72}};
    for (const auto &s : shapes)
        if (layout(s[0], s[1], s[2])) return 1;
    // the 32-bit bound: n * rows * 8 < 2^32
    const int rows = 72, n_ok = (int)((((size_t)1 << 32) - 1) / (8 * rows)), n_bad = n_ok + 1;
    if (!psi_search_stack_fits(n_ok, rows) || psi_search_stack_fits(n_bad, rows) || psi_search_stack_fits(0, rows) || psi_search_stack_fits(4, 0))
        FAIL("the bound is not n * rows * 8 < 2^32");
    if ((size_t)psi_search_stack_entry(n_ok - 1, rows, 1, rows - 1) != (size_t)(n_ok - 1) * 8 * rows + 4 * (size_t)(2 * rows - 1))
        FAIL("the largest offset of an accepted shape wraps");
    // residency: workgroups per CU and the choice
    const size_t cu = 163840, s1 = 5608, s2 = 7872;
    for (int r = 9; r <= 72; r++) {
        const size_t dyn = (size_t)64 * r * 8;
        const int w1 = psi_search_wgs_per_cu(cu, s1, dyn, 6), w2 = psi_search_wgs_per_cu(cu, s2, dyn, 6);
        if (w1 > 6 || w2 > w1 || (size_t)w1 * (s1 + dyn) > cu || (w1 < 6 && (size_t)(w1 + 1) * (s1 + dyn) <= cu)) FAIL("workgroups per CU at rows %d: %d %d", r, w1, w2);
        const int spw = psi_search_spw_for(cu, s1, s2, dyn, 6);
        if (spw != (w2 >= w1 ? 2 : 1)) FAIL("choice at rows %d", r);
        if ((r <= 37 && spw != 2) || (r == 38 && spw != 1)) FAIL("rows %d: %d slices (six per CU: one slice %d, two slices %d)", r, spw, w1, w2);
    }
    if (psi_search_spw_for(cu, 0, s2, 18944, 6) != 1 || psi_search_spw_for(cu, s1, 0, 18944, 6) != 1) FAIL("unknown static sizes must choose one slice");
    printf("search_shape: stack layouts written exactly once, the 32-bit bound holds, two slices up to rows = 37 on a 163840-byte CU\n");
    return 0;
}
