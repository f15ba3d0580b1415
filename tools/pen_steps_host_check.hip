// Host check of csrc/pen_steps.h: the vertex mask -> 16-column step decision of the blend backward (lbs_joint_device.h: blend_bwd_h_body),
// with the very functions the kernel calls, against a brute-force loop over the columns.  No GPU needed:
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -Xarch_host -fsanitize=address,undefined tools/pen_steps_host_check.hip -o pen_steps_host_check
//   pen_steps_host_check
//
// For every V in 1 .. 700 and V = 10475: random masks of several densities and the single-bit masks v in {0, 5, 63, 64, 255, 256, V - 1}
// (a vertex whose columns straddle two steps, two mask words, two slices; the partial last slice), every step of the padded row, read
// through the window of mask words a stream workgroup loads for its slice (several slice lengths; the window is a heap copy of exactly
// those words, so the sanitizer sees a read outside it).  Exit status 1 at the first difference.  It does not cover the kernel's loads,
// its OR over the bodies or its barrier: those need the GPU tests.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../psi-release_amd/csrc/pen_steps.h"

static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
static unsigned long long rng()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

static long checked = 0;

// brute force: any column 16 s .. 16 s + 15 whose vertex (column / 3) has its bit set; vertices past the mask are clear
static bool brute(const std::vector<unsigned long long> &mask, int s)
{
    for (int c = 16 * s; c < 16 * s + 16; c++) {
        const int v = c / 3;
        if (v < (int)mask.size() * 64 && (mask[v >> 6] >> (v & 63) & 1ull)) return true;
    }
    return false;
}

static int check_mask(int V, const std::vector<unsigned long long> &mask, const char *what)
{
    const int words = (int)mask.size(), steps = 3 * words * 64 / 16;
    const int spans[] = {steps, 76, 9, 1};
    for (int spm : spans) {
        if (spm > steps) continue;
        for (int s_begin = 0; s_begin < steps; s_begin += spm) {
            const int s_end = s_begin + spm < steps ? s_begin + spm : steps;
            int w0, nw;
            psi_pen_step_words(s_begin, s_end, w0, nw);
            if (nw > words - w0) nw = words - w0;                // (the kernel's clamp to the mask's row)
            if (nw < 0) nw = 0;
            unsigned long long *win = (unsigned long long *)malloc((size_t)(nw > 0 ? nw : 1) * 8);
            if (nw > 0) memcpy(win, mask.data() + w0, (size_t)nw * 8);
            for (int s = s_begin; s < s_end; s++) {
                const bool got = psi_pen_step_live(win, w0, nw, s), want = brute(mask, s);
                checked++;
                if (got != want) {
                    printf("V %d %s: step %d of slice [%d, %d) window [%d, +%d): got %d, brute force %d\n", V, what, s, s_begin, s_end, w0, nw, (int)got, (int)want);
                    free(win);
                    return 1;
                }
            }
            free(win);
        }
    }
    return 0;
}

static int check_V(int V)
{
    const int Vpad = (V + 255) / 256 * 256, words = Vpad / 64;
    std::vector<unsigned long long> mask(words);
    auto clear_padding = [&]() {
        for (int v = V; v < Vpad; v++) mask[v >> 6] &= ~(1ull << (v & 63));
    };
    // the first and last vertex of a step bracket its columns
    for (int s = 0; s < 3 * Vpad / 16; s++)
        if (psi_pen_step_first_vertex(s) != (16 * s) / 3 || psi_pen_step_last_vertex(s) != (16 * s + 15) / 3 ||
            psi_pen_step_last_vertex(s) - psi_pen_step_first_vertex(s) > 5) {
            printf("V %d: vertex range of step %d\n", V, s);
            return 1;
        }
    const int shifts[] = {0, 2, 5, 9};                           // density 1, 1/4, 1/32, 1/512 of the bits
    for (int sh : shifts) {
        for (auto &w : mask) {
            w = 0ull;
            for (int i = 0; i < 64; i++)
                if ((rng() & ((1ull << sh) - 1ull)) == 0ull) w |= 1ull << i;
        }
        clear_padding();
        if (check_mask(V, mask, "random mask")) return 1;
    }
    std::fill(mask.begin(), mask.end(), 0ull);
    if (check_mask(V, mask, "empty mask")) return 1;
    const int singles[] = {0, 5, 63, 64, 255, 256, V - 1};
    for (int v : singles) {
        if (v < 0 || v >= V) continue;
        std::fill(mask.begin(), mask.end(), 0ull);
        mask[v >> 6] = 1ull << (v & 63);
        if (check_mask(V, mask, "single bit")) return 1;
        // exactly the steps that hold one of the vertex's three columns
        int live = 0;
        for (int s = 0; s < 3 * Vpad / 16; s++) live += psi_pen_step_live(mask.data(), 0, words, s) ? 1 : 0;
        const int expect = (3 * v + 2) / 16 - (3 * v) / 16 + 1;
        if (live != expect) {
            printf("V %d single bit %d: %d live steps, expected %d\n", V, v, live, expect);
            return 1;
        }
    }
    return 0;
}

int main()
{
    for (int V = 1; V <= 700; V++)
        if (check_V(V)) return 1;
    if (check_V(10475)) return 1;
    printf("pen_steps: %ld step decisions equal brute force (V = 1 .. 700, 10475)\n", checked);
    return 0;
}
