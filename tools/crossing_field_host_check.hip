// Host rehearsal of csrc/crossing_field.hip: the statements of csrc/crossing_field_shared.h (cf_consts, cf_record, cf_eval, their reverse
// mode, cf_pair_role, cf_entry_value) run serially on the CPU in the kernels' order: per (pair, role) entry the forward and the six gradient
// rows; the entries sorted stably by their cell of pair_energy and added in that order in fp64; the gradient rows sorted stably by target
// and every run added in order.  No GPU needed:
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -ffp-contract=off tools/crossing_field_host_check.hip -o crossing_field_host_check
//   crossing_field_host_check BATCH.bin OUT.bin            (add -Xarch_host -fsanitize=address,undefined for a checked run)
//
// BATCH.bin: int32 B, V, F, n; float32 sigma; B*V*3 float32; F*3 int32; n*4 int32 (i, s, j, t) ascending, i <= j; B float32 (g).
// OUT.bin:   int32 n; n*6 float32 (psi); n*2 float32 (energy); n*36 float32 (rows); n*12 int64 (targets); B*V*3 float32 (G);
//            B*B float64 (pair_energy); B float32 (loss).
// It does not cover the kernels' gathers, the 16-byte pair read, the LDS staging of the pairs pass, nor the device's division and square
// root: those need the GPU tests.
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <numeric>
#include <vector>
#include "../psi-release_amd/csrc/crossing_field_shared.h"

template <typename T>
static bool read_all(FILE *f, std::vector<T> &v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

template <typename T>
static void write_all(FILE *f, const std::vector<T> &v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s BATCH.bin OUT.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t hdr[4];
    float sigma;
    if (fread(hdr, 4, 4, f) != 4 || fread(&sigma, 4, 1, f) != 1) return 2;
    const int B = hdr[0], V = hdr[1], F = hdr[2], n = hdr[3];
    if (B < 1 || V < 1 || F < 1 || n < 0 || !(sigma > 0.0f && sigma <= 0.5f)) { fprintf(stderr, "bad header\n"); return 3; }
    std::vector<float> verts((size_t)B * V * 3), g((size_t)B);
    std::vector<int32_t> faces((size_t)F * 3), pairs((size_t)n * 4);
    if (!read_all(f, verts) || !read_all(f, faces) || !read_all(f, pairs) || !read_all(f, g)) return 2;
    fclose(f);
    for (int32_t x : faces)
        if (x < 0 || x >= V) { fprintf(stderr, "face index %d outside [0, %d)\n", (int)x, V); return 3; }
    for (int k = 0; k < n; k++) {
        const int32_t *p = &pairs[(size_t)k * 4];
        if (p[0] < 0 || p[0] >= B || p[2] < p[0] || p[2] >= B || p[1] < 0 || p[1] >= F || p[3] < 0 || p[3] >= F) { fprintf(stderr, "pair %d\n", k); return 3; }
        if (k && !std::lexicographical_compare(p - 4, p, p, p + 4)) { fprintf(stderr, "pair %d is not above its predecessor\n", k); return 3; }
    }

    const CfConsts K = cf_consts(sigma);
    std::vector<float> psi((size_t)n * 6), energy((size_t)n * 2), rows((size_t)n * 36);
    std::vector<long long> targets((size_t)n * 12);
    for (long long e = 0; e < 2ll * n; e++) {
        const int32_t *p = &pairs[(size_t)(e >> 1) * 4];
        const int role = (int)(e & 1);
        const int bi = role ? p[2] : p[0], fi = role ? p[3] : p[1], br = role ? p[0] : p[2], fr = role ? p[1] : p[3];
        const int32_t *fa = &faces[(size_t)fi * 3], *fb = &faces[(size_t)fr * 3];
        const float *vi = &verts[(size_t)bi * V * 3], *vr = &verts[(size_t)br * V * 3];
        float check[3];
        energy[e] = cf_pair_role(cf_load(vi + (size_t)fa[0] * 3), cf_load(vi + (size_t)fa[1] * 3), cf_load(vi + (size_t)fa[2] * 3),
                                 cf_load(vr + (size_t)fb[0] * 3), cf_load(vr + (size_t)fb[1] * 3), cf_load(vr + (size_t)fb[2] * 3), K, 0.0f,
                                 &psi[(size_t)e * 3], nullptr);
        const float again = cf_pair_role(cf_load(vi + (size_t)fa[0] * 3), cf_load(vi + (size_t)fa[1] * 3), cf_load(vi + (size_t)fa[2] * 3),
                                         cf_load(vr + (size_t)fb[0] * 3), cf_load(vr + (size_t)fb[1] * 3), cf_load(vr + (size_t)fb[2] * 3), K,
                                         g[bi], check, &rows[(size_t)e * 18]);
        if (memcmp(check, &psi[(size_t)e * 3], 12) != 0 || memcmp(&again, &energy[e], 4) != 0) { fprintf(stderr, "entry %lld: the second run has other bits\n", e); return 4; }
        for (int m = 0; m < 3; m++) {
            targets[(size_t)e * 6 + m] = (long long)bi * V + fa[m];
            targets[(size_t)e * 6 + 3 + m] = (long long)br * V + fb[m];
        }
    }

    // the aggregates: the entries sorted stably by cell, a row of cells after the other, a cell closed when the column changes
    std::vector<double> pair_energy((size_t)B * B, 0.0);
    std::vector<float> loss((size_t)B, 0.0f);
    {
        std::vector<long long> cell((size_t)n * 2);
        for (long long e = 0; e < 2ll * n; e++) {
            const int32_t *p = &pairs[(size_t)(e >> 1) * 4];
            cell[e] = (e & 1) ? (long long)p[2] * B + p[0] : (long long)p[0] * B + p[2];
        }
        std::vector<size_t> order(cell.size());
        std::iota(order.begin(), order.end(), (size_t)0);
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return cell[a] < cell[b]; });
        size_t q = 0;
        for (int i = 0; i < B; i++) {
            double sum = 0.0, total = 0.0;
            int cur = -1;
            for (; q < order.size() && cell[order[q]] < (long long)(i + 1) * B; q++) {
                const long long e = (long long)order[q];
                const int32_t *p = &pairs[(size_t)(e >> 1) * 4];
                if (p[0] == p[2] && (e & 1)) continue;
                const int col = (int)(cell[e] - (long long)i * B);
                if (col != cur) {
                    if (cur >= 0) pair_energy[(size_t)i * B + cur] = sum, total += sum;
                    cur = col, sum = 0.0;
                }
                sum += cf_entry_value(p[0], p[2], (int)(e & 1), energy[e & ~1ll], energy[e | 1ll]);
            }
            if (cur >= 0) pair_energy[(size_t)i * B + cur] = sum, total += sum;
            loss[i] = (float)total;
        }
    }

    // the gradient: twelve rows per pair, sorted stably by target, every run added in order
    std::vector<float> G((size_t)B * V * 3, 0.0f);
    {
        std::vector<size_t> order(targets.size());
        std::iota(order.begin(), order.end(), (size_t)0);
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return targets[a] < targets[b]; });
        for (size_t q = 0; q < order.size();) {
            const long long tgt = targets[order[q]];
            float acc[3] = {0.0f, 0.0f, 0.0f};
            for (; q < order.size() && targets[order[q]] == tgt; q++)
                for (int a = 0; a < 3; a++) acc[a] = acc[a] + rows[order[q] * 3 + a];
            for (int a = 0; a < 3; a++) G[(size_t)tgt * 3 + a] = acc[a];
        }
    }

    printf("bodies %d vertices %d faces %d pairs %d sigma %g\n", B, V, F, n, (double)sigma);
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    const int32_t n32 = n;
    fwrite(&n32, 4, 1, f);
    write_all(f, psi), write_all(f, energy), write_all(f, rows), write_all(f, targets), write_all(f, G), write_all(f, pair_energy), write_all(f, loss);
    fclose(f);
    return 0;
}
